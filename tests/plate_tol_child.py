"""Child process of tests/test_plate_gpu.py, and the home of what both share: device_case() runs one case of plate_cases() through
set_state (or reset) + eppm_plate_step_frames + get_state + get_path + eppm_plate_render_frames + get, twice in a row on one slot of a
context-less plate.  As a program it selects the tolerance library (the pytest process holds the exact test library), runs every case and
expects the kernels to equal the numpy restatement in every bit: the plate has no EPPM_TOL branch.  Prints the library's version first
and "PART OK" last."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))


def to_device(arr=None, nbytes=None):
    from eppm_amd._lib import check, lib
    p = C.c_void_p()
    n = int(arr.nbytes) if arr is not None else int(nbytes)
    check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(max(n, 1))), "malloc")
    if arr is not None:
        arr = np.ascontiguousarray(arr)
        check(lib().eppm_memcpy_h2d(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
    return p


def from_device(p, shape, dtype):
    from eppm_amd._lib import check, lib
    out = np.empty(shape, dtype)
    check(lib().eppm_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes)), "d2h")
    return out


def rgba_of(rgb, pad=0):
    """the image as RGBA rows of (w + pad) words"""
    h, w, _ = rgb.shape
    out = np.zeros((h, w + pad, 4), np.uint8)
    out[:, :w, :3] = rgb
    return out


def case_planes(c):
    """the device planes of a case: [image a, image b, mask, render output (RGBA words), fill bytes]"""
    pad = c.get("pad", 0)                      # pixels beyond every row of the images and of the render's output: pitches larger than 4 * w
    px = c["h"] * c["w"]
    return [to_device(rgba_of(c["img"], pad)), to_device(rgba_of(c["img_b"], pad)), to_device(c["mask"]), to_device(nbytes=c["h"] * (c["w"] + pad) * 4),
            to_device(nbytes=px)]


def free_planes(planes):
    from eppm_amd._lib import lib
    for p in planes:
        lib().eppm_free_device(p)


def case_params(c):
    return dict(margin_x=c["mx"], margin_y=c["my"], grow=c["grow"], accept_invalid=int(c["accept"]), thresh=c["thresh"], n_max=c["n_max"],
                min_count=c["min_count"])


def load_case(pl, slot, c):
    pl.reset(slot)
    if c["prior"] is not None:
        pl.set_state(slot, c["prior"])


def step_case(pl, slot, c, planes, k):
    """step k (0: image a with the case's path, 1: image b with the slot's own, which is that path), then the step's render"""
    h, w = c["h"], c["w"]
    pitch = (w + c.get("pad", 0)) * 4
    pl.step_frames(slot, planes[k].value, pitch, planes[2].value, c["path"] if k == 0 else None)
    pl.render_frames(slot, planes[k].value, pitch, planes[2].value, None if k else c["path"], planes[3].value, pitch, planes[4].value)
    out = from_device(planes[3], (h, pitch // 4, 4), np.uint8)[:, :w]
    assert (out[..., 3] == 255).all()
    return np.ascontiguousarray(out[..., :3]), from_device(planes[4], (h, w), np.uint8)


def read_slot(pl, slot):
    """(state, path, canvas image, coverage) of a slot"""
    return pl.state(slot), pl.path(slot), pl.plate(slot), pl.coverage(slot)


def device_case(c, pl=None, slot=0, planes=None):
    """what the two steps of case c leave in a slot: [(state, path, plate, coverage, (render, fill))] per step"""
    import eppm_amd
    own_planes, own_plate = planes is None, pl is None
    planes = case_planes(c) if own_planes else planes
    pl = eppm_amd.BackgroundPlate(None, size=(c["h"], c["w"]), **case_params(c)) if own_plate else pl
    out = []
    try:
        load_case(pl, slot, c)
        for k in (0, 1):
            r = step_case(pl, slot, c, planes, k)
            out.append(read_slot(pl, slot) + (r,))
    finally:
        if own_plate:
            pl.close()
        if own_planes:
            free_planes(planes)
    return out


def device_differences(c, res):
    from test_plate_cpu import expected, same_bits
    want, bad = expected(c), []
    for k, (state, path, plate, cov, (out, fill)) in enumerate(res):
        if not same_bits(state, want["states"][k]):
            bad.append(f"state {k + 1}")
        if not np.array_equal(np.asarray(path).view(np.uint64), np.asarray(c["path"], np.float64).view(np.uint64)):
            bad.append(f"path {k + 1}")
        if not same_bits(plate, want["words"][k]) or not same_bits(cov, want["coverage"][k]):
            bad.append(f"get {k + 1}")
        if not same_bits(out, want["renders"][k][0]) or not same_bits(fill, want["renders"][k][1]):
            bad.append(f"render {k + 1}")
    return bad


def mismatches(cases):
    bad = []
    for c in cases:
        d = device_differences(c, device_case(c))
        if d:
            bad.append((c["name"], d))
    return bad


def main():
    from test_plate_cpu import plate_cases, plate_limit_cases          # (imports conftest, which selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    if sys.argv[1:2] == ["limit"]:          # three sizes from the one given
        cases = [c for k in range(3) for c in plate_limit_cases(int(sys.argv[2]) + k)]
    else:
        cases = plate_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:3]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
