"""Child process of tests/test_deflicker_gpu.py, and the home of what both share: device_steps() runs one case of deflicker_cases() through
set_state + eppm_deflicker_step_frames + the getters on a context-less object, twice.  As a program it selects the tolerance library (the
pytest process holds the exact test library), expects the kernels to equal the numpy restatement bit for bit on every case -- flicker
removal has no EPPM_TOL branch --, and runs deflicker_sequence on the flickering clip with that library's own flows: every frame 1..5 must
be closer to the flicker-free clip than the input is.  Prints the library's version first and "PART OK" last."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))


def to_device(arr):
    from eppm_amd._lib import check, lib
    arr = np.ascontiguousarray(arr)
    p = C.c_void_p()
    check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(max(arr.nbytes, 1))), "malloc")
    check(lib().eppm_memcpy_h2d(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
    return p


def rgba(img, alpha=0x5a, pad=0):
    h, w, _ = img.shape
    out = np.full((h, w + pad, 4), alpha, np.uint8)     # the alpha byte of an input frame is ignored; pad: pixels beyond every row (the pitch)
    out[:, :w, :3] = img
    return out


def case_planes(c):
    """the caller planes of a case on the device: image 1, image 2, the backward flow, occ2"""
    pad = c.get("pad", 0)
    return [to_device(rgba(c["img1"], pad=pad)), to_device(rgba(c["cur"], pad=pad)), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
            to_device(c["occ2"])]


def read(dk, slot):
    field, valid = dk.field(slot)
    return dk.frame(slot), field, valid, dk.stats(slot)


def device_steps(c, steps=2, slot=0, slots=1):
    """[(rgb, field, valid, stats)] after each of `steps` consecutive steps of case c on the device: the first from the case's reference
    (or from an empty slot), every later one from the output before it"""
    import eppm_amd
    from eppm_amd._lib import lib
    planes = case_planes(c)
    dk = eppm_amd.Deflicker(None, size=(c["h"], c["w"]), slots=slots, **c["params"])
    out = []
    try:
        if not c["empty"]:
            dk.set_state(slot, c["ref"])
        for _ in range(steps):
            dk.step_frames(slot, planes[0].value, planes[1].value, (c["w"] + c.get("pad", 0)) * 4, planes[2].value, planes[3].value, c["cut"])
            out.append(read(dk, slot))
    finally:
        dk.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def mismatches(cases):
    from test_deflicker_cpu import np_case, same
    bad = []
    for c in cases:
        first = np_case(c)
        want = [first, np_case(c, ref=first[0])]
        for k, got in enumerate(device_steps(c)):
            if not same(got, want[k]):
                bad.append((c["name"], k, int((got[0] != want[k][0]).sum()), int((got[1].view(np.uint32) != want[k][1].view(np.uint32)).sum()),
                            got[3], want[k][3]))
    return bad


def main():
    from test_deflicker_cpu import deflicker_cases, deflicker_limit_cases, flicker_clip, psnr        # (imports conftest, which selects the test library: overridden below)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    limit = sys.argv[1:2] == ["limit"]
    cases = [c for c in deflicker_limit_cases() if (c["w"] > c["h"]) == (sys.argv[2] == "0")] if limit else deflicker_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    if limit:
        print("PART OK")
        return
    flick, plain, _ = flicker_clip()
    out = eppm_amd.deflicker_sequence(flick)
    before = [psnr(flick[k], plain[k]) for k in range(1, 6)]
    after = [psnr(out[k], plain[k]) for k in range(1, 6)]
    print("tolerance library, its own flows: before", [round(float(x), 2) for x in before], "after", [round(float(x), 2) for x in after])
    assert np.array_equal(out[0], flick[0]) and all(a > b for a, b in zip(after, before))
    print("PART OK")


if __name__ == "__main__":
    main()
