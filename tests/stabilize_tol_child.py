"""Child process of tests/test_stabilize_gpu.py, and the home of what both share: device_step() runs one case of stab_cases() through
reset / set_path + eppm_stab_step_frames + get_model / get_path / get_mask / get on a context-less stabiliser.  As a program it selects the
tolerance library (the pytest process holds the exact test library), runs every case twice and expects the kernels to equal the numpy
restatement bit for bit: the stabiliser has no EPPM_TOL branch.  Prints the library's version first and "PART OK" last."""
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


def device_step(c, runs=2):
    """the results of `runs` independent runs of case c on the device, as test_stabilize_cpu.differences() reads them"""
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = c["h"], c["w"]
    pad = c.get("pad", 0)
    planes = [to_device(rgba(c["img2"], pad=pad)), to_device(np.stack([c["u"], c["v"]], -1).astype(np.float32)), to_device(c["occ"])]
    stab = eppm_amd.Stabilizer(None, c["tau"], c["iters"], c["smooth"], size=(h, w))
    out = []
    try:
        for _ in range(runs):
            if c["path"] is None:
                stab.reset(0)
            else:
                stab.set_path(0, *c["path"])
            stab.step_frames(0, planes[0].value, (w + pad) * 4, planes[1].value, planes[2].value, c["cut"])
            cc, ss, counts = stab.path(0, counts=True)
            out.append(dict(model=stab.model(0), mask=stab.mask(0), C=cc, S=ss, counts=counts, rgb=stab.frame(0)))
    finally:
        stab.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def mismatches(cases):
    from test_stabilize_cpu import differences
    bad = []
    for c in cases:
        for k, got in enumerate(device_step(c)):
            d = differences(c, got)
            if d:
                bad.append((c["name"], k, d))
    return bad


def main():
    import eppm_amd
    eppm_amd.select_library("tol")          # before anything loads a library
    from test_stabilize_cpu import stab_cases, stab_limit_cases
    print(eppm_amd.lib().eppm_version().decode())
    cases = stab_limit_cases() if sys.argv[1:2] == ["limit"] else stab_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
