"""Child process of tests/test_tfilter_gpu.py, and the home of what both share: device_step() runs one case of tfilter_cases() through
set_state + eppm_tfilter_step_frames + get_state / get on a context-less filter.  As a program it selects the tolerance library (the
pytest process holds the exact test library), runs every case twice and expects the kernel to equal the numpy restatement bit for bit:
the filter has no EPPM_TOL branch.  Prints the library's version first and "PART OK" last."""
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
    """[(state, bytes)] of `runs` independent runs of case c on the device"""
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = c["h"], c["w"]
    pad = c.get("pad", 0)
    planes = [to_device(rgba(c["img1"], pad=pad)), to_device(rgba(c["img2"], pad=pad)), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
              to_device(c["occ"])]
    flt = eppm_amd.TemporalFilter(None, c["thresh"], c["n_max"], size=(h, w))
    out = []
    try:
        for _ in range(runs):
            if c["state"] == "empty":
                flt.reset(0)
            else:
                flt.set_state(0, c["acc"])
            flt.step_frames(0, planes[0].value, planes[1].value, (w + pad) * 4, planes[2].value, planes[3].value, c["cut"])
            out.append((flt.state(0), flt.frame(0)))
    finally:
        flt.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def mismatches(cases):
    bad = []
    for c in cases:
        res = device_step(c)
        for k, (acc, rgb) in enumerate(res):
            if not np.array_equal(acc.view(np.uint32), c["want_acc"].view(np.uint32)) or not np.array_equal(rgb, c["want_rgb"]):
                words = int((acc.view(np.uint32) != c["want_acc"].view(np.uint32)).sum())
                bad.append((c["name"], k, words, int((rgb != c["want_rgb"]).sum())))
    return bad


def main():
    from test_tfilter_cpu import tfilter_cases, tfilter_limit_cases          # (imports conftest, which selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    cases = tfilter_limit_cases() if sys.argv[1:2] == ["limit"] else tfilter_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
