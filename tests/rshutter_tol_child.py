"""Child process of tests/test_rshutter_gpu.py, and the home of what both share: frames_kernel() runs eppm_rolling_shutter_frames (the
kernels alone) on caller planes.  As a program it selects the tolerance library (the pytest process holds the exact test library), runs
every case of test_rshutter_cpu.rs_cases() twice and expects the kernels to equal the host form byte for byte: rolling-shutter
correction has no EPPM_TOL branch.  Prints the library's version first and "PART OK" last."""
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
    check(lib().eppm_malloc_device(C.byref(p), max(arr.nbytes, 1)), "malloc")
    check(lib().eppm_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "h2d")
    return p


def frames_kernel(img, u, v, params, runs=2, pad=5):
    """`runs` outputs of eppm_rolling_shutter_frames as (h, w, 3) RGB (alpha checked 255).  params: (readout, anchor, iters, axis, frame).
    The input rows are w + pad words apart, and its alpha bytes and padding hold garbage; the output rows are w + 3 words apart in a
    poisoned plane, and the padding must stay as it was."""
    import eppm_amd
    from eppm_amd._lib import check, lib
    L = lib()
    h, w = u.shape
    rng = np.random.default_rng(h * 1000 + w)
    src = rng.integers(0, 256, (h, w + pad, 4), dtype=np.uint8)
    src[:, :w, :3] = img
    opad = 3
    bufs = [to_device(src), to_device(np.stack([u, v], -1).astype(np.float32))]
    p = eppm_amd.RSParams(readout=params[0], anchor=params[1], iters=params[2], axis=params[3])
    out = []
    try:
        for k in range(runs):
            dst = np.full((h, w + opad, 4), 0xa5 + k, np.uint8)
            d = to_device(dst)
            bufs.append(d)
            check(L.eppm_rolling_shutter_frames(d, (w + opad) * 4, bufs[0], (w + pad) * 4, bufs[1], h, w, int(params[4]), C.byref(p)),
                  "eppm_rolling_shutter_frames")
            r = np.empty_like(dst)
            check(L.eppm_memcpy_d2h(r.ctypes.data, d, r.nbytes), "d2h")
            assert (r[:, :w, 3] == 255).all(), "alpha"
            assert (r[:, w:] == 0xa5 + k).all(), "the output's padding was written"
            out.append(r[:, :w, :3].copy())
    finally:
        for b in bufs:
            L.eppm_free_device(b)
    return out


def mismatches(cases):
    """[(case, run, differing pixels)] of the kernels against the host form (kept as c["host"]); the two runs of a case must also agree"""
    from test_rshutter_cpu import host_case
    bad = []
    for c in cases:
        if "host" not in c:
            c["host"] = host_case(c)
        got = frames_kernel(c["img"], c["u"], c["v"], c["params"])
        for k, g in enumerate(got):
            n = int((g != c["host"]).any(axis=2).sum())
            if n:
                bad.append((c["name"], k, n))
        if not np.array_equal(got[0], got[1]):
            bad.append((c["name"], "runs differ", int((got[0] != got[1]).any(axis=2).sum())))
    return bad


def main():
    import eppm_amd
    eppm_amd.select_library("tol")          # before anything loads a library
    from test_rshutter_cpu import LIMIT_SIZES, SIZES, rs_cases
    print(eppm_amd.lib().eppm_version().decode())
    cs = rs_cases(LIMIT_SIZES if sys.argv[1:2] == ["limit"] else SIZES)
    bad = mismatches(cs)
    changed = sum(int((c["host"] != c["img"]).any()) for c in cs)
    print(f"{len(cs)} cases, {changed} change the frame, {len(bad)} differ from the host form: {bad[:5]}")
    assert not bad and 2 * changed >= len(cs)
    print("PART OK")


if __name__ == "__main__":
    main()
