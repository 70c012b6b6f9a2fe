"""Child process of tests/test_cmap_gpu.py, and the home of what both share: device_step() runs one case of cmap_cases() through
set_state + eppm_cmap_step_frames + get_state + set_layer + render on a context-less map.  As a program it selects the tolerance library
(the pytest process holds the exact test library), runs every case twice and expects the kernels to equal the numpy restatement bit for
bit: the map has no EPPM_TOL branch.  Prints the library's version first and "PART OK" last."""
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
    """[(map, bytes)] of `runs` independent runs of case c on the device"""
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = c["h"], c["w"]
    pad = c.get("pad", 0)
    planes = [to_device(rgba(c["img1"], pad=pad)), to_device(rgba(c["img2"], pad=pad)), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
              to_device(c["occ"])]
    cm = eppm_amd.CorrespondenceMap(None, size=(h, w), thresh=c["thresh"], tear=c["tear"], use_occ=c["use_occ"])
    out = []
    try:
        for _ in range(runs):
            if c["prev"] == "empty":
                cm.reset(0)
            else:
                cm.set_state(0, c["map"], c["anchor"])
            cm.set_layer(None, 0)
            cm.step_frames(0, planes[0].value, planes[1].value, (w + pad) * 4, planes[2].value, planes[3].value, c["cut"])
            got = cm.map(0)
            cm.set_layer(c["layer"], 0)
            out.append((got, cm.render(0), cm.age(0)))
    finally:
        cm.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def mismatches(cases):
    bad = []
    for c in cases:
        res = device_step(c)
        age = 0 if c["cut"] else 1
        for k, (m, rgb, a) in enumerate(res):
            if not np.array_equal(m.view(np.uint32), c["want_map"].view(np.uint32)) or not np.array_equal(rgb, c["want_rgb"]) or a != age:
                words = int((m.view(np.uint32) != c["want_map"].view(np.uint32)).sum())
                bad.append((c["name"], k, words, int((rgb != c["want_rgb"]).sum()), a))
    return bad


def main():
    from test_cmap_cpu import cmap_cases, cmap_limit_cases          # (imports conftest, which selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    cases = cmap_limit_cases() if sys.argv[1:2] == ["limit"] else cmap_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
