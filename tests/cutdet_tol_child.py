"""Child process of tests/test_cutdet_gpu.py, and the home of what both share: device_records() runs one case of cutdet_cases() through
eppm_cutdet_step_frames + eppm_cutdet_get / eppm_cutdet_cuts on a context-less detector.  As a program it selects the tolerance library (the
pytest process holds the exact test library), runs every case twice and expects the kernels to equal the numpy restatement in every integer:
the detector has no EPPM_TOL branch.  Prints the library's version first and "PART OK" last."""
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


def rgba(img, pad=8, alpha=0x5a):
    """the image as RGBA rows of (w + pad) words: the alpha byte and the padding of an input frame are ignored"""
    h, w, _ = img.shape
    out = np.full((h, w + pad, 4), alpha, np.uint8)
    out[:, :w, :3] = img
    return out


def device_records(c, runs=2, slots=3):
    """the records of `runs` independent runs of case c on the device, each in another slot of one detector; the other slots stay empty"""
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = c["h"], c["w"]
    pad = 8
    planes = [to_device(rgba(c["img1"], pad)), to_device(rgba(c["img2"], pad)), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
              to_device(c["occ1"]), to_device(c["occ2"])]
    det = eppm_amd.CutDetector(None, c["lost_permille"], c["residual_max"], size=(h, w), slots=slots)
    out = []
    try:
        for k in range(runs):
            slot = (2 * k) % slots
            det.step_frames(slot, planes[0].value, planes[1].value, (w + pad) * 4, *[p.value for p in planes[2:]])
            rec = det.stats(slot)
            rec["cuts"] = det.cuts(slots)
            rec["slot"] = slot
            out.append(rec)
    finally:
        det.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def mismatches(cases):
    from test_cutdet_cpu import differences
    bad = []
    for c in cases:
        stepped = set()
        for k, got in enumerate(device_records(c)):
            stepped.add(got["slot"])
            d = differences(c["want"], got)
            # the verdicts of all slots in one copy: the stepped slots carry the verdict, a slot without a step reports none
            if got["cuts"] != [bool(c["want"]["cut"]) and s in stepped for s in range(len(got["cuts"]))]:
                d.append(("cuts", got["cuts"], c["want"]["cut"]))
            if d:
                bad.append((c["name"], k, d))
    return bad


def main():
    import eppm_amd
    eppm_amd.select_library("tol")          # before anything loads a library
    from test_cutdet_cpu import cutdet_cases, cutdet_limit_cases
    print(eppm_amd.lib().eppm_version().decode())
    cases = cutdet_limit_cases() if sys.argv[1:2] == ["limit"] else cutdet_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
