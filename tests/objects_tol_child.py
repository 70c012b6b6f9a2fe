"""Child process of tests/test_objects_gpu.py, and the home of what both share: device_case() runs one case of objects_cases() through
set_state (or reset) + eppm_objects_step_frames + get + get_labels + get_state on a context-less detector.  As a program it selects the
tolerance library (the pytest process holds the exact test library), runs every case twice and expects the kernels to equal the numpy
restatement in every number: the detector has no EPPM_TOL branch.  With the argument "large K" it runs objects_large_cases(K) instead.
Prints the library's version first and "PART OK" last."""
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


def case_planes(c):
    """the device planes of a case: [mask, forward flow, backward flow or None, occ2 or None]"""
    planes = [to_device(c["mask"]), to_device(np.stack([c["u"], c["v"]], -1).astype(np.float32))]
    if c["bu"] is None:
        return planes + [None, None]
    return planes + [to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)), to_device(c["occ2"])]


def free_planes(planes):
    from eppm_amd._lib import lib
    for p in planes:
        if p is not None:
            lib().eppm_free_device(p)


def load_case(det, slot, c):
    if c["prev"] == "empty":
        det.reset(slot)
    else:
        det.set_state(slot, c["carried"], c["prev_id"], c["prev_age"], c["next_id"])


def step_case(det, slot, c, planes):
    det.step_frames(slot, planes[0].value, planes[1].value, None if planes[2] is None else planes[2].value,
                    None if planes[3] is None else planes[3].value, c["cut"])


def read_slot(det, slot):
    """(labels, records, counts, carried, prev_id, prev_age) of a slot; a set error word makes every one of these calls fail"""
    car, pid, page, nxt = det.state(slot)
    counts = det.counts(slot)
    assert counts["next_id"] == nxt
    return det.labels(slot), det.objects(slot), counts, car, pid, page


def device_case(c, runs=2):
    """what `runs` runs of case c on one detector leave in its slot"""
    import eppm_amd
    planes = case_planes(c)
    det = eppm_amd.ObjectDetector(None, size=(c["h"], c["w"]), connectivity=c["conn"], min_area=c["min_area"], max_objects=c["max_objects"],
                                  min_overlap=c["min_overlap"])
    out = []
    try:
        for _ in range(runs):
            load_case(det, 0, c)
            step_case(det, 0, c, planes)
            out.append(read_slot(det, 0))
    finally:
        det.close()
        free_planes(planes)
    return out


def mismatches(cases):
    from test_objects_cpu import differences
    bad = []
    for c in cases:
        for k, res in enumerate(device_case(c)):
            d = differences(c, *res)
            if d:
                bad.append((c["name"], k, d))
    return bad


def main():
    from test_objects_cpu import objects_cases, objects_large_cases          # (imports conftest, which selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    cases = objects_large_cases(int(sys.argv[2])) if sys.argv[1:2] == ["large"] else objects_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:3]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
