"""Child process of tests/test_draft_gpu.py: draft mode on the tolerance library (the pytest process holds the exact test library).  At
stop level 1 the levels from 1 up are whatever the tolerance library computes, and level 0 must be the oracle composition of that level-1
flow, bit for bit, in both directions.  Prints the library's version first and "PART OK" last."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))


def main():
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    from eppm_amd import synth
    from test_draft_cpu import oracle_jbu
    a, b = synth.bundled_pair()
    a, b = a[100:257, 100:311].copy(), b[100:257, 100:311].copy()
    full = eppm_amd.EPPM()
    full.init(a, b, 157, 211)
    full.compute_flow_bidirectional()
    e = eppm_amd.EPPM()
    e.init(a, b, 157, 211)
    e.set_stop_level(1)
    u, v, bu, bv, _, _ = e.compute_flow_bidirectional()
    for name, guide in (("flow", "img1"), ("flow_bwd", "img2")):
        for l in (2, 1):
            assert np.array_equal(e.plane(name, l).view(np.uint32), full.plane(name, l).view(np.uint32)), f"{name} level {l} != the full path's"
        want = oracle_jbu(e.plane(name, 1), e.plane(guide, 0))
        got = e.plane(name, 0)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{name} level 0: {bad} words differ from the oracle composition")
        assert bad == 0
    f0 = e.plane("flow", 0)
    assert np.array_equal(u.view(np.uint32), np.ascontiguousarray(f0["x"]).view(np.uint32))
    assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(f0["y"]).view(np.uint32))
    e.close(); full.close()
    print("PART OK")


if __name__ == "__main__":
    main()
