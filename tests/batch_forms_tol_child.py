"""Child process of tests/test_batch_forms_gpu.py: the batch sizes at which THIS library's launchers change their kernel (the tolerance
library with the test hooks: its own probe answers), radius 9, through one context of 512 pairs of 83x61.  DESIGN.md section 9.2: a batch
is the same arithmetic per pair, so every slot must equal the library's own single-pair context on the same pair, bit for bit -- forward
flow at every size, backward flow and both occlusion masks too.  Every batch is seen to take the forms the probe answers (launch log).
Prints the library's version first and "PART OK" last."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))


def main():
    import eppm_amd
    import test_batch_forms_cpu as T               # (its imports select the exact test library: overridden below, before anything is loaded)
    from test_temporal_cpu import make_clip
    eppm_amd.select_library("tol_test")
    print(eppm_amd.lib().eppm_version().decode())
    from eppm_amd._lib import launch_log
    R, nclips = 9, 13
    clips = [make_clip(T.H, T.W, 500 + s, n=3, max_flow=4.0)[0] for s in range(nclips)]
    want = []
    for c in clips:
        e = eppm_amd.EPPM()
        e.init(c[0], c[1], T.H, T.W)
        want.append([x.tobytes() for x in e.compute_flow_bidirectional()])
        e.close()
    assert len({w[0] for w in want}) == nclips
    sizes = T.change_sizes(R)
    print("change-point sizes of this library:", sizes)
    assert sizes and max(sizes) <= T.CAPACITY and len(sizes) >= 8
    b = eppm_amd.EPPMBatch(T.H, T.W, T.CAPACITY)
    for n in sizes:
        who = [int(p) % nclips for p in np.random.default_rng(7000 + n).permutation(n)]
        b.set_data([(clips[s][0], clips[s][1]) for s in who])
        with launch_log() as log:
            res = b.compute_flow_bidirectional()
        T.check_reached(log.entries(), R, n)
        bad = [(k, j) for k in range(n) for j in range(6) if res[k][j].tobytes() != want[who[k]][j]]
        print(f"n = {n}: {len(bad)} (slot, output) pairs differ from the single-pair context", bad[:4])
        assert not bad
    b.close()
    # give the 512-pair slab back before the process ends: what a dead process held returns to the device only some time after its exit,
    # and the tests that follow in the parent process count free device bytes
    eppm_amd.lib().eppm_release_cached_memory()
    eppm_amd.lib().eppm_device_synchronize()
    print("PART OK")


if __name__ == "__main__":
    main()
