"""Where the pixels of every correspondence-map step go with the engine's own flow: a 256x192 noisy moving clip
(tests/test_tfilter_cpu.py: moving_clip, sigma 5) through a streaming context with a map attached; the restatement of
tests/test_cmap_cpu.py, fed with the context's backward flow and occ2, gives the outcome of every pixel (and must equal the device's map
bit for bit), and the same step from the same previous map with the true flow and the analytic mask stands beside it.

    python tools/cmap_losses.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    import test_cmap_cpu as T          # (imports conftest, which selects the test library: overridden below, before anything is loaded)
    from test_tfilter_cpu import moving_clip
    import eppm_amd
    eppm_amd.select_library("")
    h, w = 192, 256
    _, noisy, flows, masks = moving_clip(h, w, 5, seed=61)
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_temporal(True)
    cm = eppm_amd.CorrespondenceMap(e)
    M = T.np_seed(h, w)
    pct = lambda m: 100 * m.mean()          # noqa: E731
    for k in range(1, 5):
        if k == 1:
            e.set_data(noisy[0], noisy[1])
        else:
            e.push_frame(noisy[k])
        _, _, bu, bv, _, o2 = e.compute_flow_bidirectional()
        cm.step()
        new, end, _ = T.np_step(M, noisy[0], noisy[k], bu, bv, o2, 90.0, 2.0, 1, False)
        assert np.array_equal(new.view(np.uint32), cm.map(0).view(np.uint32))
        print(f"step {k}: lost {pct(end >= T.LOST23):.2f} % (steps 2-3 {pct(end == T.LOST23):.2f}, nearest tap lost {pct(end == T.LOSTN):.2f}, "
              f"left the frame {pct(end == T.LOST6):.2f}, colour check {pct(end == T.LOSTC):.2f}); kept: smooth {pct(end == T.SMOOTH):.2f}, "
              f"tear {pct(end == T.TEAR):.2f}; occ2 != 0: {pct(o2 != 0):.2f} %")
        # the same step on the true flows and the analytic mask, from the same previous map
        _, tend, _ = T.np_step(M, noisy[0], noisy[k], flows[k - 1][0], flows[k - 1][1], masks[k - 1], 90.0, 2.0, 1, False)
        print(f"        true flow from the same map: lost {pct(tend >= T.LOST23):.2f} %, colour check {pct(tend == T.LOSTC):.2f} %")
        M = new
    cm.close()
    e.close()


if __name__ == "__main__":
    main()
