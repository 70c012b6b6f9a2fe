"""Cost of one deinterlacer step next to the bidirectional call it follows and to the temporal filter's step: the
`deint_step` stage time from eppm_stage_times for a single pair and for a batch of slots stepped by the same launch, on pairs of field
frames (image 1 the top field of a frame, image 2 the bottom field of its successor, both bobbed), with the bytes the lanes request per
pixel -- a real row: frame word 4, output word 4, mask byte 1; a missing row: two frame words 8, backward vector 8, mask byte 1, four
reference taps 16, output word 4, mask byte 1; half the rows each: 23.5 B per pixel on average -- as a share of 8 TB/s.  One library per
process:

    python tools/deint_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--thresh N]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--thresh", type=int, default=24)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import io, synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    requested = {"deint_step": (9 + 38) / 2, "tfilter_step": 4 + 8 + 1 + 64 + 16 + 4}
    pairs = []
    for k in range(a.batch):
        f0, f1 = synth.make_pair_cached(h, w, seed=1234 + k)[:2]
        pairs.append((io.deint_bob_host(f0[0::2], h, 0), io.deint_bob_host(f1[1::2], h, 1)))
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "thresh": a.thresh,
           "requested_bytes_per_pixel": requested}

    def stages(ctx, step, names, before=None):
        """the median stage times (ms) of `names` over a.steps calls of step(); before(): synchronous work ahead of every call"""
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(a.steps):
            if before:
                before()
            step()
        ctx.synchronize()
        got = ctx.stage_times()
        ctx.enable_stage_timing(False)
        ms = {}
        for n in names:
            t = sorted(v for name, v in got if name == n)
            ms[n] = t[len(t) // 2]
        return ms

    def measure(ctx, nslots, tag):
        import time
        di = eppm_amd.Deinterlacer(ctx, thresh=a.thresh)
        tf = eppm_amd.TemporalFilter(ctx)
        ctx.compute_flow_bidirectional_device()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            ctx.compute_flow_bidirectional_device()
            ctx.synchronize()
        r = {"bidir_dev_ms_per_pair": (time.perf_counter() - t0) * 1e3 / 3 / nslots}
        ms = stages(ctx, lambda: di.step(parity=[1] * nslots), ("deint_step",), before=di.reset)      # every timed step starts from image 1
        st = [di.stats(k) for k in range(nslots)]
        r["step_ms_per_pair"] = ms["deint_step"] / nslots
        r["share_temporal"] = float(np.mean([s["temporal"] / max(s["temporal"] + s["spatial"], 1) for s in st]))
        r["share_of_8TBs"] = requested["deint_step"] * h * w * nslots / (ms["deint_step"] * 1e-3) / 8e12
        r["step_share_of_bidir_dev"] = r["step_ms_per_pair"] / r["bidir_dev_ms_per_pair"]
        tf.step()
        r["tfilter_step_ms_per_pair"] = stages(ctx, tf.step, ("tfilter_step",))["tfilter_step"] / nslots
        di.close()
        tf.close()
        out[tag] = r

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    measure(e, 1, "single")
    e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    measure(b, a.batch, "batch")
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
