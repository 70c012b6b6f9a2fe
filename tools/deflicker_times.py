"""Cost of one step of flicker removal next to the bidirectional call it follows and to the temporal filter's
step: the `deflicker_fit` (iters accumulate and field launches) and `deflicker_apply` stage times from eppm_stage_times for a single pair
and for a batch of slots stepped by the same launches, on a pair whose image 2 carries a gain ramp and an offset, with the bytes the
lanes request per pixel -- accumulate: frame word 4, backward vector 8, mask byte 1, four reference taps 16, and from the second pass on
the four field taps of 24 B each; apply: frame word 4, four field taps 96, output word 4; the field's 24 B per cell stay in the caches --
as a share of 8 TB/s.  One library per process:

    python tools/deflicker_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--cell N] [--iters N]

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
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    requested = {"deflicker_fit": 29 * a.iters + 96 * (a.iters - 1), "deflicker_apply": 104, "tfilter_step": 4 + 8 + 1 + 64 + 16 + 4}
    ramp = 1.0 + 0.08 * (np.arange(w) / (w - 1) - 0.5)[None, :, None]
    flick = lambda img: np.clip(np.rint(img * ramp * 1.05 + 5.0), 0, 255).astype(np.uint8)       # noqa: E731
    pairs = []
    for k in range(a.batch):
        f0, f1 = synth.make_pair_cached(h, w, seed=1234 + k)[:2]
        pairs.append((f0, flick(f1)))
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "cell": a.cell, "iters": a.iters,
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
        dk = eppm_amd.Deflicker(ctx, cell=a.cell, iters=a.iters)
        tf = eppm_amd.TemporalFilter(ctx)
        ctx.compute_flow_bidirectional_device()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            ctx.compute_flow_bidirectional_device()
            ctx.synchronize()
        r = {"bidir_dev_ms_per_pair": (time.perf_counter() - t0) * 1e3 / 3 / nslots}
        ms = stages(ctx, dk.step, ("deflicker_fit", "deflicker_apply"), before=dk.reset)      # every timed step starts from image 1
        st = [dk.stats(k) for k in range(nslots)]
        r.update({n: v / nslots for n, v in ms.items()})
        r["step_ms_per_pair"] = sum(ms.values()) / nslots
        r["share_used"] = float(np.mean([s["used"] / (h * w) for s in st]))
        r["share_valid_cells"] = float(np.mean([s["valid_cells"] / s["cells"] for s in st]))
        r["share_of_8TBs"] = {n: requested[n] * h * w * nslots / (ms[n] * 1e-3) / 8e12 for n in ms}
        r["step_share_of_bidir_dev"] = r["step_ms_per_pair"] / r["bidir_dev_ms_per_pair"]
        tf.step()
        r["tfilter_step_ms_per_pair"] = stages(ctx, tf.step, ("tfilter_step",))["tfilter_step"] / nslots
        dk.close()
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
