"""Cost of one step of film-defect removal next to the bidirectional call it follows and to the temporal filter's
step: the `defect_detect` and `defect_apply` stage times from eppm_stage_times for a single pair and for a batch of slots stepped by one
launch, on a natural share of undecided pixels (the middle frame of a three-frame clip, the engine's own flows) and on 100 % (every saved
backward vector points out of the frame, so every lane selects its window medians), with the bytes a step moves if every plane pixel is
fetched once (detect: 36 B read -- frame word, forward, own and saved backward vector, one word of each neighbour frame -- and 17 B
written; apply: 9 B read, 5 B written) as a share of 8 TB/s.  One library per process:

    python tools/defect_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES = {"defect_detect": 36 + 17, "defect_apply": 9 + 5, "tfilter_step": 4 + 8 + 1 + 16 + 16 + 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "hbm_bytes_per_pixel": HBM_BYTES}

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

    def measure(ctx, nslots, frames, tag):
        """frames: per slot (f0, f1): the clip f0, f1, f0; the timed step repairs f1 on the pair (f1, f0)"""
        import time
        flt = eppm_amd.DefectFilter(ctx)
        tf = eppm_amd.TemporalFilter(ctx)
        single = nslots == 1
        res = ctx.compute_flow_bidirectional()                       # the pair (f0, f1): its backward flow is what the next step reads
        res = [res] if single else res
        saved = [(frames[k][0], np.stack(res[k][2:4], -1)) for k in range(nslots)]
        far = [(frames[k][0], np.full((h, w, 2), 1e6, np.float32)) for k in range(nslots)]
        if single:
            ctx.push_frame(frames[0][0])
        else:
            ctx.push_frames([f[0] for f in frames], [False] * nslots)
        t0 = time.perf_counter()
        for _ in range(3):
            ctx.compute_flow_bidirectional_device()
            ctx.synchronize()
        r = {"bidir_dev_ms_per_pair": (time.perf_counter() - t0) * 1e3 / 3 / nslots}
        for name, state in (("natural", saved), ("all_second_chance", far)):
            load = lambda: [flt.set_state(k, state[k][0], state[k][1], True) for k in range(nslots)]      # noqa: E731
            ms = stages(ctx, flt.step, ("defect_detect", "defect_apply"), before=load)
            st = [flt.stats(k) for k in range(nslots)]
            r[name] = {n: v / nslots for n, v in ms.items()}
            r[name]["step_ms_per_pair"] = sum(ms.values()) / nslots
            r[name]["share_second_chance_or_undecided"] = float(np.mean([(s["second_chance"] + s["undecided"]) / (h * w) for s in st]))
            r[name]["share_hit_or_grown"] = float(np.mean([(s["hit"] + s["grown"]) / (h * w) for s in st]))
            r[name]["share_of_8TBs"] = {n: HBM_BYTES[n] * h * w * nslots / (ms[n] * 1e-3) / 8e12 for n in ms}
            r[name]["step_share_of_bidir_dev"] = r[name]["step_ms_per_pair"] / r["bidir_dev_ms_per_pair"]
        tf.step()
        r["tfilter_step_ms_per_pair"] = stages(ctx, tf.step, ("tfilter_step",))["tfilter_step"] / nslots
        flt.close()
        tf.close()
        out[tag] = r

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    measure(e, 1, pairs[:1], "single")
    e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    measure(b, a.batch, pairs, "batch")
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
