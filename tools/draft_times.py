"""Cost and quality of draft mode (eppm_set_stop_level): for the stop levels 0, 1 and 2, ms per pair of the
device-resident compute (images set, eppm_compute_device + synchronize, wall clock), the stage table of one compute, the end-point error
against synth.make_pair's ground truth (16-px border excluded) and against the stop-level-0 flow, at

    1024x436 single pair | 1024x436 batch of 8 | 1920x1080 | 3840x2160 at patch radius 17

and the upsampling kernel against the smoothing kernel on the same pixels and taps: stage flow_jbu_L0 of the stop-level-1 row over stage
flow_blf_final of the stop-level-0 row.  One process, one context at a time, one library per process:

    python tools/draft_times.py [--lib exact|tol] [--steps N] [--only NAME]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("1024x436", 436, 1024, 9, 1, 20.0), ("1024x436_batch8", 436, 1024, 9, 8, 20.0), ("1920x1080", 1080, 1920, 9, 1, 40.0),
         ("3840x2160_r17", 2160, 3840, 17, 1, 60.0))
BORDER = 16


def epe(u, v, gu, gv):
    known = ~((u > 1e9) | (v > 1e9) | (gu > 1e9) | (gv > 1e9))
    e = np.sqrt((u.astype(np.float64) - gu) ** 2 + (v.astype(np.float64) - gv) ** 2)
    inner = (slice(BORDER, -BORDER), slice(BORDER, -BORDER))
    return float(e[inner][known[inner]].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", default=None, help="one case by name")
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    out = {"library": eppm_amd.lib().eppm_version().decode(), "steps": a.steps, "cases": {}}
    for name, h, w, R, batch, max_flow in CASES:
        if a.only and a.only != name:
            continue
        pairs = [synth.make_pair_cached(h, w, seed=1234 + k, max_flow=max_flow) for k in range(batch)]
        prm = eppm_amd.Params(patch_r=R)
        if batch == 1:
            e = eppm_amd.EPPM(params=prm)
            e.init(pairs[0][0], pairs[0][1], h, w)
            flows = lambda: [e.compute_flow()]                       # noqa: E731
        else:
            e = eppm_amd.EPPMBatch(h, w, batch, params=prm)
            e.set_data([p[:2] for p in pairs])
            flows = e.compute_flow
        nl = int(eppm_amd.lib().eppm_num_levels(e._ctx))
        steps = max(4, a.steps // 4) if h * w > 4e6 else a.steps
        rows, base = {}, None
        for s in range(nl):
            e.set_stop_level(s)
            for _ in range(3):
                e.compute_flow_device(); e.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                e.compute_flow_device()
            e.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps / batch
            e.enable_stage_timing(True)
            e.stage_times()
            e.compute_flow_device(); e.synchronize()
            st = e.stage_times()
            e.enable_stage_timing(False)
            got = flows()
            if s == 0:
                base = got
            rows[s] = {"ms_per_pair": round(ms, 4), "stages_ms_per_pair": {n: round(t / batch, 4) for n, t in st},
                       "epe_gt": round(float(np.mean([epe(f[0], f[1], p[2], p[3]) for f, p in zip(got, pairs)])), 4),
                       "epe_vs_stop0": round(float(np.mean([epe(f[0], f[1], g[0], g[1]) for f, g in zip(got, base)])), 4)}
        e.close()
        c = {"stop": rows}
        for s in range(1, nl):
            c[f"speedup_stop{s}"] = round(rows[0]["ms_per_pair"] / rows[s]["ms_per_pair"], 3)
        if nl > 1:
            c["jbu_L0_over_blf_final"] = round(rows[1]["stages_ms_per_pair"]["flow_jbu_L0"] / rows[0]["stages_ms_per_pair"]["flow_blf_final"], 4)
        out["cases"][name] = c
        print(f"{name}: " + ", ".join(f"s={s} {rows[s]['ms_per_pair']:.3f} ms EPE {rows[s]['epe_gt']:.3f}" for s in rows) +
              f"; flow_jbu_L0 / flow_blf_final {c.get('jbu_L0_over_blf_final', float('nan')):.3f}", file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
