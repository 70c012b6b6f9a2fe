"""Cost of one step of the motion-compensated temporal filter next to the bidirectional call it follows: ms per
device-resident step for a single pair and for a batch of slots stepped by one launch, the `tfilter_step` stage time from
eppm_stage_times, and the bytes the step moves (97 B per pixel: 4 frame + 8 flow + 1 mask + 4 x 16 taps read, 16 state + 4 output
written; the taps of neighbouring lanes overlap, so HBM sees fewer) as a share of 8 TB/s.  One library per process:

    python tools/tfilter_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL = 4 + 8 + 1 + 4 * 16 + 16 + 4          # requested by the lanes
HBM_BYTES_PER_PIXEL = 4 + 8 + 1 + 16 + 16 + 4          # if every state pixel is fetched once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=50)
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
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch,
           "bytes_per_pixel": BYTES_PER_PIXEL, "hbm_bytes_per_pixel": HBM_BYTES_PER_PIXEL}

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def stage(ctx, flt, n=10):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            flt.step()
        ctx.synchronize()
        ms = sorted(t for name, t in ctx.stage_times() if name == "tfilter_step")
        ctx.enable_stage_timing(False)
        return ms[len(ms) // 2]

    def shares(ms, npx):
        return {"requested_share_of_8TBs": BYTES_PER_PIXEL * npx / (ms * 1e-3) / 8e12, "hbm_share_of_8TBs": HBM_BYTES_PER_PIXEL * npx / (ms * 1e-3) / 8e12}

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_bidir_dev_ms"] = per_call(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()), max(3, a.steps // 5))
    flt = eppm_amd.TemporalFilter(e)
    flt.step()
    out["single_step_dev_ms"] = per_call(lambda: (flt.step(), e.synchronize()))
    out["single_stage_ms"] = stage(e, flt)
    out["single_step_share_of_bidir_dev"] = out["single_stage_ms"] / out["single_bidir_dev_ms"]
    out["single_bandwidth"] = shares(out["single_stage_ms"], h * w)
    n = flt.state(0)[..., 3]
    out["single_share_n_ge_2"] = float((n >= 2).mean())
    flt.close()
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out["batch_bidir_dev_ms_per_pair"] = per_call(lambda: (b.compute_flow_bidirectional_device(), b.synchronize()), 3) / a.batch
    flt = eppm_amd.TemporalFilter(b)
    flt.step()
    out["batch_step_dev_ms_per_pair"] = per_call(lambda: (flt.step(), b.synchronize())) / a.batch
    out["batch_stage_ms_per_pair"] = stage(b, flt) / a.batch
    out["batch_step_share_of_bidir_dev"] = out["batch_stage_ms_per_pair"] / out["batch_bidir_dev_ms_per_pair"]
    out["batch_bandwidth"] = shares(out["batch_stage_ms_per_pair"], h * w)
    flt.close()
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
