"""Cost of one stabiliser step next to the bidirectional call it follows: ms per device-resident step for a single
pair and for a batch of slots stepped together, the `stab_fit` (every accumulate and solve launch) and `stab_warp` stage times from
eppm_stage_times, and the bytes the lanes request: 9 B per pixel per fit pass (8 flow + 1 mask) and, in the warp, 4 x 4 taps + 8 flow +
1 mask read and 4 output + 1 mask written; as a share of 8 TB/s.  One library per process:

    python tools/stab_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--iters I]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIT_BYTES_PER_PIXEL_PER_PASS = 8 + 1
WARP_BYTES_PER_PIXEL = 4 * 4 + 8 + 1 + 4 + 1           # requested by the lanes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "iters": a.iters,
           "launches_per_step": 2 * a.iters + 1, "fit_bytes_per_pixel": FIT_BYTES_PER_PIXEL_PER_PASS * a.iters,
           "warp_bytes_per_pixel": WARP_BYTES_PER_PIXEL}

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def stages(ctx, stab, n=10):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            stab.step()
        ctx.synchronize()
        t = ctx.stage_times()
        ctx.enable_stage_timing(False)
        med = lambda name: sorted(ms for k, ms in t if k == name)[n // 2]          # noqa: E731
        return med("stab_fit"), med("stab_warp")

    def report(prefix, fit, warp, bidir, npx):
        out[prefix + "_fit_stage_ms"] = fit
        out[prefix + "_warp_stage_ms"] = warp
        out[prefix + "_step_share_of_bidir_dev"] = (fit + warp) / bidir
        out[prefix + "_fit_requested_share_of_8TBs"] = FIT_BYTES_PER_PIXEL_PER_PASS * a.iters * npx / (fit * 1e-3) / 8e12
        out[prefix + "_warp_requested_share_of_8TBs"] = WARP_BYTES_PER_PIXEL * npx / (warp * 1e-3) / 8e12

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_bidir_dev_ms"] = per_call(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()), max(3, a.steps // 5))
    stab = eppm_amd.Stabilizer(e, iters=a.iters)
    stab.step()
    out["single_step_dev_ms"] = per_call(lambda: (stab.step(), e.synchronize()))
    fit, warp = stages(e, stab)
    report("single", fit, warp, out["single_bidir_dev_ms"], h * w)
    m = stab.model(0)
    out["single_model"] = {"p": [float(x) for x in m["p"]], "n_valid": m["n_valid"], "n_inliers": m["n_inliers"], "valid": m["valid"]}
    stab.close()
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out["batch_bidir_dev_ms_per_pair"] = per_call(lambda: (b.compute_flow_bidirectional_device(), b.synchronize()), 3) / a.batch
    stab = eppm_amd.Stabilizer(b, iters=a.iters)
    stab.step()
    out["batch_step_dev_ms_per_pair"] = per_call(lambda: (stab.step(), b.synchronize())) / a.batch
    fit, warp = stages(b, stab)
    report("batch", fit / a.batch, warp / a.batch, out["batch_bidir_dev_ms_per_pair"], h * w)
    stab.close()
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
