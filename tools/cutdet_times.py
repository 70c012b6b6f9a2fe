"""Cost of one cut-detector step next to the bidirectional call it follows: the `cutdet` stage time from
eppm_stage_times, the enqueue + cuts() round trip from Python (the step, the synchronisation and the one small copy), for a single pair and
for a batch of slots stepped together, and the bytes the lanes request (18 B per pixel: 4 image 2 + 4 one gathered word of image 1 +
8 flow + 1 + 1 masks) as a share of 8 TB/s.  Also the cost of the per-step host read in auto_cut mode (denoise_sequence with and without
auto_cut on a cut-free clip) and, with --shares, the lost shares and mean residuals of a clip of two shots at the same size, at stop
levels 0 and 1.  One library per process:

    python tools/cutdet_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--shares]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL = 4 + 4 + 8 + 1 + 1           # requested by the lanes


def shot(h, w, nframes, seed, step, sigma=5.0):
    """a synthetic shot: a smooth textured scene seen through a window that moves by `step` px per frame, Gaussian noise of `sigma`"""
    import numpy as np
    from eppm_amd import synth
    pad = nframes * max(abs(step[0]), abs(step[1]), 1)
    scene = synth.make_pair_cached(h + 2 * pad, w + 2 * pad, seed=seed)[0]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(nframes):
        f = scene[pad - k * step[1]: pad - k * step[1] + h, pad - k * step[0]: pad - k * step[0] + w].astype(np.float64)
        out.append(np.clip(np.rint(f + rng.normal(0, sigma, f.shape)), 0, 255).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--shares", action="store_true")
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "launches_per_step": 2,
           "bytes_per_pixel": BYTES_PER_PIXEL}

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def stage(ctx, det, n=10):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            det.step()
        ctx.synchronize()
        t = ctx.stage_times()
        ctx.enable_stage_timing(False)
        return sorted(ms for k, ms in t if k == "cutdet")[n // 2]

    def report(prefix, ms, bidir, npx):
        out[prefix + "_stage_ms"] = ms
        out[prefix + "_share_of_bidir_dev"] = ms / bidir
        out[prefix + "_requested_share_of_8TBs"] = BYTES_PER_PIXEL * npx / (ms * 1e-3) / 8e12

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_bidir_dev_ms"] = per_call(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()), max(3, a.steps // 5))
    det = eppm_amd.CutDetector(e)
    det.step()
    out["single_step_and_cuts_ms"] = per_call(lambda: (det.step(), det.cuts()))
    report("single", stage(e, det), out["single_bidir_dev_ms"], h * w)
    s = det.stats(0)
    out["single_record"] = {k: s[k] for k in ("n", "c1", "c2", "n_tracked", "sad", "cut")}
    det.close()
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out["batch_bidir_dev_ms_per_pair"] = per_call(lambda: (b.compute_flow_bidirectional_device(), b.synchronize()), 3) / a.batch
    det = eppm_amd.CutDetector(b)
    det.step()
    out["batch_step_and_cuts_ms_per_pair"] = per_call(lambda: (det.step(), det.cuts())) / a.batch
    report("batch", stage(b, det) / a.batch, out["batch_bidir_dev_ms_per_pair"], h * w)
    det.close()
    b.close()

    # the price of the per-step host read: a cut-free clip with and without auto_cut
    clip = shot(h, w, 6, 77, (2, 1))
    for key, kw in (("denoise_ms_per_pair", {}), ("denoise_auto_cut_ms_per_pair", {"auto_cut": True})):
        eppm_amd.denoise_sequence(clip[:3], **kw)
        t0 = time.perf_counter()
        eppm_amd.denoise_sequence(clip, **kw)
        out[key] = (time.perf_counter() - t0) * 1e3 / (len(clip) - 1)

    if a.shares:
        film = clip[:4] + shot(h, w, 3, 78, (5, -4))
        for level in (0, 1):
            cuts, stats = eppm_amd.detect_cuts(film, stop_level=level)
            out[f"shares_stop_level_{level}"] = [
                {"pair": k, "cut": int(c), "lost1": round(1 - r["c1"][0] / r["n"], 4), "lost2": round(1 - r["n_tracked"] / r["n"], 4),
                 "mean_residual": round(r["sad"] / max(r["n_tracked"], 1), 3)} for k, (c, r) in enumerate(zip(cuts, stats))]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
