"""ms per pair over a steady-motion clip for the three ways of walking it, with the mean level-2 PatchMatch cost
and the end-point error against the clip's ground truth per row:
  (a) set_images + compute per pair      (b) push_image + compute      (c) b + temporal mode at num_iter 10, 8, 6
Control rows: push without a prior at 8 and 6 iterations.  --rows a: row (a) alone, for a library built from a commit without the
streaming entry points.  --batch N: instead, N copies of the clip through one N-slot batch context in temporal mode (push_frames, section
13.1): ms per step and per pair (a step advances N pairs), and whether every slot's flows equal slot 0's.
Usage: python tools/temporal_times.py [--lib tol] [--frames N] [--reps R] [--size WxH] [--batch N]; one JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clip(h, w, seed, n):
    from eppm_amd import synth
    a, b, u, v = synth.make_pair_cached(h, w, seed=seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = [a, b]
    while len(frames) < n:
        frames.append(np.clip(synth._bilinear(frames[-1].astype(np.float64), xx - u, yy - v), 0, 255).astype(np.uint8))
    return frames, u, v


def walk(frames, gt, mode, num_iter, reps):
    import eppm_amd
    from eppm_amd import io
    h, w, _ = frames[0].shape
    e = eppm_amd.EPPM(params=eppm_amd.Params(num_iter=num_iter))
    e.init(h, w)
    if mode == "temporal":
        e.set_temporal(True)
    L = len(e.level_dims()) - 1
    best, costs, epes, stages = float("inf"), [], [], {}
    for rep in range(reps + 1):                       # the first walk warms up
        last = rep == reps
        if last:
            e.enable_stage_timing(True)
            e.stage_times()
        e.set_data(frames[0], frames[1])
        e.compute_flow()
        t0 = time.perf_counter()
        for k in range(1, len(frames) - 1):
            if mode == "set_images":
                e.set_data(frames[k], frames[k + 1])
            else:
                e.push_frame(frames[k + 1])
            u, v = e.compute_flow()
            if last:
                c = e.plane("cost1", L)                                # after the left-right check, which marks rejected pixels with a huge cost
                costs.append(float(c[c < 1e9].mean()))
                epes.append(io.flow_error(u, v, gt[0], gt[1])[0])
        dt = (time.perf_counter() - t0) * 1e3 / (len(frames) - 2)
        if not last:
            best = min(best, dt)
    for name, ms in e.stage_times():
        if name.startswith("temporal") or name in ("prepare", "patchmatch"):
            stages.setdefault(name, []).append(ms)
    e.close()
    return {"mode": mode, "num_iter": num_iter, "ms_per_pair": round(best, 4), "mean_cost_L": round(float(np.mean(costs)), 5),
            "epe": round(float(np.mean(epes)), 5), "stage_ms": {k: round(float(np.mean(v)), 4) for k, v in stages.items()}}


def walk_batch(frames, gt, slots, num_iter, reps):
    import eppm_amd
    from eppm_amd import io
    h, w, _ = frames[0].shape
    e = eppm_amd.EPPMBatch(h, w, slots, params=eppm_amd.Params(num_iter=num_iter))
    e.set_temporal(True)
    out = [(np.empty((h, w), np.float32), np.empty((h, w), np.float32)) for _ in range(slots)]
    best, epes, same, stages = float("inf"), [], True, {}
    for rep in range(reps + 1):                       # the first walk warms up
        last = rep == reps
        if last:
            e.enable_stage_timing(True)
            e.stage_times()
        e.set_data([(frames[0], frames[1])] * slots)
        e.compute_flow(out)
        t0 = time.perf_counter()
        for k in range(1, len(frames) - 1):
            e.push_frames([frames[k + 1]] * slots)
            res = e.compute_flow(out)
            if last:
                epes.append(io.flow_error(res[0][0], res[0][1], gt[0], gt[1])[0])
                same = same and all(np.array_equal(res[0][0], r[0]) and np.array_equal(res[0][1], r[1]) for r in res[1:])
        dt = (time.perf_counter() - t0) * 1e3 / (len(frames) - 2)
        if not last:
            best = min(best, dt)
    for name, ms in e.stage_times():
        if name.startswith("temporal") or name in ("prepare", "patchmatch"):
            stages.setdefault(name, []).append(ms)
    e.close()
    return {"mode": "batch_temporal", "slots": slots, "num_iter": num_iter, "ms_per_step": round(best, 4), "ms_per_pair": round(best / slots, 4),
            "epe": round(float(np.mean(epes)), 5), "slots_equal": bool(same), "stage_ms": {k: round(float(np.mean(v)), 4) for k, v in stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default="1024x436")
    ap.add_argument("--rows", default="all", help="a: row (a) only, which needs no streaming entry point (a library built from an earlier commit)")
    ap.add_argument("--batch", type=int, default=0, help="N > 0: N copies of the clip through one N-slot batch context in temporal mode")
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library(a.lib)
    w, h = (int(t) for t in a.size.split("x"))
    frames, u, v = clip(h, w, 1234, a.frames)
    print(json.dumps({"version": eppm_amd.lib().eppm_version().decode(), "size": a.size, "frames": a.frames, "reps": a.reps}))
    if a.batch > 0:
        print(json.dumps(walk_batch(frames, (u, v), a.batch, 10, a.reps)), flush=True)
        return
    rows = (("set_images", 10), ("push", 10), ("temporal", 10), ("temporal", 8), ("temporal", 6), ("push", 8), ("push", 6))
    for mode, it in (rows[:1] if a.rows == "a" else rows):
        print(json.dumps(walk(frames, (u, v), mode, it, a.reps)), flush=True)


if __name__ == "__main__":
    main()
