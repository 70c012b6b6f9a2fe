"""Cost of one dense-trajectory step next to the bidirectional call it follows: ms per device-resident step for a
single pair and for a batch of pairs stepped as one sequence, the three stages' device times from eppm_stage_times, and the live, seeded
and ended counts.  One library per process:

    python tools/track_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--spacing S]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--spacing", type=int, default=8)
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    ncells = -(-w // a.spacing) * -(-h // a.spacing)
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "spacing": a.spacing, "cells": ncells, "steps": a.steps, "batch": a.batch}

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_bidir_dev_ms"] = per_call(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()), max(3, a.steps // 3))
    e.compute_flow_bidirectional_device()
    t = eppm_amd.Tracker(e, spacing=a.spacing)
    e.enable_stage_timing(True)
    e.stage_times()
    t.step()                                         # frame 0: seeds image 1 first
    first = e.stage_times()
    c = t.counts()
    out["first_step"] = {"stages_ms": [[n, round(ms, 4)] for n, ms in first], "live": c["live"], "seeded": c["seeded"], "ended": c["ended"]}
    t.step()
    st = e.stage_times()
    c = t.counts()
    out["single_stages_ms"] = {n: round(ms, 4) for n, ms in st}
    out["second_step_counts"] = {k: c[k] for k in ("live", "seeded", "ended", "dropped")}
    e.enable_stage_timing(False)
    out["single_step_dev_ms"] = per_call(lambda: (t.step(), e.synchronize()))
    out["single_step_share_of_bidir_dev"] = out["single_step_dev_ms"] / out["single_bidir_dev_ms"]
    c = t.counts()
    out["single_after"] = {k: c[k] for k in ("live", "seeded", "ended", "dropped", "frame")}
    t.close()
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    b.compute_flow_bidirectional()
    t0 = time.perf_counter()
    for _ in range(3):
        b.compute_flow_bidirectional()
    out["batch_bidir_ms_per_pair"] = (time.perf_counter() - t0) * 1e3 / 3 / a.batch
    t = eppm_amd.Tracker(b, spacing=a.spacing)

    def sequence():
        t.set([], [], [], 0, 0)
        for k in range(a.batch):
            t.step(k)
        b.synchronize()
    out["batch_step_ms_per_pair"] = per_call(sequence, max(3, a.steps // 3)) / a.batch
    out["batch_step_share_of_bidir"] = out["batch_step_ms_per_pair"] / out["batch_bidir_ms_per_pair"]
    c = t.counts()
    out["batch_after"] = {k: c[k] for k in ("live", "seeded", "ended", "dropped", "frame")}
    t.close()
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
