"""Cost of the bidirectional call against the forward one: ms per pair of eppm_compute and eppm_compute_bidirectional (wall clock of
the synchronous host call, images already set), single-pair and batch contexts, and the share of every backward stage in one
bidirectional call from eppm_stage_times.  One library per process:

    python tools/bidir_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

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
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": eppm_amd.lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch}

    def per_pair(fn, npairs):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.steps / npairs

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_fwd_ms"] = per_pair(e.compute_flow, 1)
    out["single_bidir_ms"] = per_pair(e.compute_flow_bidirectional, 1)
    out["single_fwd_ms_again"] = per_pair(e.compute_flow, 1)
    # device-resident forms (no host boundary): what the GPU work costs
    out["single_fwd_dev_ms"] = per_pair(lambda: (e.compute_flow_device(), e.synchronize()), 1)
    out["single_bidir_dev_ms"] = per_pair(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()), 1)
    e.enable_stage_timing(True)
    e.stage_times()
    e.compute_flow_bidirectional()
    st = e.stage_times()
    total = sum(ms for n, ms in st)
    out["stages_ms"] = {n: round(ms, 4) for n, ms in st}
    out["stage_sum_ms"] = total
    out["bwd_stage_sum_ms"] = sum(ms for n, ms in st if "bwd" in n or n == "fb_occlusion")
    out["fb_occlusion_share"] = dict(st)["fb_occlusion"] / total
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out["batch_fwd_ms"] = per_pair(b.compute_flow, a.batch)
    out["batch_bidir_ms"] = per_pair(b.compute_flow_bidirectional, a.batch)
    b.enable_stage_timing(True)
    b.stage_times()
    b.compute_flow()
    out["batch_fwd_stages_ms_per_pair"] = {n: round(ms / a.batch, 4) for n, ms in b.stage_times()}
    b.compute_flow_bidirectional()
    out["batch_bidir_stages_ms_per_pair"] = {n: round(ms / a.batch, 4) for n, ms in b.stage_times()}
    b.close()
    out["ratio_single"] = out["single_bidir_ms"] / out["single_fwd_ms"]
    out["ratio_batch"] = out["batch_bidir_ms"] / out["batch_fwd_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
