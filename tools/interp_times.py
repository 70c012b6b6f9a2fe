"""Cost of frame interpolation next to the bidirectional call it follows: ms per interpolated frame for a
single pair with nt = 1 (host-pointer and device forms) and for a batch of pairs with nt = 7, and the three stages' device times from
eppm_stage_times.  One library per process:

    python tools/interp_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

Prints one JSON line."""
import argparse
import ctypes as C
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
    from eppm_amd._lib import check, lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch}

    def per_call(fn):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out["single_bidir_ms"] = per_call(e.compute_flow_bidirectional)
    out["single_bidir_dev_ms"] = per_call(lambda: (e.compute_flow_bidirectional_device(), e.synchronize()))
    e.compute_flow_bidirectional()
    out["single_interp_ms_per_frame"] = per_call(lambda: e.interpolate([0.5]))
    d = C.c_void_p()
    check(lib().eppm_malloc_device(C.byref(d), C.c_size_t(h * w * 4)), "malloc")
    out["single_interp_dev_ms_per_frame"] = per_call(lambda: (e.interpolate_device([0.5], [d.value], w * 4), e.synchronize()))
    e.enable_stage_timing(True)
    e.stage_times()
    e.interpolate_device([0.5], [d.value], w * 4)
    st = e.stage_times()
    out["single_stages_ms"] = {n: round(ms, 4) for n, ms in st}
    out["single_interp_dev_share_of_bidir_dev"] = out["single_interp_dev_ms_per_frame"] / out["single_bidir_dev_ms"]
    lib().eppm_free_device(d)
    e.close()

    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    t0 = time.perf_counter()
    for _ in range(3):
        b.compute_flow_bidirectional()
    out["batch_bidir_ms_per_pair"] = (time.perf_counter() - t0) * 1e3 / 3 / a.batch
    times = [k / 8 for k in range(1, 8)]
    out["batch_interp_ms_per_frame"] = per_call(lambda: b.interpolate(times)) / (a.batch * len(times))
    b.enable_stage_timing(True)
    b.stage_times()
    b.interpolate(times)
    st = b.stage_times()
    agg = {}
    for n, ms in st:
        agg[n] = agg.get(n, 0.0) + ms
    out["batch_stages_ms_per_frame"] = {n: round(ms / (a.batch * len(times)), 5) for n, ms in agg.items()}
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
