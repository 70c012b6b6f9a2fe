"""Cost of rolling-shutter correction next to the forward-only compute it follows.  One library per process:

    python tools/rshutter_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

The engine's own flow on the bench's synthetic pair: ms per corrected frame for a single pair (host-pointer form; device form plus a
synchronise) and for a batch of pairs (host-pointer form), the two stages' device times from eppm_stage_times at 1, 3 and 8 fixed-point
steps, and the forward-only compute as the yardstick.  "frames": the kernels alone on caller planes (eppm_rolling_shutter_frames:
velocity + gather + synchronise) on a uniform 20-px motion along the readout axis, rows and columns.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

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
    L = lib()
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": L.eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "requested_bytes_per_pixel_and_pair": 11}

    def per_call(fn):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def dev(arr):
        p = C.c_void_p()
        check(L.eppm_malloc_device(C.byref(p), arr.nbytes), "malloc")
        check(L.eppm_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "h2d")
        return p

    def stages(e, fn):
        e.enable_stage_timing(True)
        e.stage_times()
        fn()
        st = e.stage_times()
        e.enable_stage_timing(False)
        return {n: round(ms, 4) for n, ms in st if n.startswith("rs_")}

    d_out = C.c_void_p()
    check(L.eppm_malloc_device(C.byref(d_out), h * w * 4), "malloc")
    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    r = {"compute_ms": per_call(e.compute_flow), "compute_dev_ms": per_call(lambda: (e.compute_flow_device(), e.synchronize()))}
    e.compute_flow()
    for iters in (1, 3, 8):
        kw = dict(readout=1.0, iters=iters)
        r[f"iters{iters}_host_ms"] = per_call(lambda: e.rolling_shutter(**kw))
        r[f"iters{iters}_dev_ms"] = per_call(lambda: (e.rolling_shutter_device(d_out.value, w * 4, **kw), e.synchronize()))
        r[f"iters{iters}_stages_ms"] = stages(e, lambda: e.rolling_shutter_device(d_out.value, w * 4, **kw))
    r["share_of_dev_compute"] = r["iters3_dev_ms"] / r["compute_dev_ms"]
    out["engine"] = r
    e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    t0 = time.perf_counter()
    for _ in range(3):
        b.compute_flow()
    r = {"compute_ms_per_pair": (time.perf_counter() - t0) * 1e3 / 3 / a.batch}
    for iters in (3, 8):
        kw = dict(readout=1.0, iters=iters)
        r[f"iters{iters}_host_ms_per_frame"] = per_call(lambda: b.rolling_shutter(**kw)) / a.batch
        r[f"iters{iters}_stages_ms_per_frame"] = {n: round(ms / a.batch, 5) for n, ms in stages(b, lambda: b.rolling_shutter(**kw)).items()}
    out["engine_batch"] = r
    b.close()

    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = pairs[0][0]
    d_img = dev(img)
    r = {}
    for axis, vec in ((0, (0.0, 20.0)), (1, (20.0, 0.0))):
        flow = np.empty((h, w, 2), np.float32)
        flow[..., 0], flow[..., 1] = vec
        d_flow = dev(flow)
        for iters in (3, 8):
            p = eppm_amd.RSParams(readout=1.0, iters=iters, axis=axis)
            r[f"axis{axis}_iters{iters}_ms"] = per_call(lambda: check(L.eppm_rolling_shutter_frames(d_out, w * 4, d_img, w * 4, d_flow, h, w, 0, C.byref(p)),
                                                                      "eppm_rolling_shutter_frames"))
        L.eppm_free_device(d_flow)
    out["frames"] = r
    L.eppm_free_device(d_img)
    L.eppm_free_device(d_out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
