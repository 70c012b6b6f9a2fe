"""Cost of the synthetic shutter next to the forward-only compute it follows.  One library per process:

    python tools/mblur_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

(b) the engine's own flow on the bench's synthetic pair: ms per blurred frame for a single pair (host-pointer form; device form plus a
synchronise) and for a batch of pairs (host-pointer form), the two stages' device times from eppm_stage_times, and the forward-only
compute as the yardstick.  (a) a static field (the early-out path) and (c) a uniform 20-px motion at taps 8 and 32 (every pixel gathers)
have no context that computes them, so they run through eppm_motion_blur_frames on caller planes: ms per call (pack + gather + synchronise);
"shift20" is (c) as a context sees it (image 2 = image 1 moved by 20 px), which gives its stage times.  Prints one JSON line."""
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
    out = {"library": L.eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch}

    def per_call(fn):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def dev(arr):
        p = C.c_void_p()
        check(L.eppm_malloc_device(C.byref(p), C.c_size_t(arr.nbytes)), "malloc")
        check(L.eppm_memcpy_h2d(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
        return p

    def stages(e, fn):
        e.enable_stage_timing(True)
        e.stage_times()
        fn()
        st = e.stage_times()
        e.enable_stage_timing(False)
        return {n: round(ms, 4) for n, ms in st if n.startswith("mblur")}

    # (b) and shift20: the context forms
    d_out = C.c_void_p()
    check(L.eppm_malloc_device(C.byref(d_out), C.c_size_t(h * w * 4)), "malloc")
    shifted = np.roll(pairs[0][0], 20, axis=1)
    for label, (i1, i2) in (("engine", pairs[0]), ("shift20", (pairs[0][0], shifted))):
        e = eppm_amd.EPPM()
        e.init(i1, i2, h, w)
        r = {}
        if label == "engine":
            r["compute_ms"] = per_call(e.compute_flow)
            r["compute_dev_ms"] = per_call(lambda: (e.compute_flow_device(), e.synchronize()))
        u, v = e.compute_flow()
        r["share_of_vectors_20px"] = float((np.hypot(u - 20.0, v) < 0.5).mean())
        for taps in (8, 32):
            r[f"taps{taps}_host_ms"] = per_call(lambda: e.motion_blur(taps=taps))
            r[f"taps{taps}_dev_ms"] = per_call(lambda: (e.motion_blur_device(d_out.value, w * 4, taps=taps), e.synchronize()))
            r[f"taps{taps}_stages_ms"] = stages(e, lambda: e.motion_blur_device(d_out.value, w * 4, taps=taps))
        if label == "engine":
            r["share_of_dev_compute"] = r["taps8_dev_ms"] / r["compute_dev_ms"]
        out[label] = r
        e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    t0 = time.perf_counter()
    for _ in range(3):
        b.compute_flow()
    r = {"compute_ms_per_pair": (time.perf_counter() - t0) * 1e3 / 3 / a.batch}
    for taps in (8, 32):
        r[f"taps{taps}_host_ms_per_frame"] = per_call(lambda: b.motion_blur(taps=taps)) / a.batch
        r[f"taps{taps}_stages_ms_per_frame"] = {n: round(ms / a.batch, 5) for n, ms in stages(b, lambda: b.motion_blur(taps=taps)).items()}
    out["engine_batch"] = r
    b.close()

    # (a) and (c): the kernels alone on caller planes, one frame
    img = np.zeros((h, w, 4), np.uint8)
    img[..., :3] = pairs[0][0]
    d_img = dev(img)
    for label, vec in (("static", (0.0, 0.0)), ("uniform20", (20.0, 0.0))):
        flow = np.empty((h, w, 2), np.float32)
        flow[..., 0], flow[..., 1] = vec
        d_flow = dev(flow)
        r = {}
        for taps in (8, 32):
            p = eppm_amd.MBlurParams(taps=taps)
            r[f"taps{taps}_frames_ms"] = per_call(lambda: check(L.eppm_motion_blur_frames(d_out, C.c_size_t(w * 4), d_img, C.c_size_t(w * 4), d_flow, h, w,
                                                                                           C.byref(p)), "eppm_motion_blur_frames"))
        out[label] = r
        L.eppm_free_device(d_flow)
    L.eppm_free_device(d_img)
    L.eppm_free_device(d_out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
