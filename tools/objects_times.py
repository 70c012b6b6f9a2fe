"""Cost of one step of the moving-object detector next to the bidirectional call it follows and next to the
stabiliser's fit (section 16), in one process: ms per device-resident step for a single pair and for a batch of slots stepped by one
sequence of launches, the `objects_fit`, `objects_label` and `objects_assign` stage times from eppm_stage_times beside `stab_fit`, and --
because the labelling's work depends on the mask -- the wall time of a synchronous eppm_objects_step_frames on caller planes for masks of
several classes (empty, full, random at 45 %, checkerboard, one-pixel spiral, comb, a few rectangles).  One library per process:

    python tools/objects_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--classes-only]

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spiral(h, w):
    m = np.zeros((h, w), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    while True:
        for _ in range(2):
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if 0 <= nx < w and 0 <= ny < h and not m[ny, nx] and not (0 <= fx < w and 0 <= fy < h and m[fy, fx]):
                x, y = nx, ny
                m[y, x] = 1
                break
            dx, dy = -dy, dx
        else:
            return m


def masks(h, w):
    rng = np.random.default_rng(7)
    ys, xs = np.mgrid[0:h, 0:w]
    comb = np.zeros((h, w), np.uint8)
    comb[:, ::2] = 1
    comb[-1, :] = 1
    rects = np.zeros((h, w), np.uint8)
    for k in range(6):
        y0, x0 = int(rng.integers(0, h - 60)), int(rng.integers(0, w - 90))
        rects[y0:y0 + 60, x0:x0 + 90] = 1
    return {"empty": np.zeros((h, w), np.uint8), "full": np.ones((h, w), np.uint8), "rects": rects,
            "rand45": (rng.random((h, w)) < 0.45).astype(np.uint8), "checker": ((xs + ys) % 2 == 0).astype(np.uint8),
            "comb": comb, "spiral": spiral(h, w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--classes-only", action="store_true", help="only the mask classes on caller planes (what a kernel profile wants)")
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import check, lib
    h, w = a.height, a.width
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch, "launches_per_step": 9}

    def to_device(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(arr.nbytes)), "malloc")
        check(lib().eppm_memcpy_h2d(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
        return p

    # the mask classes, on caller planes: a uniform vector field, every step from an empty slot
    flow = to_device(np.full((h, w, 2), 1.25, np.float32))
    occ = to_device(np.zeros((h, w), np.uint8))
    det = eppm_amd.ObjectDetector(None, size=(h, w), connectivity=8, min_area=16, max_objects=64)
    out["classes"] = {}
    for name, m in masks(h, w).items():
        d_mask = to_device(m)
        for k in range(3):
            det.step_frames(0, d_mask.value, flow.value, flow.value, occ.value)
        t0 = time.perf_counter()
        for k in range(a.steps):
            det.step_frames(0, d_mask.value, flow.value, flow.value, occ.value)
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        out["classes"][name] = {"step_frames_wall_ms": ms, **det.counts(0)}
        lib().eppm_free_device(d_mask)
    det.close()
    lib().eppm_free_device(flow)
    lib().eppm_free_device(occ)
    if a.classes_only:
        print(json.dumps(out))
        return

    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def stages(ctx, obj, names, n=10):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            obj.step()
        ctx.synchronize()
        got = ctx.stage_times()
        ctx.enable_stage_timing(False)
        res = {}
        for name in names:
            ms = sorted(t for k, t in got if k == name)
            res[name] = ms[len(ms) // 2]
        return res

    def measure(ctx, sync, n_pairs, tag, bidir_steps):
        res = {}
        res[f"{tag}_bidir_dev_ms_per_pair"] = per_call(lambda: (ctx.compute_flow_bidirectional_device(), sync()), bidir_steps) / n_pairs
        od = eppm_amd.ObjectDetector(ctx)
        res[f"{tag}_step_dev_ms_per_pair"] = per_call(lambda: (od.step(), sync())) / n_pairs
        st = stages(ctx, od, ("objects_fit", "objects_label", "objects_assign"))
        res[f"{tag}_counts_slot0"] = od.counts(0)
        od.close()
        stab = eppm_amd.Stabilizer(ctx)
        stab.step()
        st.update(stages(ctx, stab, ("stab_fit", "stab_warp")))
        stab.close()
        for name, ms in st.items():
            res[f"{tag}_{name}_stage_ms_per_pair"] = ms / n_pairs
            res[f"{tag}_{name}_share_of_bidir_dev"] = ms / n_pairs / res[f"{tag}_bidir_dev_ms_per_pair"]
        return res

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out.update(measure(e, e.synchronize, 1, "single", max(3, a.steps // 5)))
    e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out.update(measure(b, b.synchronize, a.batch, "batch", 3))
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
