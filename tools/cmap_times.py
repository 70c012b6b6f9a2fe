"""Cost of one step and one render of the dense correspondence map next to the bidirectional call they follow and
next to the temporal filter's step (section 15), in one process: ms per device-resident step (the step launches the render of the slots
it covers) for a single pair and for a batch of slots stepped by one launch, the `cmap_step`, `cmap_render` and `tfilter_step` stage
times from eppm_stage_times, and the bytes each moves as a share of 8 TB/s.  The tool steps the same pair again and again, along which
a map would lose a few per cent of its pixels per step and the lost lanes would skip their gathers, so every timed map step starts from
the identity map loaded with eppm_cmap_set_state (not from an empty slot, whose step reads no map): all four map taps and all four
anchor taps of nearly every lane are read.  The step requests 73 B per pixel (4 frame + 8 flow + 1 mask
+ 4 x 8 map taps + 4 x 4 anchor taps read, 8 map + 4 frame written), the render 32 B (8 map + 4 frame + 4 x 4 layer taps read, 4
written); the taps of neighbouring lanes overlap, so HBM sees fewer (37 B and 20 B if every plane is fetched once).  One library per
process:

    python tools/cmap_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = {"cmap_step": (4 + 8 + 1 + 4 * 8 + 4 * 4 + 8 + 4, 4 + 8 + 1 + 8 + 4 + 8 + 4), "cmap_render": (8 + 4 + 4 * 4 + 4, 8 + 4 + 4 + 4),
         "tfilter_step": (4 + 8 + 1 + 4 * 16 + 16 + 4, 4 + 8 + 1 + 16 + 16 + 4)}          # (requested by the lanes, if every plane pixel is fetched once)


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
    from eppm_amd import io, synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "steps": a.steps, "batch": a.batch,
           "bytes_per_pixel": {k: v[0] for k, v in BYTES.items()}, "hbm_bytes_per_pixel": {k: v[1] for k, v in BYTES.items()}}

    def per_call(fn, n=a.steps):
        for _ in range(3):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def stages(ctx, obj, names, n=10, prep=None):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            if prep:
                prep()
            obj.step()
        ctx.synchronize()
        got = ctx.stage_times()
        ctx.enable_stage_timing(False)
        res = {}
        for name in names:
            ms = sorted(t for k, t in got if k == name)
            res[name] = ms[len(ms) // 2]
        return res

    def shares(name, ms, npx):
        req, hbm = BYTES[name]
        return {"requested_share_of_8TBs": req * npx / (ms * 1e-3) / 8e12, "hbm_share_of_8TBs": hbm * npx / (ms * 1e-3) / 8e12}

    def measure(ctx, sync, n_pairs, tag, bidir_steps):
        res = {}
        res[f"{tag}_bidir_dev_ms_per_pair"] = per_call(lambda: (ctx.compute_flow_bidirectional_device(), sync()), bidir_steps) / n_pairs
        cm = eppm_amd.CorrespondenceMap(ctx)
        seed = io.cmap_seed(h, w)

        def load():
            for k in range(n_pairs):
                cm.set_state(k, seed, pairs[k][0])
        total = 0.0
        for k in range(a.steps + 3):
            load()
            t0 = time.perf_counter()
            cm.step()
            sync()
            if k >= 3:
                total += time.perf_counter() - t0
        res[f"{tag}_step_and_render_dev_ms_per_pair"] = total * 1e3 / a.steps / n_pairs
        st = stages(ctx, cm, ("cmap_step", "cmap_render"), prep=load)
        res[f"{tag}_known_share_slot0"] = float(cm.known(0).mean())
        cm.close()
        flt = eppm_amd.TemporalFilter(ctx)
        flt.step()
        st.update(stages(ctx, flt, ("tfilter_step",)))
        flt.close()
        for name, ms in st.items():
            res[f"{tag}_{name}_stage_ms_per_pair"] = ms / n_pairs
            res[f"{tag}_{name}_share_of_bidir_dev"] = ms / n_pairs / res[f"{tag}_bidir_dev_ms_per_pair"]
            res[f"{tag}_{name}_bandwidth"] = shares(name, ms / n_pairs, h * w)
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
