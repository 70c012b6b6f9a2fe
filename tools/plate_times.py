"""Cost of one step and one render of a background plate next to the bidirectional call they follow and next to
the temporal filter's step (section 15), a neighbour of similar traffic, in one process: the `plate_fit`, `plate_block`,
`plate_accumulate` and `plate_render` stage times from eppm_stage_times for a single pair and for a batch of slots stepped by one
sequence of launches, `tfilter_step` measured in the same run, and per stage the bytes it moves -- as the lanes request them and as HBM
sees them if every byte is fetched once -- as a share of 8 TB/s.  Every step starts from the identity path, so that the whole canvas is
sampled.  One library per process:

    python tools/plate_times.py [--lib exact|tol] [--steps N] [--batch B] [--width W --height H] [--margin MX MY]

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
ITERS = 3
# bytes per pixel, (requested by the lanes, HBM if every byte is fetched once); frame pixels except where noted
BYTES = {
    "plate_fit": (ITERS * (8 + 1) + (8 + 1 + 16 + 4 + 1), ITERS * (8 + 1) + (8 + 1 + 4 + 4 + 1)),       # 3 x (flow, occ1) + the warp launch
    "plate_block": (1 + 1, 1 + 1),                                # mask in (the halo re-reads of a tile come from L2), blocked plane out
    "plate_accumulate": (16 + 4 + 16 + 16, 4 + 1 + 16 + 16),     # per CANVAS pixel: 4 image taps, 4 blocked bytes, the state in and out
    "plate_render": (4 + 1 + 4 + 1, 4 + 1 + 4 + 1),              # image, blocked byte, word and fill byte; the 4 x 16 B canvas taps of blocked pixels on top
    "tfilter_step": (4 + 8 + 1 + 4 * 16 + 16 + 4, 4 + 8 + 1 + 16 + 16 + 4),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="exact", choices=["exact", "tol"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--margin", type=int, nargs=2, default=(0, 0), metavar=("MX", "MY"))
    a = ap.parse_args()
    import eppm_amd
    eppm_amd.select_library("tol" if a.lib == "tol" else "")
    from eppm_amd import synth
    from eppm_amd._lib import lib
    h, w = a.height, a.width
    mx, my = a.margin
    cpx, px = (h + 2 * my) * (w + 2 * mx), h * w
    pairs = [synth.make_pair_cached(h, w, seed=1234 + k)[:2] for k in range(a.batch)]
    out = {"library": lib().eppm_version().decode(), "size": [w, h], "canvas": [w + 2 * mx, h + 2 * my], "steps": a.steps, "batch": a.batch,
           "launches_per_step": 2 * ITERS + 1 + 4, "bytes_per_pixel": {k: {"requested": r, "hbm": m} for k, (r, m) in BYTES.items()}}

    def per_call(fn, n):
        for _ in range(2):
            fn()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    def median_stages(ctx, fn, names, n):
        ctx.enable_stage_timing(True)
        ctx.stage_times()
        for _ in range(n):
            fn()
        ctx.synchronize()
        got = ctx.stage_times()
        ctx.enable_stage_timing(False)
        res = {}
        for name in names:
            ms = sorted(t for k, t in got if k == name)
            res[name] = ms[len(ms) // 2]
        return res

    def measure(ctx, n_pairs, tag, bidir_steps):
        res = {f"{tag}_bidir_dev_ms_per_pair": per_call(lambda: (ctx.compute_flow_bidirectional_device(), ctx.synchronize()), bidir_steps) / n_pairs}
        pl = eppm_amd.BackgroundPlate(ctx, margin_x=mx, margin_y=my)

        def step():
            for s in range(n_pairs):
                pl.set_path(s, IDENT)
            pl.step()
        step()
        st = median_stages(ctx, step, ("plate_fit", "plate_block", "plate_accumulate"), a.steps)
        st.update(median_stages(ctx, lambda: pl.render(0), ("plate_render",), a.steps))
        st["plate_render"] *= n_pairs          # a render covers one slot: scaled, so that the division below leaves one slot's time
        res[f"{tag}_coverage_slot0"] = float((pl.coverage(0) >= 1).mean())
        res[f"{tag}_fill_slot0"] = {str(k): float((pl.render(0)[1] == k).mean()) for k in (0, 1, 2)}
        pl.close()
        flt = eppm_amd.TemporalFilter(ctx)
        flt.step()
        st.update(median_stages(ctx, flt.step, ("tfilter_step",), a.steps))
        flt.close()
        for name, ms in st.items():
            one = ms / n_pairs
            n_px = cpx if name == "plate_accumulate" else px
            res[f"{tag}_{name}"] = {"stage_ms_per_pair": one, "share_of_bidir_dev": one / res[f"{tag}_bidir_dev_ms_per_pair"],
                                    "requested_MB": BYTES[name][0] * n_px / 1e6, "hbm_MB": BYTES[name][1] * n_px / 1e6,
                                    "requested_share_of_8TBs": BYTES[name][0] * n_px / (one * 1e-3) / 8e12,
                                    "hbm_share_of_8TBs": BYTES[name][1] * n_px / (one * 1e-3) / 8e12}
        return res

    e = eppm_amd.EPPM()
    e.init(pairs[0][0], pairs[0][1], h, w)
    out.update(measure(e, 1, "single", max(3, a.steps // 4)))
    e.close()
    b = eppm_amd.EPPMBatch(h, w, a.batch)
    b.set_data(pairs)
    out.update(measure(b, a.batch, "batch", 3))
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
