"""What the pre-test of the two-phase random search rejects, from the CPU oracle: per PatchMatch iteration the
share of guesses 0 .. G-1 it rejects, the survivors per quarter-block workgroup (16x4 pixels x G guesses) and the instruction work of
the two-phase kernel relative to the one-phase kernel -- (G waves x rows/S + ceil(survivors / 64) waves) / G.  From it the centre rows
(EPPM_SEARCH_PRE_ROWS) and the threshold iteration (EPPM_SEARCH_PRE_FROM) can be re-derived for other shapes.  CPU only.

usage: search_pretest_stats.py [--rows N] [--eps E] [--blocks N] [--iters 0,1,2,3,5,9] [--pair synthetic|natural] [--height H --width W]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import search_pretest_model as M  # noqa: E402  (this folder)
from eppm_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--eps", type=float, default=2.0 ** -13)
    ap.add_argument("--blocks", type=int, default=80)
    ap.add_argument("--iters", default="0,1,2,3,5,9")
    ap.add_argument("--pair", default="synthetic", choices=["synthetic", "natural"])
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    a = ap.parse_args()
    img = synth.make_pair_cached(a.height, a.width, seed=1234)[:2] if a.pair == "synthetic" else synth.natural_pair(a.height, a.width)
    (i1, c1), (i2, c2) = [(p[0][2], p[1][2]) for p in (O.prepare(O.rgb2rgba(x)) for x in img)]          # level 2
    h, w = i1.shape
    P = (i1, i2, c1, c2)
    S, G = 10, 6
    rows_a = M.centre_rows((S - a.rows) // 2, a.rows)
    U = M.rest_weight(i1, rows_a)
    rng = np.random.default_rng(1)
    by, bx = np.divmod(rng.choice(((h + 3) // 4) * ((w + 15) // 16), a.blocks, replace=False), (w + 15) // 16)
    ys, xs = np.mgrid[0:4, 0:16]
    py = (by[:, None, None] * 4 + ys).reshape(-1)
    px = (bx[:, None, None] * 16 + xs).reshape(-1)
    blk = np.repeat(np.arange(a.blocks), 64)
    ok = (py < h) & (px < w)
    py, px, blk = py[ok], px[ok], blk[ok]
    print(f"{a.pair} {w}x{h} level 2, {a.blocks} quarter blocks, rows {rows_a}, eps {a.eps:g}")
    print("iters_done | rejected per guess | survivors per workgroup mean / max | work")
    for k in [int(v) for v in a.iters.split(",")]:
        nnf, cost = O.patchmatch(*P, iters_done=k)
        mx, my = nnf["x"][py, px].astype(np.int64), nnf["y"][py, px].astype(np.int64)
        surv = np.zeros(a.blocks, np.int64)
        rej_g = []
        for mag in M.search_windows(30, G):
            x0, x1 = np.maximum(mx - mag, 0), np.minimum(mx + mag + 1, w + 1)
            y0, y1 = np.maximum(my - mag, 0), np.minimum(my + mag + 1, h + 1)
            gx = x0 + rng.integers(0, 1 << 30, mx.shape) % (x1 - x0)
            gy = y0 + rng.integers(0, 1 << 30, my.shape) % (y1 - y0)
            N, D = M.centre_sums(*P, px, py, gx, gy, rows_a)
            rej = M.rejects(N, D, U[py, px], cost[py, px], a.eps) | ((gx == mx) & (gy == my))          # (the skip rule sits out too)
            rej_g.append(rej.mean())
            np.add.at(surv, blk, ~rej)
        work = (G * a.rows / S + np.ceil(surv / 64)).mean() / G
        print(f"{k:10d} | " + " ".join(f"{100 * r:5.1f}" for r in rej_g) + f" | {surv.mean():6.1f} / {surv.max():3d} | {work:.2f}")


if __name__ == "__main__":
    main()
