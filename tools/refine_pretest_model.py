"""The two-phase form of the LDS-window candidate refine (csrc/k_c2f_refine.hip: k_c2f_refine_win<9>; csrc/c2f_device.cuh: c2f_rows2_win,
c2f_one_win) restated in numpy float32, operation for operation and in the kernel's order of additions.  Test
infrastructure (tests/test_refine_pretest_*.py); builds on tools/search_pretest_model.py (fast_exp, the data term, the rest weight) and
needs the CPU oracle for the tables.

A pixel has 9 candidates k = m * 3 + n (x offset m outer) around its truncated flow and 4 affine passes p (0: the plain grid); the cost of
(k, p) is cs / ws = sum c_t w_t / sum w_t over the 100 samples, and the refine keeps the first candidate with the strictly smallest
minimum over the passes.  Per coherent tile the kernel forms N = sum_A c_t w_t, D_A = sum_A w_t over the centre rows A of every valid
(k, p), the pixel's rest weight U, names k* = the candidate with the smallest min(N / D_A) over passes 1 and 0 (first index on ties),
evaluates k*'s four passes in full (B = their minimum) and rejects every other (k, p) iff, in float32 and by products,
    N (1 - eps) >= B (D_A + U)   and   B (D_A + U) >= rhsmin.
A tile with a valid pair whose D_A is not above dmin takes the one-phase loop instead.  A tile whose survivors (per pass, rounded up to
whole 64-item chunks) exceed the list's capacity is drained through that list in parts: the halves of its pixels (tile rows 0-7, 8-15) if
each fits, else the quarters (4 rows each), which always fit (tile_split, drain_in_parts); a library built with EPPM_C2F_PRE_PARTS = 0 sends
it to the one-phase loop."""
import numpy as np

import search_pretest_model as M

KC = np.array([[0.177, -0.011, -0.003, 0.301], [0.125, -0.357, 0.009, 0.308], [0.205, 0.370, 0.011, 0.296]], np.float32)


def _wrap(v):
    return ((v + 32768) % 65536) - 32768


def offsets(patch_r=9):
    """(dx, dy)[p][ii][jj]: integer offset of the target of sample (ii, jj) in pass p from the candidate (c2f_device.cuh: make_c2f_tables;
    pass 0 the plain grid)"""
    S = patch_r + 1
    j = (2 * np.arange(S) - patch_r).astype(np.float32)
    dx, dy = np.zeros((4, S, S), np.int64), np.zeros((4, S, S), np.int64)
    for p in range(4):
        for ii in range(S):
            i = np.float32(2 * ii - patch_r)
            fx = fy = np.zeros(S, np.float32)
            if p:
                a, b, c, d = KC[p - 1]
                fx = ((j * a).astype(np.float32) + np.float32(i * b)).astype(np.float32)
                fy = ((j * c).astype(np.float32) + np.float32(i * d)).astype(np.float32)
            dx[p, ii] = j.astype(np.int64) + np.floor(fx).astype(np.int64)
            dy[p, ii] = int(i) + np.floor(fy).astype(np.int64)
    return dx, dy


def centres(flow, w, h):
    """known, ccx, ccy per pixel: the truncated flow added to the pixel (c2f_centre), unknown above 1e9"""
    fx, fy = flow["x"].astype(np.float32), flow["y"].astype(np.float32)
    known = ~((fx > np.float32(1e9)) | (fy > np.float32(1e9)))
    ys, xs = np.mgrid[0:h, 0:w]

    def t(f):
        return np.clip(np.trunc(np.where(known, f, 0)), -32768, 32767).astype(np.int64)
    return known, _wrap(t(fx) + xs), _wrap(t(fy) + ys)


def pass_sums(planes, px, py, gx, gy, p, rows, patch_r=9):
    """(cs, ws) of pass p of the candidates (gx, gy) of the pixels (px, py) over the sample rows `rows`, row major: c2f_term's arithmetic"""
    img1, img2, c1, c2 = planes
    R, S = patch_r, patch_r + 1
    g, cn = M.gsp(R)
    A, B = M.channels(img1), M.channels(img2)
    h, w = img1.shape
    dx, dy = offsets(R)
    pop = np.array([bin(v).count("1") for v in range(256)])
    ca, cb = A[py, px], B[np.clip(gy, 0, h - 1), np.clip(gx, 0, w - 1)]
    cs, ws = np.zeros(len(px), np.float32), np.zeros(len(px), np.float32)
    for ii in rows:
        y1 = np.clip(py + 2 * ii - R, 0, h - 1)
        for jj in range(S):
            x1 = np.clip(px + 2 * jj - R, 0, w - 1)
            y2, x2 = np.clip(gy + dy[p, ii, jj], 0, h - 1), np.clip(gx + dx[p, ii, jj], 0, w - 1)
            p1, p2 = A[y1, x1], B[y2, x2]
            cost = (M.data_term(M._linf(p1, p2)) + cn[pop[c1[y1, x1] ^ c2[y2, x2]]]).astype(np.float32)
            a, t = M._linf(ca, p1), M._linf(cb, p2)
            wt = (M.fexp(-((a * a).astype(np.float32) + (t * t).astype(np.float32)) / M.S2) * g[ii, jj]).astype(np.float32)
            cs = (cs + (cost * wt).astype(np.float32)).astype(np.float32)
            ws = (ws + wt).astype(np.float32)
    return cs, ws


def rejects(N, D, U, B, eps, rhsmin):
    """the kernel's comparison, products in float32; NaN on either side: not rejected"""
    with np.errstate(all="ignore"):
        lhs = (N * (np.float32(1) - np.float32(eps))).astype(np.float32)
        rhs = (np.asarray(B, np.float32) * (D + U).astype(np.float32)).astype(np.float32)
        return (lhs >= rhs) & (rhs >= np.float32(rhsmin))


def centre_sums(planes, flow, rows_a, patch_r=9):
    """the pre-test alone: known, ccx, ccy, valid (9), N and D (4, 9), U -- what the kernel's probing instantiation stores"""
    img1 = planes[0]
    h, w = img1.shape
    known, ccx, ccy = centres(flow, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    valid = np.zeros((h, w, 9), bool)
    N, D = np.zeros((h, w, 4, 9), np.float32), np.zeros((h, w, 4, 9), np.float32)
    for k in range(9):
        cx, cy = _wrap(ccx + k // 3 - 1), _wrap(ccy + k % 3 - 1)
        valid[:, :, k] = known & (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        sel = np.nonzero(valid[:, :, k])
        for p in range(4):
            N[:, :, p, k][sel], D[:, :, p, k][sel] = pass_sums(planes, xs[sel], ys[sel], cx[sel], cy[sel], p, rows_a, patch_r)
    return dict(known=known, ccx=ccx, ccy=ccy, valid=valid, N=N, D=D, U=M.rest_weight(img1, rows_a, patch_r))


def refine(planes, flow, rows_a, eps, dmin, rhsmin, patch_r=9, exact_all=True):
    """The two-phase refine of every known pixel as if its tile were coherent.  Returns a dict of (h, w, ...) arrays: known, ccx, ccy,
    valid (9), N and D (4, 9), U, kstar (15: no valid candidate), B, tested and rej (4, 9), small (a valid pair with D_A <= dmin), cost
    (4, 9: the exact cost, NaN where not evaluated; only k* and the survivors unless exact_all), best (the selected candidate index)."""
    img1 = planes[0]
    h, w = img1.shape
    S = patch_r + 1
    known, ccx, ccy = centres(flow, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    U = M.rest_weight(img1, rows_a, patch_r)
    valid = np.zeros((h, w, 9), bool)
    N, D = np.zeros((h, w, 4, 9), np.float32), np.zeros((h, w, 4, 9), np.float32)
    cost = np.full((h, w, 4, 9), np.nan, np.float32)
    cxs = [_wrap(ccx + k // 3 - 1) for k in range(9)]
    cys = [_wrap(ccy + k % 3 - 1) for k in range(9)]
    for k in range(9):
        valid[:, :, k] = known & (cxs[k] >= 0) & (cxs[k] < w) & (cys[k] >= 0) & (cys[k] < h)
        sel = np.nonzero(valid[:, :, k])
        for p in range(4):
            n_, d_ = pass_sums(planes, xs[sel], ys[sel], cxs[k][sel], cys[k][sel], p, rows_a, patch_r)
            N[:, :, p, k][sel], D[:, :, p, k][sel] = n_, d_
    valid4 = np.repeat(valid[:, :, None, :], 4, 2)
    small = (valid4 & ~(D > np.float32(dmin))).any((2, 3))
    with np.errstate(all="ignore"):
        est = np.minimum(N[:, :, 1] / D[:, :, 1], N[:, :, 0] / D[:, :, 0])          # group 1's passes: 1 and 0
    est = np.where(valid & ~np.isnan(est), est, np.inf)
    kstar = np.where(valid.any(2), np.argmin(est, 2), 15)                           # argmin: the first index on ties
    live = kstar != 15
    is_star = np.arange(9)[None, None, :] == kstar[:, :, None]

    def evaluate(need):
        for k in range(9):
            for p in range(4):
                sel = np.nonzero(need[:, :, p, k] & valid[:, :, k] & np.isnan(cost[:, :, p, k]))
                if len(sel[0]):
                    cs, ws = pass_sums(planes, xs[sel], ys[sel], cxs[k][sel], cys[k][sel], p, range(S), patch_r)
                    with np.errstate(all="ignore"):
                        cost[:, :, p, k][sel] = (cs / ws).astype(np.float32)
    evaluate(valid4 if exact_all else np.repeat(is_star[:, :, None, :], 4, 2))
    with np.errstate(all="ignore"):
        B = np.where(is_star[:, :, None, :], cost, np.inf).min((2, 3)).astype(np.float32)          # no cost of a tile that is not small is NaN
    tested = valid4 & live[:, :, None, None] & ~is_star[:, :, None, :]
    rej = tested & rejects(N, D, U[:, :, None, None], B[:, :, None, None], eps, rhsmin)
    if not exact_all:
        evaluate(tested & ~rej)
    # selection over k* and the survivors: the smallest cost, then the smallest index
    c = np.where(rej | ~valid4 | np.isnan(cost), np.inf, cost).min(2)
    best = np.where(live, np.argmin(c, 2), 4)
    return dict(known=known, ccx=ccx, ccy=ccy, valid=valid, N=N, D=D, U=U, kstar=kstar, B=B, rej=rej, tested=tested, small=small, cost=cost,
                best=best)


def flow_of_best(r):
    """the refined flow the selection `best` stands for: (bx - x, by - y) at known pixels, 0 at unknown ones"""
    h, w = r["best"].shape
    ys, xs = np.mgrid[0:h, 0:w]
    fx = np.where(r["known"], _wrap(r["ccx"] + r["best"] // 3 - 1) - xs, 0).astype(np.float32)
    fy = np.where(r["known"], _wrap(r["ccy"] + r["best"] % 3 - 1) - ys, 0).astype(np.float32)
    return fx, fy


def quarter_survivors(r, tile):
    """(4, 4) survivors of a tile = (slice, slice) by [quarter of its pixels: 4 tile rows, one wave per pass group][pass]"""
    s = np.zeros((16, 16, 4, 9), bool)
    v = (r["tested"][tile] & ~r["rej"][tile])
    s[:v.shape[0], :v.shape[1]] = v
    return s.reshape(4, 4, 16, 4, 9).sum((1, 2, 4))


def tile_split(qs, cap):
    """parts (1, 2 or 4) in which the kernel drains a tile with the survivors qs = quarter_survivors(): the coarsest split whose every
    part fits the list, one segment of whole 64-item chunks per pass"""
    def fits(q0, q1):
        return int(((qs[q0:q1].sum(0) + 63) // 64).sum()) * 64 <= cap
    if fits(0, 4):
        return 1
    return 2 if fits(0, 2) and fits(2, 4) else 4


def drain_in_parts(r, tile, nparts, cap=None):
    """The kernel's steps 4 and 5 for one tile = (slice, slice) of a refine(...) whose survivors' costs are known: the survivors go through
    the list part by part -- per part one list per pass, pixels in tile order, a pixel's candidates in index order --, every item lowers its
    pixel's 64-bit key (bits(cost) << 4) | k, seeded with k*'s (bits(B) << 4) | k*.  Returns (the selected candidate per pixel, 4 where a
    pixel has no valid candidate, and the largest number of list items a part needed); cap: assert that every part fits."""
    kstar, B = r["kstar"][tile], r["B"][tile]
    th, tw = kstar.shape
    key = np.where(kstar != 15, (B.view(np.uint32).astype(np.uint64) << np.uint64(4)) | kstar.astype(np.uint64), np.uint64(15))
    surv, cost = r["tested"][tile] & ~r["rej"][tile], r["cost"][tile]
    rows, most = 16 // nparts, 0
    for part in range(nparts):
        lists = [[(y, x, k) for y in range(part * rows, min((part + 1) * rows, th)) for x in range(tw) for k in range(9) if surv[y, x, p, k]]
                 for p in range(4)]
        items = sum((len(li) + 63) // 64 for li in lists) * 64
        most = max(most, items)
        assert cap is None or items <= cap, (part, nparts, items, cap)
        for p in range(4):
            for y, x, k in lists[p]:
                c = cost[y, x, p, k]
                assert not np.isnan(c)
                key[y, x] = min(key[y, x], (np.uint64(np.float32(c).view(np.uint32)) << np.uint64(4)) | np.uint64(k))
    best = (key & np.uint64(15)).astype(np.int64)
    return np.where(best == 15, 4, best), most


def tile_paths(r, span_x, span_y, cap, parts=False):
    """what k_c2f_refine_win<9> counts over one launch: tiles two-phase with one list, tiles with a weight sum too small, tiles whose
    survivors exceed one list, other tiles (incoherent or without a known pixel), pairs tested, pairs rejected; parts: and the tiles of the
    third kind drained in halves, in quarters"""
    h, w = r["best"].shape
    out = [0, 0, 0, 0, 0, 0, 0, 0]
    for y0 in range(0, h, 16):
        for x0 in range(0, w, 16):
            t = (slice(y0, y0 + 16), slice(x0, x0 + 16))
            kn = r["known"][t]
            if not kn.any():
                out[3] += 1
                continue
            cx, cy = r["ccx"][t][kn], r["ccy"][t][kn]
            if cx.max() - cx.min() > span_x or cy.max() - cy.min() > span_y:
                out[3] += 1
                continue
            if r["small"][t].any():
                out[1] += 1
                continue
            out[4] += int(r["tested"][t].sum())
            out[5] += int(r["rej"][t].sum())
            surv = (r["tested"][t] & ~r["rej"][t]).sum((0, 1, 3))          # per pass
            split = tile_split(quarter_survivors(r, t), cap)
            assert (split == 1) == (int(((surv + 63) // 64).sum()) * 64 <= cap)
            out[0 if split == 1 else 2] += 1
            if split != 1:
                out[6 if split == 2 else 7] += 1
    return tuple(out if parts else out[:6])
