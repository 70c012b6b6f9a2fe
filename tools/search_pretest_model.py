"""The pre-test of the two-phase random search (csrc/pm_device.cuh: search_patch_centre_rows, rest_weight_term; csrc/k_pm_search.hip)
restated in numpy float32, operation for operation and in the kernel's order of additions: the rest-weight plane and the two centre-row
sums are compared with the kernels' bit for bit (tests/test_search_pretest_gpu.py).  Test infrastructure (tests/test_search_pretest_*.py)
and the statistics of tools/search_pretest_stats.py; needs the CPU oracle for fast_exp and the tables.

A patch cost is sum c_k w_k / sum w_k over the (R + 1)^2 samples; the pre-test forms both sums over a few centre rows A only, bounds the
rest of the weight sum by the rest-weight plane U (source image alone) and rejects a guess iff
    N (1 - eps) >= best (D_A + U)
in float32, where best is the pixel's stored cost."""
import numpy as np

S2 = np.float32(0.1) * np.float32(0.1)          # LAMBDA_AD^2 = PM_SIG_R^2


def _oracle():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import oracle
    return oracle


def fexp(arg):
    """oracle.fast_exp over an array, evaluated once per distinct value"""
    arg = np.asarray(arg, np.float32)
    u, inv = np.unique(arg, return_inverse=True)
    return _oracle().fast_exp(u)[inv.reshape(-1)].reshape(arg.shape)


def distances():
    """the 598 distinct L-inf distances of two unorm8 texels, as floats"""
    g = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    return np.unique(np.abs(g[:, None] - g[None, :]).astype(np.float32))


def data_term(d):
    """1 - exp(-d^2 / LAMBDA_AD^2): what the kernels read from the table (the same bits)"""
    d = np.asarray(d, np.float32)
    return (np.float32(1) - fexp(-(d * d) / S2)).astype(np.float32)


def channels(img):
    """uchar4 plane -> (h, w, 3) float32 of byte / 255"""
    rgb = np.stack([img["x"], img["y"], img["z"]], -1).astype(np.float32)
    return (rgb / np.float32(255)).astype(np.float32)


def _linf(a, b):
    return np.abs(a - b).max(-1).astype(np.float32)


def gsp(patch_r=9):
    gs, cn = _oracle().pm_luts(patch_r)
    k = np.abs(2 * np.arange(patch_r + 1) - patch_r)
    return (gs[k][None, :] * gs[k][:, None]).astype(np.float32), cn          # [ii][jj] = gs[|2jj - R|] * gs[|2ii - R|]


def centre_rows(row0, rows):
    return list(range(row0, row0 + rows))


def rest_weight(img1, rows_a, patch_r=9):
    """U[y, x] = sum, row major over the samples outside rows_a, of gsp_k fast_exp(-a2_k / s)"""
    R, S = patch_r, patch_r + 1
    g, _ = gsp(R)
    c = channels(img1)
    h, w = img1.shape
    ys, xs = np.mgrid[0:h, 0:w]
    u = np.zeros((h, w), np.float32)
    for ii in range(S):
        if ii in rows_a:
            continue
        sy = np.clip(ys + 2 * ii - R, 0, h - 1)
        for jj in range(S):
            a = _linf(c, c[sy, np.clip(xs + 2 * jj - R, 0, w - 1)])
            u = (u + (fexp(-(a * a) / S2) * g[ii, jj]).astype(np.float32)).astype(np.float32)
    return u


def centre_sums(img1, img2, c1, c2, px, py, gx, gy, rows_a, patch_r=9):
    """(N, D_A) of the guesses (gx, gy) of the pixels (px, py), 1-D integer arrays: the terms of patch_terms over rows_a, row major"""
    R, S = patch_r, patch_r + 1
    g, cn = gsp(R)
    A, B = channels(img1), channels(img2)
    h, w = img1.shape
    px, py, gx, gy = (np.asarray(v, np.int64) for v in (px, py, gx, gy))
    ca, cb = A[py, px], B[np.clip(gy, 0, h - 1), np.clip(gx, 0, w - 1)]
    pop = np.array([bin(v).count("1") for v in range(256)])
    N = np.zeros(len(px), np.float32)
    D = np.zeros(len(px), np.float32)
    for ii in rows_a:
        y1, y2 = np.clip(py + 2 * ii - R, 0, h - 1), np.clip(gy + 2 * ii - R, 0, h - 1)
        for jj in range(S):
            x1, x2 = np.clip(px + 2 * jj - R, 0, w - 1), np.clip(gx + 2 * jj - R, 0, w - 1)
            p1, p2 = A[y1, x1], B[y2, x2]
            cost = (data_term(_linf(p1, p2)) + cn[pop[c1[y1, x1] ^ c2[y2, x2]]]).astype(np.float32)
            a = _linf(ca, p1)
            t = _linf(cb, p2)
            wt = (fexp(-((a * a).astype(np.float32) + (t * t).astype(np.float32)) / S2) * g[ii, jj]).astype(np.float32)
            N = (N + (cost * wt).astype(np.float32)).astype(np.float32)
            D = (D + wt).astype(np.float32)
    return N, D


def rejects(N, D, U, best, eps):
    """the kernel's comparison, products in float32; NaN on either side: not rejected"""
    lhs = (N * (np.float32(1) - np.float32(eps))).astype(np.float32)
    rhs = (np.asarray(best, np.float32) * (D + U).astype(np.float32)).astype(np.float32)
    return lhs >= rhs


def search_windows(search_range=30, num_guess=6):
    """radius of the window of guess k: search_range halved k times while >= 1 (30, 15, 7, 3, 1, 1)"""
    out, mag = [], search_range
    for _ in range(num_guess):
        out.append(mag)
        if mag // 2 >= 1:
            mag //= 2
    return out
