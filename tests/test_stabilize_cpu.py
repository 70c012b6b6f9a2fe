"""CPU tests of global camera-motion estimation and video stabilisation: a numpy restatement of 16.2 - 16.4 (Python
integers for the sums, Python floats -- float64, one rounding per operation -- for the solve and the path update, float32 arrays for the
residual and the warp) against the host forms eppm_gmotion_fit_host / eppm_stab_update_host / eppm_stab_warp_host bit for bit on the shared
generator stab_cases() (the GPU tests run the kernels on the same cases), the ABI's argument checks, and what the feature means: the
background motion of a scene with an independently moving rectangle, tripod lock, pass-through and degenerate frames."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import eppm_amd
from eppm_amd import _lib, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # (no conftest import: stabilize_tol_child.py imports this module)

F = np.float32
ARG = 1
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


# ---- the numpy restatement of section 16 ----

def centred(h, w):
    """doubled centred integer coordinates as (h, w) int64 planes"""
    X = 2 * np.arange(w, dtype=np.int64) - (w - 1)
    Y = 2 * np.arange(h, dtype=np.int64) - (h - 1)
    return np.broadcast_to(X[None, :], (h, w)), np.broadcast_to(Y[:, None], (h, w))


def np_valid(u, v, occ):
    with np.errstate(all="ignore"):
        known = (np.abs(u) <= F(1e9)) & (np.abs(v) <= F(1e9))
        return (occ == 0) & known & (np.abs(u) <= F(8192)) & (np.abs(v) <= F(8192))


def np_inlier(u, v, X, Y, pf, tau2):
    Xf, Yf = X.astype(F), Y.astype(F)
    with np.errstate(all="ignore"):
        ru = u - ((pf[0] + pf[1] * Xf) + pf[2] * Yf)
        rv = v - ((pf[3] + pf[4] * Xf) + pf[5] * Yf)
        assert ru.dtype == F and rv.dtype == F
        return (ru * ru + rv * rv) <= tau2


def isum(a):
    """an exact Python integer: int64 row sums (no row of a frame of at most 8192 x 8192 overflows), added as Python integers"""
    return sum(int(r) for r in a.sum(axis=1, dtype=np.int64))


def np_solve(s):
    """the model of twelve integer sums: (p[6] as Python floats, valid)"""
    n, sx, sy, sxx, sxy, syy = (float(x) for x in s[:6])
    c00 = sxx * syy - sxy * sxy
    c01 = sxy * sy - sx * syy
    c02 = sx * sxy - sxx * sy
    c11 = n * syy - sy * sy
    c12 = sx * sy - n * sxy
    c22 = n * sxx - sx * sx
    det = (n * c00 + sx * c01) + sy * c02
    if not (s[0] >= 3 and det > 1e-6 * ((n * sxx) * syy)):
        return [0.0] * 6, 0
    p = []
    for k in range(2):
        b0, b1, b2 = float(s[6 + 3 * k]) / 256.0, float(s[7 + 3 * k]) / 256.0, float(s[8 + 3 * k]) / 256.0
        p.append(((c00 * b0 + c01 * b1) + c02 * b2) / det)
        p.append(((c01 * b0 + c11 * b1) + c12 * b2) / det)
        p.append(((c02 * b0 + c12 * b1) + c22 * b2) / det)
    return p, 1


def np_fit(u, v, occ, tau, iters):
    """16.2: (model dict, mask)"""
    h, w = u.shape
    X, Y = centred(h, w)
    valid = np_valid(u, v, occ)
    tau2 = F(tau) * F(tau)
    with np.errstate(all="ignore"):
        qu = np.rint(np.where(valid, u, F(0)) * F(256)).astype(np.int64)
        qv = np.rint(np.where(valid, v, F(0)) * F(256)).astype(np.int64)
    m = dict(p=[0.0] * 6, n_valid=0, n_inliers=0, valid=0, passes=0)
    pf = np.zeros(6, F)
    for k in range(iters):
        if k > 0 and not m["valid"]:
            break
        use = valid if k == 0 else valid & np_inlier(u, v, X, Y, pf, tau2)
        g = use.astype(np.int64)
        s = [isum(g), isum(g * X), isum(g * Y), isum(g * X * X), isum(g * X * Y), isum(g * Y * Y),
             isum(g * qu), isum(g * X * qu), isum(g * Y * qu), isum(g * qv), isum(g * X * qv), isum(g * Y * qv)]
        assert max(abs(x) for x in s) < 2 ** 60
        m["p"], m["valid"] = np_solve(s)
        if k == 0:
            m["n_valid"] = s[0]
        m["n_inliers"] = s[0]
        m["passes"] = k + 1
        pf = np.array(m["p"], np.float64).astype(F)
    mask = np.full((h, w), 2, np.uint8)
    mask[valid] = 1
    if m["valid"]:
        mask[valid & np_inlier(u, v, X, Y, pf, tau2)] = 0
    m["p"] = np.array(m["p"], np.float64)
    return m, mask


def np_update(c, s, counts, p, valid, smooth, cut):
    """16.3: (C, S, counts, wf); c, s: six Python floats each (the identity for an empty slot)"""
    c, s = [float(x) for x in c], [float(x) for x in s]
    frames, bad = counts
    zero = np.zeros(6, F)
    if cut:
        return list(IDENT), list(IDENT), (0, 0), zero
    p = [float(x) for x in p]
    if valid:
        m00, m01, m10, m11 = 1.0 + 2.0 * p[1], 2.0 * p[2], 2.0 * p[4], 1.0 + 2.0 * p[5]
        c = [m00 * c[0] + m01 * c[2], m00 * c[1] + m01 * c[3], m10 * c[0] + m11 * c[2], m10 * c[1] + m11 * c[3],
             (m00 * c[4] + m01 * c[5]) + p[0], (m10 * c[4] + m11 * c[5]) + p[3]]
    else:
        bad += 1
    frames += 1
    a = float(F(smooth))
    b = 1.0 - a
    with np.errstate(all="ignore"):
        s = [float(np.float64(a) * np.float64(s[k]) + np.float64(b) * np.float64(c[k])) for k in range(6)]
        det = float(np.float64(s[0]) * np.float64(s[3]) - np.float64(s[1]) * np.float64(s[2]))
        if not (abs(det) > 1e-6):
            return list(IDENT), list(IDENT), (0, 0), zero
        D = np.float64
        i00, i01, i10, i11 = D(s[3]) / D(det), D(-s[1]) / D(det), D(-s[2]) / D(det), D(s[0]) / D(det)
        d00, d01, d10, d11 = D(c[0]) - D(s[0]), D(c[1]) - D(s[1]), D(c[2]) - D(s[2]), D(c[3]) - D(s[3])
        e00, e01 = d00 * i00 + d01 * i10, d00 * i01 + d01 * i11
        e10, e11 = d10 * i00 + d11 * i10, d10 * i01 + d11 * i11
        wx = (D(c[4]) - D(s[4])) - (e00 * D(s[4]) + e01 * D(s[5]))
        wy = (D(c[5]) - D(s[5])) - (e10 * D(s[4]) + e11 * D(s[5]))
        wf = np.array([wx, e00 / D(2), e01 / D(2), wy, e10 / D(2), e11 / D(2)], np.float64).astype(F)
    return c, s, (frames, bad), wf


def np_warp(wf, img2):
    """16.4: the (h, w, 3) output bytes"""
    h, w, _ = img2.shape
    X, Y = centred(h, w)
    Xf, Yf = X.astype(F), Y.astype(F)
    wf = np.asarray(wf, F)
    with np.errstate(all="ignore"):
        qx = np.arange(w, dtype=F)[None, :] + ((wf[0] + wf[1] * Xf) + wf[2] * Yf)
        qy = np.arange(h, dtype=F)[:, None] + ((wf[3] + wf[4] * Xf) + wf[5] * Yf)
        assert qx.dtype == F and qy.dtype == F
        inside = (qx >= F(0)) & (qx <= F(w - 1)) & (qy >= F(0)) & (qy <= F(h - 1))
        qx, qy = np.where(inside, qx, F(0)), np.where(inside, qy, F(0))
        x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (qx - x0.astype(F))[..., None], (qy - y0.astype(F))[..., None]
        bx, by = F(1) - ax, F(1) - ay
        img = img2.astype(F)
        val = by * (bx * img[y0, x0] + ax * img[y0, x1]) + ay * (bx * img[y1, x0] + ax * img[y1, x1])
        assert val.dtype == F
        out = np.floor(np.fmin(np.fmax(val, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    out[~inside] = 0
    return out


# ---- the shared cases ----

# w x h.  520 x 130 has 9 x 9 = 81 accumulate blocks of 64 x 16 pixels per slot: more than the solve kernel's 64 lanes, so some lanes add two slabs
SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157), (520, 130)]
# (flow, tau, iters, smooth, state, cut)
CONFIGS = [("affine", 1.0, 3, 0.9, "empty", False), ("rect", 1.0, 3, 0.9, "stepped", False), ("rect", 1.0, 8, 1.0, "empty", False),
           ("special", 0.25, 3, 0.0, "stepped", False), ("special", 1e9, 1, 0.9, "empty", False), ("special", 1.0, 8, 0.9, "stepped", True),
           ("allmasked", 1.0, 3, 0.9, "stepped", False), ("onerow", 1.0, 3, 0.9, "stepped", False), ("noinlier", 0.25, 3, 0.9, "empty", False),
           ("affine", 0.25, 1, 1.0, "singular", False), ("zero", 1.0, 1, 1.0, "last", False), ("zero", 1.0, 1, 1.0, "ulp", False),
           ("zero", 1.0, 1, 1.0, "shift", False), ("affine", 1.0, 3, 0.9, "empty", True)]
TRUE_P = (1.75, 2.5e-3, -1.5e-3, -0.625, 1e-3, 3e-3)          # the background of the affine and rectangle cases, displacement form


def affine_field(h, w, p=TRUE_P):
    X, Y = centred(h, w)
    u = p[0] + p[1] * X + p[2] * Y
    v = p[3] + p[4] * X + p[5] * Y
    return u.astype(F), v.astype(F)


def rectangle(h, w):
    """about 20 % of the area: 40 % of the columns by 50 % of the rows, off the centre"""
    rw, rh = max(1, round(0.4 * w)), max(1, round(0.5 * h))
    x0, y0 = min(w - rw, int(0.55 * w)), min(h - rh, int(0.3 * h))
    r = np.zeros((h, w), bool)
    r[y0:y0 + rh, x0:x0 + rw] = True
    return r


def _flow(kind, rng, h, w):
    u, v = affine_field(h, w)
    occ = np.where(rng.random((h, w)) < 0.7, 0, rng.integers(0, 4, (h, w))).astype(np.uint8)          # bytes 0..3, zero most often
    if kind == "rect":
        r = rectangle(h, w)
        u, v = np.where(r, u + F(4), u).astype(F), np.where(r, v - F(3), v).astype(F)
        occ = np.where(rng.random((h, w)) < 0.95, 0, rng.integers(1, 4, (h, w))).astype(np.uint8)
    elif kind == "special":
        up = np.nextafter(F(8192), F(np.inf))
        half = ((rng.integers(-2000, 2000, (h, w)) + 0.5) / 256.0).astype(F)          # u * 256 exactly half-way
        special = [F(8192), F(-8192), up, -up, F(1e10), F(-1e10), F(np.inf), F(-np.inf), F(np.nan), F(-0.0), F(1e-45), F(-1e-40), half, half]
        kind_u, kind_v = rng.integers(0, 60, (h, w)), rng.integers(0, 60, (h, w))
        for k, val in enumerate(special):
            u = np.where(kind_u == k, val, u).astype(F)
            v = np.where(kind_v == k, val, v).astype(F)
    elif kind == "allmasked":
        occ = rng.integers(1, 4, (h, w)).astype(np.uint8)
    elif kind == "onerow":
        keep = np.zeros((h, w), bool)
        keep[h // 2] = True
        occ = np.where(keep, 0, 1).astype(np.uint8)
    elif kind == "noinlier":          # +-100 px in a checkerboard: the first model is near 0 and nothing is within tau of it
        ys, xs = np.mgrid[0:h, 0:w]
        u = np.where((xs + ys) % 2 == 0, F(100), F(-100)).astype(F)
        v = (-u).astype(F)
        occ = np.zeros((h, w), np.uint8)
    elif kind == "zero":
        u, v = np.zeros((h, w), F), np.zeros((h, w), F)
        occ = np.zeros((h, w), np.uint8)
    return u, v, occ


def _state(kind, rng, h, w, smooth):
    """(C, S) of the slot before the step, or None for an empty slot"""
    if kind == "empty":
        return None
    if kind == "stepped":          # three updates of the restatement
        c, s, n = list(IDENT), list(IDENT), (0, 0)
        for _ in range(3):
            p = rng.uniform(-1, 1, 6) * np.array([5, 2e-3, 2e-3, 5, 2e-3, 2e-3])
            c, s, n, _ = np_update(c, s, n, p, 1, smooth, False)
        return c, s
    if kind == "singular":         # det S = 0, and smooth = 1 keeps it: the cut rule
        return [1.0, 0.25, 0.0, 1.0, 3.0, -2.0], [1.0, 2.0, 0.5, 1.0, 0.0, 0.0]
    if kind == "last":             # with the zero flow and smooth = 1 the warp is C: pixel (0, 0) samples the last column and row exactly
        return [1.0, 0.0, 0.0, 1.0, float(w - 1), float(h - 1)], list(IDENT)
    if kind == "ulp":              # ... and one ulp outside them
        return [1.0, 0.0, 0.0, 1.0, float(np.nextafter(F(w - 1), F(np.inf))), float(np.nextafter(F(h - 1), F(np.inf)))], list(IDENT)
    if kind == "shift":            # a fractional shift with a small rotation and zoom
        return [1.01, 0.02, -0.02, 0.99, min(2.5, (w - 1) / 2), -min(1.25, (h - 1) / 2)], list(IDENT)
    raise ValueError(kind)


def restate(c):
    """the restatement's results of one case: model, mask, paths, counts, warp, frame"""
    m, mask = np_fit(c["u"], c["v"], c["occ"], c["tau"], c["iters"])
    C0, S0 = c["path"] if c["path"] is not None else (IDENT, IDENT)
    Cn, Sn, counts, wf = np_update(C0, S0, (0, 0), m["p"], m["valid"], c["smooth"], c["cut"])
    return dict(want_model=m, want_mask=mask, want_C=np.array(Cn, np.float64), want_S=np.array(Sn, np.float64), want_counts=counts,
                want_wf=wf, want_rgb=np_warp(wf, c["img2"]))


@functools.lru_cache(maxsize=None)
def stab_cases():
    return _build(SIZES, CONFIGS, 1600)


# Thin frames at kGmMaxDim: centred coordinates up to +-4095.5 in gm_X / gm_Y, 256 and 512 slabs (four and eight trips of the solve
# kernel's loop over 64 lanes), warps that sample the last column and row at 8191; pad: pixels beyond every row of the caller's image
LIMIT_SIZES = [(8192, 20), (20, 8192)]
LIMIT_CONFIGS = [CONFIGS[k] for k in (0, 1, 3, 5, 8, 10, 11, 12)]


@functools.lru_cache(maxsize=None)
def stab_limit_cases():
    return [dict(c, pad=(0, 5, 64)[k % 3]) for k, c in enumerate(_build(LIMIT_SIZES, LIMIT_CONFIGS, 9600))]


def _build(sizes, configs, seed):
    cases = []
    for si, (w, h) in enumerate(sizes):
        for ci, (kind, tau, iters, smooth, state, cut) in enumerate(configs):
            rng = np.random.default_rng(seed + 100 * si + ci)
            u, v, occ = _flow(kind, rng, h, w)
            c = dict(name=f"{w}x{h}-{ci}-{kind}-{state}", w=w, h=h, kind=kind, tau=tau, iters=iters, smooth=smooth, state=state, cut=cut,
                     u=u, v=v, occ=occ, img2=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), path=_state(state, rng, h, w, smooth))
            c.update(restate(c))
            if kind == "rect" and h * w >= 64:          # the generator's condition: both classes are well populated after the final pass
                share0, share1 = (c["want_mask"] == 0).mean(), (c["want_mask"] == 1).mean()
                assert c["want_model"]["valid"] and share0 >= 0.1 and share1 >= 0.1, (c["name"], share0, share1)
            cases.append(c)
    return cases


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_model(got, want):
    return same_bits(got["p"], want["p"]) and all(int(got[k]) == int(want[k]) for k in ("n_valid", "n_inliers", "valid", "passes"))


def host_step(c):
    """one case through the host forms: what restate() returns, with got_ keys"""
    m, mask = io.gmotion_fit_host(c["u"], c["v"], c["occ"], c["tau"], c["iters"])
    C0, S0 = c["path"] if c["path"] is not None else io.stab_identity()
    Cn, Sn, wf, counts = io.stab_update_host(C0, S0, m, c["smooth"], c["cut"])
    return dict(model=m, mask=mask, C=Cn, S=Sn, counts=counts, wf=wf, rgb=io.stab_warp_host(wf, c["img2"]))


def differences(c, got):
    """the names of what differs from the restatement, bit for bit"""
    bad = []
    if not same_model(got["model"], c["want_model"]):
        bad.append("model")
    if not np.array_equal(got["mask"], c["want_mask"]):
        bad.append("mask")
    if not (same_bits(got["C"], c["want_C"]) and same_bits(got["S"], c["want_S"]) and tuple(got["counts"]) == tuple(c["want_counts"])):
        bad.append("path")
    if "wf" in got and not np.array_equal(np.asarray(got["wf"], F).view(np.uint32), c["want_wf"].view(np.uint32)):
        bad.append("wf")
    if not np.array_equal(got["rgb"], c["want_rgb"]):
        bad.append("frame")
    return bad


# ---- the host forms equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_forms_equal_the_restatement(size):
    cases = [c for c in stab_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) == len(CONFIGS)
    bad = [(c["name"], d) for c in cases for d in [differences(c, host_step(c))] if d]
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_host_forms_equal_the_restatement_at_the_size_limit(size):
    w, h = LIMIT_SIZES[size]
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "gmotion.h")).read()
    assert max(w, h) == int(re.search(r"constexpr int kGmMaxDim = (\d+);", src).group(1))
    assert not io_size_ok(h + (h > w), w + (w > h))          # one more along the long side is refused
    cases = [c for c in stab_limit_cases() if (c["w"], c["h"]) == (w, h)]
    assert len(cases) == len(LIMIT_CONFIGS) and {c["pad"] for c in cases} == {0, 5, 64}
    bad = [(c["name"], d) for c in cases for d in [differences(c, host_step(c))] if d]
    assert not bad, bad
    for c in cases:
        if c["state"] == "last":       # the warp's tap at (8191, 19) / (19, 8191): the closed side of the frame test
            assert np.array_equal(c["want_rgb"][0, 0], c["img2"][-1, -1]) and int(c["want_rgb"].astype(bool).any(axis=2).sum()) <= 1
        if c["state"] == "ulp":
            assert not c["want_rgb"].any()
        if c["state"] == "shift":
            assert c["want_rgb"][:, -1].any() or c["want_rgb"][-1].any()
        if c["kind"] in ("affine", "rect") and not c["cut"]:
            assert c["want_model"]["valid"] and 0 in c["want_mask"][:, 0] and 0 in c["want_mask"][:, -1] and 0 in c["want_mask"][0] and 0 in c["want_mask"][-1]


def io_size_ok(h, w):
    """whether the fit's host form accepts a frame of this size"""
    try:
        io.gmotion_fit_host(np.zeros((h, w), F), np.zeros((h, w), F), np.ones((h, w), np.uint8))
    except eppm_amd.EppmError:
        return False
    return True


def test_the_cases_cover_what_they_claim():
    cases = stab_cases()
    big = [c for c in cases if c["h"] * c["w"] >= 64]
    by = lambda kind: [c for c in big if c["kind"] == kind]          # noqa: E731
    assert all(c["want_model"]["valid"] == 0 and c["want_model"]["passes"] == 1 and c["want_model"]["n_valid"] == 0 for c in by("allmasked"))
    assert all((c["want_mask"] == 2).all() for c in by("allmasked"))
    assert all(c["want_model"]["valid"] == 0 and c["want_model"]["n_valid"] == c["w"] for c in by("onerow"))
    assert all(set(np.unique(c["want_mask"])) == {1, 2} for c in by("onerow"))
    for c in by("noinlier"):           # the first pass has a model, the second no pixel
        m = c["want_model"]
        assert m["passes"] == 2 and m["n_inliers"] == 0 and m["valid"] == 0 and m["n_valid"] == c["h"] * c["w"] and (c["want_mask"] == 1).all()
    for c in by("special"):
        assert 2 in c["want_mask"] and np.isnan(c["u"]).any() and np.isinf(c["v"]).any()
        q = c["u"][np.isfinite(c["u"])].astype(np.float64) * 256
        assert (np.abs(q - np.floor(q)) == 0.5).any()          # half-way quantisation
    assert set(np.unique(np.concatenate([c["want_mask"].ravel() for c in by("special")]))) == {0, 1, 2}
    for c in cases:
        if c["state"] == "singular" or c["cut"]:
            assert same_bits(c["want_C"], IDENT) and same_bits(c["want_S"], IDENT) and np.array_equal(c["want_rgb"], c["img2"]), c["name"]
        if c["state"] == "last":       # pixel (0, 0) is the last pixel of the frame, every other one is outside
            assert np.array_equal(c["want_rgb"][0, 0], c["img2"][-1, -1]) and int(c["want_rgb"].astype(bool).any(axis=2).sum()) <= 1
        if c["state"] == "ulp":
            assert not c["want_rgb"].any()
        if c["state"] == "shift" and c["h"] * c["w"] >= 64:
            assert c["want_rgb"].any() and not np.array_equal(c["want_rgb"], c["img2"])
    assert any(c["want_counts"] == (1, 1) for c in cases) and any(c["want_counts"] == (1, 0) for c in cases)
    assert {c["tau"] for c in cases} == {0.25, 1.0, 1e9} and {c["iters"] for c in cases} == {1, 3, 8} and {c["smooth"] for c in cases} == {0.0, 0.9, 1.0}
    assert set(np.unique(np.concatenate([c["occ"].ravel() for c in cases]))) == {0, 1, 2, 3}


def test_warp_host_on_arbitrary_warps():
    rng = np.random.default_rng(1699)
    for (w, h) in SIZES[:6]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for k in range(12):
            wf = (rng.uniform(-1, 1, 6) * np.array([w, 0.3, 0.3, h, 0.3, 0.3])).astype(F)
            if k >= 8:
                wf[rng.integers(0, 6)] = [F(np.nan), F(np.inf), F(-np.inf), F(3e38)][k - 8]
            assert np.array_equal(io.stab_warp_host(wf, img), np_warp(wf, img)), (w, h, k)


def test_states_after_three_updates():
    """the path through three host updates (an invalid model among them) equals the restatement's, counts included"""
    rng = np.random.default_rng(1698)
    for smooth in (0.0, 0.9, 1.0):
        c, s, n = list(IDENT), list(IDENT), (0, 0)
        hc, hs = io.stab_identity()
        hn = (0, 0)
        for k in range(3):
            p = rng.uniform(-1, 1, 6) * np.array([5, 2e-3, 2e-3, 5, 2e-3, 2e-3])
            valid = int(k != 1)
            c, s, n, wf = np_update(c, s, n, p, valid, smooth, False)
            hc, hs, hwf, hn = io.stab_update_host(hc, hs, dict(p=p, valid=valid), smooth, False, hn)
            assert same_bits(hc, c) and same_bits(hs, s) and hn == n and np.array_equal(hwf.view(np.uint32), wf.view(np.uint32))
        assert n == (3, 1)
        if smooth == 0.0:
            assert same_bits(s, c) and not wf.any()          # pass-through: S is C bit for bit and the warp the identity
        if smooth == 1.0:
            assert same_bits(s, IDENT)                        # tripod lock: S never moves


# ---- arguments ----

def test_argument_checks_of_the_host_forms():
    L = _lib.lib()
    u = np.zeros((4, 4), F)
    o = np.zeros((4, 4), np.uint8)
    m = _lib.CGMotionModel()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    good = _lib.CStabParams(1.0, 3, 0.9)
    assert L.eppm_gmotion_fit_host(C.byref(good), ptr(u), ptr(u), ptr(o), 4, 4, C.byref(m), None) == 0
    for bad in [(0.0, 3, 0.9), (-1.0, 3, 0.9), (float("nan"), 3, 0.9), (float("inf"), 3, 0.9), (1.0, 0, 0.9), (1.0, 9, 0.9), (1.0, 3, -0.1),
                (1.0, 3, 1.5), (1.0, 3, float("nan"))]:
        p = _lib.CStabParams(*bad)
        assert L.eppm_gmotion_fit_host(C.byref(p), ptr(u), ptr(u), ptr(o), 4, 4, C.byref(m), None) == ARG, bad
    for h, w in [(0, 4), (4, 0), (1, 8193), (8193, 1), (8192, 8193)]:
        assert L.eppm_gmotion_fit_host(C.byref(good), ptr(u), ptr(u), ptr(o), h, w, C.byref(m), None) == ARG, (h, w)
    assert L.eppm_gmotion_fit_host(C.byref(good), None, ptr(u), ptr(o), 4, 4, C.byref(m), None) == ARG
    img = np.zeros((4, 4, 3), np.uint8)
    wf = np.zeros(6, F)
    assert L.eppm_stab_warp_host(ptr(wf), ptr(img), 4, 4, ptr(img)) == ARG          # the warp gathers
    d = _lib.CStabParams()
    assert L.eppm_stab_default_params(C.byref(d)) == 0 and (d.tau, d.iters, round(d.smooth, 6)) == (1.0, 3, 0.9)
    for name in ("Stabilizer", "stabilize_sequence", "stabilize_sequences"):
        assert hasattr(eppm_amd, name)


# ---- what it means ----

def test_the_background_motion_is_recovered_beside_a_moving_rectangle():
    """(a) on the rectangle cases the fitted displacement is within the quantisation step, 1/256 px, of the true background field at every
    pixel, and the mask is the rectangle"""
    for c in stab_cases():
        if c["kind"] != "rect" or c["h"] * c["w"] < 64:
            continue
        m, mask = io.gmotion_fit_host(c["u"], c["v"], c["occ"], c["tau"], c["iters"])
        X, Y = centred(c["h"], c["w"])
        p, t = m["p"], TRUE_P
        eu = (p[0] + p[1] * X + p[2] * Y) - (t[0] + t[1] * X + t[2] * Y)
        ev = (p[3] + p[4] * X + p[5] * Y) - (t[3] + t[4] * X + t[5] * Y)
        worst = float(np.sqrt(eu * eu + ev * ev).max())
        print(c["name"], "worst error of the fitted displacement", worst, "inlier share", (mask == 0).mean())
        assert worst <= 1.0 / 256.0, (c["name"], worst)
        ok = c["occ"] == 0
        assert np.array_equal(mask[ok] == 1, rectangle(c["h"], c["w"])[ok]), c["name"]


def band_limited(rng, h, w, sigma, lo, hi):
    """band-limited noise in [lo, hi], (h, w, 3) float64: white noise under a separable Gaussian"""
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = rng.standard_normal((h + 2 * r, w + 2 * r, 3))
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, a)
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, a)
    a = (a - a.min()) / (a.max() - a.min())
    return lo + (hi - lo) * a


def moving_clip(h, w, nframes, seed=11, sigma=5.0, bg_v=(2, 1), sq_v=(-1, 2), sq=24):
    """nframes noisy (h, w, 3) uint8 frames: a band-limited background translating by bg_v = (dx, dy) per frame (the camera), a textured
    sq x sq square moving by sq_v over it (an object of its own), Gaussian noise of `sigma`"""
    rng = np.random.default_rng(seed)
    pad = nframes * max(abs(bg_v[0]), abs(bg_v[1]), 1)
    canvas = band_limited(rng, h + 2 * pad, w + 2 * pad, 2.0, 40, 215)
    tex = band_limited(rng, sq, sq, 1.2, 30, 225)
    frames = []
    for k in range(nframes):
        f = canvas[pad - k * bg_v[1]: pad - k * bg_v[1] + h, pad - k * bg_v[0]: pad - k * bg_v[0] + w].copy()
        sx, sy = w // 2 + k * sq_v[0], h // 4 + k * sq_v[1]
        f[sy:sy + sq, sx:sx + sq] = tex
        frames.append(np.clip(np.rint(np.rint(f) + rng.normal(0, sigma, f.shape)), 0, 255).astype(np.uint8))
    return frames


def jitter_clip(h, w, offsets, seed=5):
    """a static textured scene seen through a window that moves by integer offsets: (frames, the true forward flows between them)"""
    rng = np.random.default_rng(seed)
    pad = 16
    scene = rng.integers(0, 256, (h + 2 * pad, w + 2 * pad, 3), dtype=np.uint8)
    frames = [scene[pad + oy:pad + oy + h, pad + ox:pad + ox + w].copy() for ox, oy in offsets]
    flows = [(offsets[k][0] - offsets[k + 1][0], offsets[k][1] - offsets[k + 1][1]) for k in range(len(offsets) - 1)]
    return frames, flows


def host_stabilize(frames, flows, smooth, tau=1.0, iters=3):
    """the host forms over a clip with constant true flows: (output frames, paths C)"""
    h, w, _ = frames[0].shape
    c, s = io.stab_identity()
    out, paths = [frames[0].copy()], []
    for k, (fu, fv) in enumerate(flows):
        m, _ = io.gmotion_fit_host(np.full((h, w), fu, F), np.full((h, w), fv, F), np.zeros((h, w), np.uint8), tau, iters)
        c, s, wf, _ = io.stab_update_host(c, s, m, smooth)
        out.append(io.stab_warp_host(wf, frames[k + 1]))
        paths.append(c)
    return out, paths


OFFSETS = [(0, 0), (-3, 2), (2, -1), (-1, -4), (4, 3)]


def test_tripod_lock():
    """(b) integer camera translations, the true flows, smooth = 1: every output frame is frame 0 wherever its source is in frame"""
    h, w = 45, 67
    frames, flows = jitter_clip(h, w, OFFSETS)
    assert flows[0] == (3, -2)
    m, _ = io.gmotion_fit_host(np.full((h, w), 3, F), np.full((h, w), -2, F), np.zeros((h, w), np.uint8))
    assert np.array_equal(m["p"].astype(F), np.array([3, 0, 0, -2, 0, 0], F))          # (3, -2) exactly in float32
    out, paths = host_stabilize(frames, flows, 1.0)
    ys, xs = np.mgrid[0:h, 0:w]
    for k in range(1, len(frames)):
        ox, oy = OFFSETS[k]
        src = (xs - ox >= 0) & (xs - ox <= w - 1) & (ys - oy >= 0) & (ys - oy <= h - 1)          # frame k shows the scene moved by -offset
        assert src.mean() > 0.7
        assert np.array_equal(out[k][src], frames[0][src]), f"frame {k}"
        assert not out[k][~src].any()


def test_pass_through():
    """(c) smooth = 0: the outputs are the input frames byte for byte"""
    frames, flows = jitter_clip(45, 67, OFFSETS)
    out, _ = host_stabilize(frames, flows, 0.0)
    for k, (a, b) in enumerate(zip(out, frames)):
        assert np.array_equal(a, b), f"frame {k}"


@pytest.mark.parametrize("size", [(1, 7), (7, 1)])
def test_a_line_of_pixels_has_no_model(size):
    """(d) 1 x 7 and 7 x 1: valid == 0 and the output is the input"""
    w, h = size
    for c in stab_cases():
        if (c["w"], c["h"]) != size or c["state"] not in ("empty", "stepped") or c["cut"]:
            continue
        m, _ = io.gmotion_fit_host(c["u"], c["v"], c["occ"], c["tau"], c["iters"])
        assert m["valid"] == 0 and not m["p"].any(), c["name"]
    img = np.random.default_rng(3).integers(0, 256, (h, w, 3), dtype=np.uint8)
    m, _ = io.gmotion_fit_host(np.full((h, w), 1, F), np.full((h, w), 1, F), np.zeros((h, w), np.uint8))
    cc, ss = io.stab_identity()
    cc, ss, wf, counts = io.stab_update_host(cc, ss, m, 0.9)
    assert m["valid"] == 0 and counts == (1, 1) and np.array_equal(io.stab_warp_host(wf, img), img)
