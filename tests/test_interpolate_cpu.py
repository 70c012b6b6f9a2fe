"""CPU tests of frame interpolation's ABI (include/eppm.h: eppm_interpolate*): the libraries export it, its argument
checks work without a GPU, and the host form equals a numpy restatement of section 11 bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io

NEW = ["eppm_interpolate", "eppm_interpolate_device", "eppm_batch_interpolate", "eppm_interpolate_frames", "eppm_interpolate_host"]
TIMES = (0.0, 1e-7, 0.25, 0.5, 0.7, 1 - 1e-7, 1.0)


def test_header_declares_and_libraries_export_the_interpolation_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eppm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eppm\w*)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    for variant in ("", "test", "tol"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW:
            getattr(L, s)
    cls = open(os.path.join(ROOT, "include", "bao_flow_patchmatch_multiscale_cuda.h")).read()
    assert "bool interpolate_frame(float t, unsigned char*** img_t)" in cls


def test_argument_errors_without_a_device():
    L = _lib.lib()
    h = w = 4
    img = np.zeros(h * w * 4, np.uint8)
    f = np.zeros(h * w, np.float32)
    pi, pf = img.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    null = C.c_void_p()
    ts = (C.c_float * 1)(0.5)
    outs = (C.c_void_p * 1)(img.ctypes.data)
    # context forms: NULL context, NULL times / outputs, nt < 1
    assert L.eppm_interpolate(null, 1, ts, outs, C.c_size_t(w * 3)) == 1
    assert L.eppm_interpolate_device(null, 1, ts, outs, C.c_size_t(w * 4)) == 1
    assert L.eppm_batch_interpolate(null, 1, ts, outs, C.c_size_t(w * 3)) == 1

    def host(t, hh=h, ww=w, out=pi, a=pi, b=pi, u=pf, v=pf, o1=pi, o2=pi):
        return L.eppm_interpolate_host(out, a, b, u, v, o1, o2, hh, ww, C.c_float(t))

    def frames(t, hh=h, ww=w, out=pi, a=pi, flow=pf, o1=pi):
        return L.eppm_interpolate_frames(out, C.c_size_t(w * 4), a, a, C.c_size_t(w * 4), flow, o1, o1, hh, ww, C.c_float(t))

    for t in (float("nan"), -0.1, 1.5, float("inf")):
        assert host(t) == 1, t
        assert frames(t) == 1, t
    for bad in (dict(out=null), dict(a=null), dict(b=null), dict(u=null), dict(v=null), dict(o1=null), dict(o2=null), dict(hh=0), dict(ww=0),
                dict(hh=-3)):
        assert host(0.5, **bad) == 1, bad
    for bad in (dict(out=null), dict(a=null), dict(flow=null), dict(o1=null), dict(hh=0), dict(ww=0)):
        assert frames(0.5, **bad) == 1, bad
    assert L.eppm_interpolate_frames(pi, C.c_size_t(w * 4 - 4), pi, pi, C.c_size_t(w * 4), pf, pi, pi, h, w, C.c_float(0.5)) == 1   # pitch < 4w
    assert host(0.5) == 0 and host(0.0) == 0 and host(1.0) == 0


# ---------------------------------------------------------------------------------------------------
# numpy restatement of DESIGN.md section 11: every float operation one float32 rounding, left to right
# ---------------------------------------------------------------------------------------------------
def _bilinear(I, qx, qy):
    """I: (h, w, 3) float32; (qx, qy) clamped into the frame first; taps and weights as the occlusion test's."""
    f32 = np.float32
    h, w, _ = I.shape
    qx = np.minimum(np.maximum(qx, f32(0)), f32(w - 1))
    qy = np.minimum(np.maximum(qy, f32(0)), f32(h - 1))
    x0 = np.floor(qx).astype(np.int64)
    y0 = np.floor(qy).astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    ax = (qx - x0.astype(f32))[..., None]
    ay = (qy - y0.astype(f32))[..., None]
    bx, by = f32(1) - ax, f32(1) - ay
    return by * (bx * I[y0, x0] + ax * I[y0, x1]) + ay * (bx * I[y1, x0] + ax * I[y1, x1])


def _nearest(valid, axis, reverse):
    """Per pixel: coordinate along `axis` of the nearest valid pixel strictly before it (reverse: strictly after), -1 / n for none."""
    n = valid.shape[axis]
    idx = np.arange(n).reshape((-1, 1) if axis == 0 else (1, -1))
    if not reverse:
        last = np.maximum.accumulate(np.where(valid, idx, -1), axis=axis)
        prev = np.concatenate([np.full_like(np.take(last, [0], axis), -1), np.delete(last, n - 1, axis)], axis=axis)
        return prev
    nxt = np.flip(np.minimum.accumulate(np.flip(np.where(valid, idx, n), axis), axis=axis), axis)
    return np.concatenate([np.delete(nxt, 0, axis), np.full_like(np.take(nxt, [0], axis), n)], axis=axis)


def interpolate_np(img1, img2, u, v, occ1, occ2, t, parts=None):
    """parts: a dict that receives the splat mask and the two fill passes' source planes (-1: a hole), for the ledger."""
    f32 = np.float32
    t = f32(t)
    if t == 0:
        return img1.copy()
    if t == 1:
        return img2.copy()
    h, w = u.shape
    I1, I2 = img1.astype(f32), img2.astype(f32)
    ys, xs = np.mgrid[0:h, 0:w]
    HOLE = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(invalid="ignore", over="ignore"):
        known = ((np.abs(u) <= f32(1e9)) & (np.abs(v) <= f32(1e9))).ravel()
    src = np.nonzero(known)[0]
    x, y = xs.ravel()[src], ys.ravel()[src]
    fx, fy = u.ravel()[src], v.ravel()[src]
    xf, yf = x.astype(f32), y.astype(f32)
    # (a) splat
    c2 = _bilinear(I2, xf + fx, yf + fy)
    c1 = I1[y, x]
    cost = (np.abs(c1[:, 0] - c2[:, 0]) + np.abs(c1[:, 1] - c2[:, 1])) + np.abs(c1[:, 2] - c2[:, 2])
    cls = (occ1.ravel()[src] != 0).astype(np.uint64)
    key = (((cls << np.uint64(31)) | cost.astype(f32).view(np.uint32).astype(np.uint64)) << np.uint64(32)) | src.astype(np.uint64)
    bx, by = np.floor(xf + t * fx), np.floor(yf + t * fy)
    keys = np.full(h * w, HOLE, np.uint64)
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = bx + f32(dx), by + f32(dy)
            ok = (cx >= 0) & (cx <= f32(w - 1)) & (cy >= 0) & (cy <= f32(h - 1))
            np.minimum.at(keys, cy[ok].astype(np.int64) * w + cx[ok].astype(np.int64), key[ok])
    keys = keys.reshape(h, w)
    splat = keys != HOLE
    s0 = np.where(splat, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    # (b) pass 1: nearest splatted pixel left, right, up, down; ties in that order
    L, R = _nearest(splat, 1, False), _nearest(splat, 1, True)
    U, D = _nearest(splat, 0, False), _nearest(splat, 0, True)
    big = np.int64(1) << 40
    dist = np.stack([np.where(L >= 0, xs - L, big), np.where(R < w, R - xs, big), np.where(U >= 0, ys - U, big), np.where(D < h, D - ys, big)])
    cand = np.stack([s0[ys, np.clip(L, 0, w - 1)], s0[ys, np.clip(R, 0, w - 1)], s0[np.clip(U, 0, h - 1), xs], s0[np.clip(D, 0, h - 1), xs]])
    pick = np.argmin(dist, axis=0)
    found = np.take_along_axis(dist, pick[None], 0)[0] < big
    f1 = np.where(splat, s0, np.where(found, np.take_along_axis(cand, pick[None], 0)[0], -1))
    # (b) pass 2: nearest filled pixel of pass 1 in the row, ties to the left
    filled = f1 >= 0
    L, R = _nearest(filled, 1, False), _nearest(filled, 1, True)
    dl = np.where(L >= 0, xs - L, big)
    dr = np.where(R < w, R - xs, big)
    f2 = np.where(filled, f1, np.where((dl <= dr) & (dl < big), f1[ys, np.clip(L, 0, w - 1)], np.where(dr < big, f1[ys, np.clip(R, 0, w - 1)], -1)))
    if parts is not None:
        parts.update(splat=splat, f1=f1, f2=f2)
    # (c) blend
    ux = np.where(f2 >= 0, u.ravel()[np.maximum(f2, 0)], f32(0)).astype(f32)
    uy = np.where(f2 >= 0, v.ravel()[np.maximum(f2, 0)], f32(0)).astype(f32)
    s = f32(1) - t
    X, Y = xs.astype(f32), ys.astype(f32)
    x0 = np.minimum(np.maximum(X - t * ux, f32(0)), f32(w - 1))
    y0 = np.minimum(np.maximum(Y - t * uy, f32(0)), f32(h - 1))
    x1 = np.minimum(np.maximum(X + s * ux, f32(0)), f32(w - 1))
    y1 = np.minimum(np.maximum(Y + s * uy, f32(0)), f32(h - 1))
    c0, c1 = _bilinear(I1, x0, y0), _bilinear(I2, x1, y1)
    near = lambda q: np.floor(q + f32(0.5)).astype(np.int64)        # noqa: E731
    a = (occ1[near(y0), near(x0)] != 0)[..., None]
    b = (occ2[near(y1), near(x1)] != 0)[..., None]
    c = np.where(a & ~b, c0, np.where(b & ~a, c1, s * c0 + t * c1))
    return np.minimum(255, np.floor(c + f32(0.5))).astype(np.uint8)


def smooth_flow(rng, h, w, amp):
    gh, gw = max(2, h // 16 + 2), max(2, w // 16 + 2)
    g = rng.uniform(-amp, amp, (2, gh, gw)).astype(np.float32)
    ys = np.linspace(0, gh - 1, h)
    xs = np.linspace(0, gw - 1, w)
    out = []
    for c in range(2):
        rows = np.array([np.interp(xs, np.arange(gw), g[c, i]) for i in range(gh)])
        out.append(np.ascontiguousarray(np.array([np.interp(ys, np.arange(gh), rows[:, j]) for j in range(w)]).T, np.float32))
    return out


def interpolation_cases():
    """(name, img1, img2, u, v, occ1, occ2): the cases the CPU and GPU tests share."""
    rng = np.random.default_rng(29)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                   # noqa: E731
    occ = lambda h, w: rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))         # noqa: E731
    cases = []
    for k, (h, w, amp) in enumerate(((48, 64, 4.0), (53, 41, 9.0), (90, 120, 20.0))):
        u, v = smooth_flow(rng, h, w, amp)
        cases.append((f"random{k}", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))
    # NaN / 1e10 vectors
    h, w = 40, 56
    u, v = smooth_flow(rng, h, w, 3.0)
    for a in (u, v):
        idx = rng.integers(0, a.size, 80)
        a.reshape(-1)[idx[:40]] = np.nan
        a.reshape(-1)[idx[40:]] = 1e10 * rng.choice([-1, 1], 40)
    u[0, :5] = 1e9
    cases.append(("unknown", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))
    # vectors leaving the frame on every side
    h, w = 30, 44
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    u = ((xs - w / 2) * 0.9).astype(np.float32)
    v = ((ys - h / 2) * 1.3).astype(np.float32)
    cases.append(("leaving", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))
    # crossing flows: the left half moves right, the right half left, with equal costs on a flat image (ties down to the source index)
    h, w = 36, 48
    u = np.where(np.arange(w)[None, :] < w // 2, 9.0, -9.0).astype(np.float32).repeat(h, 0)
    v = rng.integers(-2, 3, (h, w)).astype(np.float32)
    flat = np.full((h, w, 3), 77, np.uint8)
    cases.append(("crossing", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))
    cases.append(("crossing_flat", flat, flat.copy(), u, v, occ(h, w), np.zeros((h, w), np.uint8)))
    # nothing known: zero fill; exactly one known vector: both fill passes
    h, w = 33, 29
    nan = np.full((h, w), np.nan, np.float32)
    cases.append(("all_unknown", img(h, w), img(h, w), nan, nan.copy(), occ(h, w), occ(h, w)))
    u1, v1 = nan.copy(), nan.copy()
    u1[20, 7], v1[20, 7] = 2.5, -3.25
    cases.append(("one_known", img(h, w), img(h, w), u1, v1, occ(h, w), occ(h, w)))
    # 1x1, 1xN, Nx1 and an odd size
    for h, w in ((1, 1), (1, 37), (37, 1), (53, 41)):
        u = rng.uniform(-3, 3, (h, w)).astype(np.float32)
        v = rng.uniform(-3, 3, (h, w)).astype(np.float32)
        cases.append((f"size{h}x{w}", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))
    return cases + block_edge_cases()


BLOCK_EDGE_SIZES = ((63, 3), (64, 4), (65, 5), (129, 9))       # (w, h) around the kernels' 64x4 blocks (k_interp.hip: interp_grid)


def block_edge_cases():
    """Frames one short of, equal to and one past a 64x4 block in both directions, and two blocks and a pixel wide.  Per size: a smooth
    flow with the special values; then a single known vector in the first and in the last pixel (the fill passes walk a whole row and
    column, up to 128 steps) and known vectors in column 0 only (every hole walks left, up to 128 steps)."""
    rng = np.random.default_rng(30)
    img = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                   # noqa: E731
    occ = lambda h, w: rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))         # noqa: E731
    cases = []
    for w, h in BLOCK_EDGE_SIZES:
        add = lambda name, u, v: cases.append((f"{name}_{w}x{h}", img(h, w), img(h, w), u, v, occ(h, w), occ(h, w)))   # noqa: E731
        u, v = smooth_flow(rng, h, w, 3.0)
        for a in (u, v):
            idx = rng.choice(a.size, 12, replace=False)
            a.reshape(-1)[idx[:6]] = np.nan
            a.reshape(-1)[idx[6:]] = 1e10 * rng.choice([-1, 1], 6)
        u[h - 1, w - 3:] = 1e9
        add("edge_random", u, v)
        nan = np.full((h, w), np.nan, np.float32)
        u, v = nan.copy(), nan.copy()
        u[0, 0], v[0, 0] = 1.5, 0.75
        add("corner_only", u, v)
        u, v = nan.copy(), nan.copy()
        u[h - 1, w - 1], v[h - 1, w - 1] = -1.5, -0.75
        add("far_corner_only", u, v)
        u, v = nan.copy(), nan.copy()
        u[:, 0] = rng.uniform(0, 2, h).astype(np.float32)
        v[:, 0] = rng.uniform(-1, 1, h).astype(np.float32)
        add("column_only", u, v)
    return cases


# (w, h) thin frames 8192 long: section 16's bound, which the objects fed from the same planes obey (the caller-plane form's
# own check is h*w < 2^31): splats at coordinate 8191, fill walks along a whole row or column of 8192, 32 KiB image rows
LIMIT_SIZES = ((8192, 20), (20, 8192))
LIMIT_TIMES = (1e-7, 0.5, 0.7)
_LIMIT = {}


def limit_cases(size):
    """the cases of LIMIT_SIZES[size], built on first use (not at import): a smooth flow with the special values; vectors that leave the
    frame by a fraction of a pixel at both ends of the long side and land exactly on its last pixel; a single known vector in the first
    and in the last pixel (the fill passes walk the whole long side)"""
    if size not in _LIMIT:
        w, h = LIMIT_SIZES[size]
        rng = np.random.default_rng(31 + size)
        img = lambda: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                        # noqa: E731
        occ = lambda: rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))              # noqa: E731
        cases = []
        add = lambda name, u, v: cases.append((f"{name}_{w}x{h}", img(), img(), u, v, occ(), occ()))   # noqa: E731
        u, v = smooth_flow(rng, h, w, 3.0)
        for a in (u, v):
            idx = rng.choice(a.size, 200, replace=False)
            a.reshape(-1)[idx[:100]] = np.nan
            a.reshape(-1)[idx[100:]] = 1e10 * rng.choice([-1, 1], 100)
        u[h - 1, w - 3:] = 1e9
        add("limit_random", u, v)
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
        along, n = (xs, w) if w > h else (ys, h)
        f = rng.uniform(-1.5, 1.5, (h, w)).astype(np.float32)
        near, far = along < 64, along >= n - 64
        f[near] = (-along - np.float32(0.25) * rng.integers(-2, 3, (h, w)))[near]              # ends within half a pixel of coordinate 0 ...
        f[far] = (np.float32(n - 1) - along + np.float32(0.25) * rng.integers(-2, 3, (h, w)))[far]          # ... and of the last one
        g = rng.uniform(-0.5, 0.5, (h, w)).astype(np.float32)
        add("limit_ends", *((f, g) if w > h else (g, f)))
        nan = np.full((h, w), np.nan, np.float32)
        u, v = nan.copy(), nan.copy()
        u[0, 0], v[0, 0] = 1.5, 0.75
        add("limit_corner_only", u, v)
        u, v = nan.copy(), nan.copy()
        u[h - 1, w - 1], v[h - 1, w - 1] = -1.5, -0.75
        add("limit_far_corner_only", u, v)
        _LIMIT[size] = cases
    return _LIMIT[size]


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_host_form_equals_numpy_restatement_at_the_size_limit(size):
    w, h = LIMIT_SIZES[size]
    for name, a, b, u, v, o1, o2 in limit_cases(size):
        for t in LIMIT_TIMES:
            parts = {}
            want = interpolate_np(a, b, u, v, o1, o2, t, parts)
            got = io.interpolate(a, b, u, v, o1, o2, t)
            bad = int((got != want).any(-1).sum())
            assert bad == 0, f"{name} t={t}: {bad} of {u.size} pixels differ"
            splat = parts["splat"]
            if name.startswith("limit_ends") and t == 0.5:          # splats on the first and the last pixels of the long side
                line = splat.any(axis=0 if w > h else 1)
                assert line[0] and line[-1], name
            if "corner_only" in name:                               # one splat: pass 1 fills its row and column, pass 2 everything else
                assert 0 < splat.sum() <= 4 and (parts["f1"] < 0).any() and (parts["f2"] >= 0).all(), name
                src = int(np.nonzero(np.isfinite(u).ravel())[0][0])
                assert (parts["f2"] == src).all(), name


@pytest.mark.parametrize("case", interpolation_cases(), ids=lambda c: c[0])
def test_host_form_equals_numpy_restatement(case):
    name, a, b, u, v, o1, o2 = case
    for t in TIMES:
        got = io.interpolate(a, b, u, v, o1, o2, t)
        want = interpolate_np(a, b, u, v, o1, o2, t)
        assert got.dtype == np.uint8 and got.shape == a.shape
        bad = int((got != want).any(-1).sum())
        assert bad == 0, f"{name} t={t}: {bad} of {u.size} pixels differ"


def test_block_edge_ledger():
    """What the single-vector cases reach at 129x9 (t = 0.5), from the restatement's own planes: pass 1 leaves holes that pass 2 fills, and
    both walk more than a block's width.  The splatted pixels' columns are filled in every row by pass 1, so pass 2 finds a filled pixel in
    every row: with one known vector no row can stay unfilled (only a frame without any splat keeps holes: `all_unknown`)."""
    cases = {c[0]: c for c in block_edge_cases()}
    assert len(cases) == 4 * len(BLOCK_EDGE_SIZES)
    for name, col in (("far_corner_only_129x9", 128), ("corner_only_129x9", 0)):
        _, a, b, u, v, o1, o2 = cases[name]
        h, w = u.shape
        src = int(np.nonzero(np.isfinite(u).ravel())[0][0])
        parts = {}
        interpolate_np(a, b, u, v, o1, o2, 0.5, parts)
        splat, f1, f2 = parts["splat"], parts["f1"], parts["f2"]
        ys, xs = np.nonzero(splat)
        assert 0 < len(xs) <= 4 and (abs(xs - col) <= 2).all()
        hole1 = f1 < 0
        assert hole1.any() and (f2[hole1] == src).all() and (f1[~hole1] == src).all()
        rows, cols = np.unique(ys), np.unique(xs)
        assert not hole1[rows].any() and not hole1[:, cols].any()                   # pass 1: the splats' rows and columns, whole
        assert hole1[np.setdiff1d(np.arange(h), rows)][:, np.setdiff1d(np.arange(w), cols)].all()  # and nothing else
        assert (f2 >= 0).all()
    # column 0 only: every row is splatted near its left end; the holes right of it walk left through two blocks
    _, a, b, u, v, o1, o2 = cases["column_only_129x9"]
    parts = {}
    interpolate_np(a, b, u, v, o1, o2, 0.5, parts)
    assert parts["splat"][:, :3].any(1).all() and not parts["splat"][:, 4:].any() and (parts["f1"] >= 0).all()
    # the smooth cases hold NaN, +-1e10 and 1e9, and both known and unknown vectors in the last row
    for w, h in BLOCK_EDGE_SIZES:
        u, v = cases[f"edge_random_{w}x{h}"][3:5]
        assert np.isnan(u).any() and (np.abs(u) == np.float32(1e10)).any() and (u == np.float32(1e9)).any() and np.isnan(v).any()


def test_endpoints_return_the_inputs():
    for name, a, b, u, v, o1, o2 in interpolation_cases():
        assert np.array_equal(io.interpolate(a, b, u, v, o1, o2, 0.0), a), name
        assert np.array_equal(io.interpolate(a, b, u, v, o1, o2, 1.0), b), name
        assert np.array_equal(io.interpolate(a, b, u, v, o1, o2, -0.0), a), name


def test_fill_and_choice_rules():
    """Small hand-checked cases of the rules section 11 states."""
    h, w = 5, 7
    a = np.zeros((h, w, 3), np.uint8)
    b = np.full((h, w, 3), 200, np.uint8)
    z = np.zeros((h, w), np.uint8)
    # nothing known: ut = 0 everywhere, the plain blend 0.5 * 0 + 0.5 * 200
    nan = np.full((h, w), np.nan, np.float32)
    assert (io.interpolate(a, b, nan, nan, z, z, 0.5) == 100).all()
    # masks choose the frame: a = occ1(x0) != 0 alone -> image 1's colour only (visible in image 1, hidden in image 2); b alone -> image 2's
    zero = np.zeros((h, w), np.float32)
    one = np.ones((h, w), np.uint8)
    assert (io.interpolate(a, b, zero, zero, one, z, 0.5) == 0).all()         # a && !b: c0
    assert (io.interpolate(a, b, zero, zero, z, one, 0.5) == 200).all()       # b && !a: c1 (the surface was disoccluded)
    assert (io.interpolate(a, b, zero, zero, one, one, 0.25) == 50).all()     # both: the blend 0.75 * 0 + 0.25 * 200
    # a consistent vector wins over an inconsistent one of lower cost at a shared target
    img1 = np.zeros((1, 8, 3), np.uint8)
    img2 = np.zeros((1, 8, 3), np.uint8)
    u = np.full((1, 8), np.nan, np.float32)
    v = np.zeros((1, 8), np.float32)
    u[0, 0], u[0, 6] = 4.0, -4.0             # at t = 0.5: source 0 -> block {2, 3}, source 6 -> block {4, 5}
    u[0, 1] = 2.0                            # source 1 -> block {2, 3}
    o1 = np.zeros((1, 8), np.uint8)
    o1[0, 1] = 1                             # the competitor of source 0 at x = 2, 3 is inconsistent
    img2[0, 4] = 90                          # source 0's photo cost 270, source 1's 0
    out = interpolate_np(img1, img2, u, v, o1, np.zeros_like(o1), 0.5)
    assert np.array_equal(io.interpolate(img1, img2, u, v, o1, np.zeros_like(o1), 0.5), out)
    # at x = 2 source 0 wins (consistent): ut = 4, x0 = 0, x1 = 4 -> 0.5 * 0 + 0.5 * 90 = 45
    assert out[0, 2, 0] == 45, out[0, :, 0]
