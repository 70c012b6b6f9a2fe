"""CPU tests of the dense correspondence map: the ABI's argument checks, a numpy restatement of the step and the
render against eppm_cmap_step_host / eppm_cmap_render_host bit for bit on the shared generator cmap_cases() (the GPU tests run the kernels
on the same cases), and what the map means: exactly on an integer-motion clip, and against frame-to-frame warping on a sub-pixel one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io
from test_tfilter_cpu import _smooth, moving_clip, same_bits

F = np.float32
ARG, STATE = 1, 3
LOST = F(1e10)
SMOOTH, TEAR, LOST23, LOSTN, LOST6, LOSTC, CUT = range(7)           # where a pixel's step ended (np_step's second result)


# ---- the numpy restatement of section 19 ----

def np_seed(h, w):
    m = np.empty((h, w, 2), F)
    m[..., 0] = np.arange(w, dtype=F)[None, :]
    m[..., 1] = np.arange(h, dtype=F)[:, None]
    return m


def np_known(x, y):
    with np.errstate(invalid="ignore"):
        return (np.abs(x) <= F(1e9)) & (np.abs(y) <= F(1e9))


def np_in_frame(px, py, h, w):
    with np.errstate(invalid="ignore"):
        return (px >= F(0)) & (px <= F(w - 1)) & (py >= F(0)) & (py <= F(h - 1))


def np_taps(qx, qy, h, w):
    """taps and weights of points inside the frame (callers replace every other point by (0, 0) first)"""
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = qx - x0.astype(F), qy - y0.astype(F)
    return x0, y0, x1, y1, ax, ay, F(1) - ax, F(1) - ay


def np_bl(t, plane):
    """bl() of a float32 plane (h, w) at taps t"""
    x0, y0, x1, y1, ax, ay, bx, by = t
    out = by * (bx * plane[y0, x0] + ax * plane[y0, x1]) + ay * (bx * plane[y1, x0] + ax * plane[y1, x1])
    assert out.dtype == F
    return out


def np_step(M, A, img2, bu, bv, occ, thresh, tear, use_occ, cut):
    """(new map, where every pixel's step ended, the branch taken at steps 4 / 5): every operation one float32 rounding, in the order of section 19.  M: the previous map;
    A: the anchor frame's bytes."""
    h, w = bu.shape
    if cut:
        return np_seed(h, w), np.full((h, w), CUT), np.full((h, w), -1)
    with np.errstate(all="ignore"):
        qx = np.arange(w, dtype=F)[None, :] + bu
        qy = np.arange(h, dtype=F)[:, None] + bv
        ok = np_known(bu, bv) & np_in_frame(qx, qy, h, w)
        if use_occ:
            ok &= occ == 0
        end = np.where(ok, -1, LOST23)
        qx, qy = np.where(ok, qx, F(0)), np.where(ok, qy, F(0))
        t = np_taps(qx, qy, h, w)
        x0, y0, x1, y1 = t[:4]
        nx, ny = np.floor(qx + F(0.5)).astype(np.int64), np.floor(qy + F(0.5)).astype(np.int64)
        mx, my = M[..., 0], M[..., 1]
        mnx, mny = mx[ny, nx], my[ny, nx]
        end = np.where((end < 0) & ~np_known(mnx, mny), LOSTN, end)
        smooth = np.ones((h, w), bool)
        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            smooth &= np_known(mx[yy, xx], my[yy, xx]) & (np.abs(mx[yy, xx] - mnx) <= F(tear)) & (np.abs(my[yy, xx] - mny) <= F(tear))
        sx = np.where(smooth, np_bl(t, mx), mnx + (qx - nx.astype(F)))
        sy = np.where(smooth, np_bl(t, my), mny + (qy - ny.astype(F)))
        case = np.where(smooth, SMOOTH, TEAR)
        inside = np_in_frame(sx, sy, h, w)
        end = np.where((end < 0) & ~inside, LOST6, end)
        live = end < 0
        u = np_taps(np.where(live, sx, F(0)), np.where(live, sy, F(0)), h, w)
        a, cur = A.astype(F), img2.astype(F)
        p = [np_bl(u, a[..., c]) for c in range(3)]
        d = (np.abs(cur[..., 0] - p[0]) + np.abs(cur[..., 1] - p[1])) + np.abs(cur[..., 2] - p[2])
        end = np.where(live & ~(d <= F(thresh)), LOSTC, end)
        kept = end < 0
        out = np.empty((h, w, 2), F)
        out[..., 0] = np.where(kept, sx, LOST)
        out[..., 1] = np.where(kept, sy, LOST)
        # the branch a pixel took at steps 4 / 5 is reported for every pixel that reached them
        reached = (end < 0) | (end == LOST6) | (end == LOSTC)
    return out, np.where(kept, case, end), np.where(reached, case, -1)


def np_render(cur, M, layer):
    """(bytes, the pixels that composite the layer): layer is (h, w, 4) RGBA"""
    h, w, _ = cur.shape
    with np.errstate(all="ignore"):
        sx, sy = M[..., 0], M[..., 1]
        ok = np_known(sx, sy) & np_in_frame(sx, sy, h, w)
        t = np_taps(np.where(ok, sx, F(0)), np.where(ok, sy, F(0)), h, w)
        lay = layer.astype(F)
        pa = np_bl(t, lay[..., 3])
        out = np.empty((h, w, 3), np.uint8)
        for c in range(3):
            pc = np_bl(t, lay[..., c] * lay[..., 3])
            v = (pc + (F(255) - pa) * cur[..., c].astype(F)) / F(255)
            assert v.dtype == F
            byte = np.floor(np.fmin(np.fmax(v, F(0)), F(255)) + F(0.5)).astype(np.uint8)
            out[..., c] = np.where(ok, byte, cur[..., c])
    return out, ok


def default_layer(anchor):
    return np.concatenate([anchor, np.full(anchor.shape[:2] + (1,), 255, np.uint8)], -1)


# ---- the shared cases ----

SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157)]           # w x h
# (previous map, tear, thresh, use_occ, cut, layer).  Previous maps: "seed"; "stepped" (three steps of the restatement from the seed);
# "torn" (two half-planes offset by more than `tear`, with lost pixels); "blocky" (constant over 4 x 4 blocks, with lost pixels: the one
# kind of map whose taps agree at tear = 0); "empty" (an empty slot: the seed, and image 1 is the anchor).
CONFIGS = [("seed", 2.0, 90.0, 1, False, None), ("stepped", 2.0, 90.0, 1, False, "ramp"), ("torn", 2.0, 90.0, 0, False, "a255"),
           ("blocky", 0.0, 90.0, 1, False, "a0"), ("torn", 1e9, 90.0, 1, False, "ramp"), ("torn", 2.0, 0.0, 1, False, None),
           ("torn", 2.0, 1e9, 1, False, "ramp"), ("empty", 2.0, 90.0, 1, False, "ramp"), ("stepped", 2.0, 90.0, 1, True, "a255"),
           ("empty", 2.0, 90.0, 0, True, None)]
# The four outcomes every uncut case of at least 64 pixels must send at least 5 % of its pixels through -- the smooth case, the tear case,
# lost at steps 2-3, lost at the colour check -- except where the case's own state and parameters make one unreachable, which is then
# asserted to be EMPTY: neighbouring taps of a seed map differ by exactly 1, so with tear = 2 they never tear; d is at most 765, so
# with thresh = 1e9 nothing fails the colour check; with tear = 1e9 only a lost tap tears, which the torn map's lost pixels provide.
UNREACHABLE = {("seed", 2.0): "tear", ("empty", 2.0): "tear"}


def _vectors(rng, h, w, shift, integer):
    """backward vectors: ~60 % the coherent shift, ~15 % to random places inside the frame, the rest the special ones"""
    ys, xs = np.mgrid[0:h, 0:w]
    tx, ty = rng.uniform(0, w - 1, (h, w)), rng.uniform(0, h - 1, (h, w))
    whole = (rng.random((h, w)) < 0.4) | integer
    tx, ty = np.where(whole, np.rint(tx), tx), np.where(whole, np.rint(ty), ty)
    coherent = rng.random((h, w)) < 0.8
    bu = np.where(coherent, shift[0], tx - xs).astype(F)
    bv = np.where(coherent, shift[1], ty - ys).astype(F)
    kind = rng.integers(0, 64, (h, w))
    xf, yf = xs.astype(F), ys.astype(F)
    up = lambda v: np.nextafter(F(v), F(np.inf))                          # noqa: E731
    special = {
        0: (F(w - 1) - xf, bv), 1: (bu, F(h - 1) - yf), 2: (F(w - 1) - xf, F(h - 1) - yf),          # exactly on the last column / row
        3: (up(w - 1) - xf, bv), 4: (bu, up(h - 1) - yf),                                           # one ulp outside (where the sum is exact)
        5: (-xf - F(1e-45), bv), 6: (bu, -yf - F(1e-45)),                                           # just below 0 (x = 0 / y = 0: a denormal)
        7: (np.full((h, w), F(1e10)), bv), 8: (bu, np.full((h, w), F(-1e10))),
        9: (np.full((h, w), F(np.inf)), bv), 10: (bu, np.full((h, w), F(-np.inf))),
        11: (np.full((h, w), F(np.nan)), bv), 12: (bu, np.full((h, w), F(np.nan))),
        13: (np.where(xs >= 0, F(-0.0), F(0)), np.where(xs >= 0, F(-0.0), F(0))),
        14: (bu + F(w), bv), 15: (bu, bv - F(h)),                                                   # plainly outside
    }
    for k, (su, sv) in special.items():
        bu = np.where(kind == k, su, bu).astype(F)
        bv = np.where(kind == k, sv, bv).astype(F)
    return bu, bv


def _sprinkle_lost(rng, m, share):
    """lost pixels: the canonical (1e10, 1e10) and every other value that reads as lost"""
    h, w, _ = m.shape
    hit = rng.random((h, w)) < share
    how = rng.integers(0, 5, (h, w))
    vals = [(LOST, LOST), (F(np.nan), F(3)), (F(2), F(-np.inf)), (F(2e9), F(1)), (F(-1e10), F(np.nan))]
    for k, (vx, vy) in enumerate(vals):
        m[..., 0] = np.where(hit & (how == k), vx, m[..., 0])
        m[..., 1] = np.where(hit & (how == k), vy, m[..., 1])
    return m


def _prev_map(rng, kind, h, w, tear, integer):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind in ("seed", "empty"):
        return np_seed(h, w)
    if kind == "stepped":
        m = np_seed(h, w)
        blank, zero = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
        for _ in range(3):
            shift = (F(rng.integers(-2, 3)) * F(0.5), F(rng.integers(-1, 2)) * F(0.25))
            bu, bv = _vectors(rng, h, w, shift, False)
            few = rng.random((h, w)) < 0.06                  # few vectors off the shift per step: the losses add up over three
            bu, bv = np.where(few, bu, shift[0]).astype(F), np.where(few, bv, shift[1]).astype(F)
            m = np_step(m, blank, blank, bu, bv, zero, 1e9, 2.0, 0, False)[0]
        return m
    if kind == "torn":                                       # a boundary between two surfaces: the right / lower part comes from elsewhere
        off = 3.0 if tear < 1e8 else 40.0
        frac = 0.0 if integer else 0.25
        split = (xs + ys // 2) % max(8, w // 3) >= max(4, w // 6)          # slanted stripes, so that every size has boundaries
        m = np.empty((h, w, 2), F)
        m[..., 0] = (xs + np.where(split, -off - frac, 0.0)).astype(F)
        m[..., 1] = (ys + np.where(split, frac, 0.0)).astype(F)
        return _sprinkle_lost(rng, m, 0.10)
    if kind == "blocky":
        m = np.empty((h, w, 2), F)
        m[..., 0] = ((xs // 4) * 4).astype(F)
        m[..., 1] = ((ys // 4) * 4).astype(F)
        return _sprinkle_lost(rng, m, 0.04)
    raise ValueError(kind)


def _case(seed, w, h, prev, tear, thresh, use_occ, cut, layer):
    rng = np.random.default_rng(seed)
    integer = thresh == 0.0                                  # d = 0 needs whole positions: the anchor's own bytes
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if prev == "empty":
        anchor = img1
    elif min(h, w) >= 4:
        anchor = np.rint(_smooth(rng, h, w, 1.5, 0, 255)).astype(np.uint8)          # band-limited, so that a sub-pixel sample is near its taps
    else:
        anchor = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    M = _prev_map(rng, prev, h, w, tear, integer)
    shift = (F(1), F(0)) if integer else (F(1.5), F(-0.25))
    bu, bv = _vectors(rng, h, w, shift, integer)
    occ = np.where(rng.random((h, w)) < 0.8, 0, rng.integers(0, 4, (h, w))).astype(np.uint8)        # bytes 0..3, zero most often
    # image 2: the anchor at the composed position where there is one, plus noise: small for most pixels, beyond every finite thresh for some
    s, _, _ = np_step(M, anchor, np.zeros((h, w, 3), np.uint8), bu, bv, occ, 1e9, tear, 0, False)
    base = _sample(anchor, s)
    amp = rng.choice([0 if integer else 8, 90], (h, w, 1), p=[0.7, 0.3])
    noise = np.sign(rng.integers(0, 2, (h, w, 3)) - 0.5) * rng.integers(amp // 2, amp + 1)
    img2 = np.clip(np.rint(base) + noise, 0, 255).astype(np.uint8)
    c = dict(name=f"{w}x{h}-{prev}-tear{tear:g}-t{thresh:g}-occ{use_occ}{'-cut' if cut else ''}", h=h, w=w, prev=prev, map=M, anchor=anchor,
             img1=img1, img2=img2, bu=bu, bv=bv, occ=occ, thresh=thresh, tear=tear, use_occ=use_occ, cut=cut)
    c["want_map"], end, branch = np_step(M, anchor, img2, bu, bv, occ, thresh, tear, use_occ, cut)
    c["want_anchor"] = img2 if cut else anchor
    if layer is None:
        c["layer"] = None
        lay = default_layer(c["want_anchor"])
    else:
        lay = np.empty((h, w, 4), np.uint8)
        lay[..., :3] = rng.integers(0, 256, (h, w, 3))
        lay[..., 3] = {"a0": 0, "a255": 255}.get(layer, (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 3) % 256)
        c["layer"] = lay
    c["want_rgb"], c["drawn"] = np_render(img2, c["want_map"], lay)
    if h * w >= 64 and not cut:
        # a case that failed these could pass on one branch of the rule alone
        shares = dict(smooth=(branch == SMOOTH).mean(), tear=(branch == TEAR).mean(),
                      lost23=((end == LOST23) | (end == LOSTN)).mean(), colour=(end == LOSTC).mean())
        absent = {UNREACHABLE.get((prev, tear))} | ({"colour"} if thresh >= 765 else set())
        for k, v in shares.items():
            if k in absent:
                assert v == 0, (c["name"], k, v)
            else:
                assert v >= 0.05, (c["name"], k, shares)
    if cut:
        assert same_bits(c["want_map"], np_seed(h, w))
    return c


def _sample(img, s):
    """the bilinear sample of an image at a map, mid-grey where the map is lost (float64 is enough: it only builds image 2)"""
    h, w, _ = img.shape
    with np.errstate(all="ignore"):
        ok = np_known(s[..., 0], s[..., 1])
        qx = np.clip(np.where(ok, s[..., 0], 0).astype(np.float64), 0, w - 1)
        qy = np.clip(np.where(ok, s[..., 1], 0).astype(np.float64), 0, h - 1)
    x0, y0 = np.floor(qx).astype(int), np.floor(qy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = (qx - x0)[..., None], (qy - y0)[..., None]
    a = img.astype(np.float64)
    out = (1 - ay) * ((1 - ax) * a[y0, x0] + ax * a[y0, x1]) + ay * ((1 - ax) * a[y1, x0] + ax * a[y1, x1])
    return np.where(ok[..., None], out, 128.0)


_CASES = None


def cmap_cases():
    """Every case once (built on first use, then shared and never modified): dicts with the inputs of one step and one render and the
    restatement's results (want_map, want_anchor, want_rgb)."""
    global _CASES
    if _CASES is None:
        _CASES = [_case(1000 * i + j, w, h, *cfg) for i, (w, h) in enumerate(SIZES) for j, cfg in enumerate(CONFIGS)]
        drawn = np.concatenate([c["drawn"].ravel() for c in _CASES])
        assert drawn.mean() >= 0.05 and (~drawn).mean() >= 0.05, "the render takes both of its branches"
        for c in _CASES:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _CASES


# Thin frames at kGmMaxDim: map values and bilinear taps at coordinate 8191, vectors that end on the last column / row and one ulp beyond
# them, 32 KiB image rows; pad: pixels beyond every row of the caller's images
LIMIT_SIZES = [(8192, 20), (20, 8192)]
LIMIT_CONFIGS = [CONFIGS[k] for k in (0, 1, 2, 5, 7)]
_LIMIT = None


def cmap_limit_cases():
    global _LIMIT
    if _LIMIT is None:
        _LIMIT = [dict(_case(88000 + 10 * i + j, w, h, *cfg), pad=(0, 3, 64)[j % 3]) for i, (w, h) in enumerate(LIMIT_SIZES)
                  for j, cfg in enumerate(LIMIT_CONFIGS)]
        for c in _LIMIT:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _LIMIT


def host_step(c):
    """case c through the host forms: (map, bytes)"""
    m = io.cmap_step_host(None if c["prev"] == "empty" else c["map"], c["anchor"], c["img2"], c["bu"], c["bv"], c["occ"], c["thresh"], c["tear"],
                          c["use_occ"], c["cut"])
    return m, io.cmap_render_host(m, c["img2"], c["layer"], c["want_anchor"])


# ---- 1. the restatement equals the host forms ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_numpy_restatement_equals_the_host_forms(size):
    cases = [c for c in cmap_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) == len(CONFIGS)
    for c in cases:
        got, rgb = host_step(c)
        assert same_bits(got, c["want_map"]), c["name"]
        assert np.array_equal(rgb, c["want_rgb"]), c["name"]
        if c["cut"]:
            assert same_bits(got, np_seed(c["h"], c["w"]))
        if c["prev"] == "empty":                      # the empty-slot rule is the seed read as the previous map
            again = io.cmap_step_host(np_seed(c["h"], c["w"]), c["anchor"], c["img2"], c["bu"], c["bv"], c["occ"], c["thresh"], c["tear"],
                                      c["use_occ"], c["cut"])
            assert same_bits(again, got)


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_numpy_restatement_equals_the_host_forms_at_the_size_limit(size):
    from test_tfilter_cpu import ends_reached
    w, h = LIMIT_SIZES[size]
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "gmotion.h")).read()
    assert max(w, h) == int(re.search(r"constexpr int kGmMaxDim = (\d+);", src).group(1))
    cases = [c for c in cmap_limit_cases() if (c["w"], c["h"]) == (w, h)]
    assert len(cases) == len(LIMIT_CONFIGS) and {c["pad"] for c in cases} == {0, 3, 64}
    for c in cases:
        got, rgb = host_step(c)
        assert same_bits(got, c["want_map"]), c["name"]
        assert np.array_equal(rgb, c["want_rgb"]), c["name"]
        for axis, reached in ends_reached(c["bu"], c["bv"]).items():
            assert all(reached.values()), (c["name"], axis, reached)
        known = np_known(c["want_map"][..., 0], c["want_map"][..., 1])
        far = c["want_map"][..., 0 if w > h else 1][known]
        assert far.max() > max(w, h) - 2 and far.min() < 1, c["name"]          # the composed map still points at both ends of the long side


def test_seed_and_default_layer():
    """the seed map renders the default layer as the anchor itself, and a layer of alpha 0 as the current frame"""
    rng = np.random.default_rng(3)
    h, w = 9, 13
    anchor, cur = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert same_bits(io.cmap_seed(h, w), np_seed(h, w))
    assert np.array_equal(io.cmap_render_host(np_seed(h, w), cur, None, anchor), anchor)
    clear = np.zeros((h, w, 4), np.uint8)
    clear[..., :3] = 200
    assert np.array_equal(io.cmap_render_host(np_seed(h, w), cur, clear), cur)
    lost = np.full((h, w, 2), LOST)
    assert np.array_equal(io.cmap_render_host(lost, cur, None, anchor), cur)


# ---- 2. ABI: arguments and states ----

def test_header_declares_the_map_and_arguments_are_checked():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    names = ["eppm_cmap_default_params", "eppm_cmap_create", "eppm_cmap_create_size", "eppm_cmap_destroy", "eppm_cmap_reset", "eppm_cmap_step",
             "eppm_cmap_step_frames", "eppm_cmap_get_state", "eppm_cmap_set_state", "eppm_cmap_set_layer", "eppm_cmap_render",
             "eppm_cmap_render_device", "eppm_cmap_age", "eppm_cmap_step_host", "eppm_cmap_render_host"]
    for s in names:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS
    L = eppm_amd.lib()
    p = _lib.CCMapParams()
    assert L.eppm_cmap_default_params(C.byref(p)) == 0 and (p.thresh, p.tear, p.use_occ) == (90.0, 2.0, 1)
    assert L.eppm_cmap_default_params(None) == ARG
    q = eppm_amd.CMapParams(tear=3.0)
    assert (q.thresh, q.tear, q.use_occ) == (90.0, 3.0, 1)
    with pytest.raises(TypeError):
        eppm_amd.CMapParams(n_max=3)
    out = C.c_void_p()
    assert L.eppm_cmap_create(None, None, C.byref(out)) == ARG
    assert L.eppm_cmap_create_size(4, 4, 1, 0, None, None) == ARG
    # section 16's frame bounds
    for h, w, n in ((0, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 4097), (65536, 65536, 1), (8193, 4, 1), (4, 8193, 1), (8192, 8200, 1)):
        assert L.eppm_cmap_create_size(h, w, n, 0, None, C.byref(out)) == ARG and not out.value
    bad = _lib.CCMapParams(90.0, -1.0, 1)
    assert L.eppm_cmap_create_size(4, 4, 1, 0, C.byref(bad), C.byref(out)) == ARG
    assert L.eppm_cmap_destroy(None) == 0
    assert L.eppm_cmap_reset(None, 0) == ARG
    assert L.eppm_cmap_step(None, None, None) == ARG
    assert L.eppm_cmap_step_frames(None, 0, None, None, C.c_size_t(0), None, None, 0) == ARG
    assert L.eppm_cmap_get_state(None, 0, None) == ARG and L.eppm_cmap_set_state(None, 0, None, None, C.c_size_t(0)) == ARG
    assert L.eppm_cmap_set_layer(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_cmap_render(None, 0, None, C.c_size_t(0)) == ARG and L.eppm_cmap_render_device(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_cmap_age(None, 0) == -1
    m, m2 = np_seed(4, 4), np.zeros((4, 4, 2), F)
    rgb, rgb2, lay = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 4), np.uint8)
    z, o = np.zeros((4, 4), F), np.zeros((4, 4), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    good = [C.byref(p), ptr(m2), ptr(m), ptr(rgb), ptr(rgb2), ptr(z), ptr(z), ptr(o)]
    assert L.eppm_cmap_step_host(*good, 4, 4, 0) == 0
    for k in range(len(good)):
        bad = list(good)
        bad[k] = None
        assert (L.eppm_cmap_step_host(*bad, 4, 4, 0) == ARG) == (k != 2), k          # map_in NULL is the seed
    assert L.eppm_cmap_step_host(*good, 4, 0, 0) == ARG and L.eppm_cmap_step_host(*good, 8193, 4, 0) == ARG
    bad = list(good)
    bad[1] = good[2]
    assert L.eppm_cmap_step_host(*bad, 4, 4, 0) == ARG            # the step gathers: not in place
    # the parameter limits
    inf, nan = float("inf"), float("nan")
    for thresh, tear, use_occ, ok in ((0.0, 0.0, 0, True), (1e9, 1e9, 1, True), (3.4e38, 3.4e38, 1, True), (-1.0, 2.0, 1, False),
                                      (inf, 2.0, 1, False), (nan, 2.0, 1, False), (90.0, -0.5, 1, False), (90.0, inf, 1, False),
                                      (90.0, nan, 1, False), (90.0, 2.0, 2, False), (90.0, 2.0, -1, False)):
        pp = _lib.CCMapParams(thresh, tear, use_occ)
        good[0] = C.byref(pp)
        assert (L.eppm_cmap_step_host(*good, 4, 4, 0) == 0) == ok, (thresh, tear, use_occ)
    rgood = [ptr(rgb2), ptr(m), ptr(rgb), ptr(lay), ptr(rgb)]
    assert L.eppm_cmap_render_host(*rgood, 4, 4) == 0
    for k in range(3):
        bad = list(rgood)
        bad[k] = None
        assert L.eppm_cmap_render_host(*bad, 4, 4) == ARG, k
    assert L.eppm_cmap_render_host(rgood[0], rgood[1], rgood[2], None, rgood[4], 4, 4) == 0          # the default layer
    assert L.eppm_cmap_render_host(rgood[0], rgood[1], rgood[2], rgood[3], None, 4, 4) == 0
    assert L.eppm_cmap_render_host(rgood[0], rgood[1], rgood[2], None, None, 4, 4) == ARG
    assert L.eppm_cmap_render_host(*rgood, 0, 4) == ARG
    with pytest.raises(eppm_amd.EppmError):
        io.cmap_step_host(m, rgb, rgb, z, z, o, thresh=-1.0)


def test_no_input_reads_outside_a_plane():
    """maps and vectors of every special value, on planes of their exact size: the host forms return, and a map value outside the frame or
    unknown never becomes a tap"""
    rng = np.random.default_rng(9)
    h, w = 5, 6
    vals = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, 1e9, -1e9, 3e38, -1.0, -1e-45, -0.0, 0.0, w - 1, h - 1, np.nextafter(F(w - 1), F(np.inf)), 1e5], F)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for k in range(20):
        M = vals[rng.integers(0, len(vals), (h, w, 2))]
        bu, bv = vals[rng.integers(0, len(vals), (h, w))], vals[rng.integers(0, len(vals), (h, w))]
        occ = rng.integers(0, 256, (h, w)).astype(np.uint8)
        got = io.cmap_step_host(M, img, img, bu, bv, occ, 1e9, 1e9, k & 1)
        want, _, _ = np_step(M, img, img, bu, bv, occ, 1e9, 1e9, k & 1, False)
        assert same_bits(got, want)
        assert np.array_equal(io.cmap_render_host(M, img, None, img), np_render(img, M, default_layer(img))[0])


def test_arithmetic_under_sanitizers(tmp_path):
    """cmap.h's step and render under ASan + UBSan + float-cast checks on exactly sized planes (tests/csrc/cmap_sanitize_driver.cpp, a
    program of its own, built without HIP)"""
    exe = str(tmp_path / "cmap_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "cmap_sanitize_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- 3. meaning, exact ----

def test_integer_motion_equals_an_integer_chain():
    """moving_clip(96, 128, 8): clean frames, true backward flows, analytic masks, defaults.  The reference is an integer-only chain,
    independent of the bilinear code: known_k[y, x] = ~occ_k & in-frame & known_{k-1}[y + bv, x + bu], anchor_k = anchor_{k-1}[y + bv,
    x + bu].  With whole vectors ax = ay = 0, so bl() returns the weight-1 tap, a lost or torn neighbour falls to the tear case, which
    gives the same value, and the clean frames make d = 0: the known sets are equal and the maps equal the chain's coordinates exactly."""
    h, w = 96, 128
    clean, _, flows, masks = moving_clip(h, w, 8)
    ys, xs = np.mgrid[0:h, 0:w]
    known, ax_, ay_ = np.ones((h, w), bool), xs.copy(), ys.copy()
    M = None
    for k in range(1, 8):
        bu, bv = flows[k - 1]
        M = io.cmap_step_host(M, clean[0], clean[k], bu, bv, masks[k - 1])
        sx, sy = xs + bu.astype(np.int64), ys + bv.astype(np.int64)
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        cx, cy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
        known = (masks[k - 1] == 0) & inside & known[cy, cx]
        ax_, ay_ = ax_[cy, cx], ay_[cy, cx]
        got = np_known(M[..., 0], M[..., 1])
        assert np.array_equal(got, known), f"the known set after step {k}: {int((got != known).sum())} pixels differ"
        assert np.array_equal(M[..., 0][known], ax_[known].astype(F)) and np.array_equal(M[..., 1][known], ay_[known].astype(F)), f"step {k}"
        out = io.cmap_render_host(M, clean[k], None, clean[0])
        assert np.array_equal(out[known], clean[k][known]), f"the default layer after step {k}"
        assert np.array_equal(out[~known], clean[k][~known])
    assert 0.5 < known.mean() < 0.95, known.mean()


# ---- 4. meaning, sub-pixel ----

def subpixel_clip(h, w, nframes, seed=17):
    """a band-limited background (sigma = 2 px) translating by 0.5 px per frame along x, sampled from a canvas of twice the resolution:
    (frames, the true backward flow)"""
    rng = np.random.default_rng(seed)
    hi = _smooth(rng, 2 * h, 2 * (w + nframes), 4.0, 40, 215)
    frames = [np.rint(hi[0:2 * h:2, 2 * nframes - k: 2 * nframes - k + 2 * w: 2]).astype(np.uint8) for k in range(nframes)]
    return frames, (np.full((h, w), -0.5, F), np.zeros((h, w), F))


def psnr_in(a, b, border=8):
    d = a[border:-border, border:-border].astype(np.float64) - b[border:-border, border:-border].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / np.mean(d ** 2))


def test_composed_map_beats_warping_frame_to_frame():
    """8 frames moving by 0.5 px: the render of the composed map resamples the anchor once, warping the anchor frame to frame resamples
    it seven times with the same bilinear taps.  Only asserted: the map form is the closer of the two to the current clean frame.
    Measured: map form 50.67 dB, frame to frame 37.00 dB."""
    h, w = 96, 128
    frames, (bu, bv) = subpixel_clip(h, w, 8)
    occ = np.zeros((h, w), np.uint8)
    M, warped = None, frames[0]
    one_step = io.cmap_step_host(None, frames[0], frames[0], bu, bv, occ, thresh=1e9)          # the map of a single step: the same taps
    for k in range(1, 8):
        M = io.cmap_step_host(M, frames[0], frames[k], bu, bv, occ)
        warped = io.cmap_render_host(one_step, warped, None, warped)
    out = io.cmap_render_host(M, frames[7], None, frames[0])
    known = np_known(M[..., 0], M[..., 1])
    assert known[8:-8, 8:-8].all()
    composed, chained = psnr_in(out, frames[7]), psnr_in(warped, frames[7])
    print(f"map form {composed:.2f} dB, frame to frame {chained:.2f} dB")
    assert composed > chained
