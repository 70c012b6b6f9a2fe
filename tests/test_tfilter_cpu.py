"""CPU tests of the motion-compensated temporal filter: the ABI's argument checks, a numpy restatement of the
per-pixel rule against eppm_tfilter_step_host bit for bit on the shared generator tfilter_cases() (the GPU tests run the kernel on the same
cases), and what the filter means on a static and on a moving scene."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io

F = np.float32
ARG, STATE = 1, 3


# ---- the numpy restatement of section 15 ----

def np_seed(img):
    h, w, _ = img.shape
    acc = np.empty((h, w, 4), F)
    acc[..., :3] = img.astype(F)
    acc[..., 3] = F(1)
    return acc


def np_bytes(acc):
    with np.errstate(all="ignore"):
        return np.floor(np.fmin(np.fmax(acc[..., :3], F(0)), F(255)) + F(0.5)).astype(np.uint8)


def np_step(acc, img2, bu, bv, occ, thresh, n_max, cut):
    """(new state, bytes, blend mask): every operation one float32 rounding, in the order of section 15."""
    h, w = bu.shape
    cur = img2.astype(F)
    with np.errstate(all="ignore"):
        known = (np.abs(bu) <= F(1e9)) & (np.abs(bv) <= F(1e9))
        qx = np.arange(w, dtype=F)[None, :] + bu
        qy = np.arange(h, dtype=F)[:, None] + bv
        inside = (qx >= F(0)) & (qx <= F(w - 1)) & (qy >= F(0)) & (qy <= F(h - 1))
        ok = known & inside & (occ == 0) & (not cut)
        qx = np.where(ok, qx, F(0))
        qy = np.where(ok, qy, F(0))
        x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (qx - x0.astype(F))[..., None], (qy - y0.astype(F))[..., None]
        bx, by = F(1) - ax, F(1) - ay
        a00, a01, a10, a11 = acc[y0, x0, :3], acc[y0, x1, :3], acc[y1, x0, :3], acc[y1, x1, :3]
        p = by * (bx * a00 + ax * a01) + ay * (bx * a10 + ax * a11)
        assert p.dtype == F
        n_prev = acc[np.floor(qy + F(0.5)).astype(np.int64), np.floor(qx + F(0.5)).astype(np.int64), 3]
        d = (np.abs(cur[..., 0] - p[..., 0]) + np.abs(cur[..., 1] - p[..., 1])) + np.abs(cur[..., 2] - p[..., 2])
        blend = ok & (d <= F(thresh))
        n = np.fmin(n_prev + F(1), F(n_max))
        out = np.empty((h, w, 4), F)
        out[..., :3] = np.where(blend[..., None], p + (cur - p) / n[..., None], cur)
        out[..., 3] = np.where(blend, n, F(1))
    return out, np_bytes(out), blend


# ---- the shared cases ----

SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157)]           # w x h
# (state, thresh, n_max, cut): state "seeded" / "stepped" (three steps of the restatement) / "nmax" (n = n_max everywhere) / "empty"
CONFIGS = [("seeded", 1e9, 8, False), ("stepped", 1e9, 8, False), ("nmax", 1e9, 8, False), ("seeded", 0.0, 8, False),
           ("stepped", 40.0, 255, False), ("stepped", 1e9, 1, False), ("nmax", 40.0, 255, False), ("empty", 1e9, 8, False),
           ("stepped", 1e9, 8, True), ("empty", 40.0, 8, True)]


def _vectors(rng, h, w, integer_share):
    """backward vectors: ~70 % land inside the frame (integer or fractional), the rest are the special ones"""
    ys, xs = np.mgrid[0:h, 0:w]
    tx, ty = rng.uniform(0, w - 1, (h, w)), rng.uniform(0, h - 1, (h, w))
    whole = rng.random((h, w)) < integer_share
    tx, ty = np.where(whole, np.rint(tx), tx), np.where(whole, np.rint(ty), ty)
    bu, bv = (tx - xs).astype(F), (ty - ys).astype(F)
    kind = rng.integers(0, 40, (h, w))
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


def _case(seed, w, h, state, thresh, n_max, cut):
    rng = np.random.default_rng(seed)
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    integer_share = 0.9 if thresh == 0.0 else 0.4
    if state in ("seeded", "empty"):
        acc = np_seed(img1)
    elif state == "nmax":
        acc = np.empty((h, w, 4), F)
        acc[..., :3] = rng.uniform(0, 255, (h, w, 3)).astype(F)
        acc[..., 3] = F(n_max)
    else:
        acc = np_seed(img1)
        for _ in range(3):
            bu, bv = _vectors(rng, h, w, 0.4)
            acc, _, _ = np_step(acc, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), bu, bv, np.zeros((h, w), np.uint8), 1e9, n_max, False)
    bu, bv = _vectors(rng, h, w, integer_share)
    occ = np.where(rng.random((h, w)) < 0.7, 0, rng.integers(0, 4, (h, w))).astype(np.uint8)        # bytes 0..3, zero most often
    # image 2: the compensated previous state plus noise, so that the comparison goes both ways at every threshold
    _, _, reach = np_step(acc, np.zeros((h, w, 3), np.uint8), bu, bv, np.zeros((h, w), np.uint8), 1e9, n_max, False)
    base = np.where(reach[..., None], _sample(acc, bu, bv), rng.uniform(0, 255, (h, w, 3)))
    amp = {0.0: 0, 40.0: 25}.get(thresh, 60)
    noise = rng.integers(-amp, amp + 1, (h, w, 3)) * (rng.random((h, w, 1)) < 0.6)
    img2 = np.clip(np.rint(base) + noise, 0, 255).astype(np.uint8)
    c = dict(name=f"{w}x{h}-{state}-t{thresh:g}-n{n_max}{'-cut' if cut else ''}", h=h, w=w, state=state, acc=acc, img1=img1, img2=img2, bu=bu, bv=bv,
             occ=occ, thresh=thresh, n_max=n_max, cut=cut)
    c["want_acc"], c["want_rgb"], blend = np_step(acc, img2, bu, bv, occ, thresh, n_max, cut)
    if h * w >= 64 and not cut:
        # a case that failed these could pass on resets (or on blends) alone
        share = blend.mean()
        assert share >= 0.10, (c["name"], "blend share", share)
        assert 1.0 - share >= 0.10, (c["name"], "reset share", 1.0 - share)
    if cut:
        assert not blend.any()
    return c


def _sample(acc, bu, bv):
    """the bilinear sample of the state where the vector reaches the frame (float64 is enough: it only builds image 2)"""
    h, w = bu.shape
    with np.errstate(all="ignore"):
        qx = np.clip(np.nan_to_num(np.arange(w)[None, :] + bu.astype(np.float64), nan=0.0), 0, w - 1)
        qy = np.clip(np.nan_to_num(np.arange(h)[:, None] + bv.astype(np.float64), nan=0.0), 0, h - 1)
    x0, y0 = np.floor(qx).astype(int), np.floor(qy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = (qx - x0)[..., None], (qy - y0)[..., None]
    a = acc[..., :3].astype(np.float64)
    return (1 - ay) * ((1 - ax) * a[y0, x0] + ax * a[y0, x1]) + ay * ((1 - ax) * a[y1, x0] + ax * a[y1, x1])


_CASES = None


def tfilter_cases():
    """Every case once (built on first use, then shared and never modified): dicts with the inputs of one step and the restatement's
    result (want_acc, want_rgb)."""
    global _CASES
    if _CASES is None:
        _CASES = [_case(1000 * i + j, w, h, *cfg) for i, (w, h) in enumerate(SIZES) for j, cfg in enumerate(CONFIGS)]
        for c in _CASES:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _CASES


# Thin frames at 8192, section 16's bound, which the objects chained with the filter obey (its own check, h*w < 2^31, lies far beyond):
# taps at x = 8191 / y = 8191, 32 KiB image rows, and image planes whose pitch is larger than 4 * w (pad: pixels beyond every row)
LIMIT_SIZES = [(8192, 20), (20, 8192)]
LIMIT_CONFIGS = [("stepped", 40.0, 255, False), ("empty", 1e9, 8, False), ("nmax", 40.0, 255, False), ("seeded", 0.0, 8, False)]
_LIMIT = None


def tfilter_limit_cases():
    global _LIMIT
    if _LIMIT is None:
        _LIMIT = [dict(_case(77000 + 10 * i + j, w, h, *cfg), pad=(0, 3, 64)[j % 3]) for i, (w, h) in enumerate(LIMIT_SIZES)
                  for j, cfg in enumerate(LIMIT_CONFIGS)]
        for c in _LIMIT:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _LIMIT


def ends_reached(bu, bv):
    """what a case's vectors reach on a frame: a target exactly on the last column / row from a pixel of the first ones and of the last
    ones, one within a pixel beyond them, and one exactly on coordinate 0 -- in x and in y"""
    h, w = bu.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = xs.astype(F) + bu, ys.astype(F) + bv
    out = {}
    for name, q, pos, n in (("x", qx, xs, w), ("y", qy, ys, h)):
        out[name] = dict(last=bool((q == F(n - 1)).any()), last_from_far=bool(((q == F(n - 1)) & (pos < n // 8)).any()),
                         first_from_far=bool(((q >= 0) & (q < 1) & (pos >= n - n // 8)).any()),
                         beyond=bool(((q > F(n - 1)) & (q < F(n))).any()), zero=bool(((q == 0) & (pos > 0)).any()))
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1. ABI ----

def test_header_declares_the_filter_and_arguments_are_checked():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    names = ["eppm_tfilter_default_params", "eppm_tfilter_create", "eppm_tfilter_create_size", "eppm_tfilter_destroy", "eppm_tfilter_reset", "eppm_tfilter_step",
             "eppm_tfilter_step_frames", "eppm_tfilter_get", "eppm_tfilter_get_device", "eppm_tfilter_get_state", "eppm_tfilter_set_state",
             "eppm_tfilter_seed_host", "eppm_tfilter_step_host"]
    for s in names:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS
    L = eppm_amd.lib()
    p = _lib.CTFilterParams()
    assert L.eppm_tfilter_default_params(C.byref(p)) == 0 and (p.thresh, p.n_max) == (40.0, 8)
    assert L.eppm_tfilter_default_params(None) == ARG
    out = C.c_void_p()
    assert L.eppm_tfilter_create(None, None, C.byref(out)) == ARG
    assert L.eppm_tfilter_create_size(4, 4, 1, 0, None, None) == ARG
    for h, w, n in ((0, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 4097), (65536, 65536, 1)):
        assert L.eppm_tfilter_create_size(h, w, n, 0, None, C.byref(out)) == ARG and not out.value
    bad = _lib.CTFilterParams(40.0, 0)
    assert L.eppm_tfilter_create_size(4, 4, 1, 0, C.byref(bad), C.byref(out)) == ARG
    assert L.eppm_tfilter_destroy(None) == 0
    assert L.eppm_tfilter_reset(None, 0) == ARG
    assert L.eppm_tfilter_step(None, None, None) == ARG
    assert L.eppm_tfilter_step_frames(None, 0, None, None, C.c_size_t(0), None, None, 0) == ARG
    assert L.eppm_tfilter_get(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_tfilter_get_device(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_tfilter_get_state(None, 0, None) == ARG and L.eppm_tfilter_set_state(None, 0, None) == ARG
    assert L.eppm_tfilter_seed_host(None, None, 4, 4) == ARG
    acc, acc2 = np.zeros((4, 4, 4), F), np.zeros((4, 4, 4), F)
    rgb, rgb2 = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)
    z, o = np.zeros((4, 4), F), np.zeros((4, 4), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    assert L.eppm_tfilter_seed_host(ptr(acc), ptr(rgb), 0, 4) == ARG and L.eppm_tfilter_seed_host(ptr(acc), None, 4, 4) == ARG
    good = [C.byref(p), ptr(acc2), ptr(rgb2), ptr(acc), ptr(rgb), ptr(z), ptr(z), ptr(o)]
    assert L.eppm_tfilter_step_host(*good, 4, 4, 0) == 0
    for k in range(len(good)):
        bad = list(good)
        bad[k] = None
        assert L.eppm_tfilter_step_host(*bad, 4, 4, 0) == ARG, k
    assert L.eppm_tfilter_step_host(*good, 4, 0, 0) == ARG
    bad = list(good)
    bad[1] = good[3]
    assert L.eppm_tfilter_step_host(*bad, 4, 4, 0) == ARG            # the step gathers: not in place
    # the parameter limits
    for thresh, n_max, ok in ((0.0, 1, True), (1e9, 255, True), (3.4e38, 8, True), (-1.0, 8, False), (float("inf"), 8, False),
                              (float("nan"), 8, False), (40.0, 0, False), (40.0, 256, False), (40.0, -3, False)):
        q = _lib.CTFilterParams(thresh, n_max)
        good[0] = C.byref(q)
        assert (L.eppm_tfilter_step_host(*good, 4, 4, 0) == 0) == ok, (thresh, n_max)
    with pytest.raises(eppm_amd.EppmError):
        io.tfilter_step_host(acc, rgb, z, z, o, thresh=-1.0)


# ---- 2. the restatement equals the host form ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_numpy_restatement_equals_the_host_form(size):
    cases = [c for c in tfilter_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) == len(CONFIGS)
    for c in cases:
        acc = c["acc"]
        if c["state"] == "empty":                     # the empty-slot rule: the seed of image 1, then the step
            acc = io.tfilter_seed_host(c["img1"])
            assert same_bits(acc, np_seed(c["img1"]))
        got, rgb = io.tfilter_step_host(acc, c["img2"], c["bu"], c["bv"], c["occ"], c["thresh"], c["n_max"], c["cut"])
        assert same_bits(got, c["want_acc"]), c["name"]
        assert np.array_equal(rgb, c["want_rgb"]), c["name"]
        if c["cut"]:
            assert np.array_equal(rgb, c["img2"]) and (got[..., 3] == 1).all()


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_numpy_restatement_equals_the_host_form_at_the_size_limit(size):
    cases = [c for c in tfilter_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) == len(LIMIT_CONFIGS) and {c["pad"] for c in cases} == {0, 3, 64}
    for c in cases:
        acc = io.tfilter_seed_host(c["img1"]) if c["state"] == "empty" else c["acc"]
        got, rgb = io.tfilter_step_host(acc, c["img2"], c["bu"], c["bv"], c["occ"], c["thresh"], c["n_max"], c["cut"])
        assert same_bits(got, c["want_acc"]) and np.array_equal(rgb, c["want_rgb"]), c["name"]
        for axis, reached in ends_reached(c["bu"], c["bv"]).items():
            assert all(reached.values()), (c["name"], axis, reached)


def test_output_byte_is_total():
    """any state gives a byte: NaN -> 0, +-inf and out-of-range values clamp"""
    acc = np.zeros((1, 7, 4), F)
    acc[0, :, 0] = [np.nan, np.inf, -np.inf, -3.0, 255.4, 255.6, 127.5]
    acc[0, :, 3] = 1
    zero = np.zeros((1, 7), F)
    # n_max 1 and thresh 1e9 at zero motion: out = p + (cur - p) / 1
    _, rgb = io.tfilter_step_host(acc, np.full((1, 7, 3), 9, np.uint8), zero, zero, np.zeros((1, 7), np.uint8), 1e9, 1)
    assert rgb[0, 0, 0] == 9 and rgb[0, 1, 0] == 9 and rgb[0, 3, 0] == 9          # NaN / inf samples fail d <= thresh or give cur
    got, _ = io.tfilter_step_host(acc, np.full((1, 7, 3), 9, np.uint8), zero, zero, np.ones((1, 7), np.uint8), 1e9, 1)
    assert (got[..., :3] == 9).all()
    assert np.array_equal(np_bytes(acc)[0, :, 0], [0, 255, 0, 0, 255, 255, 128])


# ---- 3. meaning, static ----

def test_static_scene_is_the_running_mean():
    rng = np.random.default_rng(5)
    h, w, n_max = 24, 40, 8
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n_max)]
    zero, occ = np.zeros((h, w), F), np.zeros((h, w), np.uint8)
    acc = io.tfilter_seed_host(frames[0])
    for k in range(1, n_max):
        acc, rgb = io.tfilter_step_host(acc, frames[k], zero, zero, occ, 1e9, n_max)
        mean = np.mean([f.astype(np.float64) for f in frames[:k + 1]], axis=0)
        assert np.abs(acc[..., :3] - mean).max() <= 1e-3
        assert (acc[..., 3] == k + 1).all()
        assert np.abs(rgb.astype(np.float64) - mean).max() <= 0.5 + 1e-3
    acc, rgb = io.tfilter_step_host(acc, frames[0], zero, zero, occ, 1e9, n_max, cut=True)
    assert np.array_equal(rgb, frames[0]) and (acc[..., 3] == 1).all() and same_bits(acc, np_seed(frames[0]))


# ---- 4. meaning, moving ----

def _smooth(rng, h, w, sigma, lo, hi):
    """band-limited noise in [lo, hi]: white noise under a separable Gaussian"""
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = rng.standard_normal((h + 2 * r, w + 2 * r, 3))
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, a)
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, a)
    a = (a - a.min()) / (a.max() - a.min())
    return lo + (hi - lo) * a


def moving_clip(h, w, nframes, seed=11, sigma=5.0, bg_v=(2, 1), sq_v=(-1, 2), sq=24):
    """(clean frames, noisy frames, backward flows (bu, bv), occ2 masks): a band-limited background translating by bg_v = (dx, dy) per frame
    and a textured sq x sq square moving by sq_v over it; the masks are the analytic disocclusions (background the square uncovers)."""
    rng = np.random.default_rng(seed)
    pad = nframes * max(abs(bg_v[0]), abs(bg_v[1]), 1)
    canvas = _smooth(rng, h + 2 * pad, w + 2 * pad, 2.0, 40, 215)
    tex = _smooth(rng, sq, sq, 1.2, 30, 225)
    sx0, sy0 = w // 2, h // 4
    ys, xs = np.mgrid[0:h, 0:w]
    clean, inside = [], []
    for k in range(nframes):
        f = canvas[pad - k * bg_v[1]: pad - k * bg_v[1] + h, pad - k * bg_v[0]: pad - k * bg_v[0] + w].copy()
        sx, sy = sx0 + k * sq_v[0], sy0 + k * sq_v[1]
        f[sy:sy + sq, sx:sx + sq] = tex
        m = np.zeros((h, w), bool)
        m[sy:sy + sq, sx:sx + sq] = True
        clean.append(np.rint(f).astype(np.uint8))
        inside.append(m)
    noisy = [np.clip(np.rint(c + rng.normal(0, sigma, c.shape)), 0, 255).astype(np.uint8) for c in clean]
    flows, masks = [], []
    for k in range(1, nframes):
        bu = np.where(inside[k], -sq_v[0], -bg_v[0]).astype(F)
        bv = np.where(inside[k], -sq_v[1], -bg_v[1]).astype(F)
        srcx, srcy = np.clip(xs - bg_v[0], 0, w - 1), np.clip(ys - bg_v[1], 0, h - 1)
        masks.append((~inside[k] & inside[k - 1][srcy, srcx]).astype(np.uint8))
        flows.append((bu, bv))
    return clean, noisy, flows, masks


def psnr(a, b, border=8):
    d = a[border:-border, border:-border].astype(np.float64) - b[border:-border, border:-border].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / np.mean(d ** 2))


def host_filter(noisy, flows, masks, thresh=40.0, n_max=8):
    """the host form along a clip: (outputs, last state)"""
    acc = io.tfilter_seed_host(noisy[0])
    out = [noisy[0]]
    for k in range(1, len(noisy)):
        acc, rgb = io.tfilter_step_host(acc, noisy[k], *flows[k - 1], masks[k - 1], thresh, n_max)
        out.append(rgb)
    return out, acc


def test_moving_scene_gains_6_db():
    """96x128, 8 frames, sigma 5, true flows, defaults.  Pixels averaged over 8 frames gain 10 log10(8) = 9.0 dB; about 6 % reset every frame
    (entering border, disocclusion), which leaves 0.94 / 8 + 0.06 = 0.1775 of the noise power: +7.5 dB.  The bar is 6 dB; measured 34.21 -> 42.42 dB, +8.2 dB (the
    8-px border that is left out holds most of the resets)."""
    clean, noisy, flows, masks = moving_clip(128, 96, 8)
    out, acc = host_filter(noisy, flows, masks)
    before, after = psnr(noisy[-1], clean[-1]), psnr(out[-1], clean[-1])
    fresh = float((acc[8:-8, 8:-8, 3] == 1).mean())
    print(f"noisy {before:.2f} dB, filtered {after:.2f} dB, gain {after - before:.2f} dB, interior pixels at n = 1: {100 * fresh:.1f} %")
    assert after >= before + 6.0
