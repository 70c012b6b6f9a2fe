"""CPU tests of film-defect removal: the ABI's argument checks, a vectorised numpy restatement of the arithmetic
against eppm_defect_step_host byte for byte on the shared generator defect_cases() (the GPU tests run the kernels on the same cases), and
what the filter means on a moving clip with planted blotches and true flows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io, synth

F = np.float32
ARG, STATE = 1, 3
DEFAULTS = dict(detect=60.0, agree=30.0, radius=3, grow=1)


# ---- the numpy restatement of section 23 ----

def np_known(vx, vy):
    with np.errstate(all="ignore"):
        return (np.abs(vx) <= F(1e9)) & (np.abs(vy) <= F(1e9))


def np_sample(img, vx, vy):
    """(sample (h, w, 3) float32, valid (h, w)): every operation one float32 rounding, in the order of section 23"""
    h, w = vx.shape
    a = img.astype(F)
    with np.errstate(all="ignore"):
        qx = np.arange(w, dtype=F)[None, :] + vx
        qy = np.arange(h, dtype=F)[:, None] + vy
        ok = np_known(vx, vy) & (qx >= F(0)) & (qx <= F(w - 1)) & (qy >= F(0)) & (qy <= F(h - 1))
        qx, qy = np.where(ok, qx, F(0)), np.where(ok, qy, F(0))
        x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (qx - x0.astype(F))[..., None], (qy - y0.astype(F))[..., None]
        bx, by = F(1) - ax, F(1) - ay
        s = by * (bx * a[y0, x0] + ax * a[y0, x1]) + ay * (bx * a[y1, x0] + ax * a[y1, x1])
    assert s.dtype == F
    return s, ok


def np_dist(a, b):
    return (np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])) + np.abs(a[..., 2] - b[..., 2])


def np_chance(prev, cur, nxt, bvx, bvy, fvx, fvy, detect, agree):
    """(decided, hit, replacement bytes) of one chance"""
    p, okp = np_sample(prev, bvx, bvy)
    n, okn = np_sample(nxt, fvx, fvy)
    c = cur.astype(F)
    decided = okp & okn & (np_dist(p, n) <= F(agree))
    hit = decided & (np_dist(c, p) > F(detect)) & (np_dist(c, n) > F(detect))
    repl = np.floor(np.fmin(np.fmax((p + n) * F(0.5), F(0)), F(255)) + F(0.5)).astype(np.uint8)
    return decided, hit, repl


def np_windows(plane, r, fill=None):
    """the (2r+1)^2 shifted copies of a plane, coordinates clamped to the frame (fill: a constant outside instead)"""
    h, w = plane.shape
    pad = np.pad(plane, r, mode="edge") if fill is None else np.pad(plane, r, mode="constant", constant_values=fill)
    return np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])


def np_median(plane, r):
    """the lower median of every window: element (n - 1) / 2 of the ascending order"""
    win = np.sort(np_windows(plane, r), axis=0)
    return win[(win.shape[0] - 1) // 2]


def np_step(prev, cur, nxt, bu, bv, fu, fv, detect=60.0, agree=30.0, radius=3, grow=1):
    """(rgb, mask, stats, code) of one step; prev or nxt None: the passing step"""
    h, w, _ = cur.shape
    code = np.zeros((h, w), np.uint8)
    repl = cur.copy()
    if prev is not None and nxt is not None:
        d1, h1, r1 = np_chance(prev, cur, nxt, bu, bv, fu, fv, detect, agree)
        d2, h2, r2 = np.zeros((h, w), bool), np.zeros((h, w), bool), cur
        if radius > 0:
            known = np_known(fu, fv) & np_known(bu, bv)
            has_median = np_windows(known, radius).all(axis=0)
            med = [np.where(has_median, np_median(np.where(known, v, F(0)), radius), F(np.nan)) for v in (bu, bv, fu, fv)]
            d2, h2, r2 = np_chance(prev, cur, nxt, *med, detect, agree)
            d2, h2 = d2 & ~d1, h2 & ~d1
        und = ~d1 & ~d2
        code = (np.where(d1, h1, h2).astype(np.uint8) | (d2.astype(np.uint8) << 1) | (und.astype(np.uint8) << 2)).astype(np.uint8)
        repl = np.where(d1[..., None], r1, np.where(d2[..., None], r2, cur))
    hit = (code & 1) != 0
    near = np_windows(hit, grow, fill=False).any(axis=0)
    mask = np.where(hit, 1, np.where(((code & 4) == 0) & near, 2, 0)).astype(np.uint8)
    out = np.where((mask != 0)[..., None], repl, cur).astype(np.uint8)
    stats = dict(hit=int((mask == 1).sum()), grown=int((mask == 2).sum()), second_chance=int(((code & 2) != 0).sum()),
                 undecided=int(((code & 4) != 0).sum()))
    return out, mask, stats, code


# ---- the shared cases ----

SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157)]           # w x h
# random cases: (detect, agree, radius, grow, passing) -- passing: None, "prev" or "next" is NULL
RANDOM = [(60.0, 30.0, 3, 1, None), (0.0, 0.0, 1, 1, None), (1e9, 1e9, 3, 0, None), (0.0, 1e9, 4, 4, None), (60.0, 1e9, 0, 1, None),
          (60.0, 30.0, 3, 1, "prev"), (60.0, 30.0, 3, 1, "next")]
# planted cases at the default thresholds: (radius, grow)
PLANTED = [(3, 1), (1, 0), (4, 4), (0, 1), (4, 1)]


def _vectors(rng, h, w):
    """vectors into a frame: ~60 % land inside (integer or fractional), the rest are the special ones"""
    ys, xs = np.mgrid[0:h, 0:w]
    tx, ty = rng.uniform(0, w - 1, (h, w)), rng.uniform(0, h - 1, (h, w))
    whole = rng.random((h, w)) < 0.4
    tx, ty = np.where(whole, np.rint(tx), tx), np.where(whole, np.rint(ty), ty)
    u, v = (tx - xs).astype(F), (ty - ys).astype(F)
    kind = rng.integers(0, 40, (h, w))
    xf, yf = xs.astype(F), ys.astype(F)
    up = lambda a: np.nextafter(F(a), F(np.inf))                          # noqa: E731
    special = {
        0: (F(w - 1) - xf, v), 1: (u, F(h - 1) - yf), 2: (F(w - 1) - xf, F(h - 1) - yf),            # exactly on the last column / row
        3: (up(w - 1) - xf, v), 4: (u, up(h - 1) - yf),                                             # one ulp outside (where the sum is exact)
        5: (-xf - F(1e-45), v), 6: (u, -yf - F(1e-45)),                                             # just below 0 (x = 0 / y = 0: a denormal)
        7: (np.full((h, w), F(1e10)), v), 8: (u, np.full((h, w), F(-1e10))),
        9: (np.full((h, w), F(np.inf)), v), 10: (u, np.full((h, w), F(-np.inf))),
        11: (np.full((h, w), F(np.nan)), v), 12: (u, np.full((h, w), F(np.nan))),
        13: (np.full((h, w), F(-0.0)), np.full((h, w), F(-0.0))),
        14: (u + F(w), v), 15: (u, v - F(h)),                                                       # plainly outside
    }
    for k, (su, sv) in special.items():
        u = np.where(kind == k, su, u).astype(F)
        v = np.where(kind == k, sv, v).astype(F)
    return u, v


def _random_case(seed, w, h, detect, agree, radius, grow, passing):
    rng = np.random.default_rng(seed)
    flat = lambda: np.clip(128 + rng.integers(-9, 10, (h, w, 3)), 0, 255).astype(np.uint8)      # noqa: E731
    prev, nxt = flat(), flat()
    cur = np.where(rng.random((h, w, 1)) < 0.5, flat(), rng.integers(0, 256, (h, w, 3))).astype(np.uint8)
    bu, bv = _vectors(rng, h, w)
    fu, fv = _vectors(rng, h, w)
    # unknown vectors are rare enough to leave windows without one: clear most of them in one half of the frame
    if w * h >= 64:
        calm = (np.mgrid[0:h, 0:w][1] < w // 2) & (rng.random((h, w)) < 0.97)
        for a in (bu, bv, fu, fv):
            a[calm & ~(np.abs(a) <= F(1e9))] = F(0.25)
    c = dict(name=f"random-{w}x{h}-d{detect:g}-a{agree:g}-r{radius}-g{grow}{'-no' + passing if passing else ''}", h=h, w=w,
             prev=None if passing == "prev" else prev, cur=cur, next=None if passing == "next" else nxt, bu=bu, bv=bv, fu=fu, fv=fv,
             params=dict(detect=detect, agree=agree, radius=radius, grow=grow), planted=False)
    return c


def _smooth(rng, h, w):
    base = synth._octave_noise(rng, h, w)
    chans = []
    for _ in range(3):
        c = 0.7 * base + 0.3 * synth._octave_noise(rng, h, w)
        chans.append((c - c.mean()) / (c.std() + 1e-9) * 47.0 + 110.0)
    return np.stack(chans, -1)


def _planted_case(seed, w, h, radius, grow):
    """the neighbours are integer shifts of one smooth image, cur carries blotches; own vectors are true, except salted wrong at
    isolated pixels (the median rescues them), all wrong in one block of columns (undecided) and unknown at a few pixels"""
    rng = np.random.default_rng(seed)
    m = 4
    big = _smooth(rng, h + 2 * m, w + 2 * m)
    sp, sn = ((2, 1), (-2, -1)) if h >= 8 else ((2, 0), (-1, 0))           # (dx, dy): cur(x, y) = prev(x + dx, y + dy); likewise next
    if w < 8:
        sp, sn = (0, sp[1]), (0, sn[1])
    cut = lambda dx, dy: big[m - dy:m - dy + h, m - dx:m - dx + w]         # noqa: E731
    noisy = lambda a: np.clip(np.rint(a) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)   # noqa: E731
    prev, clean, nxt = noisy(cut(*sp)), noisy(cut(0, 0)), noisy(cut(*sn))
    cur = clean.copy()
    blotch = np.zeros((h, w), bool)
    for _ in range(max(1, h * w // 9)):
        y, x, s = rng.integers(0, h), rng.integers(0, w), rng.integers(1, 4)
        blotch[y:y + s, x:x + s] = True
    cur[blotch] = np.where(rng.random((int(blotch.sum()), 1)) < 0.5, 8, 250)
    bu, bv = np.full((h, w), F(sp[0])), np.full((h, w), F(sp[1]))
    fu, fv = np.full((h, w), F(sn[0])), np.full((h, w), F(sn[1]))
    ys, xs = np.mgrid[0:h, 0:w]
    salt = rng.random((h, w)) < 0.25
    block = (xs >= w // 10) & (xs < w // 10 + max(1, (w * 18) // 100)) if w >= 8 else (ys < max(1, h // 5))
    wrong = salt | block
    which = rng.integers(0, 3, (h, w))                                     # the backward vector, the forward vector or both
    which = np.where(block, 2, which)
    far = block | (rng.random((h, w)) < 0.7)                               # plainly outside (all of the block), or a wrong offset
    off_u = np.where(far, F(w + 3), rng.choice([-9, -7, -5, 5, 7, 9], (h, w)) + rng.random((h, w))).astype(F)
    off_v = np.where(far, F(0), rng.choice([-6, -4, 4, 6], (h, w)) + rng.random((h, w))).astype(F)
    for (u, v), sel in (((bu, bv), which != 1), ((fu, fv), which != 0)):
        u[wrong & sel] += off_u[wrong & sel]
        v[wrong & sel] += off_v[wrong & sel]
    lost = rng.random((h, w)) < 0.0015
    bu[lost] = F(np.nan)
    return dict(name=f"planted-{w}x{h}-r{radius}-g{grow}", h=h, w=w, prev=prev, cur=cur, next=nxt, bu=bu, bv=bv, fu=fu, fv=fv,
                params=dict(DEFAULTS, radius=radius, grow=grow), planted=True)


def _finish(c):
    c["want_rgb"], c["want_mask"], c["want_stats"], code = np_step(c["prev"], c["cur"], c["next"], c["bu"], c["bv"], c["fu"], c["fv"], **c["params"])
    n = c["h"] * c["w"]
    if c["planted"] and n >= 64 and c["params"]["radius"] > 0:
        # a case that failed these could pass on one path alone
        shares = {"chance-1 hit": (code == 1).mean(), "chance-1 decided, not hit": (code == 0).mean(),
                  "chance-2 decided": ((code & 2) != 0).mean(), "undecided": ((code & 4) != 0).mean()}
        for k, v in shares.items():
            assert v >= 0.10, (c["name"], k, v)
        if c["params"]["grow"] > 0:
            assert (c["want_mask"] == 2).mean() >= 0.02, (c["name"], "grown", (c["want_mask"] == 2).mean())
    if c["prev"] is None or c["next"] is None:
        assert not c["want_mask"].any() and not any(c["want_stats"].values()) and np.array_equal(c["want_rgb"], c["cur"])
    return c


_CASES = None


def defect_cases():
    """Every case once (built on first use, then shared and never modified): dicts with the inputs of one step and the restatement's
    result (want_rgb, want_mask, want_stats)."""
    global _CASES
    if _CASES is None:
        cases = []
        for i, (w, h) in enumerate(SIZES):
            cases += [_random_case(1000 * i + j, w, h, *cfg) for j, cfg in enumerate(RANDOM)]
            cases += [_planted_case(1000 * i + 500 + j, w, h, *cfg) for j, cfg in enumerate(PLANTED)]
        _CASES = [_finish(c) for c in cases]
        for c in _CASES:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _CASES


# Thin frames 8192 long: section 16's bound, which the objects chained with the filter obey (its own check, h*w < 2^31, lies far beyond):
# taps and median windows at coordinate 8191, 32 KiB image rows; pad: pixels beyond every row of the caller's images
LIMIT_SIZES = [(8192, 20), (20, 8192)]
_LIMIT = {}


def defect_limit_cases(size=None):
    """the cases of LIMIT_SIZES[size], or of both sizes; built on first use"""
    if size is None:
        return defect_limit_cases(0) + defect_limit_cases(1)
    if size not in _LIMIT:
        w, h = LIMIT_SIZES[size]
        cases = [_random_case(66000 + 10 * size + j, w, h, *RANDOM[k]) for j, k in enumerate((0, 1, 5))]
        cases += [_planted_case(66500 + 10 * size + j, w, h, *PLANTED[k]) for j, k in enumerate((0, 1))]
        _LIMIT[size] = [dict(_finish(c), pad=(0, 3, 64)[j % 3]) for j, c in enumerate(cases)]
        for c in _LIMIT[size]:
            for v in c.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _LIMIT[size]


def host_step(c):
    return io.defect_step_host(c["prev"], c["cur"], c["next"], c["bu"], c["bv"], c["fu"], c["fv"], **c["params"])


# ---- the clip of the meaning tests (also tests/test_defect_gpu.py) ----

def blotch_clip(seed=7, n=5, h=128, w=160, sigma=3.0, blotched=(1, 2, 3), count=25, rmax=3):
    """(frames with blotches, clean frames (no blotch, no noise), blotch masks, true flows): a band-limited background that moves (2, 1) per frame, a textured
    40 x 40 square that moves (-1, 2), Gaussian noise; `count` elliptical blotches of value 8 or 250 and radii up to rmax in the frames
    `blotched`.  flows[k] = (bu, bv, fu, fv) of frame k: its true vectors into frame k - 1 and k + 1."""
    rng = np.random.default_rng(seed)
    m = 2 * n + 2
    back = _smooth(rng, h + 2 * m, w + 2 * m)
    square = _smooth(rng, 40, 40)[..., ::-1] * 0.8 + 60.0
    clean, dirty, masks, flows = [], [], [], []
    ys, xs = np.mgrid[0:h, 0:w]
    inside = []
    for k in range(n):
        f = back[m - k:m - k + h, m - 2 * k:m - 2 * k + w].copy()
        x0, y0 = 70 - k, 30 + 2 * k
        f[y0:y0 + 40, x0:x0 + 40] = square
        inside.append((xs >= x0) & (xs < x0 + 40) & (ys >= y0) & (ys < y0 + 40))
        clean.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        f = np.clip(np.rint(f + rng.normal(0.0, sigma, f.shape)), 0, 255).astype(np.uint8)
        d, mk = f.copy(), np.zeros((h, w), bool)
        if k in blotched:
            for _ in range(count):
                cy, cx = rng.integers(8, h - 8), rng.integers(8, w - 8)
                ry, rx = rng.uniform(0.8, rmax), rng.uniform(0.8, rmax)
                e = ((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0
                d[e] = 8 if rng.random() < 0.5 else 250
                mk |= e
        dirty.append(d)
        masks.append(mk)
    for k in range(n):
        sq = inside[k]
        flows.append((np.where(sq, F(1), F(-2)), np.where(sq, F(-2), F(-1)), np.where(sq, F(-1), F(2)), np.where(sq, F(2), F(1))))
    return dirty, clean, masks, flows


def psnr(a, b):
    e = (a[8:-8, 8:-8].astype(np.float64) - b[8:-8, 8:-8].astype(np.float64)) ** 2
    return 10.0 * np.log10(255.0 ** 2 / max(e.mean(), 1e-12))


def clip_quality(dirty, clean, masks, repaired, repair_masks, frames=(1, 2, 3)):
    """over the repaired frames: (share of blotch pixels hit or grown, share of clean interior pixels hit, PSNR of the damaged frames,
    PSNR of the repaired frames), PSNR on the interior against the clean frames (8-px border left out)"""
    found = np.concatenate([(repair_masks[k] != 0)[masks[k]] for k in frames])
    false_hit = np.concatenate([(repair_masks[k] == 1)[8:-8, 8:-8][~masks[k][8:-8, 8:-8]] for k in frames])
    before = np.mean([psnr(dirty[k], clean[k]) for k in frames])
    after = np.mean([psnr(repaired[k], clean[k]) for k in frames])
    return float(found.mean()), float(false_hit.mean()), float(before), float(after)


# what the restatement reaches on blotch_clip() with true flows and the default parameters (measured)
TRUE_FLOW_QUALITY = dict(found=0.9448, false_hit=0.000042, before=23.68, after=35.16, clean_loss=0.0)


# ---- 1. ABI ----

def test_header_declares_the_defect_filter_and_arguments_are_checked():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    names = ["eppm_defect_default_params", "eppm_defect_create", "eppm_defect_create_size", "eppm_defect_destroy", "eppm_defect_reset",
             "eppm_defect_step", "eppm_defect_step_frames", "eppm_defect_get", "eppm_defect_get_device", "eppm_defect_get_mask",
             "eppm_defect_get_stats", "eppm_defect_get_state", "eppm_defect_set_state", "eppm_defect_step_host"]
    for s in names:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS
    for variant in ("", "test", "tol", "tol_test"):
        so = C.CDLL(eppm_amd.lib_path(variant))
        for s in names:
            assert hasattr(so, s), (variant, s)
    assert not [s for s in _lib.TEST_SYMBOLS if "defect" in s]
    L = eppm_amd.lib()
    p = _lib.CDefectParams()
    assert L.eppm_defect_default_params(C.byref(p)) == 0 and (p.detect, p.agree, p.radius, p.grow) == (60.0, 30.0, 3, 1)
    assert L.eppm_defect_default_params(None) == ARG
    out = C.c_void_p()
    assert L.eppm_defect_create(None, None, C.byref(out)) == ARG
    assert L.eppm_defect_create_size(4, 4, 1, 0, None, None) == ARG
    for h, w, n in ((0, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 4097), (65536, 65536, 1)):
        assert L.eppm_defect_create_size(h, w, n, 0, None, C.byref(out)) == ARG and not out.value
    bad = [(np.nan, 30.0, 3, 1), (np.inf, 30.0, 3, 1), (-1.0, 30.0, 3, 1), (60.0, np.nan, 3, 1), (60.0, np.inf, 3, 1), (60.0, -0.5, 3, 1),
           (60.0, 30.0, 5, 1), (60.0, 30.0, -1, 1), (60.0, 30.0, 3, -1), (60.0, 30.0, 3, 5)]
    rgb, rgb2 = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)
    mask, z, st = np.zeros((4, 4), np.uint8), np.zeros((4, 4), F), _lib.CDefectStats()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    for b in bad:
        q = _lib.CDefectParams(*b)
        assert L.eppm_defect_create_size(4, 4, 1, 0, C.byref(q), C.byref(out)) == ARG and not out.value, b
        assert L.eppm_defect_step_host(C.byref(q), vp(rgb2), vp(mask), C.byref(st), vp(rgb), vp(rgb), vp(rgb), vp(z), vp(z), vp(z), vp(z), 4, 4) == ARG, b
    assert L.eppm_defect_destroy(None) == 0
    assert L.eppm_defect_reset(None, 0) == ARG
    assert L.eppm_defect_step(None, None, None) == ARG
    assert L.eppm_defect_step_frames(None, 0, None, None, C.c_size_t(0), None, None, 0) == ARG
    assert L.eppm_defect_get(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_defect_get_device(None, 0, None, C.c_size_t(0)) == ARG
    assert L.eppm_defect_get_mask(None, 0, None) == ARG and L.eppm_defect_get_stats(None, 0, None) == ARG
    assert L.eppm_defect_get_state(None, 0, None, None, None) == ARG and L.eppm_defect_set_state(None, 0, None, None, 0) == ARG
    # the host form: NULL planes, sizes, the flows of a detecting step, rgb_out == rgb_cur
    host = lambda *a: L.eppm_defect_step_host(C.byref(p), *a, 4, 4)       # noqa: E731
    full = [vp(rgb2), vp(mask), C.byref(st), vp(rgb), vp(rgb), vp(rgb), vp(z), vp(z), vp(z), vp(z)]
    assert host(*full) == 0
    for k in (0, 1, 2, 4, 6, 7, 8, 9):
        assert host(*[None if i == k else a for i, a in enumerate(full)]) == ARG, k
    assert L.eppm_defect_step_host(None, *full, 4, 4) == ARG
    assert host(*[vp(rgb) if i == 0 else a for i, a in enumerate(full)]) == ARG
    assert host(*[None if i in (3, 6, 7, 8, 9) else a for i, a in enumerate(full)]) == 0          # the passing step reads no flow
    assert L.eppm_defect_step_host(C.byref(p), *full, 0, 4) == ARG and L.eppm_defect_step_host(C.byref(p), *full, 65536, 65536) == ARG
    assert b"eppm_defect_step_host" in L.eppm_last_error()


# ---- 2. the restatement against the host form ----

def test_host_form_equals_the_restatement_byte_for_byte():
    for c in defect_cases():
        rgb, mask, stats = host_step(c)
        assert np.array_equal(mask, c["want_mask"]), (c["name"], int((mask != c["want_mask"]).sum()))
        assert np.array_equal(rgb, c["want_rgb"]), (c["name"], int((rgb != c["want_rgb"]).any(axis=-1).sum()))
        assert stats == c["want_stats"], (c["name"], stats, c["want_stats"])


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_host_form_equals_the_restatement_at_the_size_limit(size):
    from test_tfilter_cpu import ends_reached
    cases = defect_limit_cases(size)
    assert {(c["w"], c["h"]) for c in cases} == {LIMIT_SIZES[size]} and {c["pad"] for c in cases} == {0, 3, 64}
    for c in cases:
        rgb, mask, stats = host_step(c)
        assert np.array_equal(mask, c["want_mask"]), (c["name"], int((mask != c["want_mask"]).sum()))
        assert np.array_equal(rgb, c["want_rgb"]), (c["name"], int((rgb != c["want_rgb"]).any(axis=-1).sum()))
        assert stats == c["want_stats"], (c["name"], stats, c["want_stats"])
        if not c["planted"]:
            for u, v in ((c["bu"], c["bv"]), (c["fu"], c["fv"])):
                for axis, reached in ends_reached(u, v).items():
                    assert all(reached.values()), (c["name"], axis, reached)
        elif c["params"]["radius"] > 0:                # repairs in the first and the last columns and rows
            m = c["want_mask"] != 0
            assert m[:, :4].any() and m[:, -4:].any() and m[:4].any() and m[-4:].any(), c["name"]


def test_cases_cover_every_size_and_parameter():
    cases = defect_cases()
    assert {(c["w"], c["h"]) for c in cases} == set(SIZES)
    assert {c["params"]["radius"] for c in cases} >= {0, 1, 3, 4} and {c["params"]["grow"] for c in cases} >= {0, 1, 4}
    assert {c["params"]["detect"] for c in cases} >= {0.0, 60.0, 1e9} and {c["params"]["agree"] for c in cases} >= {0.0, 30.0, 1e9}
    assert any(c["prev"] is None for c in cases) and any(c["next"] is None for c in cases)
    # an unknown vector inside an otherwise good window: some pixel of a planted case is undecided only because of it
    c = next(c for c in cases if c["name"] == "planted-211x157-r3-g1")
    healed = dict(c, bu=np.where(np.isnan(c["bu"]), F(2), c["bu"]))
    code_a = np_step(c["prev"], c["cur"], c["next"], c["bu"], c["bv"], c["fu"], c["fv"], **c["params"])[3]
    code_b = np_step(c["prev"], c["cur"], c["next"], healed["bu"], c["bv"], c["fu"], c["fv"], **c["params"])[3]
    assert (((code_a & 4) != 0) & ((code_b & 2) != 0)).sum() > 0


# ---- 3. meaning ----

def true_flow_run(step):
    dirty, clean, masks, flows = blotch_clip()
    rep, rm = [dirty[0]], [np.zeros(masks[0].shape, np.uint8)]
    for k in range(1, len(dirty) - 1):
        r = step(dirty[k - 1], dirty[k], dirty[k + 1], *flows[k], **DEFAULTS)
        rep.append(r[0])
        rm.append(r[1])
    rep.append(dirty[-1])
    rm.append(np.zeros(masks[0].shape, np.uint8))
    return clip_quality(dirty, clean, masks, rep, rm), (dirty, clean, masks, rep, rm)


def test_blotches_are_concealed_on_true_flows():
    """Measured with the restatement (TRUE_FLOW_QUALITY); the host form reaches it with a margin of 0.02 in the
    shares and 1 dB in PSNR."""
    want, _ = true_flow_run(lambda *a, **k: np_step(*a, **k)[:2])
    print("restatement on true flows: found %.4f false hits %.6f PSNR %.2f -> %.2f dB" % want)
    got, (dirty, clean, masks, rep, rm) = true_flow_run(lambda *a, **k: io.defect_step_host(*a, **k)[:2])
    print("host form on true flows:   found %.4f false hits %.6f PSNR %.2f -> %.2f dB" % got)
    q = TRUE_FLOW_QUALITY
    assert got[0] >= q["found"] - 0.02 and got[1] <= q["false_hit"] + 0.02
    assert got[2] >= q["before"] - 1.0 and got[3] >= q["after"] - 1.0
    assert abs(want[0] - q["found"]) <= 0.02 and abs(want[3] - q["after"]) <= 1.0      # the recorded figures are the restatement's
    # off the blotches (and off their grown rims) nothing changes; the first and the last frame are never repaired
    for k in (1, 2, 3):
        assert np.array_equal(rep[k][rm[k] == 0], dirty[k][rm[k] == 0])
    # a clip with no blotch at all loses little
    dirty0, clean0, masks0, flows0 = blotch_clip(blotched=())
    r = io.defect_step_host(dirty0[1], dirty0[2], dirty0[3], *flows0[2], **DEFAULTS)
    loss = psnr(dirty0[2], clean0[2]) - psnr(r[0], clean0[2])
    print("blotch-free clip: loss %.3f dB, hit share %.6f" % (loss, (r[1] == 1)[8:-8, 8:-8].mean()))
    assert loss <= q["clean_loss"] + 0.3 and (r[1] == 1)[8:-8, 8:-8].mean() <= 0.0002
