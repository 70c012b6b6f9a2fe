"""CPU tests of background plates: a numpy restatement of the arithmetic -- the forms of a path, the blocked
plane, the accumulation and the render, built from float32 single-rounding operations -- against the host forms in every bit on
plate_cases(); the meaning of a plate on a static scene behind a moving square, with derived equalities; the ABI and its argument
checks; and plate.h under sanitizers.  tests/test_plate_gpu.py holds the kernels to the same restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io
from test_stabilize_cpu import OFFSETS, jitter_clip

F = np.float32
ARG = 1
FLT_MAX = float(np.finfo(np.float32).max)
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


# ---- 1. the restatement ----

def np_forms(path):
    """(fwd, inv, ok): the two displacement forms of a path, float64 operations one rounding each, then cast"""
    p = np.asarray(path, np.float64)
    z = np.zeros(6, F)
    with np.errstate(all="ignore"):
        det = p[0] * p[3] - p[1] * p[2]
        if not abs(det) > 1e-6:
            return z, z.copy(), False
        fwd = np.array([p[4], (p[0] - 1.0) / 2.0, p[1] / 2.0, p[5], p[2] / 2.0, (p[3] - 1.0) / 2.0]).astype(F)
        i00, i01, i10, i11 = p[3] / det, -p[1] / det, -p[2] / det, p[0] / det
        itx, ity = -(i00 * p[4] + i01 * p[5]), -(i10 * p[4] + i11 * p[5])
        inv = np.array([itx, (i00 - 1.0) / 2.0, i01 / 2.0, ity, i10 / 2.0, (i11 - 1.0) / 2.0]).astype(F)
    return fwd, inv, True


def np_advance(path, p, valid):
    """the path advanced by a pair's model: gm_update's expressions for C"""
    c = np.asarray(path, np.float64)
    if not valid:
        return c.copy()
    m00, m01, m10, m11 = 1.0 + 2.0 * p[1], 2.0 * p[2], 2.0 * p[4], 1.0 + 2.0 * p[5]
    return np.array([m00 * c[0] + m01 * c[2], m00 * c[1] + m01 * c[3], m10 * c[0] + m11 * c[2], m10 * c[1] + m11 * c[3],
                     (m00 * c[4] + m01 * c[5]) + p[0], (m10 * c[4] + m11 * c[5]) + p[3]])


def np_block(mask, grow, accept_invalid):
    m = np.asarray(mask, np.uint8)
    b = (m == 1) | ((m > 1) & (not accept_invalid))
    h, w = m.shape
    pad = np.zeros((h + 2 * grow, w + 2 * grow), bool)
    pad[grow:grow + h, grow:grow + w] = b
    out = np.zeros((h, w), bool)
    for dy in range(2 * grow + 1):
        for dx in range(2 * grow + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out.astype(np.uint8)


def _position(form, x, y, h, w):
    """(float)x + ((f0 + f1 * X) + f2 * Y) and the same for y, on integer grids x, y"""
    f = np.asarray(form, F)
    X, Y = (2 * x - (w - 1)).astype(F), (2 * y - (h - 1)).astype(F)
    with np.errstate(all="ignore"):
        qx = x.astype(F) + ((f[0] + f[1] * X) + f[2] * Y)
        qy = y.astype(F) + ((f[3] + f[4] * X) + f[5] * Y)
    return qx, qy


def _taps(qx, qy, h, w):
    """inside test (a NaN fails) and interp_sample's taps and weights; outside positions count as 0"""
    with np.errstate(invalid="ignore"):
        inside = (qx >= 0) & (qx <= F(w - 1)) & (qy >= 0) & (qy <= F(h - 1))
    qx, qy = np.where(inside, qx, F(0)), np.where(inside, qy, F(0))
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = qx - x0.astype(F), qy - y0.astype(F)
    return inside, x0, y0, x1, y1, ax, ay, F(1) - ax, F(1) - ay


def np_accumulate(state, fwd, ok, img, blocked, mx, my, thresh, n_max):
    """one frame into the canvas states: (ch, cw, 4) float32 in, a new array out"""
    h, w, _ = img.shape
    ch, cw = h + 2 * my, w + 2 * mx
    st = np.array(state, F)
    assert st.shape == (ch, cw, 4)
    if not ok:
        return st
    yc, xc = np.mgrid[0:ch, 0:cw]
    qx, qy = _position(fwd, xc - mx, yc - my, h, w)
    inside, x0, y0, x1, y1, ax, ay, bx, by = _taps(qx, qy, h, w)
    B = np.asarray(blocked, np.uint8)
    take = inside & ((B[y0, x0] | B[y0, x1] | B[y1, x0] | B[y1, x1]) == 0)
    im = img.astype(F)
    c = [by * (bx * im[y0, x0, k] + ax * im[y0, x1, k]) + ay * (bx * im[y1, x0, k] + ax * im[y1, x1, k]) for k in range(3)]
    n = st[..., 3]
    with np.errstate(all="ignore"):
        fresh = ~(n >= 1)
        d = (np.abs(c[0] - st[..., 0]) + np.abs(c[1] - st[..., 1])) + np.abs(c[2] - st[..., 2])
        near = d <= F(thresh)
        n1 = np.fmin(n + F(1), F(n_max))
        mean = [st[..., k] + (c[k] - st[..., k]) / n1 for k in range(3)]
        down = n - F(1)
    out = st.copy()
    for k in range(3):
        out[..., k] = np.where(take & fresh, c[k], np.where(take & near, mean[k], st[..., k]))
    out[..., 3] = np.where(take & fresh, F(1), np.where(take & near, n1, np.where(take, down, n)))
    return out


def np_word(rgb):
    """tfilter_word's three bytes of float components (..., 3): clamped and rounded, NaN -> 0"""
    with np.errstate(all="ignore"):
        return np.floor(np.fmin(np.fmax(rgb, F(0)), F(255)) + F(0.5)).astype(np.uint8)


def np_render(state, inv, ok, img, blocked, mx, my, min_count):
    h, w, _ = img.shape
    ch, cw = h + 2 * my, w + 2 * mx
    st = np.asarray(state, F)
    y, x = np.mgrid[0:h, 0:w]
    qx, qy = _position(inv, x, y, h, w)
    with np.errstate(all="ignore"):
        qx, qy = qx + F(mx), qy + F(my)
    inside, x0, y0, x1, y1, ax, ay, bx, by = _taps(qx, qy, ch, cw)
    a00, a01, a10, a11 = st[y0, x0], st[y0, x1], st[y1, x0], st[y1, x1]
    m = F(min_count)
    with np.errstate(all="ignore"):
        seen = (a00[..., 3] >= m) & (a01[..., 3] >= m) & (a10[..., 3] >= m) & (a11[..., 3] >= m)
        blend = np.stack([by * (bx * a00[..., k] + ax * a01[..., k]) + ay * (bx * a10[..., k] + ax * a11[..., k]) for k in range(3)], -1)
    B = np.asarray(blocked, np.uint8)
    filled = (B != 0) & bool(ok) & inside & seen
    fill = np.where(B == 0, 0, np.where(filled, 1, 2)).astype(np.uint8)
    return np.where(filled[..., None], np_word(blend), img), fill


def np_coverage(state):
    n = np.asarray(state, F)[..., 3]
    with np.errstate(invalid="ignore"):
        live = n >= 1
        return np.where(live, np.fmin(np.where(live, n, F(0)), F(255)), F(0)).astype(np.uint8)


# ---- 2. the cases ----

SIZES = [(1, 1), (5, 3), (64, 16), (65, 17), (130, 37)]          # (w, h): below a tile, a tile, one past it both ways, partial tiles
MASKS = ["all0", "all1", "corner_tl", "corner_tr", "corner_bl", "corner_br", "checker", "bytes", "bytes_accept"]
GROWS = [0, 1, 8]
PRIORS = ["empty", "n1", "nmax", "n0", "nneg", "nnan", "nbig", "cnan", "cinf"]
THRESH = [0.0, 40.0, FLT_MAX]
MIN_COUNT = [1, 2, 255]


def case_paths(w, h, mx, my):
    a, z = 0.1, 1.05
    rot = (z * np.cos(a), -z * np.sin(a), z * np.sin(a), z * np.cos(a), 1.5, -0.5)
    return [("identity", IDENT), ("int", (1, 0, 0, 1, 3.0, -2.0)), ("sub", (1, 0, 0, 1, 0.5, 0.25)), ("sub2", (1, 0, 0, 1, -1.75, 2.3125)),
            ("rotzoom", rot), ("outside", (1, 0, 0, 1, 3.0 * (w + 2 * mx) + 10, -2.0 * (h + 2 * my) - 7)), ("det0", (1, 2, 0.5, 1, 3.0, 1.0)),
            ("zero", (0, 0, 0, 0, 0, 0)), ("nan_a", (np.nan, 0, 0, 1, 0, 0)), ("nan_t", (1, 0, 0, 1, np.nan, 0.5)),
            ("inf_t", (1, 0, 0, 1, np.inf, 0)), ("inf_a", (np.inf, 0, 0, 1, 0, 0)), ("huge", (1e300, 0, 0, 1e-300, 1e300, -1e300))]


def make_mask(kind, h, w, rng):
    m = np.zeros((h, w), np.uint8)
    if kind == "all1":
        m[:] = 1
    elif kind.startswith("corner"):
        m[0 if kind[7] == "t" else h - 1, 0 if kind[8] == "l" else w - 1] = 1
    elif kind == "checker":
        m = ((np.add.outer(np.arange(h) // 3, np.arange(w) // 5)) & 1).astype(np.uint8)
    elif kind.startswith("bytes"):
        m = (rng.integers(0, 256, (h, w)) * (rng.random((h, w)) < 0.08)).astype(np.uint8)
    return m


def make_prior(kind, ch, cw, n_max, rng):
    """None: an empty slot; else (ch, cw, 4) float32 with colours near the images' and the named counts"""
    if kind == "empty":
        return None
    st = np.empty((ch, cw, 4), F)
    st[..., :3] = rng.integers(95, 146, (ch, cw, 3)).astype(F) + rng.integers(0, 4, (ch, cw, 3)).astype(F) / F(4)
    n = {"n1": 1, "nmax": n_max, "n0": 0, "nneg": -1, "nnan": np.nan, "nbig": 1e30}.get(kind)
    if n is not None:
        st[..., 3] = F(n)
        pick = rng.random((ch, cw)) < 0.25          # and a share of ordinary counts among them
        st[..., 3][pick] = rng.integers(1, n_max + 1, (ch, cw)).astype(F)[pick]
    else:
        st[..., 3] = rng.integers(0, n_max + 1, (ch, cw)).astype(F)
        bad = rng.random((ch, cw, 3)) < 0.2
        st[..., :3][bad] = np.nan if kind == "cnan" else rng.choice([np.inf, -np.inf], int(bad.sum())).astype(F)
    return st


def _one_case(rng, k, w, h, mx, my, pname, path):
    """case number k of a size: the mask, grow, prior, thresh, n_max and min_count that k selects, and two images"""
    mask_kind = MASKS[k % len(MASKS)]
    grow = GROWS[(k // 2) % 3]
    prior = PRIORS[(k * 4 + k // 9) % len(PRIORS)]
    thresh = THRESH[(k // 3 + k) % 3]
    n_max = (1, 64, 255, 8)[(k // 5) % 4]
    min_count = MIN_COUNT[(k // 7 + k) % 3]
    img = rng.integers(100, 141, (h, w, 3)).astype(np.uint8)
    img_b = img.copy()
    noise = rng.random((h, w)) < 0.5
    img_b[noise] = (img_b[noise].astype(int) + rng.integers(-3, 4, (int(noise.sum()), 3))).astype(np.uint8)
    far = rng.random((h, w)) < 0.1
    img_b[far] = rng.integers(0, 256, (int(far.sum()), 3)).astype(np.uint8)
    return dict(name=f"{w}x{h}_m{mx}.{my}_{pname}_{mask_kind}_g{grow}_{prior}_t{thresh:g}_n{n_max}_c{min_count}", w=w, h=h, mx=mx,
                my=my, pname=pname, path=np.array(path, np.float64), mask_kind=mask_kind, mask=make_mask(mask_kind, h, w, rng),
                grow=grow, accept=mask_kind == "bytes_accept", prior_kind=prior,
                prior=make_prior(prior, h + 2 * my, w + 2 * mx, n_max, rng), thresh=thresh, n_max=n_max, min_count=min_count,
                img=img, img_b=img_b)


_CASES = None


def plate_cases():
    """every case: a size, margins, a path, a mask with its grow and accept_invalid, a prior state, thresh, n_max, min_count and two
    images (the second a perturbed first, so that the second step confirms, contradicts and replaces).  Built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(22)
    cases = []
    for w, h in SIZES:
        k = 0
        for mx, my in ((0, 0), (3, 2), (w, h)):
            for pname, path in case_paths(w, h, mx, my):
                for rep in range(2):
                    cases.append(_one_case(rng, k, w, h, mx, my, pname, path))
                    k += 1
    _CASES = cases
    return cases


# Frames and canvases at kGmMaxDim: (w, h, mx, my).  The frame at the limit leaves no room for a margin along its long side (the canvas
# obeys the same bound: one pixel more is refused); a frame 6 / 4 short of it takes the margins (3, 2) to a canvas of exactly 8192.
# Paths that make the canvas's first column or row sample the frame's last one (a tap at coordinate 8191), and its last one sample half a
# pixel into the frame; pad: pixels beyond
# every row of the caller's image and of the render's output
LIMIT_SIZES = [(8192, 20, 0, 0), (8192, 20, 0, 2), (8186, 20, 3, 2), (20, 8192, 0, 0), (20, 8192, 3, 0), (20, 8188, 3, 2)]
_LIMIT = {}


def plate_limit_cases(size):
    """the cases of LIMIT_SIZES[size]; built on first use"""
    if size not in _LIMIT:
        w, h, mx, my = LIMIT_SIZES[size]
        rng = np.random.default_rng(2200 + size)
        far = (float(w + mx - 1), 0.0) if w > h else (0.0, float(h + my - 1))          # the canvas's first column / row samples the frame's last
        back = (0.5 - far[0], 0.0) if w > h else (0.0, 0.5 - far[1])                   # its last one samples between the frame's first two
        paths = [("int", (1, 0, 0, 1, 3.0, -2.0)), ("sub2", (1, 0, 0, 1, -1.75, 2.3125)), ("far", (1, 0, 0, 1) + far), ("back", (1, 0, 0, 1) + back)]
        _LIMIT[size] = [dict(_one_case(rng, 5 * size + 3 * j + 1, w, h, mx, my, *pp), pad=(0, 3, 64)[(size + j) % 3]) for j, pp in enumerate(paths)]
    return _LIMIT[size]


LIMIT_IDS = [f"{w}x{h}_m{mx}.{my}" for w, h, mx, my in LIMIT_SIZES]


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=LIMIT_IDS)
def test_host_forms_equal_the_restatement_at_the_size_limit(size):
    w, h, mx, my = LIMIT_SIZES[size]
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "gmotion.h")).read()
    limit = int(re.search(r"constexpr int kGmMaxDim = (\d+);", src).group(1))
    assert max(w + 2 * mx, h + 2 * my) == limit
    L, out = eppm_amd.lib(), C.c_void_p()
    pp = _lib.CPlateParams()
    assert L.eppm_plate_default_params(C.byref(pp)) == 0
    pp.margin_x, pp.margin_y = mx + (w > h), my + (h > w)     # one more pixel of margin along the long side: the canvas passes the bound
    assert L.eppm_plate_create_size(h, w, 1, 0, C.byref(pp), C.byref(out)) == ARG and not out.value
    cases = plate_limit_cases(size)
    bad = [(c["name"], d) for c in cases for d in [differences(c, *host_case(c))] if d]
    assert not bad, (len(bad), bad[:3])
    for c in cases:
        want = expected(c)
        assert want["ok"], c["name"]
        yc, xc = np.mgrid[0:h + 2 * my, 0:w + 2 * mx]
        qx, qy = _position(want["fwd"], xc - mx, yc - my, h, w)
        inside = _taps(qx, qy, h, w)[0]
        q, n, first, last = (qx, w, inside[:, 0], inside[:, -1]) if w > h else (qy, h, inside[0], inside[-1])
        if c["pname"] == "far":
            assert first.any() and q[inside].max() == n - 1 and inside.sum() <= min(w + 2 * mx, h + 2 * my), c["name"]
        if c["pname"] == "back":
            assert last.any() and q[inside].min() == 0.5 and inside.sum() <= min(w + 2 * mx, h + 2 * my), c["name"]
        if c["pname"] in ("int", "sub2"):
            assert inside.mean() > 0.5 and q[inside].max() > n - 4, c["name"]


def expected(c):
    """the restatement's results of a case, computed once: forms, blocked plane, the states after step 1 (image a) and step 2 (image b),
    and after each the render of the step's image, the canvas words and the coverage"""
    if "want" not in c:
        fwd, inv, ok = np_forms(c["path"])
        B = np_block(c["mask"], c["grow"], c["accept"])
        ch, cw = c["h"] + 2 * c["my"], c["w"] + 2 * c["mx"]
        st0 = np.zeros((ch, cw, 4), F) if c["prior"] is None else c["prior"]
        st1 = np_accumulate(st0, fwd, ok, c["img"], B, c["mx"], c["my"], c["thresh"], c["n_max"])
        st2 = np_accumulate(st1, fwd, ok, c["img_b"], B, c["mx"], c["my"], c["thresh"], c["n_max"])
        r1 = np_render(st1, inv, ok, c["img"], B, c["mx"], c["my"], c["min_count"])
        r2 = np_render(st2, inv, ok, c["img_b"], B, c["mx"], c["my"], c["min_count"])
        c["want"] = dict(fwd=fwd, inv=inv, ok=ok, blocked=B, states=(st1, st2), renders=(r1, r2), words=(np_word(st1[..., :3]), np_word(st2[..., :3])),
                         coverage=(np_coverage(st1), np_coverage(st2)))
    return c["want"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_forms(a, b):
    """bit for bit, except that a NaN may be any NaN (its sign and payload are the processor's choice and never reach a result)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(a.view(np.uint32)[~both], b.view(np.uint32)[~both])


def kw(c):
    return dict(margins=(c["mx"], c["my"]))


def host_case(c):
    """the host forms on a case: (fwd, inv, ok, blocked, (st1, st2), (render 1, render 2))"""
    fwd, inv, ok = io.plate_forms_host(c["path"])
    B = io.plate_block_host(c["mask"], c["grow"], c["accept"])
    ch, cw = c["h"] + 2 * c["my"], c["w"] + 2 * c["mx"]
    st0 = np.zeros((ch, cw, 4), F) if c["prior"] is None else c["prior"]
    st1 = io.plate_accumulate_host(st0, fwd, c["img"], B, thresh=c["thresh"], n_max=c["n_max"], **kw(c)) if ok else np.array(st0, F)
    st2 = io.plate_accumulate_host(st1, fwd, c["img_b"], B, thresh=c["thresh"], n_max=c["n_max"], **kw(c)) if ok else st1.copy()
    r1 = io.plate_render_host(st1, inv, ok, c["img"], B, min_count=c["min_count"], **kw(c))
    r2 = io.plate_render_host(st2, inv, ok, c["img_b"], B, min_count=c["min_count"], **kw(c))
    return fwd, inv, ok, B, (st1, st2), (r1, r2)


def differences(c, fwd, inv, ok, B, states, renders):
    want, bad = expected(c), []
    if ok != want["ok"] or not same_forms(fwd, want["fwd"]) or not same_forms(inv, want["inv"]):
        bad.append("forms")
    if not same_bits(B, want["blocked"]):
        bad.append("blocked")
    for k in (0, 1):
        if not same_bits(states[k], want["states"][k]):
            bad.append(f"state {k + 1}")
        if not same_bits(renders[k][0], want["renders"][k][0]) or not same_bits(renders[k][1], want["renders"][k][1]):
            bad.append(f"render {k + 1}")
    return bad


@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_forms_equal_the_restatement(size):
    cases = [c for c in plate_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = [(c["name"], d) for c in cases for d in [differences(c, *host_case(c))] if d]
    assert not bad, (len(bad), bad[:3])


def test_the_cases_cover_what_they_claim():
    cases = plate_cases()
    for w, h in SIZES:
        mine = [c for c in cases if (c["w"], c["h"]) == (w, h)]
        assert {c["mask_kind"] for c in mine} == set(MASKS) and {c["grow"] for c in mine} == set(GROWS)
        assert {c["prior_kind"] for c in mine} == set(PRIORS) and {c["thresh"] for c in mine} == set(THRESH)
        assert {c["min_count"] for c in mine} == set(MIN_COUNT) and {(c["mx"], c["my"]) for c in mine} == {(0, 0), (3, 2), (w, h)}
        assert {c["pname"] for c in mine} == {n for n, _ in case_paths(w, h, 0, 0)}
    # every branch is taken somewhere: fresh, confirmed, contradicted, unchanged; and every fill byte
    took = dict(fresh=0, confirmed=0, contradicted=0, replaced=0, fills=set(), dead=0, capped=0)
    for c in cases:
        e = expected(c)
        st0 = np.zeros_like(e["states"][0]) if c["prior"] is None else c["prior"]
        with np.errstate(invalid="ignore"):
            for a, b in ((st0, e["states"][0]), (e["states"][0], e["states"][1])):
                ch = a.view(np.uint32) != b.view(np.uint32)
                moved = ch.any(-1)
                took["fresh"] += int((moved & ~(a[..., 3] >= 1)).sum())
                took["confirmed"] += int((moved & (b[..., 3] > a[..., 3]) & (a[..., 3] >= 1)).sum())
                took["contradicted"] += int((moved & (b[..., 3] < a[..., 3])).sum())
                took["capped"] += int((moved & (a[..., 3] >= 1) & (b[..., 3] == a[..., 3]) & (b[..., 3] == c["n_max"])).sum())
        took["fills"] |= set(np.unique(e["renders"][0][1]).tolist()) | set(np.unique(e["renders"][1][1]).tolist())
        took["dead"] += not e["ok"]
    assert took["fresh"] > 1000 and took["confirmed"] > 1000 and took["contradicted"] > 1000 and took["capped"] > 100, took
    assert took["fills"] == {0, 1, 2} and took["dead"] >= 4 * len(SIZES) * 3


def test_forms_of_special_paths():
    fwd, inv, ok = io.plate_forms_host(IDENT)
    assert ok and not fwd.any() and not inv.any()
    fwd, inv, ok = io.plate_forms_host((1, 0, 0, 1, 3, -2))
    assert ok and fwd.tolist() == [3, 0, 0, -2, 0, 0] and inv.tolist() == [-3, 0, 0, 2, 0, 0]
    for p in ((1, 2, 0.5, 1, 0, 0), (0, 0, 0, 0, 1, 1), (np.nan, 0, 0, 1, 0, 0), (1e-3, 0, 0, 1e-3, 0, 0), (1, 0, 0, 1e-6, 0, 0)):
        fwd, inv, ok = io.plate_forms_host(p)
        assert not ok and not fwd.any() and not inv.any(), p
    a, z = 0.3, 1.25                                  # inv is the inverse: the round trip of a pixel is the pixel
    p = (z * np.cos(a), -z * np.sin(a), z * np.sin(a), z * np.cos(a), 4.5, -7.25)
    fwd, inv, ok = np_forms(p)
    h, w = 37, 130
    y, x = np.mgrid[0:h, 0:w]
    qx, qy = _position(fwd, x, y, h, w)
    X, Y = 2 * qx.astype(np.float64) - (w - 1), 2 * qy.astype(np.float64) - (h - 1)
    bx = qx + ((inv[0] + inv[1] * X) + inv[2] * Y)
    by = qy + ((inv[3] + inv[4] * X) + inv[5] * Y)
    assert np.abs(bx - x).max() < 1e-3 and np.abs(by - y).max() < 1e-3


# ---- 3. what a plate means ----

def square_clip(h, w, sq=9, v=(1, 1), start=(20, 12)):
    """jitter_clip's static random-byte scene seen through a window moving by OFFSETS, and over it a square of other bytes moving by the
    integer velocity v in frame coordinates.  Returns (scene, frames, the true flows (u, v) per pair, the square's box per frame)."""
    frames, cam = jitter_clip(h, w, OFFSETS)
    scene = np.random.default_rng(5).integers(0, 256, (h + 32, w + 32, 3), dtype=np.uint8)          # jitter_clip's scene (seed 5, pad 16)
    assert np.array_equal(scene[16:16 + h, 16:16 + w], frames[0])
    tex = np.random.default_rng(6).integers(0, 256, (sq, sq, 3), dtype=np.uint8)
    boxes, flows = [], []
    for k, f in enumerate(frames):
        x0, y0 = start[0] + k * v[0], start[1] + k * v[1]
        f[y0:y0 + sq, x0:x0 + sq] = tex
        boxes.append((x0, y0, x0 + sq, y0 + sq))
    for k in range(len(frames) - 1):
        u = np.full((h, w), cam[k][0], F)
        vv = np.full((h, w), cam[k][1], F)
        x0, y0, x1, y1 = boxes[k]
        u[y0:y1, x0:x1], vv[y0:y1, x0:x1] = v
        flows.append((u, vv))
    return scene, frames, flows, boxes


def test_plate_of_a_static_scene_behind_a_moving_square():
    """Integer camera translations, the true flows, occ1 = 0, margins (16, 16): the canvas is the scene.  The bilinear weights of an
    integer translation are 0 and 1 up to the float cast of the fit, so a byte moves by far less than 0.5 and rounds back to itself:
    (1) every canvas pixel with n >= 1 IS the scene's byte; (2) every scene pixel that some accumulated frame shows outside the grown
    square has n >= 1, and no other: the set is computed from the geometry alone.  A frame shows a pixel when its four taps (section
    22.1: the pixel and its right and lower neighbours, clamped to the frame; a tap counts even with weight 0) are outside the square
    grown by `grow`, so the one-pixel rim left of and above a grown square is not shown by that frame -- 17 canvas pixels here have no
    other frame to show them (printed); (3) the render returns the scene's byte at every blocked pixel whose fill is 1."""
    h, w, grow, m = 45, 67, 2, 16
    scene, frames, flows, boxes = square_clip(h, w)
    path = np.array(IDENT)
    st = np.zeros((h + 2 * m, w + 2 * m, 4), F)
    occ = np.zeros((h, w), np.uint8)
    covered = np.zeros((h + 2 * m, w + 2 * m), bool)
    literal = np.zeros_like(covered)
    kept = []
    for k, (u, v) in enumerate(flows):
        model, mask = io.gmotion_fit_host(u, v, occ)
        x0, y0, x1, y1 = boxes[k]
        sq = np.zeros((h, w), bool)
        sq[y0:y1, x0:x1] = True
        assert model["valid"] and np.array_equal(mask == 1, sq) and not (mask == 2).any()
        fwd, inv, ok = io.plate_forms_host(path)
        ox, oy = OFFSETS[k]
        assert ok and fwd.tolist() == [-ox, 0, 0, -oy, 0, 0]
        B = io.plate_block_host(mask, grow)
        grown = np.zeros((h, w), bool)
        grown[max(y0 - grow, 0):y1 + grow, max(x0 - grow, 0):x1 + grow] = True
        assert np.array_equal(B != 0, grown)
        st = io.plate_accumulate_host(st, fwd, frames[k], B, margins=(m, m))
        kept.append((inv, B))
        yy, xx = np.mgrid[0:h, 0:w]
        xr, yr = np.minimum(xx + 1, w - 1), np.minimum(yy + 1, h - 1)
        shows = ~(grown | grown[yy, xr] | grown[yr, xx] | grown[yr, xr])
        covered[m + oy:m + oy + h, m + ox:m + ox + w] |= shows              # frame k's pixel (x, y) is canvas pixel (x + ox + m, y + oy + m)
        literal[m + oy:m + oy + h, m + ox:m + ox + w] |= ~grown
        path = np_advance(path, model["p"], model["valid"])
    seen = st[..., 3] >= 1
    assert seen.sum() > h * w              # more than one frame's worth: the window moved
    assert np.array_equal(st[..., :3][seen], scene[seen].astype(F))                     # (1)
    assert np.array_equal(np_word(st[..., :3])[seen], scene[seen])
    assert np.array_equal(seen, covered)                                                # (2), exactly
    print("pixels outside every grown square in some frame but never accumulated (a tap inside the grown square):", int((literal & ~seen).sum()))
    assert st[..., 3].max() == len(flows)
    filled = 0
    for k, (inv, B) in enumerate(kept):                                                 # (3) against the finished canvas
        out, fill = io.plate_render_host(st, inv, True, frames[k], B, margins=(m, m))
        ox, oy = OFFSETS[k]
        truth = scene[m + oy:m + oy + h, m + ox:m + ox + w]
        assert np.array_equal(fill != 0, B != 0)
        assert np.array_equal(out[fill == 1], truth[fill == 1]) and np.array_equal(out[fill != 1], frames[k][fill != 1])
        x0, y0, x1, y1 = boxes[k]
        filled += int((fill[y0:y1, x0:x1] == 1).sum())
    assert filled > 0              # part of the square's footprint is revealed, at least min_count times, by the other frames


# ---- 4. ABI: arguments and states ----

NAMES = ["eppm_plate_default_params", "eppm_plate_create", "eppm_plate_create_size", "eppm_plate_destroy", "eppm_plate_reset", "eppm_plate_canvas_dims",
         "eppm_plate_step", "eppm_plate_step_frames", "eppm_plate_render", "eppm_plate_render_frames", "eppm_plate_get", "eppm_plate_get_device",
         "eppm_plate_get_mask", "eppm_plate_get_path", "eppm_plate_set_path", "eppm_plate_get_state", "eppm_plate_set_state",
         "eppm_plate_forms_host", "eppm_plate_block_host", "eppm_plate_accumulate_host", "eppm_plate_render_host"]


def test_header_symbols_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(eppm_plate_\w+)\s*\(", hdr))
    assert declared == set(NAMES) and declared <= set(_lib.SYMBOLS)
    assert {s for s in _lib.SYMBOLS if s.startswith("eppm_plate_")} == declared
    for variant in ("", "test", "tol", "tol_test"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", eppm_amd.lib_path(variant)], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert {s for s in exported if s.startswith("eppm_plate_")} == declared, variant
    for s in ("PlateParams", "BackgroundPlate", "background_plate", "background_plates", "remove_objects_sequence"):
        assert hasattr(eppm_amd, s), s
    assert C.sizeof(_lib.CPlateParams) == 36
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "plate.cpp")).read()
    assert "sizeof(PlateRec) == 128" in src and "sizeof(TfState) == 16" in src          # the device record and a canvas state: static_asserts


def test_arguments_are_checked():
    L = eppm_amd.lib()
    p = _lib.CPlateParams()
    assert L.eppm_plate_default_params(C.byref(p)) == 0
    assert (p.tau, p.iters, p.margin_x, p.margin_y, p.grow, p.accept_invalid, p.thresh, p.n_max, p.min_count) == (1.0, 3, 0, 0, 2, 0, 40.0, 64, 2)
    assert L.eppm_plate_default_params(None) == ARG
    q = eppm_amd.PlateParams(grow=5, margin_x=7)
    assert (q.grow, q.margin_x, q.margin_y) == (5, 7, 0)
    with pytest.raises(TypeError):
        eppm_amd.PlateParams(smooth=0.5)
    out = C.c_void_p()
    assert L.eppm_plate_create(None, None, C.byref(out)) == ARG
    assert L.eppm_plate_create_size(4, 4, 1, 0, None, None) == ARG
    for h, w, n in ((0, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 4097), (65536, 65536, 1), (8193, 4, 1), (4, 8193, 1), (8192, 8200, 1)):
        assert L.eppm_plate_create_size(h, w, n, 0, None, C.byref(out)) == ARG and not out.value
    assert b"out of range" in L.eppm_last_error()
    assert L.eppm_plate_destroy(None) == 0
    assert L.eppm_plate_reset(None, 0) == ARG and L.eppm_plate_canvas_dims(None, None, None) == ARG
    assert L.eppm_plate_step(None, None, None) == ARG
    assert L.eppm_plate_step_frames(None, 0, None, 0, None, None, 0) == ARG
    assert L.eppm_plate_render(None, None, 0, None, 0, None) == ARG
    assert L.eppm_plate_render_frames(None, 0, None, 0, None, None, None, 0, None) == ARG
    assert L.eppm_plate_get(None, 0, None, 0, None) == ARG and L.eppm_plate_get_device(None, 0, None, 0) == ARG
    assert L.eppm_plate_get_mask(None, 0, None) == ARG and L.eppm_plate_get_path(None, 0, None) == ARG
    assert L.eppm_plate_set_path(None, 0, None) == ARG
    assert L.eppm_plate_get_state(None, 0, None) == ARG and L.eppm_plate_set_state(None, 0, None) == ARG
    # the parameter limits, through a host form and through create (before the device is touched)
    h, w = 4, 5
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)              # noqa: E731
    mask, B = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    inf, nan = float("inf"), float("nan")
    good = (1.0, 3, 0, 0, 2, 0, 40.0, 64, 2)
    trials = [(good, True), ((3e38, 8, 4093, 4094, 8, 1, FLT_MAX, 255, 255), True), ((1.0, 1, 0, 0, 0, 7, 0.0, 1, 1), True)]
    for k, vals in ((0, (0.0, -1.0, inf, nan)), (1, (0, 9)), (2, (-1, 4094, 2 ** 30)), (3, (-1, 4095, 2 ** 30)), (4, (-1, 9)), (6, (-1.0, inf, nan)),
                    (7, (0, 256)), (8, (0, 256))):
        for v in vals:
            t = list(good)
            t[k] = v
            trials.append((tuple(t), False))
    for vals, ok in trials:
        pp = _lib.CPlateParams(*vals)
        assert (L.eppm_plate_block_host(C.byref(pp), ptr(mask), h, w, ptr(B)) == 0) == ok, vals
        if not ok:
            assert L.eppm_plate_create_size(h, w, 1, 0, C.byref(pp), C.byref(out)) == ARG and not out.value, vals
    assert L.eppm_plate_block_host(C.byref(p), None, h, w, ptr(B)) == ARG and L.eppm_plate_block_host(C.byref(p), ptr(mask), h, w, None) == ARG
    assert L.eppm_plate_block_host(None, ptr(mask), h, w, ptr(B)) == ARG and L.eppm_plate_block_host(C.byref(p), ptr(mask), h, w, ptr(mask)) == ARG
    assert L.eppm_plate_block_host(C.byref(p), ptr(mask), 0, w, ptr(B)) == ARG and L.eppm_plate_block_host(C.byref(p), ptr(mask), 8193, 4, ptr(B)) == ARG
    fwd, img, st, o, fill = np.zeros(6, F), np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 4), F), np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
    acc = [C.byref(p), ptr(fwd), ptr(img), ptr(B)]
    assert L.eppm_plate_accumulate_host(*acc, h, w, ptr(st)) == 0
    for k in range(4):
        a = list(acc)
        a[k] = None
        assert L.eppm_plate_accumulate_host(*a, h, w, ptr(st)) == ARG, k
    assert L.eppm_plate_accumulate_host(*acc, h, w, None) == ARG and L.eppm_plate_accumulate_host(*acc, h, 0, ptr(st)) == ARG
    ren = [C.byref(p), ptr(fwd), 1, ptr(img), ptr(B), h, w, ptr(st), ptr(o), ptr(fill)]
    assert L.eppm_plate_render_host(*ren) == 0
    assert L.eppm_plate_render_host(*ren[:9], None) == 0                     # the fill plane is optional
    for k in (0, 1, 3, 4, 7, 8):
        a = list(ren)
        a[k] = None
        assert L.eppm_plate_render_host(*a) == ARG, k
    path, ok = np.array(IDENT), C.c_int()
    forms = [ptr(path), ptr(fwd), ptr(fwd.copy()), C.byref(ok)]
    assert L.eppm_plate_forms_host(*forms) == 0 and ok.value == 1
    for k in range(4):
        a = list(forms)
        a[k] = None
        assert L.eppm_plate_forms_host(*a) == ARG, k
    with pytest.raises(eppm_amd.EppmError):
        io.plate_block_host(mask, grow=9)
    with pytest.raises(ValueError):
        io.plate_accumulate_host(st[:2], fwd, img, B)
    with pytest.raises(ValueError):
        io.plate_forms_host(np.zeros(5))


def test_no_input_reads_outside_a_plane():
    """any path, any mask bytes, any state on planes of their exact size: the host forms return what the restatement says"""
    rng = np.random.default_rng(7)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-30, 0.0, -0.0, 0.5, 1.0, 2.0, 255.0, 256.0, -1.0, 3e38])
    for k in range(60):
        h, w = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        mx, my = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        path = np.where(rng.random(6) < 0.3, special[rng.integers(0, len(special), 6)], np.array(IDENT) + rng.normal(0, 0.3, 6) * (1, 1, 1, 1, 8, 8))
        mask = rng.integers(0, 256, (h, w)).astype(np.uint8) * (rng.random((h, w)) < 0.3)
        st = special[rng.integers(0, len(special), (h + 2 * my, w + 2 * mx, 4))].astype(F)
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        c = dict(name=str(k), h=h, w=w, mx=mx, my=my, path=path, mask=mask.astype(np.uint8), grow=int(rng.integers(0, 9)), accept=bool(k & 1), prior=st,
                 thresh=float(rng.choice(THRESH)), n_max=int(rng.choice([1, 64, 255])), min_count=int(rng.choice(MIN_COUNT)), img=img, img_b=img[::-1, ::-1].copy())
        assert not differences(c, *host_case(c)), k
        # and forms that no path gives: the accumulation and the render take any six floats
        wild = special[rng.integers(0, len(special), 6)].astype(F)
        B = np_block(c["mask"], c["grow"], c["accept"])
        assert same_bits(io.plate_accumulate_host(st, wild, img, B, margins=(mx, my)), np_accumulate(st, wild, True, img, B, mx, my, 40.0, 64)), k
        got, want = io.plate_render_host(st, wild, True, img, B, margins=(mx, my)), np_render(st, wild, True, img, B, mx, my, 2)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), k


def test_semantics_under_sanitizers(tmp_path):
    """plate.h -- the per-pixel functions and the host forms -- under ASan + UBSan + float-cast checks on exactly sized planes
    (tests/csrc/plate_sanitize_driver.cpp, a program of its own, built without HIP)"""
    exe = str(tmp_path / "plate_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "plate_sanitize_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
