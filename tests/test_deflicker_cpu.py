"""CPU tests of flicker removal: the ABI's argument checks, a vectorised numpy restatement of the arithmetic against
eppm_deflicker_step_host bit for bit on the shared generator deflicker_cases() (the GPU tests run the kernels on the same cases), what
the step guarantees (keep 0, no valid cell, a global gain and offset on a static scene), what it reaches on a flickering clip with true
flows, and the two clip drivers against recording fakes."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, api, io
from test_defect_cpu import _smooth, blotch_clip, np_sample, psnr
import test_clip_drivers_cpu as drv

F = np.float32
D = np.float64
ARG, STATE = 1, 3
DEFAULTS = dict(cell=32, iters=2, reject=60.0, tau=12.0, keep=1.0, n_min=32)
LAMBDA = 64.0


# ---- the numpy restatement of section 24 ----

def np_field_at(field, h, w, cell):
    """(h, w, 6) float32: the field between cell centres, every operation one float32 rounding"""
    cy, cx, _ = field.shape

    def taps(n, cells):
        g = (np.arange(n, dtype=F) + F(0.5)) * F(1.0 / cell) - F(0.5)
        g = np.fmin(np.fmax(g, F(0)), F(cells - 1))
        i0 = np.floor(g).astype(np.int64)
        i1 = np.minimum(i0 + 1, cells - 1)
        a = g - i0.astype(F)
        return i0, i1, a, F(1) - a
    x0, x1, ax, bx = taps(w, cx)
    y0, y1, ay, by = taps(h, cy)
    ax, bx, ay, by = ax[None, :, None], bx[None, :, None], ay[:, None, None], by[:, None, None]
    g = lambda yy, xx: field[yy[:, None], xx[None, :]]         # noqa: E731
    out = by * (bx * g(y0, x0) + ax * g(y0, x1)) + ay * (bx * g(y1, x0) + ax * g(y1, x1))
    assert out.dtype == F
    return out


def np_models(sums, n_min):
    """(a (cy, cx, 3), b (cy, cx, 3), valid (cy, cx)) in float64 from the integer sums (cy, cx, 13)"""
    n = sums[..., 0]
    valid = n >= n_min
    N = np.where(valid, n, 1).astype(D)[..., None]
    Sv, Sq, Svv, Svq = (sums[..., 1 + k::4][..., :3].astype(D) for k in range(4))
    Sp, Svp = Sq / 16.0, Svq / 16.0
    lnn = (LAMBDA * N) * N
    var, cov = N * Svv - Sv * Sv, N * Svp - Sv * Sp
    a = np.fmin(np.fmax((cov + lnn) / (var + lnn), 0.5), 2.0)
    b = (Sp - a * Sv) / N
    return a, b, valid


def np_smooth(a, b, valid):
    """(cy, cx, 6) float32: the (1, 2, 1) x (1, 2, 1) average over the valid cells of every 3 x 3 neighbourhood, row by row"""
    cy, cx = valid.shape
    val = np.pad(np.concatenate([a, b], -1), ((1, 1), (1, 1), (0, 0)))
    ok = np.pad(valid, 1)
    num, den = np.zeros((cy, cx, 6), D), np.zeros((cy, cx), D)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wgt = D((2 - abs(dx)) * (2 - abs(dy)))
            o = ok[1 + dy:1 + dy + cy, 1 + dx:1 + dx + cx]
            num = num + np.where(o[..., None], wgt * val[1 + dy:1 + dy + cy, 1 + dx:1 + dx + cx], 0.0)
            den = den + np.where(o, wgt, 0.0)
    ident = np.array([1, 1, 1, 0, 0, 0], F)
    with np.errstate(all="ignore"):
        out = np.where(den[..., None] > 0, (num / den[..., None]).astype(F), ident)
    return out.astype(F)


def np_step(ref, cur, bu, bv, occ2, cell=32, iters=2, reject=60.0, tau=12.0, keep=1.0, n_min=32, cut=False, want_members=False):
    """(rgb, field, valid, stats) of one step; want_members: also the (h, w) membership of the last pass"""
    h, w = bu.shape
    cy, cx = -(-h // cell), -(-w // cell)
    p, ok = np_sample(ref, bu, bv)
    ok = ok & (occ2 == 0) & (not cut)
    v = cur.astype(F)
    vi = cur.astype(np.int64)
    with np.errstate(all="ignore"):
        qp = np.where(ok[..., None], np.rint(p * F(16)), 0).astype(np.int64)
    cid = (np.arange(h)[:, None] // cell) * cx + np.arange(w)[None, :] // cell
    field = np.tile(np.array([1, 1, 1, 0, 0, 0], F), (cy, cx, 1))
    for k in range(iters):
        at = np_field_at(field, h, w, cell) if k else np.tile(np.array([1, 1, 1, 0, 0, 0], F), (h, w, 1))
        with np.errstate(all="ignore"):
            f = at[..., :3] * v + at[..., 3:]
            d = (np.abs(f[..., 0] - p[..., 0]) + np.abs(f[..., 1] - p[..., 1])) + np.abs(f[..., 2] - p[..., 2])
            member = ok & (d <= F(reject if k == 0 else tau))
        sums = np.zeros((cy * cx, 13), np.int64)
        idx = cid[member]
        np.add.at(sums[:, 0], idx, 1)
        for c in range(3):
            vv, qq = vi[..., c][member], qp[..., c][member]
            for j, term in enumerate((vv, qq, vv * vv, vv * qq)):
                np.add.at(sums[:, 1 + 4 * c + j], idx, term)
        assert sums.max(initial=0) < 2 ** 32
        a, b, valid = np_models(sums.reshape(cy, cx, 13), n_min)
        field = np_smooth(a, b, valid)
    at = np_field_at(field, h, w, cell)
    s = (F(1) + F(keep) * (at[..., :3] - F(1))) * v + F(keep) * at[..., 3:]
    rgb = np.floor(np.fmin(np.fmax(s, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    stats = dict(used=int(sums[:, 0].sum()), valid_cells=int(valid.sum()), cells=cy * cx)
    out = (rgb, field, valid.astype(np.uint8), stats)
    return out + (member,) if want_members else out


# ---- the shared cases ----

SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157)]           # w x h
# parameter cases on 67 x 45: what differs from the defaults, the cut flag, the empty-slot flag
VARIANTS = [(dict(iters=1), False, False), (dict(iters=4), False, False), (dict(keep=0.0), False, False), (dict(keep=0.5), False, False),
            (dict(reject=0.0), False, False), (dict(tau=0.0), False, False), (dict(reject=1e9), False, False), (dict(tau=1e9), False, False),
            (dict(reject=1e9, tau=1e9, iters=4, cell=16), False, False), ({}, True, False), ({}, False, True), ({}, True, True),
            (dict(cell=16, keep=0.5), False, True)]


def _vectors(rng, h, w):
    """small vectors (40 % whole; smaller in a frame of fewer than nine columns or rows, so that some stay inside), and one pixel in three
    a special one: on the last column or row, one ulp outside, unknown, infinite, NaN, -0.0, plainly outside"""
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = rng.uniform(-0.6, 0.6, (h, w)) * min(1, (w - 1) / 8), rng.uniform(-0.6, 0.6, (h, w)) * min(1, (h - 1) / 8)
    whole = rng.random((h, w)) < 0.4
    u, v = np.where(whole, np.rint(2 * u), u).astype(F), np.where(whole, np.rint(2 * v), v).astype(F)
    kind = rng.integers(0, 48, (h, w))
    xf, yf = xs.astype(F), ys.astype(F)
    up = lambda a: np.nextafter(F(a), F(np.inf))                          # noqa: E731
    full = lambda x: np.full((h, w), F(x))                                # noqa: E731
    special = {
        0: (F(w - 1) - xf, v), 1: (u, F(h - 1) - yf), 2: (F(w - 1) - xf, F(h - 1) - yf),            # exactly on the last column / row
        3: (up(w - 1) - xf, v), 4: (u, up(h - 1) - yf),                                             # one ulp outside (where the sum is exact)
        5: (-xf - F(1e-45), v), 6: (u, -yf - F(1e-45)),                                             # just below 0 (x = 0 / y = 0: a denormal)
        7: (full(1e10), v), 8: (u, full(-1e10)), 9: (full(np.inf), v), 10: (u, full(-np.inf)),
        11: (full(np.nan), v), 12: (u, full(np.nan)), 13: (full(-0.0), full(-0.0)),
        14: (u + F(w), v), 15: (u, v - F(h)),                                                       # plainly outside
    }
    for k, (su, sv) in special.items():
        u = np.where(kind == k, su, u).astype(F)
        v = np.where(kind == k, sv, v).astype(F)
    return u, v


def _case(seed, w, h, params, cut=False, empty=False):
    """a smooth reference, image 2 = the reference under a gain ramp and an offset plus noise; mask bytes 0-3 on a tenth of the pixels; the
    grid's last cell fully masked (invalid), one cell flat and one saturated in both frames where the grid has them"""
    rng = np.random.default_rng(seed)
    p = dict(DEFAULTS, **params)
    cell = p["cell"]
    cy, cx = -(-h // cell), -(-w // cell)
    base = np.clip(_smooth(rng, h, w) * (0.4 if min(h, w) >= 16 else 0.1) + 60.0, 0, 255)
    ys, xs = np.mgrid[0:h, 0:w]
    gain = 1.0 + rng.uniform(-0.08, 0.08) + rng.uniform(-0.08, 0.08) * (xs / max(w - 1, 1) - 0.5) + rng.uniform(-0.08, 0.08) * (ys / max(h - 1, 1) - 0.5)
    ref = np.clip(np.rint(base + rng.normal(0, 1.0, base.shape)), 0, 255).astype(np.uint8)
    img1 = np.clip(np.rint(base + rng.normal(0, 1.0, base.shape)), 0, 255).astype(np.uint8)
    cur = np.clip(np.rint(gain[..., None] * base + rng.uniform(-6, 6) + rng.normal(0, 1.0, base.shape)), 0, 255).astype(np.uint8)
    occ2 = np.where(rng.random((h, w)) < 0.1, rng.integers(1, 4, (h, w)), 0).astype(np.uint8)
    bu, bv = _vectors(rng, h, w)
    cid = (ys // cell) * cx + xs // cell
    if cx * cy > 1:
        occ2[cid == cx * cy - 1] = 1 + seed % 3
    if cx * cy > 3:
        for a in (ref, img1):
            a[cid == 1] = 70
        cur[cid == 1] = 77              # a flat cell: no variance, the gain is 1 and the offset moves it
        for a in (ref, img1, cur):
            a[cid == 2] = 255           # a saturated cell
    name = f"{w}x{h}-" + "-".join(f"{k}{p[k]:g}" for k in sorted(p)) + ("-cut" if cut else "") + ("-empty" if empty else "")
    return dict(name=name, h=h, w=w, ref=ref, img1=img1, cur=cur, bu=bu, bv=bv, occ2=occ2, params=p, cut=cut, empty=empty)


def np_case(c, ref=None, **kw):
    """the restatement on a case; ref: another reference (the second step's)"""
    r = ref if ref is not None else (c["img1"] if c["empty"] else c["ref"])
    return np_step(r, c["cur"], c["bu"], c["bv"], c["occ2"], cut=c["cut"], **c["params"], **kw)


_CASES = None


def deflicker_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for k, (w, h) in enumerate(SIZES):
        out.append(_case(100 + k, w, h, {}))
    for k, (w, h) in enumerate(SIZES[-2:]):
        for cell in (16, 64):
            out.append(_case(200 + 10 * k + cell, w, h, dict(cell=cell)))
    for k, (params, cut, empty) in enumerate(VARIANTS):
        out.append(_case(300 + k, 67, 45, params, cut, empty))
    # n_min at and one above the count of cell (0, 0): with one pass the counts do not depend on n_min
    probe = _case(400, 67, 45, dict(iters=1))
    n00 = int(np_case(probe, want_members=True)[4][:32, :32].sum())
    assert n00 > 100
    for n_min in (n00, n00 + 1):
        out.append(_case(400, 67, 45, dict(iters=1, n_min=n_min)))
    for c in out:
        p = c["params"]
        if c["cut"] or c["h"] * c["w"] < 64 or (p["reject"], p["tau"]) != (60.0, 12.0):
            continue
        _, _, valid, st, member = np_case(c, want_members=True)
        share = member.mean()
        assert 0.1 <= share <= 0.9, (c["name"], share)
        assert st["cells"] == 1 or 0 < st["valid_cells"] < st["cells"], (c["name"], st)
    _CASES = out
    return out


# Thin frames 8192 long: section 16's bound, which the objects chained with this one obey (its own check, h*w < 2^31, lies far beyond),
# at every cell size: grids of 512 / 256 / 128 cells by 2 / 1 / 1, and the same turned; pad: pixels beyond every row of the caller's images
LIMIT_SIZES = [(8192, 20), (20, 8192)]
LIMIT_CELLS = (16, 32, 64)
_LIMIT = None


def deflicker_limit_cases():
    global _LIMIT
    if _LIMIT is None:
        _LIMIT = [dict(_case(7000 + 10 * i + j, w, h, dict(cell=cell), empty=j == 2), pad=(0, 3, 64)[j]) for i, (w, h) in enumerate(LIMIT_SIZES)
                  for j, cell in enumerate(LIMIT_CELLS)]
    return _LIMIT


def host_case(c, ref=None):
    r = ref if ref is not None else (c["img1"] if c["empty"] else c["ref"])
    return io.deflicker_step_host(r, c["cur"], c["bu"], c["bv"], c["occ2"], cut=c["cut"], **c["params"])


def same(got, want):
    """the frame bytes, the field's bits, the valid bytes and the stats"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            and np.array_equal(got[2], want[2]) and got[3] == want[3])


# ---- the clip of the meaning tests (also tests/test_deflicker_gpu.py) ----

def flicker_clip(seed=11):
    """(flickering frames, the same frames without flicker, true backward flows): blotch_clip without blotches (sigma 2, n 6, 128 x 160);
    frames 1..5 are multiplied by a gain plane, 1 +- 0.12 with a linear ramp of up to +- 0.12 across the frame in a random direction, and
    get an offset of up to +- 8.  flows[k] = (bu, bv) of frame k into frame k - 1."""
    plain, _, _, flows = blotch_clip(blotched=(), sigma=2.0, n=6)
    rng = np.random.default_rng(seed)
    h, w, _ = plain[0].shape
    ys, xs = np.mgrid[0:h, 0:w]
    out = [plain[0].copy()]
    for k in range(1, 6):
        th = rng.uniform(0, 2 * np.pi)
        t = ((xs / (w - 1) - 0.5) * np.cos(th) + (ys / (h - 1) - 0.5) * np.sin(th)) * 2.0 / (abs(np.cos(th)) + abs(np.sin(th)))
        gain = 1.0 + rng.uniform(-0.12, 0.12) + rng.uniform(-0.12, 0.12) * t
        out.append(np.clip(np.rint(gain[..., None] * plain[k] + rng.uniform(-8, 8)), 0, 255).astype(np.uint8))
    return out, plain, [(f[0], f[1]) for f in flows]


def run_clip(frames, flows, step, **params):
    """frames 1 .. n - 1 through step(ref, cur, bu, bv, occ2, **params)[0], each corrected towards the corrected frame before it"""
    h, w, _ = frames[0].shape
    out = [frames[0]]
    for k in range(1, len(frames)):
        out.append(step(out[-1], frames[k], flows[k][0], flows[k][1], np.zeros((h, w), np.uint8), **params)[0])
    return out


# per frame 1..5 on flicker_clip() with true flows, a zero mask and the default parameters (measured)
TRUE_FLOW_PSNR = dict(before=[30.54, 30.98, 36.20, 36.00, 37.35], after=[53.83, 48.42, 49.72, 49.17, 47.78])


# ---- 1. ABI ----

def test_header_declares_the_deflicker_object_and_arguments_are_checked():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    for s in _lib.SYMBOLS:
        if s.startswith("eppm_deflicker"):
            assert re.search(rf"\b{s}\s*\(", hdr), s
    assert sum(s.startswith("eppm_deflicker") for s in _lib.SYMBOLS) == 14
    L = eppm_amd.lib()
    p = _lib.CDeflickerParams()
    assert L.eppm_deflicker_default_params(C.byref(p)) == 0
    assert (p.cell, p.iters, p.reject, p.tau, p.keep, p.n_min) == (32, 2, 60.0, 12.0, 1.0, 32)
    assert L.eppm_deflicker_default_params(None) == ARG
    f = C.c_void_p()
    bad = [dict(cell=8), dict(cell=48), dict(cell=128), dict(iters=0), dict(iters=5), dict(reject=-1.0), dict(reject=np.inf), dict(reject=np.nan),
           dict(tau=-1.0), dict(tau=np.inf), dict(tau=np.nan), dict(keep=-0.1), dict(keep=1.5), dict(keep=np.nan), dict(n_min=0)]
    for kw in bad:                                  # refused before any HIP call: no device is needed to be told so
        q = _lib.CDeflickerParams(**dict(DEFAULTS, **kw))
        assert L.eppm_deflicker_create_size(8, 8, 1, 0, C.byref(q), C.byref(f)) == ARG and not f.value, kw
    for h, w, n in ((0, 8, 1), (8, 0, 1), (65536, 65536, 1), (8, 8, 0), (8, 8, 4097)):
        assert L.eppm_deflicker_create_size(h, w, n, 0, None, C.byref(f)) == ARG and not f.value, (h, w, n)
    assert L.eppm_deflicker_create_size(8, 8, 1, 0, None, None) == ARG
    assert L.eppm_deflicker_create(None, None, C.byref(f)) == ARG
    assert L.eppm_deflicker_destroy(None) == 0
    for fn in ("reset", "step", "get", "get_device", "get_field", "get_stats", "get_state", "set_state"):
        assert getattr(L, f"eppm_deflicker_{fn}")(None, 0, None, 0) == ARG, fn      # 0: NULL or zero, whichever the slot is (int slot, size_t, pointer)
    assert L.eppm_deflicker_step_frames(None, 0, None, None, C.c_size_t(0), None, None, 0) == ARG
    z, o = np.zeros((4, 4), F), np.zeros((4, 4), np.uint8)
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(eppm_amd.EppmError, match="cell 7"):
        io.deflicker_step_host(img, img, z, z, o, cell=7)
    with pytest.raises(ValueError):
        io.deflicker_step_host(img, img[:3], z, z, o)
    q = _lib.CDeflickerParams(**DEFAULTS)
    ptr = img.ctypes.data_as(C.c_void_p)
    assert L.eppm_deflicker_step_host(C.byref(q), ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 4, 4, 0) == ARG         # rgb_out is rgb_ref
    assert b"gathers" in L.eppm_last_error()


# ---- 2. bit parity ----

def test_host_form_equals_the_restatement_bit_for_bit():
    cases = deflicker_cases()
    assert len(cases) >= 24
    for c in cases:
        want, got = np_case(c), host_case(c)
        assert same(got, want), c["name"]
        again = np_case(c, ref=want[0])             # the second step of the GPU tests: the output is the next reference
        assert same(host_case(c, ref=want[0]), again), c["name"] + " (second step)"


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_host_form_equals_the_restatement_at_the_size_limit(size):
    from test_tfilter_cpu import ends_reached
    w, h = LIMIT_SIZES[size]
    cases = [c for c in deflicker_limit_cases() if (c["w"], c["h"]) == (w, h)]
    assert [c["params"]["cell"] for c in cases] == list(LIMIT_CELLS) and {c["pad"] for c in cases} == {0, 3, 64}
    for c in cases:
        want, got = np_case(c), host_case(c)
        assert same(got, want), c["name"]
        assert same(host_case(c, ref=want[0]), np_case(c, ref=want[0])), c["name"] + " (second step)"
        cell = c["params"]["cell"]
        assert want[3]["cells"] == (-(-w // cell)) * (-(-h // cell)) and max(-(-w // cell), -(-h // cell)) == 8192 // cell
        assert 0 < want[3]["valid_cells"] < want[3]["cells"], (c["name"], want[3])
        assert want[2].reshape(-(-h // cell), -(-w // cell))[-1, -2:].any() or want[2].reshape(-(-h // cell), -(-w // cell))[-2:, -1].any(), c["name"]
        for axis, reached in ends_reached(c["bu"], c["bv"]).items():
            assert reached["last"] and reached["beyond"] and reached["zero"], (c["name"], axis, reached)


def test_cases_cover_every_size_and_parameter():
    cases = deflicker_cases()
    assert {(c["w"], c["h"]) for c in cases} == set(SIZES)
    for size in SIZES[-2:]:
        assert {c["params"]["cell"] for c in cases if (c["w"], c["h"]) == size} == {16, 32, 64}
    grids = {(-(-c["w"] // c["params"]["cell"]), -(-c["h"] // c["params"]["cell"])) for c in cases}
    assert (5, 3) in grids and (2, 1) in grids and (1, 1) in grids
    assert {c["params"]["iters"] for c in cases} >= {1, 2, 4} and {c["params"]["keep"] for c in cases} == {0.0, 0.5, 1.0}
    assert {c["params"]["reject"] for c in cases} == {0.0, 60.0, 1e9} and {c["params"]["tau"] for c in cases} == {0.0, 12.0, 1e9}
    assert {(c["cut"], c["empty"]) for c in cases} == {(False, False), (True, False), (False, True), (True, True)}
    a, b = [c for c in cases if c["params"]["n_min"] != 32]
    assert b["params"]["n_min"] == a["params"]["n_min"] + 1
    va, vb = np_case(a)[2], np_case(b)[2]
    assert va[0, 0] == 1 and vb[0, 0] == 0          # the count of cell (0, 0) is a's n_min exactly
    seen = set()
    for c in cases:
        with np.errstate(all="ignore"):
            u, v = c["bu"], c["bv"]
            seen |= {k for k, m in (("nan", np.isnan(u) | np.isnan(v)), ("inf", np.isinf(u) | np.isinf(v)), ("big", np.abs(u) == F(1e10)),
                                    ("-0", np.signbit(u) & (u == 0)), ("frac", (u != np.rint(u)) & np.isfinite(u)),
                                    ("edge", u + np.arange(c["w"], dtype=F)[None, :] == F(c["w"] - 1))) if m.any()}
        assert set(np.unique(c["occ2"])) <= {0, 1, 2, 3}
    assert seen == {"nan", "inf", "big", "-0", "frac", "edge"}
    assert any(set(np.unique(c["occ2"])) == {0, 1, 2, 3} for c in cases)
    big = [c for c in cases if c["w"] == 211 and c["params"]["cell"] == 32][0]
    model = np_models(np.zeros((1, 1, 13), np.int64) + np.array([64] + [64 * 77, 64 * 70 * 16, 64 * 77 * 77, 64 * 77 * 70 * 16] * 3), 32)
    assert model[0].tolist() == [[[1.0, 1.0, 1.0]]] and model[1].tolist() == [[[-7.0, -7.0, -7.0]]]     # a flat cell: gain 1 and an offset
    assert (big["cur"][:32, 32:64] == 77).all() and (big["cur"][:32, 64:96] == 255).all()


# ---- 3. properties ----

def test_keep_zero_and_a_grid_without_a_valid_cell_return_image_two():
    c = [c for c in deflicker_cases() if (c["w"], c["h"]) == (211, 157) and c["params"]["cell"] == 32][0]
    for step in (np_step, io.deflicker_step_host):
        rgb, field, valid, st = step(c["ref"], c["cur"], c["bu"], c["bv"], c["occ2"], **dict(c["params"], keep=0.0))
        assert np.array_equal(rgb, c["cur"]) and valid.any() and (field != np.array([1, 1, 1, 0, 0, 0], F)).any()
        rgb, field, valid, st = step(c["ref"], c["cur"], c["bu"], c["bv"], c["occ2"], **dict(c["params"], n_min=40000))
        assert np.array_equal(rgb, c["cur"]) and not valid.any() and st["valid_cells"] == 0 and st["used"] > 0
        assert (field == np.array([1, 1, 1, 0, 0, 0], F)).all()
        rgb, field, valid, st = step(c["ref"], c["cur"], c["bu"], c["bv"], np.ones_like(c["occ2"]), **c["params"])
        assert np.array_equal(rgb, c["cur"]) and st == dict(used=0, valid_cells=0, cells=35)
        rgb, field, valid, st = step(c["ref"], c["cur"], c["bu"], c["bv"], c["occ2"], cut=True, **c["params"])
        assert np.array_equal(rgb, c["cur"]) and st == dict(used=0, valid_cells=0, cells=35)


@pytest.mark.parametrize("g,o", [(0.9, 6.0), (0.9, -6.0), (1.1, 6.0), (1.1, -6.0)])
def test_a_global_gain_and_offset_on_a_static_scene_come_back_within_the_derived_bound(g, o):
    """Frame 0 r, zero flow, image 2 v = rint(g r + o) = g r + o + e with |e| <= 1/2, one pass with every pixel a member (asserted from
    the inputs).  A cell's model is a = (cov + lambda) / (V + lambda) per N^2, with V the variance of v in the cell and cov = cov(v, r);
    cov - V / g = -cov(v, e) / g, so a - 1 / g = (lambda (1 - 1 / g) - cov(v, e) / g) / (V + lambda): the lambda bias, |g - 1| lambda /
    (V + lambda) in units of the reference's deviation, and what the rounding of v adds, both computed here from the inputs.  With b =
    mean r - a mean v the model's error at a pixel is (a - 1 / g) (v - mean v) + (e - mean e) / g.  Smoothing and the bilinear field are
    convex combinations of cell models, so |out - r| <= max |a - 1 / g| (max v - min v) + 1 / g, plus 1/2 for the output's rounding and
    0.01 for the float32 operations in between."""
    rng = np.random.default_rng(5)
    h, w, cell = 96, 128, 32
    r = np.clip(np.rint(_smooth(rng, h, w) * 0.5 + 30.0), 30, 140).astype(np.uint8)
    v = np.rint(g * r.astype(D) + o)
    assert v.min() >= 1 and v.max() <= 254                      # no saturation
    v = v.astype(np.uint8)
    assert np.abs(v.astype(int) - r.astype(int)).sum(-1).max() <= 60        # every pixel is a member of the one pass
    cells = lambda a: a.reshape(h // cell, cell, w // cell, cell, 3)          # noqa: E731
    vc, ec = cells(v.astype(D)), cells(v.astype(D) - (g * r.astype(D) + o))
    V = vc.var(axis=(1, 3))
    cov_ve = (vc * ec).mean(axis=(1, 3)) - vc.mean(axis=(1, 3)) * ec.mean(axis=(1, 3))
    gain_err = (np.abs(LAMBDA * (1 - 1 / g) - cov_ve / g) / (V + LAMBDA)).max()
    bound = gain_err * (float(v.max()) - float(v.min())) + 1 / g + 0.5 + 0.01
    z = np.zeros((h, w), F)
    for step in (np_step, io.deflicker_step_host):
        rgb, _, valid, st = step(r, v, z, z, np.zeros((h, w), np.uint8), **dict(DEFAULTS, iters=1))
        assert st == dict(used=h * w, valid_cells=12, cells=12) and valid.all()
        err = np.abs(rgb.astype(int) - r.astype(int)).max()
        print(f"g {g} o {o}: worst error {err}, derived bound {bound:.2f}, uncorrected {np.abs(v.astype(int) - r.astype(int)).max()}")
        assert err <= bound
        if (g - 1) * o > 0:             # gain and offset push the same way: the bound is well below the flicker itself
            assert bound < 0.5 * np.abs(v.astype(int) - r.astype(int)).max()


# ---- 4. quality ----

def test_flicker_is_removed_on_true_flows():
    flick, plain, flows = flicker_clip()
    assert len(flick) == 6 and flick[0].shape == (128, 160, 3) and np.array_equal(flick[0], plain[0])
    out = run_clip(flick, flows, np_step, **DEFAULTS)
    before = [psnr(flick[k], plain[k]) for k in range(1, 6)]
    after = [psnr(out[k], plain[k]) for k in range(1, 6)]
    print("before", [round(float(x), 2) for x in before], "after", [round(float(x), 2) for x in after])
    assert np.allclose(before, TRUE_FLOW_PSNR["before"], atol=0.005) and np.allclose(after, TRUE_FLOW_PSNR["after"], atol=0.005), (before, after)
    assert all(a > b for a, b in zip(after, before))
    recorded = np.mean(TRUE_FLOW_PSNR["after"]) - np.mean(TRUE_FLOW_PSNR["before"])
    assert np.mean(after) - np.mean(before) >= 0.5 * recorded
    same_clip = run_clip(plain, flows, np_step, **DEFAULTS)           # what a clip without flicker loses: reported, not asserted
    print("flicker-free clip after the filter", [round(float(psnr(same_clip[k], plain[k])), 2) for k in range(1, 6)])
    host = run_clip(flick, flows, io.deflicker_step_host, **DEFAULTS)
    assert all(np.array_equal(a, b) for a, b in zip(out, host))


# ---- 5. the drivers against recording fakes ----

FAKED = ("EPPM", "EPPMBatch", "CutDetector", "Deflicker")


def run_driver(monkeypatch, fn, *args, script=None, **kw):
    """(trace, result or exception) of a driver under test_clip_drivers_cpu's fakes"""
    mod = sys.modules[eppm_amd.deflicker_sequence.__module__]
    for name in FAKED:
        monkeypatch.setattr(mod, name, type(name, (drv.Fake,), {"real": getattr(api, name)}))
    drv.TRACE.clear(); drv.COUNT.clear(); drv.SCRIPT.clear()
    drv.SCRIPT.update(script or {})
    try:
        end = drv.nest(getattr(eppm_amd, fn)(*args, **kw))
    except Exception as ex:
        end = ex
    return list(drv.TRACE), end


FRAME = "uint8[4, 6, 3]:"
OPEN1 = ["EPPM1.__init__(0, None)", "EPPM1.init((4, 6))", "EPPM1.set_temporal(True)", "EPPM1.set_stop_level(0)"]
OPEN2 = ["EPPMBatch1.__init__(4, 6, 2, 0, None)", "EPPMBatch1.set_temporal(True)", "EPPMBatch1.set_stop_level(0)"]
DK = "Deflicker1.__init__({}, 32, 2, 60.0, 12.0, 1.0, 32, None, 1, 0)"
BIDIR1, BIDIR = "EPPM1.compute_flow_bidirectional_device(None, None, None, None)", "EPPMBatch1.compute_flow_bidirectional_device()"
LOOK = ["CutDetector1.step(None)", "CutDetector1.cuts(None)"]


def test_one_clip_is_set_data_then_pushes_with_one_step_and_one_frame_per_pair(monkeypatch):
    trace, end = run_driver(monkeypatch, "deflicker_sequence", drv.clip(0, 3), cell=16, params="P")
    assert trace == ["EPPM1.__init__(0, 'P')", "EPPM1.init((4, 6))", "EPPM1.set_temporal(True)", "EPPM1.set_stop_level(0)",
                     "Deflicker1.__init__(EPPM1, 16, 2, 60.0, 12.0, 1.0, 32, None, 1, 0)",
                     f"EPPM1.set_data({FRAME}0, {FRAME}1)", BIDIR1, "Deflicker1.step(None, None)", "Deflicker1.frame(0)",
                     f"EPPM1.push_frame({FRAME}2)", BIDIR1, "Deflicker1.step(None, None)", "Deflicker1.frame(0)",
                     "Deflicker1.close()", "EPPM1.close()"]
    assert end == [f"{FRAME}0", "'Deflicker1.frame#8'", "'Deflicker1.frame#12'"]          # frame 0 is the input itself


def test_auto_cut_passes_the_verdict_to_the_step_and_restarts_the_prior(monkeypatch):
    trace, end = run_driver(monkeypatch, "deflicker_sequence", drv.clip(0, 4), auto_cut=True, fields=True, lost_permille=400,
                            script=dict(cuts={1: [0]}))
    read = ["Deflicker1.frame(0)", "Deflicker1.field(0)"]
    assert trace == OPEN1 + [DK.format("EPPM1"), "CutDetector1.__init__(EPPM1, 400, -1.0, None, 1, 0)",
                             f"EPPM1.set_data({FRAME}0, {FRAME}1)", BIDIR1] + LOOK + ["Deflicker1.step([False], None)"] + read + [
                             f"EPPM1.push_frame({FRAME}2)", BIDIR1] + LOOK + ["EPPM1.temporal_reset()", "Deflicker1.step([True], None)"] + read + [
                             f"EPPM1.push_frame({FRAME}3)", BIDIR1] + LOOK + ["Deflicker1.step([False], None)"] + read + [
                             "CutDetector1.close()", "Deflicker1.close()", "EPPM1.close()"]
    assert end == ["tuple", [f"{FRAME}0", "'Deflicker1.frame#11'", "'Deflicker1.frame#19'", "'Deflicker1.frame#26'"],
                   ["'Deflicker1.field#12'", "'Deflicker1.field#20'", "'Deflicker1.field#27'"]]


def test_two_slots_a_clip_change_and_an_idle_slot(monkeypatch):
    """clips of 2, 3 and 2 frames through two slots: slot 0 takes clip 2 at the second step (cut flag, nothing read), slot 1 idles at the
    third (its last frame again, nothing read)"""
    trace, end = run_driver(monkeypatch, "deflicker_sequences", drv.clips((2, 3, 2)), slots=2)
    assert trace == OPEN2 + [DK.format("EPPMBatch1"),
                             f"EPPMBatch1.set_data([({FRAME}0, {FRAME}1), ({FRAME}10, {FRAME}11)])", BIDIR, "Deflicker1.step([False, False], None)",
                             "Deflicker1.frame(0)", "Deflicker1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}20, {FRAME}12], [True, False])", BIDIR, "Deflicker1.step([True, False], None)",
                             "Deflicker1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}21, {FRAME}12], [False, False])", BIDIR, "Deflicker1.step([False, False], None)",
                             "Deflicker1.frame(0)", "Deflicker1.close()", "EPPMBatch1.close()"]
    assert end == [[f"{FRAME}0", "'Deflicker1.frame#7'"], [f"{FRAME}10", "'Deflicker1.frame#8'", "'Deflicker1.frame#12'"],
                   [f"{FRAME}20", "'Deflicker1.frame#16'"]]


def test_one_slot_takes_the_clips_in_turn(monkeypatch):
    trace, end = run_driver(monkeypatch, "deflicker_sequences", drv.clips((2, 2)), slots=1, keep=0.5)
    assert trace == ["EPPMBatch1.__init__(4, 6, 1, 0, None)", "EPPMBatch1.set_temporal(True)", "EPPMBatch1.set_stop_level(0)",
                     "Deflicker1.__init__(EPPMBatch1, 32, 2, 60.0, 12.0, 0.5, 32, None, 1, 0)",
                     f"EPPMBatch1.set_data([({FRAME}0, {FRAME}1)])", BIDIR, "Deflicker1.step([False], None)", "Deflicker1.frame(0)",
                     f"EPPMBatch1.push_frames([{FRAME}10], [True])", BIDIR, "Deflicker1.step([True], None)",
                     f"EPPMBatch1.push_frames([{FRAME}11], [False])", BIDIR, "Deflicker1.step([False], None)", "Deflicker1.frame(0)",
                     "Deflicker1.close()", "EPPMBatch1.close()"]
    assert end == [[f"{FRAME}0", "'Deflicker1.frame#7'"], [f"{FRAME}10", "'Deflicker1.frame#14'"]]


def test_more_slots_than_clips_and_verdicts_on_a_live_and_an_idle_slot(monkeypatch):
    """eight slots asked for, two clips: two slots.  At the second step the detector calls both slots cut: slot 0 idles (nothing read),
    slot 1's frame is read all the same -- a cut step returns image 2 itself"""
    trace, end = run_driver(monkeypatch, "deflicker_sequences", drv.clips((2, 3)), slots=8, auto_cut=True, script=dict(cuts={1: [0, 1]}))
    assert trace == OPEN2 + [DK.format("EPPMBatch1"), "CutDetector1.__init__(EPPMBatch1, 530, -1.0, None, 1, 0)",
                             f"EPPMBatch1.set_data([({FRAME}0, {FRAME}1), ({FRAME}10, {FRAME}11)])", BIDIR] + LOOK + [
                             "Deflicker1.step([False, False], None)", "Deflicker1.frame(0)", "Deflicker1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}1, {FRAME}12], [False, False])", BIDIR] + LOOK + [
                             "EPPMBatch1.temporal_reset(0)", "EPPMBatch1.temporal_reset(1)", "Deflicker1.step([True, True], None)", "Deflicker1.frame(1)",
                             "CutDetector1.close()", "Deflicker1.close()", "EPPMBatch1.close()"]
    assert end == [[f"{FRAME}0", "'Deflicker1.frame#10'"], [f"{FRAME}10", "'Deflicker1.frame#11'", "'Deflicker1.frame#19'"]]


def test_a_compute_that_fails_in_flight_closes_detector_stage_and_context_in_order(monkeypatch):
    trace, end = run_driver(monkeypatch, "deflicker_sequences", drv.clips((4, 4)), slots=2, auto_cut=True, script=dict(fail_at=2))
    assert isinstance(end, RuntimeError) and str(end) == "scripted failure in compute"
    assert trace == OPEN2 + [DK.format("EPPMBatch1"), "CutDetector1.__init__(EPPMBatch1, 530, -1.0, None, 1, 0)",
                             f"EPPMBatch1.set_data([({FRAME}0, {FRAME}1), ({FRAME}10, {FRAME}11)])", BIDIR] + LOOK + [
                             "Deflicker1.step([False, False], None)", "Deflicker1.frame(0)", "Deflicker1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}2, {FRAME}12], [False, False])", BIDIR,
                             "CutDetector1.close()", "Deflicker1.close()", "EPPMBatch1.close()"]
    trace, end = run_driver(monkeypatch, "deflicker_sequence", drv.clip(0, 4), script=dict(fail_at=2))
    assert isinstance(end, RuntimeError)
    assert trace == OPEN1 + [DK.format("EPPM1"), f"EPPM1.set_data({FRAME}0, {FRAME}1)", BIDIR1, "Deflicker1.step(None, None)", "Deflicker1.frame(0)",
                             f"EPPM1.push_frame({FRAME}2)", BIDIR1, "Deflicker1.close()", "EPPM1.close()"]


@pytest.mark.parametrize("fn,args,kw,message", [
    ("deflicker_sequence", (drv.clip(0, 3),), dict(stop_level=1.5), "stop level must be an integer, not 1.5"),
    ("deflicker_sequence", (drv.clip(0, 3),), dict(stop_level=True), "stop level must be an integer, not True"),
    ("deflicker_sequence", (drv.clip(0, 3),), dict(bogus=1), "unknown parameter bogus"),
    ("deflicker_sequence", (drv.clip(0, 3),), dict(cell=16, residual_max=1.0), "need auto_cut=True"),
    ("deflicker_sequence", (drv.clip(0, 1),), {}, "at least two frames"),
    ("deflicker_sequences", (drv.clips((2, 1)),), {}, "at least two frames"),
    ("deflicker_sequences", (drv.clips((2, 2)),), dict(slots=0), "at least one slot"),
    ("deflicker_sequences", (drv.clips((2, 2)),), dict(lost_permille=400), "need auto_cut=True"),
])
def test_a_refusal_opens_nothing(monkeypatch, fn, args, kw, message):
    trace, end = run_driver(monkeypatch, fn, *args, **kw)
    assert isinstance(end, (eppm_amd.EppmError, TypeError)) and message in str(end) and trace == []
