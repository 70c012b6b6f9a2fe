"""CPU tests of dense point trajectories (include/eppm.h: eppm_track*, eppm_tracker*): the header declares the ABI and
the libraries export it, argument errors are caught without a GPU, and the host form equals a numpy restatement of section 12 bit for bit on
cases that reach every branch."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io

NEW = ["eppm_track_default_params", "eppm_track_capacity", "eppm_tracker_create", "eppm_tracker_destroy", "eppm_track_step",
       "eppm_track_step_frames", "eppm_tracker_get", "eppm_tracker_get_ended", "eppm_tracker_set", "eppm_track_step_host",
       "eppm_track_seeds_host"]
f32 = np.float32
DEFAULTS = dict(spacing=8, min_eig=2500, fb_alpha=0.01, fb_beta=0.5, mb_alpha=0.01, mb_beta=0.002, capacity=0)


def test_header_declares_and_libraries_export_the_tracking_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eppm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eppm\w*)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    for variant in ("", "test", "tol"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW:
            getattr(L, s)
    cls = open(os.path.join(ROOT, "include", "bao_flow_patchmatch_multiscale_cuda.h")).read()
    assert "track_step" in cls and "create_tracker" in cls


def test_default_parameters_are_the_spec():
    p = eppm_amd.TrackParams()
    assert {k: getattr(p, k) for k in DEFAULTS} == pytest.approx(DEFAULTS)
    assert p.fb_alpha == f32(0.01) and p.mb_beta == f32(0.002)
    assert _lib.lib().eppm_track_capacity(C.byref(p), 436, 1024) == 4 * 128 * 55
    assert _lib.lib().eppm_track_capacity(C.byref(eppm_amd.TrackParams(spacing=7)), 37, 53) == 4 * 8 * 6


def test_argument_errors_without_a_device():
    L = _lib.lib()
    null = C.c_void_p()
    h, w = 9, 11
    img = np.zeros((h, w, 3), np.uint8)
    fl = np.zeros((h, w), np.float32)
    i32 = np.zeros(4 * 4, np.int32)
    xy = np.zeros((4 * 4, 2), np.float32)
    cnt = _lib.CTrackCounts()
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)       # noqa: E731
    t = C.c_void_p()
    assert L.eppm_tracker_create(null, None, C.byref(t)) == 1
    assert L.eppm_track_step(null, null, 0) == 1
    assert L.eppm_tracker_get(null, 0, None, None, None, None) == 1
    assert L.eppm_tracker_get_ended(null, 0, None, None, None, None, None) == 1
    assert L.eppm_tracker_set(null, 0, None, None, None, 0, 0) == 1
    assert L.eppm_track_step_frames(null, ptr(img), ptr(img), C.c_size_t(w * 4), ptr(fl), ptr(fl), h, w) == 1
    assert L.eppm_tracker_destroy(null) == 0
    assert L.eppm_track_default_params(None) == 1

    def host(p=None, n=0, ids=i32, xyin=xy, hh=h, ww=w, a=img, flow=fl, out=i32, frame=0, next_id=0):
        p = eppm_amd.TrackParams() if p is None else p
        return L.eppm_track_step_host(C.byref(p), ptr(a), ptr(a), ptr(flow), ptr(flow), ptr(flow), ptr(flow), hh, ww, n, ptr(ids), ptr(ids),
                                      ptr(xyin), next_id, frame, ptr(out), ptr(out), ptr(xy), ptr(out), ptr(out), ptr(xy), ptr(out), C.byref(cnt))
    assert host() == 0
    for bad in (dict(spacing=0), dict(min_eig=-1), dict(min_eig=(1 << 40) + 1), dict(capacity=-1), dict(capacity=(1 << 26) + 1),
                dict(fb_alpha=float("nan")), dict(mb_beta=-1.0), dict(fb_beta=float("inf"))):
        p = eppm_amd.TrackParams(**bad)
        assert host(p) == 1, bad
        assert L.eppm_track_capacity(C.byref(p), h, w) == -1, bad
    assert host(hh=0) == 1 and host(ww=-1) == 1
    assert host(n=17) == 1                                            # more tracks than the capacity (4 cells x 4)
    assert host(n=-1) == 1 and host(frame=-1) == 1 and host(next_id=-1) == 1
    for px, py in ((-0.5, 0.0), (0.0, h - 0.5), (w - 1 + 1e-3, 1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        pts = xy.copy()
        pts[0] = (px, py)
        assert host(n=1, xyin=pts) == 1, (px, py)
    pts = xy.copy()
    pts[0] = (w - 1, h - 1)
    assert host(n=1, xyin=pts) == 0
    n = C.c_int()
    assert L.eppm_track_seeds_host(C.byref(eppm_amd.TrackParams()), None, h, w, 0, None, C.byref(n)) == 1
    assert L.eppm_track_seeds_host(C.byref(eppm_amd.TrackParams()), ptr(img), h, w, 0, None, C.byref(n)) == 0 and n.value == 0


# ---------------------------------------------------------------------------------------------------
# numpy restatement of DESIGN.md section 12: every float operation one float32 rounding, left to right
# ---------------------------------------------------------------------------------------------------
def seeds_np(img, p):
    """(cell indices, x, y) of the textured cells of img, in cell order."""
    h, w, _ = img.shape
    s = p["spacing"]
    ncx, ncy = -(-w // s), -(-h // s)
    j, i = np.divmod(np.arange(ncx * ncy), ncx)
    sx = np.minimum(i * s + s // 2, w - 1)
    sy = np.minimum(j * s + s // 2, h - 1)
    g = img.astype(np.int64).sum(-1)
    xs, ys = np.arange(w), np.arange(h)
    gx = g[:, np.minimum(xs + 1, w - 1)] - g[:, np.maximum(xs - 1, 0)]
    gy = g[np.minimum(ys + 1, h - 1), :] - g[np.maximum(ys - 1, 0), :]
    d = np.arange(-2, 3)
    tx = np.clip(sx[:, None, None] + d[None, None, :], 0, w - 1)
    ty = np.clip(sy[:, None, None] + d[None, :, None], 0, h - 1)
    GX, GY = gx[ty, tx], gy[ty, tx]
    a, b, c = (GX * GX).sum((1, 2)), (GX * GY).sum((1, 2)), (GY * GY).sum((1, 2))
    S = a + c - 2 * np.int64(p["min_eig"])
    ok = (S >= 0) & (S * S >= (a - c) ** 2 + 4 * b * b)
    k = np.nonzero(ok)[0]
    return k, sx[k], sy[k]


def _known(a, b):
    with np.errstate(invalid="ignore"):
        return (np.abs(a) <= f32(1e9)) & (np.abs(b) <= f32(1e9))


def _bilinear(U, V, qx, qy):
    h, w = U.shape
    x0 = np.floor(qx).astype(np.int64)
    y0 = np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = qx - x0.astype(f32), qy - y0.astype(f32)
    bx, by = f32(1) - ax, f32(1) - ay
    taps = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    known = np.all([_known(U[t], V[t]) for t in taps], axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        ou = by * (bx * U[y0, x0] + ax * U[y0, x1]) + ay * (bx * U[y1, x0] + ax * U[y1, x1])
        ov = by * (bx * V[y0, x0] + ax * V[y0, x1]) + ay * (bx * V[y1, x0] + ax * V[y1, x1])
    return known, ou, ov


def advance_np(x, y, u, v, bu, bv, p):
    """(reason per track, new x, new y); reason 0: alive."""
    h, w = u.shape
    fa, fb, ma, mb = (f32(p[k]) for k in ("fb_alpha", "fb_beta", "mb_alpha", "mb_beta"))
    reason = np.zeros(len(x), np.int32)
    k1, wx, wy = _bilinear(u, v, x, y)
    reason[~k1] = 1
    with np.errstate(invalid="ignore", over="ignore"):
        qx, qy = x + wx, y + wy
        inside = (qx >= f32(0)) & (qx <= f32(w - 1)) & (qy >= f32(0)) & (qy <= f32(h - 1))
    reason[(reason == 0) & ~inside] = 2
    live = reason == 0
    sqx, sqy = np.where(live, qx, f32(0)), np.where(live, qy, f32(0))
    k3, gx, gy = _bilinear(bu, bv, sqx, sqy)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = wx + gx, wy + gy
        ww = wx * wx + wy * wy
        bad = (dx * dx + dy * dy) > fa * (ww + (gx * gx + gy * gy)) + fb
    reason[live & (~k3 | bad)] = 3
    cx = np.clip(np.floor(x + f32(0.5)).astype(np.int64), 0, w - 1)
    cy = np.clip(np.floor(y + f32(0.5)).astype(np.int64), 0, h - 1)
    xl, xr = np.maximum(cx - 1, 0), np.minimum(cx + 1, w - 1)
    yu, yd = np.maximum(cy - 1, 0), np.minimum(cy + 1, h - 1)
    nb = [(cy, xl), (cy, xr), (yu, cx), (yd, cx)]
    k4 = np.all([_known(u[t], v[t]) for t in nb], axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        ux, vx = f32(0.5) * (u[cy, xr] - u[cy, xl]), f32(0.5) * (v[cy, xr] - v[cy, xl])
        uy, vy = f32(0.5) * (u[yd, cx] - u[yu, cx]), f32(0.5) * (v[yd, cx] - v[yu, cx])
        mbad = (ux * ux + uy * uy) + (vx * vx + vy * vy) > ma * ww + mb
    reason[(reason == 0) & (~k4 | mbad)] = 4
    return reason, qx, qy


def step_np(img1, img2, u, v, bu, bv, ids, starts, xy, next_id, frame, p):
    h, w = u.shape
    s = p["spacing"]
    ncx, ncy = -(-w // s), -(-h // s)
    cap = p["capacity"] or 4 * ncx * ncy
    ids, starts = np.asarray(ids, np.int32), np.asarray(starts, np.int32)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    seeded = dropped = 0
    k0 = np.zeros(0, np.int64)
    if frame == 0 and len(ids) == 0:
        k0, sx, sy = seeds_np(img1, p)
        n0 = len(sx)
        acc = min(n0, cap)
        ids = np.arange(next_id, next_id + acc, dtype=np.int32)
        starts = np.zeros(acc, np.int32)
        xy = np.stack([sx[:acc], sy[:acc]], -1).astype(np.float32)
        next_id += acc
        seeded, dropped = acc, n0 - acc
    reason, qx, qy = advance_np(xy[:, 0], xy[:, 1], u, v, bu, bv, p)
    alive = reason == 0
    cov = np.zeros(ncx * ncy, bool)
    cov[(np.floor(qy[alive]).astype(np.int64) // s) * ncx + np.floor(qx[alive]).astype(np.int64) // s] = True
    k, sx, sy = seeds_np(img2, p)
    keep = ~cov[k]
    sx, sy = sx[keep], sy[keep]
    S = int(alive.sum())
    acc = min(len(sx), cap - S)
    # slot_reasons / seed0_cells / seed_cells: the step's per-slot and per-cell flags, for the ledgers (same_state does not look at them)
    out = dict(slot_reasons=reason, seed0_cells=k0, seed_cells=k[keep],
               ids=np.concatenate([ids[alive], np.arange(next_id, next_id + acc, dtype=np.int32)]),
               starts=np.concatenate([starts[alive], np.full(acc, frame + 1, np.int32)]),
               xy=np.concatenate([np.stack([qx[alive], qy[alive]], -1), np.stack([sx[:acc], sy[:acc]], -1).astype(np.float32)]),
               ended_ids=ids[~alive], ended_starts=starts[~alive], ended_xy=xy[~alive], reasons=reason[~alive],
               live=S + acc, ended=int((~alive).sum()), seeded=seeded + acc, dropped=dropped + len(sx) - acc, frame=frame + 1,
               next_id=next_id + acc)
    return out


def same_state(got, want, what):
    for k in ("live", "ended", "seeded", "dropped", "frame", "next_id"):
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    for k in ("ids", "starts", "ended_ids", "ended_starts", "reasons"):
        assert np.array_equal(np.asarray(got[k], np.int32), np.asarray(want[k], np.int32)), f"{what}: {k}"
    for k in ("xy", "ended_xy"):
        a, b = np.asarray(got[k], np.float32).reshape(-1, 2), np.asarray(want[k], np.float32).reshape(-1, 2)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {k}"


# ---------------------------------------------------------------------------------------------------
# crafted cases
# ---------------------------------------------------------------------------------------------------
def _smooth(rng, h, w, scale, amp):
    k = rng.normal(size=(h // scale + 2, w // scale + 2)).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32) / scale
    y0, x0 = ys.astype(int), xs.astype(int)
    ay, ax = ys - y0, xs - x0
    f = (1 - ay) * ((1 - ax) * k[y0, x0] + ax * k[y0, x0 + 1]) + ay * ((1 - ax) * k[y0 + 1, x0] + ax * k[y0 + 1, x0 + 1])
    return (amp * f).astype(np.float32)


def tracking_cases():
    """(name, img1, img2, u, v, bu, bv, params, state or None) tuples: state = (ids, starts, xy, next_id, frame)."""
    out = []
    rng = np.random.default_rng(12)
    h, w = 45, 61
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img1[30:, 40:] = (90, 100, 110)                                   # a flat region: rejected by min_eig 2500, accepted by 0
    img2[:14, :20] = (20, 20, 20)
    u = _smooth(rng, h, w, 9, 2.0) + f32(1.25)
    v = _smooth(rng, h, w, 9, 1.5) - f32(0.5)
    bu, bv = -u + _smooth(rng, h, w, 7, 0.3), -v + _smooth(rng, h, w, 7, 0.3)
    u[5, 5], v[20, 33], u[40, 10] = np.nan, f32(1e10), -np.inf        # reason 1 (and 4 around them)
    u[:, 50:] += f32(9.0)                                             # leaves the frame (2) and a motion boundary (4) at x = 50
    bu[10:20, 20:35] = u[10:20, 20:35]                                # inconsistent (3)
    bv[25, 25], bu[30, 12] = np.nan, f32(2e9)                         # an unknown backward tap (3)
    p = dict(DEFAULTS)
    out.append(("defaults", img1, img2, u, v, bu, bv, p, None))
    out.append(("spacing7_min_eig0", img1, img2, u, v, bu, bv, dict(p, spacing=7, min_eig=0), None))
    out.append(("spacing5_strict", img1, img2, u, v, bu, bv, dict(p, spacing=5, min_eig=40000), None))
    out.append(("spacing3_capacity40", img1, img2, u, v, bu, bv, dict(p, spacing=3, capacity=40), None))
    out.append(("spacing4_capacity_tight", img1, img2, u, v, bu, bv, dict(p, spacing=4, min_eig=0, capacity=180), None))
    # placed tracks: integer and half-integer coordinates, the last row and column, corners
    pts = [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1), (0.5, 0.5), (w - 1.5, h - 1), (w - 1, h - 1.5), (5, 5), (5.5, 5), (33, 20),
           (33.5, 19.5), (10, 40), (24.5, 24.5), (12, 30), (49.5, 7), (50, 7), (51, 22.25), (20.5, 15), (30.75, 12.5), (17.25, 3.0)]
    pts += [(float(x), float(y)) for x, y in zip(rng.uniform(0, w - 1, 60).astype(np.float32), rng.uniform(0, h - 1, 60).astype(np.float32))]
    xy = np.array(pts, np.float32)
    n = len(xy)
    ids = np.arange(100, 100 + n, dtype=np.int32)[rng.permutation(n)]
    starts = rng.integers(0, 5, n).astype(np.int32)
    out.append(("placed", img1, img2, u, v, bu, bv, p, (ids, starts, xy, 500, 5)))
    out.append(("placed_frame0", img1, img2, u, v, bu, bv, dict(p, spacing=6), (ids, starts, xy, 500, 0)))
    out.append(("placed_full", img1, img2, u, v, bu, bv, dict(p, spacing=9, capacity=n), (ids, starts, xy, 7, 2)))
    # a flow that keeps everything (the coverage decides the reseeding)
    z = np.zeros((h, w), np.float32)
    out.append(("still", img1, img1, z + f32(0.5), z, z - f32(0.5), z, dict(p, spacing=4), None))
    return out


# (w, h, spacing) thin frames 8192 long -- section 16's bound, which the tracker's own check (h*w < 2^31) lies far beyond -- with spacings
# that leave the cell count along the long side no multiple of 64: 1171 and 1639 cells (the last one partial), 3 and 4 across
LIMIT_SHAPES = ((8192, 20, 7), (20, 8192, 5))


@functools.lru_cache(maxsize=None)
def limit_tracking_cases(shape):
    """tracking_cases()' kinds on LIMIT_SHAPES[shape]: seeding from image 1, and placed tracks on the first and last pixels of the long
    side, whose taps and motion-boundary neighbours clamp at coordinate 8191"""
    w, h, spacing = LIMIT_SHAPES[shape]
    rng = np.random.default_rng(120 + shape)
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img1[h // 2:, w // 2:] = (90, 100, 110)                           # flat regions: no seeds
    img2[:h // 3, :w // 3] = (20, 20, 20)
    u = _smooth(rng, h, w, 9, 2.0) + f32(1.25)
    v = _smooth(rng, h, w, 9, 1.5) - f32(0.5)
    bu, bv = -u + _smooth(rng, h, w, 7, 0.3), -v + _smooth(rng, h, w, 7, 0.3)
    for a in (u, v, bu, bv):                                          # unknown vectors (reasons 1, 3 and 4)
        ys, xs = rng.integers(0, h, 60), rng.integers(0, w, 60)
        a[ys[:20], xs[:20]], a[ys[20:40], xs[20:40]], a[ys[40:], xs[40:]] = np.nan, f32(1e10), -np.inf
    L, along = max(h, w), (u if w > h else v)
    sl = (slice(None), slice(L - 40, L)) if w > h else (slice(L - 40, L), slice(None))
    along[sl] += f32(9.0)                                             # leaves the frame at the far end (2) and a motion boundary there (4)
    blk = (slice(h // 4, h // 2), slice(w // 4, w // 2))
    bu[blk] = u[blk]                                                  # inconsistent (3)
    p = dict(DEFAULTS, spacing=spacing)
    out = [("limit_seeded", img1, img2, u, v, bu, bv, p, None),
           ("limit_capacity", img1, img2, u, v, bu, bv, dict(p, min_eig=0, capacity=1000), None)]
    ends = [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1), (w - 1.5, h - 1), (w - 1, h - 1.5), (w - 1.25, h - 1.25), (0.5, 0.5)]
    far = [((L - 1 - d, y) if w > h else (y, L - 1 - d)) for d, y in zip(rng.uniform(0, 64, 60), rng.uniform(0, min(h, w) - 1, 60))]
    pts = ends + far + list(zip(rng.uniform(0, w - 1, 200), rng.uniform(0, h - 1, 200)))
    xy = np.array(pts, np.float32)
    n = len(xy)
    ids = np.arange(100, 100 + n, dtype=np.int32)[rng.permutation(n)]
    out.append(("limit_placed", img1, img2, u, v, bu, bv, p, (ids, rng.integers(0, 5, n).astype(np.int32), xy, 500, 5)))
    z = np.zeros((h, w), np.float32)
    out.append(("limit_still", img1, img1, z + f32(0.5), z, z - f32(0.5), z, p, None))
    return out


@pytest.mark.parametrize("shape", range(len(LIMIT_SHAPES)), ids=[f"{w}x{h}" for w, h, _ in LIMIT_SHAPES])
def test_host_form_equals_numpy_restatement_at_the_size_limit(shape):
    w, h, spacing = LIMIT_SHAPES[shape]
    ncx, ncy = -(-w // spacing), -(-h // spacing)
    assert max(ncx, ncy) % 64 != 0 and max(ncx, ncy) > 1024 and max(w, h) % spacing != 0
    reasons = set()
    for case in limit_tracking_cases(shape):
        got, want = _host(case)
        same_state(got, want, case[0])
        reasons |= set(want["reasons"].tolist())
        xy = np.asarray(want["xy"], np.float32).reshape(-1, 2)
        if case[0] in ("limit_seeded", "limit_still"):            # live tracks in the first and in the last cells of the long side
            along = xy[:, 0 if w > h else 1]
            assert along.min() < spacing and along.max() > max(w, h) - 2 * spacing, case[0]
        if case[0] == "limit_capacity":
            assert want["dropped"] > 0 and want["live"] == 1000
        if case[0] == "limit_placed":
            assert {1, 2, 3, 4} <= set(want["reasons"].tolist()) and want["live"] > 100
    assert reasons == {1, 2, 3, 4}, reasons


def _host(case, state=None):
    name, a, b, u, v, bu, bv, p, st = case
    st = state if state is not None else st
    ids, starts, xy, nid, fr = st if st is not None else ((), (), np.zeros((0, 2), np.float32), 0, 0)
    return io.track_step_host(a, b, u, v, bu, bv, ids, starts, xy, nid, fr, **p), step_np(a, b, u, v, bu, bv, ids, starts, xy, nid, fr, p)


def test_host_form_equals_numpy_restatement():
    reasons = set()
    for case in tracking_cases():
        got, want = _host(case)
        same_state(got, want, case[0])
        reasons |= set(want["reasons"].tolist())
        if case[0] == "spacing3_capacity40":
            assert want["dropped"] > 0
        if case[0] == "spacing4_capacity_tight":
            assert want["dropped"] > 0 and want["live"] == 180
    assert reasons == {1, 2, 3, 4}, reasons


def test_texture_test_and_seeds():
    case = tracking_cases()[0]
    a = case[1]
    for p in (dict(DEFAULTS), dict(DEFAULTS, spacing=7, min_eig=0), dict(DEFAULTS, spacing=5, min_eig=40000)):
        _, sx, sy = seeds_np(a, p)
        got = io.track_seeds(a, **p)
        assert np.array_equal(got, np.stack([sx, sy], -1).astype(np.float32)), p
    h, w, _ = a.shape
    assert len(io.track_seeds(a, spacing=7, min_eig=0)) == 9 * 7                 # min_eig 0 accepts every cell
    flat = np.full_like(a, 77)
    assert len(io.track_seeds(flat, spacing=4)) == 0 and len(io.track_seeds(flat, spacing=4, min_eig=0)) == -(-w // 4) * -(-h // 4)
    # the flat region of image 1 has no seed at min_eig 2500
    xy = io.track_seeds(a, spacing=4)
    assert not ((xy[:, 0] >= 42) & (xy[:, 1] >= 32)).any()


def test_multi_step_chains():
    cases = tracking_cases()
    for case in (cases[0], cases[1], cases[5], cases[7], cases[8]):
        name, a, b, u, v, bu, bv, p, st = case
        state = st
        imgs = (a, b)
        for k in range(4):
            c = (name, imgs[k % 2], imgs[(k + 1) % 2], u, v, bu, bv, p, None)
            got, want = _host(c, state)
            same_state(got, want, f"{name} step {k}")
            state = (got["ids"], got["starts"], got["xy"], got["next_id"], got["frame"])
        assert state[4] == (st[4] if st else 0) + 4


# ---------------------------------------------------------------------------------------------------
# long lists: the launch shapes at which a lane of the scan owns more than one block count
# ---------------------------------------------------------------------------------------------------
# k_track_scan / k_track_scan0 (eppm_amd/csrc/k_track.hip) scan the per-block counts with one workgroup of kScanT = 1024 lanes; blocks are
# kTB = 256 slots or cells.  Lane t owns the `per = ceil(blocks / 1024)` counts [t * per, t * per + per), cut at the number of blocks.  Up
# to 262 144 slots (cells) per == 1; every case above stays far below that.  A long list needs no large image: eppm_tracker_set takes any
# n <= capacity tracks at in-frame positions, duplicates included.
TB, SCAN_T = 256, 1024            # kTB and kScanT of eppm_amd/csrc/k_track.hip
PAST = TB * SCAN_T                # the first slot (cell) of block 1024
# ceil(capacity / 256): per 1, 2, 2, 3, 5.  1088 = 17 * 64: eppm_tracker_create (eppm_amd/csrc/tracker.cpp) lays the count arrays out one
# after the other, each 256-byte aligned, so only at a multiple of 64 blocks does a chunk that ran past the counts (the lanes behind the
# last count, b == e == n) meet the next array instead of zeroed padding.  If that layout changes, 1088 loses this reason, not its use.
LONG_NBS = (1024, 1025, 1088, 2049, 4107)
LONG_LISTS = ("full", "room5", "boundary", "hollow")
# case: (slot blocks, per, the most tracks either step holds at or behind slot 262 144).  The ledger holds every case to its row; a row
# with 64 tracks or more there must show survivors, ended tracks, all four reasons and uniform blocks behind that slot.  The rows that
# cannot: per == 1 has no such slot; a `hollow` list is 200 tracks by definition; 1025 blocks leave 219 slots there, and the `boundary`
# list (n % 256 == 1) only one; `cells_empty` starts from no track and seeds about half of 262 810 cells, its point is the cell grid.
LONG_TABLE = {
    "nbs1024_full": (1024, 1, 0), "nbs1024_room5": (1024, 1, 0), "nbs1024_boundary": (1024, 1, 0), "nbs1024_hollow": (1024, 1, 0),
    "nbs1025_full": (1025, 2, 219), "nbs1025_room5": (1025, 2, 219), "nbs1025_boundary": (1025, 2, 1), "nbs1025_hollow": (1025, 2, 0),
    "nbs1088_full": (1088, 2, 16347), "nbs1088_room5": (1088, 2, 16347), "nbs1088_boundary": (1088, 2, 16129), "nbs1088_hollow": (1088, 2, 0),
    "nbs2049_full": (2049, 3, 262363), "nbs2049_room5": (2049, 3, 262363), "nbs2049_boundary": (2049, 3, 262145),
    "nbs2049_hollow": (2049, 3, 0),
    "nbs4107_full": (4107, 5, 789211), "nbs4107_room5": (4107, 5, 789211), "nbs4107_boundary": (4107, 5, 788993),
    "nbs4107_hollow": (4107, 5, 0),
    "cells_empty": (4107, 5, 0), "cells_loaded": (4107, 5, 454657),
}
SMALL_SHAPE = (48, 64)            # (h, w)
BIG_SHAPE = (410, 641)            # spacing 1: 262 810 cells, 1027 cell blocks; default capacity 1 051 240: 4107 slot blocks
BIG_MIN_EIG = 530000              # accepts about half of the cells of the big frame's image 1 (asserted by the ledger)
FREE_X = (32, 48)                 # the all-survive lists leave the cells of these x of the small frame uncovered in their first step


def _capacity(p, h, w):
    return _lib.lib().eppm_track_capacity(C.byref(eppm_amd.TrackParams(**p)), h, w)


def _nblocks(n):
    return -(-n // TB)


def _per(nblocks):
    return -(-nblocks // SCAN_T)


def _planted_flows(rng, h, w):
    """Flows built like tracking_cases()'s first case, its planted sites scaled from 61x45 to w x h; and those sites (x, y)."""
    X = lambda x: int(round(x * (w - 1) / 60))         # noqa: E731
    Y = lambda y: int(round(y * (h - 1) / 44))         # noqa: E731
    u = _smooth(rng, h, w, 9, 2.0) + f32(1.25)
    v = _smooth(rng, h, w, 9, 1.5) - f32(0.5)
    bu, bv = -u + _smooth(rng, h, w, 7, 0.3), -v + _smooth(rng, h, w, 7, 0.3)
    u[Y(5), X(5)], v[Y(20), X(33)], u[Y(40), X(10)] = np.nan, f32(1e10), -np.inf
    u[:, X(50):] += f32(9.0)
    bu[Y(10):Y(20), X(20):X(35)] = u[Y(10):Y(20), X(20):X(35)]
    bv[Y(25), X(25)], bu[Y(30), X(12)] = np.nan, f32(2e9)
    sites = [(X(5), Y(5)), (X(33), Y(20)), (X(10), Y(40)), (X(50), Y(22)), (X(27), Y(15)), (X(25), Y(25)), (X(12), Y(30))]
    return u, v, bu, bv, sites


def _pool(rng, u, v, bu, bv, sites, p, nrand):
    """Candidate positions: random ones, clouds around the planted sites, strips along the frame's edges and (small frames) the
    half-integer lattice; with the restatement's verdict on each for a first step (r1) and, from where it lands, a second (r2)."""
    h, w = u.shape
    xs = [rng.uniform(0, w - 1, nrand)]
    ys = [rng.uniform(0, h - 1, nrand)]
    for sx, sy in sites:
        xs.append(sx + rng.uniform(-4, 4, 20000))
        ys.append(sy + rng.uniform(-4, 4, 20000))
    for lo, hi in ((0.0, 2.5), (h - 3.5, h - 1.0)):
        xs.append(rng.uniform(0, w - 1, 6000))
        ys.append(rng.uniform(lo, hi, 6000))
    if h * w <= 1 << 14:
        gy, gx = np.mgrid[0:2 * h - 1, 0:2 * w - 1] * 0.5
        xs.append(gx.ravel())
        ys.append(gy.ravel())
    x = np.clip(np.concatenate(xs), 0, w - 1).astype(np.float32)
    y = np.clip(np.concatenate(ys), 0, h - 1).astype(np.float32)
    r1, qx, qy = advance_np(x, y, u, v, bu, bv, p)
    r2 = np.full(len(x), -1, np.int32)
    s1 = r1 == 0
    r2[s1] = advance_np(qx[s1], qy[s1], u, v, bu, bv, p)[0]
    return x, y, r1, r2, qx


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _small_frame():
    rng = np.random.default_rng(31)
    h, w = SMALL_SHAPE
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img1[32:, 42:] = (90, 100, 110)
    img2[:15, :21] = (20, 20, 20)
    u, v, bu, bv, sites = _planted_flows(rng, h, w)
    p = dict(DEFAULTS)
    return _frozen(img1, img2, u, v, bu, bv), _frozen(*_pool(rng, u, v, bu, bv, sites, p, 150000))


@functools.lru_cache(maxsize=None)
def _big_frame():
    rng = np.random.default_rng(32)
    h, w = BIG_SHAPE
    img1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img1[100:180] = (90, 100, 110)                     # whole rows flat: cell blocks whose count is zero
    img2[150:240] = (20, 20, 20)
    for im in (img1, img2):
        im[396:, 200:524] = (60, 70, 80)               # flat through the last row: cell block 1025 is row 409, x 231 .. 486
    u, v, bu, bv, sites = _planted_flows(rng, h, w)
    p = dict(DEFAULTS, spacing=1, min_eig=BIG_MIN_EIG)
    return _frozen(img1, img2, u, v, bu, bv), _frozen(*_pool(rng, u, v, bu, bv, sites, p, 300000))


def _layout(rng, n, keep, end, anyp):
    """Pool indices for n slots.  By block of 256 slots, block index mod 5: 0 all of `keep`; 1 all ending (the four reasons in turn);
    2 keep / end alternating slot by slot; 3 random candidates; 4 the four reasons and `keep` in turn, so that every reason sits in
    every stretch of five slots.  keep / end[r] / anyp: pool indices of the classes."""
    i = np.arange(n)
    kind = (i // TB) % 5
    cls = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0, 1 + i % 4, np.where(i % 2 == 0, 0, 1 + (i // 2) % 4), 5], i % 5)
    idx = np.empty(n, np.int64)
    for c, pool in enumerate([keep, end[1], end[2], end[3], end[4], anyp]):
        assert len(pool) >= 8, f"class {c}: only {len(pool)} candidates"
        m = cls == c
        idx[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return idx


def _list_state(rng, n, frame, pool, all_survive):
    """(ids, starts, xy, next_id, frame).  all_survive: every track survives the first step and lands outside FREE_X, and the layout's
    classes are the second step's verdicts; otherwise they are the first step's."""
    x, y, r1, r2, qx = pool
    if all_survive:
        ok = (r1 == 0) & ((qx < f32(FREE_X[0])) | (qx >= f32(FREE_X[1])))
        keep, end, anyp = np.nonzero(ok & (r2 == 0))[0], {r: np.nonzero(ok & (r2 == r))[0] for r in (1, 2, 3, 4)}, np.nonzero(ok)[0]
    else:
        keep, end, anyp = np.nonzero(r1 == 0)[0], {r: np.nonzero(r1 == r)[0] for r in (1, 2, 3, 4)}, np.arange(len(x))
    idx = _layout(rng, n, keep, end, anyp)
    ids = (1000 + rng.permutation(n)).astype(np.int32)
    starts = rng.integers(0, frame + 1, n).astype(np.int32)
    return ids, starts, np.stack([x[idx], y[idx]], -1), 1000 + n + 17, frame


def long_list_case(name):
    """The case `name` of long_list_cases(), as a tracking_cases() tuple."""
    if name.startswith("cells"):
        (a, b, u, v, bu, bv), pool = _big_frame()
        p = dict(DEFAULTS, spacing=1, min_eig=BIG_MIN_EIG)
        st = None
        if name == "cells_loaded":
            st = _list_state(np.random.default_rng(77), TB * 2800 + 1, 4, pool, False)
        return (name, a, b, u, v, bu, bv, p, st)
    (a, b, u, v, bu, bv), pool = _small_frame()
    nbs, kind = int(name[3:].split("_")[0]), name.split("_")[1]
    cap = TB * nbs - 37                                # a ragged last block
    n, frame, all_survive = {"full": (cap, 3, True), "room5": (cap - 5, 1, True), "boundary": (TB * (nbs - 1) + 1, 2, False),
                             "hollow": (200, 0, False)}[kind]
    rng = np.random.default_rng(1000 * LONG_LISTS.index(kind) + nbs)
    return (name, a, b, u, v, bu, bv, dict(DEFAULTS, capacity=cap), _list_state(rng, n, frame, pool, all_survive))


def long_list_cases():
    """(name, (h, w), params, build) of the long-list cases; build() makes the tracking_cases() tuple (up to 16 MB of tracks).  On the
    64x48 frame, per capacity (LONG_NBS slot blocks): `full` n == capacity, every track survives the first step, no seed fits; `room5`
    n == capacity - 5, exactly five seeds fit; `boundary` one track in the last block (n % 256 == 1, behind slot 262 144 once per >= 2);
    `hollow` 200 tracks and a thousand and more blocks without one.  `cells_*`: spacing 1 on 641x410, more than 1024 cell blocks, from
    the empty state (the frame-0 seeding pass) and from a loaded one.  Every case is stepped twice (images 1, 2 then 2, 1)."""
    out = []
    for nbs in LONG_NBS:
        for kind in LONG_LISTS:
            name = f"nbs{nbs}_{kind}"
            out.append((name, SMALL_SHAPE, dict(DEFAULTS, capacity=TB * nbs - 37), functools.partial(long_list_case, name)))
    for name in ("cells_empty", "cells_loaded"):
        out.append((name, BIG_SHAPE, dict(DEFAULTS, spacing=1, min_eig=BIG_MIN_EIG), functools.partial(long_list_case, name)))
    return out


def long_list_steps(case, nsteps=2):
    """(k, the case of step k): the images alternate, so the second step consumes the first's compacted list on the other image."""
    name, a, b, u, v, bu, bv, p, st = case
    imgs = (a, b)
    for k in range(nsteps):
        yield k, (name, imgs[k % 2], imgs[(k + 1) % 2], u, v, bu, bv, p, st)


def _wg_scan(a, force_per=None):
    """wg_exclusive_scan of k_track.hip, lane by lane: (the array after the scan, the total every lane returns).  force_per: a wrong
    chunk length, to show what the long cases catch."""
    a = np.asarray(a, np.int64)
    n = len(a)
    per = force_per or -(-n // SCAN_T)
    t = np.arange(SCAN_T)
    b = np.minimum(t * per, n)
    e = np.minimum(b + per, n)
    cs = np.concatenate([[0], np.cumsum(a)])
    s = cs[e] - cs[b]                                  # lds[t]
    run = np.cumsum(s) - s                             # the exclusive prefix of lane t's chunk
    out = a.copy()                                     # a count no lane visits keeps its value
    for j in range(per):
        i = b + j
        m = i < e
        out[i[m]] = run[m] + (cs[i[m]] - cs[b[m]])
    return out, int(s.sum())


def _scatter_dest(flag, force_per=None):
    """Where k_track_scatter / k_track_seed0_scatter put the flagged lanes of a grid of len(flag) / 256 blocks: the scanned block offset
    plus the rank inside the block; and the scan's total."""
    counts = flag.reshape(-1, TB).sum(1)
    off, total = _wg_scan(counts, force_per)
    idx = np.nonzero(flag)[0]
    blk = idx // TB
    rank = np.arange(len(idx)) - (np.cumsum(counts) - counts)[blk]
    return off[blk] + rank, total


def _check_scan(flag, what):
    """The transplanted scan orders the flagged lanes 0, 1, 2, ...; with per forced to 1 (a scan that is right for every shape the other
    tests reach) it does so exactly while nothing is flagged at or behind lane 262 144.  This is the record of what the long cases can
    catch, made on a Python copy of the arithmetic; the guard on the kernels themselves is the parity test of tests/test_tracks_gpu.py."""
    n = int(flag.sum())
    dest, total = _scatter_dest(flag)
    assert total == n and np.array_equal(dest, np.arange(n)), what
    dest1, total1 = _scatter_dest(flag, force_per=1)
    wrong = total1 != n or not np.array_equal(dest1, dest)
    assert wrong == bool(flag[PAST:].any()), f"{what}: per forced to 1 {'misorders' if wrong else 'passes'}"
    return wrong


def long_list_ledger(case, steps):
    """What the case must reach, from the restatement's results `steps` (step_np's dicts of the two steps) alone."""
    name, a, b, u, v, bu, bv, p, st = case
    h, w = u.shape
    s = p["spacing"]
    cap, ncells = _capacity(p, h, w), -(-w // s) * -(-h // s)
    nbs, nbc = _nblocks(cap), _nblocks(ncells)
    per, per_c = _per(nbs), _per(nbc)
    kind = name.split("_")[1]
    n = 0 if st is None else len(st[0])
    first = steps[0]
    if kind == "full":                                 # no room is left and every seed is dropped
        assert n == cap and first["live"] == cap and first["ended"] == 0 and first["seeded"] == 0 and first["dropped"] > 0
    if kind == "room5":                                # exactly five seeds are accepted, the rest dropped
        assert n == cap - 5 and first["live"] == cap and first["ended"] == 0 and first["seeded"] == 5 and first["dropped"] > 0
    if kind == "boundary":                             # one track in the last block; behind slot 262 144 wherever such a slot exists
        assert n % TB == 1 and n == TB * (nbs - 1) + 1 and (n > PAST) == (per >= 2)
    if kind == "hollow":                               # slots >= n inactive through a thousand blocks
        assert 0 < n < TB and nbs - 1 >= 1000
    f = dict(active_past=0, surv_past=0, ended_past=0, zero_surv_blocks=0, zero_ended_blocks=0, reasons_past=set(), caught=0)
    # blocks behind index 1024 that hold tracks; 1025 blocks have one such block, which must hold survivors and ended tracks, so there
    # the uniform blocks are looked for among all the multi-count chunks (every lane's but lane 512's)
    lo = SCAN_T if nbs > SCAN_T + 1 else 1
    for k, want in enumerate(steps):
        r = want["slot_reasons"]
        m = len(r)
        surv, end = np.zeros(nbs * TB, bool), np.zeros(nbs * TB, bool)
        surv[:m], end[:m] = r == 0, r != 0
        held = slice(lo, _nblocks(m))
        f["active_past"] = max(f["active_past"], m - PAST)
        f["surv_past"] += int(surv[PAST:].sum())
        f["ended_past"] += int(end[PAST:].sum())
        f["zero_surv_blocks"] += int((surv.reshape(-1, TB).sum(1)[held] == 0).sum())
        f["zero_ended_blocks"] += int((end.reshape(-1, TB).sum(1)[held] == 0).sum())
        f["reasons_past"] |= set(r[PAST:][r[PAST:] != 0].tolist())
        f["caught"] += _check_scan(surv, f"{name} step {k}: survivors") + _check_scan(end, f"{name} step {k}: ended")
    behind = LONG_TABLE[name][2]
    assert (nbs, per, max(f["active_past"], 0)) == LONG_TABLE[name], (name, nbs, per, f)
    if behind >= 64:
        assert f["surv_past"] > 0 and f["ended_past"] > 0 and f["zero_surv_blocks"] > 0 and f["zero_ended_blocks"] > 0, (name, f)
        assert f["reasons_past"] == {1, 2, 3, 4} and f["caught"] >= 2, (name, f)
    elif behind == 1:                                  # slot 262 144 is the list's last track: the forced scan misplaces that one
        assert f["caught"] >= 1, (name, f)
    else:                                              # nothing at or behind slot 262 144: the forced scan is right
        assert f["caught"] == 0, (name, f)
    if name.startswith("cells"):
        assert per_c == 2 and nbc == 1027 and per == 5
        frac = len(seeds_np(a, p)[0]) / ncells
        assert 0.35 <= frac <= 0.65, frac              # min_eig accepts roughly half the cells
        g = dict(cells_past=0, zero_blocks_past=0, full_blocks_past=0, caught=0)
        for k, want in enumerate(steps):
            for key in ("seed0_cells", "seed_cells"):
                flag = np.zeros(nbc * TB, bool)
                flag[want[key]] = True
                counts = flag.reshape(-1, TB).sum(1)
                g["cells_past"] += int(flag[PAST:].sum())
                g["zero_blocks_past"] += int((counts[SCAN_T:] == 0).sum()) if flag.any() else 0
                g["full_blocks_past"] += int((counts[SCAN_T:] > 0).sum())
                g["caught"] += _check_scan(flag, f"{name} step {k}: {key}")
        assert g["cells_past"] > 0 and g["zero_blocks_past"] > 0 and g["full_blocks_past"] > 0 and g["caught"] >= 2, (name, g)
        if st is None:                                 # the frame-0 pass ran, and its seeds reach the cell blocks behind 1024
            assert len(steps[0]["seed0_cells"]) > 0 and steps[0]["seed0_cells"].max() >= PAST
        f.update(g)
    return f


def test_long_list_ledger():
    """The shapes of the long-list cases: which chunk lengths of the scan they run.  The cases are held to LONG_TABLE's literal rows, so
    dropping any capacity from LONG_NBS, or any list, fails here."""
    shapes = {}
    for name, (h, w), p, _ in long_list_cases():
        s = p["spacing"]
        cap, ncells = _capacity(p, h, w), -(-w // s) * -(-h // s)
        assert 0 < cap and cap * 61 <= 64 << 20, (name, cap)                    # 61 B per slot: at most 64 MB
        shapes[name] = (_nblocks(cap), _per(_nblocks(cap)), _per(_nblocks(ncells)))
    assert {k: v[:2] for k, v in shapes.items()} == {k: v[:2] for k, v in LONG_TABLE.items()}
    small = sorted({v[:2] for k, v in shapes.items() if k.startswith("nbs")})
    assert small == [(1024, 1), (1025, 2), (1088, 2), (2049, 3), (4107, 5)] and len(shapes) == 4 * len(small) + 2
    assert {v[1] for v in shapes.values()} == {1, 2, 3, 5} and shapes["cells_empty"][2] == shapes["cells_loaded"][2] == 2
    assert _capacity(dict(DEFAULTS, spacing=1, min_eig=BIG_MIN_EIG), *BIG_SHAPE) == 4 * 262810 and _nblocks(262810) == 1027
    # the shapes the other cases reach all have per == 1: tracking_cases() and the bundled 640x480 pair
    assert _per(_nblocks(4 * 80 * 60)) == 1 and all(_per(_nblocks(_capacity(c[7], *c[3].shape))) == 1 for c in tracking_cases())


@pytest.mark.parametrize("name", [c[0] for c in long_list_cases()])
def test_long_lists_host_form_equals_numpy_restatement(name):
    case = long_list_case(name)
    state, steps = case[8], []
    for k, c in long_list_steps(case):
        got, want = _host(c, state if state is not None else ((), (), np.zeros((0, 2), np.float32), 0, 0))
        same_state(got, want, f"{name} step {k}")
        steps.append(want)
        state = (got["ids"], got["starts"], got["xy"], got["next_id"], got["frame"])
    if case[8] is not None:                            # ids are a permutation: an order error cannot hide
        assert len(set(case[8][0].tolist())) == len(case[8][0])
    long_list_ledger(case, steps)
