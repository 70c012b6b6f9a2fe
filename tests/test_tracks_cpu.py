"""CPU tests of dense point trajectories (include/eppm.h: eppm_track*, eppm_tracker*): the header declares the ABI and
the libraries export it, argument errors are caught without a GPU, and the host form equals a numpy restatement of section 12 bit for bit on
cases that reach every branch."""
import ctypes as C
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
    if frame == 0 and len(ids) == 0:
        _, sx, sy = seeds_np(img1, p)
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
    out = dict(ids=np.concatenate([ids[alive], np.arange(next_id, next_id + acc, dtype=np.int32)]),
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
