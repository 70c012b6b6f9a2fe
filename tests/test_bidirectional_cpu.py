"""CPU tests of the bidirectional call's ABI (include/eppm.h: eppm_compute_bidirectional*, eppm_set_occlusion_params,
eppm_fb_occlusion*): the libraries export it, its argument checks work without a GPU, and the host form of the occlusion criterion
equals a numpy restatement of DESIGN.md section 10 bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, io

NEW = ["eppm_compute_bidirectional", "eppm_compute_bidirectional_device", "eppm_batch_compute_bidirectional",
       "eppm_set_occlusion_params", "eppm_fb_occlusion", "eppm_fb_occlusion_host"]


def test_header_declares_and_libraries_export_the_bidirectional_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eppm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eppm\w*)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    for variant in ("", "test", "tol"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW:
            getattr(L, s)
    cls = open(os.path.join(ROOT, "include", "bao_flow_patchmatch_multiscale_cuda.h")).read()
    assert "compute_flow_bidirectional(float** disp1_x, float** disp1_y, float** disp2_x, float** disp2_y" in cls
    assert "set_occlusion_params(float alpha, float beta)" in cls


def test_argument_errors_without_a_device():
    L = _lib.lib()
    f = np.zeros(16, np.float32)
    p = f.ctypes.data_as(C.c_void_p)
    null = C.c_void_p()
    assert L.eppm_compute_bidirectional(null, p, p, p, p, p, p) == 1
    assert L.eppm_compute_bidirectional(null, null, null, null, null, null, null) == 1
    assert L.eppm_compute_bidirectional_device(null, null, null, null, null) == 1
    assert L.eppm_batch_compute_bidirectional(null, null, null, null, null, null, null) == 1
    assert L.eppm_set_occlusion_params(null, C.c_float(0.01), C.c_float(0.5)) == 1
    o = np.zeros(16, np.uint8)
    po = o.ctypes.data_as(C.c_void_p)
    for a, b in ((-1.0, 0.5), (0.01, -0.5), (float("nan"), 0.5), (0.01, float("inf"))):
        assert L.eppm_fb_occlusion(po, p, p, 4, 4, C.c_float(a), C.c_float(b)) == 1, (a, b)
        assert L.eppm_fb_occlusion_host(po, p, p, p, p, 4, 4, C.c_float(a), C.c_float(b)) == 1, (a, b)
    assert L.eppm_fb_occlusion(null, p, p, 4, 4, C.c_float(0.01), C.c_float(0.5)) == 1
    assert L.eppm_fb_occlusion(po, p, p, 0, 4, C.c_float(0.01), C.c_float(0.5)) == 1
    assert L.eppm_fb_occlusion_host(null, p, p, p, p, 4, 4, C.c_float(0.01), C.c_float(0.5)) == 1
    assert L.eppm_fb_occlusion_host(po, p, p, null, p, 4, 4, C.c_float(0.01), C.c_float(0.5)) == 1
    assert L.eppm_fb_occlusion_host(po, p, p, p, p, 4, 0, C.c_float(0.01), C.c_float(0.5)) == 1
    assert L.eppm_fb_occlusion_host(po, p, p, p, p, 4, 4, C.c_float(0.01), C.c_float(0.5)) == 0


# ---------------------------------------------------------------------------------------------------
# numpy restatement of the criterion: every operation one float32 rounding, left to right
# ---------------------------------------------------------------------------------------------------
def fb_occlusion_np(u, v, bu, bv, alpha=0.01, beta=0.5):
    f32 = np.float32
    u, v, bu, bv = [np.asarray(a, f32) for a in (u, v, bu, bv)]
    h, w = u.shape
    alpha, beta = f32(alpha), f32(beta)
    one, zero = f32(1), f32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        known = lambda a, b: (np.abs(a) <= f32(1e9)) & (np.abs(b) <= f32(1e9))   # noqa: E731
        ys, xs = np.mgrid[0:h, 0:w]
        qx = xs.astype(f32) + u
        qy = ys.astype(f32) + v
        kf = known(u, v)
        inside = (qx >= zero) & (qx <= f32(w - 1)) & (qy >= zero) & (qy <= f32(h - 1))
        ok = kf & inside
        x0 = np.where(ok, np.floor(np.where(ok, qx, 0)), 0).astype(np.int64)
        y0 = np.where(ok, np.floor(np.where(ok, qy, 0)), 0).astype(np.int64)
        x1 = np.minimum(x0 + 1, w - 1)
        y1 = np.minimum(y0 + 1, h - 1)
        ax = qx - x0.astype(f32)
        ay = qy - y0.astype(f32)
        taps = [(bu[yy, xx], bv[yy, xx]) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
        kg = known(*taps[0]) & known(*taps[1]) & known(*taps[2]) & known(*taps[3])
        bx, by = one - ax, one - ay
        gx = by * (bx * taps[0][0] + ax * taps[1][0]) + ay * (bx * taps[2][0] + ax * taps[3][0])
        gy = by * (bx * taps[0][1] + ax * taps[1][1]) + ay * (bx * taps[2][1] + ax * taps[3][1])
        dx, dy = u + gx, v + gy
        inc = (dx * dx + dy * dy) > alpha * ((u * u + v * v) + (gx * gx + gy * gy)) + beta
    out = np.where(inc, 1, 0).astype(np.uint8)
    out[~kg] = 1
    out[~inside] = 2
    out[~kf] = 3
    return out


def smooth_flow(rng, h, w, amp):
    """A smooth random field: bilinear upsampling of a coarse grid of random vectors."""
    gh, gw = max(2, h // 16 + 2), max(2, w // 16 + 2)
    g = rng.uniform(-amp, amp, (2, gh, gw)).astype(np.float32)
    ys = np.linspace(0, gh - 1, h)
    xs = np.linspace(0, gw - 1, w)
    out = []
    for c in range(2):
        rows = np.array([np.interp(xs, np.arange(gw), g[c, i]) for i in range(gh)])
        out.append(np.ascontiguousarray(np.array([np.interp(ys, np.arange(gh), rows[:, j]) for j in range(w)]).T, np.float32))
    return out


def occlusion_cases():
    """(name, u, v, bu, bv, alpha, beta): the cases the CPU and GPU tests share."""
    rng = np.random.default_rng(11)
    cases = []
    for k, (h, w, amp) in enumerate(((48, 64, 4.0), (37, 91, 12.0), (120, 160, 30.0))):
        u, v = smooth_flow(rng, h, w, amp)
        bu, bv = smooth_flow(rng, h, w, amp)
        bu = (-u + rng.normal(0, 0.3, u.shape)).astype(np.float32) if k != 1 else bu    # mostly consistent, and an unrelated pair
        bv = (-v + rng.normal(0, 0.3, v.shape)).astype(np.float32) if k != 1 else bv
        cases.append((f"smooth{k}", u, v, bu, bv, 0.01, 0.5))
    # vectors landing exactly on w-1 / h-1, on integer coordinates, and just outside
    h, w = 24, 32
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    u = (w - 1 - xs).astype(np.float32)
    v = (h - 1 - ys).astype(np.float32)
    u[::3] = rng.integers(-3, 4, u[::3].shape).astype(np.float32)
    v[::3] = rng.integers(-3, 4, v[::3].shape).astype(np.float32)
    u[1::5] = (w - 1 - xs[1::5] + np.float32(1e-3)).astype(np.float32)
    v[2::7] = -ys[2::7] - np.float32(1e-4)
    bu = rng.integers(-2, 3, (h, w)).astype(np.float32)
    bv = rng.integers(-2, 3, (h, w)).astype(np.float32)
    cases.append(("edges", u, v, bu, bv, 0.01, 0.5))
    # NaN and 1e10 entries in both fields
    u, v = smooth_flow(rng, 40, 56, 3.0)
    bu, bv = (-u).copy(), (-v).copy()
    for a in (u, v, bu, bv):
        idx = rng.integers(0, a.size, 60)
        a.reshape(-1)[idx[:30]] = np.nan
        a.reshape(-1)[idx[30:]] = 1e10 * rng.choice([-1, 1], 30)
    u[0, :5] = 1e9          # the largest known magnitude
    cases.append(("unknown", u, v, bu, bv, 0.01, 0.5))
    # 1x1, 1xN, Nx1
    for h, w in ((1, 1), (1, 17), (23, 1)):
        u = rng.uniform(-2, 2, (h, w)).astype(np.float32)
        v = rng.uniform(-2, 2, (h, w)).astype(np.float32)
        u[..., :1] = 0
        v[..., :1] = 0
        bu = rng.uniform(-2, 2, (h, w)).astype(np.float32)
        bv = rng.uniform(-2, 2, (h, w)).astype(np.float32)
        cases.append((f"tiny{h}x{w}", u, v, bu, bv, 0.01, 0.5))
    # alpha = beta = 0: only exact consistency passes
    u, v = smooth_flow(rng, 30, 40, 5.0)
    iu, iv = np.round(u).astype(np.float32), np.round(v).astype(np.float32)
    cases.append(("alpha_beta_zero", iu, iv, -iu, -iv, 0.0, 0.0))
    cases.append(("alpha_beta_zero_smooth", u, v, -u, -v, 0.0, 0.0))
    return cases


@pytest.mark.parametrize("case", occlusion_cases(), ids=lambda c: c[0])
def test_host_occlusion_equals_numpy_restatement(case):
    name, u, v, bu, bv, alpha, beta = case
    got = io.fb_occlusion(u, v, bu, bv, alpha, beta)
    want = fb_occlusion_np(u, v, bu, bv, alpha, beta)
    assert got.dtype == np.uint8 and got.shape == u.shape
    bad = int((got != want).sum())
    assert bad == 0, f"{name}: {bad} of {got.size} pixels differ"


def test_occlusion_codes_cover_every_case():
    cases = {c[0]: c for c in occlusion_cases()}
    seen = set()
    for c in cases.values():
        seen |= set(np.unique(io.fb_occlusion(*c[1:])).tolist())
    assert seen == {0, 1, 2, 3}
    # a constant shift with its exact inverse: consistent where it stays in the frame, 2 where it leaves it
    h, w = 20, 30
    u = np.full((h, w), 3.0, np.float32)
    v = np.full((h, w), -2.0, np.float32)
    occ = io.fb_occlusion(u, v, -u, -v)
    assert (occ[2:, :w - 3] == 0).all() and (occ[:, w - 3:] == 2).all() and (occ[:2] == 2).all()
    # alpha = beta = 0 with integer flows: exactly consistent pixels only
    z = io.fb_occlusion(u, v, -u, -v, 0.0, 0.0)
    assert (z[2:, :w - 3] == 0).all()
    bu = -u.copy()
    bu[10, 10] += 0.25
    z = io.fb_occlusion(u, v, bu, -v, 0.0, 0.0)
    assert z[12, 7] == 1 and z[12, 8] == 0
