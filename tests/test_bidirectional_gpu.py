"""GPU tests of the bidirectional call (eppm_compute_bidirectional*): the forward flow stays eppm_compute's, the
backward flow is bit-identical to the CPU oracle's stage functions chained as the section says, the occlusion kernel equals its host
form byte for byte, batch contexts equal single-pair ones, forward-only contexts are untouched, and the outputs mean what they say."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_bidirectional_cpu import occlusion_cases

pytestmark = pytest.mark.gpu


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: shape/dtype {a.shape}{a.dtype} vs {b.shape}{b.dtype}"
    if a.dtype.kind == "f":
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    elif a.dtype.names:
        same = (a.view(np.uint8).reshape(a.shape + (-1,)) == b.view(np.uint8).reshape(b.shape + (-1,))).all(axis=-1)
    else:
        same = a == b
    n = int((~same).sum())
    assert n == 0, f"{what}: {n} of {same.size} elements differ"


def oracle_backward(st, params):
    """the backward branch as a chain of the oracle's stage entry points, from its own PatchMatch dump."""
    from oracle import oracle as O
    H, W = st["arrH"], st["arrW"]
    L = len(H) - 1
    _, _, n2, c2 = O.left_right_check(st["nnf1_pm"], st["cost1_pm"], st["nnf2_pm"], st["cost2_pm"])
    n2, c2 = O.outlier_removal(n2, c2)
    n2 = O.weighted_median(n2, st[f"img2_L{L}"], params.wmf_iters, True)
    n2 = O.fill_holes(n2, st[f"img2_L{L}"])
    f = O.nnf2flow(n2)
    levels = {L: f}
    for l in range(L - 1, -1, -1):
        f = O.mul_scalar(O.resize_flow(f, H[l], W[l], 2.0), 2.0)
        f = O.c2f_refine(f, st[f"img2_L{l}"], st[f"img1_L{l}"], st[f"cen2_L{l}"], st[f"cen1_L{l}"], params)
        f = O.flow_smoothing(f, st[f"img2_L{l}"])
        levels[l] = f
    levels[0] = O.flow_smoothing(f, st["img2_L0"])
    return n2, levels


def uv(f):
    return np.ascontiguousarray(f["x"]), np.ascontiguousarray(f["y"])


def check_against_oracle(a, b, st, ou, ov, **params):
    """One bidirectional call on (a, b) against the oracle's forward result and backward chain; returns the engine."""
    import eppm_amd
    from eppm_amd import io
    from oracle import oracle as O
    h, w, _ = a.shape
    e = eppm_amd.EPPM(params=eppm_amd.Params(**params) if params else None)
    e.init(a, b, h, w)
    fu, fv = e.compute_flow()
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    eq(u, fu, "forward u == eppm_compute"); eq(v, fv, "forward v == eppm_compute")
    eq(u, ou, "forward u == oracle"); eq(v, ov, "forward v == oracle")
    n2, levels = oracle_backward(st, O.default_params(**params))
    L = len(st["arrH"]) - 1
    eq(e.plane("nnf2", L), n2, "backward NNF after fill")
    for l, f in levels.items():
        eq(e.plane("flow_bwd", l), f, f"flow_bwd level {l}")
    eq(bu, uv(levels[0])[0], "bu"); eq(bv, uv(levels[0])[1], "bv")
    eq(o1, io.fb_occlusion(u, v, bu, bv), "occ1 == host criterion")
    eq(o2, io.fb_occlusion(bu, bv, u, v), "occ2 == host criterion")
    eq(e.plane("occ1", 0), o1, "plane occ1"); eq(e.plane("occ2", 0), o2, "plane occ2")
    u2, v2 = e.compute_flow()
    eq(u2, u, "eppm_compute after the bidirectional call, u"); eq(v2, v, "... v")
    return e, (u, v, bu, bv, o1, o2)


def test_backward_parity_crop(crop, crop_stages):
    st = crop_stages
    e, out = check_against_oracle(crop[0], crop[1], st, st["u"], st["v"])
    # the stage entries carry their own names, and a forward-only call adds none of them
    e.enable_stage_timing(True)
    e.compute_flow_bidirectional()
    names = [n for n, _ in e.stage_times()]
    for n in ("l2_post_bwd", "upsample_bwd_L1", "c2f_refine_bwd_L0", "flow_blf_bwd_L1", "flow_blf_bwd_final", "fb_occlusion"):
        assert n in names, names
    e.compute_flow()
    assert not [n for n, _ in e.stage_times() if "bwd" in n or n == "fb_occlusion"]
    e.close()


def _full(a, b, **params):
    from oracle import oracle as O
    ou, ov, st = O.compute_flow(a, b, O.default_params(**params) if params else None, dump=True)
    e, out = check_against_oracle(a, b, st, ou, ov, **params)
    e.close()
    return out


def test_backward_parity_bundled_pair(frames):
    _full(frames[0], frames[1])


def test_backward_parity_synthetic_1024x436():
    from eppm_amd import synth
    a, b, _, _ = synth.make_pair_cached(436, 1024, seed=5)
    _full(a, b)


@pytest.mark.parametrize("params", [dict(levels=1), dict(levels=2), dict(propagation=1)], ids=str)
def test_backward_parity_parameters(crop, params):
    _full(crop[0], crop[1], **params)


def test_backward_parity_patch_r17(crop):
    _full(crop[0][:96, :128].copy(), crop[1][:96, :128].copy(), patch_r=17)


def _device_occlusion(u, v, bu, bv, alpha, beta):
    from eppm_amd._lib import check, lib
    h, w = u.shape
    F = np.ascontiguousarray(np.stack([u, v], -1), np.float32)
    G = np.ascontiguousarray(np.stack([bu, bv], -1), np.float32)
    L = lib()
    dF, dG, dO = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(L.eppm_malloc_device(C.byref(dF), C.c_size_t(F.nbytes)), "malloc")
    check(L.eppm_malloc_device(C.byref(dG), C.c_size_t(G.nbytes)), "malloc")
    check(L.eppm_malloc_device(C.byref(dO), C.c_size_t(h * w)), "malloc")
    try:
        check(L.eppm_memcpy_h2d(dF, F.ctypes.data_as(C.c_void_p), C.c_size_t(F.nbytes)), "h2d")
        check(L.eppm_memcpy_h2d(dG, G.ctypes.data_as(C.c_void_p), C.c_size_t(G.nbytes)), "h2d")
        check(L.eppm_fb_occlusion(dO, dF, dG, h, w, C.c_float(alpha), C.c_float(beta)), "eppm_fb_occlusion")
        out = np.empty((h, w), np.uint8)
        check(L.eppm_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dO, C.c_size_t(h * w)), "d2h")
    finally:
        for p in (dF, dG, dO):
            L.eppm_free_device(p)
    return out


def test_occlusion_kernel_equals_host_form(frames):
    from eppm_amd import io
    cases = [c[:7] for c in occlusion_cases()]
    import eppm_amd
    e = eppm_amd.EPPM()
    e.init(frames[0], frames[1], 480, 640)
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    e.close()
    cases += [("bundled_fwd", u, v, bu, bv, 0.01, 0.5), ("bundled_bwd", bu, bv, u, v, 0.01, 0.5), ("bundled_a0", u, v, bu, bv, 0.0, 0.0),
              ("bundled_wide", u, v, bu, bv, 0.05, 2.0)]
    for name, a, b, c, d, alpha, beta in cases:
        eq(_device_occlusion(a, b, c, d, alpha, beta), io.fb_occlusion(a, b, c, d, alpha, beta), name)


def test_occlusion_params_reach_the_masks(crop):
    import eppm_amd
    from eppm_amd import io
    from eppm_amd._lib import lib
    e = eppm_amd.EPPM()
    e.init(crop[0], crop[1], 120, 160)
    u, v, bu, bv, o1, _ = e.compute_flow_bidirectional(alpha=0.0, beta=0.0)
    eq(o1, io.fb_occlusion(u, v, bu, bv, 0.0, 0.0), "alpha = beta = 0")
    _, _, _, _, o1b, _ = e.compute_flow_bidirectional(alpha=0.05, beta=1.5)
    eq(o1b, io.fb_occlusion(u, v, bu, bv, 0.05, 1.5), "alpha 0.05, beta 1.5")
    assert (o1b == 1).sum() <= (o1 == 1).sum()
    assert lib().eppm_set_occlusion_params(e._ctx, C.c_float(-1.0), C.c_float(0.5)) == 1
    assert lib().eppm_set_occlusion_params(e._ctx, C.c_float(0.01), C.c_float(float("nan"))) == 1
    e.close()


def test_state_errors(crop):
    import eppm_amd
    from eppm_amd._lib import lib
    e = eppm_amd.EPPM()
    e.init(120, 160)
    f = np.empty((120, 160), np.float32)
    p = f.ctypes.data_as(C.c_void_p)
    assert lib().eppm_compute_bidirectional(e._ctx, p, p, None, None, None, None) == 3          # before set_images
    assert lib().eppm_compute_bidirectional_device(e._ctx, None, None, None, None) == 3
    assert lib().eppm_compute_bidirectional(e._ctx, None, p, None, None, None, None) == 1
    e.set_data(crop[0], crop[1])
    e.compute_flow()
    g = np.empty((120, 160), np.uint8)
    assert lib().eppm_get_plane(e._ctx, b"occ1", 0, g.ctypes.data_as(C.c_void_p), C.c_size_t(g.nbytes)) == 3     # no bidirectional call yet
    e.compute_flow_bidirectional()
    assert lib().eppm_get_plane(e._ctx, b"occ1", 0, g.ctypes.data_as(C.c_void_p), C.c_size_t(g.nbytes)) == 0
    assert lib().eppm_get_plane(e._ctx, b"occ1", 1, g.ctypes.data_as(C.c_void_p), C.c_size_t(g.nbytes)) == 1     # level 0 only
    e.close()


def test_batch_equals_single_pairs():
    import eppm_amd
    from eppm_amd import synth
    from eppm_amd._lib import check, lib
    h, w = 120, 176
    pairs = []
    for k in range(8):
        a, b, _, _ = synth.make_pair(h, w, seed=100 + k, max_flow=4.0 + 3 * k)
        pairs.append((a, b) if k % 3 else (b, a))
    bat = eppm_amd.EPPMBatch(h, w, 8)
    bat.set_data(pairs)
    got = bat.compute_flow_bidirectional()
    fwd = bat.compute_flow()
    for k, (a, b) in enumerate(pairs):
        e = eppm_amd.EPPM()
        e.init(a, b, h, w)
        want = e.compute_flow_bidirectional()
        for name, x, y in zip(("u", "v", "bu", "bv", "occ1", "occ2"), got[k], want):
            eq(x, y, f"pair {k} {name}")
        eq(fwd[k][0], want[0], f"pair {k} forward-only u")
        # the device form of the same single-pair context
        d = [C.c_void_p() for _ in range(4)]
        sizes = [h * w * 8, h * w * 8, h * w, h * w]
        for p, n in zip(d, sizes):
            check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(n)), "malloc")
        e.compute_flow_bidirectional_device(*[p.value for p in d])
        e.synchronize()
        hf = [np.empty((h, w, 2), np.float32), np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)]
        for p, arr in zip(d, hf):
            check(lib().eppm_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), p, C.c_size_t(arr.nbytes)), "d2h")
            lib().eppm_free_device(p)
        eq(hf[0][..., 0], want[0], f"pair {k} device u"); eq(hf[1][..., 1], want[3], f"pair {k} device bv")
        eq(hf[2], want[4], f"pair {k} device occ1"); eq(hf[3], want[5], f"pair {k} device occ2")
        e.close()
    # the batch context's planes of the LAST bidirectional call need a new one (compute_flow above invalidated them)
    got = bat.compute_flow_bidirectional()
    for k in range(8):
        fb = bat.plane(k, "flow_bwd", 0)
        eq(np.ascontiguousarray(fb["x"]), got[k][2], f"pair {k} plane flow_bwd")
        eq(bat.plane(k, "occ1", 0), got[k][4], f"pair {k} plane occ1")
        eq(bat.plane(k, "occ2", 0), got[k][5], f"pair {k} plane occ2")
    bat.close()


def _free_bytes():
    from eppm_amd._lib import check, lib
    f, t = C.c_size_t(), C.c_size_t()
    check(lib().eppm_device_synchronize(), "sync")
    check(lib().eppm_device_mem_info(C.byref(f), C.byref(t)), "mem_info")
    return f.value


def test_memory_forward_only_untouched_and_bidirectional_grows_once():
    import eppm_amd
    from eppm_amd import synth
    from eppm_amd._lib import check, lib
    h, w = 1080, 1920
    a, b, _, _ = synth.make_pair_cached(h, w, seed=3, max_flow=8.0)
    e = eppm_amd.EPPM(); e.init(a, b, h, w); e.compute_flow_bidirectional(); e.close()      # code objects, pools
    check(lib().eppm_release_cached_memory(), "release")
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    created = _free_bytes()
    e.compute_flow()
    e.compute_flow()
    assert abs(created - _free_bytes()) < 2 << 20, (created, _free_bytes())             # forward only: nothing beyond the slab
    e.compute_flow_bidirectional()
    grown = created - _free_bytes()
    assert h * w * 8 <= grown <= h * w * 40 + (8 << 20), grown                           # the backward planes: once
    first = _free_bytes()
    e.compute_flow_bidirectional()
    e.compute_flow()
    assert abs(first - _free_bytes()) < 2 << 20, (first, _free_bytes())
    e.close()
    # create / bidirectional / destroy does not leak
    check(lib().eppm_release_cached_memory(), "release")
    level = _free_bytes()
    for _ in range(4):
        e = eppm_amd.EPPM(); e.init(a[:436, :1024].copy(), b[:436, :1024].copy(), 436, 1024); e.compute_flow_bidirectional(); e.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert abs(_free_bytes() - level) < 8 << 20, (level, _free_bytes())


def _shifted_pair(h, w, dx, dy, seed=21):
    """A textured image and its copy shifted by (dx, dy): I2(x, y) = I1(x - dx, y - dy), so the forward flow is (dx, dy)."""
    from eppm_amd import synth
    m = 32
    big, _, _, _ = synth.make_pair(h + 2 * m, w + 2 * m, seed=seed, max_flow=1.0)
    a = big[m:m + h, m:m + w].copy()
    b = big[m - dy:m - dy + h, m - dx:m - dx + w].copy()
    return a, b


def test_meaning_on_an_integer_shift():
    import eppm_amd
    h, w, dx, dy = 240, 320, 6, 4
    a, b = _shifted_pair(h, w, dx, dy)
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    e.close()
    m = 24
    ib, jb = slice(m, h - m), slice(m, w - m)
    # the sub-pixel refine and the smoothing leave the vectors within float rounding of the integer shift (measured: -5.999999, -4.0)
    mu, mv = float(np.median(bu[ib, jb])), float(np.median(bv[ib, jb]))
    assert abs(mu + dx) <= 1e-3 and abs(mv + dy) <= 1e-3, (mu, mv)
    near = (np.abs(bu[ib, jb] + dx) <= 0.5) & (np.abs(bv[ib, jb] + dy) <= 0.5)
    assert near.mean() >= 0.99, near.mean()
    assert (o1[ib, jb] == 0).mean() >= 0.95, np.bincount(o1[ib, jb].ravel())
    strip = o1[m:h - m, w - dx:]                     # content of image 1 that moves out of the right edge
    assert (strip == 2).mean() >= 0.90, np.bincount(strip.ravel())


TOL_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
from conftest import read_ppm, GOLDEN          # (selects the test library: overridden below, before anything is loaded)
import eppm_amd
eppm_amd.select_library(sys.argv[1])
from eppm_amd import synth
pairs = [("bundled", read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm")))]
for k in range(8):
    h, w = (96 + 24 * k, 128 + 40 * k)
    a, b, _, _ = synth.make_pair(h, w, seed=700 + k, max_flow=3.0 + 2 * k)
    pairs.append(("fuzz%%d" %% k, a, b))
out = {"version": eppm_amd.lib().eppm_version().decode()}
for name, a, b in pairs:
    h, w, _ = a.shape
    e = eppm_amd.EPPM(); e.init(a, b, h, w)
    fu, fv = e.compute_flow()
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    same = bool(np.array_equal(u.view(np.uint32), fu.view(np.uint32)) and np.array_equal(v.view(np.uint32), fv.view(np.uint32)))
    np.savez(os.path.join(sys.argv[2], name + ".npz"), bu=bu, bv=bv)
    out[name] = same
    e.close()
print(json.dumps(out))
""" % os.path.join(ROOT, "tests")


def test_tolerance_library_backward_inside_the_envelope(tmp_path):
    res = {}
    for variant in ("", "tol"):
        d = tmp_path / (variant or "exact")
        d.mkdir()
        p = subprocess.run([sys.executable, "-c", TOL_CHILD, variant, str(d)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        res[variant] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in res["tol"]["version"] and "tolerance" not in res[""]["version"]
    for name in ["bundled"] + ["fuzz%d" % k for k in range(8)]:
        assert res["tol"][name] is True and res[""][name] is True, name          # forward == that library's eppm_compute
        x, t = np.load(tmp_path / "exact" / (name + ".npz")), np.load(tmp_path / "tol" / (name + ".npz"))
        epe = float(np.sqrt((x["bu"] - t["bu"]) ** 2 + (x["bv"] - t["bv"]) ** 2).mean())
        assert epe <= (1e-3 if name == "bundled" else 3e-2), (name, epe)


def test_cli_backward_and_occlusion(frames, tmp_path):
    import eppm_amd
    from eppm_amd import io
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    f1, f2 = os.path.join(GOLDEN, "frame10.ppm"), os.path.join(GOLDEN, "frame11.ppm")
    plain, out, bwd, occ = (str(tmp_path / n) for n in ("plain.flo", "out.flo", "bwd.flo", "occ.pgm"))
    subprocess.run([exe, f1, f2, plain], check=True, capture_output=True, timeout=300)
    subprocess.run([exe, f1, f2, out, "--backward", bwd, "--occlusion", occ], check=True, capture_output=True, timeout=300)
    assert open(plain, "rb").read() == open(out, "rb").read()
    e = eppm_amd.EPPM()
    e.init(frames[0], frames[1], 480, 640)
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    e.close()
    cu, cv = io.load_flo(bwd)
    eq(cu, bu, "CLI backward u"); eq(cv, bv, "CLI backward v")
    data = open(occ, "rb").read()
    head = b"P5\n640 480\n255\n"
    assert data.startswith(head) and len(data) == len(head) + 640 * 480
    grey = np.frombuffer(data[len(head):], np.uint8).reshape(480, 640)
    eq(grey, np.array([0, 255, 128, 64], np.uint8)[o1], "CLI occlusion PGM")
