"""GPU tests of draft mode (eppm_set_stop_level).  The specification is the frozen CPU oracle: a level below the stop
level holds oracle flow_smoothing(2 * replicate2x(flow of the level above), the level's guide image), bit for bit (oracle_jbu of
test_draft_cpu.py); the levels from the stop level up are the full path's; with the stop level 0 nothing differs from a context that
never heard of the setting."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, read_ppm
from test_bidirectional_gpu import _free_bytes, eq
from test_draft_cpu import oracle_jbu

pytestmark = pytest.mark.gpu

UNKNOWN = np.float32(1e10)
ERR_ARG, ERR_STATE = 1, 3


def upsample(coarse, img):
    from eppm_amd import stages as S
    return S.flow_upsample(coarse, img)


def guide(w, h, seed):
    """a low-contrast guide (range weights stay non-zero) with a bright band, a dark block and a one-pixel line"""
    from oracle import oracle as O
    rng = np.random.default_rng([w, h, seed])
    rgb = rng.integers(90, 110, (h, w, 3), dtype=np.uint8)
    rgb[:, w // 3:w // 3 + 5] = 235
    rgb[h // 2:, w // 2:w // 2 + 40] = 12
    rgb[:, 2 * w // 3] = 0
    return O.rgb2rgba(rgb)


def coarse_flow(wc, hc, seed):
    from oracle import oracle as O
    rng = np.random.default_rng([wc, hc, seed])
    ys, xs = np.mgrid[0:hc, 0:wc]
    f = np.zeros((hc, wc), O.float2)
    f["x"] = (3.0 * np.sin(xs / 7.0) + 0.05 * ys + rng.normal(0, 0.3, (hc, wc))).astype(np.float32)
    f["y"] = (-2.0 * np.cos(xs / 11.0) + 0.03 * ys + rng.normal(0, 0.3, (hc, wc))).astype(np.float32)
    return f


# ---- 1. the kernel against the oracle ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 48), (211, 157)], ids=["64x48", "211x157"])
def test_kernel_equals_the_oracle(w, h):
    """one pixel per lane: whole tiles, and the odd size (clamp column and row of the coarse plane, partial tiles)"""
    wc, hc = int(w * 0.5), int(h * 0.5)
    img, F = guide(w, h, 1), coarse_flow(wc, hc, 2)
    eq(upsample(F, img), oracle_jbu(F, img), f"upsampling {w}x{h} <- {wc}x{hc}")


def test_kernel_unknown_blocks_and_the_fallback():
    """blocks of unknown coarse vectors larger than the 21x21 fine window, one inside and one touching the border: pixels whose whole window
    is unknown keep F'(x, y) = 2e10; isolated unknown vectors, a component exactly at half the threshold (known after doubling: strict >)
    and just above it (unknown after doubling), and negative components under an unknown one"""
    w, h = 211, 157
    wc, hc = int(w * 0.5), int(h * 0.5)
    img, F = guide(w, h, 3), coarse_flow(wc, hc, 4)
    rng = np.random.default_rng(9)
    m = rng.random((hc, wc))
    F["x"][m < 0.03] = UNKNOWN; F["y"][m < 0.03] = UNKNOWN
    F["x"][(m > 0.03) & (m < 0.04)] = np.float32(5e8)              # 2 * 5e8 = 1e9: not above the threshold
    F["y"][(m > 0.04) & (m < 0.05)] = np.float32(6e8)              # 1.2e9: unknown after doubling
    neg = (m > 0.05) & (m < 0.06)
    F["x"][neg] = UNKNOWN; F["y"][neg] = np.float32(-5.5)
    F["x"][20:40, 30:52] = UNKNOWN; F["y"][20:40, 30:52] = UNKNOWN           # 40 x 44 fine pixels
    F["x"][hc - 18:, wc - 20:] = UNKNOWN; F["y"][hc - 18:, wc - 20:] = UNKNOWN   # reaches the last row and column, the clamped ones included
    F["x"][:16, :18] = UNKNOWN; F["y"][:16, :18] = UNKNOWN
    want = oracle_jbu(F, img)
    for y, x in ((60, 82), (h - 1, w - 1), (0, 0), (h - 1, w - 12)):
        assert want["x"][y, x] == np.float32(2e10) and want["y"][y, x] == np.float32(2e10), (y, x, want[y, x])
    assert (want["x"] < 1e9).sum() > 20000
    eq(upsample(F, img), want, "upsampling with unknown blocks")


def test_kernel_two_pixels_per_lane():
    """the smallest 33- and 34-row launches that take two pixels per lane (the smoothing's rule and its test's shapes): odd height, the
    last row has no lower pixel; even height, it has; flows full of unknown vectors"""
    from test_variants_cpu import smoothing_cases
    from test_variants_gpu import smoothing_inputs
    from eppm_amd import stages as S
    done = 0
    for name, w, h, ppl in smoothing_cases():
        if ppl != 2:
            continue
        assert S.probe_dispatch("smoothing", w, h, 1) == (2,)
        img, fine = smoothing_inputs(w, h)
        F = np.ascontiguousarray(fine[::2, ::2][:int(h * 0.5), :int(w * 0.5)])
        eq(upsample(F, img), oracle_jbu(F, img), f"upsampling {name} {w}x{h}")
        done += 1
    assert done == 2


def test_upsample_arguments():
    import eppm_amd
    from eppm_amd._lib import lib
    assert lib().eppm_flow_upsample(None, 8, 8, None, 4, 4, None, C.c_size_t(32)) == ERR_ARG
    fake = C.c_void_p(256)               # refused before anything is read
    for h, w, hc, wc, pitch in ((0, 8, 4, 4, 32), (8, 0, 4, 4, 32), (8, 8, 0, 4, 32), (8, 8, 4, 0, 32), (8, 8, 4, 4, 28), (8, 8, 4, 4, 34)):
        assert lib().eppm_flow_upsample(fake, h, w, fake, hc, wc, fake, C.c_size_t(pitch)) == ERR_ARG, (h, w, hc, wc, pitch)


# ---- 2. contexts ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def pair(which):
    a, b = read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm"))
    if which == "crop":
        return a[180:300, 240:400].copy(), b[180:300, 240:400].copy()
    if which == "big":
        return a[120:360, 160:480].copy(), b[120:360, 160:480].copy()
    y, x = {"odd": (100, 100), "odd1": (200, 60), "odd2": (280, 380)}[which]
    return a[y:y + 157, x:x + 211].copy(), b[y:y + 157, x:x + 211].copy()


def engine(which, stop, **params):
    import eppm_amd
    a, b = pair(which)
    h, w, _ = a.shape
    e = eppm_amd.EPPM(params=eppm_amd.Params(**params) if params else None)
    e.init(a, b, h, w)
    e.set_stop_level(stop)
    assert e.stop_level() == stop
    return e


def check_levels(e, full, stop, name, guide_name):
    """planes `name` of the draft context e: the full context's from the stop level up, the oracle composition of e's OWN planes below"""
    nl = len(e.level_dims())
    for l in range(nl - 1, -1, -1):
        got = e.plane(name, l)
        if l >= stop:
            eq(got, full.plane(name, l), f"{name} level {l} (stop {stop}) == the full path's")
        else:
            eq(got, oracle_jbu(e.plane(name, l + 1), e.plane(guide_name, l)), f"{name} level {l} (stop {stop}) == oracle composition")


@pytest.mark.parametrize("which,params,stops", [("crop", {}, (1, 2)), ("odd", {}, (1, 2)), ("crop", {"patch_r": 17}, (1, 2)),
                                                ("crop", {"levels": 2}, (1,))], ids=["crop", "211x157", "crop_r17", "crop_levels2"])
def test_context_levels(which, params, stops):
    full = engine(which, 0, **params)
    full.compute_flow()
    for s in stops:
        e = engine(which, s, **params)
        u, v = e.compute_flow()
        check_levels(e, full, s, "flow", "img1")
        f0 = e.plane("flow", 0)
        eq(u, np.ascontiguousarray(f0["x"]), f"u == flow[0] (stop {s})"); eq(v, np.ascontiguousarray(f0["y"]), f"v == flow[0] (stop {s})")
        e.close()
    full.close()


# ---- 3. bidirectional -------------------------------------------------------------------------------------------------------------------

def test_bidirectional_draft():
    from eppm_amd import io
    a, b = pair("odd")
    full = engine("odd", 0)
    full.compute_flow_bidirectional()
    e = engine("odd", 1)
    u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
    check_levels(e, full, 1, "flow", "img1")
    check_levels(e, full, 1, "flow_bwd", "img2")
    f0, g0 = e.plane("flow", 0), e.plane("flow_bwd", 0)
    eq(u, np.ascontiguousarray(f0["x"]), "u"); eq(v, np.ascontiguousarray(f0["y"]), "v")
    eq(bu, np.ascontiguousarray(g0["x"]), "bu"); eq(bv, np.ascontiguousarray(g0["y"]), "bv")
    eq(o1, io.fb_occlusion(u, v, bu, bv), "occ1 == host criterion on the draft flows")
    eq(o2, io.fb_occlusion(bu, bv, u, v), "occ2 == host criterion on the draft flows")
    mid, = e.interpolate([0.5])
    eq(mid, io.interpolate(a, b, u, v, o1, o2, 0.5), "interpolate(0.5) == host form on the draft flows and masks")
    e.close(); full.close()


@pytest.mark.parametrize("which,params,stop", [("odd", {}, 2), ("big", {"levels": 4}, 3), ("big", {"levels": 4}, 2)], ids=["211x157_s2", "levels4_s3", "levels4_s2"])
def test_bidirectional_output_planes_alternate(which, params, stop):
    """the backward branch writes its upsamplings alternately into the level's scratch plane and the plane every smoothing writes: two and
    three upsamplings in a row, after a smoothing (s < nl - 1) and after nnf2flow (s = nl - 1); every level of both directions is checked"""
    full = engine(which, 0, **params)
    full.compute_flow_bidirectional()
    e = engine(which, stop, **params)
    u, v, bu, bv, _, _ = e.compute_flow_bidirectional()
    check_levels(e, full, stop, "flow", "img1")
    check_levels(e, full, stop, "flow_bwd", "img2")
    g0 = e.plane("flow_bwd", 0)
    eq(bu, np.ascontiguousarray(g0["x"]), "bu"); eq(bv, np.ascontiguousarray(g0["y"]), "bv")
    e.close(); full.close()


def test_batch_two_pixels_per_lane():
    """the smallest batch of 256x192 pairs whose level-0 launch takes two pixels per lane: k_flow_jbu<2> with a pair index above 0 (every
    slot another pair); slots 0, 9 and the last == the oracle composition of their own planes, in both directions"""
    import eppm_amd
    from eppm_amd import stages as S
    from test_variants_cpu import first_true
    h, w = 192, 256
    n = first_true(1, 4096, lambda k: S.probe_dispatch("smoothing", w, h, k) == (2,))
    assert n is not None and 1 < n <= 64 and S.probe_dispatch("smoothing", w, h, n - 1) == (1,), n
    a, b = read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm"))
    pairs = [(a[5 * k:5 * k + h, 10 * k:10 * k + w].copy(), b[5 * k:5 * k + h, 10 * k:10 * k + w].copy()) for k in range(n)]
    bat = eppm_amd.EPPMBatch(h, w, n)
    bat.set_stop_level(1)
    bat.set_data(pairs)
    got = bat.compute_flow_bidirectional()
    for k in (0, 9, n - 1):
        for name, guide_name, (fx, fy) in (("flow", "img1", got[k][0:2]), ("flow_bwd", "img2", got[k][2:4])):
            want = oracle_jbu(bat.plane(k, name, 1), bat.plane(k, guide_name, 0))
            eq(bat.plane(k, name, 0), want, f"slot {k} {name} level 0 == oracle composition")
            eq(fx, np.ascontiguousarray(want["x"]), f"slot {k} {name} x"); eq(fy, np.ascontiguousarray(want["y"]), f"slot {k} {name} y")
    bat.close()


# ---- 4. batch and streaming -------------------------------------------------------------------------------------------------------------

def test_batch_equals_single_contexts():
    import eppm_amd
    names = ("odd", "odd1", "odd2")
    bat = eppm_amd.EPPMBatch(157, 211, 3)
    bat.set_stop_level(1)
    assert bat.stop_level() == 1
    bat.set_data([pair(n) for n in names])
    got = bat.compute_flow_bidirectional()
    for k, n in enumerate(names):
        e = engine(n, 1)
        want = e.compute_flow_bidirectional()
        for g, x, what in zip(got[k], want, ("u", "v", "bu", "bv", "occ1", "occ2")):
            eq(g, x, f"slot {k} {what}")
        for l in range(3):
            eq(bat.plane(k, "flow", l), e.plane("flow", l), f"slot {k} flow level {l}")
            eq(bat.plane(k, "flow_bwd", l), e.plane("flow_bwd", l), f"slot {k} flow_bwd level {l}")
        e.close()
    bat.close()


def test_temporal_step_batch_equals_single_stream():
    """one seeded step at stop level 1: set_data, compute, push, compute -- every slot of the batch == a single-pair stream"""
    import eppm_amd
    names = ("odd", "odd1", "odd2")
    third = {n: np.roll(pair(n)[1], (1, -2), axis=(0, 1)) for n in names}
    bat = eppm_amd.EPPMBatch(157, 211, 3)
    bat.set_temporal(True)
    bat.set_stop_level(1)
    bat.set_data([pair(n) for n in names])
    first = bat.compute_flow()
    bat.push_frames([third[n] for n in names])
    assert all(bat.temporal_valid(k) for k in range(3))
    second = bat.compute_flow()
    for k, n in enumerate(names):
        e = engine(n, 1)
        e.set_temporal(True)
        u, v = e.compute_flow()
        eq(u, first[k][0], f"slot {k} first pair u"); eq(v, first[k][1], f"slot {k} first pair v")
        e.push_frame(third[n])
        assert e.temporal_valid()
        u, v = e.compute_flow()
        eq(second[k][0], u, f"slot {k} seeded pair u"); eq(second[k][1], v, f"slot {k} seeded pair v")
        e.close()
    bat.close()


# ---- 5. off means off -------------------------------------------------------------------------------------------------------------------

def test_off_means_off():
    from eppm_amd._lib import check, lib
    fresh = engine("odd", 0)
    fu, fv = fresh.compute_flow()
    fresh.enable_stage_timing(True)
    fresh.compute_flow_bidirectional()
    names0 = [n for n, _ in fresh.stage_times()]
    assert not [n for n in names0 if "flow_jbu" in n] and "flow_blf_final" in names0 and "c2f_refine_L0" in names0, names0
    fresh.close()
    check(lib().eppm_release_cached_memory(), "release")
    e = engine("odd", 0)
    e.enable_stage_timing(True)
    e.compute_flow()
    e.stage_times()
    created = _free_bytes()
    e.set_stop_level(1)
    u1, v1 = e.compute_flow()
    names1 = [n for n, _ in e.stage_times()]
    assert "flow_jbu_L0" in names1 and "flow_blf_L1" in names1, names1
    assert not [n for n in names1 if n in ("c2f_refine_L0", "upsample_L0", "flow_blf_L0", "flow_blf_final")], names1
    assert (u1.view(np.uint32) != fu.view(np.uint32)).any()
    assert abs(created - _free_bytes()) < 2 << 20, (created, _free_bytes())          # the setting allocates nothing
    e.compute_flow_bidirectional()
    names1 = [n for n, _ in e.stage_times()]
    assert "flow_jbu_bwd_L0" in names1 and "flow_blf_bwd_final" not in names1 and "c2f_refine_bwd_L0" not in names1, names1
    e.set_stop_level(2)
    e.compute_flow()
    names2 = [n for n, _ in e.stage_times()]
    assert "flow_jbu_L1" in names2 and "flow_jbu_L0" in names2 and not [n for n in names2 if n.startswith(("c2f_refine", "flow_blf", "upsample"))], names2
    e.set_stop_level(0)
    u0, v0 = e.compute_flow()
    eq(u0, fu, "u after 1 -> 2 -> 0 == a fresh context's"); eq(v0, fv, "v after 1 -> 2 -> 0 == a fresh context's")
    assert [n for n, _ in e.stage_times()] == [n for n in names0 if "bwd" not in n and n != "fb_occlusion"]
    e.close()


# ---- 6. state and arguments -------------------------------------------------------------------------------------------------------------

def test_state_and_arguments():
    import eppm_amd
    from eppm_amd._lib import lib
    e = engine("crop", 0)
    nl = len(e.level_dims())
    for bad in (-1, nl):
        assert lib().eppm_set_stop_level(e._ctx, bad) == ERR_ARG
        assert e.stop_level() == 0
    assert lib().eppm_set_stop_level(None, 0) == ERR_ARG and lib().eppm_stop_level(None) == -1
    e.compute_flow_bidirectional()
    e.interpolate([0.5])
    e.set_stop_level(1)
    ts = (C.c_float * 1)(0.5)
    out = np.empty((e.h, e.w, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(out.ctypes.data)
    assert lib().eppm_interpolate(e._ctx, 1, ts, ptrs, C.c_size_t(e.w * 3)) == ERR_STATE          # the planes are the other setting's
    trk = eppm_amd.Tracker(e, 0)
    try:
        with pytest.raises(eppm_amd.EppmError, match="status 3"):
            trk.step()
    finally:
        trk.close()
    e.compute_flow_bidirectional()
    e.interpolate([0.5])
    e.close()
    e = engine("crop", 0)
    e.compute_flow_begin()
    assert lib().eppm_set_stop_level(e._ctx, 1) == ERR_STATE and e.stop_level() == 0          # a compute is pending: refused, nothing changes
    e.compute_flow_end()
    assert lib().eppm_set_stop_level(e._ctx, 1) == 0
    e.close()
    two = engine("crop", 1, levels=2)
    assert lib().eppm_set_stop_level(two._ctx, 2) == ERR_ARG
    two.close()
    bat = eppm_amd.EPPMBatch(120, 160, 2)
    assert lib().eppm_set_stop_level(bat._ctx, 3) == ERR_ARG and lib().eppm_set_stop_level(bat._ctx, 2) == 0
    bat.close()


# ---- 7. the tolerance library -----------------------------------------------------------------------------------------------------------

def test_tolerance_library_levels_below_the_stop_level():
    """in a child process that loads the tolerance library: at stop level 1, level 0 (forward and backward) is the oracle composition of
    the library's OWN level-1 flow, bit for bit -- the smoothing arithmetic is exact in both libraries"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "draft_tol_child.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert lines and "tolerance arithmetic" in lines[0] and lines[-1] == "PART OK", p.stdout[-2000:]


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------------------

def test_cli_stop_level(tmp_path):
    import eppm_amd
    from eppm_amd import io
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    out, bwd = str(tmp_path / "f.flo"), str(tmp_path / "b.flo")
    f10, f11 = os.path.join(GOLDEN, "frame10.ppm"), os.path.join(GOLDEN, "frame11.ppm")
    subprocess.check_call([exe, "--stop-level", "1", "--backward", bwd, f10, f11, out], timeout=120)
    e = eppm_amd.EPPM()
    e.init(read_ppm(f10), read_ppm(f11), 480, 640)
    e.set_stop_level(1)
    u, v, bu, bv, _, _ = e.compute_flow_bidirectional()
    e.close()
    cu, cv = io.load_flo(out)
    eq(cu, u, "CLI u at stop level 1"); eq(cv, v, "CLI v at stop level 1")
    cu, cv = io.load_flo(bwd)
    eq(cu, bu, "CLI bu at stop level 1"); eq(cv, bv, "CLI bv at stop level 1")
    p = subprocess.run([exe, "--stop-level", "3", f10, f11, out], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "usage: runeppm" in p.stderr, (p.returncode, p.stderr)
