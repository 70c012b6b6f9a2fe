"""GPU tests of the streaming mode: a pushed frame leaves the context as set_images of the same pair would, bit
for bit; temporal mode off, unused or reset is eppm_compute; the advection kernels equal their host form; the seeded start equals the
numpy select over the oracle's two cost fields; and the whole seeded path equals the CPU oracle's stage functions chained from the same
initial field.  Every test runs under a time limit of its own."""
import ctypes as C
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_bidirectional_gpu import eq, oracle_backward, uv
from test_temporal_cpu import UNKNOWN, displacement, make_clip, prior_or, random_field, select, PRIOR_CASES

pytestmark = pytest.mark.gpu

TEST_SECONDS = 600


@pytest.fixture(autouse=True)
def time_limit():
    def on_alarm(signum, frame):
        raise TimeoutError(f"test exceeded {TEST_SECONDS} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


PLANES = ["img1", "img2", "census1", "census2"]


def all_planes(e):
    out = {}
    for l in range(len(e.level_dims())):
        for n in PLANES:
            out[(n, l)] = e.plane(n, l)
    return out


def rgba_dev(img):
    """(h, w, 3) uint8 -> a pitched device RGBA plane (eppm_amd.stages.Dev)"""
    from eppm_amd import stages
    from eppm_amd.api import uchar4
    h, w, _ = img.shape
    a = np.zeros((h, w), uchar4)
    a["x"], a["y"], a["z"] = img[..., 0], img[..., 1], img[..., 2]
    return stages.Dev(a, pitched=True)


def rng_states(e):
    import eppm_amd
    h, w = e.level_dims()[-1]
    nb = ((w + 15) // 16) * ((h + 15) // 16)
    out = np.zeros((nb, 6), np.uint32)
    eppm_amd._lib.check(eppm_amd.lib().eppm_probe_ctx_rng_states(e._ctx, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size)), "rng states")
    return out


# ---- push ----

@pytest.mark.parametrize("h,w", [(436, 1024), (480, 640), (157, 211)])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_push_equals_set_images(h, w, device_form):
    import eppm_amd
    frames, _, _ = make_clip(h, w, 31, n=3, max_flow=8.0)
    a, b, c = frames
    ref = eppm_amd.EPPM()
    ref.init(b, c, h, w)
    want, (wu, wv) = all_planes(ref), ref.compute_flow()
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()                      # the slab's scratch planes have been used, as in a stream
    if device_form:
        d = rgba_dev(c)
        e.push_frame_device(d.ptr.value, d.pitch)
        e.synchronize()
    else:
        e.push_frame(c)
    got = all_planes(e)
    for k in want:
        eq(got[k], want[k], f"plane {k} after push")
    u, v = e.compute_flow()
    eq(u, wu, "u after push"); eq(v, wv, "v after push")
    for l in range(len(e.level_dims())):
        eq(e.plane("flow", l), ref.plane("flow", l), f"flow level {l}")
    # a second push, and the bidirectional call on pushed planes
    e.push_frame(a)
    ref.set_data(c, a)
    r1, r2 = e.compute_flow_bidirectional(), ref.compute_flow_bidirectional()
    for x, y, n in zip(r1, r2, ("u", "v", "bu", "bv", "occ1", "occ2")):
        eq(x, y, f"bidirectional {n} after two pushes")
    e.close(); ref.close()


def test_push_host_memory_forms_equal_set_images(crop):
    """eppm_push_image from every kind of caller memory, temporal mode off: plain contiguous memory and plain memory with padded rows (both
    through the pinned staging, whose two buffers wrap around: set_data took the first), then padded rows in memory from eppm_host_alloc
    (read in place by DMA; the source is overwritten as soon as the call returns).  After each push the planes of both images at every
    level and the flow equal those of set_data on the same pair in a second context, bit for bit."""
    import eppm_amd
    from eppm_amd._lib import check
    L = eppm_amd.lib()
    a, b = crop
    h, w = 120, 160
    f = [a, b, np.roll(b, 3, axis=1), np.roll(b, (2, -4), axis=(0, 1)), b]
    stride = 3 * (w + 13)
    plain = f[2].copy()
    padded = np.full((h, w + 13, 3), 0xA5, np.uint8)
    padded[:, :w] = f[3]
    pinned = eppm_amd.pinned_empty((h, w + 13, 3))
    pinned[:] = 0x5A
    pinned[:, :w] = f[4]
    sources = [(plain, 3 * w, "plain"), (padded, stride, "plain, padded rows"), (pinned, stride, "registered, padded rows")]
    for src, _, what in sources:
        assert L.eppm_host_is_registered(C.c_void_p(src.ctypes.data), C.c_size_t(src.nbytes)) == int(src is pinned), what
    ref = eppm_amd.EPPM()
    ref.init(h, w)
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_data(f[0], f[1])
    e.compute_flow()
    for i, (src, row_stride, what) in enumerate(sources, start=1):
        check(L.eppm_push_image(e._ctx, C.c_void_p(src.ctypes.data), C.c_size_t(row_stride)), "eppm_push_image")
        if src is pinned:
            src[:] = 0                       # the push has consumed the image when it returns
        ref.set_data(f[i], f[i + 1])
        want, got = all_planes(ref), all_planes(e)
        for k in want:
            eq(got[k], want[k], f"plane {k} after push {i} ({what})")
        (u, v), (wu, wv) = e.compute_flow(), ref.compute_flow()
        eq(u, wu, f"u after push {i} ({what})"); eq(v, wv, f"v after push {i} ({what})")
    e.close(); ref.close()


def test_state_errors_and_defaults():
    import eppm_amd
    L = eppm_amd.lib()
    h, w = 96, 128
    frames, _, _ = make_clip(h, w, 5, n=3, max_flow=4.0)
    e = eppm_amd.EPPM()
    e.init(h, w)
    assert not e.temporal_valid()
    img = np.ascontiguousarray(frames[2])
    assert L.eppm_push_image(e._ctx, img.ctypes.data_as(C.c_void_p), C.c_size_t(w * 3)) == 3          # EPPM_ERR_STATE: no pair yet
    d = rgba_dev(img)
    assert L.eppm_push_image_device(e._ctx, d.ptr, C.c_size_t(d.pitch)) == 3
    e.set_data(frames[0], frames[1])
    assert L.eppm_push_image(e._ctx, img.ctypes.data_as(C.c_void_p), C.c_size_t(w * 3 - 1)) == 1      # row_stride < 3 w
    e.compute_flow()
    assert not e.temporal_valid()                              # off by default
    with pytest.raises(eppm_amd.EppmError):
        e.plane("prior1", 2)
    e.set_temporal(True)
    u0, v0 = e.compute_flow()
    assert not e.temporal_valid()                              # only a push arms the prior:
    u1, v1 = e.compute_flow()                                  # a second compute on the same pair is the same cold run
    eq(u1, u0, "second compute on one pair: u"); eq(v1, v0, "second compute on one pair: v")
    e.push_frame(frames[2])
    assert e.temporal_valid()
    e.temporal_reset()
    assert not e.temporal_valid()
    e.compute_flow()
    e.set_data(frames[0], frames[1])                           # a new pair is a new clip
    assert not e.temporal_valid()
    e.compute_flow()
    e.push_frame(frames[2])                                    # a push directly after a compute arms it
    assert e.temporal_valid()
    e.push_frame(frames[0])                                    # a second push without a compute: the fields are a pair too old
    assert not e.temporal_valid()
    e.compute_flow()
    e.push_frame(frames[1])
    assert e.temporal_valid()
    e.set_temporal(False)
    assert not e.temporal_valid()
    e.close()
    bat = eppm_amd.EPPMBatch(h, w, 2)
    bat.set_data([(frames[0], frames[1]), (frames[1], frames[2])])
    assert L.eppm_set_temporal(bat._ctx, 1) == 1               # EPPM_ERR_ARG
    assert L.eppm_push_image(bat._ctx, img.ctypes.data_as(C.c_void_p), C.c_size_t(w * 3)) == 1
    assert L.eppm_push_image_device(bat._ctx, d.ptr, C.c_size_t(d.pitch)) == 1
    assert L.eppm_set_temporal(bat._ctx, 0) == 0
    bat.close()


# ---- off means off ----

def free_bytes():
    import eppm_amd
    f, t = C.c_size_t(), C.c_size_t()
    eppm_amd._lib.check(eppm_amd.lib().eppm_device_mem_info(C.byref(f), C.byref(t)), "mem_info")
    return f.value


def test_off_means_off():
    import eppm_amd
    h, w = 436, 1024
    frames, _, _ = make_clip(h, w, 1234, n=3)
    a, b, c = frames
    fresh = eppm_amd.EPPM()
    fresh.init(b, c, h, w)
    wu, wv = fresh.compute_flow()
    cold_states = rng_states(fresh)
    fresh.close()
    eppm_amd.lib().eppm_release_cached_memory()
    # never enabled: the same flow, and a push and a compute allocate nothing
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()
    m0 = free_bytes()
    e.push_frame(c)
    u, v = e.compute_flow()
    assert free_bytes() == m0
    eq(u, wu, "never enabled: u"); eq(v, wv, "never enabled: v")
    e.close()
    # the temporal planes are allocated by the first compute with the mode on, not by eppm_create or eppm_set_temporal
    eppm_amd.lib().eppm_release_cached_memory()
    base = free_bytes()
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()
    plain = base - free_bytes()
    e.close()
    eppm_amd.lib().eppm_release_cached_memory()
    assert free_bytes() == base
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.set_temporal(True)
    e.set_temporal(False)
    e.compute_flow()
    assert base - free_bytes() == plain, "a context that never computed in temporal mode holds what a plain one holds"
    e.set_temporal(True)
    e.compute_flow()
    lh, lw = e.level_dims()[-1]
    # 40 bytes per level-L pixel, which the allocator may round up or carve out of a block it holds already
    assert plain <= base - free_bytes() <= plain + 40 * lh * lw + (4 << 20)
    e.close()
    eppm_amd.lib().eppm_release_cached_memory()
    # enabled on the first pair of a clip
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_temporal(True)
    e.set_data(b, c)
    u, v = e.compute_flow()
    eq(u, wu, "enabled, first pair: u"); eq(v, wv, "enabled, first pair: v")
    # after a reset
    e.set_data(a, b)
    e.compute_flow()
    e.push_frame(c)
    assert e.temporal_valid()
    e.temporal_reset()
    u, v = e.compute_flow()
    eq(u, wu, "after reset: u"); eq(v, wv, "after reset: v")
    eq(rng_states(e), cold_states, "generator states after a cold run in temporal mode")
    # a seeded run differs (the mode does something) and leaves the generator where a cold run leaves it
    e.set_data(a, b)
    e.compute_flow()
    e.push_frame(c)
    e.enable_stage_timing(True)
    e.stage_times()
    su, sv = e.compute_flow()
    names = [n for n, _ in e.stage_times()]
    assert "temporal_advect" in names and "temporal_select" in names and names.count("patchmatch") == 1, names
    assert not (np.array_equal(su, wu) and np.array_equal(sv, wv))
    eq(rng_states(e), cold_states, "generator states after a seeded run")
    e.close()


# ---- stages ----

@pytest.mark.parametrize("h,w,spread,unknown", PRIOR_CASES)
@pytest.mark.parametrize("backward", [False, True])
def test_prior_kernels_equal_host_form(h, w, spread, unknown, backward):
    from eppm_amd import io, stages
    rng = np.random.default_rng(h * 77 + w + int(backward))
    for _ in range(2):                                         # twice: the second call finds the scratch as the first left it
        prev = random_field(rng, h, w, spread, unknown)
        eq(stages.temporal_prior(prev, backward), io.temporal_prior(prev, backward), "eppm_temporal_prior == host form")


# ---- whole path ----

def oracle_forward_from(n1, c1, n2, c2, st, params):
    """the forward branch after PatchMatch as a chain of the oracle's stage entry points (oracle_backward's mirror image)"""
    from oracle import oracle as O
    H, W = st["arrH"], st["arrW"]
    L = len(H) - 1
    n1, c1, _, _ = O.left_right_check(n1, c1, n2, c2)
    n1, c1 = O.outlier_removal(n1, c1)
    n1 = O.weighted_median(n1, st[f"img1_L{L}"], params.wmf_iters, True)
    n1 = O.fill_holes(n1, st[f"img1_L{L}"])
    f = O.nnf2flow(n1)
    levels = {L: f}
    for l in range(L - 1, -1, -1):
        f = O.mul_scalar(O.resize_flow(f, H[l], W[l], 2.0), 2.0)
        f = O.c2f_refine(f, st[f"img1_L{l}"], st[f"img2_L{l}"], st[f"cen1_L{l}"], st[f"cen2_L{l}"], params)
        f = O.flow_smoothing(f, st[f"img1_L{l}"])
        levels[l] = f
    levels[0] = O.flow_smoothing(f, st["img1_L0"])
    return n1, levels


def oracle_planes(x, y, nl=3):
    from oracle import oracle as O
    px, py = O.prepare(O.rgb2rgba(x), nl), O.prepare(O.rgb2rgba(y), nl)
    st = {"arrH": [i.shape[0] for i in px[0]], "arrW": [i.shape[1] for i in px[0]]}
    for l in range(nl):
        st[f"img1_L{l}"], st[f"cen1_L{l}"], st[f"img2_L{l}"], st[f"cen2_L{l}"] = px[0][l], px[1][l], py[0][l], py[1][l]
    return st


def oracle_seeded_patchmatch(st, prior1, prior2, params):
    """both problems of a pair from the select over the oracle's two cost fields, then num_iter x [four sweeps + search]"""
    from oracle import oracle as O
    L = len(st["arrH"]) - 1
    i1, i2, c1, c2 = st[f"img1_L{L}"], st[f"img2_L{L}"], st[f"cen1_L{L}"], st[f"cen2_L{L}"]
    h, w = i1.shape
    rand, states0 = O.gen_rand_field(w, h, params.seed)
    out = []
    for prior, (a, b, ca, cb) in ((prior1, (i1, i2, c1, c2)), (prior2, (i2, i1, c2, c1))):
        cr = O.cost_field(rand, a, b, ca, cb, params)
        cp = O.cost_field(prior_or(prior, rand), a, b, ca, cb, params)
        nnf, cost = select(rand, cr, prior, cp)
        init = (nnf.copy(), cost.copy())
        states = states0.copy()
        for _ in range(params.num_iter):
            for d in range(4):
                cost, nnf = O.seg_propagate_dir(cost, nnf, a, b, ca, cb, d, params)
            states, cost, nnf = O.random_search(states, cost, nnf, a, b, ca, cb, params)
        out.append((nnf, cost, init, states))
    return out


def check_stream(frames, bidirectional, **params):
    """frames through one context in temporal mode; pairs 1.. against the oracle chain seeded from the previous pair's oracle fields"""
    import eppm_amd
    from eppm_amd import io
    from oracle import oracle as O
    prm = O.default_params(**params)
    h, w, _ = frames[0].shape
    e = eppm_amd.EPPM(params=eppm_amd.Params(**params) if params else None)
    e.init(h, w)
    e.set_temporal(True)
    e.set_data(frames[0], frames[1])
    res = e.compute_flow_bidirectional() if bidirectional else e.compute_flow()
    ou, ov, st = O.compute_flow(frames[0], frames[1], prm, dump=True)
    eq(res[0], ou, "pair 0 (cold) u"); eq(res[1], ov, "pair 0 (cold) v")
    L = len(st["arrH"]) - 1
    prev_fwd, prev_bwd = displacement(st["nnf1_fill"]), displacement(st["nnf2_pm"])
    for k in range(1, len(frames) - 1):
        e.push_frame(frames[k + 1])
        res = e.compute_flow_bidirectional() if bidirectional else e.compute_flow()
        prior1, prior2 = io.temporal_prior(prev_fwd, False), io.temporal_prior(prev_bwd, True)
        eq(e.plane("prior1", L), prior1, f"pair {k}: prior1"); eq(e.plane("prior2", L), prior2, f"pair {k}: prior2")
        assert ((prior1["x"] > UNKNOWN).mean() > 0.3) and ((prior2["x"] > UNKNOWN).mean() > 0.3)
        st = oracle_planes(frames[k], frames[k + 1], prm.levels)
        (n1, c1, init1, _), (n2, c2, init2, _) = oracle_seeded_patchmatch(st, prior1, prior2, prm)
        eq(e.plane("nnf_init1", L), init1[0], f"pair {k}: nnf_init1"); eq(e.plane("cost_init1", L), init1[1], f"pair {k}: cost_init1")
        eq(e.plane("nnf_init2", L), init2[0], f"pair {k}: nnf_init2"); eq(e.plane("cost_init2", L), init2[1], f"pair {k}: cost_init2")
        fill1, levels = oracle_forward_from(n1, c1, n2, c2, st, prm)
        for l, f in levels.items():
            eq(e.plane("flow", l), f, f"pair {k}: flow level {l}")
        eq(res[0], uv(levels[0])[0], f"pair {k}: u"); eq(res[1], uv(levels[0])[1], f"pair {k}: v")
        if bidirectional:
            st.update(nnf1_pm=n1, cost1_pm=c1, nnf2_pm=n2, cost2_pm=c2)
            _, blev = oracle_backward(st, prm)
            for l, f in blev.items():
                eq(e.plane("flow_bwd", l), f, f"pair {k}: flow_bwd level {l}")
            eq(res[2], uv(blev[0])[0], f"pair {k}: bu"); eq(res[3], uv(blev[0])[1], f"pair {k}: bv")
        prev_fwd, prev_bwd = displacement(fill1), displacement(n2)
    e.close()


@pytest.mark.parametrize("num_iter", [10, 6])
@pytest.mark.parametrize("bidirectional", [False, True], ids=["forward", "bidirectional"])
def test_seeded_path_equals_oracle_chain(num_iter, bidirectional):
    frames, _, _ = make_clip(192, 256, 77, n=4, max_flow=10.0)
    check_stream(frames, bidirectional, num_iter=num_iter)


def test_seeded_path_equals_oracle_chain_1024x436():
    frames, _, _ = make_clip(436, 1024, 1234, n=4)
    check_stream(frames, True)


def test_seeded_initial_cost_never_above_cold():
    import eppm_amd
    from oracle import oracle as O
    h, w = 436, 1024
    frames, _, _ = make_clip(h, w, 1234, n=3)
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_temporal(True)
    e.set_data(frames[0], frames[1])
    e.compute_flow()
    e.push_frame(frames[2])
    e.compute_flow()
    L = 2
    st = oracle_planes(frames[1], frames[2])
    rand, _ = O.gen_rand_field(st["arrW"][L], st["arrH"][L])
    cold = O.cost_field(rand, st[f"img1_L{L}"], st[f"img2_L{L}"], st[f"cen1_L{L}"], st[f"cen2_L{L}"])
    got = e.plane("cost_init1", L)
    assert (got <= cold).all() and (got < cold).mean() > 0.3
    e.close()


# ---- users of the stream ----

def test_flow_sequence_and_streaming_tracks():
    import eppm_amd
    h, w = 192, 256
    frames, _, _ = make_clip(h, w, 9, n=4, max_flow=6.0)
    flows = eppm_amd.flow_sequence(frames, bidirectional=True)
    assert len(flows) == 3
    cold = eppm_amd.flow_sequence(frames, temporal=False)
    e = eppm_amd.EPPM()
    for k in range(3):
        e.init(frames[k], frames[k + 1], h, w)
        u, v = e.compute_flow()
        eq(cold[k][0], u, f"flow_sequence(temporal=False) pair {k}: u"); eq(cold[k][1], v, "... v")
    e.close()
    eq(flows[0][0], cold[0][0], "the first pair of a clip is cold")
    # the tracker fed the same flows by hand
    from eppm_amd import io, stages
    from eppm_amd.api import float2
    got = eppm_amd.track_sequence(frames, streaming=True)
    ctx = eppm_amd.EPPM()
    ctx.init(h, w)
    trk = eppm_amd.Tracker(ctx)
    want = {i: {"start": 0, "positions": [xy], "reason": None} for i, xy in enumerate(io.track_seeds(frames[0], trk.params)[:trk.capacity])}
    for k in range(3):
        u, v, bu, bv, _, _ = flows[k]
        f, g = np.zeros((h, w), float2), np.zeros((h, w), float2)
        f["x"], f["y"], g["x"], g["y"] = u, v, bu, bv
        d1, d2, df, dg = rgba_dev(frames[k]), rgba_dev(frames[k + 1]), stages.Dev(f), stages.Dev(g)
        trk.step_frames(d1.ptr.value, d2.ptr.value, d1.pitch, df.ptr.value, dg.ptr.value)
        eppm_amd.api._track_collect(want, trk)
    trk.close(); ctx.close()
    assert sorted(got) == sorted(want) and len(got) > 50
    for i in want:
        assert got[i]["start"] == want[i]["start"] and got[i]["reason"] == want[i]["reason"], i
        eq(got[i]["positions"], np.asarray(want[i]["positions"], np.float32).reshape(-1, 2), f"track {i}")


def test_cli_sequence(tmp_path):
    import eppm_amd
    from eppm_amd import io
    h, w = 120, 160
    frames, _, _ = make_clip(h, w, 3, n=4, max_flow=5.0)
    names = []
    for k, f in enumerate(frames):
        names.append(str(tmp_path / f"f{k}.ppm"))
        with open(names[-1], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h) + f.tobytes())
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    for temporal in (1, 0):
        prefix = str(tmp_path / f"t{temporal}")
        subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--temporal", str(temporal)], check=True, capture_output=True, timeout=300)
        want = eppm_amd.flow_sequence(frames, temporal=bool(temporal))
        for k in range(3):
            u, v = io.load_flo(f"{prefix}_{k + 1:04d}.flo")
            eq(u, want[k][0], f"CLI temporal={temporal} pair {k}: u"); eq(v, want[k][1], "... v")
    assert subprocess.run([exe, "--sequence", names[0], "--out-prefix", str(tmp_path / "x")], capture_output=True, timeout=60).returncode == 2
    for stray in (["--pin"], ["--gt", names[0]], ["--batch", "2"], ["--backward", str(tmp_path / "b.flo")], ["--size", "64x64"]):
        assert subprocess.run([exe, "--sequence", *names, "--out-prefix", str(tmp_path / "x"), *stray], capture_output=True, timeout=60).returncode == 2, stray


# ---- the tolerance library: the same stream, inside its envelope around the exact library ----

TOL_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import conftest                                   # (selects the test library: overridden below, before anything is loaded)
import eppm_amd
eppm_amd.select_library(sys.argv[1])
from test_temporal_cpu import make_clip
out = {"version": eppm_amd.lib().eppm_version().decode()}
for name, (h, w, seed, mf) in {"clip1024": (436, 1024, 1234, 20.0), "clip256": (192, 256, 77, 10.0)}.items():
    frames, _, _ = make_clip(h, w, seed, n=4, max_flow=mf)
    flows = eppm_amd.flow_sequence(frames, bidirectional=True)
    np.savez(os.path.join(sys.argv[2], name + ".npz"), **{"f%%d_%%d" %% (k, j): flows[k][j] for k in range(3) for j in range(4)})
    # push == set_images and off == eppm_compute hold inside any one library
    e = eppm_amd.EPPM(); e.init(frames[0], frames[1], h, w); e.compute_flow(); e.push_frame(frames[2]); u, v = e.compute_flow(); e.close()
    r = eppm_amd.EPPM(); r.init(frames[1], frames[2], h, w); ru, rv = r.compute_flow(); r.close()
    out[name] = bool(np.array_equal(u.view(np.uint32), ru.view(np.uint32)) and np.array_equal(v.view(np.uint32), rv.view(np.uint32)))
print(json.dumps(out))
""" % os.path.join(ROOT, "tests")


def test_tolerance_library_stream_inside_the_envelope(tmp_path):
    """The tolerance library against the exact one on the same streams, with both halves of section 9.4's synthetic-pair envelope: mean
    EPE <= 3e-2 px and <= 1e-3 of the pixels off by more than 1 px; push == set_images holds inside the library bit for bit.  The stage
    planes (nnf_init*, cost_init*), the oracle chain and the generator-state probe are run for it in
    test_tolerance_stages_gpu.py::test_seeded_context_equals_the_oracle_chain (the tolerance library's test build, the oracle's variant)."""
    res = {}
    for variant in ("", "tol"):
        d = tmp_path / (variant or "exact")
        d.mkdir()
        p = subprocess.run([sys.executable, "-c", TOL_CHILD, variant, str(d)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        res[variant] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in res["tol"]["version"] and "tolerance" not in res[""]["version"]
    for name in ("clip1024", "clip256"):
        assert res["tol"][name] is True and res[""][name] is True, name
        x, t = np.load(tmp_path / "exact" / (name + ".npz")), np.load(tmp_path / "tol" / (name + ".npz"))
        for k in range(3):
            for j in (0, 2):
                epe = float(np.sqrt((x[f"f{k}_{j}"] - t[f"f{k}_{j}"]) ** 2 + (x[f"f{k}_{j + 1}"] - t[f"f{k}_{j + 1}"]) ** 2).mean())
                d = np.sqrt((x[f"f{k}_{j}"] - t[f"f{k}_{j}"]) ** 2 + (x[f"f{k}_{j + 1}"] - t[f"f{k}_{j + 1}"]) ** 2)
                off = float((d > 1.0).mean())
                print(name, "pair", k, "backward" if j else "forward", "EPE", epe, "off by > 1 px", off)
                assert epe <= 3e-2 and off <= 1e-3, (name, k, j, epe, off)          # the synthetic pairs' envelope of section 9.4
