"""GPU tests of rolling-shutter correction: the kernels on caller planes, the context forms (single, device, batch),
the call window, the clip drivers, the tolerance library and the CLI, all byte for byte against the host form (which test_rshutter_cpu.py
holds against the numpy restatement), and what the correction reaches on the engine's own flows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rshutter_tol_child import mismatches
from test_rshutter_cpu import LIMIT_SIZES, SIZES, mae, rs_cases, scene, shutter_frame
from test_stabilize_cpu import moving_clip

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape}{a.dtype} vs {b.shape}{b.dtype}"
    n = int((a != b).reshape(a.shape[0], a.shape[1], -1).any(-1).sum())
    assert n == 0, f"{what}: {n} of {a.shape[0] * a.shape[1]} pixels differ"


# ---- 1. the kernels alone on caller planes ----

def test_kernels_equal_host_form_on_the_cpu_cases():
    cs = rs_cases(SIZES)
    assert {(c["h"], c["w"]) for c in cs} == set(SIZES)
    bad = mismatches(cs)          # every case twice: both runs against the host form, and against each other
    assert not bad, (len(bad), bad[:8])
    assert 2 * sum(int((c["host"] != c["img"]).any()) for c in cs) >= len(cs)


def test_tolerance_library_equals_the_host_form():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rshutter_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for h, w in LIMIT_SIZES])
def test_kernels_equal_the_host_form_at_the_size_limit(size):
    """thin frames 8192 long, the widest and tallest eppm_rolling_shutter_frames accepts, read along both axes: coordinates up to 8191,
    rows of 32 KiB under input and output pitches larger than 4 * w"""
    mine = [c for c in rs_cases(LIMIT_SIZES) if (c["h"], c["w"]) == LIMIT_SIZES[size]]
    assert {c["params"][3] for c in mine} == {0, 1}
    bad = mismatches(mine)
    assert not bad, bad
    assert all((c["host"] != c["img"]).any() for c in mine)


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rshutter_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context forms ----

def _device_form(e, **kw):
    from eppm_amd._lib import check, lib
    h, w = e.h, e.w
    pitch = (w * 4 + 255) // 256 * 256
    d = C.c_void_p()
    check(lib().eppm_malloc_device(C.byref(d), pitch * h), "malloc")
    try:
        check(lib().eppm_memset_device(d, 0x3c, pitch * h), "memset")
        e.rolling_shutter_device(d.value, pitch, **kw)
        e.synchronize()
        r = np.empty((h, pitch), np.uint8)
        check(lib().eppm_memcpy_d2h(r.ctypes.data, d, r.nbytes), "d2h")
    finally:
        lib().eppm_free_device(d)
    assert (r[:, w * 4:] == 0x3c).all()
    r = r[:, :w * 4].reshape(h, w, 4)
    assert (r[..., 3] == 255).all()
    return r[..., :3]


def test_context_forms_equal_host_form(crop):
    import eppm_amd
    from eppm_amd import io
    a, b = crop
    h, w, _ = a.shape
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    u, v = e.compute_flow()
    want = io.rolling_shutter_host(a, u, v, 0, readout=1.0)
    assert (want != a).any()
    same(e.rolling_shutter(readout=1.0), want, "frame 0 after a forward-only compute")
    same(_device_form(e, readout=1.0), want, "device form, frame 0")
    same(e.rolling_shutter(), io.rolling_shutter_host(a, u, v), "the defaults")
    same(e.rolling_shutter(readout=-1.0, anchor=1.0, iters=8, axis=1), io.rolling_shutter_host(a, u, v, 0, -1.0, 1.0, 8, 1), "columns, last first, 8 steps")
    same(e.rolling_shutter(readout=0.75, anchor=0.0, iters=1), io.rolling_shutter_host(a, u, v, 0, 0.75, 0.0, 1, 0), "one step")
    same(e.rolling_shutter(readout=0.0), a, "readout 0")
    # a compute after the calls returns the bits it returned before
    u2, v2 = e.compute_flow()
    assert np.array_equal(u2.view(np.uint32), u.view(np.uint32)) and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    r = e.compute_flow_bidirectional()
    assert np.array_equal(r[0].view(np.uint32), u.view(np.uint32)) and np.array_equal(r[1].view(np.uint32), v.view(np.uint32))
    bu, bv = r[2], r[3]
    same(e.rolling_shutter(readout=1.0, frame=0), want, "frame 0 after a bidirectional compute")
    want1 = io.rolling_shutter_host(b, bu, bv, 1, readout=1.0)
    assert (want1 != b).any()
    same(e.rolling_shutter(readout=1.0, frame=1), want1, "frame 1")
    same(_device_form(e, readout=1.0, frame=1), want1, "device form, frame 1")
    same(_device_form(e, readout=1.0, frame=0), want, "device form, frame 0 again")
    same(e.rolling_shutter(readout=0.5, axis=1, frame=1), io.rolling_shutter_host(b, bu, bv, 1, axis=1), "frame 1, columns")
    r2 = e.compute_flow_bidirectional()
    for x, y in zip(r, r2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for name, x in (("occ1", r[4]), ("occ2", r[5])):
        assert np.array_equal(e.plane(name, 0), x)
    e.close()


def test_state_errors_and_stage_names(crop):
    import eppm_amd
    from eppm_amd._lib import CRSParams, lib
    h, w = 120, 160
    e = eppm_amd.EPPM()
    e.init(h, w)
    out = np.empty((h, w, 3), np.uint8)
    po = out.ctypes.data
    call = lambda frame=0, p=None: lib().eppm_rolling_shutter(e._ctx, p, frame, po, w * 3)       # noqa: E731
    assert call() == STATE                                           # before any compute
    e.set_data(crop[0], crop[1])
    assert call() == STATE and call(1) == STATE                      # images, no compute
    e.compute_flow()
    assert call() == 0
    assert call(1) == STATE                                          # frame 1 after a forward-only compute
    assert lib().eppm_rolling_shutter_device(e._ctx, None, 1, po, w * 4) == STATE
    nan = float("nan")
    for bad in ((1.5, 0.5, 3, 0), (-1.5, 0.5, 3, 0), (nan, 0.5, 3, 0), (0.5, -0.1, 3, 0), (0.5, 1.1, 3, 0), (0.5, nan, 3, 0), (0.5, 0.5, 0, 0),
                (0.5, 0.5, 9, 0), (0.5, 0.5, 3, 2), (0.5, 0.5, 3, -1)):
        assert call(0, C.byref(CRSParams(*bad))) == ARG, bad
    assert call(2) == ARG and call(-1) == ARG
    assert lib().eppm_rolling_shutter(e._ctx, None, 0, None, w * 3) == ARG
    assert lib().eppm_rolling_shutter(e._ctx, None, 0, po, w * 3 - 1) == ARG
    assert lib().eppm_rolling_shutter_device(e._ctx, None, 0, None, w * 4) == ARG
    assert lib().eppm_rolling_shutter_device(e._ctx, None, 0, po, w * 4 - 4) == ARG
    e.enable_stage_timing(True)
    e.stage_times()
    e.rolling_shutter()
    names = [n for n, _ in e.stage_times()]
    assert names == ["rs_velocity", "rs_gather"], names
    e.enable_stage_timing(False)
    e.push_frame(crop[0])
    assert call() == STATE and call(1) == STATE                      # after a push
    e.compute_flow_bidirectional()
    assert call() == 0 and call(1) == 0
    e.compute_flow()
    assert call() == 0 and call(1) == STATE                          # a forward-only compute ends frame 1's window
    e.set_data(crop[1], crop[0])
    assert call() == STATE
    e.compute_flow_begin()
    assert call() == STATE                                           # a compute is pending
    e.compute_flow_end()
    assert call() == 0
    e.close()


def test_batch_gives_each_pair_its_single_context_result():
    import eppm_amd
    from eppm_amd import io, synth
    h, w = 45, 67
    pairs = [synth.make_pair(h, w, seed=320 + k, max_flow=3.0 + 3 * k)[:2] for k in range(3)]
    kw = dict(readout=1.0, anchor=0.25)
    bat = eppm_amd.EPPMBatch(h, w, 3)
    bat.set_data(pairs)
    flows = bat.compute_flow()
    got = bat.rolling_shutter(**kw)
    assert len(got) == 3
    singles = []
    for k, ((a, b), (u, v)) in enumerate(zip(pairs, flows)):
        same(got[k], io.rolling_shutter_host(a, u, v, 0, **kw), f"slot {k} against the host form")
        assert (got[k] != a).any()
        e = eppm_amd.EPPM()
        e.init(a, b, h, w)
        e.compute_flow_bidirectional()
        same(got[k], e.rolling_shutter(**kw), f"slot {k} against its own context")
        singles.append(e.rolling_shutter(frame=1, **kw))
        e.close()
    assert len({g.tobytes() for g in got}) == 3
    with pytest.raises(eppm_amd.EppmError):
        bat.rolling_shutter(frame=1)                                 # forward-only
    bat.compute_flow_bidirectional()
    for k, (g, s) in enumerate(zip(bat.rolling_shutter(frame=1, **kw), singles)):
        same(g, s, f"slot {k}, frame 1")
    for k, g in enumerate(bat.rolling_shutter(**kw)):
        same(g, got[k], f"slot {k}, repeated")
    bat.close()


# ---- 3. the clip drivers and the CLI ----

def test_rolling_shutter_sequence_equals_host_form_on_the_clip_flows():
    import eppm_amd
    from eppm_amd import io
    clip = moving_clip(96, 128, 4, sigma=2.0, bg_v=(3, 1), sq_v=(-4, 3))
    kw = dict(readout=1.0, anchor=0.0)
    got = eppm_amd.rolling_shutter_sequence(clip, **kw)
    assert len(got) == 4
    fwd = eppm_amd.flow_sequence(clip)
    bid = eppm_amd.flow_sequence(clip, bidirectional=True)
    for k in range(3):
        assert np.array_equal(fwd[k][0], bid[k][0]) and np.array_equal(fwd[k][1], bid[k][1])
        same(got[k], io.rolling_shutter_host(clip[k], fwd[k][0], fwd[k][1], 0, **kw), f"frame {k}")
        assert (got[k] != clip[k]).any()
    same(got[3], io.rolling_shutter_host(clip[3], bid[2][2], bid[2][3], 1, **kw), "the last frame, from the last pair's backward flow")
    assert (got[3] != clip[3]).any()
    with pytest.raises(TypeError):
        eppm_amd.rolling_shutter_sequence(clip, lost_permille=3)
    with pytest.raises(TypeError):
        eppm_amd.rolling_shutter_sequence(clip, auto_cut=True, nonsense=3)


def _film():
    return moving_clip(96, 128, 4, seed=31), moving_clip(96, 128, 3, seed=32)


def test_rolling_shutter_sequence_with_auto_cut_warps_no_frame_across_the_cut():
    """two shots of 4 and 3 frames: pair 3 crosses the cut.  Frame 3 comes from pair 2's backward flow, frame 4 from pair 4's forward flow"""
    import eppm_amd
    from eppm_amd import io
    a, b = _film()
    clip = a + b
    kw = dict(readout=1.0, anchor=0.5)
    flows, cuts = eppm_amd.flow_sequence(clip, bidirectional=True, auto_cut=True)
    assert cuts == [k == 3 for k in range(6)], cuts
    got = eppm_amd.rolling_shutter_sequence(clip, auto_cut=True, **kw)
    assert len(got) == 7
    want, fallback = [None] * 7, clip[0]
    for k in range(1, 7):
        u, v, bu, bv = flows[k - 1][:4]
        want[k - 1] = fallback if cuts[k - 1] else io.rolling_shutter_host(clip[k - 1], u, v, 0, **kw)
        fallback = clip[k] if cuts[k - 1] else io.rolling_shutter_host(clip[k], bu, bv, 1, **kw)
    want[6] = fallback
    for k in range(7):
        same(got[k], want[k], f"frame {k}")
        assert (got[k] != clip[k]).any(), k
    same(got[3], io.rolling_shutter_host(clip[3], flows[2][2], flows[2][3], 1, **kw), "the last frame of the first shot")
    # a cut at every pair (lost_permille 0): every frame is a one-frame shot and comes back unchanged
    every = eppm_amd.rolling_shutter_sequence(clip[:3], auto_cut=True, lost_permille=0, **kw)
    for k in range(3):
        same(every[k], clip[k], f"one-frame shot {k}")


def test_rolling_shutter_sequences_equal_the_single_clip_driver():
    import eppm_amd
    a, b = _film()
    clips = [a, b, a[1:3]]
    kw = dict(readout=-0.75, anchor=1.0, axis=1)
    got = eppm_amd.rolling_shutter_sequences(clips, slots=2, **kw)
    assert [len(g) for g in got] == [4, 3, 2]
    for c, clip in enumerate(clips):
        want = eppm_amd.rolling_shutter_sequence(clip, **kw)
        for k, (g, w_) in enumerate(zip(got[c], want)):
            same(g, w_, f"clip {c} frame {k}")


def test_cli_rolling_shutter(crop, tmp_path):
    import eppm_amd
    from eppm_amd import io
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    a, b = crop
    h, w, _ = a.shape
    names = []
    for k, f in enumerate((a, b)):
        names.append(str(tmp_path / f"f{k}.ppm"))
        with open(names[-1], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h) + f.tobytes())
    out = str(tmp_path / "out.ppm")
    run = subprocess.run([exe, names[0], names[1], str(tmp_path / "f.flo"), "--rolling-shutter", "1", out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()
    same(io.load_ppm(out), e.rolling_shutter(readout=1.0), "CLI --rolling-shutter 1")
    run = subprocess.run([exe, names[0], names[1], str(tmp_path / "f.flo"), "--rolling-shutter", "-0.75", out, "--rs-anchor", "0.25", "--rs-iters", "8",
                          "--rs-columns"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    same(io.load_ppm(out), e.rolling_shutter(readout=-0.75, anchor=0.25, iters=8, axis=1), "CLI --rs-anchor 0.25 --rs-iters 8 --rs-columns")
    e.close()
    for bad in (["--rolling-shutter", "1.5", out], ["--rolling-shutter", "-1.5", out], ["--rolling-shutter", "0.5"], ["--rs-iters", "4"], ["--rs-columns"],
                ["--rolling-shutter", "0.5", out, "--rs-anchor", "1.5"], ["--rolling-shutter", "0.5", out, "--rs-iters", "9"],
                ["--rolling-shutter", "0.5", out, "--rs-iters", "0"], ["--rolling-shutter", "x", out],
                ["--rolling-shutter", "0.5", out, "--motion-blur", "0.5", out]):
        assert subprocess.run([exe, names[0], names[1], *bad], capture_output=True, timeout=60).returncode == 2, bad
    # sequence mode: P_rs_0000.ppm .. for every frame, the clip driver's bytes
    prefix = str(tmp_path / "seq")
    run = subprocess.run([exe, "--sequence", names[0], names[1], names[0], "--out-prefix", prefix, "--rolling-shutter", "0.75", "--rs-anchor", "0"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    want = eppm_amd.rolling_shutter_sequence([a, b, a], readout=0.75, anchor=0.0)
    for k, wnt in enumerate(want):
        same(io.load_ppm(f"{prefix}_rs_{k:04d}.ppm"), wnt, f"CLI sequence frame {k}")
    seq = [exe, "--sequence", names[0], names[1], "--out-prefix", prefix]
    for bad in (["--rolling-shutter", "0.5", out], ["--rolling-shutter", "0.5", "--auto-cut"], ["--rolling-shutter", "0.5", "--deinterlace"],
                ["--rolling-shutter", "0.5", "--denoise"], ["--rolling-shutter", "0.5", "--motion-blur", "0.5"], ["--rs-iters", "3"]):
        assert subprocess.run([*seq, *bad], capture_output=True, timeout=60).returncode == 2, bad


# ---- 4. meaning on the engine's own flows ----

def test_correction_on_the_engines_flows_brings_every_frame_towards_the_global_shutter():
    """A four-frame rolling-shutter clip of the CPU file's generator, 96 x 128, motion (6, -5), readout 0.75, anchor 0.5, corrected with the
    flows the engine finds on it.  MAE against the global-shutter frames, 16-pixel border left out; measured (uncorrected -> corrected,
    DESIGN.md section 27.4): 5.04 -> 0.34, 5.11 -> 0.34, 5.18 -> 0.34, 5.00 -> 0.32."""
    import eppm_amd
    h, w, m, r = 96, 128, (6.0, -5.0), 0.75
    S = scene(3)
    rs = [shutter_frame(S, h, w, k, m, r, 0.5) for k in range(4)]
    gs = [shutter_frame(S, h, w, k, m) for k in range(4)]
    got = eppm_amd.rolling_shutter_sequence(rs, readout=r)
    for k in range(4):
        before, after = mae(rs[k], gs[k], 16), mae(got[k], gs[k], 16)
        print(f"frame {k}: MAE {before:.3f} -> {after:.3f}")
        assert after < before, (k, before, after)
