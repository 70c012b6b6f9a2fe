"""GPU tests of the synthetic shutter: the kernels on caller planes, the context forms (single, device, batch), the
call window, the clip driver, the tolerance library and the CLI, all byte for byte against the host form (which test_mblur_cpu.py holds
against the numpy restatement)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from mblur_tol_child import GPU_SIZES, mismatches
from test_mblur_cpu import LIMIT_SIZES, cases, mblur_cases
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
    from eppm_amd import io
    cs = mblur_cases(GPU_SIZES)
    assert {(c["h"], c["w"]) for c in cs} == set(GPU_SIZES)
    for c in cs:
        c["host"] = io.motion_blur_host(c["img"], c["u"], c["v"], *c["params"])
    bad = mismatches(cs, "host")          # every case twice: both runs against the host form, and against each other
    assert not bad, (len(bad), bad[:8])
    assert sum(int((c["host"] != c["img"]).any()) for c in cs) > len(cs) // 2


def test_tolerance_library_equals_the_restatement():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mblur_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for h, w in LIMIT_SIZES])
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """thin frames 8192 long, the widest and tallest eppm_motion_blur_frames accepts: 256 tiles along the long side, movers on every
    border, rows of 32 KiB under input and output pitches larger than 4 * w"""
    mine = [c for c in cases(LIMIT_SIZES) if (c["h"], c["w"]) == LIMIT_SIZES[size]]
    assert len(mine) >= 3
    bad = mismatches(mine)
    assert not bad, bad


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mblur_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context forms ----

def _device_form(e, **kw):
    from eppm_amd._lib import check, lib
    h, w = e.h, e.w
    pitch = (w * 4 + 255) // 256 * 256
    d = C.c_void_p()
    check(lib().eppm_malloc_device(C.byref(d), C.c_size_t(pitch * h)), "malloc")
    try:
        check(lib().eppm_memset_device(d, 0x3c, C.c_size_t(pitch * h)), "memset")
        e.motion_blur_device(d.value, pitch, **kw)
        e.synchronize()
        r = np.empty((h, pitch), np.uint8)
        check(lib().eppm_memcpy_d2h(r.ctypes.data_as(C.c_void_p), d, C.c_size_t(r.nbytes)), "d2h")
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
    want = io.motion_blur_host(a, u, v)
    assert (want != a).any()
    got = e.motion_blur()
    same(got, want, "frame 0 after a forward-only compute")
    same(_device_form(e), want, "device form, frame 0")
    same(e.motion_blur(shutter=1.0, max_radius=31, taps=32), io.motion_blur_host(a, u, v, 1.0, 31, 32), "shutter 1, R 31, taps 32")
    same(e.motion_blur(shutter=0.25, max_radius=1, taps=1), io.motion_blur_host(a, u, v, 0.25, 1, 1), "shutter 0.25, R 1, taps 1")
    # a compute after the blur calls returns the bits it returned before
    u2, v2 = e.compute_flow()
    assert np.array_equal(u2.view(np.uint32), u.view(np.uint32)) and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    r = e.compute_flow_bidirectional()
    assert np.array_equal(r[0].view(np.uint32), u.view(np.uint32)) and np.array_equal(r[1].view(np.uint32), v.view(np.uint32))
    bu, bv = r[2], r[3]
    same(e.motion_blur(frame=0), want, "frame 0 after a bidirectional compute")
    want1 = io.motion_blur_host(b, bu, bv)
    assert (want1 != b).any()
    same(e.motion_blur(frame=1), want1, "frame 1")
    same(_device_form(e, frame=1), want1, "device form, frame 1")
    same(_device_form(e, frame=0), want, "device form, frame 0 again")
    r2 = e.compute_flow_bidirectional()
    for x, y in zip(r, r2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for name, x in (("occ1", r[4]), ("occ2", r[5])):
        assert np.array_equal(e.plane(name, 0), x)
    e.close()


def test_state_errors_and_stage_names(crop):
    import eppm_amd
    from eppm_amd._lib import CMBlurParams, lib
    h, w = 120, 160
    e = eppm_amd.EPPM()
    e.init(h, w)
    out = np.empty((h, w, 3), np.uint8)
    po = out.ctypes.data_as(C.c_void_p)
    call = lambda frame=0, p=None: lib().eppm_motion_blur(e._ctx, p, frame, po, C.c_size_t(w * 3))       # noqa: E731
    assert call() == STATE                                           # before any compute
    e.set_data(crop[0], crop[1])
    assert call() == STATE and call(1) == STATE                      # images, no compute
    e.compute_flow()
    assert call() == 0
    assert call(1) == STATE                                          # frame 1 after a forward-only compute
    assert lib().eppm_motion_blur_device(e._ctx, None, 1, po, C.c_size_t(w * 4)) == STATE
    for bad in ((0.0, 16.0, 8), (1.5, 16.0, 8), (float("nan"), 16.0, 8), (0.5, 0.5, 8), (0.5, 32.0, 8), (0.5, 16.0, 0), (0.5, 16.0, 33)):
        assert call(0, C.byref(CMBlurParams(*bad))) == ARG, bad
    assert call(2) == ARG and call(-1) == ARG
    assert lib().eppm_motion_blur(e._ctx, None, 0, None, C.c_size_t(w * 3)) == ARG
    assert lib().eppm_motion_blur(e._ctx, None, 0, po, C.c_size_t(w * 3 - 1)) == ARG
    assert lib().eppm_motion_blur_device(e._ctx, None, 0, None, C.c_size_t(w * 4)) == ARG
    assert lib().eppm_motion_blur_device(e._ctx, None, 0, po, C.c_size_t(w * 4 - 4)) == ARG
    e.enable_stage_timing(True)
    e.stage_times()
    e.motion_blur()
    names = [n for n, _ in e.stage_times()]
    assert names == ["mblur_pack", "mblur_gather"], names
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
    assert not any(np.array_equal(pairs[i][0], pairs[j][0]) for i in range(3) for j in range(i))
    bat = eppm_amd.EPPMBatch(h, w, 3)
    bat.set_data(pairs)
    flows = bat.compute_flow()
    got = bat.motion_blur(shutter=1.0)
    assert len(got) == 3
    singles = []
    for k, ((a, b), (u, v)) in enumerate(zip(pairs, flows)):
        same(got[k], io.motion_blur_host(a, u, v, 1.0), f"slot {k} against the host form")
        e = eppm_amd.EPPM()
        e.init(a, b, h, w)
        e.compute_flow_bidirectional()
        same(got[k], e.motion_blur(shutter=1.0), f"slot {k} against its own context")
        singles.append(e.motion_blur(shutter=1.0, frame=1))
        e.close()
    assert len({g.tobytes() for g in got}) == 3
    with pytest.raises(eppm_amd.EppmError):
        bat.motion_blur(frame=1)                                     # forward-only
    bat.compute_flow_bidirectional()
    for k, (g, s) in enumerate(zip(bat.motion_blur(shutter=1.0, frame=1), singles)):
        same(g, s, f"slot {k}, frame 1")
    for k, g in enumerate(bat.motion_blur(shutter=1.0)):
        same(g, got[k], f"slot {k}, repeated")
    bat.close()


# ---- 3. the clip driver and the CLI ----

def test_motion_blur_sequence_equals_host_form_on_the_clip_flows():
    import eppm_amd
    from eppm_amd import io
    clip = moving_clip(96, 128, 4, sigma=2.0, bg_v=(3, 1), sq_v=(-4, 3))
    got = eppm_amd.motion_blur_sequence(clip, shutter=1.0, taps=6)
    assert len(got) == 4
    fwd = eppm_amd.flow_sequence(clip)
    bid = eppm_amd.flow_sequence(clip, bidirectional=True)
    for k in range(3):
        assert np.array_equal(fwd[k][0], bid[k][0]) and np.array_equal(fwd[k][1], bid[k][1])
        same(got[k], io.motion_blur_host(clip[k], fwd[k][0], fwd[k][1], 1.0, 16, 6), f"frame {k}")
        assert (got[k] != clip[k]).any()
    same(got[3], io.motion_blur_host(clip[3], bid[2][2], bid[2][3], 1.0, 16, 6), "the last frame, from the last pair's backward flow")
    assert (got[3] != clip[3]).any()


def test_cli_motion_blur(crop, tmp_path):
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
    run = subprocess.run([exe, names[0], names[1], str(tmp_path / "f.flo"), "--motion-blur", "0.5", out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()
    want = e.motion_blur()
    same(io.load_ppm(out), want, "CLI --motion-blur 0.5")
    run = subprocess.run([exe, names[0], names[1], str(tmp_path / "f.flo"), "--motion-blur", "1", out, "--blur-radius", "31", "--blur-taps", "32"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    same(io.load_ppm(out), e.motion_blur(shutter=1.0, max_radius=31, taps=32), "CLI --blur-radius 31 --blur-taps 32")
    e.close()
    for bad in (["--motion-blur", "1.5", out], ["--motion-blur", "0", out], ["--motion-blur", "0.5"], ["--blur-taps", "4"],
                ["--motion-blur", "0.5", out, "--blur-radius", "32"], ["--motion-blur", "0.5", out, "--blur-taps", "33"]):
        assert subprocess.run([exe, names[0], names[1], *bad], capture_output=True, timeout=60).returncode == 2, bad
    # sequence mode: P_mb_0000.ppm .. for every frame, the clip driver's bytes
    prefix = str(tmp_path / "seq")
    run = subprocess.run([exe, "--sequence", names[0], names[1], names[0], "--out-prefix", prefix, "--motion-blur", "0.5", "--blur-taps", "4"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    want = eppm_amd.motion_blur_sequence([a, b, a], shutter=0.5, taps=4)
    for k, wnt in enumerate(want):
        same(io.load_ppm(f"{prefix}_mb_{k:04d}.ppm"), wnt, f"CLI sequence frame {k}")
    assert subprocess.run([exe, "--sequence", names[0], names[1], "--out-prefix", prefix, "--motion-blur", "0.5", out], capture_output=True,
                          timeout=60).returncode == 2
