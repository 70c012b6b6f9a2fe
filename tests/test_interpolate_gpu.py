"""GPU tests of frame interpolation (eppm_interpolate*): the kernels equal the host form byte for byte, the context
forms equal the host form on the bidirectional call's own outputs, batches equal single pairs, the state rules and the memory rules hold,
and the frames mean what they say on a synthetic sequence whose true middle frame is known exactly."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_interpolate_cpu import LIMIT_SIZES, LIMIT_TIMES, interpolation_cases, limit_cases

pytestmark = pytest.mark.gpu

TIMES = (0.0, 1e-7, 0.25, 0.5, 0.7, 1 - 1e-7, 1.0)


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape}{a.dtype} vs {b.shape}{b.dtype}"
    n = int((a != b).reshape(a.shape[0], a.shape[1], -1).any(-1).sum())
    assert n == 0, f"{what}: {n} of {a.shape[0] * a.shape[1]} pixels differ"


def _dev(arr):
    from eppm_amd._lib import check, lib
    p = C.c_void_p()
    check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(max(arr.nbytes, 1))), "malloc")
    check(lib().eppm_memcpy_h2d(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
    return p


def rgba(img, fill=0, pad=0):
    h, w, _ = img.shape
    out = np.full((h, w + pad, 4), fill, np.uint8)
    out[:, :w, :3] = img
    return out


def frames_kernel(img1, img2, u, v, o1, o2, times, pad=0, opad=0):
    """eppm_interpolate_frames (the kernels alone on caller planes) at each time; (h, w, 3) RGB of the RGBA outputs (alpha checked 255).
    pad, opad: pixels beyond every row of the input images and of the output (pitches larger than 4 * w); the output's must stay as it was."""
    from eppm_amd._lib import check, lib
    L = lib()
    h, w = u.shape
    bufs = [_dev(rgba(img1, 7, pad)), _dev(rgba(img2, 9, pad)), _dev(np.ascontiguousarray(np.stack([u, v], -1), np.float32)),
            _dev(np.ascontiguousarray(o1)), _dev(np.ascontiguousarray(o2)), _dev(np.full((h, w + opad, 4), 0x5a, np.uint8))]
    out = []
    try:
        for t in times:
            check(L.eppm_interpolate_frames(bufs[5], C.c_size_t((w + opad) * 4), bufs[0], bufs[1], C.c_size_t((w + pad) * 4), bufs[2], bufs[3], bufs[4],
                                            h, w, C.c_float(t)), "eppm_interpolate_frames")
            r = np.empty((h, w + opad, 4), np.uint8)
            check(L.eppm_memcpy_d2h(r.ctypes.data_as(C.c_void_p), bufs[5], C.c_size_t(r.nbytes)), "d2h")
            assert (r[:, :w, 3] == 255).all() and (r[:, w:] == 0x5a).all()
            out.append(r[:, :w, :3].copy())
    finally:
        for p in bufs:
            L.eppm_free_device(p)
    return out


def _check_kernel_cases(cases, times=TIMES):
    from eppm_amd import io
    for name, a, b, u, v, o1, o2 in cases:
        for t, got in zip(times, frames_kernel(a, b, u, v, o1, o2, times)):
            same(got, io.interpolate(a, b, u, v, o1, o2, t), f"{name} t={t}")


def test_kernels_equal_host_form_on_the_cpu_cases():
    _check_kernel_cases(interpolation_cases())


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_host_form_at_the_size_limit(size):
    """thin frames 8192 long: splats at coordinate 8191, vectors that leave the frame by a fraction of a pixel at both ends, fill walks
    along the whole long side, the images and the output under pitches larger than 4 * w"""
    from eppm_amd import io
    for k, (name, a, b, u, v, o1, o2) in enumerate(limit_cases(size)):
        got = frames_kernel(a, b, u, v, o1, o2, LIMIT_TIMES, pad=(3, 64, 0, 5)[k], opad=(64, 0, 3, 1)[k])
        for t, g in zip(LIMIT_TIMES, got):
            same(g, io.interpolate(a, b, u, v, o1, o2, t), f"{name} t={t}")


TOL_LIMIT_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import conftest          # (selects the test library: overridden below, before anything is loaded)
import eppm_amd
eppm_amd.select_library("tol")
from test_interpolate_cpu import LIMIT_TIMES, interpolate_np, limit_cases
from test_interpolate_gpu import frames_kernel
print(eppm_amd.lib().eppm_version().decode())
bad = []
for name, a, b, u, v, o1, o2 in limit_cases(int(sys.argv[1])):
    for t, g in zip(LIMIT_TIMES, frames_kernel(a, b, u, v, o1, o2, LIMIT_TIMES, pad=3, opad=5)):
        n = int((g != interpolate_np(a, b, u, v, o1, o2, t)).any(-1).sum())
        if n:
            bad.append((name, t, n))
print(len(bad), "differ from the restatement:", bad[:5])
assert not bad
print("PART OK")
""" % os.path.join(ROOT, "tests")


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_tolerance_library_at_the_size_limit(size):
    out = subprocess.run([sys.executable, "-c", TOL_LIMIT_CHILD, str(size)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def _bidir(a, b):
    import eppm_amd
    h, w, _ = a.shape
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    out = e.compute_flow_bidirectional()
    return e, out


def test_kernels_equal_host_form_on_engine_flows(frames):
    from eppm_amd import synth
    e, (u, v, bu, bv, o1, o2) = _bidir(frames[0], frames[1])
    e.close()
    _check_kernel_cases([("bundled", frames[0], frames[1], u, v, o1, o2)], (0.25, 0.5, 0.7))
    a, b, _, _ = synth.make_pair_cached(436, 1024, seed=5)
    e, (u, v, bu, bv, o1, o2) = _bidir(a, b)
    e.close()
    _check_kernel_cases([("synthetic_1024x436", a, b, u, v, o1, o2)], (0.5, 1 - 1e-7))


def test_context_forms_equal_host_form(frames):
    from eppm_amd import io
    from eppm_amd._lib import check, lib
    a, b = frames
    h, w, _ = a.shape
    e, (u, v, bu, bv, o1, o2) = _bidir(a, b)
    times = [0.5, 0.0, 0.25, 1.0, 0.7, 1e-7]          # more than one chunk of four
    got = e.interpolate(times)
    for t, g in zip(times, got):
        same(g, io.interpolate(a, b, u, v, o1, o2, t), f"eppm_interpolate t={t}")
    # three repeated calls are identical (the atomic minimum does not depend on the order the keys arrive in)
    for _ in range(3):
        for g0, g in zip(got, e.interpolate(times)):
            same(g, g0, "repeated call")
    # the device form, pitched planes
    pitch = (w * 4 + 255) // 256 * 256
    d = [C.c_void_p() for _ in times]
    for p in d:
        check(lib().eppm_malloc_device(C.byref(p), C.c_size_t(pitch * h)), "malloc")
    e.interpolate_device(times, [p.value for p in d], pitch)
    e.synchronize()
    for t, p, g in zip(times, d, got):
        r = np.empty((h, pitch), np.uint8)
        check(lib().eppm_memcpy_d2h(r.ctypes.data_as(C.c_void_p), p, C.c_size_t(r.nbytes)), "d2h")
        lib().eppm_free_device(p)
        r = r[:, :w * 4].reshape(h, w, 4)
        assert (r[..., 3] == 255).all()
        same(r[..., :3], g, f"device form t={t}")
    # the bidirectional outputs are unchanged by the interpolation calls
    u2, v2, bu2, bv2 = e.plane("flow", 0), e.plane("flow_bwd", 0), e.plane("occ1", 0), e.plane("occ2", 0)
    assert np.array_equal(u2["x"], u) and np.array_equal(u2["y"], v)
    assert np.array_equal(v2["x"], bu) and np.array_equal(v2["y"], bv)
    assert np.array_equal(bu2, o1) and np.array_equal(bv2, o2)
    e.close()


def test_batch_equals_single_pairs():
    import eppm_amd
    from eppm_amd import synth
    h, w = 120, 176
    pairs = []
    for k in range(3):
        a, b, _, _ = synth.make_pair(h, w, seed=300 + k, max_flow=4.0 + 4 * k)
        pairs.append((a, b))
    times = [0.25, 0.5, 0.8]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    bat.set_data(pairs)
    bat.compute_flow_bidirectional()
    got = bat.interpolate(times)
    assert len(got) == 3 and all(len(g) == 3 for g in got)
    for k, (a, b) in enumerate(pairs):
        e, _ = _bidir(a, b)
        for t, x, y in zip(times, got[k], e.interpolate(times)):
            same(x, y, f"pair {k} t={t}")
        e.close()
    bat.close()


def test_batch_equals_host_form_across_chunks():
    """blockIdx.z = pair * nt + k: k_interp_splat / k_interp_blend take the pair as z / nt, the fill passes the time as z % nt.  Three
    different pairs, six times in two chunks (four, then two), the endpoints at k == 1 and k == 3 of the first: every frame of every slot
    against the host form on that slot's own outputs, not against another context."""
    import eppm_amd
    from eppm_amd import io, synth
    h, w = 45, 67
    pairs = [synth.make_pair(h, w, seed=310 + k, max_flow=2.0 + 2 * k)[:2] for k in range(3)]
    assert not any(np.array_equal(pairs[i][0], pairs[j][0]) for i in range(3) for j in range(i))
    times = [0.5, 0.0, 0.25, 1.0, 0.7, 1e-7]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    bat.set_data(pairs)
    outs = bat.compute_flow_bidirectional()
    got = bat.interpolate(times)
    assert len(got) == 3 and all(len(g) == len(times) for g in got)
    for k, ((a, b), (u, v, bu, bv, o1, o2)) in enumerate(zip(pairs, outs)):
        for t, g in zip(times, got[k]):
            same(g, io.interpolate(a, b, u, v, o1, o2, t), f"slot {k} t={t}")
    for k, (g0, g1) in enumerate(zip(got, bat.interpolate(times))):
        for t, x, y in zip(times, g0, g1):
            same(y, x, f"repeated call: slot {k} t={t}")
    bat.close()


def test_state_errors_and_stage_names(crop):
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = 120, 160
    e = eppm_amd.EPPM()
    e.init(h, w)
    out = np.empty((h, w, 3), np.uint8)
    ts = (C.c_float * 1)(0.5)
    ptr = (C.c_void_p * 1)(out.ctypes.data)
    call = lambda: lib().eppm_interpolate(e._ctx, 1, ts, ptr, C.c_size_t(w * 3))       # noqa: E731
    assert call() == 3                                           # before any compute
    e.set_data(crop[0], crop[1])
    assert call() == 3
    e.compute_flow()
    assert call() == 3                                           # forward only
    e.compute_flow_bidirectional()
    assert call() == 0
    for bad in (0.0 - 0.1, 1.5, float("nan")):
        assert lib().eppm_interpolate(e._ctx, 1, (C.c_float * 1)(bad), ptr, C.c_size_t(w * 3)) == 1
    assert lib().eppm_interpolate(e._ctx, 0, ts, ptr, C.c_size_t(w * 3)) == 1
    assert lib().eppm_interpolate(e._ctx, 1, ts, None, C.c_size_t(w * 3)) == 1
    assert lib().eppm_interpolate(e._ctx, 1, ts, ptr, C.c_size_t(w * 3 - 1)) == 1
    assert lib().eppm_interpolate_device(e._ctx, 1, ts, (C.c_void_p * 1)(None), C.c_size_t(w * 4)) == 1
    e.enable_stage_timing(True)
    e.interpolate([0.5])
    names = [n for n, _ in e.stage_times()]
    for n in ("interp_splat", "interp_fill", "interp_blend"):
        assert n in names, names
    e.compute_flow_bidirectional()
    assert not [n for n, _ in e.stage_times() if n.startswith("interp")]
    e.set_data(crop[1], crop[0])
    assert call() == 3                                           # new images
    e.compute_flow_bidirectional()
    assert call() == 0
    e.compute_flow()
    assert call() == 3                                           # a forward-only compute ends the window
    e.close()


def _free_bytes():
    from eppm_amd._lib import check, lib
    f, t = C.c_size_t(), C.c_size_t()
    check(lib().eppm_device_synchronize(), "sync")
    check(lib().eppm_device_mem_info(C.byref(f), C.byref(t)), "mem_info")
    return f.value


def test_memory_grows_once_and_is_returned():
    import eppm_amd
    from eppm_amd import synth
    from eppm_amd._lib import check, lib
    h, w = 720, 1280
    a, b, _, _ = synth.make_pair_cached(h, w, seed=3, max_flow=8.0)
    e = eppm_amd.EPPM(); e.init(a, b, h, w); e.compute_flow_bidirectional(); e.interpolate([0.5]); e.close()     # code objects, pools
    check(lib().eppm_release_cached_memory(), "release")
    level = _free_bytes()
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow()
    e.compute_flow_bidirectional()
    bidir = _free_bytes()
    e.compute_flow_bidirectional()
    e.compute_flow()
    e.compute_flow_bidirectional()
    assert abs(bidir - _free_bytes()) < 2 << 20, (bidir, _free_bytes())       # forward and bidirectional calls alone allocate nothing new
    e.interpolate([0.5])
    grown = bidir - _free_bytes()
    assert h * w * 16 <= grown <= h * w * 4 * 19 + (8 << 20), grown            # the interpolation scratch: once
    first = _free_bytes()
    e.interpolate([0.25])
    e.interpolate([0.1 * k for k in range(1, 10)])                             # nt 9: three chunks, no growth
    e.compute_flow_bidirectional()
    e.interpolate([0.5, 0.6])
    assert abs(first - _free_bytes()) < 2 << 20, (first, _free_bytes())
    e.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert abs(_free_bytes() - level) < 8 << 20, (level, _free_bytes())        # eppm_destroy returned it


# ---------------------------------------------------------------------------------------------------
# meaning: a synthetic sequence whose middle frame is known exactly
# ---------------------------------------------------------------------------------------------------
BG_V = (4, 2)          # background motion per unit time (x, y)
SQ_V = (-8, 6)         # the square's
SQ = 48                # side of the square


def _noise(rng, h, w, cutoff):
    """Band-limited noise: white noise with the frequencies above `cutoff` cycles/px removed, scaled to 16..239 per channel."""
    out = np.empty((h, w, 3), np.uint8)
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.fftfreq(w)[None, :]
    keep = np.sqrt(fx ** 2 + fy ** 2) <= cutoff
    for c in range(3):
        x = np.real(np.fft.ifft2(np.fft.fft2(rng.normal(size=(h, w))) * keep))
        x = (x - x.min()) / (x.max() - x.min())
        out[..., c] = np.round(16 + 223 * x).astype(np.uint8)
    return out


def sequence(h=160, w=224, seed=41):
    """Frames at t = 0, 0.5, 1, the true forward / backward flows of frames 0 -> 1, and the square's masks at the three times.  Every
    displacement at t = 0.5 is an integer, so the middle frame is exact."""
    rng = np.random.default_rng(seed)
    m = 16
    bg = _noise(rng, h + 2 * m, w + 2 * m, 0.12)
    sq = _noise(rng, SQ, SQ, 0.2)
    x0, y0 = w // 2 + 10, h // 4
    out, lab = [], []
    for t in (0.0, 0.5, 1.0):
        bx, by = int(BG_V[0] * t), int(BG_V[1] * t)
        f = bg[m - by:m - by + h, m - bx:m - bx + w].copy()
        sx, sy = x0 + int(SQ_V[0] * t), y0 + int(SQ_V[1] * t)
        f[sy:sy + SQ, sx:sx + SQ] = sq
        L = np.zeros((h, w), bool)
        L[sy:sy + SQ, sx:sx + SQ] = True
        out.append(f)
        lab.append(L)
    u = np.where(lab[0], SQ_V[0], BG_V[0]).astype(np.float32)
    v = np.where(lab[0], SQ_V[1], BG_V[1]).astype(np.float32)
    bu = np.where(lab[2], -SQ_V[0], -BG_V[0]).astype(np.float32)
    bv = np.where(lab[2], -SQ_V[1], -BG_V[1]).astype(np.float32)
    return out, (u, v, bu, bv), lab


def interior(lab, border=8, r=2):
    """Middle-frame pixels more than r px from a motion boundary along their whole trajectory (the label is constant on the
    (2r+1)^2 window around the pixel in the middle frame, and around where it comes from / goes to in frames 0 and 1) and more than
    `border` px from the frame's edge."""
    h, w = lab[1].shape

    def pure(L, val, dx, dy):
        ok = np.ones((h, w), bool)
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                ys = np.clip(np.arange(h)[:, None] + dy + j, 0, h - 1)
                xs = np.clip(np.arange(w)[None, :] + dx + i, 0, w - 1)
                ok &= L[ys, xs] == val
        return ok
    half = lambda V: (V[0] // 2, V[1] // 2)       # noqa: E731
    bgx, bgy = half(BG_V)
    sqx, sqy = half(SQ_V)
    bg_ok = pure(lab[1], False, 0, 0) & pure(lab[0], False, -bgx, -bgy) & pure(lab[2], False, bgx, bgy)
    sq_ok = pure(lab[1], True, 0, 0) & pure(lab[0], True, -sqx, -sqy) & pure(lab[2], True, sqx, sqy)
    ok = bg_ok | sq_ok
    ok[:border] = ok[-border:] = False
    ok[:, :border] = ok[:, -border:] = False
    return ok


def test_meaning_exact_on_true_flow():
    from eppm_amd import io
    (f0, fm, f1), (u, v, bu, bv), lab = sequence()
    o1 = io.fb_occlusion(u, v, bu, bv)
    o2 = io.fb_occlusion(bu, bv, u, v)
    got = frames_kernel(f0, f1, u, v, o1, o2, [0.5])[0]
    same(got, io.interpolate(f0, f1, u, v, o1, o2, 0.5), "kernel == host form")
    ok = interior(lab)
    assert ok.sum() > 0.5 * ok.size
    bad = int(((got != fm).any(-1) & ok).sum())
    assert bad == 0, f"{bad} of {int(ok.sum())} interior pixels differ from the true middle frame"


# Measured on the CPU before the kernels existed (the oracle's forward flow, the oracle_backward chain of tests/test_bidirectional_gpu.py,
# the masks of io.fb_occlusion on those flows and eppm_interpolate_host): MAE 3.4763 grey levels against the true middle frame, 16 px border
# excluded; the naive blend 0.5 * I1 + 0.5 * I2 scores 12.3176 (ratio 0.28), the true flow 0.3156.  The engine's flows are the oracle's bit
# for bit, so the GPU value is the same; the bound keeps a 10 % margin.
MAE_BOUND = 3.82


def _mae(a, b, border=16):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))[border:-border, border:-border]
    return float(d.mean())


def test_meaning_end_to_end():
    import eppm_amd
    (f0, fm, f1), _, _ = sequence()
    h, w, _ = f0.shape
    e = eppm_amd.EPPM()
    e.init(f0, f1, h, w)
    e.compute_flow_bidirectional()
    mid = e.interpolate([0.5])[0]
    e.close()
    naive = np.floor((f0.astype(np.float32) + f1.astype(np.float32)) * np.float32(0.5) + np.float32(0.5)).astype(np.uint8)
    mae, mae_naive = _mae(mid, fm), _mae(naive, fm)
    assert mae <= 0.5 * mae_naive, (mae, mae_naive)
    assert mae <= MAE_BOUND, (mae, MAE_BOUND)


TOL_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
from conftest import read_ppm, GOLDEN          # (selects the test library: overridden below, before anything is loaded)
import eppm_amd
eppm_amd.select_library("tol")
from eppm_amd import io
a, b = read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm"))
h, w, _ = a.shape
e = eppm_amd.EPPM(); e.init(a, b, h, w)
u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
times = [0.25, 0.5]
got = e.interpolate(times)
e.close()
out = {"version": eppm_amd.lib().eppm_version().decode(),
       "same": all(bool(np.array_equal(g, io.interpolate(a, b, u, v, o1, o2, t))) for t, g in zip(times, got))}
print(json.dumps(out))
""" % os.path.join(ROOT, "tests")


def test_tolerance_library_interpolates_its_own_flows():
    p = subprocess.run([sys.executable, "-c", TOL_CHILD], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in res["version"]
    assert res["same"] is True


def test_cli_interpolate(frames, tmp_path):
    import eppm_amd
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    f1, f2 = os.path.join(GOLDEN, "frame10.ppm"), os.path.join(GOLDEN, "frame11.ppm")
    mid, q = str(tmp_path / "mid.ppm"), str(tmp_path / "q.ppm")
    subprocess.run([exe, f1, f2, str(tmp_path / "out.flo"), "--interpolate", "0.5", mid, "--interpolate", "0.25", q], check=True,
                   capture_output=True, timeout=300)
    e = eppm_amd.EPPM()
    e.init(frames[0], frames[1], 480, 640)
    e.compute_flow_bidirectional()
    want = e.interpolate([0.5, 0.25])
    e.close()
    head = b"P6\n640 480\n255\n"
    for path, wnt in ((mid, want[0]), (q, want[1])):
        data = open(path, "rb").read()
        assert data.startswith(head) and len(data) == len(head) + 640 * 480 * 3
        same(np.frombuffer(data[len(head):], np.uint8).reshape(480, 640, 3), wnt, f"CLI {os.path.basename(path)}")
    assert subprocess.run([exe, f1, f2, "--interpolate", "1.5", mid], capture_output=True, timeout=60).returncode == 2
