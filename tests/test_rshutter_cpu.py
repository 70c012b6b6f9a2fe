"""CPU tests of rolling-shutter correction (include/eppm_rshutter.h): the binding table against the header, the host
form's argument checks, the host form against a numpy restatement of the section bit for bit on rs_cases() (shared with the GPU tests),
identities, the exact recovery of a horizontal translation, what the correction reaches on rolling-shutter clips with true flows, and the
host code under sanitizers.  The clip generators (a periodic band-limited scene sampled at k + tau) live here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eppm_amd
from eppm_amd import _lib, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # (no conftest import: rshutter_tol_child.py imports this module)
F = np.float32
ARG = 1
NAMES = ["eppm_rs_default_params", "eppm_rolling_shutter", "eppm_rolling_shutter_device", "eppm_batch_rolling_shutter",
         "eppm_rolling_shutter_frames", "eppm_rolling_shutter_host"]


# ---- numpy restatement of DESIGN.md section 27.1 (written from the text, not from rshutter.h) ----

def np_bilinear(planes, qx, qy):
    """the float32 planes sampled bilinearly at (qx, qy): clamp into the frame, taps (x0, x1 = min(x0 + 1, w - 1)), weights
    by*(bx*v00 + ax*v01) + ay*(bx*v10 + ax*v11), one rounding per operation"""
    h, w = planes[0].shape
    qx = np.fmin(np.fmax(qx, F(0)), F(w - 1))
    qy = np.fmin(np.fmax(qy, F(0)), F(h - 1))
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = qx - x0.astype(F), qy - y0.astype(F)
    bx, by = F(1) - ax, F(1) - ay
    return [by * (bx * p[y0, x0] + ax * p[y0, x1]) + ay * (bx * p[y1, x0] + ax * p[y1, x1]) for p in planes]


def np_velocity(u, v, g, sg, axis):
    fa = v if not axis else u
    D = sg + g * fa
    valid = (np.abs(u) <= F(1e9)) & (np.abs(v) <= F(1e9)) & (sg * D >= F(0.5))
    Ds = np.where(valid, D, F(1))
    return np.where(valid, u / Ds, F(0)).astype(F), np.where(valid, v / Ds, F(0)).astype(F)


def restate(img, u, v, frame=0, readout=0.5, anchor=0.5, iters=3, axis=0):
    img = np.asarray(img, np.uint8)
    u, v = np.asarray(u, F), np.asarray(v, F)
    h, w = u.shape
    n = w if axis else h
    g = F(readout) / F(n)
    a0 = F(anchor) * F(n - 1)
    sg = F(-1.0 if frame else 1.0)
    with np.errstate(all="ignore"):
        vx, vy = np_velocity(u, v, g, sg, axis)
        ys, xs = np.mgrid[0:h, 0:w]
        X, Y = xs.astype(F), ys.astype(F)
        px, py = X.copy(), Y.copy()
        for _ in range(int(iters)):
            sx, sy = np_bilinear([vx, vy], px, py)
            t = g * ((px if axis else py) - a0)
            px, py = X + t * sx, Y + t * sy
        c = np_bilinear([img[..., k].astype(F) for k in range(3)], px, py)
        out = [np.floor(np.fmin(np.fmax(p, F(0)), F(255)) + F(0.5)) for p in c]
    return np.stack(out, -1).astype(np.uint8)


def host(img, u, v, frame=0, readout=0.5, anchor=0.5, iters=3, axis=0):
    return io.rolling_shutter_host(img, u, v, frame=frame, readout=readout, anchor=anchor, iters=iters, axis=axis)


# ---- the generators: a periodic band-limited scene in uniform motion, read by a global and by a rolling shutter ----

PERIOD = 256


def scene(seed=0, waves=10, fmax=14):
    """S(X, Y) -> (..., 3) float64 in [8, 248): a sum of `waves` cosines per channel with integer frequencies up to fmax per PERIOD pixels
    (the shortest wavelength is PERIOD / (fmax * sqrt 2) > 12 pixels), periodic with PERIOD in both directions"""
    rng = np.random.default_rng(seed)
    fx = rng.integers(-fmax, fmax + 1, (3, waves))
    fy = rng.integers(-fmax, fmax + 1, (3, waves))
    ph = rng.uniform(0, 2 * np.pi, (3, waves))
    amp = rng.uniform(0.5, 1.0, (3, waves))
    amp = 120.0 * amp / amp.sum(axis=1, keepdims=True)

    def S(X, Y):
        X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
        out = np.empty(X.shape + (3,))
        for c in range(3):
            arg = (2 * np.pi / PERIOD) * (X[..., None] * fx[c] + Y[..., None] * fy[c]) + ph[c]
            out[..., c] = 128.0 + (amp[c] * np.cos(arg)).sum(-1)
        return out
    return S


def shutter_frame(S, h, w, k, motion, readout=0.0, anchor=0.5, axis=0):
    """frame k of the scene moving by `motion` = (mx, my) pixels per frame interval: the sample at coordinate c along the readout axis is
    taken at time k + tau(c), tau(c) = readout / n * (c - anchor * (n - 1)).  readout 0: the global-shutter frame at time k."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    n = w if axis else h
    t = k + (readout / n) * ((xs if axis else ys) - anchor * (n - 1))
    return np.floor(S(xs - t * motion[0], ys - t * motion[1]) + 0.5).astype(np.uint8)


def true_flow(h, w, motion, frame, readout, axis):
    """the flow between two rolling-shutter frames of the uniform motion: a point that moves fa along the readout axis is seen again
    after 1 + g*fa intervals, so fa = ma / (1 - g*ma) forward and -ma / (1 - g*ma) backward, and f = motion * fa / ma"""
    n = w if axis else h
    g = readout / n
    k = (-1.0 if frame else 1.0) / (1.0 - g * motion[1 if not axis else 0])
    return np.full((h, w), k * motion[0], F), np.full((h, w), k * motion[1], F)


def mae(a, b, border):
    s = np.s_[border:a.shape[0] - border, border:a.shape[1] - border]
    return float(np.abs(a[s].astype(np.float64) - b[s].astype(np.float64)).mean())


# (name, h, w, motion, readout, anchor): the three clips of section 27.4
CLIPS = [("down", 40, 64, (0.0, 8.0), 1.0, 0.0), ("diagonal", 48, 64, (6.0, -5.0), 0.75, 0.5), ("up_left", 48, 64, (-7.0, 9.0), 1.0, 0.5)]


# ---- cases ----

SIZES = [(1, 1), (1, 9), (9, 1), (31, 33), (64, 64), (65, 97), (70, 200)]
LIMIT_SIZES = [(20, 8192), (8192, 20)]
# (readout, anchor, iters, axis, frame): both frames, both axes, readout of both signs, anchor 0 / 0.5 / 1, iters 1 and 8
GRID = [(0.5, 0.5, 3, 0, 0), (1.0, 0.0, 8, 0, 1), (-1.0, 1.0, 1, 1, 0), (0.75, 0.5, 3, 1, 1), (-0.5, 0.0, 8, 1, 0), (1.0, 1.0, 1, 0, 0),
         (-0.75, 0.5, 3, 0, 1), (1.0, 0.0, 3, 1, 1), (0.25, 1.0, 8, 0, 0), (-1.0, 0.5, 1, 1, 1)]


def _smooth(h, w, rng, amp):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c, d = rng.uniform(0.05, 0.25, 4)
    u = amp * np.sin(a * xs + b * ys + rng.uniform(0, 6)) + rng.uniform(-2, 2)
    v = amp * np.cos(c * xs - d * ys + rng.uniform(0, 6)) + rng.uniform(-2, 2)
    return u.astype(F), v.astype(F)


def _sprinkle(u, v, rng):
    """1e10 (unknown), NaN, +-inf, the largest known component and huge vectors at random pixels"""
    h, w = u.shape
    for val in (1e10, -1e10, np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38, 4000.0, -4000.0):
        for plane in (u, v):
            plane[rng.integers(h), rng.integers(w)] = val
    y, x = rng.integers(h), rng.integers(w)
    u[y, x] = np.nan
    v[y, x] = np.inf


def _block(u, v, y0, x0, fu, fv, size=3):
    h, w = u.shape
    y0, x0 = max(0, min(y0, h - 1)), max(0, min(x0, w - 1))
    u[y0:y0 + size, x0:x0 + size] = fu
    v[y0:y0 + size, x0:x0 + size] = fv


def rs_cases(sizes=None, grids=None):
    """dicts of name, h, w, img (h, w, 3) uint8, u, v (h, w) float32, params (readout, anchor, iters, axis, frame).  Fields: smooth ones
    with 1e10, NaN, +-inf and huge vectors sprinkled in; a mover at each border; a field half of whose vectors make sg*D < 0.5."""
    sizes = SIZES if sizes is None else sizes
    rng = np.random.default_rng(27)
    cases = []
    g = 0

    def add(name, h, w, u, v):
        nonlocal g
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        grid = (GRID if grids is None else grids)[g % len(GRID if grids is None else grids)]
        g += 1
        cases.append(dict(name=f"{name}_{h}x{w}_r{grid[0]}_a{grid[1]}_i{grid[2]}_x{grid[3]}_f{grid[4]}", h=h, w=w, img=img,
                          u=np.ascontiguousarray(u, F), v=np.ascontiguousarray(v, F), params=grid))

    for h, w in sizes:
        for rep in range(2):
            u, v = _smooth(h, w, rng, 24.0 if rep else 9.0)
            _sprinkle(u, v, rng)
            add("smooth", h, w, u, v)
        z = np.zeros((h, w), F)
        u, v = z.copy(), z.copy()
        _block(u, v, 0, w // 2, 7.0, -30.0)
        _block(u, v, h - 3, w // 3, -9.0, 40.0)
        _block(u, v, h // 2, 0, -25.0, 3.0)
        _block(u, v, h // 3, w - 3, 33.0, -4.0)
        add("border", h, w, u, v)
        # |g * fa| around and beyond one half: with both signs in the field, sg*D < 0.5 on part of it whatever the case's readout and frame
        n = max(h, w)
        u, v = [(rng.uniform(-2.0, 2.0, (h, w)) * n).astype(F) for _ in range(2)]
        add("fold", h, w, u, v)
    return cases


def host_case(c):
    r, a, i, x, f = c["params"]
    return host(c["img"], c["u"], c["v"], f, r, a, i, x)


# ---- 1. ABI ----

def _prototypes(header):
    from test_abi_cpu import _prototypes as p
    return p(header)


def test_binding_table_equals_the_header():
    from test_abi_cpu import _declared, _exported
    protos = _prototypes("eppm_rshutter.h")
    assert list(protos) == list(_lib._RS_ABI) == NAMES
    wrong = {n: (_lib._RS_ABI[n], want) for n, want in protos.items() if _lib._RS_ABI[n] != want}
    assert not wrong, wrong
    assert set(protos) == _declared("eppm_rshutter.h")
    assert not set(protos) & (set(_lib.SYMBOLS) | set(_lib.TEST_SYMBOLS) | set(_lib._YUV_ABI) | set(_lib._DEINT_ABI))
    assert not set(protos) & (_declared("eppm.h") | _declared("eppm_yuv.h") | _declared("eppm_deint.h") | _declared("eppm_test.h"))
    for variant in ("", "test", "tol", "tol_test"):
        assert set(protos) <= _exported(eppm_amd.lib_path(variant)), variant
    L = eppm_amd.lib()
    for n, (res, args) in _lib._RS_ABI.items():
        fn = getattr(L, n)
        assert fn.restype == res and list(fn.argtypes) == args, n
    p = eppm_amd.RSParams()
    assert (p.readout, p.anchor, p.iters, p.axis) == (0.5, 0.5, 3, 0)
    assert eppm_amd.RSParams(iters=5).iters == 5
    with pytest.raises(TypeError, match="^unknown rolling-shutter parameter nonsense$"):
        eppm_amd.RSParams(nonsense=1)


def test_argument_errors_without_a_device():
    L = _lib.lib()
    h = w = 4
    img = np.zeros(h * w * 4, np.uint8)
    f = np.zeros(h * w * 2, np.float32)
    pi, pf = img.ctypes.data, f.ctypes.data

    def prm(r=0.5, a=0.5, n=3, x=0):
        return C.byref(_lib.CRSParams(r, a, n, x))

    def hostc(p=None, out=pi, a=pi, u=pf, v=pf, hh=h, ww=w, frame=0):
        return L.eppm_rolling_shutter_host(out, a, u, v, hh, ww, frame, p)

    def frames(p=None, out=pi, a=pi, flow=pf, hh=h, ww=w, op=w * 4, ip=w * 4, frame=0):
        return L.eppm_rolling_shutter_frames(out, op, a, ip, flow, hh, ww, frame, p)

    nan = float("nan")
    assert L.eppm_rs_default_params(None) == ARG
    for bad in (dict(r=1.5), dict(r=-1.01), dict(r=nan), dict(r=float("inf")), dict(a=-0.1), dict(a=1.1), dict(a=nan), dict(n=0), dict(n=9),
                dict(n=-1), dict(x=2), dict(x=-1)):
        assert hostc(prm(**bad)) == ARG, bad
        assert frames(prm(**bad)) == ARG, bad          # before any HIP call: this process has no GPU
        for fn in (L.eppm_rolling_shutter, L.eppm_batch_rolling_shutter):
            assert fn(None, prm(**bad), 0, pi, w * 3) == ARG
    for bad in (dict(out=None), dict(a=None), dict(u=None), dict(v=None), dict(hh=0), dict(ww=0), dict(hh=-3), dict(hh=8193), dict(ww=8193),
                dict(frame=2), dict(frame=-1)):
        assert hostc(None, **bad) == ARG, bad
    for bad in (dict(out=None), dict(a=None), dict(flow=None), dict(hh=0), dict(ww=0), dict(op=w * 4 - 4), dict(ip=w * 4 + 2), dict(frame=2),
                dict(hh=8193), dict(ww=8193)):
        assert frames(None, **bad) == ARG, bad
    assert L.eppm_rolling_shutter(None, None, 0, pi, w * 3) == ARG
    assert L.eppm_rolling_shutter_device(None, None, 0, pi, w * 4) == ARG
    assert L.eppm_batch_rolling_shutter(None, None, 0, pi, w * 3) == ARG
    # NULL parameters are the defaults; the extremes of every range are accepted
    assert hostc(None) == 0
    for ok in (dict(r=1.0), dict(r=-1.0), dict(r=0.0), dict(a=0.0), dict(a=1.0), dict(n=1), dict(n=8), dict(x=1)):
        assert hostc(prm(**ok)) == 0, ok
        assert hostc(prm(**ok), frame=1) == 0, ok
    z = np.zeros((8193, 1), F)
    with pytest.raises(eppm_amd.EppmError):
        host(np.zeros((8193, 1, 3), np.uint8), z, z)
    with pytest.raises(ValueError):
        host(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5), F), np.zeros((4, 5), F))


# ---- 2. the host form against the restatement ----

def test_host_form_equals_the_restatement_bit_for_bit():
    cs = rs_cases()
    assert {(c["h"], c["w"]) for c in cs} == set(SIZES)
    P = [c["params"] for c in cs]
    assert {p[0] > 0 for p in P} == {True, False} and {p[1] for p in P} == {0.0, 0.5, 1.0} and {1, 8} <= {p[2] for p in P}
    assert {p[3] for p in P} == {0, 1} and {p[4] for p in P} == {0, 1}
    changed = folded = 0
    for c in cs:
        got = host_case(c)
        r, a, i, x, f = c["params"]
        want = restate(c["img"], c["u"], c["v"], f, r, a, i, x)
        bad = np.argwhere((got != want).any(axis=2))
        assert len(bad) == 0, (c["name"], len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        changed += int((got != c["img"]).any())
        if c["name"].startswith("fold"):
            n = c["w"] if x else c["h"]
            sg = F(-1.0 if f else 1.0)
            D = sg + (F(r) / F(n)) * (c["u"] if x else c["v"])
            folded += int((sg * D < F(0.5)).any() and (sg * D >= F(0.5)).any())
    assert changed >= len(cs) // 2
    assert folded >= len(SIZES) - 1           # the fold cases have vectors on both sides of sg*D = 0.5 (a 1x1 frame may not)


def test_identity_at_readout_zero_and_on_static_and_unknown_fields():
    rng = np.random.default_rng(4)
    for h, w in ((37, 70), (1, 9), (9, 1), (1, 1)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        u, v = _smooth(h, w, rng, 20.0)
        _sprinkle(u, v, rng)
        for frame in (0, 1):
            for axis in (0, 1):
                for anchor in (0.0, 0.5, 1.0):
                    assert np.array_equal(host(img, u, v, frame, 0.0, anchor, 8, axis), img), (h, w, frame, axis, anchor)
                for val in (0.0, 1e10, -1e10, np.nan, np.inf):
                    f = np.full((h, w), val, F)
                    for readout in (1.0, -0.75):
                        assert np.array_equal(host(img, f, f, frame, readout, 0.5, 3, axis), img), (h, w, frame, axis, val, readout)
                assert np.array_equal(host(img, np.full((h, w), np.nan, F), np.zeros((h, w), F), frame, 1.0, 0.0, 3, axis), img)


def test_a_horizontal_translation_is_recovered_byte_for_byte():
    """32 x 96, motion (32, 0), readout 1, anchor 0: row y is read y / 32 of an interval late and shows the scene y pixels further on.  The
    correction reads (x + y, y) exactly, so every pixel whose source lies in the frame is the global-shutter frame's byte."""
    h, w, m = 32, 96, (32.0, 0.0)
    S = scene(1)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = xs + ys <= w - 1
    assert int(inside.sum()) == 2576
    for k in (0, 1):
        gs = shutter_frame(S, h, w, k, m)
        rs = shutter_frame(S, h, w, k, m, 1.0, 0.0)
        before = int((gs != rs).any(axis=2).sum())
        assert before > 2900, before                    # every row but the first is displaced
        for frame, fu in ((0, 32.0), (1, -32.0)):
            u, v = true_flow(h, w, m, frame, 1.0, 0)
            assert (u == F(fu)).all() and (v == 0).all()
            got = host(rs, u, v, frame, 1.0, 0.0, 3, 0)
            assert np.array_equal(got[inside], gs[inside]), (k, frame, int((got != gs).any(axis=2)[inside].sum()))
            assert np.array_equal(got, restate(rs, u, v, frame, 1.0, 0.0, 3, 0))


def clip_figures(name, h, w, motion, readout, anchor, border=12, k=1):
    """{"before": MAE of the rolling-shutter frame k against the global-shutter frame, 1, 2, 3, 5: MAE of the corrected frame at that many
    iterations (frame 0, the true forward flow), "back": at 3 iterations from the true backward flow}"""
    S = scene(2)
    gs = shutter_frame(S, h, w, k, motion)
    rs = shutter_frame(S, h, w, k, motion, readout, anchor)
    out = {"before": mae(rs, gs, border)}
    u, v = true_flow(h, w, motion, 0, readout, 0)
    for it in (1, 2, 3, 5):
        out[it] = mae(host(rs, u, v, 0, readout, anchor, it, 0), gs, border)
    bu, bv = true_flow(h, w, motion, 1, readout, 0)
    out["back"] = mae(host(rs, bu, bv, 1, readout, anchor, 3, 0), gs, border)
    return out


@pytest.mark.parametrize("clip", CLIPS, ids=[c[0] for c in CLIPS])
def test_correction_brings_a_rolling_shutter_frame_towards_the_global_shutter_frame(clip):
    """The three clips of DESIGN.md section 27.4 with their true flows, MAE in grey levels with a 12-pixel border left out.  Measured here
    (before -> 1 / 2 / 3 / 5 iterations; from the backward flow): down 18.21 -> 3.75 / 0.78 / 0.18 / 0.16; 0.18, diagonal
    2.80 -> 0.33 / 0.23 / 0.23 / 0.23; 0.23, up_left 6.61 -> 1.22 / 0.31 / 0.21 / 0.20; 0.21."""
    fig = clip_figures(*clip)
    print(clip[0], {k: round(v, 3) for k, v in fig.items()})
    assert fig[3] < fig["before"] and fig["back"] < fig["before"], fig
    assert fig[3] <= fig[1], fig


def test_columns_are_rows_of_the_transposed_frame():
    """axis 1 on a frame is axis 0 on its transpose with u and v exchanged"""
    rng = np.random.default_rng(9)
    h, w = 23, 41
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    u, v = _smooth(h, w, rng, 12.0)
    for frame in (0, 1):
        a = host(img, u, v, frame, 0.8, 0.25, 4, 1)
        b = host(np.ascontiguousarray(img.transpose(1, 0, 2)), v.T, u.T, frame, 0.8, 0.25, 4, 0).transpose(1, 0, 2)
        assert np.array_equal(a, b) and (a != img).any()


# ---- 3. the host code under sanitizers ----

def test_host_form_under_sanitizers(tmp_path):
    """eppm_rolling_shutter_host under ASan + UBSan + float-cast checks: the case sizes, NaN, inf, huge and folding vectors, every parameter
    extreme (tests/csrc/rshutter_sanitize_driver.cpp, a program of its own)."""
    exe = str(tmp_path / "rshutter_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "rshutter_sanitize_driver.cpp"), os.path.join(ROOT, "eppm_amd", "csrc", "eppm_io.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
