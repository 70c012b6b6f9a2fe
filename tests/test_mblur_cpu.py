"""CPU tests of the synthetic shutter's ABI (include/eppm.h: eppm_motion_blur*): the libraries export it, its argument
checks work without a GPU, the host form equals a numpy restatement of section 18 byte for byte, gives the box filter on uniform motion,
returns static frames untouched and moves a blurred mover towards a true long exposure.  mblur_cases() is shared with the GPU tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eppm_amd
from eppm_amd import _lib, io

NEW = ["eppm_mblur_default_params", "eppm_motion_blur", "eppm_motion_blur_device", "eppm_batch_motion_blur", "eppm_motion_blur_frames",
       "eppm_motion_blur_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # (no conftest import: mblur_tol_child.py imports this module)
F = np.float32
TILE = 32


# ---- numpy restatement of DESIGN.md section 18 (written from the text, not from mblur.h) ----

def half_vectors(u, v, shutter, R):
    """(hx, hy, m) float32 planes: 0.5 * shutter * flow, zero where the vector is unknown, clamped to length R"""
    u = np.asarray(u, F)
    v = np.asarray(v, F)
    R = F(R)
    with np.errstate(all="ignore"):
        known = (np.abs(u) <= F(1e9)) & (np.abs(v) <= F(1e9))
        k = F(0.5) * F(shutter)
        hx = np.where(known, k * u, F(0)).astype(F)
        hy = np.where(known, k * v, F(0)).astype(F)
        m = np.sqrt(hx * hx + hy * hy).astype(F)
        far = m > R
        q = (R / np.where(far, m, F(1))).astype(F)
        hx = np.where(far, q * hx, hx).astype(F)
        hy = np.where(far, q * hy, hy).astype(F)
        m = np.where(far, R, m).astype(F)
    return hx, hy, m


def quant(m):
    return np.floor(np.asarray(m, F) * F(8) + F(0.5)).astype(np.int64)


def restate(img, u, v, shutter=0.5, max_radius=16, taps=8):
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    n = int(taps)
    hx, hy, m = half_vectors(u, v, shutter, max_radius)
    mq = quant(m)
    idx = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    key = (m.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - idx)
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    tkey = np.array([[key[by * TILE:(by + 1) * TILE, bx * TILE:(bx + 1) * TILE].max() for bx in range(tx)] for by in range(ty)], np.uint64)
    out = img.copy()
    T = 2 * n + 1
    cols = img.astype(np.int64)
    for by in range(ty):
        for bx in range(tx):
            K = int(tkey[max(by - 1, 0):by + 2, max(bx - 1, 0):bx + 2].max())
            j = 0xffffffff - (K & 0xffffffff)
            jy, jx = divmod(j, w)
            dx, dy, md = hx[jy, jx], hy[jy, jx], m[jy, jx]
            if int(quant(md)) < 4:
                continue
            ys, xs = np.mgrid[by * TILE:min((by + 1) * TILE, h), bx * TILE:min((bx + 1) * TILE, w)]
            own = cols[ys, xs]
            mqx = mq[ys, xs]
            S = np.zeros(own.shape, np.int64)
            for i in range(-n, n + 1):
                t = F(i) / F(n)
                xi = np.floor((xs.astype(F) + t * dx) + F(0.5)).astype(np.int64)
                yi = np.floor((ys.astype(F) + t * dy) + F(0.5)).astype(np.int64)
                dq = int(np.floor((np.abs(t) * md) * F(8) + F(0.5)))
                inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                xc, yc = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
                take = inside & (dq <= np.maximum(mq[yc, xc], mqx))
                if i == 0:
                    take = np.ones_like(take)
                S += np.where(take[..., None], cols[yc, xc], own)
            out[ys, xs] = ((2 * S + T) // (2 * T)).astype(np.uint8)
    return out


# ---- cases ----

SIZES = [(1, 1), (1, 40), (40, 1), (31, 33), (64, 64), (37, 53), (65, 97)]
# a spread of shutter {0.25, 0.5, 1} x R {1, 16, 31} x taps {1, 8, 32}: every value with every other value of another parameter at least once
GRID = [(0.5, 16, 8), (1.0, 31, 32), (0.25, 1, 1), (1.0, 16, 1), (0.5, 31, 8), (0.25, 16, 32), (1.0, 1, 8), (0.5, 1, 32), (0.25, 31, 1),
        (1.0, 16, 32), (0.25, 31, 8), (0.5, 1, 1)]


# (h, w) thin frames at the widest and tallest size eppm_motion_blur_frames and the host form accept: 256 tiles along the long side,
# movers on every border (taps clamped at coordinate 8191), 32 KiB rows under the pitches of mblur_tol_child.frames_kernel
LIMIT_SIZES = [(20, 8192), (8192, 20)]


def _smooth(h, w, rng, amp):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c, d = rng.uniform(0.05, 0.25, 4)
    u = amp * np.sin(a * xs + b * ys + rng.uniform(0, 6)) + rng.uniform(-2, 2)
    v = amp * np.cos(c * xs - d * ys + rng.uniform(0, 6)) + rng.uniform(-2, 2)
    return u.astype(F), v.astype(F)


def _sprinkle(u, v, rng):
    """vectors beyond every R, 1e10 (unknown), NaN and +-inf at random pixels"""
    h, w = u.shape
    for val in (200.0, -300.0, 1e10, -1e10, np.nan, np.inf, -np.inf, 1e9, 3e38):
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


def mblur_cases(sizes=None):
    """dicts of name, h, w, img (h, w, 3) uint8, u, v (h, w) float32, params (shutter, max_radius, taps).  Fields: smooth ones with vectors
    beyond R, 1e10, NaN and +-inf sprinkled in; a static half; a single 3x3 mover in a tile's corner (its vector is dominant in the
    diagonally neighbouring tile); two movers of equal length and different direction in one neighbourhood; a mover at each border."""
    sizes = SIZES if sizes is None else sizes
    rng = np.random.default_rng(18)
    cases = []
    g = 0

    def add(name, h, w, u, v, grid=None):
        nonlocal g
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if grid is None:
            grid = GRID[g % len(GRID)]
            g += 1
        cases.append(dict(name=f"{name}_{h}x{w}_s{grid[0]}_R{grid[1]}_n{grid[2]}", h=h, w=w, img=img, u=np.ascontiguousarray(u, F),
                          v=np.ascontiguousarray(v, F), params=grid))

    for h, w in sizes:
        for rep in range(2):
            u, v = _smooth(h, w, rng, 24.0 if rep else 9.0)
            _sprinkle(u, v, rng)
            add("smooth", h, w, u, v)
        u, v = _smooth(h, w, rng, 14.0)
        if w > 1:
            u[:, :w // 2] = 0
            v[:, :w // 2] = 0
        else:
            u[:h // 2] = 0
            v[:h // 2] = 0
        add("half", h, w, u, v)
        z = np.zeros((h, w), F)
        # a mover at each border, pointing out of and along the frame
        u, v = z.copy(), z.copy()
        _block(u, v, 0, w // 2, 7.0, -30.0)
        _block(u, v, h - 3, w // 3, -9.0, 40.0)
        _block(u, v, h // 2, 0, -25.0, 3.0)
        _block(u, v, h // 3, w - 3, 33.0, -4.0)
        add("border", h, w, u, v)
    for h, w in [s for s in sizes if s[0] >= 35 and s[1] >= 42]:          # of SIZES: 64x64, 37x53, 65x97
        z = np.zeros((h, w), F)
        for grid in [(1.0, 31, 8), (0.5, 16, 32), (1.0, 16, 1)]:
            # a 3x3 mover in the bottom-right corner of tile (0, 0): rows / columns 29..31
            u, v = z.copy(), z.copy()
            _block(u, v, 29, 29, 40.0, 40.0)
            add("corner", h, w, u, v, grid)
        # two movers of one length (|(12, 0)| == |(0, 12)|, |(6, 8)| == |(10, 0)|) in one neighbourhood: the lower index wins
        u, v = z.copy(), z.copy()
        u[20, 30] = 12.0
        v[10, 34] = 12.0
        add("equal_a", h, w, u, v, (1.0, 16, 8))
        u, v = z.copy(), z.copy()
        u[33, 5], v[33, 5] = 6.0, 8.0
        u[30, 40] = 10.0
        add("equal_b", h, w, u, v, (1.0, 31, 8))
    return cases


_CASES = {}


def cases(sizes=None):
    """mblur_cases(sizes) with the restatement's output as "want", computed once per process"""
    key = tuple(SIZES if sizes is None else sizes)
    if key not in _CASES:
        _CASES[key] = mblur_cases(sizes)
        for c in _CASES[key]:
            c["want"] = restate(c["img"], c["u"], c["v"], *c["params"])
    return _CASES[key]


def host(img, u, v, shutter=0.5, max_radius=16, taps=8):
    return io.motion_blur_host(img, u, v, shutter=shutter, max_radius=max_radius, taps=taps)


# ---- tests ----

def test_header_declares_and_libraries_export_the_motion_blur_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eppm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eppm\w*)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    for variant in ("", "test", "tol"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW:
            getattr(L, s)
    p = eppm_amd.MBlurParams()
    assert (p.shutter, p.max_radius, p.taps) == (0.5, 16.0, 8)
    with pytest.raises(TypeError):
        eppm_amd.MBlurParams(radius=3)


def test_host_form_equals_the_restatement_byte_for_byte():
    cs = cases()
    assert {(c["h"], c["w"]) for c in cs} == set(SIZES)
    assert {c["params"][0] for c in cs} == {0.25, 0.5, 1.0} and {c["params"][1] for c in cs} == {1, 16, 31} and {c["params"][2] for c in cs} == {1, 8, 32}
    changed = 0
    for c in cs:
        got = host(c["img"], c["u"], c["v"], *c["params"])
        bad = np.argwhere((got != c["want"]).any(axis=2))
        assert len(bad) == 0, (c["name"], len(bad), bad[:5], got[tuple(bad[0])], c["want"][tuple(bad[0])])
        changed += int((got != c["img"]).any())
    assert changed >= len(cs) - len(SIZES)          # the cases blur: only some 1x1 / R = 1 cases may come back unchanged


def test_host_form_equals_the_restatement_at_the_size_limit():
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "eppm_io.cpp")).read()
    assert "h > %d || w > %d" % (LIMIT_SIZES[1][0], LIMIT_SIZES[0][1]) in src[src.index("int eppm_motion_blur_host"):][:600]
    cs = cases(LIMIT_SIZES)
    assert {(c["h"], c["w"]) for c in cs} == set(LIMIT_SIZES) and len(cs) == 8
    for c in cs:
        got = host(c["img"], c["u"], c["v"], *c["params"])
        bad = np.argwhere((got != c["want"]).any(axis=2))
        assert len(bad) == 0, (c["name"], len(bad), bad[:5], got[tuple(bad[0])], c["want"][tuple(bad[0])])
        assert (got != c["img"]).any(), c["name"]
        if c["name"].startswith("border"):              # the movers on the far borders blur their pixels
            far = (got != c["img"]).any(axis=2)
            assert far[-3:].any() and far[:, -3:].any() and far[:3].any() and far[:, :3].any(), c["name"]
    h, w = LIMIT_SIZES[0]
    z = np.zeros((h, w + 1), F)
    with pytest.raises(eppm_amd.EppmError):
        host(np.zeros((h, w + 1, 3), np.uint8), z, z)


def test_dominant_vector_crosses_a_tile_corner_and_equal_lengths_resolve_to_the_lower_index():
    by_name = {c["name"]: c for c in cases()}
    c = by_name["corner_64x64_s1.0_R31_n8"]
    out = host(c["img"], c["u"], c["v"], *c["params"])
    # the half-vector (20, 20) reaches (32..51, 32..51) of the diagonal tile only: those pixels change, through that tile's neighbourhood
    assert (out[32:40, 32:40] != c["img"][32:40, 32:40]).any()
    assert np.array_equal(out, c["want"])
    # (12, 0) at (20, 30) and (0, 12) at (10, 34): index 10*w + 34 is lower, so the neighbourhood is filtered vertically
    c = by_name["equal_a_64x64_s1.0_R16_n8"]
    out = host(c["img"], c["u"], c["v"], *c["params"])
    ch = np.argwhere((out != c["img"]).any(axis=2))
    assert len(ch) and set(ch[:, 1]) <= {34, 30} and ch[:, 0].min() < 10 and np.array_equal(out, c["want"])


def _box(img, offsets):
    """(2*S + T) // (2*T) of the taps img[y + oy, x + ox] with wrap-around: valid away from the border"""
    S = sum(np.roll(img.astype(np.int64), (-oy, -ox), (0, 1)) for ox, oy in offsets)
    T = len(offsets)
    return ((2 * S + T) // (2 * T)).astype(np.uint8)


def test_uniform_motion_is_the_box_filter_along_it():
    rng = np.random.default_rng(3)
    h, w = 40, 70
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    one = np.ones((h, w), F)
    # (8, 0), shutter 1, taps 4: the nine horizontal neighbours
    out = host(img, 8 * one, 0 * one, 1.0, 16, 4)
    want = _box(img, [(i, 0) for i in range(-4, 5)])
    assert np.array_equal(out[:, 4:-4], want[:, 4:-4])
    # (6, 8), shutter 1, taps 5: half-vector (3, 4), m = 5 exactly: the 11-tap diagonal box, tap i at the rounded (0.6 i, 0.8 i)
    out = host(img, 6 * one, 8 * one, 1.0, 16, 5)
    rnd = {0: 0, 1: 1, 2: 1, 3: 2, 4: 2, 5: 3}, {0: 0, 1: 1, 2: 2, 3: 2, 4: 3, 5: 4}
    offs = [(int(np.sign(i)) * rnd[0][abs(i)], int(np.sign(i)) * rnd[1][abs(i)]) for i in range(-5, 6)]
    want = _box(img, offs)
    assert np.array_equal(out[4:-4, 3:-3], want[4:-4, 3:-3])
    # (100, 0) clamped to R: the box over x + round(i/4 * R), end taps included
    for R in (16, 31):
        out = host(img, 100 * one, 0 * one, 1.0, R, 4)
        dx = (F(R) / F(50)) * F(50)
        assert dx == F(R)
        offs = [(int(np.floor(float(F(i) / F(4) * dx) + 0.5)), 0) for i in range(-4, 5)]
        assert offs[0][0] in (-R, -R + 1) and offs[-1][0] == R
        want = _box(img, offs)
        assert np.array_equal(out[:, R:-R], want[:, R:-R]), R
        assert (out[:, R:-R] != img[:, R:-R]).any()


def test_zero_unknown_and_nan_fields_return_the_input():
    rng = np.random.default_rng(4)
    h, w = 37, 70
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for val in (0.0, 1e10, -1e10, np.nan, np.inf, 0.2):          # 0.2 * 0.5: below half a pixel at every shutter
        f = np.full((h, w), val, F)
        for prm in ((0.5, 16, 8), (1.0, 31, 32), (0.25, 1, 1)):
            assert np.array_equal(host(img, f, f, *prm), img), (val, prm)
    u = np.full((h, w), np.nan, F)
    assert np.array_equal(host(img, u, np.zeros((h, w), F)), img)


def _texture(h, w, seed):
    t = np.random.default_rng(seed).standard_normal((h, w, 3))
    for _ in range(3):
        for ax in (0, 1):
            t = (np.roll(t, 1, ax) + 2 * t + np.roll(t, -1, ax)) / 4
    return np.floor((t - t.min()) / (t.max() - t.min()) * 255).astype(np.uint8)


def test_a_blurred_mover_is_closer_to_a_true_exposure_than_the_sharp_frame():
    """A 16x16 textured square moving 16 px across a static textured background against the mean of the 17 frames of a true exposure, on
    rows 12..35, columns 28..67: the mean absolute error of the blurred frame is below half that of the sharp frame (measured here: 2.9 / 2.3 /
    2.5 grey levels at taps 4 / 8 / 16 against 11.7), and no pixel outside that window changes."""
    h, w = 48, 96
    bg, sq = _texture(h, w, 1), _texture(16, 16, 2)

    def frame(shift):
        f = bg.copy()
        f[16:32, 40 + shift:56 + shift] = sq
        return f

    sharp = frame(0)
    truth = np.mean([frame(s).astype(np.float64) for s in range(-8, 9)], axis=0)
    u = np.zeros((h, w), F)
    u[16:32, 40:56] = 16.0
    win = np.s_[12:36, 28:68]
    e_sharp = np.abs(sharp[win] - truth[win]).mean()
    for taps in (4, 8, 16):
        out = host(sharp, u, np.zeros((h, w), F), 1.0, 16, taps)
        e = np.abs(out[win] - truth[win]).mean()
        print(f"taps {taps}: blurred {e:.2f}, sharp {e_sharp:.2f}")
        assert e < 0.5 * e_sharp, (taps, e, e_sharp)
        rest = np.ones((h, w), bool)
        rest[win] = False
        assert np.array_equal(out[rest], sharp[rest])


def test_argument_errors_without_a_device():
    L = _lib.lib()
    h = w = 4
    img = np.zeros(h * w * 4, np.uint8)
    f = np.zeros(h * w * 2, np.float32)
    pi, pf = img.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    null = C.c_void_p()

    def prm(s=0.5, R=16.0, n=8):
        return C.byref(_lib.CMBlurParams(s, R, n))

    def hostc(p=None, out=pi, a=pi, u=pf, v=pf, hh=h, ww=w):
        return L.eppm_motion_blur_host(out, a, u, v, hh, ww, p)

    def frames(p=None, out=pi, a=pi, flow=pf, hh=h, ww=w, op=w * 4, ip=w * 4):
        return L.eppm_motion_blur_frames(out, C.c_size_t(op), a, C.c_size_t(ip), flow, hh, ww, p)

    assert L.eppm_mblur_default_params(null) == 1
    for bad in (dict(s=0.0), dict(s=1.5), dict(s=float("nan")), dict(s=-0.5), dict(R=0.5), dict(R=32.0), dict(R=float("nan")), dict(n=0), dict(n=33)):
        assert hostc(prm(**bad)) == 1, bad
        assert frames(prm(**bad)) == 1, bad
        for fn in (L.eppm_motion_blur, L.eppm_batch_motion_blur):
            assert fn(null, prm(**bad), 0, pi, C.c_size_t(w * 3)) == 1
    for bad in (dict(out=null), dict(a=null), dict(u=null), dict(v=null), dict(hh=0), dict(ww=0), dict(hh=-3), dict(hh=8193), dict(ww=8193)):
        assert hostc(None, **bad) == 1, bad
    for bad in (dict(out=null), dict(a=null), dict(flow=null), dict(hh=0), dict(ww=0), dict(op=w * 4 - 4), dict(ip=w * 4 + 2)):
        assert frames(None, **bad) == 1, bad
    # NULL context
    assert L.eppm_motion_blur(null, None, 0, pi, C.c_size_t(w * 3)) == 1
    assert L.eppm_motion_blur_device(null, None, 0, pi, C.c_size_t(w * 4)) == 1
    assert L.eppm_batch_motion_blur(null, None, 0, pi, C.c_size_t(w * 3)) == 1
    # NULL parameters are the defaults; the extremes of every range are accepted
    assert hostc(None) == 0
    for ok in (dict(s=1.0), dict(s=1e-3), dict(R=1.0), dict(R=31.0), dict(n=1), dict(n=32)):
        assert hostc(prm(**ok)) == 0, ok


def test_host_form_under_sanitizers(tmp_path):
    """eppm_motion_blur_host under ASan + UBSan + float-cast checks: degenerate sizes, NaN, inf and huge vectors, every parameter extreme
    (tests/csrc/mblur_sanitize_driver.cpp, a program of its own)."""
    exe = str(tmp_path / "mblur_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "mblur_sanitize_driver.cpp"), os.path.join(ROOT, "eppm_amd", "csrc", "eppm_io.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
