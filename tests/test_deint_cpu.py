"""CPU tests of motion-compensated deinterlacing: the binding table against include/eppm_deint.h and the ABI's argument
checks, a vectorised numpy restatement of the arithmetic (np_step, np_bob, written from the specification) against eppm_deint_step_host
and eppm_deint_bob_host byte for byte on the shared generator deint_cases() (the GPU tests run the kernels on the same cases), what the
step guarantees, what it reaches on moving clips with true flows, interlaced y4m files, the two clip drivers against recording fakes, and
the host code under sanitizers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, api, io, yuv
from test_abi_cpu import _declared, _exported, _prototypes
from test_defect_cpu import _smooth, np_sample
from test_deflicker_cpu import _vectors
from test_tfilter_cpu import moving_clip, psnr
import test_clip_drivers_cpu as drv

F = np.float32
ARG, STATE = 1, 3
DEFAULTS = dict(thresh=24, use_occ=1)


# ---- the numpy restatement of section 26.1 ----

def np_neighbours(h):
    """(up, dn): per row y the rows y - 1 and y + 1; a row outside the frame is replaced by the other one"""
    y = np.arange(h)
    return np.where(y > 0, y - 1, y + 1), np.where(y + 1 < h, y + 1, y - 1)


def np_bob(field, h, p):
    """the full (h, w, 3) frame of a field picture of parity p: row 2i + p is field row i, every other row the line average"""
    up, dn = np_neighbours(h)
    y = np.arange(h)
    real = (y & 1) == p
    a, b = field[np.where(real, y, up) >> 1].astype(np.int64), field[np.where(real, y, dn) >> 1].astype(np.int64)
    return np.where(real[:, None, None], a, (a + b + 1) >> 1).astype(np.uint8)


def np_step(ref, cur, bu, bv, occ2, parity, thresh=24, use_occ=1, cut=False):
    """(rgb, mask, stats) of one step.  Of cur only the rows of `parity` are read."""
    h, w = bu.shape
    real = ((np.arange(h) & 1) == parity)[:, None]
    only_real = np.where(real[..., None], cur, 0)                 # the missing rows' bytes are out of reach from here on
    up, dn = np_neighbours(h)
    U, Dn = only_real[up].astype(np.int64), only_real[dn].astype(np.int64)
    s, contrast = (U + Dn + 1) >> 1, np.abs(U - Dn).sum(-1)
    m, ok = np_sample(ref, bu, bv)
    if use_occ:
        ok = ok & (occ2 == 0)
    if cut:
        ok = np.zeros_like(ok)
    q = np.floor(np.fmin(np.fmax(m, F(0)), F(255)) + F(0.5)).astype(np.int64)
    accept = ok & (2 * np.abs(q - s).sum(-1) <= 2 * thresh + contrast)
    rgb = np.where(real[..., None], cur, np.where(accept[..., None], q, s)).astype(np.uint8)
    mask = np.where(real, 0, np.where(accept, 1, 2)).astype(np.uint8)
    return rgb, mask, dict(temporal=int((mask == 1).sum()), spatial=int((mask == 2).sum()))


# ---- the shared cases ----

SIZES = [(1, 2), (5, 3), (63, 3), (64, 4), (65, 5), (129, 9), (200, 67)]           # w x h
FLOWS = ("mixed", "zero", "integer", "fractional")
OCCS = ("random", "zero", "one")


def _flow(rng, kind, h, w):
    if kind == "mixed":         # small vectors, 40 % whole, and one pixel in three special: outside on every side, NaN, +-inf, unknown
        return _vectors(rng, h, w)
    if kind == "zero":
        return np.zeros((h, w), F), np.zeros((h, w), F)
    if kind == "integer":
        return np.full((h, w), F(min(1, w - 1))), np.full((h, w), F(-min(1, h - 1)))
    return np.full((h, w), F(0.25 * min(1, w - 1))), np.full((h, w), F(-0.5))


def _field_frame(rng, scene, parity, garbage):
    """a field frame of a scene: the rows of `parity` are the scene's, the others the bob's -- or garbage"""
    h = scene.shape[0]
    out = np_bob(scene[parity::2], h, parity)
    if garbage:
        junk = rng.integers(0, 256, out.shape, dtype=np.uint8)
        out = np.where(((np.arange(h) & 1) == parity)[:, None, None], out, junk)
    return out


def _case(seed, w, h, parity, params=None, cut=False, empty=False, flow="mixed", occ="random", garbage=False):
    """two consecutive steps: a smooth scene with noise; step k's image 2 is a field frame of it, of parity, then of parity ^ 1"""
    rng = np.random.default_rng(seed)
    p = dict(DEFAULTS, **(params or {}))
    base = np.clip(_smooth(rng, h, w) * (0.4 if min(h, w) >= 16 else 0.1) + 60.0, 0, 255)
    noisy = lambda: np.clip(np.rint(base + rng.normal(0, 3.0, base.shape)), 0, 255).astype(np.uint8)       # noqa: E731
    steps = []
    for k in range(2):
        par = parity ^ k
        bu, bv = _flow(rng, flow, h, w)
        o = {"random": np.where(rng.random((h, w)) < 0.15, rng.integers(1, 4, (h, w)), 0), "zero": np.zeros((h, w)), "one": np.ones((h, w))}[occ]
        steps.append(dict(cur=_field_frame(rng, noisy(), par, garbage), bu=bu, bv=bv, occ2=o.astype(np.uint8), parity=par))
    name = f"{w}x{h}-p{parity}-t{p['thresh']}-o{p['use_occ']}-{flow}-occ{occ}" + ("-cut" if cut else "") + ("-empty" if empty else "") + (
        "-garbage" if garbage else "")
    return dict(name=name, h=h, w=w, ref=noisy(), img1=noisy(), steps=steps, params=p, cut=cut, empty=empty, flow=flow, occ=occ, garbage=garbage,
                parity=parity)


_CASES = None


def deint_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for k, (w, h) in enumerate(SIZES):
        for parity in (0, 1):
            out.append(_case(100 + 2 * k + parity, w, h, parity, empty=(k + parity) % 2 == 1, garbage=k % 2 == 0))
    for k, (w, h) in enumerate(SIZES[-3:]):
        variants = [dict(params=dict(thresh=0)), dict(params=dict(thresh=765)), dict(params=dict(use_occ=0)), dict(cut=True), dict(cut=True, empty=True),
                    dict(flow="zero", occ="zero"), dict(flow="integer", occ="zero", empty=True), dict(flow="fractional", occ="one"),
                    dict(flow="fractional", occ="one", params=dict(use_occ=0, thresh=765)), dict(flow="zero", params=dict(thresh=765), garbage=True)]
        for j, v in enumerate(variants):
            out.append(_case(300 + 20 * k + j, w, h, (j + k) & 1, **v))
    _CASES = out
    return out


# thin frames 8192 long (section 16's bound), both ways round; pad: pixels beyond every row of the caller's images
LIMIT_SIZES = [(8192, 2), (2, 8192)]
_LIMIT = None


def deint_limit_cases():
    global _LIMIT
    if _LIMIT is None:
        _LIMIT = [dict(_case(7000 + 2 * i + parity, w, h, parity, empty=parity == 1, garbage=True), pad=(3, 64)[parity])
                  for i, (w, h) in enumerate(LIMIT_SIZES) for parity in (0, 1)]
    return _LIMIT


def run_case(c, step):
    """the case's two steps through step(ref, cur, bu, bv, occ2, parity, thresh=, use_occ=, cut=): [(rgb, mask, stats)] * 2; the second
    step's reference is the first step's output and is no cut"""
    ref = c["img1"] if c["empty"] else c["ref"]
    out = []
    for k, s in enumerate(c["steps"]):
        out.append(step(ref, s["cur"], s["bu"], s["bv"], s["occ2"], s["parity"], cut=c["cut"] and k == 0, **c["params"]))
        ref = out[-1][0]
    return out


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def field_clip(clean, first=0):
    """a progressive clip read as field frames: frame k keeps its rows of parity first ^ (k & 1), the others are bobbed"""
    h = clean[0].shape[0]
    return [np_bob(f[(first ^ (k & 1))::2], h, first ^ (k & 1)) for k, f in enumerate(clean)]


def run_fields(fields, flows, masks, step, first=0, **params):
    """field frames 1 .. n - 1 through step, each from the output before it; the first output is field frame 0 itself"""
    out = [fields[0]]
    for k in range(1, len(fields)):
        out.append(step(out[-1], fields[k], flows[k - 1][0], flows[k - 1][1], masks[k - 1], first ^ (k & 1), **params)[0])
    return out


# ---- 1. ABI ----

NAMES = ["eppm_deint_default_params", "eppm_deint_create", "eppm_deint_create_size", "eppm_deint_destroy", "eppm_deint_reset", "eppm_deint_step",
         "eppm_deint_step_frames", "eppm_deint_get", "eppm_deint_get_device", "eppm_deint_get_mask", "eppm_deint_get_stats", "eppm_deint_get_state",
         "eppm_deint_set_state", "eppm_deint_step_host", "eppm_deint_bob", "eppm_deint_bob_stream", "eppm_deint_bob_host", "eppm_deint_y4m_open_read"]


def test_binding_table_equals_the_header():
    protos = _prototypes("eppm_deint.h")
    assert list(protos) == list(_lib._DEINT_ABI) == NAMES
    wrong = {n: (_lib._DEINT_ABI[n], want) for n, want in protos.items() if _lib._DEINT_ABI[n] != want}
    assert not wrong, wrong
    assert set(protos) == _declared("eppm_deint.h")
    assert not set(protos) & (set(_lib.SYMBOLS) | set(_lib.TEST_SYMBOLS) | set(_lib._YUV_ABI))
    assert not set(protos) & (_declared("eppm.h") | _declared("eppm_yuv.h"))             # the other headers gained nothing
    for variant in ("", "test", "tol", "tol_test"):
        assert set(protos) <= _exported(eppm_amd.lib_path(variant)), variant
    L = eppm_amd.lib()
    for n, (res, args) in _lib._DEINT_ABI.items():
        fn = getattr(L, n)
        assert fn.restype == res and list(fn.argtypes) == args, n


def _err():
    return eppm_amd.lib().eppm_last_error().decode()


def test_argument_errors_arrive_without_a_gpu():
    L = eppm_amd.lib()
    p = _lib.CDeintParams()
    assert L.eppm_deint_default_params(C.byref(p)) == 0 and (p.thresh, p.use_occ) == (24, 1)
    assert eppm_amd.DeintParams(thresh=7).thresh == 7 and eppm_amd.DeintParams().use_occ == 1
    with pytest.raises(TypeError, match="^unknown deinterlacer parameter nonsense$"):
        eppm_amd.DeintParams(nonsense=1)
    assert L.eppm_deint_default_params(None) == ARG
    f = C.c_void_p()
    for bad, word in ((dict(thresh=-1), "thresh"), (dict(thresh=766), "thresh"), (dict(use_occ=2), "use_occ"), (dict(use_occ=-1), "use_occ")):
        q = _lib.CDeintParams(**dict(DEFAULTS, **bad))
        assert L.eppm_deint_create_size(8, 8, 1, 0, C.byref(q), C.byref(f)) == ARG and word in _err() and not f.value
    for h, w, n in ((1, 8, 1), (0, 8, 1), (8, 0, 1), (8, 8, 0), (65536, 65536, 1)):
        assert L.eppm_deint_create_size(h, w, n, 0, C.byref(p), C.byref(f)) == ARG and not f.value, (h, w, n)
    assert L.eppm_deint_create(None, C.byref(p), C.byref(f)) == ARG
    assert L.eppm_deint_create_size(8, 8, 1, 0, C.byref(p), None) == ARG
    assert L.eppm_deint_destroy(None) == 0
    for fn, args in (("reset", (None, 0)), ("step", (None, None, None, None)), ("step_frames", (None, 0, None, None, 0, None, None, 0, 0)),
                     ("get", (None, 0, None, 0)), ("get_device", (None, 0, None, 0)), ("get_mask", (None, 0, None)), ("get_stats", (None, 0, None)),
                     ("get_state", (None, 0, None, None)), ("set_state", (None, 0, None, 0))):
        assert getattr(L, f"eppm_deint_{fn}")(*args) == ARG, fn
    # the host forms
    h, w = 4, 5
    rgb, out, mask = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
    z, st = np.zeros((h, w), F), _lib.CDeintStats()
    a = lambda x: x.ctypes.data                                 # noqa: E731
    good = [C.byref(p), a(out), a(mask), C.byref(st), a(rgb), a(rgb), a(z), a(z), a(mask), h, w, 0, 0]
    assert L.eppm_deint_step_host(*good) == 0
    for k in range(9):
        bad = list(good)
        bad[k] = None
        assert L.eppm_deint_step_host(*bad) == ARG, k
    for k, v in ((9, 1), (10, 0), (11, 2), (11, -1)):
        bad = list(good)
        bad[k] = v
        assert L.eppm_deint_step_host(*bad) == ARG, (k, v)
    bad = list(good)
    bad[1] = bad[4]
    assert L.eppm_deint_step_host(*bad) == ARG and "rgb_out must not be rgb_ref" in _err()
    q = _lib.CDeintParams(766, 1)
    assert L.eppm_deint_step_host(C.byref(q), *good[1:]) == ARG and "thresh" in _err()
    assert L.eppm_deint_bob_host(a(out), a(rgb), h, w, 0) == 0
    for args in ((None, a(rgb), h, w, 0), (a(out), None, h, w, 0), (a(out), a(rgb), 1, w, 0), (a(out), a(rgb), h, 0, 0), (a(out), a(rgb), h, w, 2)):
        assert L.eppm_deint_bob_host(*args) == ARG, args
    # the device bob refuses before any HIP call
    for args in ((None, 32, 8, 32, 4, 5, 0), (8, 32, None, 32, 4, 5, 0), (8, 32, 8, 32, 1, 5, 0), (8, 32, 8, 32, 4, 5, 3), (8, 16, 8, 32, 4, 5, 0),
                 (8, 32, 8, 18, 4, 5, 0), (6, 32, 8, 32, 4, 5, 0)):
        assert L.eppm_deint_bob(*args) == ARG, args
        assert L.eppm_deint_bob_stream(*args, None) == ARG, args


# ---- 2. the host forms against the restatement ----

def test_host_forms_equal_the_restatement_byte_for_byte():
    for c in deint_cases():
        got, want = run_case(c, io.deint_step_host), run_case(c, np_step)
        assert all(same(g, w) for g, w in zip(got, want)), c["name"]
        for s in c["steps"]:
            p = s["parity"]
            field = s["cur"][p::2]
            assert np.array_equal(io.deint_bob_host(field, c["h"], p), np_bob(field, c["h"], p)), c["name"]


@pytest.mark.parametrize("k", range(4), ids=[f"{w}x{h}-p{p}" for w, h in LIMIT_SIZES for p in (0, 1)])
def test_host_forms_equal_the_restatement_at_the_size_limit(k):
    c = deint_limit_cases()[k]
    assert all(same(g, w) for g, w in zip(run_case(c, io.deint_step_host), run_case(c, np_step)))
    p = c["steps"][0]["parity"]
    field = c["steps"][0]["cur"][p::2]
    assert np.array_equal(io.deint_bob_host(field, c["h"], p), np_bob(field, c["h"], p))


def test_cases_cover_every_size_and_parameter():
    cases = deint_cases()
    assert {(c["w"], c["h"], c["parity"]) for c in cases} >= {(w, h, p) for w, h in SIZES for p in (0, 1)}
    assert {(c["w"], c["h"]) for c in deint_limit_cases()} == set(LIMIT_SIZES) and {c["parity"] for c in deint_limit_cases()} == {0, 1}
    assert all(c["pad"] > 0 for c in deint_limit_cases())
    assert {c["params"]["thresh"] for c in cases} == {0, 24, 765} and {c["params"]["use_occ"] for c in cases} == {0, 1}
    assert {(c["cut"], c["empty"]) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c["flow"] for c in cases} == set(FLOWS) and {c["occ"] for c in cases} == set(OCCS)
    assert {c["garbage"] for c in cases} == {False, True}
    for w, h in SIZES:          # every size with an empty and with a loaded slot, with and without garbage in the missing rows
        assert {c["empty"] for c in cases if (c["w"], c["h"]) == (w, h)} == {False, True}, (w, h)
    # the mixed flows hold every special lane in the frames that have room for them
    big = [c for c in cases if c["flow"] == "mixed" and c["w"] * c["h"] >= 1000]
    assert big
    for c in big:
        for s in c["steps"]:
            u, v, h, w = s["bu"], s["bv"], c["h"], c["w"]
            xs, ys = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
            with np.errstate(all="ignore"):
                assert np.isnan(u).any() and np.isnan(v).any() and (u == np.inf).any() and (v == -np.inf).any(), c["name"]
                assert (xs + u < 0).any() and (xs + u > w - 1).any() and (ys + v < 0).any() and (ys + v > h - 1).any(), c["name"]
                assert ((u == 0) & (v == 0)).any() and ((u != np.rint(u)) & np.isfinite(u)).any() and ((u == np.rint(u)) & (u != 0)).any(), c["name"]
    # and the gate decides both ways, the masks hold all three values, the occlusion mask matters where it is used
    for c in cases:
        if c["h"] * c["w"] < 1000 or c["cut"]:
            continue
        for (rgb, mask, st), s in zip(run_case(c, np_step), c["steps"]):
            assert set(np.unique(mask)) <= {0, 1, 2} and st["temporal"] + st["spatial"] == (mask != 0).sum()
            if c["params"]["thresh"] == 24 and c["flow"] == "mixed" and c["occ"] == "random":
                assert st["temporal"] > 0 and st["spatial"] > 0, c["name"]
    with_occ = next(c for c in cases if c["flow"] == "fractional" and c["occ"] == "one" and c["params"]["use_occ"] == 1)
    without = next(c for c in cases if c["flow"] == "fractional" and c["occ"] == "one" and c["params"]["use_occ"] == 0)
    assert run_case(with_occ, np_step)[0][2]["temporal"] == 0 and run_case(without, np_step)[0][2]["temporal"] > 0


# ---- 3. what a step guarantees ----

def test_real_rows_are_image_two_and_missing_rows_ignore_what_image_two_holds_there():
    rng = np.random.default_rng(5)
    for c in deint_cases() + deint_limit_cases():
        got = run_case(c, io.deint_step_host)
        for (rgb, mask, _), s in zip(got, c["steps"]):
            p = s["parity"]
            assert np.array_equal(rgb[p::2], s["cur"][p::2]) and (mask[p::2] == 0).all() and (mask[1 - p::2] != 0).all(), c["name"]
        other = dict(c, steps=[dict(s, cur=np.where(((np.arange(c["h"]) & 1) == s["parity"])[:, None, None], s["cur"],
                                                     rng.integers(0, 256, s["cur"].shape, dtype=np.uint8))) for s in c["steps"]])
        assert all(same(a, b) for a, b in zip(run_case(other, io.deint_step_host), got)), c["name"]


def test_a_cut_step_is_the_bob_of_the_field():
    n = 0
    for c in deint_cases():
        s = c["steps"][0]
        rgb, mask, st = io.deint_step_host(c["ref"], s["cur"], s["bu"], s["bv"], s["occ2"], s["parity"], cut=True, **c["params"])
        assert np.array_equal(rgb, np_bob(s["cur"][s["parity"]::2], c["h"], s["parity"])), c["name"]
        assert st["temporal"] == 0 and st["spatial"] == (c["h"] - len(s["cur"][s["parity"]::2])) * c["w"]
        n += c["cut"]
    assert n >= 2


def test_thresh_765_accepts_every_valid_pixel():
    rng = np.random.default_rng(9)
    h, w = 9, 33
    ref, cur = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    occ = (rng.random((h, w)) < 0.3).astype(np.uint8)
    for (u, v), parity in (((0.0, 0.0), 0), ((1.0, -1.0), 1), ((0.5, 0.25), 0)):
        bu, bv = np.full((h, w), F(u)), np.full((h, w), F(v))
        _, valid = np_sample(ref, bu, bv)
        rgb, mask, _ = io.deint_step_host(ref, cur, bu, bv, occ, parity, thresh=765)
        missing = ((np.arange(h) & 1) != parity)[:, None]
        assert np.array_equal(mask == 1, missing & valid & (occ == 0)) and (mask == 1).any()
        _, mask0, _ = io.deint_step_host(ref, cur, bu, bv, occ, parity, thresh=765, use_occ=0)
        assert np.array_equal(mask0 == 1, missing & valid)


def test_a_static_scene_is_woven_byte_exact_from_the_second_step_on():
    """Zero flow, zero mask: the candidate of a missing pixel is the scene's own byte (the reference's rows of the other parity are real
    rows, from the first step on), so the output is the scene wherever the gate accepts the scene's byte against the scene's own line
    average: 2 sum |P - s| <= 2 thresh + sum |up - dn|.  At thresh 765 that is every pixel of any scene, noise included; at the default
    thresh on the band-limited clip it is all but the few pixels whose vertical detail exceeds the gate (under 1 %; counted from the
    scene alone), and there the output is the line average, at every step alike (limits)."""
    rng = np.random.default_rng(2)
    noise = rng.integers(0, 256, (31, 45, 3), dtype=np.uint8)
    smooth = moving_clip(96, 128, 6, sigma=0, bg_v=(0, 0), sq_v=(0, 0))[0]
    assert all(np.array_equal(f, smooth[0]) for f in smooth)
    for scene, thresh in ((noise, 765), (smooth[0], 48), (smooth[0], 24)):
        h, w, _ = scene.shape
        zero = [(np.zeros((h, w), F), np.zeros((h, w), F))] * 5
        up, dn = np_neighbours(h)
        P, U, Dn = scene.astype(np.int64), scene[up].astype(np.int64), scene[dn].astype(np.int64)
        passes = 2 * np.abs(P - ((U + Dn + 1) >> 1)).sum(-1) <= 2 * thresh + np.abs(U - Dn).sum(-1)
        assert passes.all() if thresh != 24 else 0 < (~passes).mean() < 0.01
        for first in (0, 1):
            fields = field_clip([scene] * 6, first)
            assert not np.array_equal(fields[0], scene)
            for step in (np_step, io.deint_step_host):
                out = run_fields(fields, zero, [np.zeros((h, w), np.uint8)] * 5, step, first, thresh=thresh)
                for k in range(2, 6):
                    missing = ((np.arange(h) & 1) != (first ^ (k & 1)))[:, None]
                    assert np.array_equal((out[k] != scene).any(-1), missing & ~passes & (np_bob(scene[(first ^ (k & 1))::2], h, first ^ (k & 1)) != scene).any(-1))


# ---- 4. quality on true flows ----

CLIPS = dict(plain=dict(bg_v=(2, 0), sq_v=(-1, 2)), critical=dict(bg_v=(2, 1), sq_v=(-1, 2)))
# interior PSNR (dB) of frames 1..7 against the progressive frames, moving_clip(96, 128, 8, sigma=0) read as field frames (top field first),
# true flows and masks: the line average of each field, and the restatement at thresh 12 / 24 / 48 (measured)
TRUE_FLOW_PSNR = dict(
    plain={"bob": [39.27, 39.21, 39.44, 39.22, 39.36, 38.70, 39.44], 12: [46.46, 43.52, 46.12, 43.19, 47.41, 42.23, 45.74],
           24: [51.17, 44.50, 50.46, 44.53, 53.03, 42.98, 51.94], 48: [61.51, 47.19, 63.20, 46.15, 62.49, 44.68, 63.85]},
    critical={"bob": [39.24, 39.26, 39.56, 39.39, 39.83, 39.40, 39.68], 12: [42.42, 40.89, 42.34, 40.99, 42.41, 41.18, 42.63],
              24: [43.14, 41.28, 42.93, 41.04, 43.24, 41.28, 42.84], 48: [43.54, 42.17, 42.72, 41.38, 41.94, 41.03, 41.47]})


@pytest.mark.parametrize("name", list(CLIPS))
def test_every_frame_is_at_least_the_line_average_on_true_flows(name):
    clean, _, flows, masks = moving_clip(96, 128, 8, sigma=0, **CLIPS[name])
    fields = field_clip(clean)
    bob = [psnr(fields[k], clean[k]) for k in range(1, 8)]
    print(name, "line average", [round(float(x), 2) for x in bob])
    assert np.allclose(bob, TRUE_FLOW_PSNR[name]["bob"], atol=0.005), bob
    for thresh in (12, 24, 48):
        out = run_fields(fields, flows, masks, np_step, thresh=thresh)
        got = [psnr(out[k], clean[k]) for k in range(1, 8)]
        print(name, "thresh", thresh, [round(float(x), 2) for x in got], "mean gain", round(float(np.mean(got) - np.mean(bob)), 2))
        assert np.allclose(got, TRUE_FLOW_PSNR[name][thresh], atol=0.005), got
        assert all(g >= b for g, b in zip(got, bob)), (thresh, got, bob)
        if name == "plain":
            recorded = np.mean(TRUE_FLOW_PSNR[name][thresh]) - np.mean(TRUE_FLOW_PSNR[name]["bob"])
            assert recorded > 0 and np.mean(got) - np.mean(bob) >= 0.5 * recorded
        host = run_fields(fields, flows, masks, io.deint_step_host, thresh=thresh)
        assert all(np.array_equal(a, b) for a, b in zip(out, host))


# the first clip on the CPU oracle's cold bidirectional flows, computed on the bobbed field frames, and its occ2 (= the exact library, byte
# for byte), defaults, frames 1..7 (measured; recorded whichever way the figures fall)
ORACLE_FLOW_PSNR = [42.25, 39.46, 41.61, 39.55, 41.59, 39.48, 41.84]


def test_the_first_clip_on_the_cpu_oracles_flows_is_recorded():
    from oracle import oracle as O
    from test_deflicker_gpu import oracle_planes             # CPU code: the oracle's backward branch chained, the host criterion's mask
    O.set_num_threads(min(16, os.cpu_count() or 1))
    clean = moving_clip(96, 128, 8, sigma=0, **CLIPS["plain"])[0]
    fields = field_clip(clean)
    planes = oracle_planes(fields)
    out = [fields[0]]
    for k in range(1, 8):
        out.append(np_step(out[-1], fields[k], *planes[k - 1], k & 1)[0])
    got = [psnr(out[k], clean[k]) for k in range(1, 8)]
    print("oracle flows", [round(float(x), 2) for x in got], "line average", TRUE_FLOW_PSNR["plain"]["bob"])
    assert np.allclose(got, ORACLE_FLOW_PSNR, atol=0.005), got


# ---- 5. interlaced y4m files ----

def write_interlaced(path, frames, tag, fps=(25, 1), depth=8, extra=""):
    """a test-local writer: I420 planes under an I tag of the caller's choice"""
    f0 = frames[0]
    ctag = "C420mpeg2" if depth == 8 else f"C420p{depth}"
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{f0.w} H{f0.h} F{fps[0]}:{fps[1]} {tag} A1:1 {ctag}{extra}\n".encode())
        for fr in frames:
            f.write(b"FRAME\n")
            for p in fr.planes:
                f.write(np.ascontiguousarray(p).tobytes())


def _yuv_frames(rng, h, w, depth, n=2):
    fmt = yuv.YuvFormat(layout=yuv.I420, depth=depth, matrix=yuv.BT601)
    dt = np.uint16 if depth > 8 else np.uint8
    return [yuv.YuvFrame([rng.integers(0, 1 << depth, (r, b // np.dtype(dt).itemsize)).astype(dt) for r, b in yuv.plane_dims(fmt, h, w)], fmt)
            for _ in range(n)]


@pytest.mark.parametrize("native", (False, True))
@pytest.mark.parametrize("tag,mode", (("It", 1), ("Ib", 2), ("Ip", 0)))
@pytest.mark.parametrize("depth", (8, 10))
def test_interlaced_files_come_back_with_their_field_order(tmp_path, native, tag, mode, depth):
    frames = _yuv_frames(np.random.default_rng(3), 8, 6, depth)
    path = tmp_path / "a.y4m"
    write_interlaced(path, frames, tag, fps=(30000, 1001), depth=depth)
    r = yuv.read_y4m(path, native=native, interlaced=True)
    assert (r.h, r.w, r.fps, r.interlace) == (8, 6, (30000, 1001), mode) and r.fmt.depth == depth
    got = list(r)
    assert len(got) == 2 and all(np.array_equal(a, b) for g, f in zip(got, frames) for a, b in zip(g.planes, f.planes))
    if mode:            # the default still refuses, by name
        with pytest.raises(eppm_amd.EppmError, match=rf"interlaced material \({tag}\) is not supported"):
            yuv.read_y4m(path, native=native)


@pytest.mark.parametrize("native", (False, True))
def test_mixed_files_heights_that_do_not_split_and_truncation_are_refused(tmp_path, native):
    rng = np.random.default_rng(4)
    path = tmp_path / "a.y4m"
    write_interlaced(path, _yuv_frames(rng, 8, 6, 8), "Im")
    with pytest.raises(eppm_amd.EppmError, match=r"interlaced material \(Im\) is not supported"):
        yuv.read_y4m(path, native=native, interlaced=True)
    write_interlaced(path, _yuv_frames(rng, 6, 6, 8), "It")
    with pytest.raises(eppm_amd.EppmError, match=r"an interlaced 4:2:0 file needs H a multiple of 4 \(H6\)"):
        yuv.read_y4m(path, native=native, interlaced=True)
    write_interlaced(tmp_path / "b.y4m", _yuv_frames(rng, 6, 6, 8), "Ip")
    assert yuv.read_y4m(tmp_path / "b.y4m", native=native, interlaced=True).interlace == 0        # a progressive file of that height is fine
    write_interlaced(path, _yuv_frames(rng, 8, 6, 8), "Ib")
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-5])
    r = yuv.read_y4m(path, native=native, interlaced=True)
    assert r.interlace == 2
    next(r)
    with pytest.raises(eppm_amd.EppmError, match="malformed: truncated frame"):
        next(r)


def test_two_flat_fields_split_convert_and_bob_into_two_flat_frames():
    fmt = yuv.YuvFormat(layout=yuv.I420, matrix=yuv.BT601)
    top, bottom = np.array([200, 40, 90], np.uint8), np.array([30, 160, 220], np.uint8)
    h, w = 8, 6
    flat = [yuv.from_rgb(np.broadcast_to(c, (h, w, 3)), fmt) for c in (top, bottom)]
    woven = yuv.empty_frame(fmt, h, w)
    for p, a, b in zip(woven.planes, flat[0].planes, flat[1].planes):
        p[0::2], p[1::2] = a[0::2], b[1::2]
    fields = yuv.split_fields(woven)
    assert [(f.h, f.w) for f in fields] == [(4, 6), (4, 6)]
    for par, src in enumerate(flat):
        rgb = yuv.to_rgb(fields[par])
        want = yuv.to_rgb(src)[0, 0]
        assert (rgb == want).all() and np.abs(want.astype(int) - (top, bottom)[par]).max() <= 3
        assert (io.deint_bob_host(rgb, h, par) == want).all()
    with pytest.raises(eppm_amd.EppmError, match="h a multiple of 4"):
        yuv.split_fields(yuv.empty_frame(fmt, 6, 6))


# ---- 6. the drivers against recording fakes ----

FAKED = ("EPPM", "EPPMBatch", "CutDetector", "Deinterlacer")


def run_driver(monkeypatch, fn, *args, script=None, **kw):
    """(trace, result or exception) of a driver under test_clip_drivers_cpu's fakes"""
    mod = sys.modules[eppm_amd.deinterlace_sequence.__module__]
    for name in FAKED:
        monkeypatch.setattr(mod, name, type(name, (drv.Fake,), {"real": getattr(api, name)}))
    drv.TRACE.clear(); drv.COUNT.clear(); drv.SCRIPT.clear()
    drv.SCRIPT.update(script or {})
    try:
        end = drv.nest(getattr(eppm_amd, fn)(*args, **kw))
    except Exception as ex:
        end = ex
    return list(drv.TRACE), end


FRAME = "uint8[4, 6, 3]:"
OPEN1 = ["EPPM1.__init__(0, None)", "EPPM1.init((4, 6))", "EPPM1.set_temporal(True)", "EPPM1.set_stop_level(0)"]
OPEN2 = ["EPPMBatch1.__init__(4, 6, 2, 0, None)", "EPPMBatch1.set_temporal(True)", "EPPMBatch1.set_stop_level(0)"]
DI = "Deinterlacer1.__init__({}, 24, 1, None, 1, 0)"
BIDIR1, BIDIR = "EPPM1.compute_flow_bidirectional_device(None, None, None, None)", "EPPMBatch1.compute_flow_bidirectional_device()"
LOOK = ["CutDetector1.step(None)", "CutDetector1.cuts(None)"]


def test_one_clip_is_two_field_frames_per_frame_with_alternating_parity(monkeypatch):
    """two flat frames (bytes 0 and 1) are four field frames 0, 0, 1, 1: one set_data, two pushes, three steps of parity 1, 0, 1"""
    trace, end = run_driver(monkeypatch, "deinterlace_sequence", drv.clip(0, 2), thresh=12, params="P")
    assert trace == ["EPPM1.__init__(0, 'P')", "EPPM1.init((4, 6))", "EPPM1.set_temporal(True)", "EPPM1.set_stop_level(0)",
                     "Deinterlacer1.__init__(EPPM1, 12, 1, None, 1, 0)",
                     f"EPPM1.set_data({FRAME}0, {FRAME}0)", BIDIR1, "Deinterlacer1.step(None, [1], None)", "Deinterlacer1.frame(0)",
                     f"EPPM1.push_frame({FRAME}1)", BIDIR1, "Deinterlacer1.step(None, [0], None)", "Deinterlacer1.frame(0)",
                     f"EPPM1.push_frame({FRAME}1)", BIDIR1, "Deinterlacer1.step(None, [1], None)", "Deinterlacer1.frame(0)",
                     "Deinterlacer1.close()", "EPPM1.close()"]
    assert end == [f"{FRAME}0", "'Deinterlacer1.frame#8'", "'Deinterlacer1.frame#12'", "'Deinterlacer1.frame#16'"]
    # bottom field first turns every parity round; single rate keeps one frame per first field; masks are read next to the frames
    trace, end = run_driver(monkeypatch, "deinterlace_sequence", drv.clip(0, 2), tff=False, double_rate=False, masks=True)
    assert [t for t in trace if ".step(" in t] == [f"Deinterlacer1.step(None, [{p}], None)" for p in (0, 1, 0)]
    assert end == ["tuple", [f"{FRAME}0", "'Deinterlacer1.frame#13'"], ["uint8[4, 6]:2", "'Deinterlacer1.mask#14'"]]
    # one interlaced frame is a clip of two field frames
    trace, end = run_driver(monkeypatch, "deinterlace_sequence", drv.clip(3, 1))
    assert trace == OPEN1 + [DI.format("EPPM1"), f"EPPM1.set_data({FRAME}30, {FRAME}30)", BIDIR1, "Deinterlacer1.step(None, [1], None)",
                             "Deinterlacer1.frame(0)", "Deinterlacer1.close()", "EPPM1.close()"]


def test_auto_cut_passes_the_verdict_next_to_the_parity(monkeypatch):
    trace, end = run_driver(monkeypatch, "deinterlace_sequence", drv.clip(0, 2), auto_cut=True, lost_permille=400, script=dict(cuts={1: [0]}))
    read = ["Deinterlacer1.frame(0)"]
    assert trace == OPEN1 + [DI.format("EPPM1"), "CutDetector1.__init__(EPPM1, 400, -1.0, None, 1, 0)",
                             f"EPPM1.set_data({FRAME}0, {FRAME}0)", BIDIR1] + LOOK + ["Deinterlacer1.step([False], [1], None)"] + read + [
                             f"EPPM1.push_frame({FRAME}1)", BIDIR1] + LOOK + ["EPPM1.temporal_reset()", "Deinterlacer1.step([True], [0], None)"] + read + [
                             f"EPPM1.push_frame({FRAME}1)", BIDIR1] + LOOK + ["Deinterlacer1.step([False], [1], None)"] + read + [
                             "CutDetector1.close()", "Deinterlacer1.close()", "EPPM1.close()"]


def test_two_slots_a_clip_change_and_an_idle_slot_carry_their_own_parities(monkeypatch):
    """clips of 1, 2 and 1 frames are 2, 4 and 2 field frames through two slots: slot 0 takes clip 2 at the second step (cut flag, field
    frame 0, parity `first`), then steps to its field frame 1 while slot 1 ends; bottom field first"""
    trace, end = run_driver(monkeypatch, "deinterlace_sequences", drv.clips((1, 2, 1)), slots=2, tff=False)
    assert trace == OPEN2 + [DI.format("EPPMBatch1"),
                             f"EPPMBatch1.set_data([({FRAME}0, {FRAME}0), ({FRAME}10, {FRAME}10)])", BIDIR, "Deinterlacer1.step([False, False], [0, 0], None)",
                             "Deinterlacer1.frame(0)", "Deinterlacer1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}20, {FRAME}11], [True, False])", BIDIR, "Deinterlacer1.step([True, False], [1, 1], None)",
                             "Deinterlacer1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}20, {FRAME}11], [False, False])", BIDIR, "Deinterlacer1.step([False, False], [0, 0], None)",
                             "Deinterlacer1.frame(0)", "Deinterlacer1.frame(1)", "Deinterlacer1.close()", "EPPMBatch1.close()"]
    assert end == [[f"{FRAME}0", "'Deinterlacer1.frame#7'"],
                   [f"{FRAME}10", "'Deinterlacer1.frame#8'", "'Deinterlacer1.frame#12'", "'Deinterlacer1.frame#17'"],
                   [f"{FRAME}20", "'Deinterlacer1.frame#16'"]]
    # a slot with nothing left is fed its last field frame again, with that frame's parity
    trace, _ = run_driver(monkeypatch, "deinterlace_sequences", drv.clips((1, 2)), slots=8)
    assert [t for t in trace if ".step(" in t] == ["Deinterlacer1.step([False, False], [1, 1], None)", "Deinterlacer1.step([False, False], [1, 0], None)",
                                                   "Deinterlacer1.step([False, False], [1, 1], None)"]


def test_a_compute_that_fails_in_flight_closes_detector_stage_and_context_in_order(monkeypatch):
    trace, end = run_driver(monkeypatch, "deinterlace_sequences", drv.clips((2, 2)), slots=2, auto_cut=True, script=dict(fail_at=2))
    assert isinstance(end, RuntimeError) and str(end) == "scripted failure in compute"
    assert trace == OPEN2 + [DI.format("EPPMBatch1"), "CutDetector1.__init__(EPPMBatch1, 530, -1.0, None, 1, 0)",
                             f"EPPMBatch1.set_data([({FRAME}0, {FRAME}0), ({FRAME}10, {FRAME}10)])", BIDIR] + LOOK + [
                             "Deinterlacer1.step([False, False], [1, 1], None)", "Deinterlacer1.frame(0)", "Deinterlacer1.frame(1)",
                             f"EPPMBatch1.push_frames([{FRAME}1, {FRAME}11], [False, False])", BIDIR,
                             "CutDetector1.close()", "Deinterlacer1.close()", "EPPMBatch1.close()"]


@pytest.mark.parametrize("fn,args,kw,message", [
    ("deinterlace_sequence", (drv.clip(0, 2),), dict(stop_level=1.5), "stop level must be an integer, not 1.5"),
    ("deinterlace_sequence", (drv.clip(0, 2),), dict(bogus=1), "unknown parameter bogus"),
    ("deinterlace_sequence", (drv.clip(0, 2),), dict(thresh=16, residual_max=1.0), "need auto_cut=True"),
    ("deinterlace_sequence", ([],), {}, "at least one frame per clip"),
    ("deinterlace_sequence", ([np.zeros((1, 6, 3), np.uint8)],), {}, "h >= 2"),
    ("deinterlace_sequences", ([drv.clip(0, 1), []],), {}, "at least one frame per clip"),
    ("deinterlace_sequences", (drv.clips((2, 2)),), dict(slots=0), "at least one slot"),
    ("deinterlace_sequences", (drv.clips((2, 2)),), dict(lost_permille=400), "need auto_cut=True"),
])
def test_a_refusal_opens_nothing(monkeypatch, fn, args, kw, message):
    trace, end = run_driver(monkeypatch, fn, *args, **kw)
    assert isinstance(end, (eppm_amd.EppmError, TypeError)) and message in str(end) and trace == []


def test_the_step_hook_leaves_every_other_driver_as_it_was(monkeypatch):
    """a driver that passes no step_args calls stage.step with the cut flags alone"""
    mod = sys.modules[eppm_amd.deinterlace_sequence.__module__]
    for name in ("EPPM", "EPPMBatch", "CutDetector", "Deflicker"):
        monkeypatch.setattr(mod, name, type(name, (drv.Fake,), {"real": getattr(api, name)}))
    drv.TRACE.clear(); drv.COUNT.clear(); drv.SCRIPT.clear()
    eppm_amd.deflicker_sequence(drv.clip(0, 3))
    assert [t for t in drv.TRACE if ".step(" in t] == ["Deflicker1.step(None, None)"] * 2


# ---- 7. the host code under sanitizers ----

def test_host_forms_and_the_interlaced_reader_under_sanitizers(tmp_path):
    """deint.h through the two host forms at the case sizes, and the interlaced y4m open / read on good and malformed files, under ASan +
    UBSan + float-cast checks (tests/csrc/deint_sanitize_driver.cpp, a program of its own, built without HIP)"""
    exe = str(tmp_path / "deint_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "deint_sanitize_driver.cpp"), os.path.join(ROOT, "eppm_amd", "csrc", "eppm_io.cpp"), "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "deint sanitize driver: ok" in out.stdout, out.stdout + out.stderr
