"""CPU tests of scene-cut detection (include/eppm.h: eppm_cutdet_*): a numpy restatement of the specification, the
cases cutdet_cases() that the GPU tests share, the host form against the restatement in every integer of the record, what the cases cover
(asserted from the restatement), the argument checks that need no device, and the ABI."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import eppm_amd
from eppm_amd import _lib, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F = np.float32
ARG = 1
NEW = ["eppm_cutdet_default_params", "eppm_cutdet_create", "eppm_cutdet_create_size", "eppm_cutdet_destroy", "eppm_cutdet_step",
       "eppm_cutdet_step_frames", "eppm_cutdet_get", "eppm_cutdet_cuts", "eppm_cutdet_host"]
SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (67, 45), (211, 157), (520, 130)]          # (w, h); 520 x 130: nine tile columns, ragged both ways
FIELDS = ("n", "c1", "c2", "n_tracked", "sad", "cut", "stepped")


# ---- the specification, restated ----

def np_luma(img):
    a = img.astype(np.int64)
    return (77 * a[..., 0] + 150 * a[..., 1] + 29 * a[..., 2] + 128) >> 8


def np_tracked(fx, fy, occ2):
    """(tracked, nx, ny): the tracked pixels of image 2 and, where tracked, the nearest pixel of their source"""
    h, w = fx.shape
    with np.errstate(all="ignore"):
        known = (np.abs(fx) <= F(1e9)) & (np.abs(fy) <= F(1e9))                     # false for NaN
        qx = np.arange(w, dtype=F)[None, :] + fx                                     # one float32 rounding each
        qy = np.arange(h, dtype=F)[:, None] + fy
        inside = (qx >= F(0)) & (qx <= F(w - 1)) & (qy >= F(0)) & (qy <= F(h - 1))
        tracked = (occ2 == 0) & known & inside
        nx = np.where(tracked, np.floor(qx + F(0.5)), 0).astype(np.int64)
        ny = np.where(tracked, np.floor(qy + F(0.5)), 0).astype(np.int64)
    return tracked, nx, ny


def np_r16(residual_max):
    return -1 if residual_max < 0 else int(np.rint(F(residual_max) * F(16)))


def restate(c):
    """the record of case c by the specification"""
    h, w = c["h"], c["w"]
    n = h * w
    c1 = [int((np.minimum(c["occ1"], 3) == k).sum()) for k in range(4)]
    c2 = [int((np.minimum(c["occ2"], 3) == k).sum()) for k in range(4)]
    tracked, nx, ny = np_tracked(c["bu"], c["bv"], c["occ2"])
    assert nx.min() >= 0 and nx.max() <= w - 1 and ny.min() >= 0 and ny.max() <= h - 1       # the tap is always in frame
    y1, y2 = np_luma(c["img1"]), np_luma(c["img2"])
    n_tracked = int(tracked.sum())
    sad = int(np.abs(y2 - y1[ny, nx])[tracked].sum())
    lost = min(n - c1[0], n - n_tracked)
    r16 = np_r16(c["residual_max"])
    by_lost = lost * 1000 > c["lost_permille"] * n
    by_residual = r16 >= 0 and n_tracked > 0 and sad * 16 > r16 * n_tracked
    return dict(n=n, c1=c1, c2=c2, n_tracked=n_tracked, sad=sad, cut=int(by_lost or by_residual), stepped=1, by_lost=by_lost, by_residual=by_residual)


# ---- the cases ----

def _mixed_flow(rng, h, w):
    """a backward field that reaches every branch: integer and fractional vectors into the frame, vectors landing exactly on the last
    column / row, one ulp outside, a denormal below 0, vectors that leave the frame, 1e10, +-inf, NaN and -0.0"""
    xs, ys = np.arange(w, dtype=np.float64)[None, :].repeat(h, 0), np.arange(h, dtype=np.float64)[:, None].repeat(w, 1)
    kind = rng.choice(4, (h, w), p=[0.45, 0.3, 0.1, 0.15])
    tx, ty = rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w))
    fx, fy = (tx - xs).astype(F), (ty - ys).astype(F)                                      # 0: integer vectors into the frame
    frac = kind == 1                                                                       # 1: fractional ones (halves included)
    fx[frac] = (rng.integers(0, 4 * (w - 1) + 1, (h, w)) / 4.0 - xs).astype(F)[frac]
    fy[frac] = (rng.integers(0, 4 * (h - 1) + 1, (h, w)) / 4.0 - ys).astype(F)[frac]
    out = kind == 2                                                                        # 2: vectors that leave the frame
    fx[out] = (rng.choice([-1.0, 1.0], (h, w)) * (w + rng.integers(0, 50, (h, w)))).astype(F)[out]
    with np.errstate(all="ignore"):
        last_x, last_y = (w - 1 - xs).astype(F), (h - 1 - ys).astype(F)
        specials = [                                                                       # 3: one component special, the other stays put
            last_x, np.nextafter(last_x, F(np.inf)), (-xs).astype(F), np.nextafter((-xs).astype(F), F(-np.inf)),
            np.full((h, w), F(-1e-45)), np.full((h, w), F(1e10)), np.full((h, w), F(-1e10)), np.full((h, w), F(np.inf)),
            np.full((h, w), F(-np.inf)), np.full((h, w), F(np.nan)), np.full((h, w), F(-0.0)), np.full((h, w), F(1e9)),
        ]
        specials_y = [last_y, np.nextafter(last_y, F(np.inf)), (-ys).astype(F), np.nextafter((-ys).astype(F), F(-np.inf))] + specials[4:]
    which = rng.integers(0, 2 * len(specials), (h, w))
    for k in range(len(specials)):
        m = (kind == 3) & (which == k)
        fx[m], fy[m] = specials[k][m], F(0)
        m = (kind == 3) & (which == len(specials) + k)
        fx[m], fy[m] = F(0), specials_y[k][m]
    # pinned, so that the smallest sizes have them too: pixel (0, 0) one ulp outside, or a denormal below 0
    if rng.integers(0, 2):
        fx[0, 0], fy[0, 0] = np.nextafter(F(w - 1), F(np.inf)), F(0)
    else:
        fx[0, 0], fy[0, 0] = F(0), F(-1e-45)
    return fx, fy


def _masks(rng, h, w, kind):
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "ones":
        return np.ones((h, w), np.uint8)
    return rng.choice(np.array([0, 1, 2, 3, 200], np.uint8), (h, w), p=[0.7, 0.1, 0.08, 0.07, 0.05])


def _image(rng, h, w, kind):
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# (flow, masks, image 1, image 2, lost_permille, residual_max)
CONFIGS = [("mixed", "random", "random", "random", 500, -1.0), ("mixed", "random", "random", "random", 0, 0.0),
           ("mixed", "random", "random", "random", 1000, 3.5), ("mixed", "random", "random", "random", 1000, 255.0),
           ("zero", "zeros", "black", "white", 1000, 255.0), ("zero", "zeros", "black", "white", 1000, 3.5),
           ("zero", "zeros", "white", "white", 500, 0.0), ("mixed", "ones", "random", "random", 500, -1.0),
           ("mixed", "ones", "random", "random", 1000, 0.0), ("mixed", "zeros", "random", "black", 500, 3.5)]


def _threshold_case(extra, sides):
    """64 x 4, lost_permille 500: 128 + extra pixels of image 1 (sides & 1) / image 2 (sides & 2) have no partner, 128 the other"""
    h, w = 4, 64
    rng = np.random.default_rng(4242 + extra + 7 * sides)
    o1, o2 = np.zeros(h * w, np.uint8), np.zeros(h * w, np.uint8)
    o1[rng.permutation(h * w)[:128 + (extra if sides & 1 else 0)]] = 1
    o2[rng.permutation(h * w)[:128 + (extra if sides & 2 else 0)]] = 2
    z = np.zeros((h, w), F)
    return dict(name=f"64x4-threshold-{extra}-{sides}t", h=h, w=w, img1=_image(rng, h, w, "random"), img2=_image(rng, h, w, "random"), bu=z, bv=z.copy(),
                occ1=o1.reshape(h, w), occ2=o2.reshape(h, w), lost_permille=500, residual_max=-1.0, uniform=False, threshold=(extra, sides))


@functools.lru_cache(maxsize=None)
def _cases():
    return _build(tuple(SIZES), tuple(CONFIGS), 17, True)


# Thin frames at kCutMaxDim: 128 x 2 and 1 x 512 tiles, so 256 and 512 slabs under the finish kernel's 64 lanes (four and eight trips of
# its loop), taps at coordinate 8191, the largest sums of a thin frame (black against white)
LIMIT_SIZES = [(8192, 20), (20, 8192)]
LIMIT_CONFIGS = [CONFIGS[k] for k in (0, 2, 3, 4, 8, 9)]


def cutdet_limit_cases():
    return list(_build(tuple(LIMIT_SIZES), tuple(LIMIT_CONFIGS), 5017, False))


@functools.lru_cache(maxsize=None)
def _build(sizes, configs, seed, thresholds):
    out = []
    for si, (w, h) in enumerate(sizes):
        for ci, (flow, masks, i1, i2, permille, rmax) in enumerate(configs):
            rng = np.random.default_rng(1000 * si + ci + seed)
            if flow == "mixed":
                bu, bv = _mixed_flow(rng, h, w)
            else:
                bu, bv = np.zeros((h, w), F), np.zeros((h, w), F)
            out.append(dict(name=f"{w}x{h}-{ci}", h=h, w=w, img1=_image(rng, h, w, i1), img2=_image(rng, h, w, i2), bu=bu, bv=bv,
                            occ1=_masks(rng, h, w, masks), occ2=_masks(rng, h, w, masks), lost_permille=permille, residual_max=rmax,
                            uniform=masks != "random", threshold=None))
    if thresholds:
        out += [_threshold_case(0, 3), _threshold_case(1, 3), _threshold_case(1, 1), _threshold_case(1, 2)]
    for c in out:
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        c["want"] = restate(c)
    return tuple(out)


def cutdet_cases():
    """the shared cases, each with its restated record under "want"; built once, read-only"""
    return list(_cases())


def differences(want, got):
    return [(k, got[k], want[k]) for k in FIELDS if got[k] != want[k]]


def host_record(c):
    return io.cutdet_host(c["img1"], c["img2"], c["bu"], c["bv"], c["occ1"], c["occ2"], c["lost_permille"], c["residual_max"])


# ---- tests ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_form_equals_the_restatement(size):
    cases = [c for c in cutdet_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) >= len(CONFIGS)
    for c in cases:
        d = differences(c["want"], host_record(c))
        assert not d, (c["name"], d)


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_host_form_equals_the_restatement_at_the_size_limit(size):
    w, h = LIMIT_SIZES[size]
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "cutdet.h")).read()
    assert max(w, h) == int(re.search(r"constexpr int kCutMaxDim = (\d+);", src).group(1))
    cases = [c for c in cutdet_limit_cases() if (c["w"], c["h"]) == (w, h)]
    assert len(cases) == len(LIMIT_CONFIGS)
    for c in cases:
        d = differences(c["want"], host_record(c))
        assert not d, (c["name"], d)
    assert {bool(c["want"]["cut"]) for c in cases} == {False, True}
    assert max(c["want"]["sad"] for c in cases) == 255 * h * w          # black against white, every pixel tracked: the luma difference is 255
    ys, xs = np.mgrid[0:h, 0:w]
    for c in cases[:1]:                               # the mixed field: targets exactly on the last column and row and one ulp beyond them
        with np.errstate(all="ignore"):
            qx, qy = xs.astype(F) + c["bu"], ys.astype(F) + c["bv"]
        for q, n in ((qx, w), (qy, h)):
            assert (q == F(n - 1)).any() and ((q > F(n - 1)) & (q < F(n))).any() and (q == 0).any()


def test_the_cases_cover_what_they_claim():
    cases = cutdet_cases()
    verdicts, lost_alone, residual_alone = set(), 0, 0
    for c in cases:
        want = c["want"]
        verdicts.add(want["cut"])
        lost_alone += want["by_lost"] and not want["by_residual"]
        residual_alone += want["by_residual"] and not want["by_lost"]
        if c["h"] * c["w"] >= 64 and not c["uniform"] and c["threshold"] is None:
            share = want["n_tracked"] / want["n"]
            assert 0.1 <= share <= 0.9, (c["name"], share)
            assert all(k > 0 for k in want["c1"]) and all(k > 0 for k in want["c2"]), c["name"]       # bytes 0..3 and 200 all occur
    assert verdicts == {0, 1} and lost_alone >= 1 and residual_alone >= 1
    # sad at its extremes: every pixel tracked, |dY| = 255 or 0
    full = [c["want"] for c in cases if c["name"].endswith("-4")]
    assert all(r["sad"] == 255 * r["n"] and r["n_tracked"] == r["n"] and r["cut"] == 0 for r in full)     # 255 * 16 * n is not > 255 * 16 * n
    assert all(c["want"]["sad"] == 0 and c["want"]["cut"] == 0 for c in cases if c["name"].endswith("-6"))
    # the mixed fields hold what they claim
    big = next(c for c in cases if c["name"] == "211x157-0")
    fx = big["bu"]
    with np.errstate(all="ignore"):
        assert np.isnan(fx).any() and np.isposinf(fx).any() and np.isneginf(fx).any() and (fx == F(1e10)).any()
        assert ((fx == 0) & np.signbit(fx)).any() and (fx == F(-1e-45)).any() and F(-1e-45) < 0
        xs = np.arange(big["w"], dtype=F)[None, :]
        assert ((xs + fx == F(big["w"] - 1)) & (fx != 0)).any() and (xs + fx == np.nextafter(F(big["w"] - 1), F(np.inf))).any()
        assert (fx != np.rint(fx))[np.isfinite(fx)].any()


def test_the_threshold_is_strict():
    """64 x 4 at lost_permille 500: 128 lost pixels on both sides is lost * 1000 == lost_permille * n, no cut; one more on one side only
    leaves the minimum where it was; one more on both sides is a cut"""
    got = {c["threshold"]: (c["want"], host_record(c)) for c in cutdet_cases() if c["threshold"] is not None}
    for key, (want, rec) in got.items():
        assert not differences(want, rec), key
    w0 = got[(0, 3)][0]
    assert w0["n"] - w0["c1"][0] == 128 and w0["n"] - w0["n_tracked"] == 128 and 128 * 1000 == 500 * w0["n"]
    assert [got[k][1]["cut"] for k in [(0, 3), (1, 1), (1, 2), (1, 3)]] == [0, 0, 0, 1]


def test_argument_checks_without_a_device():
    L = _lib.lib()
    h, w = 4, 5
    img = np.zeros((h, w, 3), np.uint8)
    fl = np.zeros((h, w), F)
    o = np.zeros((h, w), np.uint8)
    st = _lib.CCutStats()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(p, args=None, hh=h, ww=w, stats=st):
        a = [ptr(x) for x in (img, img, fl, fl, o, o)] if args is None else args
        return L.eppm_cutdet_host(C.byref(p) if p is not None else None, *a, hh, ww, C.byref(stats) if stats is not None else None)
    d = _lib.CCutParams()
    assert L.eppm_cutdet_default_params(C.byref(d)) == 0 and (d.lost_permille, d.residual_max) == (530, -1.0)
    assert L.eppm_cutdet_default_params(None) == ARG
    assert call(d) == 0 and st.n == h * w and st.stepped == 1
    for good in [(0, -1.0), (1000, 0.0), (500, 255.0), (500, -0.0), (500, -1e30)]:
        assert call(_lib.CCutParams(*good)) == 0, good
    for bad in [(-1, -1.0), (1001, -1.0), (500, float("nan")), (500, 255.5), (500, float("inf"))]:
        assert call(_lib.CCutParams(*bad)) == ARG, bad
    assert call(None) == ARG and call(d, stats=None) == ARG
    for k in range(6):
        a = [ptr(x) for x in (img, img, fl, fl, o, o)]
        a[k] = None
        assert call(d, a) == ARG, k
    for hh, ww in [(0, 4), (4, 0), (1, 8193), (8193, 1), (8192, 8193)]:
        assert call(d, hh=hh, ww=ww) == ARG, (hh, ww)
    assert L.eppm_cutdet_destroy(None) == 0
    with pytest.raises(ValueError):
        io.cutdet_host(img, img, fl, fl, o, o[:2])
    for name in ("CutDetector", "detect_cuts"):
        assert hasattr(eppm_amd, name)


def test_header_declares_and_all_four_libraries_export_the_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eppm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(eppm\w*)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(_lib.SYMBOLS)
    assert "eppm_cut_params" in hdr and "eppm_cut_stats" in hdr
    assert C.sizeof(_lib.CCutStats) == 96 and C.sizeof(_lib.CCutParams) == 8
    for variant in ("", "test", "tol", "tol_test"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW:
            getattr(L, s)
        for s in _lib.TEST_SYMBOLS:
            assert hasattr(L, s) == variant.endswith("test"), (variant, s)


def test_the_keywords_default_to_off():
    import inspect
    for f in (eppm_amd.flow_sequence, eppm_amd.flow_sequences, eppm_amd.denoise_sequence, eppm_amd.denoise_sequences, eppm_amd.stabilize_sequence,
              eppm_amd.stabilize_sequences):
        assert inspect.signature(f).parameters["auto_cut"].default is False
