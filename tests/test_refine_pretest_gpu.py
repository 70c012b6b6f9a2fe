"""The two-phase form of the LDS-window candidate refine (k_c2f_refine_win<9>) against the oracle, bit for bit.

A coherent tile first forms the centre-row sums of its 36 (candidate, pass) pairs per pixel, evaluates the best estimate k* in full and then
only the pairs that  N (1 - eps) >= B (D_A + U)  cannot reject; a tile with a centre-row weight sum at or below 2^-60, or with more survivors
than its list holds, takes the one-phase loop.  None of that may change a flow: every case is one launch through eppm_test_c2f_refine_pre
(S.c2f_refine_pre: the batch launcher with the form chosen per call and the kernel's counters), run two-phase and one-phase, and both are
compared with O.c2f_refine as uint32.  The counters say which path the tiles took: the cases with a near-true flow (real, real_shifted, unknown) must finish most tiles in the
two-phase form at 83x61 and 33x17; the far-from-true flows (constant, borders, step) fill most survivor lists and exercise that fallback; stripes
and checker the weight-sum fallback.

Shapes: 83x61 (6 x 4 tiles, ragged both ways), 33x17 (a 1-pixel tile column, a 1-row tile row), 16x16 (one tile, every candidate near a
border)."""
import numpy as np
import pytest

from test_parity_gpu import O, S, eq  # noqa: F401  (S, O: fixtures)
from test_refine_schedule_gpu import cut, flow_of

pytestmark = pytest.mark.gpu

R = 9
SHAPES = [(83, 61), (33, 17), (16, 16)]
UNKNOWN = np.float32(1e10)


@pytest.fixture(scope="module")
def radius9(S):
    import eppm_amd
    S.set_params(eppm_amd.Params(patch_r=R))
    yield
    S.set_params(None)


@pytest.fixture(scope="module")
def upflow(crop_stages, O):
    """the crop's level-1 flow brought to level 0 as the path does it (resize, x 2): what the level-0 refine really receives"""
    h, w = crop_stages["arrH"][0], crop_stages["arrW"][0]
    return O.mul_scalar(O.resize_flow(crop_stages["flow_L1"], h, w), 2.0)


def synthetic(O, kind, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "flat":
        a = np.full((h, w), 117, np.uint8)
        b = a
    elif kind == "checker":          # saturated 8x8 blocks, image 2 shifted by (2, 1)
        a = ((((ys // 8) + (xs // 8)) & 1) * 255).astype(np.uint8)
        b = np.roll(a, (1, 2), (0, 1))
    else:                            # "stripes": saturated columns one pixel wide -- every sample (odd offsets) differs from its centre by 1.0,
        a = ((xs & 1) * 255).astype(np.uint8)          # so every weight underflows and every centre-row weight sum is (next to) zero
        b = np.roll(a, 2, 1)
    i1, i2 = (O.rgb2rgba(np.ascontiguousarray(np.repeat(v[:, :, None], 3, 2))) for v in (a, b))
    return i1, i2, O.census(i1), O.census(i2)


def case(O, crop_stages, upflow, kind, w, h):
    """-> (planes, [flows])"""
    ys, xs = np.mgrid[0:h, 0:w]
    z = np.zeros((h, w))
    pl = cut(crop_stages, 0, 0, w, h)
    if kind == "constant":
        return pl, [flow_of(z + 3, z - 2, O)]
    if kind == "real":               # true flow about (7, 4): the candidates of the last columns and rows leave the image on the right and below
        return pl, [np.ascontiguousarray(upflow[:h, :w])]
    if kind == "real_shifted":       # image 2 cut 8 columns and 5 rows further in: true flow about (-1, -1), so that the candidates of the first
        p2 = cut(crop_stages, 8, 5, w, h)          # columns and rows leave the image on the left and above, k* itself on the border
        f = np.ascontiguousarray(upflow[:h, :w]).copy()
        f["x"] -= 8
        f["y"] -= 5
        return (pl[0], p2[1], pl[2], p2[3]), [f]
    if kind == "step":               # a step of 30 rows (the window admits a spread of 21 at most) through the middle: the tile row that holds it
        return pl, [flow_of(z + 1, np.where(ys < h // 2, 0, 30), O)]          # is incoherent, its neighbours are coherent
    if kind == "unknown":
        rng = np.random.default_rng(9)
        fx, fy = upflow["x"][:h, :w].astype(np.float64), upflow["y"][:h, :w].astype(np.float64)          # the real flow, with holes
        m = rng.random((h, w)) < 0.1
        fx[m] = UNKNOWN
        fy[m] = UNKNOWN
        x0 = 16 * ((w - 1) // 16)
        fx[:16, x0:] = UNKNOWN       # a tile with no known pixel
        fy[:16, x0:] = UNKNOWN
        fx[h // 2, 3] = UNKNOWN      # one component alone marks the vector unknown
        return pl, [flow_of(fx, fy, O)]
    if kind == "borders":            # candidate columns / rows past each of the four borders, so that k* itself lies on the border
        return pl, [flow_of(np.where(xs < w // 2, -xs, (w - 1) - xs), z, O), flow_of(z, np.where(ys < h // 2, -ys, (h - 1) - ys), O),
                    flow_of(z - 60, z + 50, O)]
    if kind == "flat":
        return synthetic(O, "flat", w, h), [flow_of(z + 4, z + 3, O)]
    if kind == "checker":
        return synthetic(O, "checker", w, h), [flow_of(z + 2, z + 1, O)]
    assert kind == "stripes"
    return synthetic(O, "stripes", w, h), [flow_of(z + 2, z, O)]


def run(S, O, flows, planes, what):
    """one launch in each form against the oracle; -> the two-phase launch's counters"""
    op = O.default_params(patch_r=R)
    want = [O.c2f_refine(f, *p, op) for f, p in zip(flows, planes)]
    stats = {}
    for pre in (1, 0):
        got, stats[pre] = S.c2f_refine_pre(flows, planes, pre)
        for k in range(len(flows)):
            eq(got[k], want[k], "%s, pair %d, c2f_pre = %d" % (what, k, pre))
    h, w = flows[0].shape
    tiles = ((w + 15) // 16) * ((h + 15) // 16) * len(flows)
    assert sum(stats[1][:4]) == tiles and stats[0] == (0, 0, 0, tiles, 0, 0), (what, stats)
    print(what, "tiles two-phase / weight sum small / list full / one-phase, pairs tested, rejected:", stats[1])
    return stats[1]


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", ["constant", "real", "real_shifted", "step", "unknown", "borders", "flat", "checker", "stripes"])
def test_two_phase_equals_the_oracle(S, O, crop_stages, upflow, radius9, kind, w, h):
    pl, flows = case(O, crop_stages, upflow, kind, w, h)
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    for n, f in enumerate(flows):
        st = run(S, O, [f], [pl], "%s %d, %dx%d" % (kind, n, w, h))
        if kind in ("constant", "real"):
            assert st[0] + st[2] > 0 and st[1] == 0 and st[5] > 0, st  # the pre-test ran and rejected something
        if kind in ("real", "real_shifted"):
            # Coherent tiles all, none with a small weight sum; a near-true flow lets most survivor lists fit (a tile whose list is full is
            # legitimate and falls back), so the two-phase form itself meets the candidates past each of the four borders, k* on the border
            # and the pixels without a candidate (k = 15): more than half of the tiles wherever there are several.
            assert st[0] + st[2] == tiles and st[5] > 0, st
            assert st[0] > tiles // 2 or tiles == 1, st
        if kind == "constant" and (w, h) == (83, 61):
            assert st[0] + st[2] == tiles, st                          # every tile is coherent
        if kind == "step" and (w, h) == (83, 61):
            assert st[3] >= 6 and st[0] > 0, st                        # the tile row with the step took the per-access path
        if kind == "unknown":
            assert st[3] >= 1 and st[1] == 0, st                       # the tile without a known pixel does what it did,
            assert st[0] > (tiles - st[3]) // 2 or tiles == 1, st      # most of the others are two-phase around their holes
        if kind == "stripes":
            assert st[1] > 0 and st[2] == 0, st                        # tiles fell back before anything was tested
            if w > 16 * ((w - 1) // 16) + 1:                           # (a 1-pixel tile column at the border sees its own clamped column: weights of 1)
                assert st[1] == tiles and st[4] == 0, st
        if kind == "flat":
            assert st[5] == 0, st                                      # B = 0 (identical images): nothing may be rejected


def test_counters_equal_the_numpy_model_on_the_crop(S, O, crop_stages, upflow, radius9):
    """tiles by path, pairs tested and pairs rejected of one launch equal what tools/refine_pretest_model.py counts: the kernel's pre-test
    decides every one of the 140 000 pairs as the float32 restatement does, which is what tests/test_refine_pretest_cpu.py proves things about"""
    import ctypes as C
    import os
    import sys
    import eppm_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import refine_pretest_model as RM
    w, h = SHAPES[0]
    pl, flows = case(O, crop_stages, upflow, "real", w, h)
    _, row0, rows, cap, eps, dmin, rhsmin = S.probe_c2f_pretest(R)
    sx, sy = C.c_int(), C.c_int()
    assert eppm_amd.lib().eppm_probe_c2f_window(R, C.byref(sx), C.byref(sy)) == 0
    r = RM.refine(pl, flows[0], list(range(row0, row0 + rows)), eps, dmin, rhsmin, R, exact_all=False)
    want = RM.tile_paths(r, sx.value, sy.value, cap)
    _, st = S.c2f_refine_pre(flows, [pl], 1)
    print("kernel", st, "model", want)
    assert st == want


@pytest.mark.parametrize("kind", ["real", "real_shifted", "unknown"])
def test_pretest_sums_equal_the_numpy_model_to_the_last_bit(S, O, crop_stages, upflow, radius9, kind):
    """N, D_A and U as the kernel's pre-test forms them (its probing instantiation: the same code, which also stores them) against
    tools/refine_pretest_model.py as uint32, for every valid (candidate, pass) of every known pixel of the 83x61 crop: the CPU proof of
    tests/test_refine_pretest_cpu.py is about the arithmetic the kernel runs.  The flow of the probing launch is the oracle's."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import refine_pretest_model as RM
    w, h = SHAPES[0]
    pl, flows = case(O, crop_stages, upflow, kind, w, h)
    _, row0, rows, cap, eps, dmin, rhsmin = S.probe_c2f_pretest(R)
    rows_a = list(range(row0, row0 + rows))
    r = RM.centre_sums(pl, flows[0], rows_a, R)
    got, N, D, U = S.c2f_refine_probe(flows, [pl])
    eq(got[0], O.c2f_refine(flows[0], *pl, O.default_params(patch_r=R)), "probing launch, " + kind)
    known, valid = r["known"], np.repeat(r["valid"][:, :, None, :], 4, 2)
    assert valid.sum() > 100000 or kind == "unknown"
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    full_tiles = np.ones((h, w), bool)
    if kind == "unknown":            # the tile without a known pixel forms nothing
        full_tiles[:16, 16 * ((w - 1) // 16):] = False
        assert np.isnan(U[0][~full_tiles]).all()
    assert (u32(U[0])[known & full_tiles] == u32(r["U"])[known & full_tiles]).all()
    assert np.isnan(U[0][~known]).all()
    assert (u32(N[0])[valid] == u32(r["N"])[valid]).all()
    assert (u32(D[0])[valid] == u32(r["D"])[valid]).all()


@pytest.mark.parametrize("w,h", SHAPES)
def test_two_pair_batch_with_fallback_tiles(S, O, crop_stages, upflow, radius9, w, h):
    """pair 0: the crop with its real flow (two-phase tiles); pair 1: stripes (every tile falls back) -- one launch"""
    p0, f0 = case(O, crop_stages, upflow, "real", w, h)
    p1, f1 = case(O, crop_stages, upflow, "stripes", w, h)
    st = run(S, O, [f0[0], f1[0]], [p0, p1], "real + stripes, %dx%d" % (w, h))
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    assert st[1] >= tiles - 2 and st[0] > 0, st
