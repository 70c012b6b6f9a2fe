"""The LDS-window candidate refine of radius 9 (k_c2f_refine_win<9>) against the oracle, bit for bit, at the smallest shapes that reach
every path of one launch.

c2f_pass2_win evaluates the six (pass, row candidate) terms of a sample in phases across the terms (c2f_device.cuh: c2f_terms), two samples
at a time: a change of instruction order, not of arithmetic, so every flow must stay what the oracle computes.  Each case goes through the
stage call S.c2f_refine with the switch "c2f_no_split" on (the images here have 2 to 10 tiles: a context would split them), on planes built
as the refine cases of tests/test_parity_gpu.py build theirs (the level-0 planes of the crop, cut to size), and is compared as uint32.  The
batch case needs several pairs in one launch, which the stage call cannot issue: it goes through eppm_test_c2f_refine_batch
(S.c2f_refine_batch), the same launcher with blockIdx.y = pair.  The radius-17 kernel (k_c2f_refine_win4) is unchanged and has no case here."""
import ctypes as C

import numpy as np
import pytest

from test_parity_gpu import O, S, eq  # noqa: F401  (S, O: fixtures)
from test_variants_cpu import option

pytestmark = pytest.mark.gpu

R = 9
W, H = 40, 24                      # 2.5 x 1.5 tiles
UNKNOWN = np.float32(1e10)


def cut(st, x0, y0, w, h):
    return tuple(np.ascontiguousarray(st[k][y0:y0 + h, x0:x0 + w]) for k in ("img1_L0", "img2_L0", "cen1_L0", "cen2_L0"))


@pytest.fixture(scope="module")
def planes(crop_stages):
    return cut(crop_stages, 0, 0, W, H)


@pytest.fixture(scope="module")
def radius9(S):
    import eppm_amd
    S.set_params(eppm_amd.Params(patch_r=R))
    with option("c2f_no_split", 1, 0):
        yield
    S.set_params(None)


def flow_of(fx, fy, O):
    f = np.zeros(np.shape(fx), O.float2)
    f["x"], f["y"] = np.asarray(fx).astype(np.float32), np.asarray(fy).astype(np.float32)
    return f


def check(S, O, planes, fx, fy, what):
    f = flow_of(fx, fy, O)
    i1, i2, c1, c2 = planes
    want = O.c2f_refine(f, i1, i2, c1, c2, O.default_params(patch_r=R))
    eq(S.c2f_refine(f, S.PlaneSet(i1, i2, c1, c2)), want, what)
    return want


def test_ragged_tiles_constant_flow(S, O, planes, radius9):
    z = np.zeros((H, W))
    check(S, O, planes, z + 3, z - 2, "40x24, constant integer flow")


def test_image_borders(S, O, planes, radius9):
    """candidate columns and rows past each of the four borders: the whole column is skipped (cx < 0, cx >= w), a row only at selection"""
    ys, xs = np.mgrid[0:H, 0:W]
    z = np.zeros((H, W))
    check(S, O, planes, -xs, z, "centres on column 0: column -1 skipped")
    check(S, O, planes, (W - 1) - xs, z, "centres on the last column: column w skipped")
    check(S, O, planes, z, -ys, "centres on row 0: row -1 skipped at selection")
    check(S, O, planes, z, (H - 1) - ys, "centres on the last row: row h skipped at selection")
    check(S, O, planes, -xs, (H - 1) - ys, "centres on the lower left corner")
    check(S, O, planes, z - 60, z + 50, "every candidate outside the image")


def test_window_boundary(S, O, crop_stages, radius9):
    """one tile whose candidate centres spread exactly SPAN_X (the window's last column is read) and one at SPAN_X + 1 (per-access path),
    next to constant-flow tiles, in one launch; the same along y"""
    import eppm_amd
    sx, sy = C.c_int(), C.c_int()
    assert eppm_amd.lib().eppm_probe_c2f_window(R, C.byref(sx), C.byref(sy)) == 0
    sx, sy = sx.value, sy.value

    def spreads(c, axis):          # max - min of the centres per 16-pixel tile along the axis (the other axis holds one tile row here)
        c = np.moveaxis(c, axis, 0)
        return [int(c[t:t + 16].max() - c[t:t + 16].min()) for t in range(0, c.shape[0], 16)]

    w, h = 48 + sx - 15 + 2, 16                      # three tiles in a row, wide enough for the shifted centres
    pl = cut(crop_stages, 0, 0, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    fx = np.zeros((h, w))
    fx[:, 15] = sx - 15                              # tile 0: spread exactly sx
    fx[:, 47] = sx - 15 + 1                          # tile 2: one more
    assert spreads(xs + fx, 1)[:3] == [sx, 15, sx + 1] and int((xs + fx).max()) < w
    check(S, O, pl, fx, np.zeros((h, w)), "x spread = SPAN_X in tile 0, SPAN_X + 1 in tile 2")
    w, h = 16, 48 + sy - 15 + 2
    pl = cut(crop_stages, 0, 0, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    fy = np.zeros((h, w))
    fy[15, :] = sy - 15
    fy[47, :] = sy - 15 + 1
    assert spreads(ys + fy, 0)[:3] == [sy, 15, sy + 1] and int((ys + fy).max()) < h
    check(S, O, pl, np.zeros((h, w)), fy, "y spread = SPAN_Y in tile 0, SPAN_Y + 1 in tile 2")


def test_unknown_flow(S, O, planes, radius9):
    rng = np.random.default_rng(9)
    fx, fy = rng.normal(0, 1.5, (H, W)) + 2, rng.normal(0, 1.5, (H, W)) - 1
    m = rng.random((H, W)) < 0.1
    fx[m] = UNKNOWN
    fy[m] = UNKNOWN
    fx[:16, 16:32] = UNKNOWN                         # a tile with no known pixel
    fy[:16, 16:32] = UNKNOWN
    fx[20, 3] = UNKNOWN                              # one component alone marks the vector unknown
    fy[21, 35] = UNKNOWN
    want = check(S, O, planes, fx, fy, "unknown vectors scattered, one tile fully unknown")
    assert (want["x"][:16, 16:32] == 0).all() and (want["y"][:16, 16:32] == 0).all()


def test_ties_first_minimum_wins(S, O, radius9):
    """a flat image pair: the nine candidates of a pixel cost the same, the strict < keeps the first one evaluated"""
    a = np.zeros((H, W), O.uchar4)
    for ch in ("x", "y", "z"):
        a[ch] = 117
    ca = O.census(a)
    z = np.zeros((H, W))
    want = check(S, O, (a, a.copy(), ca, ca.copy()), z + 4, z + 3, "flat pair")
    inner = want[2:-2, 2:W - 6]                      # pixels whose nine candidates lie inside the image
    assert (inner["x"] == 3).all() and (inner["y"] == 2).all()        # the first candidate: (-1, -1) from the centre


def test_batch_of_three_pairs(S, O, crop_stages, radius9):
    rng = np.random.default_rng(3)
    z = np.zeros((H, W))
    pls = [cut(crop_stages, x0, y0, W, H) for x0, y0 in ((0, 0), (64, 40), (100, 90))]
    fx2, fy2 = rng.normal(0, 2.0, (H, W)) - 3, rng.normal(0, 2.0, (H, W)) + 2
    fx2[rng.random((H, W)) < 0.05] = UNKNOWN
    flows = [flow_of(z + 2, z - 1, O), flow_of(fx2, fy2, O),
             flow_of(rng.integers(-30, 31, (H, W)), rng.integers(-30, 31, (H, W)), O)]          # coherent, noisy, incoherent
    got = S.c2f_refine_batch(flows, pls)
    op = O.default_params(patch_r=R)
    for k in range(3):
        eq(got[k], O.c2f_refine(flows[k], *pls[k], op), "pair %d of a three-pair launch" % k)
