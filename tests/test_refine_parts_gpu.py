"""The two-phase window refine with more survivors than one list holds (k_c2f_refine_win<9>), bit for bit
against the oracle through eppm_test_c2f_refine_pre.

Such a tile used to run its pre-test and then the whole one-phase loop.  Now its survivors go through the list in parts -- the halves of
the tile's pixels, else the quarters -- and the tile stays in the two-phase form.  Every case is one launch in each form (two-phase,
one-phase), both compared with O.c2f_refine as uint32, and the kernel's counters say which path the tiles took: [2] tiles with more
survivors than one list, of which [6] drained in halves and [7] in quarters, so that [2] - [6] - [7], the tiles that fell back to the
one-phase loop for a full list, must be 0 everywhere.  The constant flows and the counters expected of them were chosen with the numpy
model (tests/test_refine_bound_cpu.py: FLOWS, COUNTERS, held to the model there) so that each split is reached at each shape that has the
pixels for it.

Shapes: 83x61 (6 x 4 tiles, ragged both ways), 33x17 (a 1-pixel tile column, a 1-row tile row), 16x16 (one tile)."""
import numpy as np
import pytest

from test_parity_gpu import O, S, eq  # noqa: F401  (S, O: fixtures)
from test_refine_bound_cpu import COUNTERS, FLOWS
from test_refine_pretest_gpu import R, SHAPES, case, radius9, upflow  # noqa: F401  (radius9, upflow: fixtures)
from test_refine_schedule_gpu import cut, flow_of

pytestmark = pytest.mark.gpu


def run(S, O, flows, planes, what):
    """one launch in each form against the oracle; -> the two-phase launch's eight counters"""
    op = O.default_params(patch_r=R)
    want = [O.c2f_refine(f, *p, op) for f, p in zip(flows, planes)]
    stats = {}
    for pre in (1, 0):
        got, stats[pre] = S.c2f_refine_pre(flows, planes, pre, parts=True)
        for k in range(len(flows)):
            eq(got[k], want[k], "%s, pair %d, c2f_pre = %d" % (what, k, pre))
    h, w = flows[0].shape
    tiles = ((w + 15) // 16) * ((h + 15) // 16) * len(flows)
    st = stats[1]
    print(what, "tiles one list / weight sum small / several lists / one-phase, pairs tested, rejected, tiles in halves / quarters:", st)
    assert sum(st[:4]) == tiles and stats[0] == (0, 0, 0, tiles, 0, 0, 0, 0), (what, stats)
    assert st[2] - st[6] - st[7] == 0, (what, st)          # no tile took the one-phase loop because its list was full
    return st


def test_the_library_drains_full_lists_in_parts(S):
    assert S.probe_c2f_parts(R)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", ["far", "halves", "quarters"])
def test_overflowing_tiles_stay_two_phase(S, O, crop_stages, radius9, kind, w, h):
    """constant flows away from the truth (about (7, 4)): the counters are the model's, tile for tile and pair for pair"""
    fx, fy = FLOWS[kind][w, h]
    z = np.zeros((h, w))
    st = run(S, O, [flow_of(z + fx, z + fy, O)], [cut(crop_stages, 0, 0, w, h)], "%s (%d, %d), %dx%d" % (kind, fx, fy, w, h))
    assert st == COUNTERS[kind, w, h]
    if kind == "far":
        assert st[2] >= (w // 16) * (h // 16) and st[7] > 0          # every whole tile overflows
    if kind == "halves":
        assert st[6] > 0 and st[7] == 0
    if kind == "quarters":
        assert st[7] > 0


@pytest.mark.parametrize("w,h", SHAPES)
def test_real_flow_fits_one_list(S, O, crop_stages, upflow, radius9, w, h):
    pl, flows = case(O, crop_stages, upflow, "real", w, h)
    st = run(S, O, flows, [pl], "real, %dx%d" % (w, h))
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    assert st[0] + st[2] == tiles and st[0] > tiles // 2 or tiles == 1, st
    assert st[5] > 0 and st[1] == 0, st
    if (w, h) == (83, 61):
        assert st == (24, 0, 0, 0, 140172, 119370, 0, 0)             # the model's counters of the crop


@pytest.mark.parametrize("w,h", SHAPES)
def test_two_pair_batch_one_list_and_parts(S, O, crop_stages, upflow, radius9, w, h):
    """pair 0: the real flow; pair 1: the zero flow, whose tiles are drained in parts -- one launch; the counters add up"""
    pl, flows = case(O, crop_stages, upflow, "real", w, h)
    z = np.zeros((h, w))
    st = run(S, O, [flows[0], flow_of(z, z, O)], [pl, pl], "real + far, %dx%d" % (w, h))
    far = COUNTERS["far", w, h]
    assert st[6:] == far[6:] and st[2] >= far[2] and st[1] == 0, st


@pytest.mark.parametrize("w,h", SHAPES)
def test_flat_image_fills_every_quarter(S, O, crop_stages, upflow, radius9, w, h):
    """identical flat images: B = 0, nothing may be rejected, so a pixel keeps all 8 x 4 pairs: a whole tile has 8 192 survivors,
    a quarter exactly the 2 048 it can have at most"""
    pl, flows = case(O, crop_stages, upflow, "flat", w, h)
    st = run(S, O, flows, [pl], "flat, %dx%d" % (w, h))
    assert st[5] == 0 and st[1] == 0 and st[3] == 0, st
    # the numpy model's counters (tools/refine_pretest_model.py: tile_paths): every tile but the narrow ones at the right border needs quarters
    assert st == {(83, 61): (4, 0, 20, 0, 146072, 0, 0, 20), (33, 17): (4, 0, 2, 0, 12816, 0, 0, 2), (16, 16): (0, 0, 1, 0, 4888, 0, 0, 1)}[w, h]


@pytest.mark.parametrize("w,h", SHAPES)
def test_checker_blocks_take_the_weight_sum_fallback(S, O, crop_stages, upflow, radius9, w, h):
    """saturated 8x8 blocks: fallback (a) is decided before any list is written and stays"""
    pl, flows = case(O, crop_stages, upflow, "checker", w, h)
    st = run(S, O, flows, [pl], "checker, %dx%d" % (w, h))
    assert st[1] > 0, st


@pytest.mark.parametrize("w,h", SHAPES)
def test_unknown_pixels_in_overflowing_tiles(S, O, crop_stages, radius9, w, h):
    """the zero flow with holes, a tile without a known pixel among them: unknown lanes write no item and keep their place in the prefix"""
    rng = np.random.default_rng(11)
    fx, fy = np.zeros((h, w)), np.zeros((h, w))
    m = rng.random((h, w)) < 0.1
    fx[m] = 1e10
    fy[m] = 1e10
    if w > 16:
        fx[:16, 16 * ((w - 1) // 16):] = 1e10
        fy[:16, 16 * ((w - 1) // 16):] = 1e10
    fx[h // 2, 3] = 1e10                                              # one component alone marks the vector unknown
    st = run(S, O, [flow_of(fx, fy, O)], [cut(crop_stages, 0, 0, w, h)], "far with holes, %dx%d" % (w, h))
    # the numpy model's counters (tools/refine_pretest_model.py: tile_paths)
    assert st == {(83, 61): (3, 0, 20, 1, 142352, 57906, 16, 4), (33, 17): (3, 0, 2, 1, 14608, 4308, 1, 1), (16, 16): (0, 0, 1, 0, 6448, 1386, 1, 0)}[w, h]
