"""The two-phase window refine's part loop (csrc/k_c2f_refine.hip: k_c2f_refine_win<9>) on the CPU.

A tile whose survivors exceed its list is no longer sent to the one-phase loop: the kernel drains the survivors of half of the tile's pixels
(tile rows 0-7, then 8-15) through the list, or of a quarter (4 rows: one wave per pass group) if a half does not fit.  The costs lower the
same per-pixel keys whichever way the survivors are grouped, so the selection cannot depend on the split -- which is what
tools/refine_pretest_model.py: drain_in_parts restates and this file checks, together with the split the kernel's counters must report
for the flows of tests/test_refine_parts_gpu.py (COUNTERS: the kernel is held to these numbers, the model is held to them here).

Not here: the issue's bounding weight for the pre-test (an approximate weight with a proven two-sided bound) is not built, so there is no
exhaustive weight check; the pre-test's rule, eps and rejection rate are those of tests/test_refine_pretest_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import refine_pretest_model as RM  # noqa: E402

R = 9
CAP = 2688             # items of a tile's survivor list (asserted against the library below)
# Constant flows on the cut of the crop whose true flow is about (7, 4), by what they make of the survivor lists, and per shape what
# RM.tile_paths(..., parts=True) counts: tiles two-phase with one list, weight sum too small, more survivors than one list, other, pairs
# tested, pairs rejected, tiles drained in halves, in quarters.  "far": every tile with enough pixels overflows, both splits occur;
# "halves": no tile needs quarters; "quarters": at 16x16 and 33x17 a tile that needs them.
FLOWS = {
    "far": {(83, 61): (0, 0), (33, 17): (0, 0), (16, 16): (0, 0)},
    "halves": {(83, 61): (5, 4), (33, 17): (5, 4), (16, 16): (4, 0)},
    "quarters": {(83, 61): (3, -2), (33, 17): (3, -2), (16, 16): (3, -2)},
}
COUNTERS = {
    ("far", 83, 61): (4, 0, 20, 0, 158576, 65085, 11, 9),
    ("far", 33, 17): (4, 0, 2, 0, 16768, 5000, 1, 1),
    ("far", 16, 16): (0, 0, 1, 0, 7440, 1571, 0, 1),
    ("halves", 83, 61): (19, 0, 5, 0, 141728, 104037, 5, 0),
    ("halves", 33, 17): (4, 0, 2, 0, 11480, 5362, 2, 0),
    ("halves", 16, 16): (0, 0, 1, 0, 5792, 1568, 1, 0),
    ("quarters", 83, 61): (6, 0, 18, 0, 150480, 71878, 14, 4),
    ("quarters", 33, 17): (4, 0, 2, 0, 14216, 5922, 1, 1),
    ("quarters", 16, 16): (0, 0, 1, 0, 5712, 1410, 0, 1),
}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def knobs():
    import eppm_amd
    eppm_amd.lib()
    from eppm_amd import stages
    _, row0, rows, cap, eps, dmin, rhsmin = stages.probe_c2f_pretest(R)
    assert cap == CAP
    return list(range(row0, row0 + rows)), cap, eps, dmin, rhsmin


def const_case(O, crop_stages, w, h, fx, fy):
    planes = tuple(np.ascontiguousarray(crop_stages[k][:h, :w]) for k in ("img1_L0", "img2_L0", "cen1_L0", "cen2_L0"))
    f = np.zeros((h, w), O.float2)
    f["x"], f["y"] = np.float32(fx), np.float32(fy)
    return planes, f


@pytest.fixture(scope="module")
def far_crop(O, knobs, crop_stages):
    """the 83x61 cut with the zero flow: 20 of its 24 tiles overflow one list, 11 fit in halves, 9 need quarters"""
    rows_a, cap, eps, dmin, rhsmin = knobs
    planes, flow = const_case(O, crop_stages, 83, 61, 0, 0)
    return planes, flow, RM.refine(planes, flow, rows_a, eps, dmin, rhsmin, R, exact_all=False)


def tiles_of(h, w):
    return [(slice(y0, min(y0 + 16, h)), slice(x0, min(x0 + 16, w))) for y0 in range(0, h, 16) for x0 in range(0, w, 16)]


def test_a_quarter_of_a_tile_always_fits_the_list(knobs):
    """64 pixels x 8 candidates other than k* x 4 passes: the split ends at quarters whatever the survivors"""
    assert 64 * 8 * 4 <= knobs[1]
    full = np.full((4, 4), 64 * 8)
    assert RM.tile_split(full, knobs[1]) == 4 and RM.tile_split(full // 8, knobs[1]) == 1
    halves = np.zeros((4, 4), int)
    halves[0], halves[3] = 8 * 64, 8 * 64 - 63            # 32 + 32 chunks: over one list (42 chunks), each half within it
    assert RM.tile_split(halves, knobs[1]) == 2
    halves[1, 0] = 10 * 64 + 1                            # the first half now needs 43 chunks: quarters, although the second half would fit
    assert RM.tile_split(halves, knobs[1]) == 4


def test_every_split_selects_what_one_list_selects(O, knobs, far_crop):
    """1, 2 and 4 parts (one list as long as it takes; halves; quarters) give every pixel of every tile the same candidate, the one
    oracle.c2f_refine keeps; the split the kernel would choose fits the list in every part"""
    cap = knobs[1]
    planes, flow, r = far_crop
    assert not r["small"].any()
    seen = {1: 0, 2: 0, 4: 0}
    for t in tiles_of(61, 83):
        split = RM.tile_split(RM.quarter_survivors(r, t), cap)
        seen[split] += 1
        one, items = RM.drain_in_parts(r, t, 1)
        assert (items <= cap) == (split == 1)
        for nparts in (2, 4):
            got, _ = RM.drain_in_parts(r, t, nparts, cap if nparts >= split else None)
            assert (got == one).all(), (t, nparts)
        known = r["known"][t]
        assert (one[known] == r["best"][t][known]).all()
    print("tiles drained in 1 / 2 / 4 parts:", seen)
    assert seen[2] > 0 and seen[4] > 0
    want = O.c2f_refine(flow, *planes, O.default_params(patch_r=R))
    fx, fy = RM.flow_of_best(r)
    assert (fx.view(np.uint32) == want["x"].view(np.uint32)).all() and (fy.view(np.uint32) == want["y"].view(np.uint32)).all()


def test_the_model_counts_what_the_gpu_test_expects_far_crop(knobs, far_crop):
    assert RM.tile_paths(far_crop[2], 10 ** 6, 10 ** 6, knobs[1], parts=True) == COUNTERS["far", 83, 61]


@pytest.mark.parametrize("w,h", [(33, 17), (16, 16)])
@pytest.mark.parametrize("kind", ["far", "halves", "quarters"])
def test_the_model_counts_what_the_gpu_test_expects(O, knobs, crop_stages, kind, w, h):
    """(the two other 83x61 lines of COUNTERS come from the same call; it takes a quarter of a minute each there)"""
    rows_a, cap, eps, dmin, rhsmin = knobs
    planes, flow = const_case(O, crop_stages, w, h, *FLOWS[kind][w, h])
    r = RM.refine(planes, flow, rows_a, eps, dmin, rhsmin, R, exact_all=False)
    got = RM.tile_paths(r, 10 ** 6, 10 ** 6, cap, parts=True)
    assert got == COUNTERS[kind, w, h]
    assert got[:6] == RM.tile_paths(r, 10 ** 6, 10 ** 6, cap)          # the six counters of before: the same tiles in the third
