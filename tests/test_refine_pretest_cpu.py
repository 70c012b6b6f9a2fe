"""The two-phase window refine (csrc/k_c2f_refine.hip: k_c2f_refine_win<9>): what its rejection rests on, on the CPU.

A (candidate, pass) other than k*'s is left unevaluated iff  N (1 - eps) >= B (D_A + U)  and the right-hand side is at least 2^-100
(tools/refine_pretest_model.py restates the kernel's float32 arithmetic).  That must imply that its exact cost is STRICTLY above B, the
exact cost of k* -- strictly, because a tie with a smaller candidate index would win the reference's selection.  The facts behind it are
section 3.7's (cost terms >= 0, a weight never exceeds its source half, float sums of <= 100 non-negative terms), checked exhaustively by
tests/test_search_pretest_cpu.py on the same patch term; here: eps against its error terms, and the implication itself and the selection
against the oracle on the fields the kernel meets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import refine_pretest_model as RM  # noqa: E402

R = 9
W, H = 83, 61          # the crop of tests/test_batch_forms_*: 6 x 4 tiles, ragged both ways
DELTA = 0.0            # test_search_pretest_cpu.py::test_weight_never_exceeds_its_source_half (the same weight, exhaustive)
# Float error of the comparison's two sides, relative.  Four sums of non-negative terms: cost and weight sum of the exact evaluation (99
# additions each), N (10 K - 1 additions over the K centre rows) and D_A + U (10 K - 1 for D_A, 99 - 10 K for U, 1 to join them: 99); one
# quotient per exact cost (B is the minimum of four of them: no further rounding), the two products of the comparison, and the product
# 1 - eps itself is exact.  The recount gives section 3.7's bound; it does not depend on K.
SUM_TERMS = (99 + 99 + 99 + 99) * 2.0 ** -24 + 3 * 2.0 ** -24


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
    return list(range(row0, row0 + rows)), cap, eps, dmin, rhsmin


def test_eps_covers_the_error_terms_four_times(knobs):
    rows_a, _, eps, dmin, rhsmin = knobs
    assert eps > 0 and np.log2(eps) == round(np.log2(eps))
    assert eps >= 4 * (DELTA + SUM_TERMS), (eps, 4 * (DELTA + SUM_TERMS))
    assert 1 <= len(rows_a) <= R + 1 and rows_a[0] == (R + 1 - len(rows_a)) // 2          # the centre rows
    # the guards keep every quantity of the comparison a normal float: weight sums above 2^-60, right-hand sides of at least 2^-100
    assert rhsmin >= 2.0 ** -126 * 2.0 ** 24 and dmin >= 2.0 ** -60


@pytest.fixture(scope="module")
def crop_case(crop_stages, O):
    """the 83x61 cut of the crop's level-0 planes and the flow its level-0 refine receives: the level-1 flow up-sampled and doubled"""
    st = crop_stages
    planes = tuple(np.ascontiguousarray(st[k][:H, :W]) for k in ("img1_L0", "img2_L0", "cen1_L0", "cen2_L0"))
    up = O.mul_scalar(O.resize_flow(st["flow_L1"], st["arrH"][0], st["arrW"][0]), 2.0)
    return planes, np.ascontiguousarray(up[:H, :W])


def synthetic(O, kind, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == "flat":
        a = np.full((h, w), 117, np.uint8)
        b = a
    else:          # saturated 8x8 checker blocks, image 2 shifted by (2, 1)
        a = ((((ys // 8) + (xs // 8)) & 1) * 255).astype(np.uint8)
        b = np.roll(a, (1, 2), (0, 1))
    i1, i2 = (O.rgb2rgba(np.ascontiguousarray(np.repeat(v[:, :, None], 3, 2))) for v in (a, b))
    return i1, i2, O.census(i1), O.census(i2)


def const_flow(O, w, h, fx, fy):
    f = np.zeros((h, w), O.float2)
    f["x"], f["y"] = np.float32(fx), np.float32(fy)
    return f


def check_selection(O, planes, flow, r):
    """the model's selection over k* and the survivors is the oracle's refined flow"""
    want = O.c2f_refine(flow, *planes, O.default_params(patch_r=R))
    fx, fy = RM.flow_of_best(r)
    assert (fx.view(np.uint32) == want["x"].view(np.uint32)).all() and (fy.view(np.uint32) == want["y"].view(np.uint32)).all()


def test_rejected_pairs_cost_strictly_more_than_the_best_estimate_on_the_crop(O, knobs, crop_case):
    rows_a, cap, eps, dmin, rhsmin = knobs
    planes, flow = crop_case
    r = RM.refine(planes, flow, rows_a, eps, dmin, rhsmin, R, exact_all=True)
    assert not r["small"].any()
    rej, B = r["rej"], r["B"][:, :, None, None]
    assert not np.isnan(r["cost"][r["rej"]]).any()
    assert (r["cost"][rej] > np.broadcast_to(B, rej.shape)[rej]).all()     # every rejected pair: exact cost strictly above B
    check_selection(O, planes, flow, r)
    nrej, n = int(rej.sum()), int(r["tested"].sum())
    print(f"crop {W}x{H}: rejected {nrej} of {n} tested pairs ({nrej / n:.3f}); k* is the selected candidate at "
          f"{(r['kstar'] == r['best'])[r['known']].mean():.3f} of the pixels")
    assert 2 * nrej >= n                                                   # a pre-test that silently rejects nothing fails here
    # and the survivor lists of every tile fit: the crop runs in the two-phase form, not in its fallback
    paths = RM.tile_paths(r, 10 ** 6, 10 ** 6, cap)
    assert paths[0] == 24 and paths[1:4] == (0, 0, 0), paths


def test_flat_image_every_cost_ties_and_the_first_valid_candidate_wins(O, knobs):
    rows_a, _, eps, dmin, rhsmin = knobs
    w, h = 40, 24
    planes = synthetic(O, "flat", w, h)
    flow = const_flow(O, w, h, 4, 3)
    r = RM.refine(planes, flow, rows_a, eps, dmin, rhsmin, R, exact_all=True)
    assert not r["rej"][r["cost"] > 0].any()                               # nothing with a positive cost is rejected
    assert not (r["rej"] & (r["cost"] <= r["B"][:, :, None, None])).any()  # nor anything that ties with B
    first = np.argmax(r["valid"], 2)
    assert (r["best"][r["valid"].any(2)] == first[r["valid"].any(2)]).all()
    check_selection(O, planes, flow, r)


def test_saturated_checker_blocks_are_classified_for_the_fallback(O, knobs):
    """where a pixel's patch lies across saturated edges the centre-row weights underflow: such a tile must take the one-phase loop"""
    rows_a, cap, eps, dmin, rhsmin = knobs
    w, h = 40, 24
    planes = synthetic(O, "checker", w, h)
    r = RM.refine(planes, const_flow(O, w, h, 2, 1), rows_a, eps, dmin, rhsmin, R, exact_all=True)
    paths = RM.tile_paths(r, 10 ** 6, 10 ** 6, cap)
    print("checker tiles two-phase / small / full / other:", paths[:4])
    assert r["small"].any() and paths[1] >= 1
    # in the tiles that are not classified, the rule is sound as everywhere
    m = r["rej"] & ~r["small"][:, :, None, None] & ~np.isnan(r["cost"])
    assert (r["cost"][m] > np.broadcast_to(r["B"][:, :, None, None], m.shape)[m]).all()
