"""The two-phase random search (csrc/k_pm_search.hip, PRE): what its rejection rests on, on the CPU.

A guess is rejected without its exact cost iff  N (1 - eps) >= best (D_A + U)  (tools/search_pretest_model.py restates the kernel's
float32 arithmetic).  That is sound -- the reference's `cost < best` is false for every rejected guess -- because
  1. every cost term c_k (data term + census term) is >= 0,
  2. the weight of a sample never exceeds its source half: fast_exp(-(a + t)/s) <= fast_exp(-a/s) (1 + delta) for t >= 0,
  3. float sums of <= 100 non-negative terms are within 99 * 2^-24 relative of the real sums,
and eps covers (2) and (3) four times over.  (1) and (2) are checked exhaustively here, the implication itself against the oracle's
patch_dist on small fields of every kind the kernel meets."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import search_pretest_model as M  # noqa: E402

# Measured worst case of fact 2 over all 598 x 598 (a, t) pairs of squared texel distances: fast_exp never exceeds its value at the
# smaller argument (the polynomial's error is below the spacing of the arguments' results; the final ldexp rounds monotonically).
DELTA = 0.0
# Float error of the comparison's two sides, relative: four sums of at most 100 non-negative terms (cost and weight sum of the exact
# evaluation, N and D_A + U of the pre-test), the exact evaluation's quotient, the addition D_A + U and the two products.
SUM_TERMS = 4 * 99 * 2.0 ** -24 + 4 * 2.0 ** -24


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def S():
    import eppm_amd
    eppm_amd.lib()
    from eppm_amd import stages
    return stages


def knobs(S):
    _, row0, rows, frm, eps, _ = S.probe_search_pretest(0, 256, 109)
    return M.centre_rows(row0, rows), frm, eps


def test_cost_terms_are_nonnegative(O):
    d = M.distances()
    assert len(d) == 598
    assert (M.data_term(d) >= 0).all()
    gs, cn = O.pm_luts(9)
    assert len(cn) == 9 and (cn >= 0).all() and (gs > 0).all()


def test_weight_never_exceeds_its_source_half(O):
    d = M.distances()
    a2 = (d * d).astype(np.float32)
    fa = M.fexp(-a2 / M.S2)
    fs = M.fexp(-(a2[:, None] + a2[None, :]).astype(np.float32) / M.S2)          # [a][t]
    over = fs.astype(np.float64) - fa[:, None]
    worst = float(np.where(over > 0, over / np.maximum(fa[:, None], np.float32(1e-45)), 0).max())
    print("worst delta", worst)
    assert worst <= DELTA


def test_eps_covers_the_error_terms_four_times(S):
    _, _, eps = knobs(S)
    assert eps > 0 and np.log2(eps) == round(np.log2(eps))
    assert eps >= 4 * (DELTA + SUM_TERMS), (eps, 4 * (DELTA + SUM_TERMS))


# ---- the implication on fields ---------------------------------------------------------------------------------------------------
W, H = 48, 20          # three blocks across, two down: partial blocks on both edges


def _planes(O, a, b):
    i1, i2 = O.rgb2rgba(a), O.rgb2rgba(b)
    return i1, i2, O.census(i1), O.census(i2)


@functools.lru_cache(None)
def planes(kind):
    from oracle import oracle as O
    from eppm_amd import synth
    if kind == "textured":
        a, b, _, _ = synth.make_pair(H, W, seed=7, max_flow=3.0)
    elif kind == "flat":
        a = np.full((H, W, 3), 77, np.uint8)
        b = a.copy()
    else:          # saturated blocks: black / white 6x6 squares, shifted by (2, 1) in image 2 -- weights across an edge underflow
        ys, xs = np.mgrid[0:H, 0:W]
        a = np.repeat((((ys // 6 + xs // 6) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
        b = np.roll(a, (1, 2), (0, 1))
    return _planes(O, np.ascontiguousarray(a), np.ascontiguousarray(b))


@functools.lru_cache(None)
def field(kind, iters):
    from oracle import oracle as O
    nnf, cost = O.patchmatch(*planes(kind), iters_done=iters)
    return nnf, cost


def guesses(nnf, seed):
    """per pixel: six guesses drawn in the reference's windows, the eight neighbours of the match and the match itself -> (px, py, gx, gy)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    bx, by = nnf["x"].astype(np.int64), nnf["y"].astype(np.int64)
    gx, gy = [], []
    for mag in M.search_windows():
        x0, x1 = np.maximum(bx - mag, 0), np.minimum(bx + mag + 1, W + 1)
        y0, y1 = np.maximum(by - mag, 0), np.minimum(by + mag + 1, H + 1)
        gx.append(x0 + rng.integers(0, 1 << 30, bx.shape) % (x1 - x0))
        gy.append(y0 + rng.integers(0, 1 << 30, by.shape) % (y1 - y0))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            gx.append(np.clip(bx + dx, 0, W))
            gy.append(np.clip(by + dy, 0, H))
    n = len(gx)
    return (np.tile(xs, (n, 1, 1)).reshape(-1), np.tile(ys, (n, 1, 1)).reshape(-1), np.stack(gx).reshape(-1), np.stack(gy).reshape(-1))


def check_implication(O, S, kind, nnf, cost, seed):
    """every guess the pre-test rejects is one the reference does not accept; returns (rejected, total, survivors that tie)"""
    rows_a, _, eps = knobs(S)
    P = planes(kind)
    px, py, gx, gy = guesses(nnf, seed)
    N, D = M.centre_sums(*P, px, py, gx, gy, rows_a)
    U = M.rest_weight(P[0], rows_a)
    best = cost[py, px]
    rej = M.rejects(N, D, U[py, px], best, eps)
    for k in np.flatnonzero(rej):
        exact = O.patch_dist(*P, int(px[k]), int(py[k]), int(gx[k]), int(gy[k]))
        assert not exact < best[k], (kind, int(px[k]), int(py[k]), int(gx[k]), int(gy[k]), exact, float(best[k]))
    return int(rej.sum()), len(rej), rej, best


@pytest.mark.parametrize("iters", [0, 3, 10])
def test_rejected_guesses_are_not_accepted_textured(O, S, iters):
    nnf, cost = field("textured", iters)
    nrej, n, _, _ = check_implication(O, S, "textured", nnf, cost, 100 + iters)
    print(f"iterations {iters}: rejected {nrej} of {n}")
    if iters == 10:
        assert 2 * nrej >= n          # a converged field: a pre-test that silently rejects nothing fails here


def test_rejected_guesses_are_not_accepted_flat(O, S):
    """every cost ties: whatever is rejected the reference rejects too, and a tie with a positive cost survives to its exact evaluation"""
    nnf, cost = field("flat", 10)
    _, _, rej, best = check_implication(O, S, "flat", nnf, cost, 5)
    assert not rej[best > 0].any()


def test_rejected_guesses_are_not_accepted_saturated_blocks(O, S):
    for iters in (0, 10):
        nnf, cost = field("saturated", iters)
        check_implication(O, S, "saturated", nnf, cost, 9 + iters)


def test_a_stored_cost_of_zero_rejects_every_guess(O, S):
    """cost < 0 is never true: the reference accepts nothing at such a pixel, and the pre-test rejects everything there"""
    nnf, cost = field("textured", 3)
    cost = cost.copy()
    cost[::3, ::5] = 0.0
    _, _, rej, best = check_implication(O, S, "textured", nnf, cost, 77)
    assert rej[best == 0].all()


# ---- the decision ----------------------------------------------------------------------------------------------------------------
SHAPES = [(256, 109, 2, 1), (256, 109, 2, 8), (480, 270, 2, 1), (960, 540, 2, 1), (48, 20, 1, 1), (48, 20, 2, 64), (16, 16, 1, 1)]


def test_decision_below_the_threshold_is_the_old_form(S):
    _, frm, _ = knobs(S)
    for w, h, problems, npairs in SHAPES:
        for it in range(0, max(frm, 0)):
            assert not S.probe_search_pretest(it, w, h, 9, problems, npairs)[0], (it, w, h)
    if frm >= 0:
        assert S.probe_search_pretest(frm, 256, 109, 9, 2, 8)[0]          # the flagship's launch, from the threshold on


def test_decision_never_for_eighth_blocks_radius_17_or_the_gathering_form(S):
    for w, h, problems, npairs in SHAPES:
        for it in (0, 3, 9, 1000):
            pre = S.probe_search_pretest(it, w, h, 9, problems, npairs)
            if S.probe_dispatch("search", w, h, 9, problems, npairs, 1)[0] == 2:
                assert not pre[0] and not pre[5], (it, w, h, problems, npairs)
            for r in (17, 4, 12):          # radius 17, and radii that only the gathering kernel (RT = 0) serves
                pre = S.probe_search_pretest(it, w, h, r, problems, npairs)
                assert not pre[0] and not pre[5], (it, w, h, r)
