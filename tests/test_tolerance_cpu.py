"""The oracle's tolerance variants (oracle/eppm_oracle.c: orc_set_tol_variant) against a second restatement of the tolerance patch cost,
written in numpy float64 straight from DESIGN.md section 9.2 and independent of the C oracle.  The variants are the reference of the stage
parity tests of the tolerance kernels (tests/test_tolerance_stages_gpu.py), so they get a check of their own, as the exact oracle has in
test_oracle_cpu.py::test_patch_costs_against_a_second_restatement."""
import numpy as np
import pytest

from oracle import oracle as O

# the affine passes of the candidate refine (bao_pmflow_kernel.cu:319-332), as test_oracle_cpu.py states them
PLANE_COEFS = [None, (0.177, -0.011, -0.003, 0.301), (0.125, -0.357, 0.009, 0.308), (0.205, 0.370, 0.011, 0.296)]
POPCOUNT = np.array([bin(v).count("1") for v in range(256)])


def tol_tables64(R):
    """section 9.2's tables as REAL numbers (float64, no float32 rounding anywhere): gs, cn, td, ta and the exp2 constant c"""
    s = float(np.float32(0.1) * np.float32(0.1))                    # the float product the reference forms (LAMBDA_AD^2 = PM_SIG_R^2)
    k = np.arange(256, dtype=np.float64) / 255.0
    sig_s = 0.5 * R
    gs = np.exp(-(np.arange(R + 1, dtype=np.float64) ** 2) / (sig_s * sig_s))
    cn = -np.expm1(-(np.arange(9, dtype=np.float64) ** 2) / float(np.float32(0.3) * np.float32(8) * np.float32(0.3) * np.float32(8)))
    return gs, cn, -np.expm1(-(k * k) / s), np.exp(-(k * k) / s), np.log2(np.e) / (255.0 * 255.0 * s)


def tol_patch_cost64(img1, img2, c1, c2, x1, y1, x2, y2, R, form):
    """cost_sum / weight_sum of section 9.2 for arrays of (pixel, target) pairs, every operation in float64.
    form "pm": cost = td[k_d] + cn[hamming], weight = ta[k_a] ta[k_b] gs_j gs_i, the plain patch of bao_pmflow_kernel.cu:255-301.
    form "refine_exp2": the four affine passes of :334-513, weight = exp2(log2(gs_j gs_i) + 24 - c k_a^2 - c k_b^2), results below 2^-126
    vanish (the +24 is the common factor that cancels); the nested strict-< minimum of the four passes.
    form "refine_table": the four passes with the table weights."""
    h, w = img1.shape
    gs, cn, td, ta, c = tol_tables64(R)
    rgb1 = np.stack([img1["x"], img1["y"], img1["z"]], -1).astype(np.int64)
    rgb2 = np.stack([img2["x"], img2["y"], img2["z"]], -1).astype(np.int64)
    x1, y1, x2, y2 = (np.asarray(v, np.int64) for v in (x1, y1, x2, y2))

    def tex(rgb, x, y):                       # point sampling, clamp addressing
        return rgb[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]

    def cen(cc, x, y):
        return cc[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)

    def linf(a, b):
        return np.abs(a - b).max(-1)

    ctr1, ctr2 = tex(rgb1, x1, y1), tex(rgb2, x2, y2)
    f32 = np.float32
    uu, vv = (x2 - x1).astype(f32), (y2 - y1).astype(f32)
    costs = []
    for coef in (PLANE_COEFS if form != "pm" else [None]):
        cs, ws = np.zeros(len(x1)), np.zeros(len(x1))
        for i in range(-R, R + 1, 2):
            for j in range(-R, R + 1, 2):
                sx1, sy1 = x1 + j, y1 + i
                if form == "pm":
                    sx2, sy2 = x2 + j, y2 + i
                else:                          # the sample positions are integer decisions of float32 coordinate sums, formed left to right
                    cx1, cy1 = (x1 + j).astype(f32), (y1 + i).astype(f32)
                    if coef is None:
                        cx2, cy2 = cx1 + uu, cy1 + vv
                    else:
                        cx2 = ((cx1 + uu) + f32(j) * f32(coef[0])) + f32(i) * f32(coef[1])
                        cy2 = ((cy1 + vv) + f32(j) * f32(coef[2])) + f32(i) * f32(coef[3])
                    sx2, sy2 = np.floor(cx2).astype(np.int64), np.floor(cy2).astype(np.int64)
                p1, p2 = tex(rgb1, sx1, sy1), tex(rgb2, sx2, sy2)
                cost = td[linf(p1, p2)] + cn[POPCOUNT[cen(c1, sx1, sy1) ^ cen(c2, sx2, sy2)]]
                ka, kb = linf(ctr1, p1), linf(ctr2, p2)
                g = gs[abs(j)] * gs[abs(i)]
                if form == "refine_exp2":
                    wgt = np.exp2(np.log2(g) + 24.0 - c * ka * ka - c * kb * kb)
                    wgt = np.where(wgt < 2.0 ** -126, 0.0, wgt)
                else:
                    wgt = ta[ka] * ta[kb] * g
                cs += cost * wgt
                ws += wgt
        with np.errstate(invalid="ignore", divide="ignore"):
            costs.append(cs / ws)
    if form == "pm":
        return costs[0]
    m34 = np.where(costs[2] < costs[3], costs[2], costs[3])         # __min(c1, __min(c2, __min(c3, c4))) with __min(a, b) = a < b ? a : b
    m234 = np.where(costs[1] < m34, costs[1], m34)
    return np.where(costs[0] < m234, costs[0], m234)


def sample_pairs(rng, h, w, n):
    """(pixel, target) pairs: uniform pixels, targets up to 4 past every edge (clamp addressing), plus the corners"""
    x1, y1 = rng.integers(0, w, n), rng.integers(0, h, n)
    x2, y2 = rng.integers(-4, w + 4, n), rng.integers(-4, h + 4, n)
    fixed = np.array([(0, 0, w, h), (w - 1, h - 1, -3, -2), (5, 7, 5, 7), (0, h - 1, w + 3, -4), (w - 1, 0, -4, h + 3)])
    return (np.concatenate([fixed[:, k], v]) for k, v in enumerate((x1, y1, x2, y2)))


@pytest.mark.parametrize("R", [9, 17, 5])
@pytest.mark.parametrize("variant,form,planefit", [((7, 1), "pm", False), ((23, 2), "refine_exp2", True), ((7, 2), "refine_table", True)],
                         ids=["patchmatch_7_1", "refine_23_2", "refine_7_2"])
def test_tolerance_variants_against_a_second_restatement(crop_stages, R, variant, form, planefit):
    """orc_patch_dist under (7, 1) -- tables, fma, the chunked order -- and orc_patch_dist_planefit under (23, 2) -- the weight as one exp2
    of a summed argument with the +24 bias -- and (7, 2) against the float64 restatement above, at a few thousand (pixel, target) pairs
    of the crop's level planes, clamped targets included, radii 9, 17 and the generic 5.  Agreement within (n + 2) 2^-23 relative, n the
    sample count (R + 1)^2: the worst-case accumulation bound of n fused steps and one division (derived, not measured)."""
    st = crop_stages
    n = (R + 1) * (R + 1)
    bound = (n + 2) * 2.0 ** -23
    worst = 0.0
    for level, count, seed in ((1, 1200, 5), (0, 600, 6), (2, 400, 7)):
        i1, i2, c1, c2 = (st[f"{k}_L{level}"] for k in ("img1", "img2", "cen1", "cen2"))
        h, w = i1.shape
        x1, y1, x2, y2 = sample_pairs(np.random.default_rng([seed, R]), h, w, count)
        want = tol_patch_cost64(i1, i2, c1, c2, x1, y1, x2, y2, R, form)
        O.set_tol_variant(*variant)
        try:
            got = np.array([O.patch_dist(i1, i2, c1, c2, int(a), int(b), int(c), int(d), patch_r=R, planefit=planefit)
                            for a, b, c, d in zip(x1, y1, x2, y2)], np.float64)
        finally:
            O.set_tol_variant()
        assert np.isfinite(want).all() and np.isfinite(got).all()
        rel = np.abs(got - want) / np.abs(want)
        k = int(rel.argmax())
        worst = max(worst, float(rel.max()))
        assert rel.max() <= bound, (level, R, variant, (int(x1[k]), int(y1[k]), int(x2[k]), int(y2[k])), got[k], want[k], float(rel[k]), bound)
    print(f"R={R} {variant} {form}: largest relative deviation {worst:.3e} (bound {bound:.3e})")


def test_the_lockstep_oracle_is_back_after_a_variant(crop_stages):
    """orc_set_tol_variant() restores the exact arithmetic (the stage tests' children rely on the finally blocks above and theirs)."""
    st = crop_stages
    i1, i2, c1, c2 = st["img1_L1"], st["img2_L1"], st["cen1_L1"], st["cen2_L1"]
    before = np.float32(O.patch_dist(i1, i2, c1, c2, 20, 20, 23, 19))
    O.set_tol_variant(7, 1)
    try:
        mid = np.float32(O.patch_dist(i1, i2, c1, c2, 20, 20, 23, 19))
    finally:
        O.set_tol_variant()
    after = np.float32(O.patch_dist(i1, i2, c1, c2, 20, 20, 23, 19))
    assert before.view(np.uint32) == after.view(np.uint32) and mid.view(np.uint32) != before.view(np.uint32)


# ---------------------------------------------------------------- the refine cases of the GPU stage tests, checked on the CPU first
import ctypes as C  # noqa: E402
import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def _refine_outputs(variant):
    """the oracle's refine of every case of tol_stage_child.refine_cases() under a tolerance variant (computed once per variant)"""
    from tol_stage_child import refine_cases
    out = []
    O.set_tol_variant(*variant)
    try:
        for name, planes, flow, R in refine_cases():
            out.append(O.c2f_refine(flow, *planes, O.default_params(patch_r=R)))
    finally:
        O.set_tol_variant()
    return out


def _planefit_costs(planes, R, xs, ys, tx, ty):
    """orc_patch_dist_planefit at many (pixel, target) pairs under the variant the caller set (the planes and tables passed once)"""
    i1, i2, c1, c2 = (np.ascontiguousarray(p) for p in planes)
    h, w = i1.shape
    gs, cn = O.pm_luts(R)
    fn = O.lib().orc_patch_dist_planefit
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (i1, i2, c1, c2)]
    g, c = gs.ctypes.data_as(C.c_void_p), cn.ctypes.data_as(C.c_void_p)
    return np.array([fn(*ptr, w, h, R, g, c, int(p), int(q), int(r), int(s)) for p, q, r, s in zip(xs, ys, tx, ty)], np.float64)


def test_refine_cases_meet_the_cap_on_the_cpu():
    """The stage tests allow the tolerance library's refine to differ from the oracle variant (23, 2) at no more than 1e-4 of a case's
    pixels.  That is a condition on the INPUTS: two CPU readings of the same arithmetic class -- (23, 2), the weight as one exp2, against
    (7, 2), table weights -- must already stay under it on every case, or the case is replaced."""
    from tol_stage_child import REFINE_DIFFER_CAP, REFINE_TABLE_VARIANT, REFINE_VARIANT, differing, refine_cases
    a, b = _refine_outputs(REFINE_VARIANT), _refine_outputs(REFINE_TABLE_VARIANT)
    for (name, planes, flow, R), fa, fb in zip(refine_cases(), a, b):
        share = float(differing(fa, fb).mean())
        print(f"{name}: (23, 2) vs (7, 2) differ at {share:.2e} of {fa.size} pixels")
        assert share <= REFINE_DIFFER_CAP, (name, share)


def test_the_nan_cost_case_has_nan_costs_in_every_reading():
    """The NaN-cost case of the refine is there for 0/0 costs: at its masked pixels all nine candidates cost NaN under (23, 2), under
    (7, 2) and in the float64 restatement of the exp2 form, so the oracle keeps the centre candidate there; the other known pixels get finite costs."""
    from tol_stage_child import NAN_CASE, REFINE_TABLE_VARIANT, REFINE_VARIANT, assert_nan_candidates, differing, nan_cost_case, refine_cases
    planes, flow, mask = nan_cost_case()
    assert mask.sum() > 4000 and NAN_CASE in [c[0] for c in refine_cases()]
    for variant in (REFINE_VARIANT, REFINE_TABLE_VARIANT):
        O.set_tol_variant(*variant)
        try:
            assert_nan_candidates(planes, flow, mask)
            out = O.c2f_refine(flow, *planes, O.default_params())
        finally:
            O.set_tol_variant()
        assert not differing(out, flow)[mask].any()
    ys, xs = np.nonzero(mask)
    tx, ty = xs + flow["x"][ys, xs].astype(np.int64), ys + flow["y"][ys, xs].astype(np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            assert np.isnan(tol_patch_cost64(*planes, xs, ys, tx + dx, ty + dy, 9, "refine_exp2")).all()
    known = ~mask & ~(flow["x"] > 1e9)
    ys, xs = np.nonzero(known)
    tx, ty = xs + flow["x"][ys, xs].astype(np.int64), ys + flow["y"][ys, xs].astype(np.int64)
    assert np.isfinite(tol_patch_cost64(*planes, xs, ys, tx, ty, 9, "refine_exp2")).all()


def test_refine_tie_margin_covers_four_times_the_float32_deviation():
    """The margin inside which the stage tests call two refine candidates tied is 4 x the largest relative deviation of the oracle
    variant's float32 cost from the float64 evaluation of section 9.2's formula, at the oracle's own chosen target of EVERY known pixel of
    every case (a cost that is NaN must be NaN in both; a relative deviation needs a cost above 0)."""
    from tol_stage_child import REFINE_TIE_MARGIN, REFINE_VARIANT, refine_cases
    outs = _refine_outputs(REFINE_VARIANT)
    worst = {}
    for (name, planes, flow, R), f in zip(refine_cases(), outs):
        known = ~((flow["x"] > 1e9) | (flow["y"] > 1e9))
        ys, xs = np.nonzero(known)
        tx, ty = xs + f["x"][ys, xs].astype(np.int64), ys + f["y"][ys, xs].astype(np.int64)
        want = tol_patch_cost64(*planes, xs, ys, tx, ty, R, "refine_exp2")
        O.set_tol_variant(*REFINE_VARIANT)
        try:
            got = _planefit_costs(planes, R, xs, ys, tx, ty)
        finally:
            O.set_tol_variant()
        assert np.array_equal(np.isnan(want), np.isnan(got)), name
        ok = np.isfinite(want) & np.isfinite(got) & (want > 0)
        if ok.any():
            dev = float((np.abs(got[ok] - want[ok]) / want[ok]).max())
            print(f"{name}: {int(ok.sum())} targets, largest relative deviation {dev:.3e}")
            worst[R] = max(worst.get(R, 0.0), dev)
    print("largest relative deviation of the float32 oracle variant from float64, by radius:", worst)
    dev = max(worst.values())
    assert 4 * dev <= REFINE_TIE_MARGIN <= 8 * dev, (dev, REFINE_TIE_MARGIN)
