"""Stage parity for every size-dependent kernel variant.

The launchers of the smoothing, the candidate refine, the random search and the classic sweep choose between kernels by the size of
the launch; the stage tests of test_parity_gpu.py run at 80x60 to 160x120 and reach one side of each choice.  Here every variant runs
on its own, at the smallest ragged shape on its side of the boundary -- taken from the library's own decision functions
(tests/test_variants_cpu.py, whose ledger asserts that no variant is left out) -- against the CPU oracle's stage function on the same
inputs, bit for bit.  The speculative sweeps' cooperative "few evaluations" paths are chosen by the data: they run on a converged field.
The case functions take the stage module and the oracle as arguments: tests/tol_stage_child.py runs the search and the sweep cases on
the tolerance library with them."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN, read_ppm
from test_parity_gpu import O, S, eq, refine_battery  # noqa: F401  (S, O: fixtures)
from test_variants_cpu import CONVERGED_MODES, DIRS, RADII, option, refine_cases, search_cases, smoothing_cases, sweep_cases

pytestmark = pytest.mark.gpu

UNKNOWN = np.float32(1e10)
THRESH = np.float32(1e9)             # kUnknownFlowThresh: a component ABOVE it marks the vector unknown (strict >)
BLF_R = 10                           # radius of the smoothing window


# ---- a. smoothing, both kernels ---------------------------------------------------------------------------------------------------------

def smoothing_inputs(w, h):
    """(img, flow): a low-contrast guide image with a few hard edges, and a smooth flow with unknown vectors planted where the two-pixel
    kernel's r = 100 trick and its last-row branch could go wrong"""
    from oracle import oracle as O
    rng = np.random.default_rng([w, h, 5])
    rgb = rng.integers(90, 110, (h, w, 3), dtype=np.uint8)            # range weights stay non-zero
    rgb[:, w // 3:w // 3 + 7] = 235                                    # hard edges: a bright band, a dark block, a one-pixel line
    rgb[h // 2:, w // 2:w // 2 + 300] = 12
    rgb[:, 2 * w // 3] = 0
    img = O.rgb2rgba(rgb)
    ys, xs = np.mgrid[0:h, 0:w]
    fx = (3.0 * np.sin(xs / 57.0) + 0.05 * ys).astype(np.float32)
    fy = (-2.0 * np.cos(xs / 91.0) + 0.03 * ys).astype(np.float32)
    m = rng.random((h, w))
    fx[m < 0.02] = UNKNOWN; fy[m < 0.02] = UNKNOWN                     # isolated unknown pixels among known ones
    fx[(m > 0.02) & (m < 0.03)] = np.float32(2e9)                      # only x above the threshold
    fy[(m > 0.03) & (m < 0.04)] = np.float32(3e9)                      # only y
    fx[(m > 0.04) & (m < 0.042)] = THRESH                              # exactly the threshold: a KNOWN vector (strict >)
    fy[(m > 0.042) & (m < 0.044)] = THRESH
    neg = (m > 0.044) & (m < 0.054)                                    # unknown vectors with a negative component: 0 * negative enters the sums
    fx[neg] = UNKNOWN; fy[neg] = np.float32(-5.5)
    neg = (m > 0.054) & (m < 0.064)
    fx[neg] = np.float32(-7.25); fy[neg] = UNKNOWN
    for x0 in (100, w // 2 + 50, w - 140):                             # rectangles larger than the 21x21 window, one reaching the last row
        fx[2:31, x0:x0 + 40] = UNKNOWN; fy[2:31, x0:x0 + 40] = UNKNOWN
        fx[h - 12:, x0 + 60:x0 + 100] = UNKNOWN; fy[h - 12:, x0 + 60:x0 + 100] = UNKNOWN
    fx[:2, ::3] = UNKNOWN; fy[:2, ::3] = UNKNOWN                       # the first and last two rows and columns
    fx[-2:, 1::3] = UNKNOWN; fy[-2:, 1::3] = UNKNOWN
    fx[::2, :2] = UNKNOWN; fy[::2, :2] = UNKNOWN
    fx[1::2, -2:] = UNKNOWN; fy[1::2, -2:] = UNKNOWN
    flow = np.zeros((h, w), O.float2)
    flow["x"], flow["y"] = fx, fy
    assert np.isfinite(fx).all() and np.isfinite(fy).all()
    return img, flow


def window_count(mask):
    """per pixel, how many pixels of its 21x21 window (inside the image) are set in mask"""
    h, w = mask.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = mask.astype(np.int64).cumsum(0).cumsum(1)
    ys, xs = np.mgrid[0:h, 0:w]
    y0, y1 = np.maximum(ys - BLF_R, 0), np.minimum(ys + BLF_R + 1, h)
    x0, x1 = np.maximum(xs - BLF_R, 0), np.minimum(xs + BLF_R + 1, w)
    return c[y1, x1] - c[y0, x1] - c[y1, x0] + c[y0, x0]


@pytest.mark.parametrize("name,w,h,ppl", smoothing_cases(), ids=[c[0] for c in smoothing_cases()])
def test_smoothing_both_kernels(S, O, name, w, h, ppl):
    """k_flow_blf<2> (two pixels per lane; odd height: the last row has no lower pixel; even height: it has) and k_flow_blf<1> one column
    narrower, on flows full of unknown vectors, == the oracle bit for bit"""
    img, flow = smoothing_inputs(w, h)
    want = O.flow_smoothing(flow, img)
    unknown = (flow["x"] > THRESH) | (flow["y"] > THRESH)
    assert not unknown[(flow["x"] == THRESH) & (flow["y"] <= THRESH)].any()
    known_taps, unknown_taps = window_count(~unknown), window_count(unknown)
    blind = known_taps == 0                              # the whole window unknown or outside the image: the oracle leaves the pixel as it was
    assert blind.any() and blind[h - 1].any()
    assert np.array_equal(want["x"][blind].view(np.uint32), flow["x"][blind].view(np.uint32))
    assert np.array_equal(want["y"][blind].view(np.uint32), flow["y"][blind].view(np.uint32))
    mixed = ~unknown & (unknown_taps > 0)                # known pixels that meet an unknown tap
    assert mixed.sum() >= 1000 and mixed[h - 1].any() and mixed[h - 2].any()
    eq(S.flow_smoothing(flow, img), want, f"smoothing {w}x{h} ({ppl} per lane)")


# ---- b. refine, split path --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,w,h,R,factor", refine_cases(), ids=[c[0] for c in refine_cases()])
def test_refine_split_path(S, O, crop_stages, name, w, h, R, factor):
    """k_c2f_refine_tiled<R, 3 | 4> + k_c2f_select<3 | 4>, which a context takes for every level under 256 tiles, given the adversarial
    flows of the window kernels' test: with "c2f_force_split" the stage launcher brings the scratch and splits by the library's decision"""
    st = crop_stages
    planes = tuple(np.ascontiguousarray(st[k][:h, :w]) for k in ("img1_L0", "img2_L0", "cen1_L0", "cen2_L0"))
    with option("c2f_force_split", 1, 0):
        refine_battery(S, O, planes, R, full=True, extras=(name == "R9_factor3_aligned" or name == "R17_factor4_aligned"))


def test_refine_has_no_split_at_other_radii(S, O, crop_stages):
    from test_variants_cpu import probe
    st = crop_stages
    planes = tuple(st[k] for k in ("img1_L0", "img2_L0", "cen1_L0", "cen2_L0"))
    h, w = planes[0].shape
    assert probe("refine", w, h, 5, 1, 0) == 0
    with option("c2f_force_split", 1, 0):
        refine_battery(S, O, planes, 5, full=False)              # (no window at this radius either: the battery without the spread cases)
        with option("c2f_no_split", 1, 0):                       # "c2f_no_split" keeps its meaning
            refine_battery(S, O, planes, 9, full=False)


# ---- c / d. PatchMatch planes and start fields -------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def _frames():
    return read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm"))


@functools.lru_cache(None)
def pm_planes(w, h):
    """(img1, img2, census1, census2) of size w x h: a region of the bundled pair where it fits, else noise and its shifted copy"""
    from oracle import oracle as O
    if w == 80 and h == 60:                                      # the level-1 planes of the crop
        from test_temporal_gpu import oracle_planes
        a, b = _frames()
        st = oracle_planes(a[180:300, 240:400].copy(), b[180:300, 240:400].copy())
        return tuple(st[f"{k}_L1"] for k in ("img1", "img2", "cen1", "cen2"))
    a, b = _frames()
    if h <= a.shape[0] and w <= a.shape[1]:
        y0, x0 = (a.shape[0] - h) // 2, (a.shape[1] - w) // 2
        a, b = a[y0:y0 + h, x0:x0 + w].copy(), b[y0:y0 + h, x0:x0 + w].copy()
    else:
        rng = np.random.default_rng([h, w])
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = np.roll(a, (1, -3), axis=(0, 1))
        b[::7] = rng.integers(0, 256, b[::7].shape, dtype=np.uint8)
    ra, rb = O.rgb2rgba(a), O.rgb2rgba(b)
    return ra, rb, O.census(ra), O.census(rb)


def start_field(kind, w, h):
    """"random": the field a PatchMatch run starts from; "arbitrary": what a caller of the stage launchers may hand over -- targets on the
    last row / column, one past them (the reference's inclusive random range), far outside the image, negative"""
    from oracle import oracle as O
    if kind == "random":
        return O.gen_rand_field(w, h)[0]
    rng = np.random.default_rng(77)
    nnf = np.zeros((h, w), O.short2)
    nnf["x"] = rng.integers(0, w + 1, (h, w))
    nnf["y"] = rng.integers(0, h + 1, (h, w))
    m = rng.random((h, w))
    nnf["x"][m < 0.05] = w; nnf["y"][(m > 0.05) & (m < 0.1)] = h               # one past the last column / row
    nnf["x"][(m > 0.1) & (m < 0.13)] = -7; nnf["y"][(m > 0.13) & (m < 0.16)] = h + 40      # outside: gather path
    nnf["x"][(m > 0.16) & (m < 0.18)] = w + 300
    return nnf


@functools.lru_cache(None)
def _start(kind, w, h, R, variant):
    """(nnf, cost) of a start field under the oracle (variant: the tolerance variant in force, part of the key)"""
    from oracle import oracle as O
    nnf = start_field(kind, w, h)
    return nnf, O.cost_field(nnf, *pm_planes(w, h), O.default_params(patch_r=R))


def run_search_case(S, O, case, variant=None):
    """one pm_random_search launch: NNF, cost and generator states == the oracle"""
    import eppm_amd
    name, side, w, h, R, table, kind, extra, rows = case
    params = dict(patch_r=R, **dict(extra))
    planes = pm_planes(w, h)
    S.set_params(eppm_amd.Params(**params))
    try:
        p, op = eppm_amd.Params(**params), O.default_params(**params)
        nnf, cost = _start(kind, w, h, R, variant)
        ostates = O.gen_rand_field(w, h, op.seed)[1]             # the generator where the field left it: a fresh object's position
        P = S.PlaneSet(*planes)
        rng = S.PmRng(w, h, p)
        eq(rng.block_states(), ostates, f"{name}: generator states before the search")
        with option("rand_table", 2 if table else 0, 1):
            gcost, gnnf = S.pm_random_search(rng, cost, nnf, P)
        wstates, wcost, wnnf = O.random_search(ostates, cost, nnf, *planes, op)
        assert (wnnf["x"] != nnf["x"]).mean() > 0.02, f"{name}: the search accepts guesses"
        eq(gnnf, wnnf, f"{name} ({rows} rows per workgroup): NNF")
        eq(gcost, wcost, f"{name} ({rows} rows per workgroup): cost")
        eq(rng.block_states(), wstates, f"{name}: generator states after the search")
    finally:
        S.set_params(None)


def run_sweep_case(S, O, case, variant=None):
    """the four directions of the classic sweep, each == the oracle"""
    import eppm_amd
    name, side, w, h, R, seg_len, kind, form = case
    params = dict(patch_r=R, seg_len=seg_len)
    planes = pm_planes(w, h)
    S.set_params(eppm_amd.Params(**params))
    try:
        op = O.default_params(**params)
        nnf, cost = _start(kind, w, h, R, variant)
        P = S.PlaneSet(*planes)
        ocost, onnf = cost, nnf
        with option("sweep_spec", 0, -1):
            for d in DIRS:
                cost, nnf = S.pm_seg_propagate(cost, nnf, P, d)
                ocost, onnf = O.seg_propagate_dir(ocost, onnf, *planes, d, op)
                eq(nnf, onnf, f"{name} {form} dir {d}: NNF")
                eq(cost, ocost, f"{name} {form} dir {d}: cost")
    finally:
        S.set_params(None)


@pytest.mark.parametrize("case", search_cases(), ids=[c[0] for c in search_cases()])
def test_search_quarter_and_eighth_block(S, O, case):
    """k_pm_random_search reading numbers drawn ahead in both workgroup shapes (ROWS = 4 / 2) and drawing while it searches, both radii"""
    run_search_case(S, O, case)


@pytest.mark.parametrize("case", sweep_cases(), ids=[c[0] for c in sweep_cases()])
def test_classic_sweep_lane_widths_tile_and_gather(S, O, case):
    """k_pm_sweep in the classic form: both lane widths at radius 9 (with and without the up-front fetch), radius 17, strips, and the
    segment lengths on both sides of the LDS tile's limit"""
    run_sweep_case(S, O, case)


# ---- e. speculative sweeps on a converged field ------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def converged_field(R):
    """the oracle's field on the level-1 crop planes after as many iterations as it takes for the NEXT iteration's sweeps to change fewer
    than 10 % of the pixels (at least 7): (nnf, cost, iterations)"""
    from oracle import oracle as O
    planes = pm_planes(80, 60)
    h, w = planes[0].shape
    op = O.default_params(patch_r=R)
    nnf, states = O.gen_rand_field(w, h, op.seed)
    cost = O.cost_field(nnf, *planes, op)
    for it in range(40):
        if it >= 7:
            c, n = cost, nnf
            for d in DIRS:
                c, n = O.seg_propagate_dir(c, n, *planes, d, op)
            if ((n["x"] != nnf["x"]) | (n["y"] != nnf["y"])).mean() < 0.10:
                return nnf, cost, it
        for d in DIRS:
            cost, nnf = O.seg_propagate_dir(cost, nnf, *planes, d, op)
        states, cost, nnf = O.random_search(states, cost, nnf, *planes, op)
    raise AssertionError("the oracle's field does not converge on these planes")


@pytest.mark.parametrize("mode", CONVERGED_MODES)
@pytest.mark.parametrize("R", RADII)
def test_sweeps_on_a_converged_field(S, O, R, mode):
    """the iteration after convergence, direction by direction: few candidates are accepted, so phase A takes its cooperative
    few-evaluations path (radius 17: EPPM_SPEC_COOP17_MAX) and phase B walks short lists"""
    import eppm_amd
    planes = pm_planes(80, 60)
    nnf, cost, its = converged_field(R)
    op = O.default_params(patch_r=R)
    ocost, onnf = cost, nnf
    S.set_params(eppm_amd.Params(patch_r=R))
    try:
        P = S.PlaneSet(*planes)
        with option("sweep_spec", mode, -1):
            for d in DIRS:
                cost, nnf = S.pm_seg_propagate(cost, nnf, P, d)
                ocost, onnf = O.seg_propagate_dir(ocost, onnf, *planes, d, op)
                eq(nnf, onnf, f"R={R} sweep_spec {mode} iteration {its + 1} dir {d}: NNF")
                eq(cost, ocost, f"R={R} sweep_spec {mode} iteration {its + 1} dir {d}: cost")
    finally:
        S.set_params(None)
    changed = ((onnf["x"] != converged_field(R)[0]["x"]) | (onnf["y"] != converged_field(R)[0]["y"])).mean()
    assert changed < 0.10, changed


@pytest.mark.parametrize("R", RADII)
def test_merged_sweeps_through_a_context(crop, R):
    """the merged form (one phase A for the four sweeps, k_pm_spec_all: radius 9's cooperative path EPPM_MERGED_COOP9_MAX) exists in
    contexts only: ten iterations on the crop with sweep_spec 3, whole flow == the oracle"""
    import eppm_amd
    from oracle import oracle as O
    a, b = crop
    h, w, _ = a.shape
    with option("sweep_spec", 3, -1):
        e = eppm_amd.EPPM(params=eppm_amd.Params(patch_r=R, num_iter=10))
        e.init(a, b, h, w)
        u, v = e.compute_flow()
        e.close()
    ou, ov = O.compute_flow(a, b, O.default_params(patch_r=R, num_iter=10))
    eq(u, ou, f"u R={R} merged sweeps"); eq(v, ov, f"v R={R} merged sweeps")
