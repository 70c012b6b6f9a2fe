"""Stage parity of the tolerance library's kernels: the GPU part of tests/test_tolerance_stages_gpu.py (not collected by pytest).

    python tests/tol_stage_child.py <library variant> <part> [argument ...]

One child process per test: the pytest process holds the exact test library, a process loads one library.  The child selects the
library named on its command line ("tol_test"), runs one part below and prints "PART OK" as its last line; the oracle side runs here
too, under the tolerance variant the part names, which is restored in a finally block.  The functions are also importable: the tie
invariant (part b) runs in the pytest process against the exact test library with the same code.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conftest  # noqa: E402,F401  (selects the exact test library; main() overrides it before anything is loaded)
from test_parity_gpu import eq  # noqa: E402
from test_configs_gpu import _fuzz_case  # noqa: E402
from test_temporal_gpu import oracle_planes, oracle_seeded_patchmatch, rng_states  # noqa: E402

PM_VARIANT = (7, 1)            # tables | fma | the chunked order, PatchMatch scope: every bit of every plane must agree
REFINE_VARIANT = (23, 2)       # ... | the weight as one exp2 of a summed argument, refine scope: decisions must agree up to near ties
REFINE_TABLE_VARIANT = (7, 2)  # the CPU reading of the same arithmetic class the cap is checked with (table weights instead of exp2)

# Relative margin inside which two candidates of the refine count as tied.  Derived on the CPU alone: the largest relative deviation of
# the oracle variant's float32 cost (orc_patch_dist_planefit under (23, 2)) from the float64 evaluation of section 9.2's refine formula
# (test_tolerance_cpu.py: tol_patch_cost64) at the oracle's chosen target of every known pixel of every case of refine_cases() is
# 6.00e-6 (on the noise images of the ragged cases; 1.0e-6 on the crop at R = 9, 1.7e-6 at R = 17); times 4 for v_exp_f32's 1 ulp and the
# different rounding of its argument: 2.4e-5.  The kernels take no part in it;
# test_tolerance_cpu.py::test_refine_tie_margin_covers_four_times_the_float32_deviation measures the deviation again and holds the
# constant between 4 and 8 times it.
REFINE_TIE_MARGIN = 2.4e-5
REFINE_DIFFER_CAP = 1e-4       # differing pixels per case: a condition on the inputs, met by (23, 2) against (7, 2) on the CPU


class tol_variant:
    """with tol_variant(mode, scope): the oracle computes with that tolerance variant; the lockstep oracle is back afterwards"""

    def __init__(self, mode, scope):
        self.v = (mode, scope)

    def __enter__(self):
        from oracle import oracle as O
        O.set_tol_variant(*self.v)

    def __exit__(self, *exc):
        from oracle import oracle as O
        O.set_tol_variant()
        return False


class option:
    """with option(name, value, default): a switch of include/eppm_test.h, back at its default afterwards"""

    def __init__(self, name, value, default):
        self.name, self.value, self.default = name.encode(), value, default

    def __enter__(self):
        import eppm_amd
        assert eppm_amd.lib().eppm_test_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        import eppm_amd
        eppm_amd.lib().eppm_test_set_option(self.name, self.default)
        return False


def stages(**params):
    """eppm_amd.stages with the launcher parameters set, the ABI's and the oracle's parameter structs"""
    import eppm_amd
    from eppm_amd import stages as S
    from oracle import oracle as O
    p = eppm_amd.Params(**params) if params else None
    S.set_params(p)
    return S, p, O.default_params(**params)


def crop_planes(level):
    a, b = conftest.read_ppm(os.path.join(conftest.GOLDEN, "frame10.ppm")), conftest.read_ppm(os.path.join(conftest.GOLDEN, "frame11.ppm"))
    st = oracle_planes(a[180:300, 240:400].copy(), b[180:300, 240:400].copy())
    return tuple(st[f"{k}_L{level}"] for k in ("img1", "img2", "cen1", "cen2"))


def rgba_planes(a, b):
    from oracle import oracle as O
    ra, rb = O.rgb2rgba(a), O.rgb2rgba(b)
    return ra, rb, O.census(ra), O.census(rb)


def flat_planes(seed, t=2):
    """the flat / saturated-block image kind of the fuzz generator (kind 2): costs tie by construction, weights underflow"""
    assert t % 4 == 2
    a, b, _ = _fuzz_case(seed, t)
    return rgba_planes(a, b)


def image_planes(name):
    rng = np.random.default_rng(len(name) * 1000 + sum(name.encode()))
    if name == "crop_L1":
        return crop_planes(1)
    if name == "crop_L2":
        return crop_planes(2)
    if name == "ragged":                         # no dimension a multiple of 16
        a = rng.integers(0, 256, (77, 101, 3), dtype=np.uint8)
        b = np.roll(a, (2, -3), axis=(0, 1))
        b[::9] = rng.integers(0, 256, b[::9].shape, dtype=np.uint8)
        return rgba_planes(a, b)
    if name == "strip":                          # 24 x 4000, whose third level is 6 x 1000: 100 segments per row, patches taller than the image
        a = rng.integers(0, 256, (24, 4000, 3), dtype=np.uint8)
        b = np.roll(a, (1, -3), axis=(0, 1))
        b[::7] = rng.integers(0, 256, b[::7].shape, dtype=np.uint8)
        st = oracle_planes(a, b)
        assert st["img1_L2"].shape == (6, 1000)
        return tuple(st[f"{k}_L2"] for k in ("img1", "img2", "cen1", "cen2"))
    if name.startswith("flat"):
        return flat_planes(int(name[4:]))
    raise ValueError(name)


SWEEP_FORMS = (1, 2, 3)        # sweep_spec: speculative with the work list, without it, and the merged form's switch; classic is the default


def same_bits_as_cost_field(S, P, cost, nnf, what):
    """section 9.2's tie invariant: a stored cost is the bits the cost field gives for the stored match, whichever kernel wrote it"""
    eq(cost, S.pm_cost_field(nnf, P), f"{what}: stored cost == cost field of the stored NNF")


def patchmatch_substages(planes, iters=2, oracle=True, invariant=False, what="", **params):
    """random field, cost field, iters x [four sweeps in every form + search] through the stage entry points; with `oracle` every plane
    against the oracle (the caller sets the variant), with `invariant` the tie invariant after every kernel"""
    from oracle import oracle as O
    S, p, op = stages(**params)
    try:
        i1, i2, c1, c2 = planes
        h, w = i1.shape
        P = S.PlaneSet(i1, i2, c1, c2)
        rng = S.PmRng(w, h, p)
        nnf = S.pm_gen_rand_field(rng)
        cost = S.pm_cost_field(nnf, P)
        if oracle:
            onnf, ostates = O.gen_rand_field(w, h, op.seed)
            eq(nnf, onnf, f"{what} random NNF")
            eq(rng.block_states(), ostates, f"{what} RNG states after the field")
            ocost = O.cost_field(onnf, i1, i2, c1, c2, op)
            eq(cost, ocost, f"{what} initial cost field")
        for it in range(iters):
            for d in range(4):
                spec = {}
                for mode in SWEEP_FORMS:
                    with option("sweep_spec", mode, -1):
                        spec[mode] = S.pm_seg_propagate(cost, nnf, P, d)
                cost, nnf = S.pm_seg_propagate(cost, nnf, P, d)
                forms = [("classic", cost, nnf)] + [(f"sweep_spec {m}", spec[m][0], spec[m][1]) for m in SWEEP_FORMS]
                if oracle:
                    ocost, onnf = O.seg_propagate_dir(ocost, onnf, i1, i2, c1, c2, d, op)
                for name, fc, fn in forms:
                    tag = f"{what} iter {it} dir {d} {name}"
                    if oracle:
                        eq(fn, onnf, f"{tag}: NNF"); eq(fc, ocost, f"{tag}: cost")
                    if invariant:
                        same_bits_as_cost_field(S, P, fc, fn, tag)
            cost, nnf = S.pm_random_search(rng, cost, nnf, P)
            tag = f"{what} iter {it} search"
            if oracle:
                ostates, ocost, onnf = O.random_search(ostates, ocost, onnf, i1, i2, c1, c2, op)
                eq(nnf, onnf, f"{tag}: NNF"); eq(cost, ocost, f"{tag}: cost"); eq(rng.block_states(), ostates, f"{tag}: RNG states")
            if invariant:
                same_bits_as_cost_field(S, P, cost, nnf, tag)
        if invariant:                             # the two optional propagation modes write costs too
            jc, jn = S.pm_jump_propagate(cost, nnf, P)
            same_bits_as_cost_field(S, P, jc, jn, f"{what} jump flood")
            pc, pn = S.pm_parallel_propagate(cost, nnf, P)
            same_bits_as_cost_field(S, P, pc, pn, f"{what} 4-neighbour")
    finally:
        S.set_params(None)


# ---- (a) PatchMatch stages against the oracle variant (7, 1), every bit ----

def part_substages(image, patch_r, seg_len):
    with tol_variant(*PM_VARIANT):
        patchmatch_substages(image_planes(image), iters=3 if image == "crop_L1" else 2, what=f"{image} R={patch_r} seg_len={seg_len}",
                             patch_r=int(patch_r), seg_len=int(seg_len))


def part_arbitrary_nnf():
    """targets on the last row / column, one past them and far outside: the clamp path of the parity planes and their replicate padding"""
    from oracle import oracle as O
    i1, i2, c1, c2 = crop_planes(1)
    h, w = i1.shape
    with tol_variant(*PM_VARIANT):
        for R in (9, 17, 5, 4):
            S, p, op = stages(patch_r=R)
            try:
                P = S.PlaneSet(i1, i2, c1, c2)
                rng = np.random.default_rng(77 + R)
                nnf = np.zeros((h, w), O.short2)
                nnf["x"] = rng.integers(0, w + 1, (h, w))
                nnf["y"] = rng.integers(0, h + 1, (h, w))
                m = rng.random((h, w))
                nnf["x"][m < 0.05] = w; nnf["y"][(m > 0.05) & (m < 0.1)] = h               # one past the last column / row
                nnf["x"][(m > 0.1) & (m < 0.13)] = -7; nnf["y"][(m > 0.13) & (m < 0.16)] = h + 40      # outside
                nnf["x"][(m > 0.16) & (m < 0.18)] = w + 300
                nnf["x"][(m > 0.18) & (m < 0.2)] = -1; nnf["y"][(m > 0.2) & (m < 0.22)] = -300
                cost = O.cost_field(nnf, i1, i2, c1, c2, op)
                eq(S.pm_cost_field(nnf, P), cost, f"R={R}: cost field of the arbitrary NNF")
                for mode in (-1,) + SWEEP_FORMS:
                    gc, gn, oc, on = cost, nnf, cost, nnf
                    with option("sweep_spec", mode, -1):
                        for d in range(4):
                            gc, gn = S.pm_seg_propagate(gc, gn, P, d)
                            oc, on = O.seg_propagate_dir(oc, on, i1, i2, c1, c2, d, op)
                            eq(gn, on, f"R={R} sweep_spec {mode} dir {d}: NNF"); eq(gc, oc, f"R={R} sweep_spec {mode} dir {d}: cost")
            finally:
                S.set_params(None)


def part_launcher():
    """baoCudaPatchMatch (ten iterations, every form of the sweeps the switch offers), the jump flood and the 4-neighbour propagation"""
    from oracle import oracle as O
    with tol_variant(*PM_VARIANT):
        for level, params in ((2, {}), (1, dict(num_iter=4)), (2, dict(patch_r=17, num_iter=3)), (2, dict(patch_r=5, num_iter=3, seg_len=7)),
                              (2, dict(propagation=1, num_iter=2)), (2, dict(propagation=2, num_iter=2))):
            i1, i2, c1, c2 = crop_planes(level)
            S, p, op = stages(**params)
            try:
                want = {}
                for name, pl in (("forward", (i1, i2, c1, c2)), ("backward", (i2, i1, c2, c1))):
                    want[name] = O.patchmatch(*pl, op)
                for mode in (-1, 0, 1, 2, 3):
                    with option("sweep_spec", mode, -1):
                        for name, pl in (("forward", (i1, i2, c1, c2)), ("backward", (i2, i1, c2, c1))):
                            nnf, cost = S.patchmatch(S.PlaneSet(*pl))
                            eq(nnf, want[name][0], f"baoCudaPatchMatch L{level} {params} sweep_spec {mode} {name}: NNF")
                            eq(cost, want[name][1], f"baoCudaPatchMatch L{level} {params} sweep_spec {mode} {name}: cost")
            finally:
                S.set_params(None)
        for R in (9, 17, 4):
            i1, i2, c1, c2 = crop_planes(1)
            h, w = i1.shape
            S, p, op = stages(patch_r=R)
            try:
                P = S.PlaneSet(i1, i2, c1, c2)
                onnf, _ = O.gen_rand_field(w, h)
                ocost = O.cost_field(onnf, i1, i2, c1, c2, op)
                cost, nnf, oc, on = ocost, onnf, ocost, onnf
                for rnd in range(2):                                # second round: many candidates equal the own match
                    cost, nnf = S.pm_jump_propagate(cost, nnf, P)
                    oc, on = O.jump_propagate(oc, on, i1, i2, c1, c2, op)
                    eq(nnf, on, f"R={R} jump flood {rnd}: NNF"); eq(cost, oc, f"R={R} jump flood {rnd}: cost")
                cost, nnf, oc, on = ocost, onnf, ocost, onnf
                for launch in range(3):
                    cost, nnf = S.pm_parallel_propagate(cost, nnf, P)
                    oc, on = O.parallel_propagate(oc, on, i1, i2, c1, c2, op)
                    eq(nnf, on, f"R={R} 4-neighbour {launch}: NNF"); eq(cost, oc, f"R={R} 4-neighbour {launch}: cost")
            finally:
                S.set_params(None)


def variant_cases(stage, patch_r, group):
    """the cases of tests/test_variants_gpu.py's parts c ("search") and d ("sweep") of one radius and group (the first word of their
    names), built from THIS library's dispatch probe"""
    import test_variants_cpu as V
    cases = {"search": V.search_cases, "sweep": V.sweep_cases}[stage]()
    return [c for c in cases if c[4] == int(patch_r) and c[0].split("_")[0] == group]


def part_variants(stage, patch_r, group):
    """every size-dependent variant of the search and the classic sweep (lanes per chain in this library: EPPM_LPC9 = 32 either way, the
    small launches fetch up front) against the oracle variant (7, 1), every bit"""
    import test_variants_gpu as G
    from eppm_amd import stages as S
    from oracle import oracle as O
    cases = variant_cases(stage, patch_r, group)
    assert cases
    run = {"search": G.run_search_case, "sweep": G.run_sweep_case}[stage]
    with tol_variant(*PM_VARIANT):
        for case in cases:
            run(S, O, case, variant=PM_VARIANT)
            print("case", case[0], case[-1], "OK")


# ---- (b) one cost, one bit pattern, whichever kernel wrote it (no oracle) ----

TIE_CASES = [("crop_L1", dict()), ("flat11", dict()), ("flat12", dict()), ("flat13", dict(patch_r=17)), ("flat14", dict(patch_r=5, seg_len=7)),
             ("flat15", dict(patch_r=4, seg_len=2)), ("flat16", dict(seg_len=25)), ("ragged", dict(patch_r=17, seg_len=3))]


def part_tie_invariant():
    for image, params in TIE_CASES:
        patchmatch_substages(image_planes(image), iters=2, oracle=False, invariant=True, what=f"{image} {params}", **params)


# ---- (c) candidate refine against the oracle variant (23, 2), decision level ----

RAGGED_STREAM = {(33, 250): 1}          # stream 0 of 250x33: 1 of 8250 pixels differs between the two CPU readings (1.21e-4)


def _flow(fx, fy):
    from oracle import oracle as O
    f = np.zeros(np.shape(fx), O.float2)
    f["x"], f["y"] = np.asarray(fx, np.float32), np.asarray(fy, np.float32)
    return f


NAN_CASE = "NaN costs (every weight of a patch vanishes) beside finite ones"


def nan_cost_case():
    """(planes, flow, mask): a pair on which `mask` pixels see 0/0 costs at ALL nine candidates and all four passes, in every reading of the
    tolerance arithmetic, beside pixels with ordinary finite costs in the same tiles.  What the exact test's black / white pair is for -- the
    nested __min and the strict < on NaN: such a pixel must keep its centre candidate -- without that pair's weights of 2^-144, which the
    refine's 2^24 bias and the tables' 2^48 bias put on different sides of the underflow.  Here a term is either a normal number in every
    reading or below 2^-150 in every reading:
      * right part of the source: columns alternate 0 / 255.  A patch samples at odd offsets, so every source sample differs from its
        centre by 255 (factor 2^-144);
      * right part of the target: black with 3x3 blobs, 32 apart, whose rows are red, green, blue.  The flow sends every pixel of the right
        part to the nearest blob centre, so all nine candidates are blob pixels; no pass samples the candidate's own row (the affine row
        offset is never 0), so every target sample differs from its centre by 255 too: 2^-288, zero under either bias;
      * left part: low-contrast texture in both images, small flows: finite costs;
      * a moat of unknown vectors (1e10) where a patch would mix the two parts or clamp at the border of the right part."""
    r = np.random.default_rng([21, 96, 160, 0])
    h, w = 96, 160
    tex = r.integers(100, 131, (h, 84, 3), dtype=np.uint8)
    a, b = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    a[:, :64] = tex[:, :64]
    a[:, 65::2] = 255
    b[:, :84] = np.roll(tex, (1, -1), axis=(0, 1))
    centres = np.array([(x, y) for x in (110, 142) for y in (20, 52, 84)])
    for cx, cy in centres:
        for k, col in enumerate(((255, 0, 0), (0, 255, 0), (0, 0, 255))):
            b[cy - 1 + k, cx - 1:cx + 2] = col
    fx, fy = r.integers(-2, 3, (h, w)).astype(np.float64), r.integers(-2, 3, (h, w)).astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    near = np.argmin((xs[..., None] - centres[:, 0]) ** 2 + (ys[..., None] - centres[:, 1]) ** 2, -1)
    right = xs >= 74
    fx[right], fy[right] = (centres[near, 0] - xs)[right], (centres[near, 1] - ys)[right]
    unknown = ((xs >= 54) & (xs < 74)) | (right & ((ys < 10) | (ys >= h - 10) | (xs >= w - 10)))
    fx[unknown] = 1e10; fy[unknown] = 1e10
    return rgba_planes(a, b), _flow(fx, fy), right & ~unknown


def assert_nan_candidates(planes, flow, mask, step=9):
    """the oracle (under the variant the caller set) sees NaN at all nine candidates of the masked pixels (every step-th one is evaluated)"""
    from oracle import oracle as O
    i1, i2, c1, c2 = planes
    ys, xs = np.nonzero(mask)
    n = 0
    for y, x in list(zip(ys, xs))[::step]:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                cost = O.patch_dist(i1, i2, c1, c2, int(x), int(y), int(x + flow["x"][y, x]) + dx, int(y + flow["y"][y, x]) + dy, planefit=True)
                assert np.isnan(cost), (x, y, dx, dy, cost)
                n += 1
    assert n >= 9 * 500
    return n


def refine_cases(span9=(32, 23), span17=(27, 19)):
    """(name, planes, flow, patch_r) of every refine case: those of test_c2f_refine_window_and_fallback_paths, the flat kind of the fuzz
    generator in a textured variant, and the noisy / unknown flows of test_c2f.  span9 / span17: the admissible centre spread of the
    library's window kernels (eppm_probe_c2f_window of the library under test; the defaults serve the CPU pre-check only, whose result
    does not depend on where the window ends)."""
    out = []
    P0 = crop_planes(0)
    h, w = P0[0].shape
    rng = np.random.default_rng(21)
    z = np.zeros((h, w))
    out.append(("constant flow", P0, _flow(z + 3.7, z - 2.2), 9))
    sx, sy = span9
    for dxs, dys in ((-1, -1), (0, 0), (1, 1), (0, -40), (-40, 0), (1, -40), (-40, 1)):
        fx, fy = z.copy(), z.copy()
        fx[:, 15::16] = sx - 15 + dxs
        fy[15::16, :] = sy - 15 + dys
        out.append(("centre spread = limit %+d (x), %+d (y)" % (dxs, dys), P0, _flow(fx, fy), 9))
        fx, fy = z.copy(), z.copy()
        fx[:, 0::16] = -(sx - 15 + dxs)
        fy[0::16, :] = -(sy - 15 + dys)
        out.append(("centre spread = limit %+d (x), %+d (y), negative side" % (dxs, dys), P0, _flow(fx, fy), 9))
    out.append(("random jumps", P0, _flow(rng.integers(-40, 41, (h, w)), rng.integers(-40, 41, (h, w))), 9))
    out.append(("targets far outside the image", P0, _flow(z - 300.0, z + 250.0), 9))
    fx, fy = rng.normal(0, 1.5, (h, w)) + 5, rng.normal(0, 1.5, (h, w)) - 4
    m = rng.random((h, w)) < 0.1
    fx[m] = 1e10; fy[m] = 1e10
    fx[:16, :16] = 1e10; fy[:16, :16] = 1e10                       # a tile without any known pixel
    out.append(("noisy flow with unknown vectors", P0, _flow(fx, fy), 9))
    # ragged sizes, each from a generator stream of its own.  RAGGED_STREAM names the stream: a case on which the two CPU readings of
    # the arithmetic ((23, 2) and (7, 2)) already differ above the cap is REPLACED by the next stream, never exempted
    # (test_tolerance_cpu.py::test_refine_cases_meet_the_cap_on_the_cpu)
    for (hh, ww) in ((77, 101), (33, 250), (130, 47), (17, 19)):
        r = np.random.default_rng([21, hh, ww, RAGGED_STREAM.get((hh, ww), 0)])
        a = r.integers(0, 256, (hh, ww, 3), dtype=np.uint8)
        b = np.roll(a, (2, -3), axis=(0, 1))
        out.append(("ragged %dx%d" % (ww, hh), rgba_planes(a, b), _flow(r.normal(0, 2.0, (hh, ww)) - 3, r.normal(0, 2.0, (hh, ww)) + 2), 9))
    # The NaN-cost pair of the exact test (black source, white target, a black patch) is REPLACED: its weights are exp(-100) = 2^-144,
    # which the refine's 2^24 bias puts on both sides of v_exp_f32's flush threshold 2^-126 and the table form's 2^48 bias keeps, so the two
    # CPU readings (23, 2) and (7, 2) disagree there by construction (23 of 6144 pixels, 3.7e-3: above the cap).  In its place two cases:
    # nan_cost_case() below, which keeps what the pair is for (0/0 costs), and the pair's layout with texture: a dark source (0..31), a
    # bright target (224..255) carrying a displaced dark patch -- saturated edges whose cross weights (2^-87 with the bias) stay normal
    # numbers in every reading.  Stream 0 of the latter differs at 1 of 6144 pixels between the two CPU readings (1.63e-4): stream 1.
    r = np.random.default_rng([21, 64, 96, 1])
    a = r.integers(0, 32, (64, 96, 3), dtype=np.uint8)
    b = r.integers(224, 256, (64, 96, 3), dtype=np.uint8)
    b[20:40, 30:60] = a[18:38, 33:63]
    out.append(("dark source, bright target with a dark patch", rgba_planes(a, b), _flow(r.integers(-2, 3, (64, 96)), r.integers(-2, 3, (64, 96))), 9))
    planes, flow, _ = nan_cost_case()
    out.append((NAN_CASE, planes, flow, 9))
    # the flat / saturated-block kind with texture: the blocks of _fuzz_case's kind 2 over a noise base, so that costs do not tie exactly
    for seed in (11, 12):
        fa, fb, _ = _fuzz_case(seed, 2)
        hh, ww, _ = fa.shape
        tex = rng.integers(0, 48, (hh, ww, 3))
        ta = np.clip(fa.astype(int) // 2 + 64 + tex, 0, 255).astype(np.uint8)
        tb = np.roll(ta, (2, -1), axis=(0, 1))
        out.append(("textured blocks of fuzz kind 2, seed %d" % seed, rgba_planes(ta, tb), _flow(rng.normal(0, 1.5, (hh, ww)) - 1, rng.normal(0, 1.5, (hh, ww)) + 2), 9))
    sx, sy = span17
    for dxs, dys in ((-1, -1), (0, 0), (1, 1), (0, -40), (-40, 0)):
        fx, fy = z.copy(), z.copy()
        fx[:, 15::16] = sx - 15 + dxs
        fy[15::16, :] = sy - 15 + dys
        out.append(("R=17 centre spread = limit %+d (x), %+d (y)" % (dxs, dys), P0, _flow(fx, fy), 17))
    out.append(("R=17 constant flow", P0, _flow(z + 2.0, z - 1.0), 17))
    out.append(("R=17 random jumps", P0, _flow(rng.integers(-30, 31, (h, w)), rng.integers(-30, 31, (h, w))), 17))
    out.append(("R=17 noisy flow", P0, _flow(rng.normal(0, 2.5, (h, w)) + 6, rng.normal(0, 2.5, (h, w)) - 3), 17))
    out.append(("R=5 noisy flow (generic radius)", P0, _flow(rng.normal(0, 2.5, (h, w)) - 2, rng.normal(0, 2.5, (h, w)) + 1), 5))
    return out


def differing(a, b):
    return (a["x"].view(np.uint32) != b["x"].view(np.uint32)) | (a["y"].view(np.uint32) != b["y"].view(np.uint32))


def check_refine_decisions(got, want, flow_in, planes, R, what):
    """the four rules of the refine: equal flows except at near ties of the oracle variant's own cost, never unknown / NaN on one side
    only, at most REFINE_DIFFER_CAP of the pixels.  The oracle must be under REFINE_VARIANT."""
    from oracle import oracle as O
    i1, i2, c1, c2 = planes
    h, w = i1.shape
    diff = differing(got, want)
    n = int(diff.sum())
    print(f"{what}: {n} of {diff.size} pixels differ")
    assert n <= REFINE_DIFFER_CAP * diff.size, f"{what}: {n} of {diff.size} pixels differ (cap {REFINE_DIFFER_CAP})"
    for y, x in zip(*np.nonzero(diff)):
        fin = flow_in[y, x]
        assert not (fin["x"] > 1e9 or fin["y"] > 1e9), f"{what}: unknown input vector at ({x}, {y}) not written as (0, 0) on one side"
        tg = (int(got["x"][y, x]) + x, int(got["y"][y, x]) + y)
        to = (int(want["x"][y, x]) + x, int(want["y"][y, x]) + y)
        assert got["x"][y, x] == np.floor(got["x"][y, x]) and got["y"][y, x] == np.floor(got["y"][y, x]), (what, x, y, got[y, x])
        assert abs(tg[0] - to[0]) <= 2 and abs(tg[1] - to[1]) <= 2, f"{what}: ({x}, {y}) chose {tg}, not a candidate of the centre the oracle chose {to} from"
        cg = np.float32(O.patch_dist(i1, i2, c1, c2, int(x), int(y), tg[0], tg[1], patch_r=R, planefit=True))
        co = np.float32(O.patch_dist(i1, i2, c1, c2, int(x), int(y), to[0], to[1], patch_r=R, planefit=True))
        assert np.isfinite(cg) and np.isfinite(co), f"{what}: ({x}, {y}) targets {tg} / {to} cost {cg} / {co}: NaN or unknown on one side only"
        rel = abs(float(cg) - float(co)) / max(abs(float(cg)), abs(float(co)), 1e-30)
        print(f"    ({x}, {y}): library {tg} cost {cg!r}, oracle variant {to} cost {co!r}, relative gap {rel:.3e}")
        assert rel <= REFINE_TIE_MARGIN, f"{what}: ({x}, {y}) chose {tg} (cost {cg}) where the oracle variant chose {to} (cost {co}): gap {rel:.3e} > {REFINE_TIE_MARGIN}"


def part_refine(which):
    """which = "r9" / "r17": the cases of one radius group through baoCudaBLFCostFilterRefine, with and without c2f_no_split"""
    import eppm_amd
    from oracle import oracle as O
    sx, sy = C.c_int(), C.c_int()
    spans = {}
    for R in (9, 17):
        assert eppm_amd.lib().eppm_probe_c2f_window(R, C.byref(sx), C.byref(sy)) == 0
        spans[R] = (sx.value, sy.value)
    print("admissible centre spread of the window kernels:", spans)
    cases = [c for c in refine_cases(spans[9], spans[17]) if (c[3] == 17) == (which == "r17")]
    with tol_variant(*REFINE_VARIANT):
        for name, planes, flow, R in cases:
            S, p, op = stages(patch_r=R)
            try:
                want = O.c2f_refine(flow, *planes, op)
                if name == NAN_CASE:
                    _, _, mask = nan_cost_case()
                    print(f"{name}: {assert_nan_candidates(planes, flow, mask)} candidates evaluated by the oracle variant, all NaN")
                    assert not differing(want, flow)[mask].any()           # a pixel whose candidates are all NaN keeps its centre
                for no_split in (0, 1):
                    with option("c2f_no_split", no_split, 0):
                        got = S.c2f_refine(flow, S.PlaneSet(*planes))
                    check_refine_decisions(got, want, flow, planes, R, f"{name} (c2f_no_split {no_split})")
            finally:
                S.set_params(None)


def part_refine_launcher():
    """baoCudaBLF_C2F (upsample x2, x2.0, candidate refine) from the crop's level-2 flow, as test_c2f runs it, and the refine on a flow
    with planted unknown vectors"""
    from oracle import oracle as O
    u, v, st = O.compute_flow(*[conftest.read_ppm(os.path.join(conftest.GOLDEN, f))[180:300, 240:400].copy() for f in ("frame10.ppm", "frame11.ppm")], dump=True)
    planes = tuple(st[f"{k}_L1"] for k in ("img1", "img2", "cen1", "cen2"))
    S, p, op = stages()
    try:
        with tol_variant(*REFINE_VARIANT):
            up = O.mul_scalar(O.resize_flow(st["flow_L2"], st["arrH"][1], st["arrW"][1], 2.0), 2.0)
            want = O.c2f_refine(up, *planes, op)
            for no_split in (0, 1):
                with option("c2f_no_split", no_split, 0):
                    got = S.blf_c2f(st["flow_L2"], S.PlaneSet(*planes), (st["arrH"][2], st["arrW"][2]))
                check_refine_decisions(got, want, up, planes, 9, f"baoCudaBLF_C2F level 1 (c2f_no_split {no_split})")
            fl = st["flow_L1"].copy()
            fl["x"][5:9, 7:30] = 1e10
            fl["y"][5:9, 7:30] = 1e10
            check_refine_decisions(S.c2f_refine(fl, S.PlaneSet(*planes)), O.c2f_refine(fl, *planes, op), fl, planes, 9, "refine with unknown flow")
    finally:
        S.set_params(None)


# ---- (d) whole PatchMatch in a context ----

def oracle_level_post(n1, c1, n2, c2, img, params):
    """what a context's nnf1 / cost1 / nnf2 / cost2 planes hold after eppm_compute: the exact integer stages on the PatchMatch planes"""
    from oracle import oracle as O
    n1, c1, n2, c2 = O.left_right_check(n1, c1, n2, c2)
    n1, c1 = O.outlier_removal(n1, c1)
    n1 = O.fill_holes(O.weighted_median(n1, img, params.wmf_iters, True), img)
    return n1, c1, n2, c2


def check_generator_states(e, rand_table, want, tag):
    """A context that draws while it searches ("rand_table" 0) keeps its generator where the oracle's is after the run.  One that reads
    numbers drawn ahead runs the search kernels without a state (k_pm_random_search<.., TAB>): the probe then shows where the drawing left
    the buffer, which no oracle stream position describes -- what holds there is that every run leaves the same states (the property the
    streaming mode relies on: a seeded run leaves what a cold run leaves)."""
    got = rng_states(e)
    if rand_table == 0:
        eq(got, want, f"{tag}: generator states after PatchMatch == the oracle's")
    else:
        e.compute_flow()
        eq(rng_states(e), got, f"{tag}: generator states after a second run == after the first")


def part_context(which):
    import eppm_amd
    from oracle import oracle as O
    a, b = conftest.read_ppm(os.path.join(conftest.GOLDEN, "frame10.ppm")), conftest.read_ppm(os.path.join(conftest.GOLDEN, "frame11.ppm"))
    region = {"crop": (slice(180, 300), slice(240, 400)), "odd": (slice(100, 223), slice(200, 357))}[which]          # 160 x 120, 157 x 123
    a, b = a[region].copy(), b[region].copy()
    h, w, _ = a.shape
    prm = O.default_params()
    st = oracle_planes(a, b)
    L = 2
    fw = tuple(st[f"{k}_L{L}"] for k in ("img1", "img2", "cen1", "cen2"))
    bw = (fw[1], fw[0], fw[3], fw[2])
    with tol_variant(*PM_VARIANT):
        (n1, c1), (n2, c2) = O.patchmatch(*fw, prm), O.patchmatch(*bw, prm)
        lh, lw = fw[0].shape
        nnf, states = O.gen_rand_field(lw, lh, prm.seed)           # the generator states a run leaves: the field, then num_iter searches
        cost = O.cost_field(nnf, *fw, prm)                         # (what a search draws does not depend on the planes it searches)
        for it in range(prm.num_iter):
            states, cost, nnf = O.random_search(states, cost, nnf, *fw, prm)
        want = oracle_level_post(n1, c1, n2, c2, fw[0], prm)
    for rand_table in (1, 0):
        for mode in (-1, 3):
            with option("rand_table", rand_table, 1), option("sweep_spec", mode, -1):
                e = eppm_amd.EPPM()
                e.init(a, b, h, w)
                e.compute_flow()
            tag = f"{which} {w}x{h} rand_table {rand_table} sweep_spec {mode}"
            for name, plane in zip(("nnf1", "cost1", "nnf2", "cost2"), want):
                eq(e.plane(name, L), plane, f"{tag}: {name} after eppm_compute")
            check_generator_states(e, rand_table, states, tag)
            e.close()


def part_context_seeded():
    """one seeded (temporal) pair: nnf_init* / cost_init* against select() over the variant's two cost fields, the planes after the seeded
    PatchMatch and the generator states"""
    import eppm_amd
    from eppm_amd import io
    from oracle import oracle as O
    from test_temporal_cpu import displacement, make_clip
    frames, _, _ = make_clip(192, 256, 77, n=3, max_flow=10.0)
    h, w, _ = frames[0].shape
    prm = O.default_params()
    L = 2
    with tol_variant(*PM_VARIANT):
        st0 = oracle_planes(frames[0], frames[1])
        fw = tuple(st0[f"{k}_L{L}"] for k in ("img1", "img2", "cen1", "cen2"))
        (n1, c1), (n2, c2) = O.patchmatch(*fw, prm), O.patchmatch(fw[1], fw[0], fw[3], fw[2], prm)
        cold = oracle_level_post(n1, c1, n2, c2, fw[0], prm)
        prior1, prior2 = io.temporal_prior(displacement(cold[0]), False), io.temporal_prior(displacement(n2), True)
        st = oracle_planes(frames[1], frames[2])
        (s1, sc1, init1, states1), (s2, sc2, init2, _) = oracle_seeded_patchmatch(st, prior1, prior2, prm)
        want = oracle_level_post(s1, sc1, s2, sc2, st[f"img1_L{L}"], prm)
    for rand_table in (1, 0):                                      # numbers drawn ahead (the default), and drawn while searching
        tag = f"rand_table {rand_table}"
        with option("rand_table", rand_table, 1):
            e = eppm_amd.EPPM()
            e.init(h, w)
        e.set_temporal(True)
        e.set_data(frames[0], frames[1])
        e.compute_flow()
        for name, plane in zip(("nnf1", "cost1", "nnf2", "cost2"), cold):
            eq(e.plane(name, L), plane, f"{tag} pair 0 (cold): {name}")
        cold_states = rng_states(e)
        e.push_frame(frames[2])
        e.compute_flow()
        eq(e.plane("prior1", L), prior1, f"{tag} prior1"); eq(e.plane("prior2", L), prior2, f"{tag} prior2")
        eq(e.plane("nnf_init1", L), init1[0], f"{tag} nnf_init1"); eq(e.plane("cost_init1", L), init1[1], f"{tag} cost_init1")
        eq(e.plane("nnf_init2", L), init2[0], f"{tag} nnf_init2"); eq(e.plane("cost_init2", L), init2[1], f"{tag} cost_init2")
        for name, plane in zip(("nnf1", "cost1", "nnf2", "cost2"), want):
            eq(e.plane(name, L), plane, f"{tag} seeded pair: {name} after eppm_compute")
        eq(rng_states(e), cold_states, f"{tag} seeded pair: generator states == those a cold run leaves")
        if rand_table == 0:                                        # (with the numbers drawn ahead the search kernels carry no state: check_generator_states)
            eq(cold_states, states1, f"{tag}: generator states == the oracle's after the run")
        e.close()


def part_probes():
    """what the test build of the tolerance library answers: its own window (50 rows), the texel unpacking against make_texel, the
    parity planes of a context, and EPPM_ERR_ARG with a message for the probe of a table its patch term does not have"""
    import eppm_amd
    from eppm_amd import stages as S
    L = eppm_amd.lib()
    assert b"tolerance arithmetic" in L.eppm_version()
    sx, sy = C.c_int(), C.c_int()
    assert L.eppm_probe_c2f_window(9, C.byref(sx), C.byref(sy)) == 0
    print("window spread R=9:", sx.value, sy.value)
    assert (sx.value, sy.value) == (32, 23)                 # EPPM_C2F_WIN_H = 50 here: 50 - 3 - 24 rows, two more than the exact library's 21
    words = np.concatenate([np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32), np.array([0, 0xffffffff, 0x80ff00ff], np.uint32)])
    y = np.zeros((len(words), 8), np.float32)
    assert L.eppm_probe_unpack_texel(words.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(words)) == 0
    eq(y[:, :4].copy(), y[:, 4:].copy(), "unpack_texel == make_texel")
    for ch in range(3):                                       # a channel is the INTEGER 4 * byte as a bit pattern
        assert np.array_equal(y[:, ch].view(np.uint32), ((words >> (8 * ch)) & 0xff) * 4)
    assert np.array_equal(y[:, 3].view(np.uint32), (words >> 24) * 0x01010101)
    # the shared float formulas still serve the stages the tolerance library takes unchanged (prefilter, smoothing, weighted median): their
    # probes work here and give the exact library's bits
    from oracle import oracle as O
    xs = -np.concatenate([np.linspace(0, 120, 2001), np.linspace(86, 106, 4001)]).astype(np.float32)
    eq(S.probe_fast_exp(xs), O.fast_exp(xs), "fast_exp in the tolerance build")
    xd = np.random.default_rng(1).random(20000, dtype=np.float32) * 2
    eq(S.probe_div_const(xd, 0), (xd / (np.float32(0.1) * np.float32(0.1))).astype(np.float32), "x/(.1f*.1f) in the tolerance build")
    eq(S.probe_div_const(xd, 1), (xd / (np.float32(0.02) * np.float32(0.02))).astype(np.float32), "x/(.02f*.02f) in the tolerance build")
    cb = np.arange(256, dtype=np.float32)
    eq(S.probe_div_const(cb, 2), (cb / np.float32(255)).astype(np.float32), "unorm8 in the tolerance build")
    x = np.linspace(0, 1, 16, dtype=np.float32)
    out = np.zeros_like(x)
    assert L.eppm_probe_delta_table(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(x), 0) == 1      # EPPM_ERR_ARG
    assert b"no delta table" in L.eppm_last_error()
    assert L.eppm_test_set_option(b"no_such_option", 1) == 1
    e = eppm_amd.EPPM()
    e.init(120, 160)
    pitch, pad, kernels = C.c_int(), C.c_int(), C.c_int()
    assert L.eppm_probe_pm_parity(e._ctx, C.byref(pitch), C.byref(pad), C.byref(kernels)) == 0
    print("parity planes of a 160x120 context: pitch", pitch.value, "pad", pad.value, "kernels", kernels.value)
    assert pitch.value > 0 and kernels.value != 0              # the tolerance kernels read them at both radii
    e.close()


PARTS = {"variants": part_variants, "substages": part_substages, "arbitrary_nnf": part_arbitrary_nnf, "launcher": part_launcher, "tie_invariant": part_tie_invariant,
         "refine": part_refine, "refine_launcher": part_refine_launcher, "context": part_context, "context_seeded": part_context_seeded,
         "probes": part_probes}


def main(argv):
    import eppm_amd
    from oracle import oracle as O
    eppm_amd.select_library(argv[1])
    O.set_num_threads(min(16, os.cpu_count() or 1))
    print("library:", eppm_amd.lib().eppm_version().decode())
    PARTS[argv[2]](*argv[3:])
    print("PART OK")


if __name__ == "__main__":
    main(sys.argv)
