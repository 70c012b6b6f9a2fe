"""Adversarial stage parity for the prepare kernels (k_prepare.hip) and the level-2 post kernels (k_post.hip).

Every comparison is the HIP stage against the CPU oracle's function on the same BUILT input, bit for bit: these stages are integer or
byte work, or share their float formulas by construction, so there is no tolerance to choose.  The inputs, the shapes and the ledger
that proves every planted situation occurs are in tests/test_stage_edges_cpu.py (no GPU needed); read the builders' docstrings there
for what each input holds.  Section 4 reads the planes a CONTEXT prepares -- the fused blur + decimation, the blur + resize with real
bilinear weights, the one batched census launch, the image-2-only form of a frame push -- level by level, where so far only a differing
final flow would have shown a wrong byte."""
import pytest

from test_parity_gpu import O, S, eq  # noqa: F401  (S, O: fixtures)
from test_stage_edges_cpu import (BLUR_INPUTS, BLUR_RADII, BLUR_SIGMAS, CTX_CASES, PREPARE_SHAPES, RESIZE_RATIOS, SHAPES, WMF_RUNS, blur_input,
                                  census_planes, ctx_image, ctx_oracle, ctx_raw, fill_fields, lr_inputs, nnf2flow_input, outlier_inputs,
                                  resize_cases, resize_flow_input, resize_rgba_input, sid, wmf_fields, wmf_oracle)

pytestmark = pytest.mark.gpu

cid = lambda c: "%dx%d_%dlevels" % c  # noqa: E731


# ---- 2. post kernels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_left_right_check(S, O, shape):
    """both NNFs and both costs: targets that round-trip, miss by one in x or in y only, lie on the last row / column, at x == w, y == h,
    at a negative x or y, far outside, at kInvalid; the second pass reads the first one's marks"""
    nnf1, c1, nnf2, c2 = lr_inputs(*shape)
    got, want = S.left_right_check(nnf1, c1, nnf2, c2), O.left_right_check(nnf1, c1, nnf2, c2)
    for g, w, what in zip(got, want, ("nnf1", "cost1", "nnf2", "cost2")):
        eq(g, w, f"left-right check {sid(shape)}: {what}")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_outlier_removal(S, O, shape):
    """votes of 83, 84 and 85 with a full and with a cut window, flow differences of exactly 2 and exactly 3, skipped and voted invalid
    pixels, relative flows that agree only through the int16 wrap"""
    nnf, cost = outlier_inputs(*shape)
    gn, gc = S.outlier_removal(nnf, cost)
    wn, wc = O.outlier_removal(nnf, cost)
    eq(gn, wn, f"outlier removal {sid(shape)}: NNF")
    eq(gc, wc, f"outlier removal {sid(shape)}: cost")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_weighted_median(S, O, shape):
    """every field of wmf_fields for 1, 2, 3 and 20 launches with occlusion only and for 1 and 3 launches with all pixels"""
    w, h = shape
    for name, (nnf, img) in wmf_fields(w, h).items():
        for iters, only_occ in WMF_RUNS:
            eq(S.weighted_median(nnf, img, iters, only_occ), wmf_oracle(w, h, name, iters, only_occ),
               f"weighted median {sid(shape)} '{name}' x{iters} {'occlusion only' if only_occ else 'all pixels'}")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_fill_holes(S, O, shape):
    """holes that see nothing in one to four directions, equal colour distances, a nearest valid pixel more than 64 pixels away, walks
    over one-negative pixels, results that wrap in int16"""
    for name, (nnf, img) in fill_fields(*shape).items():
        eq(S.fill_holes(nnf, img), O.fill_holes(nnf, img), f"fill holes {sid(shape)} '{name}'")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_nnf2flow(S, O, shape):
    """components at kInvalid, one above and one below it, -1, -32768, 0 and 32767, in x only, in y only and in both"""
    nnf = nnf2flow_input(*shape)
    eq(S.nnf2flow(nnf), O.nnf2flow(nnf), f"NNF -> flow {sid(shape)}")


# ---- 3. prepare kernels ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", PREPARE_SHAPES, ids=sid)
def test_blur(S, O, shape):
    """radii 0, 2 and 6; sigmas 0.5, 1, 2 and one whose off-centre weights all underflow; RGBA noise with a varying non-zero alpha,
    constant 0, constant 255 and a one-pixel checker"""
    for name in BLUR_INPUTS:
        img = blur_input(name, *shape)
        for radius in BLUR_RADII:
            for sigma in BLUR_SIGMAS:
                eq(S.gauss_filter_rgba(img, sigma, radius), O.gauss_filter_rgba(img, sigma, radius),
                   f"blur {sid(shape)} '{name}' sigma {sigma} radius {radius}")


def test_blur_rejects_radius_7(S):
    """the LDS tile and weight table hold a radius of 6: a larger one is an argument error, by contract"""
    from eppm_amd._lib import EppmError
    for radius in (7, -1):
        with pytest.raises(EppmError, match="radius"):
            S.gauss_filter_rgba(blur_input("random_rgba", 5, 3), 1.0, radius)


@pytest.mark.parametrize("shape", PREPARE_SHAPES, ids=sid)
def test_resize_rgba_and_flow(S, O, shape):
    """ratios 1/2, 1/4, 1, 2 (a negative source coordinate truncates toward zero) and the two inexact ratios a context forms below an
    odd-width level, to the output sizes pyr_init_dim gives; the flow resize on unknown vectors next to known and negative ones.  The
    cases whose output plane would be empty are no launch (test_stage_edges_cpu.test_resize_ledger names them)."""
    w, h = shape
    cases = [c for c in resize_cases() if (c[0], c[1]) == shape]
    assert cases and {c[2] for c in cases} <= {n for n, _ in RESIZE_RATIOS}
    img, flow = resize_rgba_input(w, h), resize_flow_input(w, h)
    for _, _, name, ratio, ow, oh in cases:
        eq(S.resize_rgba(img, oh, ow, ratio), O.resize_rgba(img, oh, ow, ratio), f"resize RGBA {sid(shape)} -> {ow}x{oh} ratio '{name}'")
        eq(S.resize_flow(flow, oh, ow, ratio), O.resize_flow(flow, oh, ow, ratio), f"resize flow {sid(shape)} -> {ow}x{oh} ratio '{name}'")


@pytest.mark.parametrize("shape", PREPARE_SHAPES, ids=sid)
def test_census(S, O, shape):
    """areas of one luminance, distinct colours of equal float luminance, extremes either side of the tile border and on the last row
    and column"""
    a, b = census_planes(*shape)
    c1, c2 = S.census_transform(a, b)
    eq(c1, O.census(a), f"census {sid(shape)} image 1")
    eq(c2, O.census(b), f"census {sid(shape)} image 2")


# ---- 4. the context's own prepare path, plane by plane ----------------------------------------------------------------------------------------

def ctx_planes(read, levels):
    return [{n: read(n, l) for n in ("img1", "img2", "census1", "census2")} for l in range(levels)]


def eq_planes(got, case, k1, k2, what, alpha=False):
    """the planes a context holds for images k1 (image 1) and k2 (image 2) == the oracle's, at every level, alpha byte included"""
    w, h, levels = case
    for l in range(levels):
        for n, k, idx in (("img1", k1, 0), ("img2", k2, 0), ("census1", k1, 1), ("census2", k2, 1)):
            if k is not None:
                eq(got[l][n], ctx_oracle(w, h, levels, k, alpha)[idx][l], f"{what} {cid(case)}: {n} level {l}")


@pytest.mark.parametrize("case", CTX_CASES, ids=cid)
def test_context_prepare_planes(S, O, case):
    """set_data from host images: launch_gauss_rgba2, the fused step or blur + resize per level (test_context_branch_ledger says which),
    one k_census_batch launch"""
    import eppm_amd
    w, h, levels = case
    e = eppm_amd.EPPM(params=eppm_amd.Params(levels=levels))
    e.init(ctx_image(w, h, 0), ctx_image(w, h, 1), h, w)
    assert e.level_dims() == list(zip(*O.pyr_init_dim(h, w, levels)))
    eq_planes(ctx_planes(e.plane, levels), case, 0, 1, "context")
    e.close()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=sid)
def test_context_rejects_the_degenerate_shapes(shape):
    """a context holds at least 4x4 pixels by contract (eppm_create): the three degenerate shapes of the stage tests are an argument
    error there, so section 4 runs its own sizes"""
    import eppm_amd
    from eppm_amd._lib import EppmError
    w, h = shape
    with pytest.raises(EppmError, match="out of range"):
        eppm_amd.EPPM().init(h, w)
    with pytest.raises(EppmError, match="out of range"):
        eppm_amd.EPPMBatch(h, w, 3)


@pytest.mark.parametrize("case", CTX_CASES, ids=cid)
def test_context_prepare_planes_device_entry(S, O, case):
    """eppm_set_images_device on pitched RGBA planes whose alpha is non-zero: the fourth channel travels through every level"""
    import eppm_amd
    w, h, levels = case
    d1, d2 = S.Dev(ctx_raw(w, h, 0, True), pitched=True), S.Dev(ctx_raw(w, h, 1, True), pitched=True)
    assert d1.pitch == d2.pitch
    e = eppm_amd.EPPM(params=eppm_amd.Params(levels=levels))
    e.init(h, w)
    e.set_data_device(d1.ptr.value, d2.ptr.value, d1.pitch)
    got = ctx_planes(e.plane, levels)
    eq_planes(got, case, 0, 1, "device entry", alpha=True)
    assert any((got[l]["img1"]["w"] != 0).any() for l in range(levels))
    # the device form of the frame push: image 2 alone is prepared, from a plane with alpha
    d3 = S.Dev(ctx_raw(w, h, 2, True), pitched=True)
    e.push_frame_device(d3.ptr.value, d3.pitch)
    eq_planes(ctx_planes(e.plane, levels), case, 1, 2, "device push", alpha=True)
    e.close()


@pytest.mark.parametrize("case", CTX_CASES, ids=cid)
def test_batch_context_prepare_planes(S, O, case):
    """three slots with different images: the blockIdx.z addressing of the prepare kernels and of the census job scan"""
    import eppm_amd
    w, h, levels = case
    b = eppm_amd.EPPMBatch(h, w, 3, params=eppm_amd.Params(levels=levels))
    pairs = ((0, 1), (2, 3), (1, 4))
    b.set_data([(ctx_image(w, h, k1), ctx_image(w, h, k2)) for k1, k2 in pairs])
    for slot, (k1, k2) in enumerate(pairs):
        eq_planes(ctx_planes(lambda n, l: b.plane(slot, n, l), levels), case, k1, k2, f"batch slot {slot}")
    # one more frame per slot: the image-2-only form over three slots
    nxt = (5, 0, 2)
    b.push_frames([ctx_image(w, h, k) for k in nxt])
    for slot, ((_, k2), k3) in enumerate(zip(pairs, nxt)):
        eq_planes(ctx_planes(lambda n, l: b.plane(slot, n, l), levels), case, k2, k3, f"batch slot {slot} after a push")
    b.close()


@pytest.mark.parametrize("case", CTX_CASES, ids=cid)
def test_frame_push_prepare_planes(S, O, case):
    """after each of two pushed frames every level of img1 / census1 is the previous pair's img2 / census2, and img2 / census2 are the
    oracle's planes of the new frame: the `only2` form of prepare"""
    import eppm_amd
    w, h, levels = case
    e = eppm_amd.EPPM(params=eppm_amd.Params(levels=levels))
    e.init(ctx_image(w, h, 0), ctx_image(w, h, 1), h, w)
    prev = ctx_planes(e.plane, levels)
    for k in (2, 3):
        e.push_frame(ctx_image(w, h, k))
        got = ctx_planes(e.plane, levels)
        for l in range(levels):
            eq(got[l]["img1"], prev[l]["img2"], f"push {cid(case)} frame {k}: img1 level {l} is the previous img2")
            eq(got[l]["census1"], prev[l]["census2"], f"push {cid(case)} frame {k}: census1 level {l} is the previous census2")
        eq_planes(got, case, k - 1, k, f"push frame {k}")
        prev = got
    e.close()
