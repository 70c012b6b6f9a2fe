"""The reference's stage launchers (driver .cpp:40-62) callable on numpy planes.

Every function uploads its inputs, calls the ``baoCuda*`` / ``eppm_pm_*`` entry point of the C ABI on
device buffers, and downloads the result: the parity tests read like calls of the reference's own
launchers.  Structured dtypes: uchar4 / short2 / float2 as in eppm_amd.api.
"""
import ctypes as C

import numpy as np

from ._lib import CParams, check, check_launcher, lib, probe_dispatch  # noqa: F401
from .api import float2, short2, uchar4


class Dev:
    """A pitched or linear device buffer holding a 2-D plane."""

    def __init__(self, arr=None, shape=None, dtype=None, pitched=False):
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            shape, dtype = arr.shape, arr.dtype
        self.h, self.w = shape
        self.dtype = np.dtype(dtype)
        row = self.w * self.dtype.itemsize
        self.ptr = C.c_void_p()
        if pitched:
            pitch = C.c_size_t()
            check(lib().eppm_malloc_pitched(C.byref(self.ptr), C.byref(pitch), row, self.h), "malloc_pitched")
            self.pitch = pitch.value
        else:
            check(lib().eppm_malloc_device(C.byref(self.ptr), row * self.h), "malloc")
            self.pitch = row
        if arr is not None:
            self.put(arr)

    def put(self, arr):
        arr = np.ascontiguousarray(arr, self.dtype)
        row = self.w * self.dtype.itemsize
        check(lib().eppm_memcpy2d_h2d(self.ptr, self.pitch, arr.ctypes.data, row, row, self.h), "h2d")

    def get(self):
        out = np.empty((self.h, self.w), self.dtype)
        row = self.w * self.dtype.itemsize
        check(lib().eppm_memcpy2d_d2h(out.ctypes.data, row, self.ptr, self.pitch, row, self.h), "d2h")
        return out

    def free(self):
        if self.ptr:
            lib().eppm_free_device(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def set_params(params=None):
    check(lib().eppm_set_launcher_params(C.byref(params) if params is not None else None), "eppm_set_launcher_params")


def probe_fast_exp(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    check(lib().eppm_probe_fast_exp(x.ctypes.data, y.ctypes.data, x.size), "probe_fast_exp")
    return y


def probe_div_const(x, which):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    check(lib().eppm_probe_div_const(x.ctypes.data, y.ctypes.data, x.size, which), "probe_div_const")
    return y


def probe_delta_table(d, which):
    """the table form of a range term at the distances d (test library; include/eppm_test.h)"""
    x = np.ascontiguousarray(d, np.float32)
    y = np.empty_like(x)
    check(lib().eppm_probe_delta_table(x.ctypes.data, y.ctypes.data, x.size, which), "probe_delta_table")
    return y


def gauss_filter_rgba(img, sigma, radius):
    h, w = img.shape
    a, b = Dev(img, pitched=True), Dev(shape=(h, w), dtype=uchar4, pitched=True)
    check(lib().eppm_gauss_filter_rgba(b.ptr, a.ptr, a.pitch, h, w, sigma, radius), "gauss")
    return b.get()


def resize_rgba(img, out_h, out_w, ratio):
    h, w = img.shape
    a, b = Dev(img, pitched=True), Dev(shape=(out_h, out_w), dtype=uchar4, pitched=True)
    check(lib().eppm_resize_rgba(b.ptr, b.pitch, out_h, out_w, a.ptr, a.pitch, h, w, ratio), "resize_rgba")
    return b.get()


def census_transform(img1, img2):
    """baoCudaCensusTransform"""
    h, w = img1.shape
    a, b = Dev(img1, pitched=True), Dev(img2, pitched=True)
    c1, c2 = Dev(shape=(h, w), dtype=np.uint8, pitched=True), Dev(shape=(h, w), dtype=np.uint8, pitched=True)
    lib().baoCudaCensusTransform(c1.ptr, c2.ptr, a.ptr, b.ptr, w, h, a.pitch, c1.pitch)
    check_launcher("baoCudaCensusTransform")
    return c1.get(), c2.get()


def prepare(raw1, raw2, dims):
    """baoCudaPatchMatchMultiscalePrepare on raw RGBA planes; dims = [(h,w)] per level.  Returns (imgs1, imgs2, cens1, cens2)."""
    n = len(dims)
    h, w = dims[0]
    r1, r2 = Dev(raw1, pitched=True), Dev(raw2, pitched=True)
    p1 = [Dev(shape=d, dtype=uchar4, pitched=True) for d in dims]
    p2 = [Dev(shape=d, dtype=uchar4, pitched=True) for d in dims]
    t1 = [Dev(shape=d, dtype=uchar4, pitched=True) for d in dims]
    t2 = [Dev(shape=d, dtype=uchar4, pitched=True) for d in dims]
    c1 = [Dev(shape=d, dtype=np.uint8, pitched=True) for d in dims]
    c2 = [Dev(shape=d, dtype=np.uint8, pitched=True) for d in dims]

    def tab(bufs):
        return (C.c_void_p * n)(*[b.ptr for b in bufs])

    arrH = (C.c_int * n)(*[d[0] for d in dims])
    arrW = (C.c_int * n)(*[d[1] for d in dims])
    p4 = (C.c_size_t * n)(*[b.pitch for b in p1])
    pc = (C.c_size_t * n)(*[b.pitch for b in c1])
    lib().baoCudaPatchMatchMultiscalePrepare(tab(p1), tab(p2), tab(c1), tab(c2), tab(t1), tab(t2), arrH, arrW, p4, pc, n, r1.ptr, r2.ptr, h, w)
    check_launcher("baoCudaPatchMatchMultiscalePrepare")
    return [b.get() for b in p1], [b.get() for b in p2], [b.get() for b in c1], [b.get() for b in c2]


class PlaneSet:
    """Device copies of (img1, img2, census1, census2) of one level."""

    def __init__(self, img1, img2, c1, c2):
        self.h, self.w = img1.shape
        self.i1, self.i2 = Dev(img1, pitched=True), Dev(img2, pitched=True)
        self.c1, self.c2 = Dev(c1, pitched=True), Dev(c2, pitched=True)

    def args(self):
        return (self.i1.ptr, self.i2.ptr, self.c1.ptr, self.c2.ptr)


class PmRng:
    def __init__(self, w, h, params=None):
        self.p = C.c_void_p()
        self.w, self.h = w, h
        check(lib().eppm_pm_rng_create(C.byref(self.p), w, h, C.byref(params) if params is not None else None), "rng_create")

    def block_states(self):
        nb = ((self.w + 15) // 16) * ((self.h + 15) // 16)
        out = np.empty((nb, 6), np.uint32)
        check(lib().eppm_pm_rng_block_states(self.p, out.ctypes.data, out.size), "rng_block_states")
        return out

    def __del__(self):
        try:
            if self.p:
                lib().eppm_pm_rng_destroy(self.p)
        except Exception:
            pass


def pm_gen_rand_field(rng):
    nnf = Dev(shape=(rng.h, rng.w), dtype=short2)
    check(lib().eppm_memset_device(nnf.ptr, 0, nnf.pitch * nnf.h), "memset")
    check(lib().eppm_pm_gen_rand_field(rng.p, nnf.ptr, rng.w, rng.h, nnf.pitch), "pm_gen_rand_field")
    return nnf.get()


def pm_cost_field(nnf, P):
    n, c = Dev(nnf), Dev(shape=(P.h, P.w), dtype=np.float32)
    check(lib().eppm_pm_cost_field(c.ptr, n.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch),
          "pm_cost_field")
    return c.get()


def pm_seg_propagate(cost, nnf, P, direction):
    n, c = Dev(nnf), Dev(cost)
    check(lib().eppm_pm_seg_propagate(c.ptr, n.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch, direction), "pm_seg_propagate")
    return c.get(), n.get()


def pm_jump_propagate(cost, nnf, P):
    n, c = Dev(nnf), Dev(cost)
    check(lib().eppm_pm_jump_propagate(c.ptr, n.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch),
          "pm_jump_propagate")
    return c.get(), n.get()


def pm_parallel_propagate(cost, nnf, P):
    """One launch of the 4-neighbour propagation (baoParallelPropagate, bao_pmflow_kernel.cu:720-795)."""
    n, c = Dev(nnf), Dev(cost)
    check(lib().eppm_pm_parallel_propagate(c.ptr, n.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch), "pm_parallel_propagate")
    return c.get(), n.get()


def pm_random_search(rng, cost, nnf, P):
    n, c = Dev(nnf), Dev(cost)
    check(lib().eppm_pm_random_search(rng.p, c.ptr, n.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch), "pm_random_search")
    return c.get(), n.get()


def pm_search_launch(rng, costs, nnfs, pairs, ndir=1, pretest=False, sums=False):
    """eppm_test_pm_search (test library): ONE random-search launch over len(pairs) x ndir problems as a context issues it (parity planes,
    numbers drawn ahead).  pairs: (img1, img2) uchar4 per pair; costs / nnfs: one per problem, pair p's direction k at p * ndir + k.
    pretest: the two-phase form.  Returns (costs, nnfs, rest-weight planes or None), one array per problem; sums (with pretest): also the
    pre-test's (N, D_A) planes of every pixel with its match in nnfs as the guess, as a fourth and fifth list."""
    h, w = nnfs[0].shape
    n = len(nnfs)
    assert n == len(pairs) * ndir == len(costs)
    c = Dev(np.concatenate([np.ascontiguousarray(x, np.float32) for x in costs]))
    f = Dev(np.concatenate([np.ascontiguousarray(x, short2) for x in nnfs]))
    i1, i2 = (Dev(np.concatenate([np.ascontiguousarray(p[k], uchar4) for p in pairs])) for k in range(2))
    u = Dev(shape=(n * h, w), dtype=np.float32) if pretest else None
    pn, pd = (Dev(shape=(n * h, w), dtype=np.float32) for _ in range(2)) if pretest and sums else (None, None)
    check(lib().eppm_test_pm_search(rng.p, c.ptr, f.ptr, i1.ptr, i2.ptr, w, h, ndir, len(pairs), int(pretest), u.ptr if u else None,
                                    pn.ptr if pn else None, pd.ptr if pd else None), "eppm_test_pm_search")
    split = lambda a: [a[k * h:(k + 1) * h] for k in range(n)]  # noqa: E731
    out = (split(c.get()), split(f.get()), split(u.get()) if u else None)
    return out + (split(pn.get()), split(pd.get())) if pn else out


def probe_search_pretest(iteration, w, h, patch_r=9, problems=2, npairs=1):
    """eppm_probe_search_pretest (test library, no GPU needed): (two-phase form at this iteration?, first centre row, centre rows, threshold
    iteration, eps, has the launch a two-phase form at all?)"""
    out = (C.c_int * 5)()
    eps = C.c_float()
    check(lib().eppm_probe_search_pretest(iteration, w, h, patch_r, problems, npairs, out, C.byref(eps)), "eppm_probe_search_pretest")
    return bool(out[0]), out[1], out[2], out[3], eps.value, bool(out[4])


def patchmatch(P):
    """baoCudaPatchMatch -> (nnf, cost)"""
    n, c = Dev(shape=(P.h, P.w), dtype=short2), Dev(shape=(P.h, P.w), dtype=np.float32)
    lib().baoCudaPatchMatch(n.ptr, c.ptr, *P.args(), P.w, P.h, P.i1.pitch, c.pitch, n.pitch, P.c1.pitch)
    check_launcher("baoCudaPatchMatch")
    return n.get(), c.get()


def left_right_check(nnf1, cost1, nnf2, cost2):
    h, w = nnf1.shape
    a, b, c, d = Dev(nnf1), Dev(cost1), Dev(nnf2), Dev(cost2)
    lib().baoCudaLeftRightCheck(a.ptr, b.ptr, c.ptr, d.ptr, w, h, b.pitch, a.pitch)
    check_launcher("baoCudaLeftRightCheck")
    return a.get(), b.get(), c.get(), d.get()


def outlier_removal(nnf, cost):
    h, w = nnf.shape
    a, b = Dev(nnf), Dev(cost)
    lib().baoCudaOutlierRemoval(a.ptr, b.ptr, w, h, b.pitch, a.pitch)
    check_launcher("baoCudaOutlierRemoval")
    return a.get(), b.get()


def weighted_median(nnf, img, num_iter=20, only_occlusion=True):
    h, w = nnf.shape
    a, i = Dev(nnf), Dev(img, pitched=True)
    lib().baoCudaWeightedMedianFilter(a.ptr, None, i.ptr, w, h, i.pitch, w * 4, a.pitch, num_iter, only_occlusion)
    check_launcher("baoCudaWeightedMedianFilter")
    return a.get()


def fill_holes(nnf, img):
    h, w = nnf.shape
    a, i = Dev(nnf), Dev(img, pitched=True)
    lib().baoCudaFillHole(a.ptr, None, i.ptr, w, h, i.pitch, w * 4, a.pitch)
    check_launcher("baoCudaFillHole")
    return a.get()


def nnf2flow(nnf):
    h, w = nnf.shape
    a, f = Dev(nnf), Dev(shape=(h, w), dtype=float2)
    lib().baoCudaNNF2Flow(f.ptr, a.ptr, w, h, a.pitch, f.pitch)
    check_launcher("baoCudaNNF2Flow")
    return f.get()


def resize_flow(flow, out_h, out_w, ratio=2.0):
    h, w = flow.shape
    a, b = Dev(flow), Dev(shape=(out_h, out_w), dtype=float2)
    check(lib().eppm_resize_flow(b.ptr, out_h, out_w, a.ptr, h, w, ratio), "resize_flow")
    return b.get()


def flow_upsample(coarse, img):
    """eppm_flow_upsample (draft mode's kernel): the (hc, wc) float2 flow `coarse` up to the size of the uchar4 guide
    image, in one launch."""
    h, w = img.shape
    hc, wc = coarse.shape
    a, i, b = Dev(coarse), Dev(img, pitched=True), Dev(shape=(h, w), dtype=float2)
    check(lib().eppm_flow_upsample(b.ptr, h, w, a.ptr, hc, wc, i.ptr, i.pitch), "eppm_flow_upsample")
    return b.get()


def c2f_refine(flow, P):
    """baoCudaBLFCostFilterRefine"""
    f = Dev(flow)
    lib().baoCudaBLFCostFilterRefine(f.ptr, *P.args(), P.w, P.h, P.i1.pitch, P.c1.pitch)
    check_launcher("baoCudaBLFCostFilterRefine")
    return f.get()


def c2f_refine_batch(flows, planes):
    """eppm_test_c2f_refine_batch (test library): the candidate refine of len(flows) pairs of one size in ONE launch, as a batch context
    issues it.  flows: (h, w) float2 per pair; planes: (img1, img2, census1, census2) per pair.  Returns the refined flow per pair."""
    n = len(flows)
    h, w = flows[0].shape
    f = Dev(np.concatenate([np.ascontiguousarray(x, float2) for x in flows]))
    i1, i2, c1, c2 = (Dev(np.concatenate([np.ascontiguousarray(p[k]) for p in planes])) for k in range(4))
    check(lib().eppm_test_c2f_refine_batch(f.ptr, i1.ptr, i2.ptr, c1.ptr, c2.ptr, w, h, n), "eppm_test_c2f_refine_batch")
    out = f.get()
    return [out[k * h:(k + 1) * h] for k in range(n)]


def c2f_refine_pre(flows, planes, pre, parts=False):
    """eppm_test_c2f_refine_pre (test library): c2f_refine_batch with the window kernel's coherent tiles one-phase (pre = 0) or two-phase
    (pre = 1).  Returns (refined flow per pair, the kernel's counters: tiles two-phase, tiles with a weight sum too small, tiles with more
    survivors than one list holds, other tiles, pairs tested, pairs rejected; with `parts` also: tiles drained in halves, in quarters)."""
    n = len(flows)
    h, w = flows[0].shape
    f = Dev(np.concatenate([np.ascontiguousarray(x, float2) for x in flows]))
    i1, i2, c1, c2 = (Dev(np.concatenate([np.ascontiguousarray(p[k]) for p in planes])) for k in range(4))
    stat = (C.c_uint * 8)()
    check(lib().eppm_test_c2f_refine_pre(f.ptr, i1.ptr, i2.ptr, c1.ptr, c2.ptr, w, h, n, int(pre), stat), "eppm_test_c2f_refine_pre")
    out = f.get()
    return [out[k * h:(k + 1) * h] for k in range(n)], tuple(stat[:8 if parts else 6])


def c2f_refine_probe(flows, planes):
    """eppm_test_c2f_refine_probe (test library): the two-phase launch by the kernel's probing instantiation.  Returns (refined flow per pair,
    N, D: (pairs, h, w, 4, 9) float32 -- [pass][candidate] --, U: (pairs, h, w)); NaN where the kernel formed nothing."""
    n = len(flows)
    h, w = flows[0].shape
    f = Dev(np.concatenate([np.ascontiguousarray(x, float2) for x in flows]))
    i1, i2, c1, c2 = (Dev(np.concatenate([np.ascontiguousarray(p[k]) for p in planes])) for k in range(4))
    pr = Dev(shape=(n * h, w * 73), dtype=np.float32)
    check(lib().eppm_test_c2f_refine_probe(f.ptr, i1.ptr, i2.ptr, c1.ptr, c2.ptr, w, h, n, pr.ptr), "eppm_test_c2f_refine_probe")
    out, p = f.get(), pr.get().reshape(n, h, w, 73)
    return [out[k * h:(k + 1) * h] for k in range(n)], p[..., :36].reshape(n, h, w, 4, 9), p[..., 36:72].reshape(n, h, w, 4, 9), p[..., 72]


def probe_c2f_pretest(patch_r=9):
    """eppm_probe_c2f_pretest (test library, no GPU needed): (on by default?, first centre row, centre rows, items of a tile's survivor
    list, eps, smallest admissible weight sum, smallest right-hand side that may reject)"""
    out, fl = _c2f_pretest_knobs(patch_r)
    return bool(out[0]), out[1], out[2], out[3], fl[0], fl[1], fl[2]


def probe_c2f_parts(patch_r=9):
    """eppm_probe_c2f_pretest's fifth knob: does a tile with more survivors than one list holds stay two-phase, drained in parts?"""
    return bool(_c2f_pretest_knobs(patch_r)[0][4])


def _c2f_pretest_knobs(patch_r):
    out = (C.c_int * 5)()
    fl = (C.c_float * 3)()
    check(lib().eppm_probe_c2f_pretest(patch_r, out, fl), "eppm_probe_c2f_pretest")
    return out, fl


def blf_c2f(flow_coarse, P_fine, coarse_dims):
    """baoCudaBLF_C2F from level l+1 (flow_coarse) to level l (P_fine): upsample x2, x2.0, candidate refine."""
    ch, cw = coarse_dims
    fine = Dev(shape=(P_fine.h, P_fine.w), dtype=float2)
    coarse = Dev(flow_coarse)
    tab = lambda a, b: (C.c_void_p * 2)(a, b)  # noqa: E731
    arrH = (C.c_int * 2)(P_fine.h, ch)
    arrW = (C.c_int * 2)(P_fine.w, cw)
    p4 = (C.c_size_t * 2)(P_fine.i1.pitch, 0)
    pc = (C.c_size_t * 2)(P_fine.c1.pitch, 0)
    lib().baoCudaBLF_C2F(tab(fine.ptr, coarse.ptr), tab(P_fine.i1.ptr, None), tab(P_fine.i2.ptr, None), tab(P_fine.c1.ptr, None),
                         tab(P_fine.c2.ptr, None), None, None, arrH, arrW, p4, pc, 0)
    check_launcher("baoCudaBLF_C2F")
    return fine.get()


def flow_smoothing(flow, img):
    h, w = flow.shape
    f, i = Dev(flow), Dev(img, pitched=True)
    lib().baoCudaFlowSmoothing(f.ptr, i.ptr, w, h, i.pitch, f.pitch)
    check_launcher("baoCudaFlowSmoothing")
    return f.get()


def temporal_prior(prev, backward=False):
    """eppm_temporal_prior (the advection kernels of a streaming context) on a numpy displacement field."""
    d_prev = Dev(np.ascontiguousarray(prev, short2))
    d_out = Dev(shape=prev.shape, dtype=short2)
    check(lib().eppm_temporal_prior(d_out.ptr, d_prev.ptr, d_prev.h, d_prev.w, int(bool(backward))), "eppm_temporal_prior")
    check(lib().eppm_device_synchronize(), "eppm_device_synchronize")
    return d_out.get()


def temporal_prior_batch(prevs, backward=False, armed=None, calls=1):
    """eppm_temporal_prior_batch on (npairs, h, w) short2 displacement fields: every slot in one splat and one gather launch; armed: None
    (all) or a flag per slot.  calls > 1: the call is repeated on the same device planes, and the result of every call is returned."""
    prevs = np.ascontiguousarray(prevs, short2)
    n, h, w = prevs.shape
    d_prev = Dev(prevs.reshape(n * h, w))
    d_out = Dev(shape=(n * h, w), dtype=short2)
    flags = None if armed is None else (C.c_uint8 * n)(*[int(bool(x)) for x in armed])
    out = []
    for _ in range(calls):
        check(lib().eppm_temporal_prior_batch(d_out.ptr, d_prev.ptr, h, w, int(bool(backward)), n, flags), "eppm_temporal_prior_batch")
        check(lib().eppm_device_synchronize(), "eppm_device_synchronize")
        out.append(d_out.get().reshape(n, h, w))
    return out[0] if calls == 1 else out


def flow_to_color(flow, max_disp_x=20.0, max_disp_y=20.0):
    """bao_cuda_convert_flow_to_colorshow (float2 form, basic/bao_basic_cuda.cuh:839-845): (h,w) float2 -> (h,w) uchar4 {R,G,B,0}."""
    h, w = flow.shape
    f, c = Dev(flow), Dev(shape=(h, w), dtype=uchar4)
    check(lib().eppm_flow_to_color(c.ptr, f.ptr, h, w, max_disp_x, max_disp_y), "eppm_flow_to_color")
    return c.get()
