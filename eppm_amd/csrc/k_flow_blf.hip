// k_flow_blf.hip -- coarse-to-fine step, joint-bilateral smoothing of the refined flow (reference: bao_pmflow_refine_kernel.cu:756-799).
#include <type_traits>

#include "eppm_device.cuh"
#include "eppm_internal.h"

// ---- every tuning knob of the smoothing: set with -D (tools/build_variant.sh), cited by name in profiles/ ----
#ifndef EPPM_BLF_UNROLL
#define EPPM_BLF_UNROLL 21      // taps of a row the compiler may interleave
#endif
#ifndef EPPM_BLF_MIX
#define EPPM_BLF_MIX 3          // two pixels per lane: every M-th tap column's range weights by formula, the rest by table (LDS / VALU balance); 0: all by table
#endif
#ifndef EPPM_BLF_MIX1
#define EPPM_BLF_MIX1 2         // one pixel per lane (the smaller launches)
#endif
#ifdef EPPM_BLF_WAVES           // (no default: the compiler's choice) waves per SIMD of k_flow_blf
#define EPPM_BLF_OCC __attribute__((amdgpu_waves_per_eu(EPPM_BLF_WAVES, EPPM_BLF_WAVES)))
#else
#define EPPM_BLF_OCC
#endif
#define EPPM_BLF_PRAGMA_(x) _Pragma(#x)
#define EPPM_BLF_UNROLL_PRAGMA(n) EPPM_BLF_PRAGMA_(unroll n)

namespace eppm {

// ---------------------------------------------------------------------------------------------------
// refine :764-799: 21x21 joint bilateral filter of the flow guided by image 1 (Jacobi).
//
// 32x16 output tile, 256 threads: a lane filters TWO vertically adjacent pixels, so each tap row it reads from
// LDS serves both (rows 0..20 the upper pixel, 1..21 the lower one) -- one pixel per lane reads 21 B of LDS per
// tap and is LDS-bandwidth bound.  The (32+20)x(16+20) halo tile holds {r, g, b, flow x} and {flow y} per texel.
// Taps the reference skips (outside the image, or unknown flow, refine :781) are stored with r = 100: their range
// distance is ~100, the exponent -2.5e7 and fast_exp returns exactly 0, so they add 0 * flow = 0 and 0 to the
// sums -- no validity flag, no divergent branch (unknown flows are the finite marker 1e10, never inf).
// ---------------------------------------------------------------------------------------------------
// PPL = pixels per lane: 2 (32x16 tile) for large launches, 1 (32x8 tile, twice the waves) otherwise, see launch_flow_blf.
constexpr int BT_W = 32, BR = kBlfRadius, BTW = BT_W + 2 * BR;
// which taps of the smoothing evaluate their range weight instead of reading it (pixel: 0 upper / only, 1 lower)
template <int PPL>
__device__ __forceinline__ constexpr bool blf_by_formula(int dx, int pixel)
{
    constexpr int M = (PPL == 1) ? EPPM_BLF_MIX1 : EPPM_BLF_MIX;
    return M == 1 ? (PPL == 2 ? pixel == 1 : (dx & 1)) : M >= 2 ? dx % M == 0 : false;
}
template <int PPL>
__global__ __launch_bounds__(256) EPPM_BLF_OCC void k_flow_blf(float* __restrict__ out_, const float* __restrict__ in_,
                                                  const uint32_t* __restrict__ img_, int ipitch, int w, int h, int fpitch,
                                                  const float* __restrict__ blf_lut, size_t pstride)
{
    float* __restrict__ out = pair_ptr(out_, pstride, blockIdx.z);
    const float* __restrict__ in = pair_ptr(in_, pstride, blockIdx.z);
    const uint32_t* __restrict__ img = pair_ptr(img_, pstride, blockIdx.z);
    constexpr int BT_H = 8 * PPL, BTH = BT_H + 2 * BR;
    __shared__ float4 s_t[BTH * BTW];          // r, g, b (unorm), flow x
    __shared__ float s_fy[BTH * BTW];
    __shared__ float s_lut[BR + 1];
    __shared__ DeltaTab s_D;                   // exp(-d^2 / POSTPROC_BLF_SIG_R^2) by table: the same bits as the formula (eppm_device.cuh)
    const int x0 = blockIdx.x * BT_W, y0 = blockIdx.y * BT_H;
    const int tid = threadIdx.y * BT_W + threadIdx.x;
    if (tid <= BR) s_lut[tid] = blf_lut[tid];
    load_delta_tab<false>(s_D, blf_lut + BR + 1, tid, 256);
    for (int t = tid; t < BTW * BTH; t += 256) {
        const int cy = y0 + t / BTW - BR, cx = x0 + t % BTW - BR;
        float4 e = make_float4(100.0f, 0.0f, 0.0f, 0.0f);
        float fy = 0.0f;
        if (cx >= 0 && cy >= 0 && cx < w && cy < h) {
            e.w = in[(cy * fpitch + cx) * 2];
            fy = in[(cy * fpitch + cx) * 2 + 1];
            if (!(e.w > kUnknownFlowThresh || fy > kUnknownFlowThresh)) {     // refine :781
                const rgbf c = unpack_rgb(img[cy * ipitch + cx]);
                e.x = c.x; e.y = c.y; e.z = c.z;
            }
        }
        s_t[t] = e;
        s_fy[t] = fy;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, ya = y0 + PPL * threadIdx.y;        // pixels (x, ya) and, PPL = 2, (x, ya + 1)
    if (x >= w || ya >= h) return;
    const bool has_b = (PPL == 2) && (ya + 1 < h);
    const rgbf ca = unpack_rgb(img[ya * ipitch + x]);
    const rgbf cb = unpack_rgb(img[(has_b ? ya + 1 : ya) * ipitch + x]);
    float nxa = 0.f, nya = 0.f, wa = 0.f, nxb = 0.f, nyb = 0.f, wb = 0.f;
    const int base = (PPL * threadIdx.y) * BTW + threadIdx.x;
    // tap rows ya-10 .. ya+11: row 0 serves only the upper pixel, row 21 only the lower one, rows 1..20 both
    auto tap_row = [&](int r, auto use_a, auto use_b) {
        const float gya = use_a ? s_lut[abs(r - BR)] : 0.0f;
        const float gyb = use_b ? s_lut[abs(r - 1 - BR)] : 0.0f;
EPPM_BLF_UNROLL_PRAGMA(EPPM_BLF_UNROLL)
        for (int dx = 0; dx <= 2 * BR; dx++) {
            const int ti = base + r * BTW + dx;
            const float4 tp = s_t[ti];
            const float tfy = s_fy[ti];
            const rgbf pix = {tp.x, tp.y, tp.z};
            const float gx = s_lut[abs(dx - BR)];
            if (use_a) {
                // (a skipped tap, r = 100, meets the entry of d = 1: exp(-2500) = 0 exactly, as the formula gives for d ~ 100)
                // one pixel per lane (PPL = 1): every other tap column by formula
                const bool tab_a = EPPM_DELTA_BLF && !blf_by_formula<PPL>(dx, 0);
                const float delta_r = tab_a ? __builtin_amdgcn_fmed3f(max_abs_diff(ca, pix), 0.0f, 1.0f) : max_abs_diff(ca, pix);
                const float coef_r = tab_a ? delta_lookup_off(s_D, delta_r) : fast_exp(div_wmf2(-(delta_r * delta_r)));
                const float coef_s = gx * gya;
                const float wgt = coef_r * coef_s;
                nxa += wgt * tp.w;
                nya += wgt * tfy;
                wa += wgt;
            }
            if (use_b) {
                // EPPM_BLF_MIX: the lower pixel EVALUATES the weight (the same bits: the table was filled by this formula; a skipped tap's
                // distance ~100 gives exp(-2.5e7) = 0 exactly) -- the table reads of both pixels made the LDS array the kernel's bound
                // (28 array cycles per tap against 14.5 issue cycles per CU); one of two by formula: 18 against 21.5
                const bool tab_b = EPPM_DELTA_BLF && !blf_by_formula<PPL>(dx, 1);
                const float delta_r = tab_b ? __builtin_amdgcn_fmed3f(max_abs_diff(cb, pix), 0.0f, 1.0f) : max_abs_diff(cb, pix);
                const float coef_r = tab_b ? delta_lookup_off(s_D, delta_r) : fast_exp(div_wmf2(-(delta_r * delta_r)));
                const float coef_s = gx * gyb;
                const float wgt = coef_r * coef_s;
                nxb += wgt * tp.w;
                nyb += wgt * tfy;
                wb += wgt;
            }
        }
    };
    if (PPL == 2) {
        tap_row(0, std::true_type{}, std::false_type{});
#pragma unroll 1
        for (int r = 1; r <= 2 * BR; r++) tap_row(r, std::true_type{}, std::true_type{});
        tap_row(2 * BR + 1, std::false_type{}, std::true_type{});
    } else {
#pragma unroll 1
        for (int r = 0; r <= 2 * BR; r++) tap_row(r, std::true_type{}, std::false_type{});
    }
    {
        const int ci = base + BR * BTW + BR;
        float ox = s_t[ci].w, oy = s_fy[ci];
        if (wa != 0) { ox = nxa / wa; oy = nya / wa; }
        out[(ya * fpitch + x) * 2] = ox;
        out[(ya * fpitch + x) * 2 + 1] = oy;
    }
    if (has_b) {
        const int ci = base + (BR + 1) * BTW + BR;
        float ox = s_t[ci].w, oy = s_fy[ci];
        if (wb != 0) { ox = nxb / wb; oy = nyb / wb; }
        out[((ya + 1) * fpitch + x) * 2] = ox;
        out[((ya + 1) * fpitch + x) * 2 + 1] = oy;
    }
}
int flow_blf_pixels_per_lane(int w, int h, int npairs)
{
    const int wgs2 = ((w + BT_W - 1) / BT_W) * ((h + 15) / 16) * npairs;
    // two pixels per lane halve the LDS traffic but double the work quantum: they pay from about 8 workgroups per CU
    // (1920x1080: 0.96 vs 1.03 ms); below that the finer quantum balances the 256 CUs better (1024x436: 0.25 vs 0.27 ms)
    return wgs2 >= 8 * 256 ? 2 : 1;
}
void launch_flow_blf(float* out, const float* in, const uint32_t* img, int ipitch, int w, int h, int flow_pitch,
                     const float* blf_lut, hipStream_t s, Batch bt)
{
    dim3 block(BT_W, 8);
    const int ppl = flow_blf_pixels_per_lane(w, h, bt.n);
    launch_note(kLaunchSmoothing, w, h, bt.n, ppl);
    if (ppl == 2) {
        hipLaunchKernelGGL(k_flow_blf<2>, dim3((w + BT_W - 1) / BT_W, (h + 15) / 16, bt.n), block, 0, s, out, in, img, ipitch, w, h, flow_pitch, blf_lut, bt.stride);
    } else {
        hipLaunchKernelGGL(k_flow_blf<1>, dim3((w + BT_W - 1) / BT_W, (h + 7) / 8, bt.n), block, 0, s, out, in, img, ipitch, w, h, flow_pitch, blf_lut, bt.stride);
    }
}

}  // namespace eppm
