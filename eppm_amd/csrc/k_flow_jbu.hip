// k_flow_jbu.hip -- draft mode: joint-bilateral UPSAMPLING of the flow, one launch per level below the stop level
// in place of resize + candidate refine + smoothing (reference: the dead code at bao_pmflow_refine_kernel.cu:829-888).
#include <type_traits>

#include "eppm_device.cuh"
#include "eppm_internal.h"

// ---- the tuning knobs of the upsampling: set with -D (tools/build_variant.sh); the smoothing's values (k_flow_blf.hip) ----
#ifndef EPPM_JBU_UNROLL
#define EPPM_JBU_UNROLL 21      // taps of a row the compiler may interleave
#endif
#ifndef EPPM_JBU_MIX
#define EPPM_JBU_MIX 3          // two pixels per lane: every M-th tap column's range weights by formula, the rest by table (LDS / VALU balance); 0: all by table
#endif
#ifndef EPPM_JBU_MIX1
#define EPPM_JBU_MIX1 2         // one pixel per lane (the smaller launches)
#endif
#define EPPM_JBU_PRAGMA_(x) _Pragma(#x)
#define EPPM_JBU_UNROLL_PRAGMA(n) EPPM_JBU_PRAGMA_(unroll n)

namespace eppm {

// ---------------------------------------------------------------------------------------------------
// JBU(F, I): the smoothing of k_flow_blf.hip on the fine level's guide image I, with a tap's flow read from the COARSE level:
//     F'(cx, cy) = 2 * F[min(cy >> 1, hc - 1)][min(cx >> 1, wc - 1)]
// i.e. the oracle's flow_smoothing(2 * replicate2x(F), I), bit for bit.  Fused: the doubled, 2x-replicated plane is never written; the only
// difference from k_flow_blf is where the halo tile's flow comes from when the workgroup stages it -- a quarter of the smoothing's flow
// bytes from memory --, and the tap loop is the smoothing's, texel for texel: the same taps in the same dy-outer / dx-inner order, the
// same DeltaTab / formula mix, the r = 100 marker for skipped taps (outside the image, or a component of F' above the unknown-flow
// threshold), one product per tap (the two or four taps on one coarse texel are never merged), the same divide, and F'(x, y) where the
// weight sum is 0.  (A first form kept the flow tile at coarse resolution, 12 + 4 bytes of LDS per tap against 20: it needed a second
// staging pass with its own barrier and two LDS instructions per guide texel and ran 1.04-1.34 x the smoothing's time)
// ---------------------------------------------------------------------------------------------------
constexpr int JT_W = 32, JR = kBlfRadius, JTW = JT_W + 2 * JR;
// which taps of the smoothing evaluate their range weight instead of reading it (pixel: 0 upper / only, 1 lower)
template <int PPL>
__device__ __forceinline__ constexpr bool jbu_by_formula(int dx, int pixel)
{
    constexpr int M = (PPL == 1) ? EPPM_JBU_MIX1 : EPPM_JBU_MIX;
    return M == 1 ? (PPL == 2 ? pixel == 1 : (dx & 1)) : M >= 2 ? dx % M == 0 : false;
}
template <int PPL>
__global__ __launch_bounds__(256) void k_flow_jbu(float* __restrict__ out_, const float* __restrict__ in_,
                                                  const uint32_t* __restrict__ img_, int ipitch, int w, int h, int wc, int hc,
                                                  const float* __restrict__ blf_lut, size_t pstride)
{
    float* __restrict__ out = pair_ptr(out_, pstride, blockIdx.z);
    const float* __restrict__ in = pair_ptr(in_, pstride, blockIdx.z);
    const uint32_t* __restrict__ img = pair_ptr(img_, pstride, blockIdx.z);
    constexpr int JT_H = 8 * PPL, JTH = JT_H + 2 * JR;
    __shared__ float4 s_t[JTH * JTW];          // r, g, b (unorm), flow x
    __shared__ float s_fy[JTH * JTW];
    __shared__ float s_lut[JR + 1];
    __shared__ DeltaTab s_D;                   // exp(-d^2 / POSTPROC_BLF_SIG_R^2) by table: the same bits as the formula (eppm_device.cuh)
    const int x0 = blockIdx.x * JT_W, y0 = blockIdx.y * JT_H;
    const int tid = threadIdx.y * JT_W + threadIdx.x;
    if (tid <= JR) s_lut[tid] = blf_lut[tid];
    load_delta_tab<false>(s_D, blf_lut + JR + 1, tid, 256);
    for (int t = tid; t < JTW * JTH; t += 256) {
        const int cy = y0 + t / JTW - JR, cx = x0 + t % JTW - JR;
        float4 e = make_float4(100.0f, 0.0f, 0.0f, 0.0f);
        float fy = 0.0f;
        if (cx >= 0 && cy >= 0 && cx < w && cy < h) {
            const int ci = (min(cy >> 1, hc - 1) * wc + min(cx >> 1, wc - 1)) * 2;         // F'(cx, cy): the coarse texel, doubled (exact)
            e.w = 2.0f * in[ci];
            fy = 2.0f * in[ci + 1];
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
    const int base = (PPL * threadIdx.y) * JTW + threadIdx.x;
    // tap rows ya-10 .. ya+11: row 0 serves only the upper pixel, row 21 only the lower one, rows 1..20 both
    auto tap_row = [&](int r, auto use_a, auto use_b) {
        const float gya = use_a ? s_lut[abs(r - JR)] : 0.0f;
        const float gyb = use_b ? s_lut[abs(r - 1 - JR)] : 0.0f;
EPPM_JBU_UNROLL_PRAGMA(EPPM_JBU_UNROLL)
        for (int dx = 0; dx <= 2 * JR; dx++) {
            const int ti = base + r * JTW + dx;
            const float4 tp = s_t[ti];
            const float tfy = s_fy[ti];
            const rgbf pix = {tp.x, tp.y, tp.z};
            const float gx = s_lut[abs(dx - JR)];
            if (use_a) {
                // (a skipped tap, r = 100, meets the entry of d = 1: exp(-2500) = 0 exactly, as the formula gives for d ~ 100)
                // one pixel per lane (PPL = 1): every other tap column by formula
                const bool tab_a = EPPM_DELTA_BLF && !jbu_by_formula<PPL>(dx, 0);
                const float delta_r = tab_a ? __builtin_amdgcn_fmed3f(max_abs_diff(ca, pix), 0.0f, 1.0f) : max_abs_diff(ca, pix);
                const float coef_r = tab_a ? delta_lookup_off(s_D, delta_r) : fast_exp(div_wmf2(-(delta_r * delta_r)));
                const float coef_s = gx * gya;
                const float wgt = coef_r * coef_s;
                nxa += wgt * tp.w;
                nya += wgt * tfy;
                wa += wgt;
            }
            if (use_b) {
                // EPPM_JBU_MIX: the lower pixel EVALUATES the weight (the same bits: the table was filled by this formula; a skipped tap's
                // distance ~100 gives exp(-2.5e7) = 0 exactly) -- the table reads of both pixels made the LDS array the kernel's bound
                // (28 array cycles per tap against 14.5 issue cycles per CU); one of two by formula: 18 against 21.5
                const bool tab_b = EPPM_DELTA_BLF && !jbu_by_formula<PPL>(dx, 1);
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
        for (int r = 1; r <= 2 * JR; r++) tap_row(r, std::true_type{}, std::true_type{});
        tap_row(2 * JR + 1, std::false_type{}, std::true_type{});
    } else {
#pragma unroll 1
        for (int r = 0; r <= 2 * JR; r++) tap_row(r, std::true_type{}, std::false_type{});
    }
    {
        const int ci = base + JR * JTW + JR;
        float ox = s_t[ci].w, oy = s_fy[ci];
        if (wa != 0) { ox = nxa / wa; oy = nya / wa; }
        out[(ya * w + x) * 2] = ox;
        out[(ya * w + x) * 2 + 1] = oy;
    }
    if (has_b) {
        const int ci = base + (JR + 1) * JTW + JR;
        float ox = s_t[ci].w, oy = s_fy[ci];
        if (wb != 0) { ox = nxb / wb; oy = nyb / wb; }
        out[((ya + 1) * w + x) * 2] = ox;
        out[((ya + 1) * w + x) * 2 + 1] = oy;
    }
}
void launch_flow_jbu(float* out, const float* in_coarse, const uint32_t* img, int ipitch, int w, int h, int wc, int hc, const float* blf_lut,
                     hipStream_t s, Batch bt)
{
    dim3 block(JT_W, 8);
    const int ppl = flow_blf_pixels_per_lane(w, h, bt.n);
    launch_note(kLaunchJbu, w, h, bt.n, ppl);
    if (ppl == 2) {
        hipLaunchKernelGGL(k_flow_jbu<2>, dim3((w + JT_W - 1) / JT_W, (h + 15) / 16, bt.n), block, 0, s, out, in_coarse, img, ipitch, w, h, wc, hc, blf_lut, bt.stride);
    } else {
        hipLaunchKernelGGL(k_flow_jbu<1>, dim3((w + JT_W - 1) / JT_W, (h + 7) / 8, bt.n), block, 0, s, out, in_coarse, img, ipitch, w, h, wc, hc, blf_lut, bt.stride);
    }
}

}  // namespace eppm
