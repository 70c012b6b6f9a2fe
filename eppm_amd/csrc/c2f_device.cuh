// c2f_device.cuh -- the plane-fitting candidate refine of the coarse-to-fine step (reference: bao_pmflow_kernel.cu:2005-2041), what the
// kernels of k_c2f_refine.hip are made of: the knobs, the offset tables of the affine passes, the window geometry, the patch term and
// the passes over it, the per-pixel frame.
#pragma once
#include "eppm_device.cuh"

// ---------------------------------------------------------------------------------------------------
// Every tuning knob of the refine kernels and their launcher: set with -D (tools/build_variant.sh), cited by name in profiles/
// ---------------------------------------------------------------------------------------------------
#ifndef EPPM_C2F_UNROLL
#define EPPM_C2F_UNROLL 2
#endif
// Waves per SIMD the register allocator plans for.  LDS would allow 5 (29 KB per workgroup), but at 4 the 116-VGPR
// schedule keeps more gathers in flight per wave and is 1.5 % faster than the 92-VGPR one (A/B on one box,
// tools/gpu.sh ab); unroll 1 / 5 of the sample loop and 3 waves are slower, and so is a software-pipelined loop
// that issues the gathers of the next sample pair before computing the current one (161 VGPRs, +6 % instructions,
// +3.5 % time: the kernel waits on VALU issue, not on memory).
#ifndef EPPM_C2F_WAVES
#define EPPM_C2F_WAVES 4
#endif
#ifndef EPPM_C2F_WAVES_MIN
#define EPPM_C2F_WAVES_MIN 2
#endif
#define EPPM_C2F_OCC __attribute__((amdgpu_waves_per_eu(EPPM_C2F_WAVES_MIN, EPPM_C2F_WAVES)))     // (min, max): radius 17 only fits 2
#ifndef EPPM_C2F_WIN_H
#ifdef EPPM_TOL
#define EPPM_C2F_WIN_H 50
#else
#define EPPM_C2F_WIN_H 48      // the data term's table (4.2 KB, eppm_device.cuh: DeltaTab) and two workgroups per CU: 48 window rows (admissible spread 21)
#endif
#endif
#ifndef EPPM_C2F_PASS2
#define EPPM_C2F_PASS2 1       // k_c2f_refine_win: a pass group evaluates its two passes together (c2f_pass2_win); 0: one after the other
#endif
#ifndef EPPM_C2F_WIN_WAVES
#define EPPM_C2F_WIN_WAVES 4
#endif
// k_c2f_refine_win<9>, coherent tiles of the exact library: the two-phase form -- a pre-test over the
// EPPM_C2F_PRE_ROWS centre rows of every (candidate, pass), the best estimate in full, and only what the bound cannot reject after it.
// 0: the one-phase loop (also the two-phase form's fallback).  The test switch "c2f_pre" overrides it per launch.
#ifndef EPPM_C2F_PRE
#define EPPM_C2F_PRE 1
#endif
#ifndef EPPM_C2F_PRE_ROWS
#define EPPM_C2F_PRE_ROWS 5
#endif
#ifndef EPPM_C2F_PRE_EPS
#define EPPM_C2F_PRE_EPS 0x1p-13f             // shrinks the lower bound: >= 4 x the float error of its two sides (tests/test_refine_pretest_cpu.py)
#endif
// A tile whose survivors exceed one list is drained in parts -- the pixels' halves, else their quarters, each through the same list -- and
// stays in the two-phase form.  0: such a tile takes the one-phase loop after its pre-test, as before.
#ifndef EPPM_C2F_PRE_PARTS
#define EPPM_C2F_PRE_PARTS 1
#endif
#define EPPM_C2F_PRE_DMIN 0x1p-60f            // a tile with a centre-row weight sum not above this takes the one-phase loop (its costs may be 0/0)
#define EPPM_C2F_PRE_RHSMIN 0x1p-100f         // no rejection unless best * (D_A + U) is a normal number this far from underflow
#ifndef EPPM_C2F_SPLIT_BELOW_WAVES
#define EPPM_C2F_SPLIT_BELOW_WAVES 1024              // fewer than 1 wave per SIMD on 256 CUs (at 256 threads per tile)
#endif
#ifndef EPPM_C2F_WINDOW
#define EPPM_C2F_WINDOW 1      // radius 9: k_c2f_refine_win; 0: k_c2f_refine_tiled<9, 0>
#endif
#ifndef EPPM_C2F_WINDOW17
#define EPPM_C2F_WINDOW17 1    // radius 17: k_c2f_refine_win4; 0: k_c2f_refine_tiled<17, 0>
#endif
#ifdef EPPM_TOL
#define EPPM_C2F_LOG2 true      // the tolerance library's tile kernels keep log2(gs_j gs_i): their weight is one exp2 (eppm_device.cuh)
#else
#define EPPM_C2F_LOG2 false
#endif
#define EPPM_PRAGMA_(x) _Pragma(#x)
#define EPPM_UNROLL(n) EPPM_PRAGMA_(unroll n)

namespace eppm {

__device__ __forceinline__ Planes to_dev(const PlanesH& h, size_t pstride = 0, unsigned pair = 0)
{
    Planes p;
    p.pk1 = pair_ptr((const float4*)h.pk1, pstride, pair); p.pk2 = pair_ptr((const float4*)h.pk2, pstride, pair);
    p.w = h.w; p.h = h.h; p.pitch = h.pitch;
    return p;
}

// texel (sx, sy) for an LDS tile: from the 4-byte plane when the launch has one (converted here, bit for bit what the float4
// plane holds: both come from make_texel), else from the float4 plane
__device__ __forceinline__ float4 stage_texel(const uint32_t* __restrict__ pc, const float4* __restrict__ pk, unsigned idx)
{
    if (pc) { const uint32_t w = pc[idx]; return make_texel(w, w >> 24); }
    return pk[idx];
}

// ---------------------------------------------------------------------------------------------------
// The per-pixel frame of kernel.cu:2005-2041: 3x3 integer candidates (x offset outer, y offset inner) around the truncated
// up-sampled flow; cost = min of 4 affine passes; strict < keeps the first minimum; the centre candidate
// is the initial best with cost 999999.  In place: a thread reads and writes only its own pixel.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool c2f_unknown(float fvx, float fvy) { return fvx > kUnknownFlowThresh || fvy > kUnknownFlowThresh; }
__device__ __forceinline__ int c2f_centre(float f, int x) { return (int)(int16_t)(f2short(f) + x); }      // candidate centre from flow
__device__ __forceinline__ void c2f_store_flow(float* flow, int idx, int fx, int fy)      // a refined flow is integer
{
    flow[idx * 2] = (float)fx;
    flow[idx * 2 + 1] = (float)fy;
}
__device__ __forceinline__ float c2f_min(float a, float b) { return (a < b) ? a : b; }                    // the reference's __min: b where a is NaN
// __min(cost1,__min(cost2,__min(cost3,cost4))), kernel.cu:512
__device__ __forceinline__ float c2f_min4(float c1, float c2, float c3, float c4) { return c2f_min(c1, c2f_min(c2, c2f_min(c3, c4))); }
// the candidate loop of kernel.cu:2028-2040 over cost_of(m, n), m the x offset, and the flow store
template <class F>
__device__ __forceinline__ void c2f_select_best(float* flow, int x, int y, int ccx, int ccy, int w, int h, F cost_of)
{
    int bx = ccx, by = ccy;
    float min_cost = 999999;
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const int cx = (int)(int16_t)(ccx + m - 1);
        if (cx < 0 || cx >= w) continue;
#pragma unroll
        for (int n = 0; n < 3; n++) {
            const int cy = (int)(int16_t)(ccy + n - 1);
            if (cy < 0 || cy >= h) continue;
            const float cv = cost_of(m, n);
            if (cv < min_cost) { min_cost = cv; bx = cx; by = cy; }
        }
    }
    flow[(y * w + x) * 2] = (float)(bx - x);
    flow[(y * w + x) * 2 + 1] = (float)(by - y);
}

// XCD-aware tile order: workgroups are dealt round robin over the 8 XCDs (b % 8), each with its own L2.
// Give XCD k the k-th contiguous eighth of the row-major tile list so that neighbouring tiles -- which
// share their R-pixel halos and their target windows -- hit the same L2 (speed only, never correctness).
// SPLIT workgroups share a tile (and an XCD): part = which of them this one is (-1: SPLIT 0); false: a padding workgroup, no tile.
template <int SPLIT>
__device__ __forceinline__ bool c2f_tile_origin(const Planes& P, int& x0, int& y0, int& part)
{
    const int tiles_x = (P.w + kBlock - 1) / kBlock, tiles = tiles_x * ((P.h + kBlock - 1) / kBlock);
    const int per_xcd = (tiles + 7) / 8;
    const int slot = SPLIT ? (blockIdx.x >> 3) / SPLIT : (blockIdx.x >> 3);
    part = SPLIT ? (blockIdx.x >> 3) % SPLIT : -1;
    const int tile = (blockIdx.x & 7) * per_xcd + slot;
    if (slot >= per_xcd || tile >= tiles) return false;
    x0 = (tile % tiles_x) * kBlock; y0 = (tile / tiles_x) * kBlock;
    return true;
}

// The source tile of a 16x16 tile kernel: TWU^2 texels (R halo, clamped at load).
// Row stride padded to a multiple of 16 texels (256 B): a ds_read_b128 wave access is served in groups made
// of 8 lanes of one tile row and 8 of the next (MI355X LDS lane groups); with the stride = 0 mod 256 B the two
// halves fall on disjoint banks (34-texel rows cost a 2-way conflict on about every read)
template <int R> struct C2fSrcTile { static constexpr int TWU = kBlock + 2 * R, TW = (TWU + 15) / 16 * 16; };
// The two-phase window refine keeps its per-pixel selection keys and its survivor list in that padding (TW - TWU texels per row, never staged,
// never read by a sample), addressed as one byte space: PADB bytes per row, the 256 8-byte keys in rows [0, KROWS), CAP 2-byte items after them.
template <int R> struct C2fPreList {
    static constexpr int PADB = (C2fSrcTile<R>::TW - C2fSrcTile<R>::TWU) * 16, KROWS = PADB ? (256 * 8 + PADB - 1) / PADB : 0;
    static constexpr int CAP = PADB ? (C2fSrcTile<R>::TWU - KROWS) * (PADB / 2) : 0;
};
// ---------------------------------------------------------------------------------------------------
// The same stage restructured for CDNA4 (bit-identical results).  The reference evaluates the 36
// (candidate, pass) patch costs of a pixel one after the other, re-fetching and re-converting the 100
// source samples 36 times.  Here the sample loop is outermost within a pass: the source texel comes from
// an LDS tile (16x16 + R halo, clamped at load), its conversion and its range term a^2 are computed once
// per sample and shared by the 9 candidates, whose 9 pairs of running sums advance together -- each sum
// still adds its terms in the reference's i-outer/j-inner order.  Target texels are one 16-byte gather each
// (unorm rgb + census).  The passes run 4th to 1st so the reference's nested
// __min(c1,__min(c2,__min(c3,c4))) becomes a running select with the same NaN behaviour.
// ---------------------------------------------------------------------------------------------------
// Affine passes: the target of sample (i,j) is floor(((x+j + uu) + j*A) + i*B) in float (kernel.cu:334-513).
// x+j+uu = cx+j is an integer M, and for every M an image can produce the float sum rounds so that
//   floor(...) = M + floor(fl(fl(j*A) + fl(i*B)))
// (checked exhaustively for -R <= M < 32764 by tests/test_oracle_cpu.py::test_planefit_offsets; the launcher
// falls back to the generic kernel beyond that).  So the warp of a pass is a table of integer offsets
// (dx, dy) per sample and the per-sample float coordinate arithmetic of the reference becomes one integer add.  Along a sample row dy takes at most two consecutive values: the four
// clamped row offsets a row can need are formed once per row and a per-sample flag picks three of them.
struct C2fOff { int dx16, up; };     // dx16 = (j + x-offset) * 16 (bytes); up = 1 if this sample's dy is the row minimum + 1

template <int R>
struct C2fTables {
    static constexpr int S = R + 1;
    C2fOff off[3][S * S];             // passes 1..3
    int rowdy[3][S];                  // i + min over the row of the y-offset
};

// The tables depend only on the radius and on the reference's coefficients: they are compile-time constants in
// __constant__ memory (k_c2f_refine.hip).  Their index is wave-uniform, so they arrive through the scalar cache (s_load) and cost
// no vector instruction; `up` steers a scalar branch.
constexpr int cfloor(float v) { const int t = (int)v; return ((float)t > v) ? t - 1 : t; }
template <int R>
constexpr C2fTables<R> make_c2f_tables()
{
    constexpr int S = R + 1;
    constexpr float kc[3][4] = {
        {0.177f, -0.011f, -0.003f, 0.301f},
        {0.125f, -0.357f, 0.009f, 0.308f},
        {0.205f, 0.370f, 0.011f, 0.296f},
    };
    C2fTables<R> T{};
    for (int p = 0; p < 3; p++)
        for (int ii = 0; ii < S; ii++) {
            const int i = 2 * ii - R;
            int dy[S] = {};
            int lo = 1 << 30;
            for (int jj = 0; jj < S; jj++) {
                const int j = 2 * jj - R;
                const float fx = (float)(j)*kc[p][0] + (float)(i)*kc[p][1];
                const float fy = (float)(j)*kc[p][2] + (float)(i)*kc[p][3];
                T.off[p][ii * S + jj].dx16 = (j + cfloor(fx)) * 16;
                dy[jj] = i + cfloor(fy);
                lo = dy[jj] < lo ? dy[jj] : lo;
            }
            T.rowdy[p][ii] = lo;
            for (int jj = 0; jj < S; jj++) T.off[p][ii * S + jj].up = dy[jj] - lo;      // 0 or 1
        }
    return T;
}
template <int R> __device__ __forceinline__ const C2fTables<R>& c2f_tables();         // radius 9 and 17: k_c2f_refine.hip

// ---------------------------------------------------------------------------------------------------
// The LDS window of the target image (k_c2f_refine_win, radius 9: two pass groups; k_c2f_refine_win4, radius 17: four): WH rows of
// WW texels.  A read lands at window column (cx + dx) - wx0 with cx in [mnx-1, mxx+1], dx in [XLO, XHI] and wx0 = mnx - 1 + XLO, i.e.
// at most (mxx - mnx) + 2 + (XHI - XLO), which must stay <= WW - 1 (rows likewise): SPAN_X, SPAN_Y are the admissible spread
// (max - min) of a tile's candidate centres.
// ---------------------------------------------------------------------------------------------------
template <int R>
struct C2fWinShape {
    // extreme sample offsets over all four passes (pass 0: the plain +-R grid)
    static constexpr int xlo() { int v = -R; const auto T = make_c2f_tables<R>(); for (int p = 0; p < 3; p++) for (int t = 0; t < (R + 1) * (R + 1); t++) v = T.off[p][t].dx16 / 16 < v ? T.off[p][t].dx16 / 16 : v; return v; }
    static constexpr int xhi() { int v = R; const auto T = make_c2f_tables<R>(); for (int p = 0; p < 3; p++) for (int t = 0; t < (R + 1) * (R + 1); t++) v = T.off[p][t].dx16 / 16 > v ? T.off[p][t].dx16 / 16 : v; return v; }
    static constexpr int ylo() { int v = -R; const auto T = make_c2f_tables<R>(); for (int p = 0; p < 3; p++) for (int i = 0; i <= R; i++) v = T.rowdy[p][i] < v ? T.rowdy[p][i] : v; return v; }
    static constexpr int yhi() { int v = R; const auto T = make_c2f_tables<R>(); for (int p = 0; p < 3; p++) for (int i = 0; i <= R; i++) v = T.rowdy[p][i] + 1 > v ? T.rowdy[p][i] + 1 : v; return v; }
    static constexpr int XLO = xlo(), XHI = xhi(), YLO = ylo(), YHI = yhi();
    // radius 9: row stride 64 texels = 1 KiB (conflict-free ds_read_b128); larger: >= 8 px of admissible flow spread, row stride a multiple of 256 B
    static constexpr int WW = (R == 9) ? 64 : (kBlock + 2 + (XHI - XLO) + 8 + 15) / 16 * 16;
    static constexpr int WH = (R == 9) ? EPPM_C2F_WIN_H : kBlock + 2 + (YHI - YLO) + 7;
    static constexpr int SPAN_X = WW - 3 - (XHI - XLO), SPAN_Y = WH - 3 - (YHI - YLO);
    static_assert(SPAN_X >= kBlock - 1 && SPAN_Y >= kBlock - 1, "window too small for a constant-flow tile (spread kBlock - 1)");
};

// ---------------------------------------------------------------------------------------------------
// One (sample, target) term of a patch cost.  C2fSample is the source half, formed once per sample for all the targets it meets.
// ---------------------------------------------------------------------------------------------------
#ifdef EPPM_TOL
struct C2fSample { rgbf p1; uint32_t k1; float lsrc; };         // lsrc: log2 of the source half of the weight
__device__ __forceinline__ rgbf c2f_weight_centre(const rgbf c) { return tol_scale_centre(c); }
template <class LUT>
__device__ __forceinline__ C2fSample c2f_sample(const LUT& L, const rgbf c1, const float4 q1, int t)
{
    const rgbf p1 = texel_rgb(q1);
    const uint32_t k1 = __float_as_uint(q1.w);
    return {p1, k1, tol_exp_arg_scaled(c1, p1, L.gsp[t])};      // L.gsp: log2(gs_j gs_i), load_patch_lut<true>
}
template <class LUT>
__device__ __forceinline__ void c2f_term(const LUT& L, const C2fSample& s, const rgbf c2, const float4 q2, float& cs, float& ws)
{
    const rgbf p2 = texel_rgb(q2);
    const float cost = tol_cost(L.tab(), s.p1, p2, s.k1, __float_as_uint(q2.w));
    patch_accum(cs, ws, cost, __builtin_amdgcn_exp2f(tol_exp_arg_scaled(c2, p2, s.lsrc)));
}
#else
struct C2fSample { rgbf p1; uint32_t k1; float a2, gsp; };      // a2: the range term of the source half, squared
__device__ __forceinline__ rgbf c2f_weight_centre(const rgbf c) { return c; }
template <class LUT>
__device__ __forceinline__ C2fSample c2f_sample(const LUT& L, const rgbf c1, const float4 q1, int t)
{
    const rgbf p1 = texel_rgb(q1);
    const uint32_t k1 = __float_as_uint(q1.w);
    float a2 = max_abs_diff(c1, p1);
    a2 *= a2;
    return {p1, k1, a2, L.gsp[t]};
}
template <class LUT>
__device__ __forceinline__ void c2f_term(const LUT& L, const C2fSample& s, const rgbf c2, const float4 q2, float& cs, float& ws)
{
    const rgbf p1 = s.p1, p2 = texel_rgb(q2);
    float cost = max_abs_diff(p1, p2);
    cost = EPPM_DELTA_PATCH ? delta_lookup(L.D, cost) : one_minus_fast_exp(div_ad2(-(cost * cost)));      // the same bits either way (eppm_device.cuh: DeltaTab)
    cost += census_cost(L.cnx, s.k1, __float_as_uint(q2.w));
    float temp = max_abs_diff(c2, p2);
    temp *= temp;
    float weight = fast_exp(div_ad2(-(s.a2 + temp)));
    weight *= s.gsp;
    cost *= weight;
    cs += cost;
    ws += weight;
}
#endif

// The N terms of one sample, term k with the centre c2[k], the target texel q2[k] and the sums (cs[k], ws[k]).
// They are written in PHASES across the terms -- the distances, the data term's first-level reads, the census reads, the second-level
// reads, the weights, the accumulation (tolerance library: offsets and exponent arguments, td[] reads, cn[] reads, exponentials,
// accumulation) -- so that the order of the source already is the interleaved schedule: N LDS round trips in flight together and N
// exponent polynomials side by side.  Term by term (N x c2f_term) the scheduler has to find that order itself, and where its attempt
// does not fit the kernel's register budget it keeps the source order: passes 4/3 of k_c2f_refine_win<9> ran one term after the other,
// each waiting out two LDS round trips of its own (profiles/refine_schedule_isa.txt; DESIGN.md section 8 rows 51-55 for the forms that
// were measured and not kept).  Every term is c2f_term operation for operation, and a sum receives its terms in the same order: the
// same bits.
template <int N, class LUT>
__device__ __forceinline__ void c2f_terms(const LUT& L, const C2fSample& s, const rgbf (&c2)[N], const float4 (&q2)[N], float (&cs)[N], float (&ws)[N])
{
#if !defined(EPPM_TOL) && !EPPM_DELTA_PATCH
#pragma unroll
    for (int k = 0; k < N; k++) c2f_term(L, s, c2[k], q2[k], cs[k], ws[k]);
#elif defined(EPPM_TOL)
    uint32_t od[N], oc[N];
    float arg[N], cost[N], cen[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const rgbf p2 = texel_rgb(q2[k]);
        od[k] = linf_off(s.p1, p2);
        oc[k] = (uint32_t)__builtin_popcount(s.k1 ^ __float_as_uint(q2[k].w));
        arg[k] = tol_exp_arg_scaled(c2[k], p2, s.lsrc);
    }
#pragma unroll
    for (int k = 0; k < N; k++) cost[k] = tol_at(L.tab().td, od[k]);
#pragma unroll
    for (int k = 0; k < N; k++) cen[k] = tol_at(L.tab().cn, oc[k]);
#pragma unroll
    for (int k = 0; k < N; k++) arg[k] = __builtin_amdgcn_exp2f(arg[k]);
#pragma unroll
    for (int k = 0; k < N; k++) patch_accum(cs[k], ws[k], cost[k] + cen[k], arg[k]);
#else
    float d[N], temp[N], cen[N], cost[N], weight[N];
    uint32_t t1[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const rgbf p2 = texel_rgb(q2[k]);
        d[k] = max_abs_diff(s.p1, p2);
        temp[k] = max_abs_diff(c2[k], p2);
    }
#pragma unroll
    for (int k = 0; k < N; k++) t1[k] = delta_lookup_l1(L.D, d[k]);
#pragma unroll
    for (int k = 0; k < N; k++) cen[k] = census_cost(L.cnx, s.k1, __float_as_uint(q2[k].w));
#pragma unroll
    for (int k = 0; k < N; k++) cost[k] = delta_lookup_l2(d[k], t1[k]);
#pragma unroll
    for (int k = 0; k < N; k++) {
        temp[k] *= temp[k];
        weight[k] = fast_exp(div_ad2(-(s.a2 + temp[k])));
        weight[k] *= s.gsp;
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        cost[k] += cen[k];
        cost[k] *= weight[k];
        cs[k] += cost[k];
        ws[k] += weight[k];
    }
#endif
}

// One affine pass (PASS 0: the plain grid) of the candidates (cx, ccy-1), (cx, ccy), (cx, ccy+1): one x offset m, the three y offsets n.
// run: the running minimum over the passes, or (RAW, or the first pass run: PASS 3) this pass's cost.
// WIN: the target texels come from an LDS window of the target image instead of per-lane gathers (k_c2f_refine_win):
// `s_win` is the window (row stride WW texels, cells pre-clamped to the image at load), `wbase` this lane's byte offset of
// candidate (cx, ccy-1) with zero sample offset.  The sample's offset is a scalar, the three row candidates are WW texels apart.
template <int R, int PASS, bool RAW = false, bool WIN = false, int WW = 0>
__device__ __forceinline__ void c2f_pass(const Planes& P, const PatchLutT<R + 1>& L, const float4* __restrict__ s_src,
                                         int TW, int tx, int ty, int cx16, int wmax16, int ccy, const rgbf c1, const rgbf (&c2)[3], float (&run)[3],
                                         const float4* __restrict__ s_win = nullptr, int wbase = 0)
{
    constexpr int S = R + 1;
    constexpr int TP = (PASS == 0) ? 0 : PASS - 1;
    const C2fTables<R>& T = c2f_tables<R>();
    const rgbf c1w = c2f_weight_centre(c1), c2w[3] = {c2f_weight_centre(c2[0]), c2f_weight_centre(c2[1]), c2f_weight_centre(c2[2])};
    float cs[3] = {0.0f, 0.0f, 0.0f}, ws[3] = {0.0f, 0.0f, 0.0f};
    const unsigned pitch16 = (unsigned)P.pitch << 4;
#pragma unroll 1
    for (int ii = 0; ii < S; ii++) {
        // clamped row offsets of the targets: rows ccy-1+dy .. ccy+1+dy (+1 more where dy steps inside the row)
        unsigned Rr[4];
        const int rdy = (PASS == 0) ? 2 * ii - R : T.rowdy[TP][ii];
        const int rb = ccy - 1 + rdy;
        if (!WIN) {
#pragma unroll
            for (int k = 0; k < 4; k++) Rr[k] = __umul24((unsigned)iclamp(rb + k, 0, P.h - 1), pitch16);
        }
EPPM_UNROLL(EPPM_C2F_UNROLL)
        for (int jj = 0; jj < S; jj++) {
            const C2fSample smp = c2f_sample(L, c1w, s_src[(ty + 2 * ii) * TW + tx + 2 * jj], ii * S + jj);
            // byte offsets of the three targets: clamped column (in bytes throughout: no shift) + clamped rows
            const int dx16 = (PASS == 0) ? (2 * jj - R) * 16 : T.off[TP][ii * S + jj].dx16;
            float4 q2[3];                                 // the three gathers are issued back to back, then consumed
            if (WIN) {
                // one vector add (lane base + scalar sample offset), three LDS reads with immediate row offsets
                const int soff = (rdy + ((PASS != 0) ? T.off[TP][ii * S + jj].up : 0)) * (WW * 16) + dx16;
                const char* wp = reinterpret_cast<const char*>(s_win) + (wbase + soff);
#pragma unroll
                for (int n = 0; n < 3; n++) q2[n] = *reinterpret_cast<const float4*>(wp + n * (WW * 16));
            } else {
                const unsigned Xb = (unsigned)med3i(cx16 + dx16, 0, wmax16);
                if (PASS != 0 && T.off[TP][ii * S + jj].up) {         // wave-uniform; compiles to three selects on a scalar condition
#pragma unroll
                    for (int n = 0; n < 3; n++) q2[n] = texel_at(P.pk2, Rr[n + 1] + Xb);
                } else {
#pragma unroll
                    for (int n = 0; n < 3; n++) q2[n] = texel_at(P.pk2, Rr[n] + Xb);
                }
            }
#pragma unroll
            for (int n = 0; n < 3; n++) c2f_term(L, smp, c2w[n], q2[n], cs[n], ws[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < 3; n++) {
        const float c = cs[n] / ws[n];
        run[n] = (RAW || PASS == 3) ? c : c2f_min(c, run[n]);
    }
}

// Two affine passes of one candidate column evaluated together from the LDS window: the source sample, its range term a^2 and
// the spatial weight are formed once per sample for the 6 (pass, row candidate) terms, which are evaluated together (c2f_terms); each
// of the 6 pairs of running sums still adds its terms in the reference's sample order.  outA / outB: raw costs of pass PA / PB for the
// three row candidates.
template <int R, int PA, int PB, int WW>
__device__ __forceinline__ void c2f_pass2_win(const PatchLutT<R + 1>& L, const float4* __restrict__ s_src, int TW, int tx, int ty,
                                              const rgbf c1, const rgbf (&c2)[3], const float4* __restrict__ s_win, int wbase,
                                              float (&outA)[3], float (&outB)[3])
{
    constexpr int S = R + 1;
    constexpr int TA = (PA == 0) ? 0 : PA - 1, TB = (PB == 0) ? 0 : PB - 1;
    const C2fTables<R>& T = c2f_tables<R>();
    const rgbf c1w = c2f_weight_centre(c1), c2w[3] = {c2f_weight_centre(c2[0]), c2f_weight_centre(c2[1]), c2f_weight_centre(c2[2])};
    const rgbf c2w6[6] = {c2w[0], c2w[1], c2w[2], c2w[0], c2w[1], c2w[2]};
    float cs[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, ws[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // pass PA's three row candidates, then pass PB's
#pragma unroll 1
    for (int ii = 0; ii < S; ii++) {
        const int rdyA = (PA == 0) ? 2 * ii - R : T.rowdy[TA][ii];
        const int rdyB = (PB == 0) ? 2 * ii - R : T.rowdy[TB][ii];
EPPM_UNROLL(EPPM_C2F_UNROLL)
        for (int jj = 0; jj < S; jj++) {
            const C2fSample smp = c2f_sample(L, c1w, s_src[(ty + 2 * ii) * TW + tx + 2 * jj], ii * S + jj);
            const int soffA = (rdyA + ((PA != 0) ? T.off[TA][ii * S + jj].up : 0)) * (WW * 16) + ((PA == 0) ? (2 * jj - R) * 16 : T.off[TA][ii * S + jj].dx16);
            const int soffB = (rdyB + ((PB != 0) ? T.off[TB][ii * S + jj].up : 0)) * (WW * 16) + ((PB == 0) ? (2 * jj - R) * 16 : T.off[TB][ii * S + jj].dx16);
            const char* wa = reinterpret_cast<const char*>(s_win) + (wbase + soffA);
            const char* wb = reinterpret_cast<const char*>(s_win) + (wbase + soffB);
            float4 q[6];
#pragma unroll
            for (int n = 0; n < 3; n++) { q[n] = *reinterpret_cast<const float4*>(wa + n * (WW * 16)); q[3 + n] = *reinterpret_cast<const float4*>(wb + n * (WW * 16)); }
            c2f_terms<6>(L, smp, c2w6, q, cs, ws);
        }
    }
#pragma unroll
    for (int n = 0; n < 3; n++) { outA[n] = cs[n] / ws[n]; outB[n] = cs[3 + n] / ws[3 + n]; }
}

#ifndef EPPM_TOL
// ---- the two-phase form of k_c2f_refine_win ----
// c2f_pass2_win over the sample rows [I0, I1) only and for NC row candidates (3: a candidate column, 1: one candidate), the sums left
// undivided: cs / ws [0, NC) of pass PA, [NC, 2 NC) of pass PB.  All rows: c2f_pass2_win's sums, term for term and in its order.
template <int R, int PA, int PB, int WW, int I0, int I1, int NC>
__device__ __forceinline__ void c2f_rows2_win(const PatchLutT<R + 1>& L, const float4* __restrict__ s_src, int TW, int tx, int ty,
                                              const rgbf c1, const rgbf (&c2)[NC], const float4* __restrict__ s_win, int wbase,
                                              float (&cs)[2 * NC], float (&ws)[2 * NC])
{
    constexpr int S = R + 1;
    constexpr int TA = (PA == 0) ? 0 : PA - 1, TB = (PB == 0) ? 0 : PB - 1;
    const C2fTables<R>& T = c2f_tables<R>();
    const rgbf c1w = c2f_weight_centre(c1);
    rgbf c2w[2 * NC];
#pragma unroll
    for (int n = 0; n < NC; n++) { c2w[n] = c2f_weight_centre(c2[n]); c2w[NC + n] = c2w[n]; }
#pragma unroll
    for (int n = 0; n < 2 * NC; n++) { cs[n] = 0.0f; ws[n] = 0.0f; }
#pragma unroll 1
    for (int ii = I0; ii < I1; ii++) {
        const int rdyA = (PA == 0) ? 2 * ii - R : T.rowdy[TA][ii];
        const int rdyB = (PB == 0) ? 2 * ii - R : T.rowdy[TB][ii];
EPPM_UNROLL(EPPM_C2F_UNROLL)
        for (int jj = 0; jj < S; jj++) {
            const C2fSample smp = c2f_sample(L, c1w, s_src[(ty + 2 * ii) * TW + tx + 2 * jj], ii * S + jj);
            const int soffA = (rdyA + ((PA != 0) ? T.off[TA][ii * S + jj].up : 0)) * (WW * 16) + ((PA == 0) ? (2 * jj - R) * 16 : T.off[TA][ii * S + jj].dx16);
            const int soffB = (rdyB + ((PB != 0) ? T.off[TB][ii * S + jj].up : 0)) * (WW * 16) + ((PB == 0) ? (2 * jj - R) * 16 : T.off[TB][ii * S + jj].dx16);
            const char* wa = reinterpret_cast<const char*>(s_win) + (wbase + soffA);
            const char* wb = reinterpret_cast<const char*>(s_win) + (wbase + soffB);
            float4 q[2 * NC];
#pragma unroll
            for (int n = 0; n < NC; n++) { q[n] = *reinterpret_cast<const float4*>(wa + n * (WW * 16)); q[NC + n] = *reinterpret_cast<const float4*>(wb + n * (WW * 16)); }
            c2f_terms<2 * NC>(L, smp, c2w, q, cs, ws);
        }
    }
}

// one affine pass of one candidate from the LDS window, all samples in the reference's order: its cost
template <int R, int PASS, int WW>
__device__ __forceinline__ float c2f_one_win(const PatchLutT<R + 1>& L, const float4* __restrict__ s_src, int TW, int tx, int ty,
                                             const rgbf c1, const rgbf c2, const float4* __restrict__ s_win, int wbase)
{
    constexpr int S = R + 1;
    constexpr int TP = (PASS == 0) ? 0 : PASS - 1;
    const C2fTables<R>& T = c2f_tables<R>();
    const rgbf c1w = c2f_weight_centre(c1), c2w[1] = {c2f_weight_centre(c2)};
    float cs[1] = {0.0f}, ws[1] = {0.0f};
#pragma unroll 1
    for (int ii = 0; ii < S; ii++) {
        const int rdy = (PASS == 0) ? 2 * ii - R : T.rowdy[TP][ii];
EPPM_UNROLL(EPPM_C2F_UNROLL)
        for (int jj = 0; jj < S; jj++) {
            const C2fSample smp = c2f_sample(L, c1w, s_src[(ty + 2 * ii) * TW + tx + 2 * jj], ii * S + jj);
            const int soff = (rdy + ((PASS != 0) ? T.off[TP][ii * S + jj].up : 0)) * (WW * 16) + ((PASS == 0) ? (2 * jj - R) * 16 : T.off[TP][ii * S + jj].dx16);
            const float4 q[1] = {*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + (wbase + soff))};
            c2f_terms<1>(L, smp, c2w, q, cs, ws);
        }
    }
    return cs[0] / ws[0];
}
#endif

}  // namespace eppm
