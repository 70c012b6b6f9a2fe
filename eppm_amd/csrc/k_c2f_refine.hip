// k_c2f_refine.hip -- coarse-to-fine step, the plane-fitting candidate refine (reference: bao_pmflow_kernel.cu:2005-2041): the
// any-radius kernel, the tile kernels of radius 9 and 17 (gathers, or an LDS window of the target), the split launch's select.
// The passes and the patch term they evaluate: c2f_device.cuh.
#include <type_traits>

#include "c2f_device.cuh"
#include "eppm_internal.h"

namespace eppm {

__constant__ C2fTables<9> c2f_tab9 = make_c2f_tables<9>();
__constant__ C2fTables<17> c2f_tab17 = make_c2f_tables<17>();
template <> __device__ __forceinline__ const C2fTables<9>& c2f_tables<9>() { return c2f_tab9; }
template <> __device__ __forceinline__ const C2fTables<17>& c2f_tables<17>() { return c2f_tab17; }

// kernel.cu:2005-2041 as written, any radius
__global__ __launch_bounds__(256) void k_c2f_refine(PlanesH Ph, float* __restrict__ flow_, const float* __restrict__ lut, int R, size_t pstride)
{
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    load_patch_lut(L, lut, R, threadIdx.y * kBlock + threadIdx.x, 256);
    __syncthreads();
    const Planes P = to_dev(Ph, pstride, blockIdx.z);
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.z);
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const float fvx = flow[(y * P.w + x) * 2], fvy = flow[(y * P.w + x) * 2 + 1];
    if (c2f_unknown(fvx, fvy)) { c2f_store_flow(flow, y * P.w + x, 0, 0); return; }
    const int ccx = c2f_centre(fvx, x), ccy = c2f_centre(fvy, y);
    int bx = ccx, by = ccy;
    float min_cost = 999999;
#pragma unroll 1
    for (int m = 0; m < 3; m++) {
        const int cx = (int)(int16_t)(ccx + m - 1);
#pragma unroll 1
        for (int n = 0; n < 3; n++) {
            const int cy = (int)(int16_t)(ccy + n - 1);
            if (cx < 0 || cy < 0 || cx >= P.w || cy >= P.h) continue;
            const float cv = patch_dist_planefit(P, L, R, x, y, cx, cy);
            if (cv < min_cost) { min_cost = cv; bx = cx; by = cy; }
        }
    }
    flow[(y * P.w + x) * 2] = (float)(bx - x);
    flow[(y * P.w + x) * 2 + 1] = (float)(by - y);
}

// The tile kernel (c2f_device.cuh: c2f_pass), target texels gathered.
// SPLIT: a launch with few tiles (fewer than 256: under one wave per SIMD) does not fill the chip and runs latency bound.
// Then a tile is given to 3 workgroups (one candidate column m each) or to 4 (one affine pass
// each), whichever divides more evenly over the 256 CUs; the costs of a pixel (9 x 4 passes) go to a scratch plane and
// k_c2f_select replays the reference's nested minimum and candidate loop.  Same costs, same selection order.
template <int R, int SPLIT>
__global__ __launch_bounds__(256) EPPM_C2F_OCC void k_c2f_refine_tiled(PlanesH Ph, float* __restrict__ flow_, const float* __restrict__ lut,
                                                                       float* __restrict__ cost9_, size_t pstride)
{
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.y);             // blockIdx.y = pair of the batch
    float* __restrict__ cost9 = pair_ptr_opt(cost9_, pstride, blockIdx.y);
    constexpr int TWU = C2fSrcTile<R>::TWU, TW = C2fSrcTile<R>::TW;
    __shared__ EPPM_LUT_ALIGN PatchLutT<R + 1> L;
    __shared__ float4 s_src[TWU * TW];
    const int tid = threadIdx.y * kBlock + threadIdx.x;
    load_patch_lut<EPPM_C2F_LOG2>(L, lut, R, tid, 256);
    const Planes P = to_dev(Ph, pstride, blockIdx.y);
    int x0, y0, part;
    if (!c2f_tile_origin<SPLIT>(P, x0, y0, part)) return;
    const int m_only = (SPLIT == 3) ? part : -1;
    for (int t = tid; t < TWU * TWU; t += 256) {
        const int ry = t / TWU, rx = t % TWU;
        const int sy = iclamp(y0 + ry - R, 0, P.h - 1), sx = iclamp(x0 + rx - R, 0, P.w - 1);
        s_src[ry * TW + rx] = P.pk1[(unsigned)(sy * P.pitch + sx)];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const float fvx = flow[(y * P.w + x) * 2], fvy = flow[(y * P.w + x) * 2 + 1];
    if (c2f_unknown(fvx, fvy)) {
        if (SPLIT == 0) c2f_store_flow(flow, y * P.w + x, 0, 0);
        return;
    }
    const int ccx = c2f_centre(fvx, x), ccy = c2f_centre(fvy, y);
    const rgbf c1 = texel_rgb(s_src[(threadIdx.y + R) * TW + threadIdx.x + R]);
    // the candidate loop with a column's three costs formed together (and SPLIT's exits), hence not c2f_select_best
    int bx = ccx, by = ccy;
    float min_cost = 999999;
#pragma unroll 1
    for (int m = 0; m < 3; m++) {                    // x offset outer, as the reference's candidate loop (kernel.cu:2028)
        if (SPLIT == 3 && m != m_only) continue;
        const int cx = (int)(int16_t)(ccx + m - 1);
        if (cx < 0 || cx >= P.w) continue;           // every candidate of this column is skipped (:2030)
        rgbf c2[3];
#pragma unroll
        for (int n = 0; n < 3; n++) c2[n] = texel_rgb(tex_px(P.pk2, P.pitch, P.w, P.h, cx, ccy + n - 1));
        float run[3];
        const int cx16 = cx << 4, wmax16 = (P.w - 1) << 4;
        if (SPLIT == 4) {                            // this workgroup's pass only, raw cost
            if (part == 3) c2f_pass<R, 3, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
            else if (part == 2) c2f_pass<R, 2, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
            else if (part == 1) c2f_pass<R, 1, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
            else c2f_pass<R, 0, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
#pragma unroll
            for (int n = 0; n < 3; n++) cost9[(size_t)(y * P.w + x) * 36 + part * 9 + m * 3 + n] = run[n];
            continue;
        }
        c2f_pass<R, 3>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
        c2f_pass<R, 2>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
        c2f_pass<R, 1>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
        c2f_pass<R, 0>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
        if (SPLIT == 3) {
#pragma unroll
            for (int n = 0; n < 3; n++) cost9[(size_t)(y * P.w + x) * 36 + m * 3 + n] = run[n];      // nested minimum already formed
            continue;
        }
#pragma unroll
        for (int n = 0; n < 3; n++) {
            const int cy = (int)(int16_t)(ccy + n - 1);
            if (cy < 0 || cy >= P.h) continue;
            const float cv = run[n];
            if (cv < min_cost) { min_cost = cv; bx = cx; by = cy; }
        }
    }
    if (SPLIT != 0) return;
    flow[(y * P.w + x) * 2] = (float)(bx - x);
    flow[(y * P.w + x) * 2 + 1] = (float)(by - y);
}

// ---------------------------------------------------------------------------------------------------
// The same tile kernel with the TARGET texels staged in LDS as well.  After up-sampling, the flow of a 16x16 tile is
// nearly constant, so the 3 600 target texels a pixel reads (9 candidates x 4 passes x 100 samples) and those of its
// 255 neighbours fall into one small window of the target image: (tile + flow spread) + candidate +-1 + the sample and
// warp offsets.  A workgroup whose candidate centres span at most SPAN_X x SPAN_Y pixels (C2fWinShape) loads that window once
// (rows clamped to the image at load, like the source tile) and every target fetch becomes ONE vector add and an LDS read
// with an immediate offset -- no clamps, no per-candidate address arithmetic, no gather round trips through the texture
// path (the 16-byte gathers kept its addresser ~58 % busy).  A tile whose flow is not coherent enough (motion boundaries)
// takes the per-access path of k_c2f_refine_tiled inside the same workgroup.  Same arithmetic, same order: bit-identical.
//
// Workgroup = 512 threads = the 256 pixels of the tile x 2 pass groups (threadIdx.z): group 0 evaluates the 4th and 3rd affine
// pass of every candidate, group 1 the 2nd and the 1st; both read the same source tile and target window, so the LDS footprint
// (78 KB) is shared by twice the waves: two workgroups per CU = 4 waves per SIMD (the one-group form ran at 2 and was 10 %
// slower than the gather kernel).  Group 0 hands its nested minimum of passes 4 and 3 to group 1 through LDS (the source
// tile's storage, after a barrier), which finishes __min(c1,__min(c2,.)) and the candidate loop.
// ---------------------------------------------------------------------------------------------------
// PROBE (test support): the same kernel, which also writes the pre-test's N, D_A and U of every known pixel of a two-phase tile to `probe`
// (73 floats per pixel, pair after pair: N[pass][candidate], D_A[pass][candidate], U), so that the tests compare the sums the kernel itself forms.
template <int R, bool PROBE = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(EPPM_C2F_WIN_WAVES, EPPM_C2F_WIN_WAVES)))
void k_c2f_refine_win(PlanesH Ph, float* __restrict__ flow_, const float* __restrict__ lut, size_t pstride, int pre, unsigned* __restrict__ stat,
                      float* __restrict__ probe)
{
    using W = C2fWinShape<R>;
    constexpr int TWU = C2fSrcTile<R>::TWU, TW = C2fSrcTile<R>::TW, WW = W::WW, WH = W::WH;
    static_assert(TWU * TW * 16 >= 9 * 256 * 4, "the exchange buffer aliases the source tile");
    __shared__ EPPM_LUT_ALIGN PatchLutT<R + 1> L;
    __shared__ float4 s_src[TWU * TW];
    __shared__ float4 s_win[WH * WW];
    __shared__ int s_mm[4];                                          // min ccx, max ccx, min ccy, max ccy of the tile's pixels
#ifndef EPPM_TOL
    __shared__ int s_pre[1];                                         // two-phase form: a weight sum of the tile is too small
#endif
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.y);
    const int ptid = threadIdx.y * kBlock + threadIdx.x;            // pixel of the tile
    const int grp = threadIdx.z;                                     // pass group
    const int tid = grp * 256 + ptid;
    load_patch_lut<EPPM_C2F_LOG2>(L, lut, R, tid, 512);
    const Planes P = to_dev(Ph, pstride, blockIdx.y);
    const uint32_t* __restrict__ pc1 = pair_ptr_opt(Ph.pc1, pstride, blockIdx.y);
    const uint32_t* __restrict__ pc2 = pair_ptr_opt(Ph.pc2, pstride, blockIdx.y);
    int x0, y0, part;
    if (!c2f_tile_origin<0>(P, x0, y0, part)) return;
    if (tid == 0) { s_mm[0] = 0x7fffffff; s_mm[1] = -0x7fffffff; s_mm[2] = 0x7fffffff; s_mm[3] = -0x7fffffff; }
#ifndef EPPM_TOL
    if (tid == 0) s_pre[0] = 0;
#endif
    for (int t = tid; t < TWU * TWU; t += 512) {
        const int ry = t / TWU, rx = t % TWU;
        const int sy = iclamp(y0 + ry - R, 0, P.h - 1), sx = iclamp(x0 + rx - R, 0, P.w - 1);
        s_src[ry * TW + rx] = stage_texel(pc1, P.pk1, (unsigned)(sy * P.pitch + sx));
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inimg = (x < P.w && y < P.h);
    float fvx = 0.0f, fvy = 0.0f;
    if (inimg) { fvx = flow[(y * P.w + x) * 2]; fvy = flow[(y * P.w + x) * 2 + 1]; }
    const bool known = inimg && !(fvx > kUnknownFlowThresh || fvy > kUnknownFlowThresh);
    const int ccx = c2f_centre(fvx, x), ccy = c2f_centre(fvy, y);
    if (known && grp == 0) {
        atomicMin(&s_mm[0], ccx); atomicMax(&s_mm[1], ccx);
        atomicMin(&s_mm[2], ccy); atomicMax(&s_mm[3], ccy);
    }
    __syncthreads();
    const int mnx = s_mm[0], mxx = s_mm[1], mny = s_mm[2], mxy = s_mm[3];
    const bool coherent = (mxx - mnx <= W::SPAN_X) && (mxy - mny <= W::SPAN_Y);       // workgroup-uniform (no known pixel: mxx < mnx, nobody reads)
    const int wx0 = mnx - 1 + W::XLO, wy0 = mny - 1 + W::YLO;
    if (coherent && mxx >= mnx) {
        for (int t = tid; t < WH * WW; t += 512) {
            const int sy = iclamp(wy0 + t / WW, 0, P.h - 1), sx = iclamp(wx0 + t % WW, 0, P.w - 1);
            s_win[t] = stage_texel(pc2, P.pk2, (unsigned)(sy * P.pitch + sx));
        }
    }
    __syncthreads();
#ifndef EPPM_TOL
    // ---- the two-phase form of a coherent tile; every branch that holds a barrier is workgroup-uniform ----
    int path = 3;                                    // statistics: 0 two-phase, 1 a weight sum too small, 2 list drained in parts (EPPM_C2F_PRE_PARTS 0: list full), 3 one-phase as before
    if (pre && coherent && mxx >= mnx) {
        constexpr int S = R + 1, I0 = (S - EPPM_C2F_PRE_ROWS) / 2, I1 = I0 + EPPM_C2F_PRE_ROWS;
        // The row padding of the source tile (TW - TWU texels per row, never staged, never read by a sample) carries the per-pixel
        // selection keys (rows [0, KROWS)) and the survivor list (the other rows): byte o of that space.
        constexpr int PADB = C2fPreList<R>::PADB, KROWS = C2fPreList<R>::KROWS, CAP = C2fPreList<R>::CAP;
        static_assert(PADB % 8 == 0 && PADB > 0 && KROWS < TWU, "keys and items do not straddle a row's padding");
        auto pad = [&](int o) -> char* { return reinterpret_cast<char*>(s_src) + (o / PADB) * (TW * 16) + TWU * 16 + (o % PADB); };
        auto key_at = [&](int p) -> unsigned long long* { return reinterpret_cast<unsigned long long*>(pad(p * 8)); };
        auto item_at = [&](int i) -> uint16_t* { return reinterpret_cast<uint16_t*>(pad(KROWS * PADB + i * 2)); };
        const int lane = tid & 63;
        // 1. pre-test: N = sum_A c_k w_k and D_A = sum_A w_k of this lane's 2 passes x 9 candidates ([0, 9): pass 3 (group 0) or 1,
        // [9, 18): pass 2 or 0), U = the pixel's rest weight
        float N[18], D[18], U = 0.0f;
        unsigned vmask = 0;                          // bit k: candidate k = m * 3 + n lies in the image
        rgbf c1 = {0.0f, 0.0f, 0.0f};
        if (known) {
            c1 = texel_rgb(s_src[(threadIdx.y + R) * TW + threadIdx.x + R]);
#pragma unroll 1
            for (int ii = 0; ii < S; ii++) {
                if (ii >= I0 && ii < I1) continue;
                const float4* __restrict__ srow = s_src + (threadIdx.y + 2 * ii) * TW + threadIdx.x;
#pragma unroll
                for (int jj = 0; jj < S; jj++) U += rest_weight_term(c1, srow[2 * jj], L.gsp[ii * S + jj]);
            }
        }
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const int cx = (int)(int16_t)(ccx + m - 1);
            float cs[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, ws[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (known && !(cx < 0 || cx >= P.w)) {
                const int wbase = ((ccy - 1 - wy0) * WW + (cx - wx0)) * 16;
                rgbf c2[3];
#pragma unroll
                for (int n = 0; n < 3; n++) {
                    c2[n] = texel_rgb(*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + wbase + n * (WW * 16)));
                    const int cy = (int)(int16_t)(ccy + n - 1);
                    if (!(cy < 0 || cy >= P.h)) vmask |= 1u << (m * 3 + n);
                }
                if (grp == 0) c2f_rows2_win<R, 3, 2, WW, I0, I1, 3>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, cs, ws);
                else c2f_rows2_win<R, 1, 0, WW, I0, I1, 3>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, cs, ws);
            }
#pragma unroll
            for (int n = 0; n < 3; n++) { N[m * 3 + n] = cs[n]; D[m * 3 + n] = ws[n]; N[9 + m * 3 + n] = cs[3 + n]; D[9 + m * 3 + n] = ws[3 + n]; }
        }
        if (PROBE && known) {
            float* __restrict__ pp = probe + ((size_t)blockIdx.y * P.h * P.w + (size_t)y * P.w + x) * 73;
            const int qa = (grp == 0 ? 3 : 1) * 9, qb = (grp == 0 ? 2 : 0) * 9;
#pragma unroll
            for (int k = 0; k < 9; k++) { pp[qa + k] = N[k]; pp[36 + qa + k] = D[k]; pp[qb + k] = N[9 + k]; pp[36 + qb + k] = D[9 + k]; }
            if (grp == 1) pp[72] = U;
        }
        bool small = false;
#pragma unroll
        for (int k = 0; k < 9; k++)
            if ((vmask >> k) & 1) small = small || !(D[k] > EPPM_C2F_PRE_DMIN) || !(D[9 + k] > EPPM_C2F_PRE_DMIN);
        if (small) s_pre[0] = 1;
        // 2. group 1 names k*: the candidate with the smallest estimate N / D_A over its own two passes, first index on ties; 15: none
        if (grp == 1) {
            int ks = 15;
            float e_best = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                if (!((vmask >> k) & 1)) continue;
                const float e = c2f_min(N[k] / D[k], N[9 + k] / D[9 + k]);
                if (ks == 15 || e < e_best) { e_best = e; ks = k; }
            }
            *key_at(ptid) = 0xfffffffffffffff0ull | (unsigned)ks;
        }
        __syncthreads();
        path = 1;
        if (!s_pre[0]) {
            // k* in full, both groups: B = the minimum of its four passes' costs (no cost of this tile is NaN, so the nesting of c2f_min is the minimum)
            const int ks = (int)(*reinterpret_cast<const uint32_t*>(key_at(ptid)) & 15u);
            const bool live = known && ks != 15;
            if (live) {
                const int cx = (int)(int16_t)(ccx + ks / 3 - 1);
                const int wbase = ((ccy - 1 + ks % 3 - wy0) * WW + (cx - wx0)) * 16;
                const rgbf c2[1] = {texel_rgb(*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + wbase))};
                float cs[2], ws[2];
                if (grp == 0) c2f_rows2_win<R, 3, 2, WW, 0, S, 1>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, cs, ws);
                else c2f_rows2_win<R, 1, 0, WW, 0, S, 1>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, cs, ws);
                const float c = c2f_min(cs[0] / ws[0], cs[1] / ws[1]);
                atomicMin(key_at(ptid), ((unsigned long long)__float_as_uint(c) << 4) | (unsigned)ks);
            }
            __syncthreads();
            // 3. reject what the bound proves worse than B; count the survivors of this lane's two passes
            unsigned sa = 0, sb = 0, tested = 0;
            if (live) {
                const float B = __uint_as_float((uint32_t)(*key_at(ptid) >> 4));
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    if (!((vmask >> k) & 1) || k == ks) continue;
                    const float ra = B * (D[k] + U), rb = B * (D[9 + k] + U);
                    if (!(N[k] * (1.0f - EPPM_C2F_PRE_EPS) >= ra && ra >= EPPM_C2F_PRE_RHSMIN)) sa |= 1u << k;
                    if (!(N[9 + k] * (1.0f - EPPM_C2F_PRE_EPS) >= rb && rb >= EPPM_C2F_PRE_RHSMIN)) sb |= 1u << k;
                    tested += 2;
                }
            }
            const int na = __popc(sa), nb = __popc(sb);
            int ia = na, ib = nb;                    // inclusive prefix over the wave's lanes: neighbouring lanes keep neighbouring pixels
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int ta = __shfl_up(ia, d), tb = __shfl_up(ib, d);
                if (lane >= d) { ia += ta; ib += tb; }
            }
            // a wave = one quarter of the tile's pixels (ptid >> 6) in one pass group: its two totals, lane 63's prefix, go to the 16 words
            // [quarter][pass] that the keys leave free at the end of their rows of padding
            static_assert(KROWS * PADB >= 256 * 8 + 16 * 4, "the counts follow the keys");
            auto qcnt_at = [&](int i) -> int* { return reinterpret_cast<int*>(pad(256 * 8 + i * 4)); };
            const int wq = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
            if (lane == 63) { *qcnt_at(wq * 4 + (grp == 0 ? 3 : 1)) = ia; *qcnt_at(wq * 4 + (grp == 0 ? 2 : 0)) = ib; }
            if (stat && tested) { atomicAdd(stat + 4, tested); atomicAdd(stat + 5, tested - (unsigned)(na + nb)); }
            __syncthreads();
            int qc[4][4];                            // workgroup-uniform
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int p = 0; p < 4; p++) qc[q][p] = __builtin_amdgcn_readfirstlane(*qcnt_at(q * 4 + p));
            // chunks of the lists of the quarters [qlo, qhi): one list per pass, each rounded up to whole 64-item chunks
            auto chunks_of = [&](int qlo, int qhi) {
                int c = 0;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    int s = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) s += (q >= qlo && q < qhi) ? qc[q][p] : 0;
                    c += (s + 63) >> 6;
                }
                return c;
            };
            // 4. the survivors, one list per pass in segments of whole 64-item chunks, evaluated by all eight waves.  A tile whose survivors do
            // not fit the list is drained in parts through the same list: the pixels' halves if each fits, else their quarters (a quarter holds
            // at most 64 pixels x 8 candidates x 4 passes = 2 048 items).  Keys, items and costs are what one long list would give.
            static_assert(64 * 8 * 4 <= CAP, "a quarter of the tile always fits the list");
            int qw = 4;                              // quarters per part
            if (chunks_of(0, 4) * 64 > CAP) qw = (chunks_of(0, 2) * 64 <= CAP && chunks_of(2, 4) * 64 <= CAP) ? 2 : 1;
            path = 2;
            if (qw == 4 || EPPM_C2F_PRE_PARTS) {
                const int ba = ia - na, bb = ib - nb;            // this lane's items within its wave's
#pragma unroll 1
                for (int qlo = 0; qlo < 4; qlo += qw) {
                    const int qhi = qlo + qw;
                    int cnt[4], chb[5];
                    chb[0] = 0;
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        int s = 0;
#pragma unroll
                        for (int q = 0; q < 4; q++) s += (q >= qlo && q < qhi) ? qc[q][p] : 0;
                        cnt[p] = s; chb[p + 1] = chb[p] + ((s + 63) >> 6);
                    }
                    if (wq >= qlo && wq < qhi) {                 // wave-uniform; the waves of a part in quarter order: pixel order kept
                        int oa = 0, ob = 0;
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            const bool before = (q >= qlo && q < wq);
                            oa += before ? (grp == 0 ? qc[q][3] : qc[q][1]) : 0;
                            ob += before ? (grp == 0 ? qc[q][2] : qc[q][0]) : 0;
                        }
                        int at = (grp == 0 ? chb[3] : chb[1]) * 64 + oa + ba;
                        for (unsigned s = sa; s; s &= s - 1) *item_at(at++) = (uint16_t)(ptid | ((__ffs(s) - 1) << 8));
                        at = (grp == 0 ? chb[2] : chb[0]) * 64 + ob + bb;
                        for (unsigned s = sb; s; s &= s - 1) *item_at(at++) = (uint16_t)(ptid | ((__ffs(s) - 1) << 8));
                    }
                    __syncthreads();
                    for (int c = tid >> 6; c < chb[4]; c += 8) {
                        const int p = __builtin_amdgcn_readfirstlane((c >= chb[1]) + (c >= chb[2]) + (c >= chb[3]));
                        const int idx = (c - chb[p]) * 64 + lane;
                        if (idx < cnt[p]) {
                            const unsigned it = *item_at(chb[p] * 64 + idx);
                            const int ip = it & 255, k = it >> 8, tx = ip & (kBlock - 1), ty = ip / kBlock;
                            const int px = x0 + tx, py = y0 + ty;
                            const int qcx = c2f_centre(flow[(py * P.w + px) * 2], px), qcy = c2f_centre(flow[(py * P.w + px) * 2 + 1], py);
                            const int cx = (int)(int16_t)(qcx + k / 3 - 1);
                            const int wbase = ((qcy - 1 + k % 3 - wy0) * WW + (cx - wx0)) * 16;
                            const rgbf q1 = texel_rgb(s_src[(ty + R) * TW + tx + R]);
                            const rgbf q2 = texel_rgb(*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + wbase));
                            float c_;
                            if (p == 3) c_ = c2f_one_win<R, 3, WW>(L, s_src, TW, tx, ty, q1, q2, s_win, wbase);
                            else if (p == 2) c_ = c2f_one_win<R, 2, WW>(L, s_src, TW, tx, ty, q1, q2, s_win, wbase);
                            else if (p == 1) c_ = c2f_one_win<R, 1, WW>(L, s_src, TW, tx, ty, q1, q2, s_win, wbase);
                            else c_ = c2f_one_win<R, 0, WW>(L, s_src, TW, tx, ty, q1, q2, s_win, wbase);
                            atomicMin(key_at(ip), ((unsigned long long)__float_as_uint(c_) << 4) | (unsigned)k);
                        }
                    }
                    __syncthreads();                             // the list is free for the next part; after the last one the keys are final
                }
                // 5. the smallest cost, then the smallest candidate index: the reference's strict < in candidate order
                if (stat && tid == 0) {              // path 2 now: the list was drained in parts ([6] in halves, [7] in quarters)
                    atomicAdd(stat + (qw == 4 ? 0 : 2), 1u);
                    if (qw != 4) atomicAdd(stat + (qw == 2 ? 6 : 7), 1u);
                }
                if (grp != 1 || !inimg) return;
                if (!known) { c2f_store_flow(flow, y * P.w + x, 0, 0); return; }
                int k = (int)(*key_at(ptid) & 15u);
                if (k == 15) k = 4;                  // no candidate in the image: the centre stays (kernel.cu:2026)
                c2f_store_flow(flow, y * P.w + x, (int)(int16_t)(ccx + k / 3 - 1) - x, (int)(int16_t)(ccy + k % 3 - 1) - y);
                return;
            }
        }
    }
    if (stat && tid == 0) atomicAdd(stat + path, 1u);
#endif
    float res[9];                                   // group 0: __min(c3,c4) per candidate; group 1: c2 then the final cost
    float res1[9];                                  // group 1: c1 (raw)
    if (known) {
        const rgbf c1 = texel_rgb(s_src[(threadIdx.y + R) * TW + threadIdx.x + R]);
#pragma unroll
        for (int m = 0; m < 3; m++) {               // x offset outer, as the reference's candidate loop (kernel.cu:2028)
            const int cx = (int)(int16_t)(ccx + m - 1);
            float run[3] = {0.0f, 0.0f, 0.0f}, raw[3] = {0.0f, 0.0f, 0.0f};
            if (!(cx < 0 || cx >= P.w)) {            // else: every candidate of this column is skipped (:2030)
                rgbf c2[3];
                const int cx16 = cx << 4, wmax16 = (P.w - 1) << 4;
                if (coherent) {
                    const int wbase = ((ccy - 1 - wy0) * WW + (cx - wx0)) * 16;
#pragma unroll
                    for (int n = 0; n < 3; n++) c2[n] = texel_rgb(*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + wbase + n * (WW * 16)));
#if EPPM_C2F_PASS2
                    if (grp == 0) {
                        float c4[3], c3[3];
                        c2f_pass2_win<R, 3, 2, WW>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, c4, c3);
#pragma unroll
                        for (int n = 0; n < 3; n++) run[n] = c2f_min(c3[n], c4[n]);
                    } else {
                        c2f_pass2_win<R, 1, 0, WW>(L, s_src, TW, threadIdx.x, threadIdx.y, c1, c2, s_win, wbase, run, raw);
                    }
#else
                    if (grp == 0) {
                        c2f_pass<R, 3, false, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                        c2f_pass<R, 2, false, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                    } else {
                        c2f_pass<R, 1, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                        c2f_pass<R, 0, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, raw, s_win, wbase);
                    }
#endif
                } else {
#pragma unroll
                    for (int n = 0; n < 3; n++) c2[n] = texel_rgb(tex_px(P.pk2, P.pitch, P.w, P.h, cx, ccy + n - 1));
                    if (grp == 0) {
                        c2f_pass<R, 3>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                        c2f_pass<R, 2>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                    } else {
                        c2f_pass<R, 1, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                        c2f_pass<R, 0, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, raw);
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < 3; n++) { res[m * 3 + n] = run[n]; res1[m * 3 + n] = raw[n]; }
        }
    }
    __syncthreads();                                // every read of the source tile is done: its storage carries the exchange
    float* __restrict__ xch = reinterpret_cast<float*>(s_src);
    if (grp == 0 && known) {
#pragma unroll
        for (int k = 0; k < 9; k++) xch[k * 256 + ptid] = res[k];
    }
    __syncthreads();
    if (grp != 1 || !inimg) return;
    if (!known) { c2f_store_flow(flow, y * P.w + x, 0, 0); return; }
    int bx = ccx, by = ccy;
    float min_cost = 999999;
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const int cx = (int)(int16_t)(ccx + m - 1);
        if (cx < 0 || cx >= P.w) continue;
#pragma unroll
        for (int n = 0; n < 3; n++) {
            const int cy = (int)(int16_t)(ccy + n - 1);
            if (cy < 0 || cy >= P.h) continue;
            const float m34 = xch[(m * 3 + n) * 256 + ptid];
            const float c_2 = res[m * 3 + n], c_1 = res1[m * 3 + n];
            const float cv = c2f_min(c_1, c2f_min(c_2, m34));           // m34: group 0's __min(cost3, cost4)
            if (cv < min_cost) { min_cost = cv; bx = cx; by = cy; }
        }
    }
    flow[(y * P.w + x) * 2] = (float)(bx - x);
    flow[(y * P.w + x) * 2 + 1] = (float)(by - y);
}

// The same for large radii (PATCH_R 17: source tile 50x64 texels = 51 KB, target window 80x72 texels = 92 KB: one workgroup per
// CU): 1024 threads = 256 pixels x 4 pass groups, one affine pass each, so that the one resident workgroup still gives 4 waves
// per SIMD.  Groups 1..3 hand their raw pass costs to group 0 through the source tile's storage.
template <int R>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_c2f_refine_win4(PlanesH Ph, float* __restrict__ flow_, const float* __restrict__ lut, size_t pstride)
{
    using W = C2fWinShape<R>;
    constexpr int TWU = C2fSrcTile<R>::TWU, TW = C2fSrcTile<R>::TW, WW = W::WW, WH = W::WH;
    static_assert(TWU * TW * 16 >= 27 * 256 * 4, "the exchange buffer aliases the source tile");
    static_assert(sizeof(PatchLutT<R + 1>) + (TWU * TW + WH * WW) * 16 + 16 <= 160 * 1024, "LDS budget of one CU");
    __shared__ EPPM_LUT_ALIGN PatchLutT<R + 1> L;
    __shared__ float4 s_src[TWU * TW];
    __shared__ float4 s_win[WH * WW];
    __shared__ int s_mm[4];
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.y);
    const int ptid = threadIdx.y * kBlock + threadIdx.x;
    const int grp = threadIdx.z;                                     // pass group: evaluates pass 3 - grp (0-based: 3 = the 4th pass)
    const int tid = grp * 256 + ptid;
    load_patch_lut<EPPM_C2F_LOG2>(L, lut, R, tid, 1024);
    const Planes P = to_dev(Ph, pstride, blockIdx.y);
    const uint32_t* __restrict__ pc1 = pair_ptr_opt(Ph.pc1, pstride, blockIdx.y);
    const uint32_t* __restrict__ pc2 = pair_ptr_opt(Ph.pc2, pstride, blockIdx.y);
    int x0, y0, part;
    if (!c2f_tile_origin<0>(P, x0, y0, part)) return;
    if (tid == 0) { s_mm[0] = 0x7fffffff; s_mm[1] = -0x7fffffff; s_mm[2] = 0x7fffffff; s_mm[3] = -0x7fffffff; }
    for (int t = tid; t < TWU * TWU; t += 1024) {
        const int ry = t / TWU, rx = t % TWU;
        const int sy = iclamp(y0 + ry - R, 0, P.h - 1), sx = iclamp(x0 + rx - R, 0, P.w - 1);
        s_src[ry * TW + rx] = stage_texel(pc1, P.pk1, (unsigned)(sy * P.pitch + sx));
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inimg = (x < P.w && y < P.h);
    float fvx = 0.0f, fvy = 0.0f;
    if (inimg) { fvx = flow[(y * P.w + x) * 2]; fvy = flow[(y * P.w + x) * 2 + 1]; }
    const bool known = inimg && !(fvx > kUnknownFlowThresh || fvy > kUnknownFlowThresh);
    const int ccx = c2f_centre(fvx, x), ccy = c2f_centre(fvy, y);
    if (known && grp == 0) {
        atomicMin(&s_mm[0], ccx); atomicMax(&s_mm[1], ccx);
        atomicMin(&s_mm[2], ccy); atomicMax(&s_mm[3], ccy);
    }
    __syncthreads();
    const int mnx = s_mm[0], mxx = s_mm[1], mny = s_mm[2], mxy = s_mm[3];
    const bool coherent = (mxx - mnx <= W::SPAN_X) && (mxy - mny <= W::SPAN_Y);
    const int wx0 = mnx - 1 + W::XLO, wy0 = mny - 1 + W::YLO;
    if (coherent && mxx >= mnx) {
        for (int t = tid; t < WH * WW; t += 1024) {
            const int sy = iclamp(wy0 + t / WW, 0, P.h - 1), sx = iclamp(wx0 + t % WW, 0, P.w - 1);
            s_win[t] = stage_texel(pc2, P.pk2, (unsigned)(sy * P.pitch + sx));
        }
    }
    __syncthreads();
    float res[9];                                   // raw cost of this group's pass for the 9 candidates
    if (known) {
        const rgbf c1 = texel_rgb(s_src[(threadIdx.y + R) * TW + threadIdx.x + R]);
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const int cx = (int)(int16_t)(ccx + m - 1);
            float run[3] = {0.0f, 0.0f, 0.0f};
            if (!(cx < 0 || cx >= P.w)) {
                rgbf c2[3];
                const int cx16 = cx << 4, wmax16 = (P.w - 1) << 4;
                if (coherent) {
                    const int wbase = ((ccy - 1 - wy0) * WW + (cx - wx0)) * 16;
#pragma unroll
                    for (int n = 0; n < 3; n++) c2[n] = texel_rgb(*reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_win) + wbase + n * (WW * 16)));
                    if (grp == 0) c2f_pass<R, 3, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                    else if (grp == 1) c2f_pass<R, 2, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                    else if (grp == 2) c2f_pass<R, 1, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                    else c2f_pass<R, 0, true, true, WW>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run, s_win, wbase);
                } else {
#pragma unroll
                    for (int n = 0; n < 3; n++) c2[n] = texel_rgb(tex_px(P.pk2, P.pitch, P.w, P.h, cx, ccy + n - 1));
                    if (grp == 0) c2f_pass<R, 3, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                    else if (grp == 1) c2f_pass<R, 2, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                    else if (grp == 2) c2f_pass<R, 1, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                    else c2f_pass<R, 0, true>(P, L, s_src, TW, threadIdx.x, threadIdx.y, cx16, wmax16, ccy, c1, c2, run);
                }
            }
#pragma unroll
            for (int n = 0; n < 3; n++) res[m * 3 + n] = run[n];
        }
    }
    __syncthreads();                                // every read of the source tile is done: its storage carries the exchange
    float* __restrict__ xch = reinterpret_cast<float*>(s_src);
    if (grp != 0 && known) {
#pragma unroll
        for (int k = 0; k < 9; k++) xch[((grp - 1) * 9 + k) * 256 + ptid] = res[k];
    }
    __syncthreads();
    if (grp != 0 || !inimg) return;
    if (!known) { c2f_store_flow(flow, y * P.w + x, 0, 0); return; }
    int bx = ccx, by = ccy;
    float min_cost = 999999;
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const int cx = (int)(int16_t)(ccx + m - 1);
        if (cx < 0 || cx >= P.w) continue;
#pragma unroll
        for (int n = 0; n < 3; n++) {
            const int cy = (int)(int16_t)(ccy + n - 1);
            if (cy < 0 || cy >= P.h) continue;
            const int k = m * 3 + n;
            const float c_4 = res[k], c_3 = xch[k * 256 + ptid], c_2 = xch[(9 + k) * 256 + ptid], c_1 = xch[(18 + k) * 256 + ptid];
            const float cv = c2f_min4(c_1, c_2, c_3, c_4);
            if (cv < min_cost) { min_cost = cv; bx = cx; by = cy; }
        }
    }
    flow[(y * P.w + x) * 2] = (float)(bx - x);
    flow[(y * P.w + x) * 2 + 1] = (float)(by - y);
}

// the candidate loop over the costs written by the split launch: SPLIT 3 the nested minimum, SPLIT 4 the four passes' raw costs
template <int SPLIT>
__global__ __launch_bounds__(256) void k_c2f_select(float* __restrict__ flow_, const float* __restrict__ cost9_, int w, int h, size_t pstride)
{
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.z);
    const float* __restrict__ cost9 = pair_ptr(cost9_, pstride, blockIdx.z);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const float fvx = flow[(y * w + x) * 2], fvy = flow[(y * w + x) * 2 + 1];
    if (c2f_unknown(fvx, fvy)) { c2f_store_flow(flow, y * w + x, 0, 0); return; }
    c2f_select_best(flow, x, y, c2f_centre(fvx, x), c2f_centre(fvy, y), w, h, [=](int m, int n) {
        const float* __restrict__ pc = cost9 + (size_t)(y * w + x) * 36 + m * 3 + n;
        float cv = pc[0];
        if (SPLIT == 4) {                    // c2f_min4, the passes read 4th to 1st
            cv = pc[27];
            cv = c2f_min(pc[18], cv);
            cv = c2f_min(pc[9], cv);
            cv = c2f_min(pc[0], cv);
        }
        return cv;
    });
}

// admissible spread (max - min) of a tile's candidate centres in the LDS-window kernels, for the tests that probe the boundary
bool c2f_window_span(int R, int* span_x, int* span_y)
{
    if (!(R == 9 || R == 17)) return false;
    *span_x = (R == 9) ? C2fWinShape<9>::SPAN_X : C2fWinShape<17>::SPAN_X;
    *span_y = (R == 9) ? C2fWinShape<9>::SPAN_Y : C2fWinShape<17>::SPAN_Y;
    return true;
}

// the knobs the two-phase window refine was built with
void c2f_pretest_knobs(int R, int* on, int* row0, int* rows, int* cap, int* parts, float* eps, float* dmin, float* rhsmin)
{
#ifdef EPPM_TOL
    *on = 0;                                     // the tolerance library's kernel has no two-phase form: `pre` is ignored there
#else
    *on = EPPM_C2F_PRE;
#endif
    *row0 = (R + 1 - EPPM_C2F_PRE_ROWS) / 2; *rows = EPPM_C2F_PRE_ROWS;
    *cap = C2fPreList<9>::CAP;                   // items of a tile's survivor list
    *parts = EPPM_C2F_PRE_PARTS;                 // 1: a tile with more survivors is drained in parts, 0: it takes the one-phase loop
    *eps = EPPM_C2F_PRE_EPS; *dmin = EPPM_C2F_PRE_DMIN; *rhsmin = EPPM_C2F_PRE_RHSMIN;
}

static bool c2f_table_ok(int w, int h, int R) { return (w + R < 32764) && (h + R < 32764); }      // range of the offset-table identity (c2f_device.cuh)

// no_split (a context's "c2f_no_split" option): never split, so that small images go through the LDS-window kernels too
int c2f_refine_split_factor(int w, int h, int R, int npairs, bool no_split)
{
    if (no_split || !(R == 9 || R == 17) || !c2f_table_ok(w, h, R)) return 0;
    const int tiles = ((w + kBlock - 1) / kBlock) * ((h + kBlock - 1) / kBlock);
    // Round 2 split below 3 waves per SIMD, which sent level 1 of ONE 1024x436 pair (448 tiles) through the split gather kernel:
    // 0.367 ms and a 16 MB scratch plane of 36 costs per pixel; the LDS-window kernel does the same launch in 0.364 ms without it.
    if (!(tiles * npairs * 4 < EPPM_C2F_SPLIT_BELOW_WAVES)) return 0;
    // 3 or 4 workgroups per tile: the factor whose workgroup count divides more evenly over the 256 CUs
    auto imbalance = [&](int f) { const int wgs = tiles * f * npairs; return (float)((wgs + 255) / 256) * 256.0f / (float)wgs; };
    return (imbalance(4) < imbalance(3)) ? 4 : 3;
}
bool c2f_refine_wants_split(int w, int h, int R, int npairs, bool no_split) { return c2f_refine_split_factor(w, h, R, npairs, no_split) != 0; }

// the tile kernels exist for radius 9 and 17: f(the radius as a compile-time constant)
template <class F>
static void with_radius(int R, F&& f)
{
    if (R == 9) f(std::integral_constant<int, 9>{});
    else f(std::integral_constant<int, 17>{});
}

// cost9: scratch of 36 floats per pixel, or NULL (never split)
// pre: the two-phase form of k_c2f_refine_win<9>'s coherent tiles (-1 the library's EPPM_C2F_PRE, 0 off, 1 on); stat: NULL, or eight
// zeroed counters of that kernel (tiles two-phase with one list / weight sum too small / list drained in parts / one-phase, pairs tested, pairs
// rejected, tiles drained in halves, in quarters)
void launch_c2f_refine(const PlanesH& P, float* flow, const float* lut, int R, float* cost9, hipStream_t s, Batch bt, bool no_split, int pre,
                       unsigned* stat, float* probe)
{
    dim3 grid((P.w + kBlock - 1) / kBlock, (P.h + kBlock - 1) / kBlock, bt.n), block(kBlock, kBlock);
    const int per_xcd = (grid.x * grid.y + 7) / 8;
    dim3 grid1(per_xcd * 8, bt.n);               // x: padded so every XCD gets the same number of slots; y: pair
    const int f = cost9 ? c2f_refine_split_factor(P.w, P.h, R, bt.n, no_split) : 0;
    launch_note(kLaunchRefine, P.w, P.h, bt.n, f, R);
    if (f) {
        dim3 gridf(per_xcd * f * 8, bt.n), gs((P.w + 63) / 64, (P.h + 3) / 4, bt.n), bs(64, 4);
        with_radius(R, [&](auto r) {
            if (f == 3) hipLaunchKernelGGL((k_c2f_refine_tiled<r(), 3>), gridf, block, 0, s, P, flow, lut, cost9, bt.stride);
            else hipLaunchKernelGGL((k_c2f_refine_tiled<r(), 4>), gridf, block, 0, s, P, flow, lut, cost9, bt.stride);
        });
        if (f == 3) hipLaunchKernelGGL(k_c2f_select<3>, gs, bs, 0, s, flow, cost9, P.w, P.h, bt.stride);
        else hipLaunchKernelGGL(k_c2f_select<4>, gs, bs, 0, s, flow, cost9, P.w, P.h, bt.stride);
        return;
    }
    if (!(R == 9 || R == 17) || !c2f_table_ok(P.w, P.h, R)) {
        hipLaunchKernelGGL(k_c2f_refine, grid, block, 0, s, P, flow, lut, R, bt.stride);
        return;
    }
    const bool window = (R == 9) ? EPPM_C2F_WINDOW : EPPM_C2F_WINDOW17;
    if (!window) with_radius(R, [&](auto r) { hipLaunchKernelGGL((k_c2f_refine_tiled<r(), 0>), grid1, block, 0, s, P, flow, lut, (float*)nullptr, bt.stride); });
    else if (R == 9 && probe) hipLaunchKernelGGL((k_c2f_refine_win<9, true>), grid1, dim3(kBlock, kBlock, 2), 0, s, P, flow, lut, bt.stride, 1, stat, probe);
    else if (R == 9) hipLaunchKernelGGL((k_c2f_refine_win<9>), grid1, dim3(kBlock, kBlock, 2), 0, s, P, flow, lut, bt.stride, pre < 0 ? EPPM_C2F_PRE : pre, stat, (float*)nullptr);
    else hipLaunchKernelGGL((k_c2f_refine_win4<17>), grid1, dim3(kBlock, kBlock, 4), 0, s, P, flow, lut, bt.stride);
}

}  // namespace eppm
