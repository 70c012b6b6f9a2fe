// pm_device.cuh -- PatchMatch at the coarsest level (reference: bao_pmflow_kernel.cu), what its stage files share: k_pm_field.hip (:50-109
// random field, :636-645 cost field, the seeded start's select), k_pm_sweep.hip (:1049-1181 segmented propagation), k_pm_search.hip (:1519-1594).
//
// Determinism: every kernel realises the "lockstep" order of the racy original --
// all threads read before any thread writes, segment seeds are read at step 0, and the doubly visited
// forward pixel L is visited by segment 1 before segment 0.
//
// MI355X mapping: the quarter-resolution level has only ~28 k pixels (436 waves of one pixel per lane on
// 1024 SIMDs) and the sweeps only ~2.8 k serial chains per direction, so the kernels spread ONE patch
// evaluation over 16 lanes (sweeps) or the six guesses of a pixel over separate lanes (search), and the
// forward and backward problems of a pair share every launch.
#pragma once
#include "eppm_device.cuh"

// ---------------------------------------------------------------------------------------------------
// Every tuning knob of the PatchMatch kernels and launchers: set with -D (tools/build_variant.sh), cited by name in profiles/ (the host loop's: pm_driver.cpp)
// ---------------------------------------------------------------------------------------------------
// ---- field, and the parity planes of every stage ----
// every problem of the launch has its target's column-parity plane (PlanesH::pp2).  Exact library: per kernel, radius 9 only, where
// the A/B measurement adopted it (EPPM_PARITY_*); the tolerance library: every kernel, both radii.
#ifndef EPPM_PARITY_SEARCH
#define EPPM_PARITY_SEARCH 1
#endif
#ifndef EPPM_PARITY_SPEC
#define EPPM_PARITY_SPEC 0
#endif
#ifndef EPPM_PARITY_COST
#define EPPM_PARITY_COST 1
#endif
#ifndef EPPM_COST_FIELD_TILE
#define EPPM_COST_FIELD_TILE 1      // 0: the cost field and the seeded start's select gather at every radius (pm_cost_kernel)
#endif
// ---- sweeps ----
#ifndef EPPM_LPC9
#ifdef EPPM_TOL
#define EPPM_LPC9 32      // tolerance library: a lane = a chunk of 5 samples (coop_chunk): 20 of 32 lanes work, whatever the launch size
#else
#define EPPM_LPC9 16      // lanes per sweep chain at patch radius 9 (100 samples); doubled for launches that cannot fill the chip, see launch_pm_sweep
#endif
#endif
#ifndef EPPM_LPC17
#define EPPM_LPC17 64     // ... at patch radius 17 (324 samples)
#endif
#ifndef EPPM_LPC9_SPEC
#ifdef EPPM_TOL
#define EPPM_LPC9_SPEC 32     // tolerance library: see EPPM_LPC9
#else
#define EPPM_LPC9_SPEC 16     // lanes per chain in phase B at radius 9 (4 were tried -- a quarter of the waves, one round of workgroups --
#endif
#endif                        // and lost: 50-56 vs 32-41 us per 8-pair launch, the evaluations after accepted candidates take four times as long)
#ifndef EPPM_LPC17_SPEC
#define EPPM_LPC17_SPEC 64    // ... at radius 17
#endif
// 16 lanes per chain are the most instruction-efficient; when that leaves fewer than two waves per SIMD (the
// quarter-resolution level of a 1024x436 pair: 1.4) the chip is latency bound and 32 lanes per chain shorten
// the dependent step (PatchMatch 1.78 -> 1.61 ms, no change in throughput with pairs in flight)
#ifndef EPPM_LPC_SWITCH_WAVES
#define EPPM_LPC_SWITCH_WAVES (2 * 1024)
#endif
#ifndef EPPM_SWEEP_PRE
#define EPPM_SWEEP_PRE 1      // the classic form fetches its chains' pixels up front: 0 never, 1 launches that cannot fill the chip, 2 always
#endif
#ifndef EPPM_SWEEP_GB
#define EPPM_SWEEP_GB 7   // sample gathers a sweep lane keeps in flight (per image)
#endif
#ifndef EPPM_SWEEP_GB_SPEC
#define EPPM_SWEEP_GB_SPEC 3  // ... in phase B, which evaluates rarely and gains more from waves (one round of workgroups) than from depth
#endif
#ifndef EPPM_SWEEP_TILE
#define EPPM_SWEEP_TILE 1     // source tile in LDS while it stays small (16 KiB at R = 9 and the default segment length of 10); very long segments gather
#endif
#ifdef EPPM_SWEEP_WAVES       // (no default: the compiler's choice) waves per SIMD of k_pm_sweep
#define EPPM_SWEEP_OCC __attribute__((amdgpu_waves_per_eu(EPPM_SWEEP_WAVES, EPPM_SWEEP_WAVES)))
#else
#define EPPM_SWEEP_OCC
#endif
// Phase A, radius 17: one lane's evaluation is a serial chain of 324 samples (75 us), the 45 KB tile allows three workgroups per CU, and in
// the converged iterations a block has a handful of evaluations left: then a whole wave takes one evaluation (6 samples per lane,
// ordered 54-hop sum), four at a time.  (At radius 9 the same with 16 lanes per evaluation was measured and lost -- its registers cost the
// early iterations, every block of the launch, more than the late ones gain -- and as a separate instantiation for the late
// iterations only it changed nothing: profiles/r04x_c.)
#ifndef EPPM_SPEC_COOP17_MAX
#define EPPM_SPEC_COOP17_MAX 32
#endif
// Merged phase A, radius 9, a block with at most 16 evaluations (the usual case in the iterations k_pm_spec_all runs in): 16 lanes each, all
// at once -- the launch then waits for a 7-sample chain and 16 hops instead of one lane's 100 samples.  (In k_pm_sweep_spec the same lost: its
// registers cost the early iterations, which every block of that kernel also serves; k_pm_spec_all only runs late.)  PatchMatch
// 0.747 -> 0.741 ms per pair in 8-pair launches, default bench +0.4 % (two interleaved rounds each), 1920x1080 unchanged.
#ifndef EPPM_MERGED_COOP9_MAX
#define EPPM_MERGED_COOP9_MAX 16
#endif
// ---- search ----
#ifdef EPPM_SEARCH_WAVES      // (no default) waves per SIMD of k_pm_random_search
#define EPPM_SEARCH_OCC __attribute__((amdgpu_waves_per_eu(EPPM_SEARCH_WAVES, EPPM_SEARCH_WAVES)))
#else
#define EPPM_SEARCH_OCC
#endif
// EPPM_SEARCH_TERM_UNROLL (no default: a divisor of S chosen per radius): terms of a patch row interleaved, see search_patch_dist
#ifndef EPPM_SEARCH_SKIP_SAME
#define EPPM_SEARCH_SKIP_SAME 1               // a guess equal to the pixel's current match sits its evaluation out (k_pm_random_search)
#endif
#ifndef EPPM_SEARCH_HALF_BELOW_WGS
#define EPPM_SEARCH_HALF_BELOW_WGS 1024       // under four quarter-workgroups per CU: eighth-block workgroups (PatchMatch of one 1024x436 pair 1.362 -> 1.330 ms;
#endif                                        // at 4080 workgroups, one 1920x1080 pair, they lose: 4.49 -> 4.57 ms)
#ifndef EPPM_SEARCH_PK17
#define EPPM_SEARCH_PK17 1                    // the streaming search at radius 17 gathers the 4-byte target plane (PK = 1)
#endif
// The two-phase search (k_pm_random_search<.., PRE = true>): a guess whose cost can be PROVED not to beat the
// pixel's stored cost from a few centre rows of its patch is never evaluated in full.
#ifndef EPPM_SEARCH_PRE_ROWS
#define EPPM_SEARCH_PRE_ROWS 4                // centre rows of the patch the pre-test evaluates (radius 9: rows 3-6 of 0-9, 40 of 100 samples)
#endif
#ifndef EPPM_SEARCH_PRE_FROM
#define EPPM_SEARCH_PRE_FROM 2                // first PatchMatch iteration whose search runs in the two-phase form; negative: never
#endif
#ifndef EPPM_SEARCH_PRE_COOP_MAX
#define EPPM_SEARCH_PRE_COOP_MAX 96           // up to so many survivors in a workgroup, phase 2 gives each 16 lanes (all waves work) instead of one lane
#endif
#ifndef EPPM_SEARCH_PRE_EPS
#define EPPM_SEARCH_PRE_EPS 0x1p-13f          // shrinks the lower bound: >= 4 x the float error of its two sides (tests/test_search_pretest_cpu.py)
#endif

namespace eppm {

__device__ __forceinline__ Planes to_dev(const PlanesH& h)
{
    Planes p;
    p.pk1 = (const float4*)h.pk1; p.pk2 = (const float4*)h.pk2;
    p.w = h.w; p.h = h.h; p.pitch = h.pitch;
    return p;
}

// problem q of a launch: direction q % n of pair q / n; pair k's planes lie k * stride bytes after pair 0's
__device__ __forceinline__ PmProblem pm_problem(const PmBatch& B, unsigned q)
{
    PmProblem p = B.p[q % (unsigned)B.n];
    const unsigned pair = q / (unsigned)B.n;
    p.P.pk1 = pair_ptr_opt(p.P.pk1, B.stride, pair);
    p.P.pk2 = pair_ptr_opt(p.P.pk2, B.stride, pair);
    p.P.pc1 = pair_ptr_opt(p.P.pc1, B.stride, pair);
    p.P.pc2 = pair_ptr_opt(p.P.pc2, B.stride, pair);
    p.P.pp1 = pair_ptr_opt(p.P.pp1, B.stride, pair);
    p.P.pp2 = pair_ptr_opt(p.P.pp2, B.stride, pair);
    p.cost = pair_ptr_opt(p.cost, B.stride, pair);
    p.nnf = pair_ptr_opt(p.nnf, B.stride, pair);
    p.nnf_alt = pair_ptr_opt(p.nnf_alt, B.stride, pair);
    p.spec = pair_ptr_opt(p.spec, B.stride, pair);
    p.scand = pair_ptr_opt(p.scand, B.stride, pair);
    p.wl = pair_ptr_opt(p.wl, B.stride, pair);
    p.seed = pair_ptr_opt(p.seed, B.stride, pair);
    p.rng_work = pair_ptr_opt(p.rng_work, B.stride, pair);
    p.rng_work_next = pair_ptr_opt(p.rng_work_next, B.stride, pair);
    p.restw = pair_ptr_opt(p.restw, B.stride, pair);
    return p;
}

__device__ __forceinline__ Xorwow load_state(const uint32_t* p)
{
    Xorwow s;
    s.v0 = p[0]; s.v1 = p[1]; s.v2 = p[2]; s.v3 = p[3]; s.v4 = p[4]; s.d = p[5];
    return s;
}
__device__ __forceinline__ void store_state(uint32_t* p, const Xorwow& s)
{
    p[0] = s.v0; p[1] = s.v1; p[2] = s.v2; p[3] = s.v3; p[4] = s.v4; p[5] = s.d;
}

// RT = 9 / 17: the source samples of the workgroup's 16x4 pixels come from an LDS tile (16+2R)x(4+2R), loaded once,
// clamped at load -- one LDS read per sample instead of a clamped address and a gather; RT = 0: any radius, source
// samples gathered from the plane.
template <int RT> struct SearchLut { using type = PatchLutT<RT + 1>; };
template <> struct SearchLut<0> { using type = PatchLut; };          // any radius the ABI accepts

__device__ __forceinline__ float patch_dist_any(const Planes& P, const PatchLut& L, int R, int x1, int y1, int x2, int y2) { return patch_dist(P, L, R, x1, y1, x2, y2); }
template <int M> __device__ __forceinline__ float patch_dist_any(const Planes&, const PatchLutT<M>&, int, int, int, int, int) { return 0.0f; }   // never called (RT != 0)

// PK = 1: the target texels are gathered from the 4-byte plane pc2 = {R, G, B, census} and converted at use (make_texel, the function
// that built the float4 plane: the same bits).  A 64-lane gather of 4 bytes costs the L1 38 clocks where one of 16 bytes costs 52-78
// (tools/ubench/gather_rate.hip), the conversion 12 VALU instructions per texel: for launches whose search runs at the L1's lane
// rate with VALU slots to spare -- radius 17, or one small pair per launch.
// PK = 2: the S samples of a patch row are S consecutive words of the target's column-parity plane (PlanesH::pp2): 3 gathers per row of
// 10 samples (16 + 16 + 8 bytes) instead of 10, unpacked by unpack_texel.  These kernels run at the L1's lane rate; this divides their
// gathers by 3.3.  The exact library pays 10 VALU instructions per texel for its exact unpack and still wins at radius 9 in the search
// (TA busy 0.86 -> 0.36, 314 -> 280 us per 8-pair launch) and the cost field, not in phase A.
// (The source half of a sample's weight is the same for the six guesses of a pixel; forming it once per workgroup in LDS -- 26 KB,
// [sample][pixel] -- and a barrier LOSES here as it did in the exact library: search 215 -> 234 us per 8-pair launch, bench 304 -> 298,
// profiles/r06x_c_search_hoist.txt.)
#define EPPM_PM_PRAGMA_(x) _Pragma(#x)
#define EPPM_PM_UNROLL(n) EPPM_PM_PRAGMA_(unroll n)
template <int RT, int PK = 0, class LUT>
__device__ __forceinline__ float search_patch_dist(const Planes& P, const LUT& L, int R, const float4* __restrict__ s_src, int TW,
                                                   int tx, int ty, int x1, int y1, int x2, int y2, const PlanesH& PH)
{
    if (RT == 0) return patch_dist_any(P, L, R, x1, y1, x2, y2);
    constexpr int S = RT + 1;
    const int pitch16 = P.pitch << 4;
    const rgbf c1 = texel_rgb(s_src[(ty + RT) * TW + tx + RT]);
    const rgbf c2 = texel_rgb(texel_at(P.pk2, texel_off(pitch16, P.w, P.h, x2, y2)));
    PatchSum sum;
    constexpr int CS = tol_chunk(RT);          // tolerance library: chunk of the canonical summation order (PatchSum)
    static_assert(S % CS == 0, "whole chunks per row");
    if constexpr (PK == 2) {
        static_assert(S % 4 == 2, "a row = whole dwordx4 gathers + one dwordx2");
        // buffer loads: a dwordx4 at a 4-byte aligned per-lane offset in ONE instruction (a global load of that alignment is split by the
        // compiler), 32-bit offsets; the descriptor is built from workgroup-uniform values (the problem's plane, its size)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(PH.pp2), 0, 2 * P.h * PH.pp_pitch * 4, 0x00020000);
        const int xp = x2 - RT + PH.pp_pad;                       // padded column of the row's first sample, >= 1
        const int rb = ((xp & 1) * P.h) * PH.pp_pitch + (xp >> 1);
        uint32_t two = 2u;
        asm volatile("" : "+v"(two));
#pragma unroll 2
        for (int ii = 0; ii < S; ii++) {
            const int ro = (rb + iclamp(y2 + 2 * ii - RT, 0, P.h - 1) * PH.pp_pitch) * 4;      // byte offset of the row's first sample
            const float4* __restrict__ srow = s_src + (ty + 2 * ii) * TW + tx;
            uint32_t wq[S];
#pragma unroll
            for (int g = 0; g < S / 4; g++) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, ro + 16 * g, 0, 0);
                wq[4 * g] = v.x; wq[4 * g + 1] = v.y; wq[4 * g + 2] = v.z; wq[4 * g + 3] = v.w;
            }
            { const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, ro + 4 * (S - 2), 0, 0); wq[S - 2] = v.x; wq[S - 1] = v.y; }
            // terms of a row the compiler may interleave: a divisor of S that keeps the kernel at 65 VGPRs = 7 waves per SIMD (radius 9: 5 of
            // 10 -- all 10: 77 VGPRs = 6 waves, search 226 -> 213 us; radius 17: 9 of 18 -- all 18: 98 VGPRs)
#ifdef EPPM_SEARCH_TERM_UNROLL
            constexpr int TU = EPPM_SEARCH_TERM_UNROLL;
#else
            constexpr int TU = (S % 5 == 0) ? 5 : (S % 9 == 0) ? 9 : S;
#endif
EPPM_PM_UNROLL((TU))
            for (int jj = 0; jj < S; jj++) {
                float ct, wt;
                patch_terms(srow[2 * jj], unpack_texel(wq[jj], two), c1, c2, L.gsp[ii * S + jj], L.tab(), ct, wt);
                sum.add(ct, wt);
                if ((jj + 1) % CS == 0) sum.flush();
            }
        }
        return sum.result();
    }
    const uint32_t* __restrict__ pc2 = PH.pc2;
    for (int ii = 0; ii < S; ii++) {
        const int i = 2 * ii - RT;
        const unsigned r2 = __umul24((unsigned)iclamp(y2 + i, 0, P.h - 1), (unsigned)pitch16);
        const float4* __restrict__ srow = s_src + (ty + 2 * ii) * TW + tx;
        for (int j0 = 0; j0 < S; j0 += 5) {
            float4 q1[5], q2[5];
            uint32_t w2[PK == 1 ? 5 : 1];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const int jj = min(j0 + k, S - 1);
                q1[k] = srow[2 * jj];
                const unsigned o2 = r2 + ((unsigned)iclamp(x2 + 2 * jj - RT, 0, P.w - 1) << 4);
                if (PK == 1) w2[k] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(pc2) + (o2 >> 2));
                else q2[k] = texel_at(P.pk2, o2);
            }
#pragma unroll
            for (int k = 0; k < 5; k++) {
                if (j0 + k < S) {
                    float ct, wt;
                    if (PK == 1) q2[k] = make_texel(w2[k], w2[k] >> 24);
                    patch_terms(q1[k], q2[k], c1, c2, L.gsp[ii * S + j0 + k], L.tab(), ct, wt);
                    sum.add(ct, wt);
                    if ((j0 + k + 1) % CS == 0) sum.flush();
                }
            }
        }
    }
    return sum.result();
}

constexpr int pre_row0(int S) { return (S - EPPM_SEARCH_PRE_ROWS) / 2; }        // first of the centre rows of the two-phase search's pre-test
#ifndef EPPM_TOL
// ---- the pre-test of the two-phase search (exact library) ----
// A patch cost is cs / ws = sum c_k w_k / sum w_k with c_k >= 0 and w_k = gsp_k fast_exp(-(a2_k + t_k) / s): a2_k is the SOURCE half of the
// weight's argument (the pixel against its own sample), t_k >= 0 the target half, so w_k <= u_k := gsp_k fast_exp(-a2_k / s) whatever the
// guess.  With A = the EPPM_SEARCH_PRE_ROWS centre rows of the patch:  cs / ws >= sum_A c_k w_k / (sum_A w_k + sum_{not A} u_k).
// u_k of one sample: rest_weight_term (eppm_device.cuh)
// sum_A c_k w_k and sum_A w_k of a guess: rows A of search_patch_dist's parity-plane form (PK = 2) -- the same loads, the same terms, row major
template <int RT, class LUT>
__device__ __forceinline__ void search_patch_centre_rows(const Planes& P, const LUT& L, const float4* __restrict__ s_src, int TW, int tx, int ty,
                                                         int x2, int y2, const PlanesH& PH, float& cs, float& ws)
{
    constexpr int S = RT + 1, I0 = pre_row0(S);
    static_assert(S % 4 == 2 && EPPM_SEARCH_PRE_ROWS >= 1 && EPPM_SEARCH_PRE_ROWS <= S, "rows of whole dwordx4 gathers + one dwordx2");
    const int pitch16 = P.pitch << 4;
    const rgbf c1 = texel_rgb(s_src[(ty + RT) * TW + tx + RT]);
    const rgbf c2 = texel_rgb(texel_at(P.pk2, texel_off(pitch16, P.w, P.h, x2, y2)));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(PH.pp2), 0, 2 * P.h * PH.pp_pitch * 4, 0x00020000);
    const int xp = x2 - RT + PH.pp_pad;
    const int rb = ((xp & 1) * P.h) * PH.pp_pitch + (xp >> 1);
    cs = 0.0f; ws = 0.0f;
#pragma unroll 2
    for (int ii = I0; ii < I0 + EPPM_SEARCH_PRE_ROWS; ii++) {
        const int ro = (rb + iclamp(y2 + 2 * ii - RT, 0, P.h - 1) * PH.pp_pitch) * 4;
        const float4* __restrict__ srow = s_src + (ty + 2 * ii) * TW + tx;
        uint32_t wq[S];
#pragma unroll
        for (int g = 0; g < S / 4; g++) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, ro + 16 * g, 0, 0);
            wq[4 * g] = v.x; wq[4 * g + 1] = v.y; wq[4 * g + 2] = v.z; wq[4 * g + 3] = v.w;
        }
        { const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, ro + 4 * (S - 2), 0, 0); wq[S - 2] = v.x; wq[S - 1] = v.y; }
EPPM_PM_UNROLL(((S % 5 == 0) ? 5 : S))
        for (int jj = 0; jj < S; jj++) {
            float ct, wt;
            patch_terms(srow[2 * jj], unpack_texel(wq[jj], 0u), c1, c2, L.gsp[ii * S + jj], L.tab(), ct, wt);
            patch_accum(cs, ws, ct, wt);
        }
    }
}
#endif

// the (kBlock + 2 RT)^2 source samples around the 16x16 block (bx, by), clamped at load, staged by the 256 threads of a workgroup (no
// barrier): the cost-field kernels (k_pm_cost_field_tile and the seeded start's k_pm_cost_select_tile evaluate from the same tile)
// and phase A of the speculative sweeps (k_pm_sweep_spec, k_pm_spec_all)
template <int RT>
__device__ __forceinline__ void pm_stage_tile(float4* __restrict__ s_src, const Planes& P, int bx, int by, int tid)
{
    constexpr int TW = kBlock + 2 * RT;
    const int x0 = bx * kBlock - RT, y0 = by * kBlock - RT;
    for (int t = tid; t < TW * TW; t += 256) {
        const int sy = iclamp(y0 + t / TW, 0, P.h - 1), sx = iclamp(x0 + t % TW, 0, P.w - 1);
        s_src[t] = P.pk1[(unsigned)(sy * P.pitch + sx)];
    }
}

// the parity-adoption rule (EPPM_PARITY_* above): which launches read the target's column-parity plane
static inline bool pm_parity_adopted(int R, bool exact_adopts)
{
#ifdef EPPM_TOL
    (void)exact_adopts;
    return R == 9 || R == 17;
#else
    return exact_adopts && R == 9;
#endif
}
static inline bool pm_has_parity(const PmBatch& b, int R, bool exact_adopts)
{
    return pm_parity_adopted(R, exact_adopts) && b.p[0].P.pp2 && (b.n < 2 || b.p[1].P.pp2);
}

// lane i receives lane i-1: inside a 16-lane DPP row (row_ror:1) or across the whole wave (wave_shr:1, gfx9)
template <int LPC>
__device__ __forceinline__ float dpp_prev_lane(float v)
{
    if (LPC == 4) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x93 /* quad_perm:[3,0,1,2] */, 0xf, 0xf, false));
    if (LPC == 16) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /* row_ror:1 */, 0xf, 0xf, false));
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// Samples per lane of a cooperative evaluation.  Exact library: the S*S samples dealt evenly to the LPC lanes.  Tolerance library: a lane
// = a chunk of the canonical summation order (eppm_device.cuh: PatchSum) -- 5 samples at radius 9 (20 of 32 lanes work), 6 at radius 17
// (54 of 64) --, whatever LPC is.
template <int R, int LPC>
__host__ __device__ constexpr int coop_chunk()
{
#ifdef EPPM_TOL
    return tol_chunk(R);
#else
    return ((R + 1) * (R + 1) + LPC - 1) / LPC;
#endif
}
// The sums of a cooperative evaluation from the lanes' terms tc[], tw[] (zero past the last sample); complete in lane NL - 1 of the group.
// Exact library: the two running sums hop lane to lane while EVERY lane adds its whole chunk at every hop -- the additions happen in the
// reference's order (only the sum that travels through lane ln at hop ln is the real one).  Tolerance library: every lane first sums
// its own chunk from zero (fused multiply-adds), then the totals hop with one addition per hop: the canonical order of PatchSum, the
// same bits as a lane that evaluates alone.  (A DPP tree instead of the hops was 8 % cheaper and wrong: its result differed in the
// last bit from the serial kernels' and even between the lanes of one chain, and on images whose candidates TIE -- flat regions, saturated
// blocks -- strict "<" then accepted in one kernel what another had stored as equal: 0.34 px on a fuzz case)
template <int LPC, int CH, int NS, int NL>
__device__ __forceinline__ void coop_chain_sum(const float (&tc)[CH], const float (&tw)[CH], float& ac, float& aw)
{
#ifdef EPPM_TOL
    float pc = 0.0f, pw = 0.0f;
#pragma unroll
    for (int q = 0; q < CH; q++) patch_accum(pc, pw, tc[q], tw[q]);
#pragma unroll
    for (int ln = 0; ln < NL; ln++) {
        if (ln > 0) { ac = dpp_prev_lane<LPC>(ac); aw = dpp_prev_lane<LPC>(aw); }
        ac += pc; aw += pw;
    }
#else
#pragma unroll
    for (int ln = 0; ln < NL; ln++) {
        if (ln > 0) { ac = dpp_prev_lane<LPC>(ac); aw = dpp_prev_lane<LPC>(aw); }
#pragma unroll
        for (int q = 0; q < CH; q++) {
            if (ln * CH + q < NS) patch_accum(ac, aw, tc[q], tw[q]);
        }
    }
#endif
}

// One patch evaluation spread over the LPC lanes of a DPP row (16) or of a whole wave (64), for kernels whose source samples lie in
// the (kBlock + 2 RT)^2 LDS tile of a 16x16 block: the S*S samples are dealt to the lanes in contiguous chunks, each lane forms the
// terms of its chunk, and the two running sums hop lane to lane while every lane adds its chunk -- the reference's order of additions,
// as in the cooperative sweep.  r = lane within the group; every lane of the group returns the cost.
template <int RT, int LPC, class LUT>
__device__ __forceinline__ float coop_patch_dist(const Planes& P, const LUT& L, const float4* __restrict__ s_src, int TW, int tx, int ty,
                                                 int x2, int y2, int r)
{
    constexpr int S = RT + 1, NS = S * S, CH = coop_chunk<RT, LPC>(), NL = (NS + CH - 1) / CH;
    static_assert(NL <= LPC, "a lane per chunk");
    const int pitch16 = P.pitch << 4, wmax16 = (P.w - 1) << 4;
    const rgbf c1 = texel_rgb(s_src[(ty + RT) * TW + tx + RT]);
    const rgbf c2 = texel_rgb(texel_at(P.pk2, texel_off(pitch16, P.w, P.h, x2, y2)));
    const int t0 = r * CH;
    float tc[CH], tw[CH];
    float4 q2[CH];
    int so[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int t = min(t0 + k, NS - 1), ii = t / S, jj = t - ii * S;
        so[k] = (ty + 2 * ii) * TW + tx + 2 * jj;
        q2[k] = texel_at(P.pk2, texel_off16(pitch16, wmax16, P.h - 1, (x2 + 2 * jj - RT) << 4, y2 + 2 * ii - RT));
    }
#pragma unroll
    for (int k = 0; k < CH; k++) {
        tc[k] = 0.0f; tw[k] = 0.0f;
        if (t0 + k < NS) patch_terms(s_src[so[k]], q2[k], c1, c2, L.gsp[t0 + k], L.tab(), tc[k], tw[k]);
    }
    float ac = 0.0f, aw = 0.0f;
    coop_chain_sum<LPC, CH, NS, NL>(tc, tw, ac, aw);
    const int src = ((threadIdx.x & 63) / LPC) * LPC + (NL - 1);      // lane holding the complete sums (wave-relative)
    return __shfl(ac, src, 64) / __shfl(aw, src, 64);
}

// ---- merged form of the speculative sweeps: lists and stamps of all four directions live side by side --------------------------
// PmProblem::wl beyond the two-launch form's words: counters wl[8 + 4 * (iteration & 1) + d]; stamps [16 + 2U + d U, ..) = 1 + the
// iteration that listed the unit last; lists [16 + 6U + d U, ..).  d: 0 row forward, 1 column forward, 2 row reverse, 3 column reverse.
// Lists the unit (segments 2u, 2u + 1 of its line) whose chains visit pixel (px, py) in direction d, once per iteration.
__device__ __forceinline__ void merged_list_unit(uint32_t* __restrict__ wl, const PmBatch& B, int d, int px, int py)
{
    const bool row = (d & 1) == 0;
    const int along = row ? px : py, ln = row ? py : px, nseg = row ? B.nseg_row : B.nseg_col;
    const unsigned seg = (d < 2 && along < B.seg_len) ? 0u : (unsigned)(along / B.seg_len);
    const unsigned unit = (unsigned)ln * ((unsigned)(nseg + 1) >> 1) + (seg >> 1), U = (unsigned)B.wl_units, seq1 = (unsigned)B.merged_it + 1u;
    if (atomicMax(&wl[16 + 2 * U + d * U + unit], seq1) < seq1)
        wl[16 + 6 * U + d * U + atomicAdd(&wl[8 + 4 * (B.merged_it & 1) + d], 1u)] = unit;
}

// the chains of a k_pm_sweep workgroup with a source tile (k_pm_sweep.hip, TILE): SEGS consecutive segments of LINES lines of equal parity
template <int LPC> struct SweepTile { static constexpr int CPB = 256 / LPC, SEGS = (CPB >= 16) ? 4 : 2, LINES = CPB / SEGS; };
// the longest segment whose chains' pixels are fetched before the first step (k_pm_sweep: SPEC, PRE, MERGED)
constexpr int kSpecMaxSteps = 16;

}  // namespace eppm
