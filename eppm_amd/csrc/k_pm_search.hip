// k_pm_search.hip -- PatchMatch: the random search and the table of its numbers (reference: bao_pmflow_kernel.cu:1519-1594).
// Shared helpers (search_patch_dist) and the tuning knobs: pm_device.cuh.
#include "pm_device.cuh"

namespace eppm {

// ---------------------------------------------------------------------------------------------------
// Random search (kernel.cu:1519-1594): G guesses at radii search_range, /2, ... around the pre-search
// best, evaluated in order with strict <.
// Random numbers: the 16x16 block's XORWOW stream, 2x256 draws per guess in row-major pixel order.  One
// wave produces the 512*G draws of the launch in parallel (lane l owns draws [per_lane*l, per_lane*(l+1)) ),
// then jumps its state over the other lanes' draws with the GF(2) skip matrix so that the next launch
// continues the same stream.
// Evaluation: all guesses come from the pre-search best, so their costs are independent.  A workgroup
// covers a QUARTER of the reference's 16x16 block (4 rows, 64 pixels): wave k evaluates guess k of those 64
// pixels, the costs meet in LDS and wave 0 replays the reference's in-order strict-< selection.  The four
// quarter-workgroups of a block draw the same numbers (cheap); only quarter 0 advances the stored state.
// ---------------------------------------------------------------------------------------------------
// jump over the other 63 lanes' draws: v <- v * skip_mat over GF(2); Weyl counter by multiplication
__device__ __forceinline__ void xorwow_skip(Xorwow& st, const uint32_t* __restrict__ skip_mat, uint32_t skip_weyl)
{
    const uint32_t v[5] = {st.v0, st.v1, st.v2, st.v3, st.v4};
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
#pragma unroll
    for (int wd = 0; wd < 5; wd++) {
        const uint32_t vw = v[wd];
#pragma unroll 8
        for (int b = 0; b < 32; b++) {
            const uint32_t* row = skip_mat + (wd * 32 + b) * 5;
            const uint32_t m = 0u - ((vw >> b) & 1u);
            a0 ^= m & row[0]; a1 ^= m & row[1]; a2 ^= m & row[2]; a3 ^= m & row[3]; a4 ^= m & row[4];
        }
    }
    st.v0 = a0; st.v1 = a1; st.v2 = a2; st.v3 = a3; st.v4 = a4;
    st.d += skip_weyl;
}

// The draws of one search launch for every block, ahead of time (PmRngDev::rand_tab): one wave per 16x16 block does what wave G of
// the search does -- lane l draws numbers [per_lane*l, per_lane*(l+1)) of the block's stream as shorts, then jumps its state over the
// other lanes' draws -- and the states stay in `work` for the next launch's table.
__global__ __launch_bounds__(64) void k_pm_rand_table(PmRngDev rng, uint32_t* __restrict__ work, int16_t* __restrict__ tab, int G)
{
    const int block_id = blockIdx.x, lane = threadIdx.x;
    const size_t so = ((size_t)block_id * 64 + lane) * 6;
    Xorwow st = load_state(work + so);
    int16_t* __restrict__ out = tab + (size_t)block_id * 512 * G + rng.per_lane * lane;
    for (int q = 0; q < rng.per_lane; q++) out[q] = (int16_t)xorwow_next(st);
    xorwow_skip(st, rng.skip_mat, rng.skip_weyl);
    store_state(work + so, st);
}
void launch_pm_rand_table(const PmRngDev& rng, uint32_t* work, int16_t* tab, int G, hipStream_t s)
{
    hipLaunchKernelGGL(k_pm_rand_table, dim3(rng.gx * rng.gy), dim3(64), 0, s, rng, work, tab, G);
}

// TAB: the launch's random numbers come from PmRngDev::rand_tab (drawn ahead, see above): no drawing wave, no state, no LDS copy of the
// numbers -- a lane loads the two shorts of its pixel and guess -- and the workgroup is G waves instead of G + 1.
// ROWS = 2 (numbers drawn ahead only): a workgroup covers an EIGHTH of the block (2 rows, 32 pixels; a wave = two guesses of them) -- for
// launches of so few workgroups that their count per CU quantises badly (one 1024x436 pair: 872 quarter-workgroups on 256 CUs run as 4
// per CU where 3.4 are needed; the kernel runs at its CU's L1 rate, so the launch lasts as long as the fullest CU).
// PRE (exact library, quarter blocks, numbers drawn ahead, parity planes): the two-phase form.  Phase 1: every lane forms the sums of its
// guess over the centre rows of the patch only and rejects the guess when even the lower bound of its cost (pm_device.cuh:
// search_patch_centre_rows; the rest of the weight sum bounded by PmProblem::restw) cannot beat the pixel's stored cost.  The survivors of
// the workgroup are compacted into LDS.  Phase 2: up to EPPM_SEARCH_PRE_COOP_MAX survivors get 16 lanes each (coop_patch_dist), dealt over
// all waves of the workgroup; more than that are packed one per lane and evaluated by search_patch_dist.  Either way any lane serves any
// of the 64 pixels from the shared source tile, and the cost is the serial evaluation's bit for bit.  A rejected guess keeps INFINITY in
// s_cost, which the in-order selection treats as the reference treats a guess whose cost is not strictly lower: the results are the
// one-phase form's bit for bit.
template <int RT, int PK = 0, bool TAB = false, int ROWS = 4, bool PRE = false>
__global__ __launch_bounds__(576) EPPM_SEARCH_OCC void k_pm_random_search(PmBatch B, PmRngDev rng, const float* __restrict__ lut, int R,
                                                          int search_range, int G)
{
    static_assert(ROWS == 4 || (ROWS == 2 && TAB && RT != 0), "eighth-block workgroups read their numbers from the table");
    static_assert(!PRE || (ROWS == 4 && TAB && RT != 0 && PK == 2), "the pre-test reads the parity planes; a wave per guess, no drawing wave");
    using LUT = typename SearchLut<RT>::type;
    constexpr int PIXW = 16 * ROWS, NSUB = kBlock / ROWS;        // pixels per workgroup, workgroups per 16x16 block
    constexpr int TW = (RT == 0) ? 1 : kBlock + 2 * RT, TH = (RT == 0) ? 1 : ROWS + 2 * RT;
    __shared__ float4 s_src[TW * TH];
    __shared__ EPPM_LUT_ALIGN LUT L;
    __shared__ int16_t s_rand[TAB ? 2 : 8 * 512];
    __shared__ float s_cost[8][64];
    __shared__ int s_guess[8][64];
    __shared__ uint32_t s_state[TAB ? 2 : 64 * 6];
    __shared__ uint16_t s_surv[PRE ? 8 * 64 : 1];               // PRE: the surviving (guess, pixel) lanes of the workgroup, as thread ids
    __shared__ int s_nsurv;
    (void)s_surv; (void)s_nsurv;
    // problem = id mod nprob (one problem per XCD L2, see k_pm_sweep); the rest of the id walks the quarter-blocks row by row
    const unsigned nprob = B.n * B.npairs, bq = blockIdx.x % nprob, brest = blockIdx.x / nprob;
    const int bxx = brest % rng.gx, byy = brest / rng.gx;
    const PmProblem pr = pm_problem(B, bq);
    const int tid = threadIdx.x;
    const int tile_y = byy / NSUB, quarter = byy % NSUB;
    const int block_id = tile_y * rng.gx + bxx;
    load_patch_lut(L, lut, R, tid, blockDim.x);
    if (!TAB && tid < 64) {
        const size_t so = ((size_t)block_id * 64 + tid) * 6;
        Xorwow st = load_state(pr.rng_work + so);
        const int base = rng.per_lane * tid;
        for (int q = 0; q < rng.per_lane; q++) s_rand[base + q] = (int16_t)xorwow_next(st);   // short(rdn), :1550-1551
        if (quarter == 0) store_state(s_state + tid * 6, st);     // advanced by wave G while the guesses are evaluated
    }
    if (PRE && tid == 0) s_nsurv = 0;
    const Planes P = to_dev(pr.P);
    if (RT != 0) {
        const int x0 = bxx * kBlock - RT, y0 = tile_y * kBlock + quarter * ROWS - RT;
        for (int t = tid; t < TW * TH; t += blockDim.x) {
            const int sy = iclamp(y0 + t / TW, 0, P.h - 1), sx = iclamp(x0 + t % TW, 0, P.w - 1);
            s_src[t] = P.pk1[(unsigned)(sy * P.pitch + sx)];
        }
    }
    __syncthreads();
    const int lane = tid % PIXW, k = tid / PIXW;                 // ROWS = 4: wave k = guess k; wave G advances the RNG states
    if (!TAB && k == G) {
        if (quarter == 0) {
            // Off the critical path: this wave has nothing else to do, the other G waves are evaluating guesses.  (Round 3 tried
            // giving the jump to the last guess's wave after its evaluation -- six waves per workgroup, four workgroups per CU
            // instead of three: slower, 1.40 -> 1.46 ms PatchMatch for one pair, -0.4 % batched: the jump then ends the workgroup.)
            const size_t so = ((size_t)block_id * 64 + lane) * 6;
            Xorwow st = load_state(s_state + lane * 6);
            xorwow_skip(st, rng.skip_mat, rng.skip_weyl);
            store_state(pr.rng_work_next + so, st);
        }
    }
    const int pix = quarter * PIXW + lane;                       // row-major index inside the 16x16 block
    const int x = bxx * kBlock + (pix & 15), y = tile_y * kBlock + (pix >> 4);
    const bool inimg = (k < G) && (x < P.w && y < P.h);
    const int nidx = y * B.npitch + x, cidx = y * B.cpitch + x;
    int bx = 0, by = 0;
    // sampling window of guess k: mag = search_range halved k times while >= 1 (:1564)
    int mag = search_range;
    for (int q = 0; q < k; q++) if (mag / 2 >= 1) mag /= 2;
    if (inimg) { bx = pr.nnf[nidx * 2]; by = pr.nnf[nidx * 2 + 1]; }
    int gx = 0, gy = 0;
    bool evaluate = false;
    if (inimg) {
        uint32_t rdn1, rdn2;                                                     // short -> unsigned int, :1558-1559
        if (TAB) {
            const uint32_t two = *reinterpret_cast<const uint32_t*>(rng.rand_tab + ((size_t)block_id * G + k) * 512 + 2 * pix);
            rdn1 = (uint32_t)(int32_t)(int16_t)(two & 0xffffu);
            rdn2 = (uint32_t)(int32_t)(int16_t)(two >> 16);
        } else {
            rdn1 = (uint32_t)(int32_t)s_rand[512 * k + 2 * pix];
            rdn2 = (uint32_t)(int32_t)s_rand[512 * k + 2 * pix + 1];
        }
        const int xmin = max(bx - mag, 0), xmax = min(bx + mag + 1, P.w + 1);
        const int ymin = max(by - mag, 0), ymax = min(by + mag + 1, P.h + 1);
        gx = (int)(int16_t)((uint32_t)xmin + rdn1 % (uint32_t)(xmax - xmin));
        gy = (int)(int16_t)((uint32_t)ymin + rdn2 % (uint32_t)(ymax - ymin));
        // A guess equal to the pixel's current match would reproduce the stored cost bit for bit (the skip rule of the sweeps): the
        // reference evaluates and rejects it ("<"), here the lane sits the evaluation out -- a ninth of the radius-1 guesses.
        evaluate = !(EPPM_SEARCH_SKIP_SAME && gx == bx && gy == by);
        s_guess[k][lane] = (gx & 0xffff) | (gy << 16);
    }
#ifndef EPPM_TOL
    if constexpr (PRE) {
        bool survives = false;
        if (inimg) {
            s_cost[k][lane] = INFINITY;
            if (evaluate) {
                float cs, ws;
                search_patch_centre_rows<RT>(P, L, s_src, TW, lane & 15, lane >> 4, gx, gy, pr.P, cs, ws);
                // products, no division: a NaN on either side compares false and the guess survives to its exact evaluation
                survives = !(cs * (1.0f - EPPM_SEARCH_PRE_EPS) >= pr.cost[cidx] * (ws + pr.restw[cidx]));
            }
        }
        const uint64_t m = __ballot(survives);
        int base = 0;
        if ((tid & 63) == 0 && m) base = atomicAdd(&s_nsurv, __popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (survives) s_surv[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)tid;
        __syncthreads();
        const int ns = s_nsurv;                                  // (at most 64 G survivors, 64 G threads)
        if (ns <= EPPM_SEARCH_PRE_COOP_MAX) {
            // Few survivors, the usual case once the field has converged: 16 lanes each (coop_patch_dist: the serial evaluation's bits), so
            // that every wave of the workgroup shares the work -- packed into one wave the survivors would keep the other waves, and the
            // wave slots they hold, waiting at the barrier below for a whole serial evaluation.
            constexpr int CL = 16;
            for (int slot = tid / CL; slot < ns; slot += (int)blockDim.x / CL) {
                const int e = s_surv[slot], sk = e >> 6, sl = e & 63, sg = s_guess[sk][sl];
                const float cv = coop_patch_dist<RT, CL>(P, L, s_src, TW, sl & 15, sl >> 4, (int)(int16_t)(sg & 0xffff), sg >> 16, tid % CL);
                if (tid % CL == 0) s_cost[sk][sl] = cv;
            }
        } else if (tid < ns) {
            const int e = s_surv[tid], sk = e >> 6, sl = e & 63, sg = s_guess[sk][sl];
            s_cost[sk][sl] = search_patch_dist<RT, PK>(P, L, R, s_src, TW, sl & 15, sl >> 4, 0, 0, (int)(int16_t)(sg & 0xffff), sg >> 16, pr.P);
        }
    } else
#endif
    if (inimg) {
        float cv = INFINITY;
        if (evaluate) {
            cv = search_patch_dist<RT, PK>(P, L, R, s_src, TW, lane & 15, lane >> 4, x, y, gx, gy, pr.P);
        }
        s_cost[k][lane] = cv;
    }
    __syncthreads();
    if (k == 0 && inimg) {
        float best_cost = pr.cost[cidx];
        for (int g = 0; g < G; g++) {
            const float cv = s_cost[g][lane];
            if (cv < best_cost) {
                const int e = s_guess[g][lane];
                bx = (int)(int16_t)(e & 0xffff); by = e >> 16; best_cost = cv;
            }
        }
        pr.nnf[nidx * 2] = (int16_t)bx;
        pr.nnf[nidx * 2 + 1] = (int16_t)by;
        pr.cost[cidx] = best_cost;
    }
}

#ifndef EPPM_TOL
// The rest-weight plane of the two-phase search (PmProblem::restw): per pixel the sum, row major, of u_k over the patch rows the pre-test
// does not evaluate.  It depends on the source image alone, so one launch serves the searches of a whole PatchMatch run.
template <int RT>
__global__ __launch_bounds__(256) void k_pm_rest_weight(PmBatch B, const float* __restrict__ lut, int R)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = kBlock + 2 * RT, S = RT + 1, I0 = pre_row0(S);
    __shared__ float4 s_src[TW * TW];
    __shared__ EPPM_LUT_ALIGN LUT L;
    const int tid = threadIdx.y * kBlock + threadIdx.x;
    load_patch_lut(L, lut, R, tid, 256);
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const Planes P = to_dev(pr.P);
    pm_stage_tile<RT>(s_src, P, blockIdx.x, blockIdx.y, tid);
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const rgbf c1 = texel_rgb(s_src[(threadIdx.y + RT) * TW + threadIdx.x + RT]);
    float u = 0.0f;
    for (int ii = 0; ii < S; ii++) {
        if (ii >= I0 && ii < I0 + EPPM_SEARCH_PRE_ROWS) continue;
        const float4* __restrict__ srow = s_src + (threadIdx.y + 2 * ii) * TW + threadIdx.x;
        for (int jj = 0; jj < S; jj++) u += rest_weight_term(c1, srow[2 * jj], L.gsp[ii * S + jj]);
    }
    pr.restw[y * B.cpitch + x] = u;
}
#endif
void launch_pm_rest_weight(const PmBatch& b, const float* lut, int R, hipStream_t s)
{
#ifndef EPPM_TOL
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    if (R == 9) hipLaunchKernelGGL(k_pm_rest_weight<9>, dim3((w + kBlock - 1) / kBlock, (h + kBlock - 1) / kBlock, b.n * b.npairs), dim3(kBlock, kBlock), 0, s, b, lut, R);
#endif
}

int pm_search_rows(int w, int h, int R, int problems, int npairs, bool table)
{
    const int quarter_wgs = ((w + kBlock - 1) / kBlock) * ((h + kBlock - 1) / kBlock) * 4 * problems * npairs;
    return (table && R == 9 && quarter_wgs < EPPM_SEARCH_HALF_BELOW_WGS) ? 2 : 4;
}

// Test support (include/eppm_test.h: eppm_test_pm_search): the pre-test's two sums with every pixel's STORED MATCH as the guess, formed by the
// search's own helper on the search's own tile (a quarter block per workgroup) -- what tools/search_pretest_model.py is compared with.
#ifndef EPPM_TOL
template <int RT>
__global__ __launch_bounds__(64) void k_pm_pretest_probe(PmBatch B, const float* __restrict__ lut, int R, PmPretestSums out)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = kBlock + 2 * RT, TH = 4 + 2 * RT;
    __shared__ float4 s_src[TW * TH];
    __shared__ EPPM_LUT_ALIGN LUT L;
    const int tid = threadIdx.x;
    load_patch_lut(L, lut, R, tid, 64);
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const Planes P = to_dev(pr.P);
    const int x0 = blockIdx.x * kBlock - RT, y0 = blockIdx.y * 4 - RT;
    for (int t = tid; t < TW * TH; t += 64) {
        const int sy = iclamp(y0 + t / TW, 0, P.h - 1), sx = iclamp(x0 + t % TW, 0, P.w - 1);
        s_src[t] = P.pk1[(unsigned)(sy * P.pitch + sx)];
    }
    __syncthreads();
    const int x = blockIdx.x * kBlock + (tid & 15), y = blockIdx.y * 4 + (tid >> 4);
    if (x >= P.w || y >= P.h) return;
    const int k = blockIdx.z % (unsigned)B.n, pair = blockIdx.z / (unsigned)B.n, nidx = y * B.npitch + x;
    float cs, ws;
    search_patch_centre_rows<RT>(P, L, s_src, TW, tid & 15, tid >> 4, pr.nnf[nidx * 2], pr.nnf[nidx * 2 + 1], pr.P, cs, ws);
    pair_ptr(k ? out.n[1] : out.n[0], B.stride, pair)[y * B.cpitch + x] = cs;
    pair_ptr(k ? out.d[1] : out.d[0], B.stride, pair)[y * B.cpitch + x] = ws;
}
#endif
void launch_pm_pretest_probe(const PmBatch& b, const float* lut, int R, const PmPretestSums& out, hipStream_t s)
{
#ifndef EPPM_TOL
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    if (R == 9) hipLaunchKernelGGL(k_pm_pretest_probe<9>, dim3((w + kBlock - 1) / kBlock, (h + 3) / 4, b.n * b.npairs), dim3(64), 0, s, b, lut, R, out);
#endif
}

// The launches that have a two-phase form: exact library, radius 9, quarter-block workgroups.
bool pm_search_pretest_form(int w, int h, int R, int problems, int npairs)
{
#ifdef EPPM_TOL
    return false;
#else
    return R == 9 && pm_search_rows(w, h, R, problems, npairs, true) == 4;
#endif
}
// the threshold is a measurement: the first iteration from which the two-phase launch is the shorter one
bool pm_search_pretest(int iteration, int w, int h, int R, int problems, int npairs)
{
    return EPPM_SEARCH_PRE_FROM >= 0 && iteration >= EPPM_SEARCH_PRE_FROM && pm_search_pretest_form(w, h, R, problems, npairs);
}
void pm_search_pretest_knobs(int R, int* row0, int* rows, int* from, float* eps)
{
    *row0 = pre_row0(R + 1); *rows = EPPM_SEARCH_PRE_ROWS; *from = EPPM_SEARCH_PRE_FROM; *eps = EPPM_SEARCH_PRE_EPS;
}
// what the two-phase form needs besides the decision: numbers drawn ahead, the parity planes, the rest-weight planes
bool pm_search_pretest_ready(const PmBatch& b, const PmRngDev& rng, int R)
{
    return rng.rand_tab && pm_has_parity(b, R, EPPM_PARITY_SEARCH) && b.p[0].restw && (b.n < 2 || b.p[1].restw);
}

void launch_pm_random_search(const PmBatch& b, const PmRngDev& rng, const float* lut, int R, int search_range, int num_guess,
                             hipStream_t s, bool pretest)
{
    dim3 grid(rng.gx * rng.gy * 4 * b.n * b.npairs), block(64 * (num_guess + 1));      // + the wave that advances the RNG states
    const bool have_pc = b.p[0].P.pc2 && (b.n < 2 || b.p[1].P.pc2);
    if (rng.rand_tab && (R == 9 || R == 17)) {                                         // numbers drawn ahead: G waves per workgroup
        dim3 blockt(64 * num_guess);
        const bool half = pm_search_rows(b.p[0].P.w, b.p[0].P.h, R, b.n, b.npairs, true) == 2;      // (radius 9 only)
#ifndef EPPM_TOL
        const bool two_phase = pretest && R == 9 && pm_has_parity(b, R, EPPM_PARITY_SEARCH) && pm_search_pretest_ready(b, rng, R);   // (the caller's decision: quarter blocks)
#else
        const bool two_phase = false;              // the tolerance library has no two-phase kernel
#endif
        launch_note(kLaunchSearch, b.p[0].P.w, b.p[0].P.h, b.npairs, (two_phase || !half) ? 4 : 2, two_phase);
        if (pm_has_parity(b, R, EPPM_PARITY_SEARCH)) {                                 // column-parity target planes
#ifndef EPPM_TOL
            if (two_phase) {
                hipLaunchKernelGGL((k_pm_random_search<9, 2, true, 4, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
                return;
            }
#endif
            if (half)
                hipLaunchKernelGGL((k_pm_random_search<9, 2, true, 2>), dim3(grid.x * 2), dim3(32 * num_guess), 0, s, b, rng, lut, R, search_range, num_guess);
            else if (R == 9) hipLaunchKernelGGL((k_pm_random_search<9, 2, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
            else hipLaunchKernelGGL((k_pm_random_search<17, 2, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
            return;
        }
        if (half) {
            hipLaunchKernelGGL((k_pm_random_search<9, 0, true, 2>), dim3(grid.x * 2), dim3(32 * num_guess), 0, s, b, rng, lut, R, search_range, num_guess);
            return;
        }
        if (R == 9) hipLaunchKernelGGL((k_pm_random_search<9, 0, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
        else if (have_pc) hipLaunchKernelGGL((k_pm_random_search<17, 1, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
        else hipLaunchKernelGGL((k_pm_random_search<17, 0, true>), grid, blockt, 0, s, b, rng, lut, R, search_range, num_guess);
        return;
    }
    // (radius 9 gathers the float4 plane: the 4-byte plane's conversions cost it more than the narrower gathers save, at every size)
    if (R == 17 && have_pc && EPPM_SEARCH_PK17) hipLaunchKernelGGL((k_pm_random_search<17, 1>), grid, block, 0, s, b, rng, lut, R, search_range, num_guess);
    else if (R == 9) hipLaunchKernelGGL(k_pm_random_search<9>, grid, block, 0, s, b, rng, lut, R, search_range, num_guess);
    else if (R == 17) hipLaunchKernelGGL(k_pm_random_search<17>, grid, block, 0, s, b, rng, lut, R, search_range, num_guess);
    else hipLaunchKernelGGL(k_pm_random_search<0>, grid, block, 0, s, b, rng, lut, R, search_range, num_guess);
}

}  // namespace eppm
