// k_pm_field.hip -- PatchMatch, where an iteration starts from: the random field, the cost field, and the seeded start's select
// (reference: bao_pmflow_kernel.cu:50-109, :636-645).  Shared helpers and the tuning knobs: pm_device.cuh.
#include "pm_device.cuh"

namespace eppm {

// ---------------------------------------------------------------------------------------------------
// Random initial NNF (d_setup_randgen + d_gen_rand_field, kernel.cu:50-109).  The reference lets thread
// (0,0) of each 16x16 block draw 2x256 numbers serially from the block's XORWOW stream; here the 64
// lanes of one wave each own 8 consecutive draws of the same stream (lane states precomputed on the
// host by walking the stream once, eppm_api.cpp rng_create), so the numbers are identical and the draw
// is parallel.  Also rewinds the search states to the position after the 512 init draws.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pm_init_field(PmBatch B, PmRngDev rng)
{
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const int bx = blockIdx.x, by = blockIdx.y, lane = threadIdx.x;
    const int w = pr.P.w, h = pr.P.h;
    const int block_id = by * rng.gx + bx;
    const size_t so = ((size_t)block_id * 64 + lane) * 6;
    Xorwow st = load_state(rng.init_tab + so);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t r1 = xorwow_next(st);
        const uint32_t r2 = xorwow_next(st);
        const int t = lane * 4 + q;                // t = 16*i + j, row-major over the block (kernel.cu:90-101)
        const int x = bx * kBlock + (t & 15), y = by * kBlock + (t >> 4);
        if (x < w && y < h) {
            pr.nnf[(y * B.npitch + x) * 2 + 0] = (int16_t)(r1 % (uint32_t)(w + 1));
            pr.nnf[(y * B.npitch + x) * 2 + 1] = (int16_t)(r2 % (uint32_t)(h + 1));
            if (pr.scand) {                      // new images: the sweeps' evaluation cache starts empty
#pragma unroll
                for (int d = 0; d < 4; d++) pr.scand[d * B.cache_plane + y * B.cpitch + x] = -1;
            }
        }
    }
    // search stream position = 512 draws in (states are re-initialised on every call, kernel.cu:160)
#pragma unroll
    for (int k = 0; k < 6; k++) pr.rng_work[so + k] = rng.iter_tab[so + k];
    // a new run: sweep numbers start at 0 again, so the work list's lengths and stamps do
    if (pr.wl)
        for (int wi = block_id * 64 + lane; wi < 16 + 6 * B.wl_units; wi += rng.gx * rng.gy * 64) pr.wl[wi] = 0u;
}

void launch_pm_init_field(const PmBatch& b, const PmRngDev& rng, hipStream_t s)
{
    hipLaunchKernelGGL(k_pm_init_field, dim3(rng.gx, rng.gy, b.n * b.npairs), dim3(64), 0, s, b, rng);
}

// ---------------------------------------------------------------------------------------------------
// Initial cost field (kernel.cu:636-645)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pm_cost_field(PmBatch B, const float* __restrict__ lut, int R)
{
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    load_patch_lut(L, lut, R, threadIdx.y * kBlock + threadIdx.x, 256);
    __syncthreads();
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const Planes P = to_dev(pr.P);
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const int dx = pr.nnf[(y * B.npitch + x) * 2], dy = pr.nnf[(y * B.npitch + x) * 2 + 1];
    pr.cost[y * B.cpitch + x] = patch_dist(P, L, R, x, y, dx, dy);
}

// the cost field with the source samples of the 16x16 block from an LDS tile, as in the search and in phase A of the sweeps (radius 9 / 17)
template <int RT, int PK = 0>
__global__ __launch_bounds__(256) void k_pm_cost_field_tile(PmBatch B, const float* __restrict__ lut, int R)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = kBlock + 2 * RT;
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
    const int dx = pr.nnf[(y * B.npitch + x) * 2], dy = pr.nnf[(y * B.npitch + x) * 2 + 1];
    pr.cost[y * B.cpitch + x] = search_patch_dist<RT, PK>(P, L, R, s_src, TW, threadIdx.x, threadIdx.y, x, y, dx, dy, pr.P);
}

int pm_parity_kernels(int R)
{
    return (pm_parity_adopted(R, EPPM_PARITY_SEARCH) ? 1 : 0) | (pm_parity_adopted(R, EPPM_PARITY_SPEC) ? 2 : 0) | (pm_parity_adopted(R, EPPM_PARITY_COST) ? 4 : 0);
}

// which cost-field kernel a launch takes (the plain field and the seeded start's select pick by ONE rule, so that a prior's cost is the
// cost the field would give the same match): 0 any radius, 1 / 2 the LDS tile at radius 9 / 17, 3 / 4 the same reading the parity planes
static int pm_cost_kernel(const PmBatch& b, int R)
{
    if (!EPPM_COST_FIELD_TILE || (R != 9 && R != 17)) return 0;
    return (R == 9 ? 1 : 2) + (pm_has_parity(b, R, EPPM_PARITY_COST) ? 2 : 0);
}

void launch_pm_cost_field(const PmBatch& b, const float* lut, int R, hipStream_t s)
{
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    dim3 grid((w + kBlock - 1) / kBlock, (h + kBlock - 1) / kBlock, b.n * b.npairs), block(kBlock, kBlock);
    switch (pm_cost_kernel(b, R)) {
    case 3: hipLaunchKernelGGL((k_pm_cost_field_tile<9, 2>), grid, block, 0, s, b, lut, R); break;
    case 4: hipLaunchKernelGGL((k_pm_cost_field_tile<17, 2>), grid, block, 0, s, b, lut, R); break;
    case 1: hipLaunchKernelGGL(k_pm_cost_field_tile<9>, grid, block, 0, s, b, lut, R); break;
    case 2: hipLaunchKernelGGL(k_pm_cost_field_tile<17>, grid, block, 0, s, b, lut, R); break;
    default: hipLaunchKernelGGL(k_pm_cost_field, grid, block, 0, s, b, lut, R);
    }
}

// The seeded start (eppm_internal.h: PmSeed): the cost-field kernels above, evaluating the temporal prior instead of the stored match and
// keeping it where it is strictly cheaper.  Same evaluation function per radius and library as launch_pm_cost_field picks, so a prior's cost
// is bit for bit what the cost field would give that match.  A pixel without a prior skips its evaluation.  Problem z of the launch is
// direction z % n of slot z / n (pm_problem's decomposition): the prior and the copies are that slot's planes of that direction.
struct PmSeedDir { const int16_t* prior; int16_t* nnf_init; float* cost_init; };
__device__ __forceinline__ PmSeedDir pm_seed_dir(const PmBatch& B, const PmSeed& S, unsigned z)
{
    const unsigned k = z % (unsigned)B.n, slot = z / (unsigned)B.n;
    return PmSeedDir{pair_ptr(S.prior[k], S.stride, slot), pair_ptr(S.nnf_init[k], S.stride, slot), pair_ptr(S.cost_init[k], S.stride, slot)};
}
__device__ __forceinline__ void pm_select_store(const PmProblem& pr, const PmBatch& B, const PmSeedDir& D, int w, int x, int y, bool has,
                                                int px, int py, float pc)
{
    const int ni = (y * B.npitch + x) * 2, ci = y * B.cpitch + x;
    int nx = pr.nnf[ni], ny = pr.nnf[ni + 1];
    float c = pr.cost[ci];
    if (has && pc < c) {
        nx = px; ny = py; c = pc;
        pr.nnf[ni] = (int16_t)nx; pr.nnf[ni + 1] = (int16_t)ny;
        pr.cost[ci] = c;
    }
    D.nnf_init[(y * w + x) * 2] = (int16_t)nx;
    D.nnf_init[(y * w + x) * 2 + 1] = (int16_t)ny;
    D.cost_init[y * w + x] = c;
}

__global__ __launch_bounds__(256) void k_pm_cost_select(PmBatch B, PmSeed S, const float* __restrict__ lut, int R)
{
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    load_patch_lut(L, lut, R, threadIdx.y * kBlock + threadIdx.x, 256);
    __syncthreads();
    const PmSeedDir D = pm_seed_dir(B, S, blockIdx.z);
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const Planes P = to_dev(pr.P);
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const int px = D.prior[(y * P.w + x) * 2], py = D.prior[(y * P.w + x) * 2 + 1];
    const bool has = px > kInvalid && py > kInvalid;
    const float pc = has ? patch_dist(P, L, R, x, y, px, py) : 0.0f;
    pm_select_store(pr, B, D, P.w, x, y, has, px, py, pc);
}

template <int RT, int PK = 0>
__global__ __launch_bounds__(256) void k_pm_cost_select_tile(PmBatch B, PmSeed S, const float* __restrict__ lut, int R)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = kBlock + 2 * RT;
    __shared__ float4 s_src[TW * TW];
    __shared__ EPPM_LUT_ALIGN LUT L;
    const int tid = threadIdx.y * kBlock + threadIdx.x;
    load_patch_lut(L, lut, R, tid, 256);
    const PmSeedDir D = pm_seed_dir(B, S, blockIdx.z);
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const Planes P = to_dev(pr.P);
    pm_stage_tile<RT>(s_src, P, blockIdx.x, blockIdx.y, tid);
    __syncthreads();
    const int x = blockIdx.x * kBlock + threadIdx.x, y = blockIdx.y * kBlock + threadIdx.y;
    if (x >= P.w || y >= P.h) return;
    const int px = D.prior[(y * P.w + x) * 2], py = D.prior[(y * P.w + x) * 2 + 1];
    const bool has = px > kInvalid && py > kInvalid;
    const float pc = has ? search_patch_dist<RT, PK>(P, L, R, s_src, TW, threadIdx.x, threadIdx.y, x, y, px, py, pr.P) : 0.0f;
    pm_select_store(pr, B, D, P.w, x, y, has, px, py, pc);
}

void launch_pm_cost_select(const PmBatch& b, const PmSeed& seed, const float* lut, int R, hipStream_t s)
{
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    dim3 grid((w + kBlock - 1) / kBlock, (h + kBlock - 1) / kBlock, b.n * b.npairs), block(kBlock, kBlock);
    switch (pm_cost_kernel(b, R)) {
    case 3: hipLaunchKernelGGL((k_pm_cost_select_tile<9, 2>), grid, block, 0, s, b, seed, lut, R); break;
    case 4: hipLaunchKernelGGL((k_pm_cost_select_tile<17, 2>), grid, block, 0, s, b, seed, lut, R); break;
    case 1: hipLaunchKernelGGL(k_pm_cost_select_tile<9>, grid, block, 0, s, b, seed, lut, R); break;
    case 2: hipLaunchKernelGGL(k_pm_cost_select_tile<17>, grid, block, 0, s, b, seed, lut, R); break;
    default: hipLaunchKernelGGL(k_pm_cost_select, grid, block, 0, s, b, seed, lut, R);
    }
}

}  // namespace eppm
// The search is compiled in this translation unit: alone, two of its exact-library kernels (k_pm_random_search<0> and <17, 2, true>) get
// other instructions than next to the cost-field kernels, which share search_patch_dist with them (tools/kernel_isa.sh shows it)
#include "k_pm_search.hip"
