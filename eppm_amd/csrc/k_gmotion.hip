// k_gmotion.hip -- global camera motion and stabilisation (gmotion.h): a step of every slot it covers (blockIdx.z /
// blockIdx.x of the solve) is iters x (k_gmotion_accumulate, k_gmotion_solve) and one k_stab_warp.
//   accumulate  a block of 64 x 4 lanes sums a tile of 64 x 16 pixels: every lane walks four rows, so a wave reads 512 B of flow and 64 B of
//               mask per row, coalesced.  The twelve sums are 64-bit integers -- exact in any order --, reduced across the wave by
//               shuffles, across the four waves through LDS and stored as one 128-byte slab per block.  No atomics, no fences, no tickets:
//               the slabs are combined by the next launch, so the result is the same bits on every run and equals the host form's.
//   solve       one wave per slot: its lanes stride over the slot's slabs, shuffle-reduce, and lane 0 runs gmotion.h's solve; after the
//               last pass it also moves the slot's path and leaves the warp.
//   warp        one lane per pixel: the mask byte of image 1's pixel against the final model and the output word of the same (x, y).
// There is no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "gmotion.h"

namespace eppm {

namespace {

__device__ __forceinline__ bool gm_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

__device__ __forceinline__ void gm_wave_sum(int64_t (&s)[kGmSums])
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kGmSums; k++) s[k] += (int64_t)__shfl_xor((long long)s[k], off, 64);
}

struct GmPx {             // image 2's word at an in-frame pixel
    const uint8_t* __restrict__ img;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(img + (size_t)y * pitch + (size_t)x * 4); }
};

}  // namespace

__global__ __launch_bounds__(256) void k_gmotion_accumulate(StabArgs A)
{
    __shared__ int64_t part[4][kGmSums];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    char* __restrict__ blk = pair_ptr(A.mem, A.slot_stride, slot);
    const GmModel* m = reinterpret_cast<const GmModel*>(blk + A.off_model);
    const float2* __restrict__ flow = reinterpret_cast<const float2*>(pair_ptr(A.fwd, A.fwd_stride, pair));
    const uint8_t* __restrict__ occ = pair_ptr(A.occ1, A.occ_stride, pair);
    float pf[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool prev_valid = true;
    if (A.pass > 0) {
        prev_valid = m->valid != 0;
#pragma unroll
        for (int k = 0; k < 6; k++) pf[k] = m->pf[k];
    }
    int64_t s[kGmSums];
#pragma unroll
    for (int k = 0; k < kGmSums; k++) s[k] = 0;
    const int x = blockIdx.x * kGmTileW + threadIdx.x;
    if (x < A.w && prev_valid) {
        const int X = gm_X(x, A.w);
#pragma unroll
        for (int r = 0; r < kGmTileH / 4; r++) {
            const int y = blockIdx.y * kGmTileH + r * 4 + threadIdx.y;
            if (y >= A.h) break;
            const size_t i = (size_t)y * A.w + x;
            const float2 f = flow[i];
            const int Y = gm_Y(y, A.h);
            if (gm_valid(f.x, f.y, occ[i]) && (A.pass == 0 || gm_inlier(f.x, f.y, X, Y, pf, A.tau2))) gm_accumulate(s, X, Y, f.x, f.y);
        }
    }
    gm_wave_sum(s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kGmSums; k++) part[threadIdx.y][k] = s[k];
    }
    __syncthreads();
    const unsigned t = threadIdx.y * 64 + threadIdx.x;
    if (t < kGmSlabBytes / 8) {
        int64_t* __restrict__ slab = reinterpret_cast<int64_t*>(blk + (size_t)(blockIdx.y * A.tiles_x + blockIdx.x) * kGmSlabBytes);
        slab[t] = t < kGmSums ? (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]) : 0;
    }
}

__global__ __launch_bounds__(64) void k_gmotion_solve(StabArgs A)
{
    const unsigned pair = blockIdx.x, slot = A.slot0 + pair;
    char* __restrict__ blk = pair_ptr(A.mem, A.slot_stride, slot);
    GmModel* m = reinterpret_cast<GmModel*>(blk + A.off_model);
    GmState* st = reinterpret_cast<GmState*>(blk + A.off_model + sizeof(GmModel));
    const int nslabs = A.tiles_x * A.tiles_y;
    int64_t s[kGmSums];
#pragma unroll
    for (int k = 0; k < kGmSums; k++) s[k] = 0;
    for (int i = threadIdx.x; i < nslabs; i += 64) {
        const int64_t* __restrict__ slab = reinterpret_cast<const int64_t*>(blk + (size_t)i * kGmSlabBytes);
#pragma unroll
        for (int k = 0; k < kGmSums; k++) s[k] += slab[k];
    }
    gm_wave_sum(s);
    if (threadIdx.x != 0) return;
    GmModel mm;
    if (A.pass > 0) mm = *m;
    if (A.pass == 0 || mm.valid) {          // a pass after an invalid model leaves it as it is: the fit stopped there
        gm_model_from_sums(&mm, s, A.pass);
        *m = mm;
    }
    if (A.pass == A.iters - 1) {
        GmState ss = *st;
        gm_update(&ss, mm.p, mm.valid != 0, A.smooth, gm_bit(A.empty, slot), gm_bit(A.cut, slot));
        *st = ss;
    }
}

__global__ __launch_bounds__(256) void k_stab_warp(StabArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    char* __restrict__ blk = pair_ptr(A.mem, A.slot_stride, slot);
    const GmModel* m = reinterpret_cast<const GmModel*>(blk + A.off_model);
    const GmState* st = reinterpret_cast<const GmState*>(blk + A.off_model + sizeof(GmModel));
    GmModel mm;
    mm.valid = m->valid;
    float wf[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        mm.pf[k] = m->pf[k];
        wf[k] = st->wf[k];
    }
    const size_t i = (size_t)y * A.w + x;
    const float2 f = reinterpret_cast<const float2*>(pair_ptr(A.fwd, A.fwd_stride, pair))[i];
    const uint8_t o = pair_ptr(A.occ1, A.occ_stride, pair)[i];
    const GmPx P{pair_ptr(A.img2, A.img_stride, pair), A.img_pitch};
    reinterpret_cast<uint32_t*>(blk + A.off_out)[i] = gm_warp_pixel(x, y, wf, A.h, A.w, P);
    reinterpret_cast<uint8_t*>(blk + A.off_mask)[i] = gm_mask(f.x, f.y, o, gm_X(x, A.w), gm_Y(y, A.h), mm, A.tau2);
}

void launch_gmotion_accumulate(const StabArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_gmotion_accumulate, dim3(a.tiles_x, a.tiles_y, a.n), dim3(64, 4), 0, s, a);
}

void launch_gmotion_solve(const StabArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_gmotion_solve, dim3(a.n), dim3(64), 0, s, a); }

void launch_stab_warp(const StabArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_stab_warp, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

}  // namespace eppm
