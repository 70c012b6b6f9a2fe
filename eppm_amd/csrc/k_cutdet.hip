// k_cutdet.hip -- scene-cut detection from a pair's bidirectional flow (cutdet.h): a step of every slot it covers
// (blockIdx.z / blockIdx.x of the finish) is one k_cutdet_accumulate and one k_cutdet_finish.
//   accumulate  a block of 64 x 4 lanes sums a tile of 64 x 16 pixels: every lane walks four rows of its column, so a wave reads 256 B of
//               image 2, 512 B of backward flow and 2 x 64 B of masks per row, coalesced, and gathers one word of image 1 per tracked
//               pixel.  The ten sums are uint32 in the lane (at most 4 x 255), the wave (shuffles) and the tile (LDS; at most 1024 x 255),
//               stored as one 64-byte slab per block.  No atomics, no fences, no tickets: the slabs are combined by the next launch, so
//               the result is the same bits on every run and equals the host form's.
//   finish      one wave per slot: its lanes stride over the slot's slabs in 64-bit sums, shuffle-reduce, and lane 0 applies cutdet.h's
//               verdict and stores the record.
// There is no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "cutdet.h"

namespace eppm {

namespace {

struct CutPx {            // image 1's word at an in-frame pixel
    const uint8_t* __restrict__ img;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(img + (size_t)y * pitch + (size_t)x * 4); }
};

}  // namespace

__global__ __launch_bounds__(256) void k_cutdet_accumulate(CutArgs A)
{
    __shared__ uint32_t part[4][kCutSums];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const CutPx P1{pair_ptr(A.img1, A.img_stride, pair), A.img_pitch};
    const uint8_t* __restrict__ img2 = pair_ptr(A.img2, A.img_stride, pair);
    const float2* __restrict__ bwd = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair));
    const uint8_t* __restrict__ occ1 = pair_ptr(A.occ1, A.occ_stride, pair);
    const uint8_t* __restrict__ occ2 = pair_ptr(A.occ2, A.occ_stride, pair);
    uint32_t s[kCutSums];
#pragma unroll
    for (int k = 0; k < kCutSums; k++) s[k] = 0;
    const int x = blockIdx.x * kCutTileW + threadIdx.x;
    if (x < A.w) {
#pragma unroll
        for (int r = 0; r < kCutTileH / 4; r++) {
            const int y = blockIdx.y * kCutTileH + r * 4 + threadIdx.y;
            if (y >= A.h) break;
            const size_t i = (size_t)y * A.w + x;
            const uint32_t cur = *reinterpret_cast<const uint32_t*>(img2 + (size_t)y * A.img_pitch + (size_t)x * 4);
            const float2 f = bwd[i];
            cut_pixel(s, x, y, occ1[i], cur, f.x, f.y, occ2[i], A.h, A.w, P1);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kCutSums; k++) s[k] += (uint32_t)__shfl_xor((int)s[k], off, 64);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kCutSums; k++) part[threadIdx.y][k] = s[k];
    }
    __syncthreads();
    const unsigned t = threadIdx.y * 64 + threadIdx.x;
    if (t < kCutSlabBytes / 4) {
        uint32_t* __restrict__ slab = reinterpret_cast<uint32_t*>(A.mem + A.off_slabs + (size_t)slot * A.slab_stride +
                                                                  (size_t)(blockIdx.y * A.tiles_x + blockIdx.x) * kCutSlabBytes);
        slab[t] = t < kCutSums ? (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]) : 0u;
    }
}

__global__ __launch_bounds__(64) void k_cutdet_finish(CutArgs A)
{
    const unsigned pair = blockIdx.x, slot = A.slot0 + pair;
    const char* __restrict__ slabs = A.mem + A.off_slabs + (size_t)slot * A.slab_stride;
    const int nslabs = A.tiles_x * A.tiles_y;
    int64_t s[kCutSums];
#pragma unroll
    for (int k = 0; k < kCutSums; k++) s[k] = 0;
    for (int i = threadIdx.x; i < nslabs; i += 64) {
        const uint32_t* __restrict__ slab = reinterpret_cast<const uint32_t*>(slabs + (size_t)i * kCutSlabBytes);
#pragma unroll
        for (int k = 0; k < kCutSums; k++) s[k] += (int64_t)slab[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kCutSums; k++) s[k] += (int64_t)__shfl_xor((long long)s[k], off, 64);
    if (threadIdx.x != 0) return;
    CutRecord r;
    cut_record(&r, s, (int64_t)A.h * A.w, A.lost_permille, A.r16);
    *reinterpret_cast<CutRecord*>(A.mem + (size_t)slot * kCutRecordStride) = r;
}

void launch_cutdet_accumulate(const CutArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_cutdet_accumulate, dim3(a.tiles_x, a.tiles_y, a.n), dim3(64, 4), 0, s, a);
}

void launch_cutdet_finish(const CutArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cutdet_finish, dim3(a.n), dim3(64), 0, s, a); }

}  // namespace eppm
