// k_deflicker.hip -- flicker removal (deflicker.h): per pass one accumulate and one field launch, then one apply
// launch, each for every slot the step covers (blockIdx.z).
//   accumulate   a 64 x 4 block walks the 64 x CELL pixels of 64 / CELL whole cells, a wave along a row, so that the frame word, the
//                backward vector and the mask byte are coalesced and no cell is shared between blocks.  A lane keeps the thirteen
//                integer sums of its column, the lanes of a cell add them by xor shuffles, the four waves through LDS, and 13 lanes per
//                cell store the record.  Integer sums do not depend on that order.  No atomics, no fences, no tickets.
//   field        one lane per cell: the float64 models of its 3 x 3 neighbourhood from their sums, the weighted average, the store.
//   apply        one lane per pixel in 64 x 4 blocks, as k_tfilter_step: the field at the pixel and the output word into the slot's other
//                reference plane.
// The arithmetic has no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "deflicker.h"

namespace eppm {

namespace {

__device__ __forceinline__ bool dk_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct DkRef {            // the reference of a slot: its current plane, or image 1 while the slot is empty
    const uint32_t* __restrict__ ref;
    const uint8_t* __restrict__ img1;
    size_t pitch;
    int w;
    bool empty;
    __device__ uint32_t operator()(int x, int y) const
    {
        if (empty) return *reinterpret_cast<const uint32_t*>(img1 + (size_t)y * pitch + (size_t)x * 4);
        return ref[(size_t)y * w + x];
    }
};

struct DkFieldAt {
    const float* __restrict__ f;
    int cx;
    __device__ const float* operator()(int i, int j) const { return f + ((size_t)j * cx + i) * kDkField; }
};

struct DkSumsAt {
    const uint32_t* __restrict__ s;
    int cx;
    __device__ const uint32_t* operator()(int i, int j) const { return s + ((size_t)j * cx + i) * kDkSums; }
};

}  // namespace

template <int CELL>
__global__ __launch_bounds__(256) void k_deflicker_accumulate(DeflickerArgs A)
{
    constexpr int NC = 64 / CELL;                 // cells of a block, side by side
    __shared__ uint32_t part[4][NC][kDkSums];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * 64 + tx, j = blockIdx.y;
    const size_t px = (size_t)A.h * A.w, cells = (size_t)A.cx * A.cy;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    uint32_t s[kDkSums];
#pragma unroll
    for (int k = 0; k < kDkSums; k++) s[k] = 0u;
    if (x < A.w) {
        const DkRef R{reinterpret_cast<const uint32_t*>(blk + deflicker_off_ref(px, dk_bit(A.cur, slot))), pair_ptr(A.img1, A.img_stride, pair),
                      A.img_pitch, A.w, dk_bit(A.empty, slot)};
        const DkFieldAt F{reinterpret_cast<const float*>(blk + deflicker_off_field(px, cells)), A.cx};
        const uint8_t* __restrict__ img2 = pair_ptr(A.img2, A.img_stride, pair);
        const float2* __restrict__ bwd = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair));
        const uint8_t* __restrict__ occ2 = pair_ptr(A.occ2, A.occ_stride, pair);
        const bool cut = dk_bit(A.cut, slot);
        for (int r = 0; r < CELL / 4; r++) {
            const int y = j * CELL + ty + 4 * r;
            if (y >= A.h) break;
            const size_t i = (size_t)y * A.w + x;
            const uint32_t word = *reinterpret_cast<const uint32_t*>(img2 + (size_t)y * A.img_pitch + (size_t)x * 4);
            const float2 f = bwd[i];
            float p[3];
            if (!deflicker_sample(x, y, f.x, f.y, occ2[i], cut, A.h, A.w, R, p)) continue;
            float g[kDkField] = {1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f};
            if (A.pass > 0) deflicker_field_at(x, y, A.cell, A.cx, A.cy, F, g);
            if (deflicker_member(word, p, g, g + 3, A.bound)) deflicker_add(s, word, p);
        }
    }
#pragma unroll
    for (int k = 0; k < kDkSums; k++) {
#pragma unroll
        for (int d = 1; d < CELL; d <<= 1) s[k] += __shfl_xor(s[k], d, 64);
    }
    if ((tx & (CELL - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < kDkSums; k++) part[ty][tx / CELL][k] = s[k];
    }
    __syncthreads();
    const int t = ty * 64 + tx;
    if (t < NC * kDkSums) {
        const int c = t / kDkSums, k = t - c * kDkSums, ci = blockIdx.x * NC + c;
        if (ci < A.cx) {
            uint32_t* sums = reinterpret_cast<uint32_t*>(blk + deflicker_off_sums(px));
            sums[((size_t)j * A.cx + ci) * kDkSums + k] = (part[0][c][k] + part[1][c][k]) + (part[2][c][k] + part[3][c][k]);
        }
    }
}

__global__ __launch_bounds__(64) void k_deflicker_field(DeflickerArgs A)
{
    const unsigned slot = A.slot0 + blockIdx.z;
    const int cell = blockIdx.x * 64 + threadIdx.x, cells = A.cx * A.cy;
    if (cell >= cells) return;
    const size_t px = (size_t)A.h * A.w;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const DkSumsAt S{reinterpret_cast<const uint32_t*>(blk + deflicker_off_sums(px)), A.cx};
    float out[kDkField];
    const uint8_t own = deflicker_smooth(cell % A.cx, cell / A.cx, A.cx, A.cy, A.n_min, S, out);
    float* field = reinterpret_cast<float*>(blk + deflicker_off_field(px, (size_t)cells)) + (size_t)cell * kDkField;
#pragma unroll
    for (int k = 0; k < kDkField; k++) field[k] = out[k];
    reinterpret_cast<uint8_t*>(blk + deflicker_off_valid(px, (size_t)cells))[cell] = own;
}

__global__ __launch_bounds__(256) void k_deflicker_apply(DeflickerArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t px = (size_t)A.h * A.w, cells = (size_t)A.cx * A.cy;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const DkFieldAt F{reinterpret_cast<const float*>(blk + deflicker_off_field(px, cells)), A.cx};
    uint32_t* __restrict__ next = reinterpret_cast<uint32_t*>(blk + deflicker_off_ref(px, dk_bit(A.cur, slot) ? 0 : 1));
    const uint32_t word = *reinterpret_cast<const uint32_t*>(pair_ptr(A.img2, A.img_stride, pair) + (size_t)y * A.img_pitch + (size_t)x * 4);
    float g[kDkField];
    deflicker_field_at(x, y, A.cell, A.cx, A.cy, F, g);
    next[(size_t)y * A.w + x] = deflicker_out(word, g, A.keep);
}

void launch_deflicker_accumulate(const DeflickerArgs& a, hipStream_t s)
{
    const dim3 grid((a.w + 63) / 64, a.cy, a.n), block(64, 4);
    if (a.cell == 16) hipLaunchKernelGGL(k_deflicker_accumulate<16>, grid, block, 0, s, a);
    else if (a.cell == 32) hipLaunchKernelGGL(k_deflicker_accumulate<32>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_deflicker_accumulate<64>, grid, block, 0, s, a);
}

void launch_deflicker_field(const DeflickerArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_deflicker_field, dim3((a.cx * a.cy + 63) / 64, 1, a.n), dim3(64), 0, s, a);
}

void launch_deflicker_apply(const DeflickerArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_deflicker_apply, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

}  // namespace eppm
