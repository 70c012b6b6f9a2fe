// k_tfilter.hip -- the motion-compensated temporal filter (tfilter.h): one launch per step for every slot it covers
// (blockIdx.z), one lane per pixel of the new frame.  A wave is 64 consecutive pixels of one row, so the frame word (4 B), the backward
// vector (8 B), the mask byte, the new state (16 B: 1 KiB per wave and store) and the output word are coalesced, and the four float4 taps
// of neighbouring lanes are neighbours wherever the flow is smooth.  The step gathers, so it reads one of the slot's two states and writes
// the other; which is which, and whether the slot is empty or cut, are bits of the kernel arguments.  The arithmetic has no EPPM_TOL
// branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "tfilter.h"

namespace eppm {

namespace {

__device__ __forceinline__ bool tf_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct TfPrev {           // the previous state of a slot: its current plane, or image 1's seed while the slot is empty
    const float4* __restrict__ acc;
    const uint8_t* __restrict__ img1;
    size_t pitch;
    int w;
    bool empty;
    __device__ TfState operator()(int x, int y) const
    {
        if (empty) return tfilter_seed(*reinterpret_cast<const uint32_t*>(img1 + (size_t)y * pitch + (size_t)x * 4));
        const float4 v = acc[(size_t)y * w + x];
        return TfState{v.x, v.y, v.z, v.w};
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_tfilter_step(TFilterArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t i = (size_t)y * A.w + x;
    const bool cur = tf_bit(A.cur, slot);
    const float4* __restrict__ prev = reinterpret_cast<const float4*>(pair_ptr(cur ? A.st1 : A.st0, A.slot_stride, slot));
    float4* __restrict__ next = reinterpret_cast<float4*>(pair_ptr(cur ? A.st0 : A.st1, A.slot_stride, slot));
    const uint32_t word = *reinterpret_cast<const uint32_t*>(pair_ptr(A.img2, A.img_stride, pair) + (size_t)y * A.img_pitch + (size_t)x * 4);
    const float2 f = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair))[i];
    const uint8_t o = pair_ptr(A.occ2, A.occ_stride, pair)[i];
    const TfPrev P{prev, pair_ptr(A.img1, A.img_stride, pair), A.img_pitch, A.w, tf_bit(A.empty, slot)};
    const TfState s = tfilter_step_pixel(x, y, word, f.x, f.y, o, tf_bit(A.cut, slot), A.h, A.w, A.thresh, A.n_max, P);
    next[i] = make_float4(s.r, s.g, s.b, s.n);
    pair_ptr(A.out, A.slot_stride, slot)[i] = tfilter_word(s);
}

void launch_tfilter_step(const TFilterArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_tfilter_step, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

}  // namespace eppm
