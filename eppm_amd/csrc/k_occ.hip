// k_occ.hip -- occlusion masks of a bidirectional call: the forward-backward consistency test (fb_occlusion.h) of every pixel of both
// directions.  Bandwidth-bound: one lane per pixel, its own vector a coalesced float2 read, the four taps of the other field gathered
// through L2 (the fields are smooth: neighbouring lanes read neighbouring taps), one byte written.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "fb_occlusion.h"

namespace eppm {

// blockIdx.z = 2 * pair + direction; direction 0: occ1 (F = forward, G = backward), 1: occ2 (F = backward, G = forward).
// The forward and backward fields and the masks each have their own pair stride (the masks share the backward field's).
__global__ __launch_bounds__(256) void k_fb_occlusion(uint8_t* __restrict__ occ1_, uint8_t* __restrict__ occ2_, const float2* __restrict__ fwd_,
                                                      size_t fstride, const float2* __restrict__ bwd_, size_t bstride, int h, int w, float alpha,
                                                      float beta)
{
    const unsigned pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const float2* __restrict__ fwd = pair_ptr(fwd_, fstride, pair);
    const float2* __restrict__ bwd = pair_ptr(bwd_, bstride, pair);
    uint8_t* __restrict__ occ = pair_ptr(dir ? occ2_ : occ1_, bstride, pair);
    const float2* __restrict__ F = dir ? bwd : fwd;
    const float2* __restrict__ G = dir ? fwd : bwd;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const float2 f = F[(size_t)y * w + x];
    occ[(size_t)y * w + x] = fb_occlusion_pixel(x, y, f.x, f.y, (const float*)G, h, w, alpha, beta);
}

void launch_fb_occlusion(uint8_t* occ1, uint8_t* occ2, const float* fwd, size_t fwd_stride, const float* bwd, size_t bwd_stride, int h, int w,
                         float alpha, float beta, int npairs, int ndir, hipStream_t s)
{
    dim3 block(64, 4), grid((w + 63) / 64, (h + 3) / 4, npairs * ndir);
    hipLaunchKernelGGL(k_fb_occlusion, grid, block, 0, s, occ1, occ2, (const float2*)fwd, fwd_stride, (const float2*)bwd, bwd_stride, h, w,
                       alpha, beta);
}

}  // namespace eppm
