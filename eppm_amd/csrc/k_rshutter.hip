// k_rshutter.hip -- rolling-shutter correction of a frame along its flow.  Two launches per call, each over all
// pairs (blockIdx.z = pair): the velocity plane, then the gather.  The per-pixel arithmetic is rshutter.h's, shared with the host form.
// The velocity is evaluated once per pixel into a plane, so the gather's result does not depend on where velocities are evaluated: its
// fixed-point steps read four float2 taps each.  No LDS, no atomics; every lane works on its own pixel.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "rshutter.h"

namespace eppm {

namespace {

struct RgbaPx {           // a pixel word of an RGBA plane, pitch in bytes
    const uint8_t* __restrict__ p;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(p + (size_t)y * pitch + (size_t)x * 4); }
};
struct VelPx {            // a vector of the velocity plane, unpitched; callers pass in-frame coordinates only
    const float2* __restrict__ p;
    int w;
    __device__ RsVel operator()(int x, int y) const { const float2 v = p[(size_t)y * w + x]; return RsVel{v.x, v.y}; }
};

}  // namespace

// one lane per pixel: the float2 of flow in, the float2 of velocity out (both coalesced 8-byte accesses)
__global__ __launch_bounds__(256) void k_rs_velocity(const float2* __restrict__ flow_, size_t flow_stride, float2* __restrict__ vel_, size_t plane,
                                                     int h, int w, RsConst k)
{
    const int pair = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float2 f = pair_ptr(flow_, flow_stride, pair)[i];
    const RsVel v = rs_velocity(f.x, f.y, k);
    (vel_ + (size_t)pair * plane)[i] = make_float2(v.x, v.y);
}

// one lane per output pixel: packed RGB (rgb_ != NULL, pair z at z*h*w*3 bytes) or an RGBA word into rgba (pair 0)
__global__ __launch_bounds__(256) void k_rs_gather(const uint8_t* __restrict__ img_, size_t img_pitch, size_t img_stride,
                                                   const float2* __restrict__ vel_, size_t plane, uint8_t* __restrict__ rgb_,
                                                   uint8_t* __restrict__ rgba, size_t rgba_pitch, int h, int w, RsConst k, int iters)
{
    const int pair = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const RgbaPx img{pair_ptr(img_, img_stride, pair), img_pitch};
    const VelPx vel{vel_ + (size_t)pair * plane, w};
    const uint32_t out = rs_gather_pixel(x, y, k, iters, h, w, vel, img);
    if (rgb_) {
        uint8_t* __restrict__ o = rgb_ + (((size_t)pair * h + y) * w + x) * 3;
        o[0] = (uint8_t)out; o[1] = (uint8_t)(out >> 8); o[2] = (uint8_t)(out >> 16);
    } else {
        *reinterpret_cast<uint32_t*>(rgba + (size_t)y * rgba_pitch + (size_t)x * 4) = out;
    }
}

static dim3 rs_grid(const RShutterArgs& a, int npairs) { return dim3((a.w + 63) / 64, (a.h + 3) / 4, npairs); }

void launch_rs_velocity(const RShutterArgs& a, int npairs, hipStream_t s)
{
    const RsConst k = rs_const(a.readout, a.anchor, a.axis, a.frame, a.h, a.w);
    hipLaunchKernelGGL(k_rs_velocity, rs_grid(a, npairs), dim3(64, 4), 0, s, (const float2*)a.flow, a.flow_stride, (float2*)a.vel, a.plane, a.h, a.w, k);
}

void launch_rs_gather(const RShutterArgs& a, int npairs, hipStream_t s)
{
    const RsConst k = rs_const(a.readout, a.anchor, a.axis, a.frame, a.h, a.w);
    hipLaunchKernelGGL(k_rs_gather, rs_grid(a, npairs), dim3(64, 4), 0, s, a.img, a.img_pitch, a.img_stride, (const float2*)a.vel, a.plane, a.rgb,
                       a.rgba, a.rgba_pitch, a.h, a.w, k, a.iters);
}

}  // namespace eppm
