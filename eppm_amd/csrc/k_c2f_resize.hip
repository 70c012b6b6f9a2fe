// k_c2f_resize.hip -- coarse-to-fine step, the flow's way up one level (reference: basic/bao_basic_cuda.cuh:511-537 float2 bilinear
// resize, :135-142 scalar multiply).
#include "eppm_device.cuh"
#include "eppm_internal.h"

namespace eppm {

// .cuh:511-537 as written (m outer over x, n inner over y), then the x post_scale of .cuh:135-142
__global__ __launch_bounds__(256) void k_resize_flow(float* __restrict__ out_, int outH, int outW, const float* __restrict__ in_,
                                                     int h, int w, float ratio, float post_scale, size_t pstride)
{
    float* __restrict__ out = pair_ptr(out_, pstride, blockIdx.z);
    const float* __restrict__ in = pair_ptr(in_, pstride, blockIdx.z);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= outW || y >= outH) return;
    const float div_scale = 1.f / ratio;
    const float fx = (float)(x + 1) * div_scale - 1;
    const float fy = (float)(y + 1) * div_scale - 1;
    const int xx = (int)fx, yy = (int)fy;
    const float dx = fmaxf(fminf(fx - xx, 1), 0);
    const float dy = fmaxf(fminf(fy - yy, 1), 0);
    float rx = 0, ry = 0;
    for (int m = 0; m <= 1; m++)
        for (int n = 0; n <= 1; n++) {
            const int u = max(0, min(w - 1, xx + m));
            const int v = max(0, min(h - 1, yy + n));
            const float sc = fabsf(1 - m - dx) * fabsf(1 - n - dy);
            rx += in[(v * w + u) * 2] * sc;
            ry += in[(v * w + u) * 2 + 1] * sc;
        }
    out[(y * outW + x) * 2] = rx * post_scale;
    out[(y * outW + x) * 2 + 1] = ry * post_scale;
}
void launch_resize_flow(float* out, int outH, int outW, const float* in, int h, int w, float ratio, float post_scale, hipStream_t s, Batch bt)
{
    dim3 block(64, 4), grid((outW + 63) / 64, (outH + 3) / 4, bt.n);
    hipLaunchKernelGGL(k_resize_flow, grid, block, 0, s, out, outH, outW, in, h, w, ratio, post_scale, bt.stride);
}

__global__ __launch_bounds__(256) void k_mul_scalar(float* __restrict__ f, float scale, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) f[i] = f[i] * scale;
}
void launch_mul_scalar(float* flow, float scale, int h, int w, hipStream_t s)
{
    const int n = h * w * 2;
    hipLaunchKernelGGL(k_mul_scalar, dim3((n + 255) / 256), dim3(256), 0, s, flow, scale, n);
}

}  // namespace eppm
