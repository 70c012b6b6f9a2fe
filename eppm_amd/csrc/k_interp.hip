// k_interp.hip -- frame interpolation from the forward flow and the occlusion masks of a bidirectional call: splat,
// two fill passes, blend.  Every launch covers all pairs x the times of one chunk (blockIdx.z = pair * nt + k).  The per-pixel arithmetic
// is interp.h's, shared with the host form; the minimum and the fill searches are written here on their own.
// Endpoint times (0, 1) skip the splat and the fill: the blend copies the input frame.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "interp.h"

namespace eppm {

namespace {

__device__ __forceinline__ float pick_t(int k, float t0, float t1, float t2, float t3) { return k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3; }

struct RgbaPx {           // a pixel word of an RGBA plane, pitch in bytes
    const uint8_t* __restrict__ p;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(p + (size_t)y * pitch + (size_t)x * 4); }
};
struct MaskPx {
    const uint8_t* __restrict__ p;
    int w;
    __device__ uint8_t operator()(int x, int y) const { return p[(size_t)y * w + x]; }
};

}  // namespace

// (a) one lane per source pixel; four 64-bit atomic minimums into the 2x2 block around its target (no return value: global_atomic_umin_x2)
__global__ __launch_bounds__(256) void k_interp_splat(const uint8_t* __restrict__ img1_, const uint8_t* __restrict__ img2_, size_t img_pitch,
                                                      size_t img_stride, const float2* __restrict__ flow_, size_t flow_stride,
                                                      const uint8_t* __restrict__ occ1_, size_t occ_stride, uint64_t* __restrict__ keys_,
                                                      size_t plane, int h, int w, int nt, float t0, float t1, float t2, float t3)
{
    const int z = blockIdx.z, pair = z / nt, k = z - pair * nt;
    const float t = pick_t(k, t0, t1, t2, t3);
    if (interp_endpoint(t)) return;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float2 f = pair_ptr(flow_, flow_stride, pair)[i];
    if (!fb_known(f.x, f.y)) return;
    const RgbaPx img1{pair_ptr(img1_, img_stride, pair), img_pitch}, img2{pair_ptr(img2_, img_stride, pair), img_pitch};
    const bool occluded = pair_ptr(occ1_, occ_stride, pair)[i] != 0;
    uint64_t key;
    int bx, by;
    if (!interp_splat_pixel(x, y, f.x, f.y, t, h, w, img1(x, y), occluded, img2, &key, &bx, &by)) return;
    unsigned long long* __restrict__ keys = reinterpret_cast<unsigned long long*>(keys_ + (size_t)z * plane);
    for (int dy = 0; dy < 2; dy++) {
        const int ty = by + dy;
        if (ty < 0 || ty >= h) continue;
        for (int dx = 0; dx < 2; dx++) {
            const int tx = bx + dx;
            if (tx < 0 || tx >= w) continue;
            atomicMin(keys + (size_t)ty * w + tx, (unsigned long long)key);
        }
    }
}

// (b) pass 1: a splatted pixel keeps its source; a hole walks outward one step at a time, left, right, up, down, and takes the first
// splatted pixel it meets (the smallest distance, ties in that order).  The walk of a pixel ends at its nearest splatted neighbour, so
// a frame with small holes costs a few reads per hole; a hole without any in its row and column walks to the frame's edges.
__global__ __launch_bounds__(256) void k_interp_fill1(const uint64_t* __restrict__ keys_, int32_t* __restrict__ fill1_, size_t plane, int h, int w,
                                                      int nt, float t0, float t1, float t2, float t3)
{
    const int z = blockIdx.z, k = z % nt;
    if (interp_endpoint(pick_t(k, t0, t1, t2, t3))) return;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint64_t* __restrict__ K = keys_ + (size_t)z * plane;
    const size_t i = (size_t)y * w + x;
    const uint64_t own = K[i];
    int32_t r = -1;
    if (own != kInterpHole) r = (int32_t)(uint32_t)own;
    else {
        const int far = max(max(x, w - 1 - x), max(y, h - 1 - y));
        for (int d = 1; d <= far; d++) {
            uint64_t q;
            if (x - d >= 0 && (q = K[i - d]) != kInterpHole) { r = (int32_t)(uint32_t)q; break; }
            if (x + d < w && (q = K[i + d]) != kInterpHole) { r = (int32_t)(uint32_t)q; break; }
            if (y - d >= 0 && (q = K[i - (size_t)d * w]) != kInterpHole) { r = (int32_t)(uint32_t)q; break; }
            if (y + d < h && (q = K[i + (size_t)d * w]) != kInterpHole) { r = (int32_t)(uint32_t)q; break; }
        }
    }
    (fill1_ + (size_t)z * plane)[i] = r;
}

// (b) pass 2: a pixel pass 1 left a hole takes the nearest filled pixel of pass 1's result in its row, ties to the left.  Only such pixels
// write (fill2 is read only where fill1 holds a hole).
__global__ __launch_bounds__(256) void k_interp_fill2(const int32_t* __restrict__ fill1_, int32_t* __restrict__ fill2_, size_t plane, int h, int w,
                                                      int nt, float t0, float t1, float t2, float t3)
{
    const int z = blockIdx.z, k = z % nt;
    if (interp_endpoint(pick_t(k, t0, t1, t2, t3))) return;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const int32_t* __restrict__ A = fill1_ + (size_t)z * plane;
    const size_t i = (size_t)y * w + x;
    if (A[i] >= 0) return;
    int32_t r = -1;
    const int far = max(x, w - 1 - x);
    for (int d = 1; d <= far; d++) {
        int32_t q;
        if (x - d >= 0 && (q = A[i - d]) >= 0) { r = q; break; }
        if (x + d < w && (q = A[i + d]) >= 0) { r = q; break; }
    }
    (fill2_ + (size_t)z * plane)[i] = r;
}

// (c) one lane per output pixel: packed RGB (3 bytes, host-pointer forms) or an RGBA word into the caller's plane of time k (pair 0)
__global__ __launch_bounds__(256) void k_interp_blend(const uint8_t* __restrict__ img1_, const uint8_t* __restrict__ img2_, size_t img_pitch,
                                                      size_t img_stride, const float2* __restrict__ flow_, size_t flow_stride,
                                                      const uint8_t* __restrict__ occ1_, const uint8_t* __restrict__ occ2_, size_t occ_stride,
                                                      const int32_t* __restrict__ fill1_, const int32_t* __restrict__ fill2_, size_t plane,
                                                      uint8_t* __restrict__ rgb_, uint8_t* __restrict__ r0, uint8_t* __restrict__ r1,
                                                      uint8_t* __restrict__ r2, uint8_t* __restrict__ r3, size_t rgba_pitch, int h, int w, int nt,
                                                      float t0, float t1, float t2, float t3)
{
    const int z = blockIdx.z, pair = z / nt, k = z - pair * nt;
    const float t = pick_t(k, t0, t1, t2, t3);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const RgbaPx img1{pair_ptr(img1_, img_stride, pair), img_pitch}, img2{pair_ptr(img2_, img_stride, pair), img_pitch};
    uint32_t out;
    if (t == 0.0f) out = img1(x, y) | (255u << 24);
    else if (t == 1.0f) out = img2(x, y) | (255u << 24);
    else {
        int32_t src = (fill1_ + (size_t)z * plane)[i];
        if (src < 0) src = (fill2_ + (size_t)z * plane)[i];
        float ux = 0.0f, uy = 0.0f;
        if (src >= 0) {
            const float2 f = pair_ptr(flow_, flow_stride, pair)[src];
            ux = f.x; uy = f.y;
        }
        const MaskPx o1{pair_ptr(occ1_, occ_stride, pair), w}, o2{pair_ptr(occ2_, occ_stride, pair), w};
        out = interp_blend_pixel(x, y, ux, uy, t, h, w, img1, img2, o1, o2);
    }
    if (rgb_) {
        uint8_t* __restrict__ o = rgb_ + ((size_t)z * h * w + i) * 3;
        o[0] = (uint8_t)out; o[1] = (uint8_t)(out >> 8); o[2] = (uint8_t)(out >> 16);
    } else {
        uint8_t* __restrict__ d = k == 0 ? r0 : k == 1 ? r1 : k == 2 ? r2 : r3;
        *reinterpret_cast<uint32_t*>(d + (size_t)y * rgba_pitch + (size_t)x * 4) = out;
    }
}

static dim3 interp_grid(const InterpArgs& a, int npairs) { return dim3((a.w + 63) / 64, (a.h + 3) / 4, npairs * a.nt); }

void launch_interp_splat(const InterpArgs& a, int npairs, hipStream_t s)
{
    (void)hipMemsetAsync(a.keys, 0xff, (size_t)npairs * a.nt * a.plane * 8, s);
    hipLaunchKernelGGL(k_interp_splat, interp_grid(a, npairs), dim3(64, 4), 0, s, a.img1, a.img2, a.img_pitch, a.img_stride,
                       (const float2*)a.flow, a.flow_stride, a.occ1, a.occ_stride, a.keys, a.plane, a.h, a.w, a.nt, a.t[0], a.t[1], a.t[2], a.t[3]);
}

void launch_interp_fill(const InterpArgs& a, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_interp_fill1, interp_grid(a, npairs), dim3(64, 4), 0, s, (const uint64_t*)a.keys, a.fill1, a.plane, a.h, a.w, a.nt,
                       a.t[0], a.t[1], a.t[2], a.t[3]);
    hipLaunchKernelGGL(k_interp_fill2, interp_grid(a, npairs), dim3(64, 4), 0, s, (const int32_t*)a.fill1, a.fill2, a.plane, a.h, a.w, a.nt,
                       a.t[0], a.t[1], a.t[2], a.t[3]);
}

void launch_interp_blend(const InterpArgs& a, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_interp_blend, interp_grid(a, npairs), dim3(64, 4), 0, s, a.img1, a.img2, a.img_pitch, a.img_stride, (const float2*)a.flow,
                       a.flow_stride, a.occ1, a.occ2, a.occ_stride, (const int32_t*)a.fill1, (const int32_t*)a.fill2, a.plane, a.rgb, a.rgba[0],
                       a.rgba[1], a.rgba[2], a.rgba[3], a.rgba_pitch, a.h, a.w, a.nt, a.t[0], a.t[1], a.t[2], a.t[3]);
}

}  // namespace eppm
