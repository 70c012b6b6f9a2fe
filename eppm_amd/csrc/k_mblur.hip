// k_mblur.hip -- the synthetic shutter: motion blur of a frame along its flow.  Two launches per call, each over
// all pairs (blockIdx.z = pair): pack, then gather.  The per-pixel arithmetic is mblur.h's, shared with the host form; the maximum over
// the keys is written here on its own (a wave's shuffles, a few bytes of LDS, one store per tile; no atomics).
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "mblur.h"

// rows of a tile that one workgroup of the gather covers: 8 (four workgroups per tile) or 32 (DESIGN.md section 18 has both timings)
#ifndef EPPM_MBLUR_GATHER_ROWS
#define EPPM_MBLUR_GATHER_ROWS 8
#endif

namespace eppm {

namespace {

constexpr int kRowsPerStep = 8;             // a workgroup is 32 x 8 lanes: a wave covers two 128-byte row segments of a tile
static_assert(EPPM_MBLUR_GATHER_ROWS == 8 || EPPM_MBLUR_GATHER_ROWS == 32, "a gather workgroup covers a quarter of a tile or a tile");

struct PackedPx {         // a word of the packed plane, unpitched; callers pass in-frame coordinates only
    const uint32_t* __restrict__ p;
    int w;
    __device__ uint32_t operator()(int x, int y) const { return p[(size_t)y * w + x]; }
};

}  // namespace

// One workgroup per tile.  Per pixel: the float2 of flow and the RGBA word in (both coalesced), the packed word {R, G, B, mq} out; per
// tile: the maximum key.  A lane outside the frame contributes key 0, which is below every pixel's key.
__global__ __launch_bounds__(256) void k_mblur_pack(const uint8_t* __restrict__ img_, size_t img_pitch, size_t img_stride,
                                                    const float2* __restrict__ flow_, size_t flow_stride, uint32_t* __restrict__ packed_,
                                                    size_t plane, uint64_t* __restrict__ tkeys_, size_t tplane, int h, int w, float shutter,
                                                    float R)
{
    __shared__ uint64_t wave_key[4];
    const int pair = blockIdx.z;
    const uint8_t* __restrict__ img = pair_ptr(img_, img_stride, pair);
    const float2* __restrict__ flow = pair_ptr(flow_, flow_stride, pair);
    uint32_t* __restrict__ packed = packed_ + (size_t)pair * plane;
    const int x = blockIdx.x * kMBlurTile + threadIdx.x;
    uint64_t best = 0;
    for (int r = 0; r < kMBlurTile / kRowsPerStep; r++) {
        const int y = blockIdx.y * kMBlurTile + r * kRowsPerStep + threadIdx.y;
        if (x < w && y < h) {
            const size_t i = (size_t)y * w + x;
            const float2 f = flow[i];
            const uint32_t c = *reinterpret_cast<const uint32_t*>(img + (size_t)y * img_pitch + (size_t)x * 4);
            const MBlurVec v = mblur_half_vector(f.x, f.y, shutter, R);
            packed[i] = mblur_pack(c, v.m);
            const uint64_t key = mblur_key(v.m, (uint32_t)i);
            best = key > best ? key : best;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)best, off, 64);
        best = o > best ? o : best;
    }
    const int lane = threadIdx.y * kMBlurTile + threadIdx.x;
    if ((lane & 63) == 0) wave_key[lane >> 6] = best;
    __syncthreads();
    if (lane == 0) {
        uint64_t k = wave_key[0];
        for (int i = 1; i < 4; i++) k = wave_key[i] > k ? wave_key[i] : k;
        tkeys_[(size_t)pair * tplane + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = k;
    }
}

// One workgroup per EPPM_MBLUR_GATHER_ROWS rows of a tile, one lane per pixel and step.  The dominant key, its pixel and its vector are
// the same for the whole workgroup (they depend on blockIdx alone), so every tap of a wave is two row segments of the packed plane shifted
// by one constant: coalesced dword loads.  Output: packed RGB (rgb_ != NULL, pair z at z*h*w*3 bytes) or an RGBA word into rgba (pair 0).
__global__ __launch_bounds__(256) void k_mblur_gather(const uint32_t* __restrict__ packed_, size_t plane, const uint64_t* __restrict__ tkeys_,
                                                      size_t tplane, int tiles_x, int tiles_y, const float2* __restrict__ flow_,
                                                      size_t flow_stride, uint8_t* __restrict__ rgb_, uint8_t* __restrict__ rgba,
                                                      size_t rgba_pitch, int h, int w, float shutter, float R, int taps)
{
    const int pair = blockIdx.z;
    const int tx = blockIdx.x, ty = (int)(blockIdx.y * EPPM_MBLUR_GATHER_ROWS) / kMBlurTile;
    const uint64_t* __restrict__ tkeys = tkeys_ + (size_t)pair * tplane;
    uint64_t K = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int ux = tx + dx, uy = ty + dy;
            const bool in = ux >= 0 && ux < tiles_x && uy >= 0 && uy < tiles_y;
            const uint64_t k = tkeys[in ? (size_t)uy * tiles_x + ux : (size_t)ty * tiles_x + tx];
            K = k > K ? k : K;
        }
    // K is the key of a pixel of the frame (the workgroup's own tile holds at least one), so j < h*w; the clamp only keeps the read inside
    // the plane whatever the key plane holds
    const uint32_t j = min(mblur_key_pixel(K), (uint32_t)(h * w - 1));
    const float2 fj = pair_ptr(flow_, flow_stride, pair)[j];
    const MBlurVec d = mblur_half_vector(fj.x, fj.y, shutter, R);
    const PackedPx pk{packed_ + (size_t)pair * plane, w};
    const int x = tx * kMBlurTile + threadIdx.x;
    for (int r = 0; r < EPPM_MBLUR_GATHER_ROWS / kRowsPerStep; r++) {
        const int y = blockIdx.y * EPPM_MBLUR_GATHER_ROWS + r * kRowsPerStep + threadIdx.y;
        if (x >= w || y >= h) continue;
        const uint32_t out = mblur_gather_pixel(x, y, d.hx, d.hy, d.m, taps, h, w, pk);
        if (rgb_) {
            uint8_t* __restrict__ o = rgb_ + (((size_t)pair * h + y) * w + x) * 3;
            o[0] = (uint8_t)out; o[1] = (uint8_t)(out >> 8); o[2] = (uint8_t)(out >> 16);
        } else {
            *reinterpret_cast<uint32_t*>(rgba + (size_t)y * rgba_pitch + (size_t)x * 4) = out;
        }
    }
}

void launch_mblur_pack(const MBlurArgs& a, int npairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_mblur_pack, dim3(a.tiles_x, a.tiles_y, npairs), dim3(kMBlurTile, kRowsPerStep), 0, s, a.img, a.img_pitch, a.img_stride,
                       (const float2*)a.flow, a.flow_stride, a.packed, a.plane, a.tkeys, a.tplane, a.h, a.w, a.shutter, a.max_radius);
}

void launch_mblur_gather(const MBlurArgs& a, int npairs, hipStream_t s)
{
    const int gy = (a.h + EPPM_MBLUR_GATHER_ROWS - 1) / EPPM_MBLUR_GATHER_ROWS;
    hipLaunchKernelGGL(k_mblur_gather, dim3(a.tiles_x, gy, npairs), dim3(kMBlurTile, kRowsPerStep), 0, s, (const uint32_t*)a.packed, a.plane,
                       (const uint64_t*)a.tkeys, a.tplane, a.tiles_x, a.tiles_y, (const float2*)a.flow, a.flow_stride, a.rgb, a.rgba,
                       a.rgba_pitch, a.h, a.w, a.shutter, a.max_radius, a.taps);
}

}  // namespace eppm
