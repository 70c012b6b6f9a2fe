// mblur.h -- the per-pixel arithmetic of the synthetic shutter (a depth-free form of McGuire et al., "A Reconstruction
// Filter for Plausible Motion Blur", I3D 2012), shared by the kernels (k_mblur.hip) and the host form (eppm_io.cpp: eppm_motion_blur_host)
// so that both evaluate the same operations in the same order.  Every float operation is one float32 rounding, left to right; the build's
// -ffp-contract=off keeps them unfused and its divide and square root are correctly rounded.  Every weight is 0 or 1 and every sum an
// integer, so there is nothing for EPPM_TOL to change.  The maximum over the keys is NOT here: the kernels reduce it per tile, the host
// form scans.  Builds without HIP.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

constexpr int kMBlurTile = 32;              // side of a tile in pixels; max_radius < kMBlurTile keeps every reaching mover inside the 3x3 tiles around
constexpr int kMBlurMaxTaps = 32;
constexpr int kMBlurStaticQ = 4;            // a dominant length below half a pixel (in eighths) leaves the pixel untouched

// shutter in (0, 1], max_radius in [1, 31], taps in [1, 32] (false for NaN)
EPPM_HD inline bool mblur_params_ok(float shutter, float max_radius, int taps)
{
    return shutter > 0.0f && shutter <= 1.0f && max_radius >= 1.0f && max_radius <= (float)(kMBlurTile - 1) && taps >= 1 && taps <= kMBlurMaxTaps;
}

struct MBlurVec { float hx, hy, m; };       // half of the path a pixel travels while the shutter is open, and its length

// the half-vector of the flow vector (fx, fy): zero when it is unknown, clamped to length R
EPPM_HD inline MBlurVec mblur_half_vector(float fx, float fy, float shutter, float R)
{
    MBlurVec r{0.0f, 0.0f, 0.0f};
    if (!fb_known(fx, fy)) return r;
    const float k = 0.5f * shutter;
    r.hx = k * fx;
    r.hy = k * fy;
    r.m = sqrtf(r.hx * r.hx + r.hy * r.hy);
    if (r.m > R) {
        const float q = R / r.m;
        r.hx = q * r.hx;
        r.hy = q * r.hy;
        r.m = R;
    }
    return r;
}

EPPM_HD inline int mblur_quant(float m) { return (int)floorf(m * 8.0f + 0.5f); }       // a length in eighths of a pixel, <= 248

EPPM_HD inline uint32_t mblur_float_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// the word {R, G, B, mq} of a pixel: everything a tap needs of it
EPPM_HD inline uint32_t mblur_pack(uint32_t rgbx, float m) { return (rgbx & 0x00ffffffu) | ((uint32_t)mblur_quant(m) << 24); }

// the longer vector wins, equal lengths resolve to the lower pixel index (i = y*w + x < 2^26); greater than 0, the key of "no pixel"
EPPM_HD inline uint64_t mblur_key(float m, uint32_t i) { return ((uint64_t)mblur_float_bits(m) << 32) | (uint32_t)(0xffffffffu - i); }
EPPM_HD inline uint32_t mblur_key_pixel(uint64_t key) { return 0xffffffffu - (uint32_t)key; }

// the gather at (x, y) along its neighbourhood's dominant half-vector (dx, dy) of length md with n taps to each side: the output word
// {R, G, B, 255}.  pk(x, y): the packed word.  The loop has the same trip count and no branch for every pixel of a tile; a tap outside the
// frame reads the clamped pixel and discards it.
template <class Pk>
EPPM_HD inline uint32_t mblur_gather_pixel(int x, int y, float dx, float dy, float md, int n, int h, int w, const Pk& pk)
{
    const uint32_t own = pk(x, y);
    if (mblur_quant(md) < kMBlurStaticQ) return own | (255u << 24);
    const int mqx = (int)(own >> 24);
    int s0 = 0, s1 = 0, s2 = 0;
    for (int i = -n; i <= n; i++) {
        const float t = (float)i / (float)n;
        const int xi = (int)floorf(((float)x + t * dx) + 0.5f), yi = (int)floorf(((float)y + t * dy) + 0.5f);
        const int dq = (int)floorf((fabsf(t) * md) * 8.0f + 0.5f);
        const bool in = xi >= 0 && xi < w && yi >= 0 && yi < h;
        const int xc = xi < 0 ? 0 : xi > w - 1 ? w - 1 : xi, yc = yi < 0 ? 0 : yi > h - 1 ? h - 1 : yi;
        const uint32_t tap = pk(xc, yc);
        const int mqt = (int)(tap >> 24);
        const bool take = i == 0 || (in && dq <= (mqt > mqx ? mqt : mqx));
        const uint32_t c = take ? tap : own;
        s0 += (int)(c & 255u);
        s1 += (int)((c >> 8) & 255u);
        s2 += (int)((c >> 16) & 255u);
    }
    const int T = 2 * n + 1;
    return (uint32_t)((2 * s0 + T) / (2 * T)) | ((uint32_t)((2 * s1 + T) / (2 * T)) << 8) | ((uint32_t)((2 * s2 + T) / (2 * T)) << 16) | (255u << 24);
}

}  // namespace eppm
