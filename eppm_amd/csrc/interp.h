// interp.h -- the per-pixel arithmetic of frame interpolation (Baker et al., IJCV 2011, section 3.3), shared by
// the kernels (k_interp.hip) and the host form (eppm_io.cpp: eppm_interpolate_host) so that both evaluate the same operations in the
// same order.  Every operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused.  The splat's
// minimum and the two fill passes are NOT here: the kernels and the host form implement them separately.
// Pixels are passed around as one word {R, G, B, x} (R in the low byte); the fourth byte is ignored.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

constexpr uint64_t kInterpHole = ~(uint64_t)0;      // a splat target no key reached

// t == 0 and t == 1 are the input frames; anything else must lie strictly between them (false for NaN)
EPPM_HD inline bool interp_t_ok(float t) { return t >= 0.0f && t <= 1.0f; }
EPPM_HD inline bool interp_endpoint(float t) { return t == 0.0f || t == 1.0f; }

EPPM_HD inline uint32_t interp_float_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// bilinear sample of an image at (qx, qy) clamped into the frame; taps and weights as fb_occlusion_pixel.  px(x, y): the pixel's word
template <class Px>
EPPM_HD inline void interp_sample(float qx, float qy, int h, int w, const Px& px, float out[3])
{
    qx = fminf(fmaxf(qx, 0.0f), (float)(w - 1));
    qy = fminf(fmaxf(qy, 0.0f), (float)(h - 1));
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const uint32_t c00 = px(x0, y0), c01 = px(x1, y0), c10 = px(x0, y1), c11 = px(x1, y1);
    for (int c = 0; c < 3; c++) {
        const int s = 8 * c;
        const float v00 = (float)((c00 >> s) & 255u), v01 = (float)((c01 >> s) & 255u);
        const float v10 = (float)((c10 >> s) & 255u), v11 = (float)((c11 >> s) & 255u);
        out[c] = by * (bx * v00 + ax * v01) + ay * (bx * v10 + ax * v11);
    }
}

// (a) the splat of source pixel (x, y) with its known vector (fx, fy): the key (class, photo cost, source index) and the top-left corner
// (bx, by) of the 2x2 target block; false when no pixel of the block lies in the frame.  The caller min-reduces the key into each
// in-frame pixel of {bx, bx+1} x {by, by+1}.
template <class Px>
EPPM_HD inline bool interp_splat_pixel(int x, int y, float fx, float fy, float t, int h, int w, uint32_t p1, bool occluded, const Px& img2,
                                       uint64_t* key, int* bx, int* by)
{
    float c2[3];
    interp_sample((float)x + fx, (float)y + fy, h, w, img2, c2);
    const float d0 = fabsf((float)(p1 & 255u) - c2[0]);
    const float d1 = fabsf((float)((p1 >> 8) & 255u) - c2[1]);
    const float d2 = fabsf((float)((p1 >> 16) & 255u) - c2[2]);
    const float cost = (d0 + d1) + d2;
    const uint32_t hi = ((uint32_t)occluded << 31) | interp_float_bits(cost);
    *key = ((uint64_t)hi << 32) | (uint32_t)(y * w + x);
    const float px = (float)x + t * fx, py = (float)y + t * fy;
    const float fbx = floorf(px), fby = floorf(py);
    if (!(fbx >= -1.0f && fbx <= (float)(w - 1) && fby >= -1.0f && fby <= (float)(h - 1))) return false;
    *bx = (int)fbx;
    *by = (int)fby;
    return true;
}

// (c) the blend at pixel (x, y) with the filled vector (ux, uy): the output word {R, G, B, 255}.  img1 / img2 (px(x, y): the word),
// occ1 / occ2 (o(x, y): the mask byte)
template <class Px1, class Px2, class O1, class O2>
EPPM_HD inline uint32_t interp_blend_pixel(int x, int y, float ux, float uy, float t, int h, int w, const Px1& img1, const Px2& img2,
                                           const O1& occ1, const O2& occ2)
{
    const float s = 1.0f - t;
    float x0 = (float)x - t * ux, y0 = (float)y - t * uy;
    float x1 = (float)x + s * ux, y1 = (float)y + s * uy;
    x0 = fminf(fmaxf(x0, 0.0f), (float)(w - 1));
    y0 = fminf(fmaxf(y0, 0.0f), (float)(h - 1));
    x1 = fminf(fmaxf(x1, 0.0f), (float)(w - 1));
    y1 = fminf(fmaxf(y1, 0.0f), (float)(h - 1));
    float c0[3], c1[3];
    interp_sample(x0, y0, h, w, img1, c0);
    interp_sample(x1, y1, h, w, img2, c1);
    const bool a = occ1((int)floorf(x0 + 0.5f), (int)floorf(y0 + 0.5f)) != 0;
    const bool b = occ2((int)floorf(x1 + 0.5f), (int)floorf(y1 + 0.5f)) != 0;
    uint32_t out = 255u << 24;
    for (int c = 0; c < 3; c++) {
        const float v = (a && !b) ? c0[c] : (b && !a) ? c1[c] : s * c0[c] + t * c1[c];
        const int r = (int)floorf(v + 0.5f);
        out |= (uint32_t)(r < 255 ? r : 255) << (8 * c);
    }
    return out;
}

}  // namespace eppm
