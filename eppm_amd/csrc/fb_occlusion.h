// fb_occlusion.h -- the forward-backward consistency test of one pixel (Sundaram, Brox & Keutzer, ECCV 2010), shared by the kernel
// (k_occ.hip: k_fb_occlusion) and the host form (eppm_io.cpp: eppm_fb_occlusion_host) so that both evaluate the same operations in
// the same order.  Every operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused.
// Codes: 0 consistent, 1 inconsistent (or a tap of the other field unknown), 2 the vector leaves the frame, 3 the vector is unknown.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define EPPM_HD __host__ __device__
#else
#define EPPM_HD
#endif

namespace eppm {

EPPM_HD inline bool fb_known(float x, float y) { return fabsf(x) <= 1e9f && fabsf(y) <= 1e9f; }   // false for NaN too

// F: this direction's vector at (x, y); G: the other direction's field, interleaved (x, y) floats, h rows of w vectors
EPPM_HD inline uint8_t fb_occlusion_pixel(int x, int y, float fx, float fy, const float* G, int h, int w, float alpha, float beta)
{
    if (!fb_known(fx, fy)) return 3;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return 2;
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float* g00 = G + ((size_t)y0 * w + x0) * 2;
    const float* g01 = G + ((size_t)y0 * w + x1) * 2;
    const float* g10 = G + ((size_t)y1 * w + x0) * 2;
    const float* g11 = G + ((size_t)y1 * w + x1) * 2;
    if (!fb_known(g00[0], g00[1]) || !fb_known(g01[0], g01[1]) || !fb_known(g10[0], g10[1]) || !fb_known(g11[0], g11[1])) return 1;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float gx = by * (bx * g00[0] + ax * g01[0]) + ay * (bx * g10[0] + ax * g11[0]);
    const float gy = by * (bx * g00[1] + ax * g01[1]) + ay * (bx * g10[1] + ax * g11[1]);
    const float dx = fx + gx, dy = fy + gy;
    return (dx * dx + dy * dy) > alpha * ((fx * fx + fy * fy) + (gx * gx + gy * gy)) + beta ? 1 : 0;
}

}  // namespace eppm
