// tfilter.h -- the per-pixel arithmetic of the motion-compensated temporal filter, shared by the kernel
// (k_tfilter.hip) and the host form (tfilter.cpp: eppm_tfilter_step_host) so that both evaluate the same operations in the same order.
// Every float operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused, and its
// -fhip-fp32-correctly-rounded-divide-sqrt makes the device's division the host's.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

// one pixel of a slot's state: the running mean of R, G, B along the pixel's trajectory and the number of frames in it.  16 bytes, one
// vector load / store
struct TfState {
    float r, g, b, n;
};

EPPM_HD inline TfState tfilter_seed(uint32_t word)
{
    return TfState{(float)(word & 255u), (float)((word >> 8) & 255u), (float)((word >> 16) & 255u), 1.0f};
}

// the output word of a state: R | G << 8 | B << 16 | 255 << 24, every component clamped and rounded (total: NaN -> 0, inf -> 255)
EPPM_HD inline uint32_t tfilter_word(const TfState& s)
{
    const float c[3] = {s.r, s.g, s.b};
    uint32_t out = 255u << 24;
    for (int k = 0; k < 3; k++) out |= (uint32_t)(int)floorf(fminf(fmaxf(c[k], 0.0f), 255.0f) + 0.5f) << (8 * k);
    return out;
}

// One step at pixel (x, y) of the new frame (image 2 of the pair).  cur: its word; (fx, fy): the backward vector (image 2 -> image 1);
// o: the occ2 byte; cut: the frame starts another clip; A(x, y): the previous state (image 1's) at an in-frame pixel.  Every condition
// under which A must not be read is tested here, whatever the mask says: no input causes a read outside the frame.
template <class Acc>
EPPM_HD inline TfState tfilter_step_pixel(int x, int y, uint32_t cur, float fx, float fy, uint8_t o, bool cut, int h, int w, float thresh,
                                          int n_max, const Acc& A)
{
    const TfState reset = tfilter_seed(cur);
    if (cut || o != 0 || !fb_known(fx, fy)) return reset;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return reset;
    // taps and weights of fb_occlusion_pixel
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const TfState a00 = A(x0, y0), a01 = A(x1, y0), a10 = A(x0, y1), a11 = A(x1, y1);
    const float p0 = by * (bx * a00.r + ax * a01.r) + ay * (bx * a10.r + ax * a11.r);
    const float p1 = by * (bx * a00.g + ax * a01.g) + ay * (bx * a10.g + ax * a11.g);
    const float p2 = by * (bx * a00.b + ax * a01.b) + ay * (bx * a10.b + ax * a11.b);
    // the count of the tap nearest to q (interp_blend_pixel's mask lookup): one of the four taps above
    const int nx = (int)floorf(qx + 0.5f), ny = (int)floorf(qy + 0.5f);
    const float n_prev = ny == y0 ? (nx == x0 ? a00.n : a01.n) : (nx == x0 ? a10.n : a11.n);
    const float d = (fabsf(reset.r - p0) + fabsf(reset.g - p1)) + fabsf(reset.b - p2);
    if (!(d <= thresh)) return reset;            // a NaN resets too
    const float n = fminf(n_prev + 1.0f, (float)n_max);
    return TfState{p0 + (reset.r - p0) / n, p1 + (reset.g - p1) / n, p2 + (reset.b - p2) / n, n};
}

}  // namespace eppm
