// rshutter.h -- the per-pixel arithmetic of rolling-shutter correction, shared by the kernels (k_rshutter.hip) and
// the host form (eppm_io.cpp: eppm_rolling_shutter_host) so that both evaluate the same operations in the same order.  Every float
// operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused and its divide is correctly
// rounded.  Nothing here is a patch term, so there is nothing for EPPM_TOL to change.  Builds without HIP.
//
// The sample at coordinate c along the readout axis is taken at time tau(c) = g * (c - a0) frame intervals after the frame's own time.
// A point seen at p that moves with velocity vel(p) is shown by the global-shutter frame at q = p - tau(p) * vel(p); the corrected frame
// is the gather that solves p = q + tau(p) * vel(p) by a fixed number of fixed-point steps and samples the frame there.
#pragma once

#include "interp.h"
#include "tfilter.h"

namespace eppm {

constexpr int kRsMaxIters = 8;

// readout in [-1, 1], anchor in [0, 1], iters in [1, 8], axis 0 (rows) or 1 (columns); false for NaN
EPPM_HD inline bool rs_params_ok(float readout, float anchor, int iters, int axis)
{
    return readout >= -1.0f && readout <= 1.0f && anchor >= 0.0f && anchor <= 1.0f && iters >= 1 && iters <= kRsMaxIters && (axis == 0 || axis == 1);
}

// what a call computes once: tau's slope and origin, the flow's sign in time (frame 0: the flow points to the next frame, +1; frame 1: to
// the previous one, -1) and the axis
struct RsConst {
    float g, a0, sg;
    int axis;
};

EPPM_HD inline RsConst rs_const(float readout, float anchor, int axis, int frame, int h, int w)
{
    const int n = axis ? w : h;
    return RsConst{readout / (float)n, anchor * (float)(n - 1), frame ? -1.0f : 1.0f, axis};
}

EPPM_HD inline float rs_tau(const RsConst& k, float c) { return k.g * (c - k.a0); }

struct RsVel { float x, y; };       // pixels per frame interval

// The velocity of a pixel with the measured vector (fx, fy).  The vector spans sg + g*fa intervals, not one (a point that moves fa along
// the readout axis is read that much later or earlier), so it is divided by that; an unknown vector, and one whose span is less than half
// an interval in the flow's own direction, give no velocity.  |vel| <= 2e9: finite whatever the field holds.
EPPM_HD inline RsVel rs_velocity(float fx, float fy, const RsConst& k)
{
    const float fa = k.axis ? fx : fy;
    const float D = k.sg + k.g * fa;
    if (!(fb_known(fx, fy) && k.sg * D >= 0.5f)) return RsVel{0.0f, 0.0f};
    return RsVel{fx / D, fy / D};
}

// bilinear sample of the velocity plane at (qx, qy): interp_sample's clamp, taps and weights.  vel(x, y): the RsVel of an in-frame pixel
template <class V>
EPPM_HD inline RsVel rs_sample_velocity(float qx, float qy, int h, int w, const V& vel)
{
    qx = fminf(fmaxf(qx, 0.0f), (float)(w - 1));
    qy = fminf(fmaxf(qy, 0.0f), (float)(h - 1));
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const RsVel v00 = vel(x0, y0), v01 = vel(x1, y0), v10 = vel(x0, y1), v11 = vel(x1, y1);
    return RsVel{by * (bx * v00.x + ax * v01.x) + ay * (bx * v10.x + ax * v11.x), by * (bx * v00.y + ax * v01.y) + ay * (bx * v10.y + ax * v11.y)};
}

// the gather at output pixel (x, y): the output word {R, G, B, 255}.  vel(x, y): the velocity plane, px(x, y): the frame's word.  The loop
// has the same trip count for every pixel; every read is clamped into its plane (a position that overflowed to inf or NaN clamps too).
template <class V, class Px>
EPPM_HD inline uint32_t rs_gather_pixel(int x, int y, const RsConst& k, int iters, int h, int w, const V& vel, const Px& px)
{
    float qx = (float)x, qy = (float)y;
    for (int i = 0; i < iters; i++) {
        const RsVel s = rs_sample_velocity(qx, qy, h, w, vel);
        const float t = rs_tau(k, k.axis ? qx : qy);
        qx = (float)x + t * s.x;
        qy = (float)y + t * s.y;
    }
    float c[3];
    interp_sample(qx, qy, h, w, px, c);
    return tfilter_word(TfState{c[0], c[1], c[2], 1.0f});
}

}  // namespace eppm
