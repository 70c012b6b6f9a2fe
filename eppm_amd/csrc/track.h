// track.h -- the per-point arithmetic of dense point trajectories (Sundaram, Brox & Keutzer, ECCV 2010), shared by
// the kernels (k_track.hip) and the host form (tracker.cpp: eppm_track_step_host) so that both evaluate the same operations in the same
// order.  Every float operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused.  The ordering of
// the lists (the compaction) is NOT here: the kernels scan block counts, the host form keeps running counters.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

// end reasons (0: the track moves on)
enum { kTrackAlive = 0, kTrackUnknown = 1, kTrackLeaves = 2, kTrackInconsistent = 3, kTrackBoundary = 4 };

// one track of a list: 16 bytes, one vector load / store
struct TrackRec {
    int32_t id, start;
    float x, y;
};

// the parameters the kernels and the host form read (eppm_track_params after defaults and checks)
struct TrackParams {
    int spacing;
    long long min_eig;
    float fb_alpha, fb_beta, mb_alpha, mb_beta;
};

// the seed of cell `cell` (row-major over ncx columns of spacing x spacing pixels)
EPPM_HD inline void track_seed_xy(int cell, int ncx, int s, int h, int w, int* x, int* y)
{
    const int i = cell % ncx, j = cell / ncx;
    const int sx = i * s + s / 2, sy = j * s + s / 2;
    *x = sx < w - 1 ? sx : w - 1;
    *y = sy < h - 1 ? sy : h - 1;
}

// the cell of a position inside the frame
EPPM_HD inline int track_cell(float x, float y, int ncx, int s) { return ((int)floorf(y) / s) * ncx + (int)floorf(x) / s; }

// the texture test at pixel (x, y), exact integers: the 5x5 structure tensor of g = R + G + B (central differences over clamped taps) has
// lambda_min >= min_eig.  g(x, y): the grey level of an in-frame pixel
template <class Grey>
EPPM_HD inline bool track_textured(int x, int y, int h, int w, long long min_eig, const Grey& g)
{
    long long a = 0, b = 0, c = 0;
    for (int dy = -2; dy <= 2; dy++) {
        int ty = y + dy;
        ty = ty < 0 ? 0 : ty > h - 1 ? h - 1 : ty;
        const int yu = ty > 0 ? ty - 1 : 0, yd = ty < h - 1 ? ty + 1 : h - 1;
        for (int dx = -2; dx <= 2; dx++) {
            int tx = x + dx;
            tx = tx < 0 ? 0 : tx > w - 1 ? w - 1 : tx;
            const int xl = tx > 0 ? tx - 1 : 0, xr = tx < w - 1 ? tx + 1 : w - 1;
            const long long gx = (long long)g(xr, ty) - g(xl, ty), gy = (long long)g(tx, yd) - g(tx, yu);
            a += gx * gx;
            b += gx * gy;
            c += gy * gy;
        }
    }
    const long long S = a + c - 2 * min_eig, d = a - c;
    return S >= 0 && S * S >= d * d + 4 * b * b;
}

// the bilinear sample of a vector field at (qx, qy) inside the frame, taps and weights of fb_occlusion_pixel; false when a tap is unknown.
// f(x, y, &fx, &fy): the vector at an in-frame pixel
template <class Field>
EPPM_HD inline bool track_bilinear(float qx, float qy, int h, int w, const Field& f, float* ox, float* oy)
{
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    float u00, v00, u01, v01, u10, v10, u11, v11;
    f(x0, y0, &u00, &v00);
    f(x1, y0, &u01, &v01);
    f(x0, y1, &u10, &v10);
    f(x1, y1, &u11, &v11);
    if (!fb_known(u00, v00) || !fb_known(u01, v01) || !fb_known(u10, v10) || !fb_known(u11, v11)) return false;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    *ox = by * (bx * u00 + ax * u01) + ay * (bx * u10 + ax * u11);
    *oy = by * (bx * v00 + ax * v01) + ay * (bx * v10 + ax * v11);
    return true;
}

// one track at (x, y) of frame k, inside the frame: the end reason, or kTrackAlive and its position (*nx, *ny) in frame k+1.
// F: the forward field (frame k -> k+1), G: the backward field (k+1 -> k)
template <class FieldF, class FieldG>
EPPM_HD inline int track_advance(float x, float y, int h, int w, const TrackParams& p, const FieldF& F, const FieldG& G, float* nx, float* ny)
{
    float wx, wy;
    if (!track_bilinear(x, y, h, w, F, &wx, &wy)) return kTrackUnknown;
    const float qx = x + wx, qy = y + wy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return kTrackLeaves;
    float gx, gy;
    if (!track_bilinear(qx, qy, h, w, G, &gx, &gy)) return kTrackInconsistent;
    const float dx = wx + gx, dy = wy + gy;
    const float ww = wx * wx + wy * wy;
    if ((dx * dx + dy * dy) > p.fb_alpha * (ww + (gx * gx + gy * gy)) + p.fb_beta) return kTrackInconsistent;
    // motion boundary: central differences of the forward field at the pixel nearest (x, y)
    int cx = (int)floorf(x + 0.5f), cy = (int)floorf(y + 0.5f);
    cx = cx < 0 ? 0 : cx > w - 1 ? w - 1 : cx;
    cy = cy < 0 ? 0 : cy > h - 1 ? h - 1 : cy;
    const int xl = cx > 0 ? cx - 1 : 0, xr = cx < w - 1 ? cx + 1 : w - 1;
    const int yu = cy > 0 ? cy - 1 : 0, yd = cy < h - 1 ? cy + 1 : h - 1;
    float ul, vl, ur, vr, uu, vu, ud, vd;
    F(xl, cy, &ul, &vl);
    F(xr, cy, &ur, &vr);
    F(cx, yu, &uu, &vu);
    F(cx, yd, &ud, &vd);
    if (!fb_known(ul, vl) || !fb_known(ur, vr) || !fb_known(uu, vu) || !fb_known(ud, vd)) return kTrackBoundary;
    const float ux = 0.5f * (ur - ul), vx = 0.5f * (vr - vl);
    const float uy = 0.5f * (ud - uu), vy = 0.5f * (vd - vu);
    if ((ux * ux + uy * uy) + (vx * vx + vy * vy) > p.mb_alpha * ww + p.mb_beta) return kTrackBoundary;
    *nx = qx;
    *ny = qy;
    return kTrackAlive;
}

}  // namespace eppm
