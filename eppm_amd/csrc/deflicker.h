// deflicker.h -- the arithmetic of flicker removal, shared by the kernels (k_deflicker.hip) and the host form
// (deflicker.cpp: eppm_deflicker_step_host) so that both evaluate the same operations in the same order.  Every float32 operation is one
// float32 rounding and every float64 operation one float64 rounding, left to right; the build's -ffp-contract=off keeps them unfused, and
// its -fhip-fp32-correctly-rounded-divide-sqrt makes the device's division the host's.  The sums between the two are exact integers.
#pragma once

#include "tfilter.h"

namespace eppm {

constexpr int kDkSums = 13;             // per cell: n, then per colour sum v, sum qp, sum v*v, sum v*qp (qp = 16 p rounded)
constexpr int kDkField = 6;             // per cell: the gains of R, G, B, then the offsets
constexpr double kDkLambda = 64.0;      // the regression's pull towards gain 1, in units of variance per pixel

// The sample of pixel (x, y) of image 2 in the reference: validity and taps are tfilter_step_pixel's.  (fx, fy): the backward vector; o: the
// occ2 byte; R(x, y): the reference word at an in-frame pixel.  Every condition under which R must not be read is tested here, whatever
// the mask says: no input causes a read outside the frame.  false: the pixel has no sample (p is not written).
template <class Ref>
EPPM_HD inline bool deflicker_sample(int x, int y, float fx, float fy, uint8_t o, bool cut, int h, int w, const Ref& R, float p[3])
{
    if (cut || o != 0 || !fb_known(fx, fy)) return false;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return false;
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const uint32_t r00 = R(x0, y0), r01 = R(x1, y0), r10 = R(x0, y1), r11 = R(x1, y1);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a00 = (float)((r00 >> (8 * c)) & 255u), a01 = (float)((r01 >> (8 * c)) & 255u);
        const float a10 = (float)((r10 >> (8 * c)) & 255u), a11 = (float)((r11 >> (8 * c)) & 255u);
        p[c] = by * (bx * a00 + ax * a01) + ay * (bx * a10 + ax * a11);
    }
    return true;
}

// whether a sampled pixel belongs to a pass: its word under the gains a and offsets b lies within `bound` of the sample.  A NaN never does
EPPM_HD inline bool deflicker_member(uint32_t word, const float p[3], const float* a, const float* b, float bound)
{
    const float f0 = a[0] * (float)(word & 255u) + b[0];
    const float f1 = a[1] * (float)((word >> 8) & 255u) + b[1];
    const float f2 = a[2] * (float)((word >> 16) & 255u) + b[2];
    const float d = (fabsf(f0 - p[0]) + fabsf(f1 - p[1])) + fabsf(f2 - p[2]);
    return d <= bound;
}

// a member's terms added to thirteen sums: exact in 32 bits while a sum covers at most 4096 pixels (4096 * 255 * 4080 < 2^32)
EPPM_HD inline void deflicker_add(uint32_t* s, uint32_t word, const float p[3])
{
    s[0] += 1u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t v = (word >> (8 * c)) & 255u, q = (uint32_t)(int)rintf(p[c] * 16.0f);
        s[1 + 4 * c] += v;
        s[2 + 4 * c] += q;
        s[3 + 4 * c] += v * v;
        s[4 + 4 * c] += v * q;
    }
}

// the model of one cell from its sums: false if the cell has fewer than n_min members (a and b are not written; n_min >= 1)
EPPM_HD inline bool deflicker_model(const uint32_t* s, int n_min, double a[3], double b[3])
{
    if ((int)s[0] < n_min) return false;
    const double N = (double)s[0], lnn = (kDkLambda * N) * N;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double Sv = (double)s[1 + 4 * c], Sp = (double)s[2 + 4 * c] / 16.0, Svv = (double)s[3 + 4 * c], Svp = (double)s[4 + 4 * c] / 16.0;
        const double var = N * Svv - Sv * Sv, cov = N * Svp - Sv * Sp;
        const double g = fmin(fmax((cov + lnn) / (var + lnn), 0.5), 2.0);
        a[c] = g;
        b[c] = (Sp - g * Sv) / N;
    }
    return true;
}

// The smoothed field at cell (i, j) of a cx x cy grid: the (1, 2, 1) x (1, 2, 1) average over the valid cells of the 3 x 3 neighbourhood
// inside the grid, row by row; none: gain 1, offset 0.  S(i, j): the cell's thirteen sums.  Returns whether cell (i, j) itself is valid.
template <class Sums>
EPPM_HD inline uint8_t deflicker_smooth(int i, int j, int cx, int cy, int n_min, const Sums& S, float out[kDkField])
{
    double num[kDkField] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, den = 0.0;
    uint8_t own = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int ii = i + dx, jj = j + dy;
            if (ii < 0 || ii >= cx || jj < 0 || jj >= cy) continue;
            double a[3], b[3];
            if (!deflicker_model(S(ii, jj), n_min, a, b)) continue;
            const double wgt = (double)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
#pragma unroll
            for (int c = 0; c < 3; c++) {
                num[c] += wgt * a[c];
                num[3 + c] += wgt * b[c];
            }
            den += wgt;
            if (dx == 0 && dy == 0) own = 1;
        }
#pragma unroll
    for (int k = 0; k < kDkField; k++) out[k] = den > 0.0 ? (float)(num[k] / den) : (k < 3 ? 1.0f : 0.0f);
    return own;
}

// the bilinear taps of pixel x (or y) between the centres of n cells: g = (x + 0.5) / cell - 0.5 clamped to [0, n - 1], in the tap and
// weight form of fb_occlusion_pixel.  inv_cell = 1 / cell, a power of two: the product is the quotient, exactly
struct DkTap {
    int i0, i1;
    float a, b;
};
EPPM_HD inline DkTap deflicker_tap(int x, float inv_cell, int n)
{
    const float g = fminf(fmaxf(((float)x + 0.5f) * inv_cell - 0.5f, 0.0f), (float)(n - 1));
    DkTap t;
    t.i0 = (int)floorf(g);
    t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
    t.a = g - (float)t.i0;
    t.b = 1.0f - t.a;
    return t;
}

// the field at pixel (x, y): F(i, j): the kDkField floats of cell (i, j)
template <class Field>
EPPM_HD inline void deflicker_field_at(int x, int y, int cell, int cx, int cy, const Field& F, float out[kDkField])
{
    const float inv = 1.0f / (float)cell;
    const DkTap tx = deflicker_tap(x, inv, cx), ty = deflicker_tap(y, inv, cy);
    const float *g00 = F(tx.i0, ty.i0), *g01 = F(tx.i1, ty.i0), *g10 = F(tx.i0, ty.i1), *g11 = F(tx.i1, ty.i1);
#pragma unroll
    for (int k = 0; k < kDkField; k++) out[k] = ty.b * (tx.b * g00[k] + tx.a * g01[k]) + ty.a * (tx.b * g10[k] + tx.a * g11[k]);
}

// the output word of image 2's word under the field f at its pixel: keep blends the correction with the identity
EPPM_HD inline uint32_t deflicker_out(uint32_t word, const float f[kDkField], float keep)
{
    TfState s;
    s.r = (1.0f + keep * (f[0] - 1.0f)) * (float)(word & 255u) + keep * f[3];
    s.g = (1.0f + keep * (f[1] - 1.0f)) * (float)((word >> 8) & 255u) + keep * f[4];
    s.b = (1.0f + keep * (f[2] - 1.0f)) * (float)((word >> 16) & 255u) + keep * f[5];
    s.n = 0.0f;
    return tfilter_word(s);
}

}  // namespace eppm
