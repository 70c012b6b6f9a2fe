// gmotion.h -- the arithmetic of global camera-motion estimation and video stabilisation, shared by the kernels
// (k_gmotion.hip) and the host forms (stabilizer.cpp) so that both evaluate the same operations in the same order: the validity /
// quantise / inlier test of a pixel, the solve from the twelve sums, the path update and the warp pixel.  Every float32 operation is one
// rounding, left to right, and every float64 operation likewise; the build's -ffp-contract=off keeps them unfused.  The sums themselves
// are signed 64-bit integers: exact, so the order in which a kernel adds them does not matter.
#pragma once

#include "interp.h"
#include "tfilter.h"

namespace eppm {

constexpr int kGmSums = 12;            // n, SX, SY, SXX, SXY, SYY, Squ, SX.qu, SY.qu, Sqv, SX.qv, SY.qv
constexpr int kGmMaxDim = 8192;        // w, h <= 8192 and h*w <= 2^26: no sum exceeds 2^60
constexpr long long kGmMaxPixels = 1LL << 26;
constexpr int kGmMaxIters = 8;

// the fit of one pair as the kernels keep it (96 bytes); pf: p cast to float32, what the next pass and the mask test against
struct GmModel {
    double p[6];
    int64_t n_valid, n_inliers;
    int32_t valid, passes;
    float pf[6];
};

// a slot's stabiliser state (144 bytes): the camera path c and the smoothed path s in (A, t) form {a00, a01, a10, a11, tx, ty}, the
// updates since the last cut and how many of them had no valid model, and the warp of the last step in displacement form
struct GmState {
    double c[6], s[6];
    int64_t frames, invalid_steps;
    float wf[6];
    int32_t pad[2];
};

EPPM_HD inline bool gm_size_ok(int h, int w) { return h >= 1 && w >= 1 && h <= kGmMaxDim && w <= kGmMaxDim && (long long)h * w <= kGmMaxPixels; }

// doubled centred coordinates
EPPM_HD inline int gm_X(int x, int w) { return 2 * x - (w - 1); }
EPPM_HD inline int gm_Y(int y, int h) { return 2 * y - (h - 1); }

EPPM_HD inline bool gm_valid(float u, float v, uint8_t occ) { return occ == 0 && fb_known(u, v) && fabsf(u) <= 8192.0f && fabsf(v) <= 8192.0f; }

// 1/256 px steps; the product is exact, rintf rounds half to even.  Only called on a valid component: |q| <= 2^21
EPPM_HD inline int gm_quant(float u) { return (int)rintf(u * 256.0f); }

EPPM_HD inline bool gm_inlier(float u, float v, int X, int Y, const float* pf, float tau2)
{
    const float ru = u - ((pf[0] + pf[1] * (float)X) + pf[2] * (float)Y);
    const float rv = v - ((pf[3] + pf[4] * (float)X) + pf[5] * (float)Y);
    return (ru * ru + rv * rv) <= tau2;
}

// one valid pixel's terms added to the twelve sums
EPPM_HD inline void gm_accumulate(int64_t* s, int X, int Y, float u, float v)
{
    const int64_t x = X, y = Y, qu = gm_quant(u), qv = gm_quant(v);
    s[0] += 1; s[1] += x; s[2] += y; s[3] += x * x; s[4] += x * y; s[5] += y * y;
    s[6] += qu; s[7] += x * qu; s[8] += y * qu;
    s[9] += qv; s[10] += x * qv; s[11] += y * qv;
}

// the two 3x3 systems on the shared normal matrix by cofactors; false (p all 0) when the model is invalid
EPPM_HD inline bool gm_solve(const int64_t* s, double* p)
{
    const double n = (double)s[0], sx = (double)s[1], sy = (double)s[2], sxx = (double)s[3], sxy = (double)s[4], syy = (double)s[5];
    const double c00 = sxx * syy - sxy * sxy;
    const double c01 = sxy * sy - sx * syy;
    const double c02 = sx * sxy - sxx * sy;
    const double c11 = n * syy - sy * sy;
    const double c12 = sx * sy - n * sxy;
    const double c22 = n * sxx - sx * sx;
    const double det = (n * c00 + sx * c01) + sy * c02;
    if (!(s[0] >= 3 && det > 1e-6 * ((n * sxx) * syy))) {
        for (int k = 0; k < 6; k++) p[k] = 0.0;
        return false;
    }
    for (int k = 0; k < 2; k++) {
        const double b0 = (double)s[6 + 3 * k] / 256.0, b1 = (double)s[7 + 3 * k] / 256.0, b2 = (double)s[8 + 3 * k] / 256.0;
        p[3 * k] = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
        p[3 * k + 1] = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
        p[3 * k + 2] = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
    }
    return true;
}

// what a solve leaves of pass `pass` (0-based) in m
EPPM_HD inline void gm_model_from_sums(GmModel* m, const int64_t* s, int pass)
{
    m->valid = gm_solve(s, m->p) ? 1 : 0;
    if (pass == 0) m->n_valid = s[0];
    m->n_inliers = s[0];
    m->passes = pass + 1;
    for (int k = 0; k < 6; k++) m->pf[k] = (float)m->p[k];
}

// the mask byte of a pixel against the final model: 0 valid inlier, 1 valid outlier (every valid pixel of an invalid model), 2 not valid
EPPM_HD inline uint8_t gm_mask(float u, float v, uint8_t occ, int X, int Y, const GmModel& m, float tau2)
{
    if (!gm_valid(u, v, occ)) return 2;
    return m.valid && gm_inlier(u, v, X, Y, m.pf, tau2) ? 0 : 1;
}

EPPM_HD inline void gm_identity(GmState* st)
{
    for (int k = 0; k < 6; k++) st->c[k] = st->s[k] = (k == 0 || k == 3) ? 1.0 : 0.0;
    st->frames = 0;
    st->invalid_steps = 0;
}

// One update of a slot's state with the pair model (p, valid); fresh: the slot is empty, its state is the identity whatever st holds; cut:
// image 2 starts another clip.  Leaves the warp in st->wf.  The smoothing is written as smooth * S + (1 - smooth) * C, which is
// S + (1 - smooth) * (C - S) with both ends exact: smooth 1 keeps S and smooth 0 makes it C bit for bit.  Between the ends an entry that
// S and C share (the 1 of a static camera) stays exact only while 1 - smooth is exact in float64, which holds for smooth >= 0.5; below
// that a * x + b * x may differ from x by an ulp per step.  The warp C o S^-1 is evaluated as I + (C - S) o S^-1, so S == C gives the
// identity exactly.
EPPM_HD inline void gm_update(GmState* st, const double* p, bool valid, float smooth, bool fresh, bool cut)
{
    if (fresh || cut) gm_identity(st);
    for (int k = 0; k < 6; k++) st->wf[k] = 0.0f;
    if (cut) return;
    double* c = st->c;
    double* s = st->s;
    if (valid) {
        const double m00 = 1.0 + 2.0 * p[1], m01 = 2.0 * p[2], m10 = 2.0 * p[4], m11 = 1.0 + 2.0 * p[5];
        const double n00 = m00 * c[0] + m01 * c[2], n01 = m00 * c[1] + m01 * c[3];
        const double n10 = m10 * c[0] + m11 * c[2], n11 = m10 * c[1] + m11 * c[3];
        const double ntx = (m00 * c[4] + m01 * c[5]) + p[0], nty = (m10 * c[4] + m11 * c[5]) + p[3];
        c[0] = n00; c[1] = n01; c[2] = n10; c[3] = n11; c[4] = ntx; c[5] = nty;
    } else
        st->invalid_steps += 1;
    st->frames += 1;
    const double a = (double)smooth, b = 1.0 - a;
    for (int k = 0; k < 6; k++) s[k] = a * s[k] + b * c[k];
    const double det = s[0] * s[3] - s[1] * s[2];
    if (!(fabs(det) > 1e-6)) {          // a NaN too: the slot behaves as cut
        gm_identity(st);
        return;
    }
    const double i00 = s[3] / det, i01 = -s[1] / det, i10 = -s[2] / det, i11 = s[0] / det;
    const double d00 = c[0] - s[0], d01 = c[1] - s[1], d10 = c[2] - s[2], d11 = c[3] - s[3];
    const double e00 = d00 * i00 + d01 * i10, e01 = d00 * i01 + d01 * i11;
    const double e10 = d10 * i00 + d11 * i10, e11 = d10 * i01 + d11 * i11;
    const double wx = (c[4] - s[4]) - (e00 * s[4] + e01 * s[5]);
    const double wy = (c[5] - s[5]) - (e10 * s[4] + e11 * s[5]);
    st->wf[0] = (float)wx; st->wf[1] = (float)(e00 / 2.0); st->wf[2] = (float)(e01 / 2.0);
    st->wf[3] = (float)wy; st->wf[4] = (float)(e10 / 2.0); st->wf[5] = (float)(e11 / 2.0);
}

// the output word at pixel (x, y): image 2 sampled at the warped position, {0, 0, 0, 255} outside the frame (NaN too).  px(x, y): image
// 2's word at an in-frame pixel; nothing else is read
template <class Px>
EPPM_HD inline uint32_t gm_warp_pixel(int x, int y, const float* wf, int h, int w, const Px& px)
{
    const int X = gm_X(x, w), Y = gm_Y(y, h);
    const float qx = (float)x + ((wf[0] + wf[1] * (float)X) + wf[2] * (float)Y);
    const float qy = (float)y + ((wf[3] + wf[4] * (float)X) + wf[5] * (float)Y);
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return 255u << 24;
    float c[3];
    interp_sample(qx, qy, h, w, px, c);
    return tfilter_word(TfState{c[0], c[1], c[2], 0.0f});
}

}  // namespace eppm
