// plate.h -- the arithmetic of background plates, shared by the kernels (k_plate.hip) and the host forms
// (plate.cpp) so that both evaluate the same operations in the same order: the two displacement forms of a camera path, the blocked
// byte of a mask byte and its dilation, the sample and the robust running mean of a canvas pixel, and the render of a frame pixel from
// the canvas.  Every float32 operation is one rounding, left to right, and every float64 operation likewise; the build's
// -ffp-contract=off keeps them unfused.  Everything gathers: no result depends on the order in which pixels are visited.
#pragma once

#include "gmotion.h"

namespace eppm {

constexpr int kPlateMaxGrow = 8;
constexpr int kPlateMaxCount = 255;

// a slot's path record on the device (128 bytes): the camera path P (frame 0 -> image 1 of the current pair) in (A, t) form
// {a00, a01, a10, a11, tx, ty}, and the two displacement forms of the last step with their validity
struct PlateRec {
    double p[6];
    float fwd[6], inv[6];
    int32_t ok, pad[7];
};

EPPM_HD inline bool plate_params_ok(int mx, int my, int grow, float thresh, int n_max, int min_count)
{
    return mx >= 0 && my >= 0 && grow >= 0 && grow <= kPlateMaxGrow && thresh >= 0.0f && thresh <= 3.4028234663852886e38f && n_max >= 1 &&
           n_max <= kPlateMaxCount && min_count >= 1 && min_count <= kPlateMaxCount;
}

// the canvas of an h x w frame with margins (mx, my) is within the stabiliser's limits (the sums below cannot overflow: mx, my <= 8192)
EPPM_HD inline bool plate_size_ok(int h, int w, int mx, int my)
{
    return gm_size_ok(h, w) && mx >= 0 && my >= 0 && mx <= kGmMaxDim && my <= kGmMaxDim && gm_size_ok(h + 2 * my, w + 2 * mx);
}

EPPM_HD inline void plate_identity(double* p)
{
    for (int k = 0; k < 6; k++) p[k] = (k == 0 || k == 3) ? 1.0 : 0.0;
}

// fwd: the displacement form of P (anchor coordinates -> image 1); inv: that of P^-1 = (A^-1, -A^-1 t).  false (both forms zero) when
// !(|det A| > 1e-6), a NaN included: such a step accumulates nothing and its render passes the image through
EPPM_HD inline bool plate_forms(const double* p, float* fwd, float* inv)
{
    const double det = p[0] * p[3] - p[1] * p[2];
    if (!(fabs(det) > 1e-6)) {
        for (int k = 0; k < 6; k++) fwd[k] = inv[k] = 0.0f;
        return false;
    }
    fwd[0] = (float)p[4]; fwd[1] = (float)((p[0] - 1.0) / 2.0); fwd[2] = (float)(p[1] / 2.0);
    fwd[3] = (float)p[5]; fwd[4] = (float)(p[2] / 2.0); fwd[5] = (float)((p[3] - 1.0) / 2.0);
    const double i00 = p[3] / det, i01 = -p[1] / det, i10 = -p[2] / det, i11 = p[0] / det;
    const double itx = -(i00 * p[4] + i01 * p[5]), ity = -(i10 * p[4] + i11 * p[5]);
    inv[0] = (float)itx; inv[1] = (float)((i00 - 1.0) / 2.0); inv[2] = (float)(i01 / 2.0);
    inv[3] = (float)ity; inv[4] = (float)(i10 / 2.0); inv[5] = (float)((i11 - 1.0) / 2.0);
    return true;
}

// P advanced by a pair's model, gm_update's expressions for C; an invalid model leaves it unchanged
EPPM_HD inline void plate_advance(double* c, const double* p, bool valid)
{
    if (!valid) return;
    const double m00 = 1.0 + 2.0 * p[1], m01 = 2.0 * p[2], m10 = 2.0 * p[4], m11 = 1.0 + 2.0 * p[5];
    const double n00 = m00 * c[0] + m01 * c[2], n01 = m00 * c[1] + m01 * c[3];
    const double n10 = m10 * c[0] + m11 * c[2], n11 = m10 * c[1] + m11 * c[3];
    const double ntx = (m00 * c[4] + m01 * c[5]) + p[0], nty = (m10 * c[4] + m11 * c[5]) + p[3];
    c[0] = n00; c[1] = n01; c[2] = n10; c[3] = n11; c[4] = ntx; c[5] = nty;
}

// a mask byte blocks: 0 is free, 1 is blocked, every other byte is blocked unless accept_invalid
EPPM_HD inline uint8_t plate_blocked(uint8_t m, bool accept_invalid) { return m == 0 ? 0 : m == 1 ? 1 : accept_invalid ? 0 : 1; }

// The sample of canvas pixel (xc, yc): image 1 at the pixel's position under fwd; false (nothing to accumulate) when the position is
// outside the frame (a NaN too) or one of its four taps is blocked.  px(x, y): image 1's word, B(x, y): the blocked byte, both at an
// in-frame pixel; nothing else is read
template <class Px, class Bk>
EPPM_HD inline bool plate_sample(int xc, int yc, int mx, int my, const float* fwd, int h, int w, const Px& px, const Bk& B, float c[3])
{
    const int x = xc - mx, y = yc - my;
    const int X = gm_X(x, w), Y = gm_Y(y, h);
    const float qx = (float)x + ((fwd[0] + fwd[1] * (float)X) + fwd[2] * (float)Y);
    const float qy = (float)y + ((fwd[3] + fwd[4] * (float)X) + fwd[5] * (float)Y);
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return false;
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);          // interp_sample's taps
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    if (B(x0, y0) | B(x1, y0) | B(x0, y1) | B(x1, y1)) return false;
    interp_sample(qx, qy, h, w, px, c);
    return true;
}

// the state of a canvas pixel after the sample c: a value contradicted more often than confirmed empties and is replaced by the next sample
EPPM_HD inline TfState plate_update(const TfState& s, const float c[3], float thresh, int n_max)
{
    if (!(s.n >= 1.0f)) return TfState{c[0], c[1], c[2], 1.0f};
    const float d = (fabsf(c[0] - s.r) + fabsf(c[1] - s.g)) + fabsf(c[2] - s.b);
    if (d <= thresh) {
        const float n = fminf(s.n + 1.0f, (float)n_max);
        return TfState{s.r + (c[0] - s.r) / n, s.g + (c[1] - s.g) / n, s.b + (c[2] - s.b) / n, n};
    }
    return TfState{s.r, s.g, s.b, s.n - 1.0f};            // a NaN distance too
}

// The output word and the fill byte of frame pixel (x, y) of image 1.  word: the image's; b: its blocked byte; S(xc, yc): the state of an
// in-canvas pixel (ch x cw); nothing else is read, whatever inv holds.  fill 0: free, the image; 1: filled from the canvas; 2: blocked
// and not filled (no valid path, outside the canvas, or a tap seen fewer than min_count times), the image
template <class St>
EPPM_HD inline uint32_t plate_render_pixel(int x, int y, uint32_t word, uint8_t b, bool ok, const float* inv, int mx, int my, int h, int w, int ch,
                                           int cw, int min_count, const St& S, uint8_t* fill)
{
    const uint32_t pass = (word & 0xffffffu) | 255u << 24;
    *fill = 0;
    if (b == 0) return pass;
    *fill = 2;
    if (!ok) return pass;
    const int X = gm_X(x, w), Y = gm_Y(y, h);
    const float qx = ((float)x + ((inv[0] + inv[1] * (float)X) + inv[2] * (float)Y)) + (float)mx;
    const float qy = ((float)y + ((inv[3] + inv[4] * (float)X) + inv[5] * (float)Y)) + (float)my;
    if (!(qx >= 0.0f && qx <= (float)(cw - 1) && qy >= 0.0f && qy <= (float)(ch - 1))) return pass;
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < cw - 1 ? x0 + 1 : cw - 1, y1 = y0 + 1 < ch - 1 ? y0 + 1 : ch - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const TfState a00 = S(x0, y0), a01 = S(x1, y0), a10 = S(x0, y1), a11 = S(x1, y1);
    const float m = (float)min_count;
    if (!(a00.n >= m && a01.n >= m && a10.n >= m && a11.n >= m)) return pass;
    *fill = 1;
    return tfilter_word(TfState{by * (bx * a00.r + ax * a01.r) + ay * (bx * a10.r + ax * a11.r),
                                by * (bx * a00.g + ax * a01.g) + ay * (bx * a10.g + ax * a11.g),
                                by * (bx * a00.b + ax * a01.b) + ay * (bx * a10.b + ax * a11.b), 0.0f});
}

// the coverage byte of a state: min(n, 255), 0 for !(n >= 1)
EPPM_HD inline uint8_t plate_coverage(float n) { return !(n >= 1.0f) ? 0 : (uint8_t)(int)fminf(n, 255.0f); }

// ---- the host forms: the same as sequential loops ----
inline void plate_block_host(const uint8_t* mask, int h, int w, int grow, bool accept_invalid, uint8_t* blocked)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            uint8_t b = 0;
            for (int yy = (y - grow > 0 ? y - grow : 0); yy <= (y + grow < h - 1 ? y + grow : h - 1); yy++)
                for (int xx = (x - grow > 0 ? x - grow : 0); xx <= (x + grow < w - 1 ? x + grow : w - 1); xx++)
                    b |= plate_blocked(mask[(size_t)yy * w + xx], accept_invalid);
            blocked[(size_t)y * w + x] = b;
        }
}

inline void plate_accumulate_host(const float* fwd, const uint8_t* rgb, const uint8_t* blocked, int h, int w, int mx, int my, float thresh, int n_max,
                                  TfState* state)
{
    const int ch = h + 2 * my, cw = w + 2 * mx;
    auto P = [rgb, w](int x, int y) {
        const uint8_t* q = rgb + ((size_t)y * w + x) * 3;
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    };
    auto B = [blocked, w](int x, int y) { return blocked[(size_t)y * w + x]; };
    for (int yc = 0; yc < ch; yc++)
        for (int xc = 0; xc < cw; xc++) {
            float c[3];
            if (!plate_sample(xc, yc, mx, my, fwd, h, w, P, B, c)) continue;
            TfState& s = state[(size_t)yc * cw + xc];
            s = plate_update(s, c, thresh, n_max);
        }
}

inline void plate_render_host(const float* inv, bool ok, const uint8_t* rgb, const uint8_t* blocked, int h, int w, int mx, int my, int min_count,
                              const TfState* state, uint8_t* rgb_out, uint8_t* fill)
{
    const int ch = h + 2 * my, cw = w + 2 * mx;
    auto S = [state, cw](int x, int y) { return state[(size_t)y * cw + x]; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint8_t* q = rgb + i * 3;
            uint8_t f;
            const uint32_t o = plate_render_pixel(x, y, (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16, blocked[i], ok, inv, mx, my, h, w, ch,
                                                  cw, min_count, S, &f);
            rgb_out[i * 3] = (uint8_t)o; rgb_out[i * 3 + 1] = (uint8_t)(o >> 8); rgb_out[i * 3 + 2] = (uint8_t)(o >> 16);
            if (fill) fill[i] = f;
        }
}

}  // namespace eppm
