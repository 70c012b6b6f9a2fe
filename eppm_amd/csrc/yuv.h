// yuv.h -- the arithmetic of Y'CbCr 4:2:0 conversion, shared by the kernels (k_yuv.hip) and the host forms (yuv.cpp).
// Integers only once the coefficients are made: every sum below fits 32 bits for every depth, matrix and range, >> is the arithmetic
// shift, and there is no EPPM_TOL branch -- kernels, host forms and a restatement agree byte for byte.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/eppm_yuv.h"
#include "fb_occlusion.h"       // EPPM_HD

namespace eppm {

// what both directions need of a format: made on the host by yuv_coeffs, passed to the kernels by value
struct YuvK {
    int cy, crv, cbu, cgu, cgv;         // to RGB, scale 2^20
    int fy[3], fu[3], fv[3], fs;        // from RGB, scale 2^fs (fs = 24 - depth): the rows of the forward matrix over {R, G, B}
    int yoff, coff, peak;
    int shift, mask;                    // sample = (word >> shift) & mask;  word = sample << shift
    int center;                         // siting == EPPM_YUV_CENTER
};

constexpr int kYuvS = 20;
constexpr int kYuvMaxDim = 65535;       // rows and columns of a frame: sizes and offsets of a plane stay far inside their types

inline bool yuv_format_ok(const eppm_yuv_format& f, const char** why)
{
    *why = nullptr;
    if (f.layout != EPPM_YUV_NV12 && f.layout != EPPM_YUV_I420) *why = "unknown layout";
    else if (f.depth != 8 && f.depth != 10 && f.depth != 12 && f.depth != 16) *why = "depth is not 8, 10, 12 or 16";
    else if (f.msb_aligned != 0 && f.msb_aligned != 1) *why = "msb_aligned is not 0 or 1";
    else if (f.depth == 8 && f.msb_aligned) *why = "msb_aligned with depth 8";
    else if (f.matrix < EPPM_YUV_BT601 || f.matrix > EPPM_YUV_BT2020) *why = "unknown matrix";
    else if (f.full_range != 0 && f.full_range != 1) *why = "full_range is not 0 or 1";
    else if (f.siting != EPPM_YUV_LEFT && f.siting != EPPM_YUV_CENTER) *why = "unknown siting";
    return *why == nullptr;
}

// rows and bytes per row of plane 0, 1 or 2 of an h x w frame (plane 2 of NV12: 0 and 0)
inline void yuv_plane_size(const eppm_yuv_format& f, int h, int w, int plane, int* rows, size_t* row_bytes)
{
    const size_t sz = f.depth > 8 ? 2 : 1;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    if (plane == 0) { *rows = h; *row_bytes = (size_t)w * sz; }
    else if (f.layout == EPPM_YUV_NV12) { *rows = plane == 1 ? ch : 0; *row_bytes = plane == 1 ? (size_t)cw * 2 * sz : 0; }
    else { *rows = ch; *row_bytes = (size_t)cw * sz; }
}

inline double yuv_rnd(double x) { return floor(x + 0.5); }

// The one place the coefficients are made: float64, each expression evaluated left to right as written (the build does not contract).
inline YuvK yuv_coeffs(const eppm_yuv_format& f)
{
    static const double kKr[3] = {0.299, 0.2126, 0.2627}, kKb[3] = {0.114, 0.0722, 0.0593};
    const double Kr = kKr[f.matrix], Kb = kKb[f.matrix], Kg = 1.0 - Kr - Kb;
    const int d = f.depth;
    YuvK k;
    k.peak = (1 << d) - 1;
    const double yr = f.full_range ? (double)k.peak : (double)(219 << (d - 8)), cr = f.full_range ? (double)k.peak : (double)(224 << (d - 8));
    k.yoff = f.full_range ? 0 : 16 << (d - 8);
    k.coff = 1 << (d - 1);
    const double s = (double)(1 << kYuvS);
    k.cy = (int)yuv_rnd(s * 255.0 / yr);
    k.crv = (int)yuv_rnd(s * 255.0 * 2.0 * (1.0 - Kr) / cr);
    k.cbu = (int)yuv_rnd(s * 255.0 * 2.0 * (1.0 - Kb) / cr);
    k.cgu = (int)yuv_rnd(s * 255.0 * 2.0 * (1.0 - Kb) * Kb / Kg / cr);
    k.cgv = (int)yuv_rnd(s * 255.0 * 2.0 * (1.0 - Kr) * Kr / Kg / cr);
    k.fs = 24 - d;
    const double t = (double)(1 << k.fs), ys = yr / 255.0, cs = cr / 255.0;
    const double K[3] = {Kr, Kg, Kb};
    for (int c = 0; c < 3; c++) {
        k.fy[c] = (int)yuv_rnd(t * (ys * K[c]));
        k.fu[c] = (int)yuv_rnd(t * (cs * ((c == 2 ? 1.0 : 0.0) - K[c]) / (2.0 * (1.0 - Kb))));
        k.fv[c] = (int)yuv_rnd(t * (cs * ((c == 0 ? 1.0 : 0.0) - K[c]) / (2.0 * (1.0 - Kr))));
    }
    k.shift = (d > 8 && f.msb_aligned) ? 16 - d : 0;
    k.mask = k.peak;
    k.center = f.siting == EPPM_YUV_CENTER;
    return k;
}

EPPM_HD inline int yuv_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the two taps of one axis at luma coordinate x of a chroma axis of n samples: indices clamped into the plane, weights in quarters
struct YuvTap { int i0, i1, w0, w1; };
// both sitings vertically, CENTER horizontally: even x: (i - 1, i) x (1, 3); odd x: (i, i + 1) x (3, 1)
EPPM_HD inline YuvTap yuv_tap_center(int x, int n)
{
    const int i = x >> 1;
    YuvTap t;
    if (x & 1) { t.i0 = i; t.i1 = i + 1 < n ? i + 1 : n - 1; t.w0 = 3; t.w1 = 1; }
    else { t.i0 = i > 0 ? i - 1 : 0; t.i1 = i; t.w0 = 1; t.w1 = 3; }
    return t;
}
// LEFT horizontally: even x: column j alone; odd x: (j, j + 1) x (2, 2)
EPPM_HD inline YuvTap yuv_tap_left(int x, int n)
{
    const int j = x >> 1;
    YuvTap t;
    t.i0 = j;
    if (x & 1) { t.i1 = j + 1 < n ? j + 1 : n - 1; t.w0 = 2; t.w1 = 2; }
    else { t.i1 = j; t.w0 = 4; t.w1 = 0; }
    return t;
}
EPPM_HD inline YuvTap yuv_tap_h(int x, int n, int center) { return center ? yuv_tap_center(x, n) : yuv_tap_left(x, n); }
// the upsampled chroma from the two vertically blended columns (each a sum of weight 4): weight 16 in all, one rounding
EPPM_HD inline int yuv_blend(const YuvTap& th, int v0, int v1) { return (th.w0 * v0 + th.w1 * v1 + 8) >> 4; }

EPPM_HD inline int yuv_sample(unsigned word, const YuvK& k) { return (int)((word >> k.shift) & (unsigned)k.mask); }
EPPM_HD inline unsigned yuv_word(int sample, const YuvK& k) { return (unsigned)sample << k.shift; }

// one pixel: samples Y, Cb, Cr (chroma upsampled already) -> R | G << 8 | B << 16, alpha 0
EPPM_HD inline uint32_t yuv_to_rgb_pixel(int Y, int Cb, int Cr, const YuvK& k)
{
    const int y = k.cy * (Y - k.yoff) + (1 << (kYuvS - 1)), u = Cb - k.coff, v = Cr - k.coff;
    const int r = yuv_clampi((y + k.crv * v) >> kYuvS, 0, 255);
    const int g = yuv_clampi((y - k.cgu * u - k.cgv * v) >> kYuvS, 0, 255);
    const int b = yuv_clampi((y + k.cbu * u) >> kYuvS, 0, 255);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

EPPM_HD inline int yuv_luma(int r, int g, int b, const YuvK& k)
{
    return yuv_clampi(((k.fy[0] * r + k.fy[1] * g + k.fy[2] * b + (1 << (k.fs - 1))) >> k.fs) + k.yoff, 0, k.peak);
}
// chroma of a block from the sums of R, G, B over its support (total weight 2^wshift): the matrix on the sums, one rounding
EPPM_HD inline int yuv_chroma(const int* m, int sr, int sg, int sb, int wshift, const YuvK& k)
{
    const int sh = k.fs + wshift;
    return yuv_clampi(((m[0] * sr + m[1] * sg + m[2] * sb + (1 << (sh - 1))) >> sh) + k.coff, 0, k.peak);
}

// The sums of block (j, i) of an h x w image; P(x, y): the word R | G << 8 | B << 16 of an in-frame pixel.  CENTER: the 2 x 2 pixels,
// weight 4 (wshift 2); LEFT: rows 2i, 2i + 1 by columns 2j - 1, 2j, 2j + 1 with weights (1, 2, 1), weight 8 (wshift 3); clamped.
template <class Px>
EPPM_HD inline void yuv_block_sums(int j, int i, int h, int w, int center, const Px& P, int* s)
{
    s[0] = s[1] = s[2] = 0;
    const int y0 = 2 * i, y1 = 2 * i + 1 < h ? 2 * i + 1 : h - 1;
    const int xm = 2 * j > 0 ? 2 * j - 1 : 0, x0 = 2 * j, x1 = 2 * j + 1 < w ? 2 * j + 1 : w - 1;
    for (int r = 0; r < 2; r++) {
        const int y = r ? y1 : y0;
        const uint32_t a = center ? 0u : P(xm, y), b = P(x0, y), c = P(x1, y);
        const int wa = center ? 0 : 1, wb = center ? 1 : 2;
        for (int ch = 0; ch < 3; ch++)
            s[ch] += wa * (int)((a >> (8 * ch)) & 255u) + wb * (int)((b >> (8 * ch)) & 255u) + (int)((c >> (8 * ch)) & 255u);
    }
}

}  // namespace eppm
