// cutdet.h -- the arithmetic of scene-cut detection from a pair's bidirectional flow, shared by the kernels
// (k_cutdet.hip) and the host form (cutdet.cpp: eppm_cutdet_host) so that both evaluate the same operations.  The float comparisons are
// fb_occlusion.h's and tfilter.h's, one float32 rounding each; everything summed is an integer, so the sums are exact in any order.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

constexpr int kCutMaxDim = 8192;        // w, h <= 8192 and h*w <= 2^26 (section 16's bounds): no sum exceeds 2^34
constexpr long long kCutMaxPixels = 1LL << 26;

// the ten sums of a pair: the class counts of occ1 and occ2, the tracked pixels of image 2 and their luma differences
enum { kCutC1 = 0, kCutC2 = 4, kCutTracked = 8, kCutSad = 9, kCutSums = 10 };

// a slot's record as the finish kernel writes it: eppm_cut_stats (include/eppm.h)
struct CutRecord {
    int64_t n, c1[4], c2[4], n_tracked, sad;
    int32_t cut, stepped;
};
constexpr int kCutRecordStride = 128;   // bytes between the records of two slots

EPPM_HD inline bool cut_size_ok(int h, int w) { return h >= 1 && w >= 1 && h <= kCutMaxDim && w <= kCutMaxDim && (long long)h * w <= kCutMaxPixels; }

// lost_permille in [0, 1000]; residual_max negative (the test is off) or in [0, 255]; false for NaN
EPPM_HD inline bool cut_params_ok(int lost_permille, float residual_max)
{
    return lost_permille >= 0 && lost_permille <= 1000 && (residual_max < 0.0f || (residual_max >= 0.0f && residual_max <= 255.0f));
}

// the residual threshold in sixteenths of a grey level; negative: the test is off
inline int64_t cut_r16(float residual_max) { return residual_max < 0.0f ? -1 : (int64_t)rintf(residual_max * 16.0f); }

EPPM_HD inline int cut_luma(uint32_t word)
{
    return (int)((77u * (word & 255u) + 150u * ((word >> 8) & 255u) + 29u * ((word >> 16) & 255u) + 128u) >> 8);
}

EPPM_HD inline int cut_class(uint8_t o) { return o < 3 ? o : 3; }

// One pixel (x, y) into the sums s (any integer type that holds them).  o1: the occ1 byte of image 1's pixel; cur, (fx, fy), o2: image 2's
// word, backward vector and occ2 byte; P1(x, y): image 1's word at an in-frame pixel.  Every condition under which P1 must not be read is
// tested here, whatever the mask says: no input causes a read outside the frame.
template <class T, class Px>
EPPM_HD inline void cut_pixel(T* s, int x, int y, uint8_t o1, uint32_t cur, float fx, float fy, uint8_t o2, int h, int w, const Px& P1)
{
    const int k1 = cut_class(o1), k2 = cut_class(o2);
    for (int k = 0; k < 4; k++) {           // constant indices: the kernel's sums stay in registers
        s[kCutC1 + k] += (T)(k1 == k);
        s[kCutC2 + k] += (T)(k2 == k);
    }
    if (o2 != 0 || !fb_known(fx, fy)) return;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return;       // false for NaN
    const int nx = (int)floorf(qx + 0.5f), ny = (int)floorf(qy + 0.5f);                            // tfilter.h's nearest tap: in frame
    const int d = cut_luma(cur) - cut_luma(P1(nx, ny));
    s[kCutTracked] += 1;
    s[kCutSad] += (T)(d < 0 ? -d : d);
}

// the record of a pair from its sums; all arithmetic is int64, equality is not a cut
EPPM_HD inline void cut_record(CutRecord* r, const int64_t* s, int64_t n, int lost_permille, int64_t r16)
{
    r->n = n;
    for (int k = 0; k < 4; k++) r->c1[k] = s[kCutC1 + k], r->c2[k] = s[kCutC2 + k];
    r->n_tracked = s[kCutTracked];
    r->sad = s[kCutSad];
    const int64_t a = n - r->c1[0], b = n - r->n_tracked;
    const int64_t lost = a < b ? a : b;
    r->cut = (lost * 1000 > (int64_t)lost_permille * n || (r16 >= 0 && r->n_tracked > 0 && r->sad * 16 > r16 * r->n_tracked)) ? 1 : 0;
    r->stepped = 1;
}

}  // namespace eppm
