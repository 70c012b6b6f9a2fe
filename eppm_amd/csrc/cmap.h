// cmap.h -- the per-pixel arithmetic of the dense correspondence map, shared by the kernels (k_cmap.hip) and the
// host forms (cmap.cpp: eppm_cmap_step_host, eppm_cmap_render_host) so that both evaluate the same operations in the same order.  Every
// float operation is one float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused, and its
// -fhip-fp32-correctly-rounded-divide-sqrt makes the device's division the host's.  Builds without HIP.
#pragma once

#include "fb_occlusion.h"

namespace eppm {

constexpr float kCmapLost = 1e10f;     // both components of a lost pixel; anything with !fb_known reads as lost

// a position in the anchor frame.  8 bytes, one vector load / store
struct CmPt {
    float x, y;
};

// the taps and weights of a point inside the frame, as fb_occlusion_pixel derives them
struct CmTaps {
    int x0, y0, x1, y1;
    float ax, ay, bx, by;
};

EPPM_HD inline bool cmap_in_frame(float px, float py, int h, int w)      // false for NaN
{
    return px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1);
}

EPPM_HD inline CmTaps cmap_taps(float qx, float qy, int h, int w)
{
    CmTaps t;
    t.x0 = (int)floorf(qx); t.y0 = (int)floorf(qy);
    t.x1 = t.x0 + 1 < w - 1 ? t.x0 + 1 : w - 1; t.y1 = t.y0 + 1 < h - 1 ? t.y0 + 1 : h - 1;
    t.ax = qx - (float)t.x0; t.ay = qy - (float)t.y0;
    t.bx = 1.0f - t.ax; t.by = 1.0f - t.ay;
    return t;
}

EPPM_HD inline float cmap_bl(const CmTaps& t, float v00, float v01, float v10, float v11)
{
    return t.by * (t.bx * v00 + t.ax * v01) + t.ay * (t.bx * v10 + t.ax * v11);
}

EPPM_HD inline float cmap_chan(uint32_t word, int c) { return (float)((word >> (8 * c)) & 255u); }

// One step at pixel (x, y) of the new frame (image 2 of the pair).  cur: its word; (fx, fy): the backward vector (image 2 -> image 1);
// o: the occ2 byte; cut: the frame starts another clip; M(x, y): the previous map at an in-frame pixel; A(x, y): the anchor's word at an
// in-frame pixel.  Every condition under which M or A must not be read is tested here, whatever the mask says: no input causes a read
// outside the frame.
template <class Map, class Anc>
EPPM_HD inline CmPt cmap_step_pixel(int x, int y, uint32_t cur, float fx, float fy, uint8_t o, bool cut, int h, int w, float thresh, float tear,
                                    int use_occ, const Map& M, const Anc& A)
{
    const CmPt lost{kCmapLost, kCmapLost};
    if (cut) return CmPt{(float)x, (float)y};
    if ((use_occ && o != 0) || !fb_known(fx, fy)) return lost;
    const float qx = (float)x + fx, qy = (float)y + fy;
    if (!cmap_in_frame(qx, qy, h, w)) return lost;
    const CmTaps t = cmap_taps(qx, qy, h, w);
    const CmPt m00 = M(t.x0, t.y0), m01 = M(t.x1, t.y0), m10 = M(t.x0, t.y1), m11 = M(t.x1, t.y1);
    // the tap nearest to q (tfilter.h's): one of the four taps above
    const int nx = (int)floorf(qx + 0.5f), ny = (int)floorf(qy + 0.5f);
    const CmPt mn = ny == t.y0 ? (nx == t.x0 ? m00 : m01) : (nx == t.x0 ? m10 : m11);
    if (!fb_known(mn.x, mn.y)) return lost;
    const CmPt m[4] = {m00, m01, m10, m11};
    bool smooth = true;
    for (int k = 0; k < 4; k++)
        smooth = smooth && fb_known(m[k].x, m[k].y) && fabsf(m[k].x - mn.x) <= tear && fabsf(m[k].y - mn.y) <= tear;
    CmPt s;
    if (smooth) {
        s.x = cmap_bl(t, m00.x, m01.x, m10.x, m11.x);
        s.y = cmap_bl(t, m00.y, m01.y, m10.y, m11.y);
    } else {                                     // the nearest surface, translated
        s.x = mn.x + (qx - (float)nx);
        s.y = mn.y + (qy - (float)ny);
    }
    if (!cmap_in_frame(s.x, s.y, h, w)) return lost;
    const CmTaps u = cmap_taps(s.x, s.y, h, w);
    const uint32_t a00 = A(u.x0, u.y0), a01 = A(u.x1, u.y0), a10 = A(u.x0, u.y1), a11 = A(u.x1, u.y1);
    float p[3];
    for (int c = 0; c < 3; c++) p[c] = cmap_bl(u, cmap_chan(a00, c), cmap_chan(a01, c), cmap_chan(a10, c), cmap_chan(a11, c));
    const float d = (fabsf(cmap_chan(cur, 0) - p[0]) + fabsf(cmap_chan(cur, 1) - p[1])) + fabsf(cmap_chan(cur, 2) - p[2]);
    if (!(d <= thresh)) return lost;             // a NaN is lost too
    return s;
}

// The rendered word at a pixel: cur: the current frame's word; s: the pixel's map value; L(x, y): the layer's RGBA word (straight alpha)
// at an in-frame pixel.  R | G << 8 | B << 16 | 255 << 24.
template <class Lay>
EPPM_HD inline uint32_t cmap_render_pixel(uint32_t cur, CmPt s, int h, int w, const Lay& L)
{
    if (!fb_known(s.x, s.y) || !cmap_in_frame(s.x, s.y, h, w)) return (cur & 0xffffffu) | 255u << 24;
    const CmTaps t = cmap_taps(s.x, s.y, h, w);
    const uint32_t l[4] = {L(t.x0, t.y0), L(t.x1, t.y0), L(t.x0, t.y1), L(t.x1, t.y1)};
    float a[4];
    for (int k = 0; k < 4; k++) a[k] = cmap_chan(l[k], 3);
    const float pa = cmap_bl(t, a[0], a[1], a[2], a[3]);
    uint32_t out = 255u << 24;
    for (int c = 0; c < 3; c++) {
        const float pc = cmap_bl(t, cmap_chan(l[0], c) * a[0], cmap_chan(l[1], c) * a[1], cmap_chan(l[2], c) * a[2], cmap_chan(l[3], c) * a[3]);
        const float v = (pc + (255.0f - pa) * cmap_chan(cur, c)) / 255.0f;
        out |= (uint32_t)(int)floorf(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f) << (8 * c);
    }
    return out;
}

}  // namespace eppm
