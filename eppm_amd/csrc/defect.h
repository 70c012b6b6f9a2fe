// defect.h -- the per-pixel arithmetic of film-defect removal, shared by the kernels (k_defect.hip) and the host
// form (defect.cpp: eppm_defect_step_host) so that both evaluate the same operations in the same order.  Every float operation is one
// float32 rounding, left to right; the build's -ffp-contract=off keeps them unfused.  A pixel of the middle frame of three is a defect
// if it differs from both motion-compensated neighbours while the neighbours agree with each other; it is then replaced by their mean.
#pragma once

#include <string.h>

#include "fb_occlusion.h"

namespace eppm {

// the code byte of a pixel
constexpr uint8_t kDfHit = 1, kDfSecond = 2, kDfUndecided = 4;

struct DfSample {
    float c[3];
    bool ok;
};

// img at (x, y) + (vx, vy), bilinear with the taps and weights of fb_occlusion_pixel.  I(x, y): the RGBA word of an in-frame pixel.  Every
// condition under which I must not be read is tested here: no input causes a read outside the frame.
template <class Img>
EPPM_HD inline DfSample defect_sample(int x, int y, float vx, float vy, int h, int w, const Img& I)
{
    DfSample s{{0.0f, 0.0f, 0.0f}, false};
    if (!fb_known(vx, vy)) return s;
    const float qx = (float)x + vx, qy = (float)y + vy;
    if (!(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1))) return s;
    const int x0 = (int)floorf(qx), y0 = (int)floorf(qy);
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = qx - (float)x0, ay = qy - (float)y0;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const uint32_t a00 = I(x0, y0), a01 = I(x1, y0), a10 = I(x0, y1), a11 = I(x1, y1);
    for (int k = 0; k < 3; k++) {
        const float c00 = (float)((a00 >> (8 * k)) & 255u), c01 = (float)((a01 >> (8 * k)) & 255u);
        const float c10 = (float)((a10 >> (8 * k)) & 255u), c11 = (float)((a11 >> (8 * k)) & 255u);
        s.c[k] = by * (bx * c00 + ax * c01) + ay * (bx * c10 + ax * c11);
    }
    s.ok = true;
    return s;
}

EPPM_HD inline float defect_dist(const float* a, const float* b) { return (fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + fabsf(a[2] - b[2]); }

struct DfChance {
    bool decided, hit;
    uint32_t word;              // the replacement: the mean of the two samples, alpha 255 (the pixel's own word while undecided)
};

// one chance at pixel (x, y) of the current frame (word cur): (bvx, bvy) into the previous frame P, (fvx, fvy) into the next frame N
template <class ImgP, class ImgN>
EPPM_HD inline DfChance defect_chance(int x, int y, uint32_t cur, float bvx, float bvy, float fvx, float fvy, int h, int w, float detect,
                                      float agree, const ImgP& P, const ImgN& N)
{
    DfChance r{false, false, cur | 0xff000000u};
    const DfSample p = defect_sample(x, y, bvx, bvy, h, w, P);
    const DfSample n = defect_sample(x, y, fvx, fvy, h, w, N);
    if (!p.ok || !n.ok) return r;
    if (!(defect_dist(p.c, n.c) <= agree)) return r;
    r.decided = true;
    const float c[3] = {(float)(cur & 255u), (float)((cur >> 8) & 255u), (float)((cur >> 16) & 255u)};
    r.hit = defect_dist(c, p.c) > detect && defect_dist(c, n.c) > detect;
    r.word = 255u << 24;
    for (int k = 0; k < 3; k++) r.word |= (uint32_t)(int)floorf(fminf(fmaxf((p.c[k] + n.c[k]) * 0.5f, 0.0f), 255.0f) + 0.5f) << (8 * k);
    return r;
}

// ---- the window median of the four vector components ----
// A known component (|v| <= 1e9) as a key whose unsigned order is the float order; -0 sorts below +0, which no result can see because a
// vector only enters (float)x + v.  No known component has the key 0xffffffff (that pattern is a NaN's).
EPPM_HD inline uint32_t defect_key(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
EPPM_HD inline float defect_unkey(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}

struct DfKeys {                 // of one pixel: forward x, y, backward x, y; a = 0xffffffff: one of the two vectors is unknown
    uint32_t a, b, c, d;
};
constexpr uint32_t kDfUnknown = 0xffffffffu;

EPPM_HD inline DfKeys defect_keys(float fx, float fy, float bx, float by)
{
    if (!fb_known(fx, fy) || !fb_known(bx, by)) return DfKeys{kDfUnknown, kDfUnknown, kDfUnknown, kDfUnknown};
    return DfKeys{defect_key(fx), defect_key(fy), defect_key(bx), defect_key(by)};
}

// The lower median (element (n - 1) / 2 of the ascending order, n = (2 radius + 1)^2) of each component over the window: K(dx, dy) are the
// keys of the pixel at the window's offset (dx, dy), coordinates clamped to the frame.  out: forward x, y, backward x, y.  False, and out
// untouched, if the window holds an unknown vector.  A selection by key bits from the top: 32 passes over the window that each count, for
// the four components at once, the keys below a candidate; no storage but eight registers, whatever the radius.
template <class Keys>
EPPM_HD inline bool defect_median(int radius, const Keys& K, float* out)
{
    const uint32_t rank = (uint32_t)((2 * radius + 1) * (2 * radius + 1) - 1) / 2;
    uint32_t pa = 0, pb = 0, pc = 0, pd = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t ta = pa | 1u << bit, tb = pb | 1u << bit, tc = pc | 1u << bit, td = pd | 1u << bit;
        uint32_t na = 0, nb = 0, nc = 0, nd = 0;
        bool unknown = false;
        for (int dy = -radius; dy <= radius; dy++)
            for (int dx = -radius; dx <= radius; dx++) {
                const DfKeys k = K(dx, dy);
                unknown |= k.a == kDfUnknown;
                na += k.a < ta; nb += k.b < tb; nc += k.c < tc; nd += k.d < td;
            }
        if (unknown) return false;
        if (na <= rank) pa = ta;
        if (nb <= rank) pb = tb;
        if (nc <= rank) pc = tc;
        if (nd <= rank) pd = td;
    }
    out[0] = defect_unkey(pa); out[1] = defect_unkey(pb); out[2] = defect_unkey(pc); out[3] = defect_unkey(pd);
    return true;
}

// the code byte and the replacement word of a pixel after its chances: c1 always, c2 only if c1 is undecided and radius > 0 (else NULL)
EPPM_HD inline uint8_t defect_code(const DfChance& c1, const DfChance* c2, uint32_t* word)
{
    if (c1.decided) {
        *word = c1.word;
        return c1.hit ? kDfHit : 0;
    }
    if (c2 && c2->decided) {
        *word = c2->word;
        return (uint8_t)(kDfSecond | (c2->hit ? kDfHit : 0));
    }
    *word = c1.word;
    return kDfUndecided;
}

// the mask byte of a pixel: 1 hit, 2 grown (decided, not hit, a hit within `grow` pixels inside the frame), 0 untouched.  C(x, y): the
// code byte of an in-frame pixel
template <class Codes>
EPPM_HD inline uint8_t defect_mask(int x, int y, int h, int w, int grow, const Codes& C)
{
    const uint8_t own = C(x, y);
    if (own & kDfHit) return 1;
    if (own & kDfUndecided) return 0;
    const int x0 = x - grow > 0 ? x - grow : 0, x1 = x + grow < w - 1 ? x + grow : w - 1;
    const int y0 = y - grow > 0 ? y - grow : 0, y1 = y + grow < h - 1 ? y + grow : h - 1;
    bool any = false;
    for (int yy = y0; yy <= y1; yy++)
        for (int xx = x0; xx <= x1; xx++) any |= (C(xx, yy) & kDfHit) != 0;
    return any ? 2 : 0;
}

}  // namespace eppm
