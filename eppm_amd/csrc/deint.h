// deint.h -- the arithmetic of motion-compensated deinterlacing, shared by the kernels (k_deint.hip) and the host
// forms (eppm_io.cpp: eppm_deint_step_host, eppm_deint_bob_host) so that both evaluate the same operations in the same order.  The
// candidate's sample is deflicker_sample's (the float conventions of sections 15 and 24.1); everything after its rounding is integer.
#pragma once

#include "deflicker.h"

namespace eppm {

// what is wrong with a parameter pair, or NULL (host code: the object's and the host form's one check)
inline const char* deint_params_bad(int thresh, int use_occ)
{
    if (thresh < 0 || thresh > 765) return "thresh outside [0, 765]";
    if (use_occ != 0 && use_occ != 1) return "use_occ is not 0 or 1";
    return nullptr;
}

// the rows above and below row y of a frame of h >= 2 rows; a row outside the frame is replaced by the other one
EPPM_HD inline int deint_row_up(int y) { return y > 0 ? y - 1 : y + 1; }
EPPM_HD inline int deint_row_dn(int y, int h) { return y + 1 < h ? y + 1 : y - 1; }

// the line average of two words, per colour (up + dn + 1) >> 1, in bits 0..23 (alpha 0)
EPPM_HD inline uint32_t deint_average(uint32_t up, uint32_t dn)
{
    uint32_t out = 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) out |= ((((up >> (8 * c)) & 255u) + ((dn >> (8 * c)) & 255u) + 1u) >> 1) << (8 * c);
    return out;
}

// One pixel (x, y) of a MISSING row of image 2 (a row y with (y & 1) != parity).  up, dn: image 2's words at the rows deint_row_up(y) and
// deint_row_dn(y, h), which are real rows; (fx, fy): the backward vector; o: the occ2 byte; R(x, y): the reference word at an in-frame
// pixel.  deflicker_sample tests every condition under which R must not be read, whatever the mask says.  The candidate q (the bilinear
// sample of the reference under tfilter_word's rounding) is accepted iff it is valid, the step is no cut and
// 2 * sum |q - s| <= 2 * thresh + sum |up - dn|, s being the line average.  *mask: 1 temporal, 2 spatial.  Alpha 255.
template <class Ref>
EPPM_HD inline uint32_t deint_missing_pixel(int x, int y, uint32_t up, uint32_t dn, float fx, float fy, uint8_t o, bool cut, int use_occ, int thresh,
                                            int h, int w, const Ref& R, uint8_t* mask)
{
    const uint32_t s = deint_average(up, dn);
    float m[3];
    if (deflicker_sample(x, y, fx, fy, use_occ ? o : (uint8_t)0, cut, h, w, R, m)) {
        const uint32_t q = tfilter_word(TfState{m[0], m[1], m[2], 0.0f});
        int d = 0, contrast = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int qc = (int)((q >> (8 * c)) & 255u), sc = (int)((s >> (8 * c)) & 255u);
            const int uc = (int)((up >> (8 * c)) & 255u), dc = (int)((dn >> (8 * c)) & 255u);
            d += qc > sc ? qc - sc : sc - qc;
            contrast += uc > dc ? uc - dc : dc - uc;
        }
        if (2 * d <= 2 * thresh + contrast) {
            *mask = 1;
            return q;
        }
    }
    *mask = 2;
    return s | 255u << 24;
}

// One pixel (x, y) of the full frame of a field picture of parity p: F(x, i): the word of field row i.  Row 2i + p is field row i, every
// other row the line average of its neighbours.  Alpha 0.
template <class Field>
EPPM_HD inline uint32_t deint_bob_pixel(int x, int y, int p, int h, const Field& F)
{
    if ((y & 1) == p) return F(x, y >> 1) & 0xffffffu;
    return deint_average(F(x, deint_row_up(y) >> 1), F(x, deint_row_dn(y, h) >> 1));
}

}  // namespace eppm
