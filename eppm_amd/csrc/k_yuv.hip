// k_yuv.hip -- Y'CbCr 4:2:0 planes to and from RGBA words (the arithmetic: yuv.h).  Two bandwidth-bound kernels,
// templated on layout (NV12 / I420), sample word (8 / 16 bit), siting and the store form; no LDS, no scratch, plain loads and stores.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "yuv.h"

namespace eppm {

template <class T> __device__ __forceinline__ unsigned yuv_ld(const uint8_t* row, int i) { return ((const T*)row)[i]; }

// Cb and Cr of chroma column j of a chroma row: NV12 reads the interleaved pair of plane 1, I420 one sample of plane 1 and of plane 2
template <bool NV12, class T>
__device__ __forceinline__ void yuv_ld_chroma(const uint8_t* r1, const uint8_t* r2, int j, const YuvK& k, int* cb, int* cr)
{
    if (NV12) {
        *cb = yuv_sample(yuv_ld<T>(r1, 2 * j), k);
        *cr = yuv_sample(yuv_ld<T>(r1, 2 * j + 1), k);
    } else {
        *cb = yuv_sample(yuv_ld<T>(r1, j), k);
        *cr = yuv_sample(yuv_ld<T>(r2, j), k);
    }
}

// ---- to RGBA.  A lane converts the four pixels x0 .. x0 + 3 (x0 = 4 * lane) of row y of slot blockIdx.z and writes them into the slot's
// destination plane: VEC (base and pitch multiples of 16) as one 16-byte store where all four lie inside the row, else word by word, so
// no byte between the rows is written.  The four pixels blend the chroma columns x0 / 2 - 1 .. x0 / 2 + 2 (LEFT: the last three) of two
// chroma rows; the columns are blended vertically first (weight 4), then pairwise (weight 16, one rounding): the same sum as yuv.h's
// tap form, regrouped.  Neighbouring lanes and rows share the chroma samples through the cache.
template <bool NV12, class T, bool CENTER, bool VEC>
__global__ __launch_bounds__(256) void k_yuv_to_rgba(YuvSlots S, uint32_t* __restrict__ dst_, size_t dpitch, size_t dstride, size_t p0, size_t p1,
                                                     size_t p2, int h, int w, YuvK k)
{
    const int x0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x), y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x0 >= w || y >= h) return;
    const int slot = blockIdx.z;
    const uint8_t* __restrict__ py = (const uint8_t*)S.p[slot][0];
    const uint8_t* __restrict__ pu = (const uint8_t*)S.p[slot][1];
    const uint8_t* __restrict__ pv = NV12 ? pu : (const uint8_t*)S.p[slot][2];
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    const YuvTap tv = yuv_tap_center(y, ch);
    const uint8_t *u0 = pu + (size_t)tv.i0 * p1, *u1 = pu + (size_t)tv.i1 * p1;
    const uint8_t *v0 = pv + (size_t)tv.i0 * (NV12 ? p1 : p2), *v1 = pv + (size_t)tv.i1 * (NV12 ? p1 : p2);
    int cb[4], cr[4];
#pragma unroll
    for (int c = CENTER ? 0 : 1; c < 4; c++) {
        const int j = yuv_clampi((x0 >> 1) - 1 + c, 0, cw - 1);
        int b0, r0, b1, r1;
        yuv_ld_chroma<NV12, T>(u0, v0, j, k, &b0, &r0);
        yuv_ld_chroma<NV12, T>(u1, v1, j, k, &b1, &r1);
        cb[c] = tv.w0 * b0 + tv.w1 * b1;
        cr[c] = tv.w0 * r0 + tv.w1 * r1;
    }
    const uint8_t* yrow = py + (size_t)y * p0;
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        // local columns of pixel x0 + i: CENTER (0,1) (1,2) (1,2) (2,3) with weights (1,3) / (3,1); LEFT (1,1) (1,2) (2,2) (2,3) with (4,0) / (2,2)
        const int l0 = CENTER ? (i + 1) >> 1 : 1 + (i >> 1), l1 = CENTER ? l0 + 1 : l0 + (i & 1);
        YuvTap th;
        th.i0 = th.i1 = 0;
        th.w0 = CENTER ? ((i & 1) ? 3 : 1) : ((i & 1) ? 2 : 4);
        th.w1 = 4 - th.w0;
        const int Y = x0 + i < w ? yuv_sample(yuv_ld<T>(yrow, x0 + i), k) : 0;
        o[i] = yuv_to_rgb_pixel(Y, yuv_blend(th, cb[l0], cb[l1]), yuv_blend(th, cr[l0], cr[l1]), k);
    }
    uint32_t* drow = (uint32_t*)((char*)dst_ + (size_t)slot * dstride + (size_t)y * dpitch) + x0;
    if (VEC && x0 + 3 < w) {
        *(uint4*)drow = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (x0 + i < w) drow[i] = o[i];
    }
}

// N samples of type T at p (element 0 of the run), the first n of them inside the plane: ALIGNED (plane base and pitch multiples of 4;
// the run starts at a multiple of 4 bytes by construction) writes a full run as 4-byte words, anything else sample by sample
template <class T, int N, bool ALIGNED>
__device__ __forceinline__ void yuv_store_run(uint8_t* p, const unsigned* v, int n)
{
    constexpr int per = 4 / (int)sizeof(T), bits = 8 * (int)sizeof(T);
    if (ALIGNED && n >= N) {
#pragma unroll
        for (int q = 0; q < N / per; q++) {
            uint32_t word = 0;
#pragma unroll
            for (int e = 0; e < per; e++) word |= (uint32_t)v[q * per + e] << (bits * e);
            ((uint32_t*)p)[q] = word;
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; e++)
            if (e < n) ((T*)p)[e] = (T)v[e];
    }
}

// ---- from RGBA.  A lane owns the four 2 x 2 blocks j0 .. j0 + 3 (j0 = 4 * lane) of block row i: it reads its 2 x 8 RGBA words once (and,
// for LEFT siting, the column to their left), writes two luma runs of 8 samples and the chroma of its four blocks: 8 to 16 bytes per
// store run.  Coordinates outside the frame are clamped for reading and not written.
template <bool NV12, class T, bool CENTER, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rgba_to_yuv(uint8_t* __restrict__ py, uint8_t* __restrict__ pu, uint8_t* __restrict__ pv, size_t p0, size_t p1,
                                                     size_t p2, const uint32_t* __restrict__ src, size_t spitch, int h, int w, YuvK k)
{
    const int j0 = 4 * (blockIdx.x * blockDim.x + threadIdx.x), i = blockIdx.y * blockDim.y + threadIdx.y;
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    if (j0 >= cw || i >= ch) return;
    const int x0 = 2 * j0;
    uint32_t px[2][9];          // [row][column x0 - 1 + c], clamped into the frame
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int y = 2 * i + r < h ? 2 * i + r : h - 1;
        const uint32_t* row = (const uint32_t*)((const char*)src + (size_t)y * spitch);
#pragma unroll
        for (int c = CENTER ? 1 : 0; c < 9; c++) px[r][c] = row[yuv_clampi(x0 - 1 + c, 0, w - 1)];
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (2 * i + r >= h) break;
        unsigned Y[8];
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint32_t p = px[r][c + 1];
            Y[c] = yuv_word(yuv_luma((int)(p & 255u), (int)((p >> 8) & 255u), (int)((p >> 16) & 255u), k), k);
        }
        yuv_store_run<T, 8, ALIGNED>(py + (size_t)(2 * i + r) * p0 + (size_t)x0 * sizeof(T), Y, w - x0);
    }
    unsigned C[8];              // NV12: Cb, Cr interleaved; I420: four Cb, then four Cr
#pragma unroll
    for (int b = 0; b < 4; b++) {
        int s[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const uint32_t a = CENTER ? 0u : px[r][2 * b], m = px[r][2 * b + 1], c = px[r][2 * b + 2];
#pragma unroll
            for (int q = 0; q < 3; q++)
                s[q] += (CENTER ? 0 : 1) * (int)((a >> (8 * q)) & 255u) + (CENTER ? 1 : 2) * (int)((m >> (8 * q)) & 255u) + (int)((c >> (8 * q)) & 255u);
        }
        const unsigned cb = yuv_word(yuv_chroma(k.fu, s[0], s[1], s[2], CENTER ? 2 : 3, k), k);
        const unsigned cr = yuv_word(yuv_chroma(k.fv, s[0], s[1], s[2], CENTER ? 2 : 3, k), k);
        C[NV12 ? 2 * b : b] = cb;
        C[NV12 ? 2 * b + 1 : 4 + b] = cr;
    }
    const int nb = cw - j0;     // blocks of this lane inside the plane, if fewer than four
    if (NV12) {
        yuv_store_run<T, 8, ALIGNED>(pu + (size_t)i * p1 + (size_t)(2 * j0) * sizeof(T), C, 2 * nb);
    } else {
        yuv_store_run<T, 4, ALIGNED>(pu + (size_t)i * p1 + (size_t)j0 * sizeof(T), C, nb);
        yuv_store_run<T, 4, ALIGNED>(pv + (size_t)i * p2 + (size_t)j0 * sizeof(T), C + 4, nb);
    }
}

namespace {

template <bool NV12, class T, bool CENTER>
void to_rgba_vec(bool vec, dim3 grid, dim3 block, hipStream_t s, const YuvSlots& S, uint32_t* dst, size_t dp, size_t ds, const size_t* p, int h, int w,
                 const YuvK& k)
{
    if (vec) hipLaunchKernelGGL((k_yuv_to_rgba<NV12, T, CENTER, true>), grid, block, 0, s, S, dst, dp, ds, p[0], p[1], p[2], h, w, k);
    else hipLaunchKernelGGL((k_yuv_to_rgba<NV12, T, CENTER, false>), grid, block, 0, s, S, dst, dp, ds, p[0], p[1], p[2], h, w, k);
}
template <bool NV12, class T>
void to_rgba_siting(bool vec, dim3 grid, dim3 block, hipStream_t s, const YuvSlots& S, uint32_t* dst, size_t dp, size_t ds, const size_t* p, int h, int w,
                    const YuvK& k)
{
    if (k.center) to_rgba_vec<NV12, T, true>(vec, grid, block, s, S, dst, dp, ds, p, h, w, k);
    else to_rgba_vec<NV12, T, false>(vec, grid, block, s, S, dst, dp, ds, p, h, w, k);
}

template <bool NV12, class T, bool CENTER>
void from_rgba_al(bool al, dim3 grid, dim3 block, hipStream_t s, void* const* pl, const size_t* p, const uint32_t* src, size_t sp, int h, int w, const YuvK& k)
{
    uint8_t *a = (uint8_t*)pl[0], *b = (uint8_t*)pl[1], *c = (uint8_t*)pl[2];
    if (al) hipLaunchKernelGGL((k_rgba_to_yuv<NV12, T, CENTER, true>), grid, block, 0, s, a, b, c, p[0], p[1], p[2], src, sp, h, w, k);
    else hipLaunchKernelGGL((k_rgba_to_yuv<NV12, T, CENTER, false>), grid, block, 0, s, a, b, c, p[0], p[1], p[2], src, sp, h, w, k);
}
template <bool NV12, class T>
void from_rgba_siting(bool al, dim3 grid, dim3 block, hipStream_t s, void* const* pl, const size_t* p, const uint32_t* src, size_t sp, int h, int w,
                      const YuvK& k)
{
    if (k.center) from_rgba_al<NV12, T, true>(al, grid, block, s, pl, p, src, sp, h, w, k);
    else from_rgba_al<NV12, T, false>(al, grid, block, s, pl, p, src, sp, h, w, k);
}

}  // namespace

// the launch-dependent choice of k_yuv_to_rgba: 16-byte stores where the destination allows them
bool yuv_to_rgba_vec(const void* dst, size_t dst_pitch, size_t dst_stride) { return ((uintptr_t)dst | dst_pitch | dst_stride) % 16 == 0; }

void launch_yuv_to_rgba(const YuvSlots& S, int n, uint32_t* dst, size_t dst_pitch, size_t dst_stride, const size_t* pitches, int h, int w, int layout,
                        const YuvK& k, hipStream_t s)
{
    const bool vec = yuv_to_rgba_vec(dst, dst_pitch, dst_stride), nv12 = layout == EPPM_YUV_NV12, w16 = k.peak > 255;
    dim3 block(64, 4), grid(((w + 3) / 4 + 63) / 64, (h + 3) / 4, n);
    if (nv12 && !w16) to_rgba_siting<true, uint8_t>(vec, grid, block, s, S, dst, dst_pitch, dst_stride, pitches, h, w, k);
    else if (nv12) to_rgba_siting<true, uint16_t>(vec, grid, block, s, S, dst, dst_pitch, dst_stride, pitches, h, w, k);
    else if (!w16) to_rgba_siting<false, uint8_t>(vec, grid, block, s, S, dst, dst_pitch, dst_stride, pitches, h, w, k);
    else to_rgba_siting<false, uint16_t>(vec, grid, block, s, S, dst, dst_pitch, dst_stride, pitches, h, w, k);
}

void launch_rgba_to_yuv(void* const* planes, const size_t* pitches, const uint32_t* src, size_t src_pitch, int h, int w, int layout, const YuvK& k,
                        hipStream_t s)
{
    const bool nv12 = layout == EPPM_YUV_NV12, w16 = k.peak > 255;
    uintptr_t bits = (uintptr_t)planes[0] | (uintptr_t)planes[1] | pitches[0] | pitches[1];
    if (!nv12) bits |= (uintptr_t)planes[2] | pitches[2];
    const bool al = bits % 4 == 0;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    dim3 block(64, 4), grid(((cw + 3) / 4 + 63) / 64, (ch + 3) / 4, 1);
    if (nv12 && !w16) from_rgba_siting<true, uint8_t>(al, grid, block, s, planes, pitches, src, src_pitch, h, w, k);
    else if (nv12) from_rgba_siting<true, uint16_t>(al, grid, block, s, planes, pitches, src, src_pitch, h, w, k);
    else if (!w16) from_rgba_siting<false, uint8_t>(al, grid, block, s, planes, pitches, src, src_pitch, h, w, k);
    else from_rgba_siting<false, uint16_t>(al, grid, block, s, planes, pitches, src, src_pitch, h, w, k);
}

}  // namespace eppm
