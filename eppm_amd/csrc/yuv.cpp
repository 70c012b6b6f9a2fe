// yuv.cpp -- Y'CbCr 4:2:0 frames (include/eppm_yuv.h): the format's checks, the host forms and the context-less
// device calls.  The context forms are ctx_images.cpp's, the files eppm_io.cpp's, the arithmetic yuv.h's.
#include "api_internal.h"
#include "yuv.h"

using namespace eppm;

extern "C" int eppm_yuv_default_format(eppm_yuv_format* f)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_yuv_default_format: NULL argument");
    f->layout = EPPM_YUV_NV12;
    f->depth = 8;
    f->msb_aligned = 0;
    f->matrix = EPPM_YUV_BT709;
    f->full_range = 0;
    f->siting = EPPM_YUV_LEFT;
    return EPPM_OK;
}

int yuv_check(const char* what, const eppm_yuv_format* f, const void* const* planes, int nframes, const size_t* pitches, int h, int w, YuvK* k)
{
    if (!f || !planes || !pitches) return set_err(EPPM_ERR_ARG, "%s: NULL argument", what);
    const char* why = nullptr;
    if (!yuv_format_ok(*f, &why)) return set_err(EPPM_ERR_ARG, "%s: bad format: %s", what, why);
    if (h < 1 || w < 1 || h > kYuvMaxDim || w > kYuvMaxDim) return set_err(EPPM_ERR_ARG, "%s: bad size %d x %d", what, w, h);
    const int np = f->layout == EPPM_YUV_NV12 ? 2 : 3;
    for (int p = 0; p < np; p++) {
        int rows;
        size_t row;
        yuv_plane_size(*f, h, w, p, &rows, &row);
        if (pitches[p] < row) return set_err(EPPM_ERR_ARG, "%s: pitch %zu of plane %d is below the row's %zu bytes", what, pitches[p], p, row);
        if (f->depth > 8 && (pitches[p] & 1)) return set_err(EPPM_ERR_ARG, "%s: odd pitch %zu of plane %d for 16-bit words", what, pitches[p], p);
        for (int k2 = 0; k2 < nframes; k2++) {
            const void* q = planes[3 * k2 + p];
            if (!q) return set_err(EPPM_ERR_ARG, "%s: NULL plane %d", what, p);
            if (f->depth > 8 && ((uintptr_t)q & 1)) return set_err(EPPM_ERR_ARG, "%s: plane %d of 16-bit words at an odd address", what, p);
        }
    }
    if (k) *k = yuv_coeffs(*f);
    return EPPM_OK;
}

extern "C" int eppm_yuv_plane_dims(const eppm_yuv_format* f, int h, int w, int plane, int* rows, int* row_bytes)
{
    if (!f || !rows || !row_bytes) return set_err(EPPM_ERR_ARG, "eppm_yuv_plane_dims: NULL argument");
    const char* why = nullptr;
    if (!yuv_format_ok(*f, &why)) return set_err(EPPM_ERR_ARG, "eppm_yuv_plane_dims: bad format: %s", why);
    if (h < 1 || w < 1 || h > kYuvMaxDim || w > kYuvMaxDim) return set_err(EPPM_ERR_ARG, "eppm_yuv_plane_dims: bad size %d x %d", w, h);
    if (plane < 0 || plane > 2) return set_err(EPPM_ERR_ARG, "eppm_yuv_plane_dims: plane %d", plane);
    size_t row;
    yuv_plane_size(*f, h, w, plane, rows, &row);
    *row_bytes = (int)row;
    return EPPM_OK;
}

// ---- the kernels alone ----
extern "C" int eppm_yuv_to_rgba(const eppm_yuv_format* f, const void* const* d_planes, const size_t* pitches, void* d_rgba, size_t pitch, int h, int w,
                                void* stream)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_to_rgba", f, d_planes, 1, pitches, h, w, &k));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_yuv_to_rgba: NULL destination");
    if (pitch < (size_t)w * 4 || (pitch & 3) || ((uintptr_t)d_rgba & 3)) return set_err(EPPM_ERR_ARG, "eppm_yuv_to_rgba: bad RGBA pitch %zu or address", pitch);
    YuvSlots S = {};
    for (int p = 0; p < 3; p++) S.p[0][p] = d_planes[p];
    launch_yuv_to_rgba(S, 1, (uint32_t*)d_rgba, pitch, 0, pitches, h, w, f->layout, k, stream ? (hipStream_t)stream : launcher_stream());
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

extern "C" int eppm_yuv_from_rgba(const eppm_yuv_format* f, const void* d_rgba, size_t pitch, void* const* d_planes, const size_t* pitches, int h, int w,
                                  void* stream)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_from_rgba", f, d_planes, 1, pitches, h, w, &k));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_yuv_from_rgba: NULL source");
    if (pitch < (size_t)w * 4 || (pitch & 3) || ((uintptr_t)d_rgba & 3)) return set_err(EPPM_ERR_ARG, "eppm_yuv_from_rgba: bad RGBA pitch %zu or address", pitch);
    launch_rgba_to_yuv(d_planes, pitches, (const uint32_t*)d_rgba, pitch, h, w, f->layout, k, stream ? (hipStream_t)stream : launcher_stream());
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

// ---- host forms: yuv.h's operations pixel by pixel ----
namespace {
struct HostPlanes {
    const uint8_t* p[3];
    size_t s[3];
    bool w16, nv12;
    unsigned ld(int pl, int row, int idx) const
    {
        const uint8_t* r = p[pl] + (size_t)row * s[pl];
        return w16 ? ((const uint16_t*)r)[idx] : r[idx];
    }
    unsigned cb(int row, int j) const { return nv12 ? ld(1, row, 2 * j) : ld(1, row, j); }
    unsigned cr(int row, int j) const { return nv12 ? ld(1, row, 2 * j + 1) : ld(2, row, j); }
};
}  // namespace

extern "C" int eppm_yuv_to_rgb_host(const eppm_yuv_format* f, const void* const* planes, const size_t* strides, uint8_t* rgb, size_t row_stride, int h, int w)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_to_rgb_host", f, planes, 1, strides, h, w, &k));
    if (!rgb || row_stride < (size_t)w * 3) return set_err(EPPM_ERR_ARG, "eppm_yuv_to_rgb_host: NULL image or row_stride %zu < 3*w", row_stride);
    HostPlanes P;
    for (int p = 0; p < 3; p++) { P.p[p] = (const uint8_t*)planes[p]; P.s[p] = strides[p]; }
    P.w16 = f->depth > 8;
    P.nv12 = f->layout == EPPM_YUV_NV12;
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    for (int y = 0; y < h; y++) {
        const YuvTap tv = yuv_tap_center(y, ch);
        uint8_t* out = rgb + (size_t)y * row_stride;
        for (int x = 0; x < w; x++) {
            const YuvTap th = yuv_tap_h(x, cw, k.center);
            const int b0 = tv.w0 * yuv_sample(P.cb(tv.i0, th.i0), k) + tv.w1 * yuv_sample(P.cb(tv.i1, th.i0), k);
            const int b1 = tv.w0 * yuv_sample(P.cb(tv.i0, th.i1), k) + tv.w1 * yuv_sample(P.cb(tv.i1, th.i1), k);
            const int r0 = tv.w0 * yuv_sample(P.cr(tv.i0, th.i0), k) + tv.w1 * yuv_sample(P.cr(tv.i1, th.i0), k);
            const int r1 = tv.w0 * yuv_sample(P.cr(tv.i0, th.i1), k) + tv.w1 * yuv_sample(P.cr(tv.i1, th.i1), k);
            const uint32_t word = yuv_to_rgb_pixel(yuv_sample(P.ld(0, y, x), k), yuv_blend(th, b0, b1), yuv_blend(th, r0, r1), k);
            out[3 * x] = (uint8_t)word;
            out[3 * x + 1] = (uint8_t)(word >> 8);
            out[3 * x + 2] = (uint8_t)(word >> 16);
        }
    }
    return EPPM_OK;
}

extern "C" int eppm_yuv_from_rgb_host(const eppm_yuv_format* f, const uint8_t* rgb, size_t row_stride, void* const* planes, const size_t* strides, int h, int w)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_from_rgb_host", f, planes, 1, strides, h, w, &k));
    if (!rgb || row_stride < (size_t)w * 3) return set_err(EPPM_ERR_ARG, "eppm_yuv_from_rgb_host: NULL image or row_stride %zu < 3*w", row_stride);
    const bool w16 = f->depth > 8, nv12 = f->layout == EPPM_YUV_NV12;
    auto st = [&](int pl, int row, int idx, int sample) {
        uint8_t* r = (uint8_t*)planes[pl] + (size_t)row * strides[pl];
        if (w16) ((uint16_t*)r)[idx] = (uint16_t)yuv_word(sample, k);
        else r[idx] = (uint8_t)sample;
    };
    auto px = [&](int x, int y) {
        const uint8_t* q = rgb + (size_t)y * row_stride + 3 * (size_t)x;
        return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t p = px(x, y);
            st(0, y, x, yuv_luma((int)(p & 255u), (int)((p >> 8) & 255u), (int)(p >> 16), k));
        }
    const int cw = (w + 1) / 2, ch = (h + 1) / 2, wshift = k.center ? 2 : 3;
    for (int i = 0; i < ch; i++)
        for (int j = 0; j < cw; j++) {
            int s[3];
            yuv_block_sums(j, i, h, w, k.center, px, s);
            const int cb = yuv_chroma(k.fu, s[0], s[1], s[2], wshift, k), cr = yuv_chroma(k.fv, s[0], s[1], s[2], wshift, k);
            if (nv12) { st(1, i, 2 * j, cb); st(1, i, 2 * j + 1, cr); }
            else { st(1, i, j, cb); st(2, i, j, cr); }
        }
    return EPPM_OK;
}
