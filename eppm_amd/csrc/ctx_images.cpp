// ctx_images.cpp -- the images of a context (context.h): set_images (set_data, driver :159-168, + _prepare_data :212-215) from host and
// device memory, the frame push of the streaming mode, and the host upload of one image that both share.
#include "context.h"
#include "yuv.h"

using namespace eppm;

// ---- prepare: refine :1060-1071 + .cuh:642-664.  The two frames of every active pair share every launch; the raw
// RGBA planes of the active pairs are in the slabs already.  only2: image 2 alone (eppm_push_image: image 1's planes are the previous
// pair's image-2 planes); every kernel is per pixel of one image, so its planes equal those of a launch that covers both images. ----
static int prepare(eppm_ctx* c, bool only2 = false)
{
    stage_begin(c, c->ev_prep, "prepare");
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    uint32_t **p1 = c->img1, **p2 = c->img2, **tmp = c->tmpu;
    const int p0 = (int)(c->ipitch[0] / 4);
    if (only2) launch_gauss_rgba(p2[0], c->raw2, p0, c->H[0], c->W[0], .5f, 2, s, bt);
    else launch_gauss_rgba2(p1[0], c->raw1, p2[0], c->raw2, p0, c->H[0], c->W[0], .5f, 2, s, bt);    // refine :1063-1064
    const float ratio = 0.5f;                                                             // PYR_RATIO
    const float baseSigma = (1 / ratio - 1);
    const int n = (int)(log(0.25) / (double)logf(ratio));   // C++ float overload in the reference: n = 1
    const float nSigma = baseSigma * n;
    for (int i = 1; i < c->nl; i++) {
        // source level j, blur (sigma, radius), resize ratio r: .cuh:647-663
        const int j = (i <= n) ? 0 : i - n;
        const float sigma = (i <= n) ? baseSigma * i : nSigma;
        const float r = (i <= n) ? (float)pow(ratio, i) : (float)pow(ratio, i) * c->W[0] / c->W[j];
        const int radius = (int)(sigma * 3);
        const int pj = (int)(c->ipitch[j] / 4), pi = (int)(c->ipitch[i] / 4);
        if (gauss_decimate2_ok(c->H[i], c->W[i], c->H[j], c->W[j], r, radius)) {
            // exact 2:1 step: blur only the pixels the decimation keeps (a quarter of the level)
            if (only2) launch_gauss_decimate2(p2[i], p2[j], p2[i], p2[j], 1, pi, c->H[i], c->W[i], pj, c->H[j], c->W[j], sigma, radius, s, bt);
            else launch_gauss_decimate2(p1[i], p1[j], p2[i], p2[j], 2, pi, c->H[i], c->W[i], pj, c->H[j], c->W[j], sigma, radius, s, bt);
        } else {
            for (int k = only2 ? 1 : 0; k < 2; k++) {
                uint32_t** pyr = k ? p2 : p1;
                launch_gauss_rgba(tmp[j], pyr[j], pj, c->H[j], c->W[j], sigma, radius, s, bt);
                launch_resize_rgba(pyr[i], pi, c->H[i], c->W[i], tmp[j], pj, c->H[j], c->W[j], r, s, bt);
            }
        }
    }
    CensusBatch cb;
    cb.n = 0;
    for (int k = only2 ? 1 : 0; k < 2; k++)
        for (int i = 0; i < c->nl; i++) {
            CensusJob& J = cb.job[cb.n++];
            J.census = k ? c->cen2[i] : c->cen1[i]; J.cpitch = (int)c->cpitch[i];
            J.texels = k ? c->pk2[i] : c->pk1[i];   J.tpitch = c->W[i];
            J.img = k ? c->img2[i] : c->img1[i];    J.ipitch = (int)(c->ipitch[i] / 4);
            J.w = c->W[i]; J.h = c->H[i]; J.first_block = 0;
            J.packed = k ? c->pc2[i] : c->pc1[i];
        }
    launch_census_batch(cb, s, bt);
    if (c->pp1) {
        const int L = c->nl - 1;
        if (!only2) launch_parity_planes(c->pp1, c->pp_pitch, c->pp_pad, c->pc1[L], c->W[L], c->W[L], c->H[L], s, bt);
        launch_parity_planes(c->pp2, c->pp_pitch, c->pp_pad, c->pc2[L], c->W[L], c->W[L], c->H[L], s, bt);
    }
    stage_end(c, c->ev_prep);
    HIPCHK(hipGetLastError());
    c->have_images = true;
    c->have_flow = false;
    c->bwd_images = false;
    return EPPM_OK;
}

// One host RGB image (rows row_stride bytes apart) -> dst in the slab's d_rgb plane, on the stream.  An image inside memory registered
// with eppm_host_register / eppm_host_alloc is read by the copy engine where it lies (*direct; `hold` keeps its block in use until the
// caller has seen the DMA complete).  Any other image goes through image `slot` of the current pinned staging buffer (one host copy):
// the first such image of a call (*staged still false) allocates the buffer and its event, or waits for the H2D that last read it.
static int upload_rgb(eppm_ctx* c, uint8_t* dst, const uint8_t* src, size_t row_stride, HostHold& hold, int slot, bool* direct, bool* staged)
{
    const size_t row = (size_t)c->w * 3, img = row * c->h, span = row_stride * (c->h - 1) + row;
    if (hold.add(src, span)) {
        if (row_stride == row) HIPCHK(hipMemcpyAsync(dst, src, img, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemcpy2DAsync(dst, row, src, row_stride, row, c->h, hipMemcpyHostToDevice, c->stream));
        *direct = true;
        return EPPM_OK;
    }
    const int q = c->rgb_cur;
    if (!*staged) {
        HIPCHK(pinned_lazy(&c->h_rgb[q], &c->h_rgb_bytes, img * 2 * c->npairs, c->device));
        if (!c->ev_rgb[q]) HIPCHK(hipEventCreateWithFlags(&c->ev_rgb[q], hipEventDisableTiming));
        else HIPCHK(hipEventSynchronize(c->ev_rgb[q]));
    }
    uint8_t* h = c->h_rgb[q] + (size_t)slot * img;
    copy_rows(h, row, src, row_stride, row, c->h);
    HIPCHK(hipMemcpyAsync(dst, h, img, hipMemcpyHostToDevice, c->stream));
    *staged = true;
    return EPPM_OK;
}
// what a call that uploaded images owes the stream before its kernels: the staging buffer's event, and the mark of the in-place reads
static int upload_done(eppm_ctx* c, bool direct, bool staged)
{
    if (staged) {
        HIPCHK(hipEventRecord(c->ev_rgb[c->rgb_cur], c->stream));
        c->rgb_cur ^= 1;
    }
    if (direct) {
        if (!c->ev_h2d) HIPCHK(hipEventCreateWithFlags(&c->ev_h2d, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_h2d, c->stream));
    }
    return EPPM_OK;
}

// host RGB of pairs 0..n-1 -> H2D -> RGBA planes (bao_rgb2rgba, alpha = 0) -> prepare
static int set_images_host_impl(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride, HostHold& hold)
{
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_set_images: row_stride %zu < 3*w", row_stride);
    HIPCHK(hipSetDevice(c->device));
    const size_t img = (size_t)c->w * 3 * c->h;
    for (int k = 0; k < n; k++)
        if (!rgb1[k] || !rgb2[k]) return set_err(EPPM_ERR_ARG, "eppm_set_images: NULL image");
    bool staged = false, direct = false;
    for (int k = 0; k < n; k++)
        for (int f = 0; f < 2; f++)
            CHK(upload_rgb(c, c->of_pair(c->d_rgb, k) + (size_t)f * img, f ? rgb2[k] : rgb1[k], row_stride, hold, k * 2 + f, &direct, &staged));
    CHK(upload_done(c, direct, staged));
    c->n_active = n;
    c->tmp_drop();                      // a new pair is a new clip, in every slot
    const int p0 = (int)(c->raw_pitch / 4);
    launch_rgb_to_rgba(c->raw1, p0, c->d_rgb, c->h, c->w, c->stream, c->bt());
    launch_rgb_to_rgba(c->raw2, p0, c->d_rgb + img, c->h, c->w, c->stream, c->bt());
    const int r = prepare(c);
    // set_data's contract (a synchronous cudaMemcpy in the reference, driver :165-166): when the call returns the caller may reuse
    // its images.  Staged images were copied above; for images read in place, wait for their DMA (the kernels are queued already).
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}
static int set_images_host(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride)
{
    HostHold hold;
    const int r = set_images_host_impl(c, n, rgb1, rgb2, row_stride, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);     // nothing may still read the blocks when `hold` lets them go
    return r;
}

extern "C" int eppm_set_images(eppm_ctx* c, const uint8_t* rgb1, const uint8_t* rgb2, size_t row_stride)
{
    if (!c || !rgb1 || !rgb2) return set_err(EPPM_ERR_ARG, "eppm_set_images: NULL argument");
    return set_images_host(c, 1, &rgb1, &rgb2, row_stride);
}

extern "C" int eppm_batch_set_images(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride)
{
    if (!c || !rgb1 || !rgb2) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images: %d pairs, context holds %d", n, c->npairs);
    return set_images_host(c, n, rgb1, rgb2, row_stride);
}

// device-resident RGBA of pairs 0..n-1: copied into the slabs' raw planes in stream order (the caller's planes are not
// read after the copies complete, and never in place), then prepare
static int set_images_device(eppm_ctx* c, int n, const void* const* d1, const void* const* d2, size_t pitch)
{
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    for (int k = 0; k < n; k++) {
        if (!d1[k] || !d2[k]) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: NULL image");
        HIPCHK(hipMemcpy2DAsync(c->of_pair(c->raw1, k), c->raw_pitch, d1[k], pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpy2DAsync(c->of_pair(c->raw2, k), c->raw_pitch, d2[k], pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
    }
    c->n_active = n;
    c->tmp_drop();
    return prepare(c);
}

extern "C" int eppm_set_images_device(eppm_ctx* c, const void* d1, const void* d2, size_t pitch)
{
    if (!c || !d1 || !d2) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: NULL argument");
    return set_images_device(c, 1, &d1, &d2, pitch);
}

extern "C" int eppm_batch_set_images_device(eppm_ctx* c, int n, const void* const* d_rgba1, const void* const* d_rgba2, size_t pitch)
{
    if (!c || !d_rgba1 || !d_rgba2) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images_device: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images_device: %d pairs, context holds %d", n, c->npairs);
    return set_images_device(c, n, d_rgba1, d_rgba2, pitch);
}

// ---- frame push: image 2 becomes image 1 by exchanging the context's plane pointers -- the raw frame, every
// pyramid level, census plane and texel plane of the old image 2 are kept --, the new frame becomes image 2 and is prepared alone.  The
// pointers are pair 0's and every pair's planes lie at the same offsets of its slab, so one exchange serves every slot of a batch. ----
static int push_check(eppm_ctx* c, const char* what, bool batch = false)
{
    if (!batch && c->npairs != 1) return set_err(EPPM_ERR_ARG, "%s: a batch context takes one frame per slot (eppm_batch_push_images)", what);
    if (!c->have_images) return set_err(EPPM_ERR_STATE, "%s: no pair set yet (eppm_set_images first)", what);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    return EPPM_OK;
}
// also arms the temporal prior, per slot: the snapshots describe the pair that ends in the new image 1 only directly after that pair's
// compute, and only when the new frame continues the slot's clip (new_clip: NULL, or a byte per active pair)
static void push_swap(eppm_ctx* c, const uint8_t* new_clip = nullptr)
{
    for (int k = 0; k < c->n_active; k++) {
        const bool cut = new_clip && new_clip[k];
        c->tmp_valid[k] = c->temporal && c->tmp_snap[k] && !cut;
        c->tmp_snap[k] = 0;
        c->tmp_cut[k] = cut;
    }
    std::swap(c->raw1, c->raw2);
    for (int l = 0; l < c->nl; l++) {
        std::swap(c->img1[l], c->img2[l]);
        std::swap(c->cen1[l], c->cen2[l]);
        std::swap(c->pk1[l], c->pk2[l]);
        std::swap(c->pc1[l], c->pc2[l]);
    }
    std::swap(c->pp1, c->pp2);
}

static int push_image_host_impl(eppm_ctx* c, const uint8_t* rgb, size_t row_stride, HostHold& hold)
{
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_push_image: row_stride %zu < 3*w", row_stride);
    HIPCHK(hipSetDevice(c->device));
    uint8_t* dst = c->d_rgb + (size_t)c->w * 3 * c->h;     // image 2's half of the RGB staging plane, and of the pinned staging (slot 1)
    bool staged = false, direct = false;
    CHK(upload_rgb(c, dst, rgb, row_stride, hold, 1, &direct, &staged));
    CHK(upload_done(c, direct, staged));
    push_swap(c);
    launch_rgb_to_rgba(c->raw2, (int)(c->raw_pitch / 4), dst, c->h, c->w, c->stream, c->bt());
    const int r = prepare(c, true);
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}

extern "C" int eppm_push_image(eppm_ctx* c, const uint8_t* rgb, size_t row_stride)
{
    if (!c || !rgb) return set_err(EPPM_ERR_ARG, "eppm_push_image: NULL argument");
    CHK(push_check(c, "eppm_push_image"));
    HostHold hold;
    const int r = push_image_host_impl(c, rgb, row_stride, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);
    return r;
}

extern "C" int eppm_push_image_device(eppm_ctx* c, const void* d_rgba, size_t pitch)
{
    if (!c || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_push_image_device: NULL argument");
    CHK(push_check(c, "eppm_push_image_device"));
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_push_image_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    // into the old image 1's raw plane, which the swap then makes image 2's: a copy that fails leaves the context on its old pair
    HIPCHK(hipMemcpy2DAsync(c->raw1, c->raw_pitch, d_rgba, pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
    push_swap(c);
    return prepare(c, true);
}

// ---- the batch forms: one new frame per active pair, slot k's into its image-2 half of d_rgb (pinned staging slot 2k + 1) ----
static int push_images_host_impl(eppm_ctx* c, int n, const uint8_t* const* rgb, size_t row_stride, const uint8_t* new_clip, HostHold& hold)
{
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images: row_stride %zu < 3*w", row_stride);
    for (int k = 0; k < n; k++)
        if (!rgb[k]) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images: NULL image");
    HIPCHK(hipSetDevice(c->device));
    const size_t img = (size_t)c->w * 3 * c->h;
    bool staged = false, direct = false;
    for (int k = 0; k < n; k++) CHK(upload_rgb(c, c->of_pair(c->d_rgb, k) + img, rgb[k], row_stride, hold, k * 2 + 1, &direct, &staged));
    CHK(upload_done(c, direct, staged));
    push_swap(c, new_clip);
    launch_rgb_to_rgba(c->raw2, (int)(c->raw_pitch / 4), c->d_rgb + img, c->h, c->w, c->stream, c->bt());
    const int r = prepare(c, true);
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}

extern "C" int eppm_batch_push_images(eppm_ctx* c, int n, const uint8_t* const* rgb, size_t row_stride, const uint8_t* new_clip)
{
    if (!c || !rgb) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images: NULL argument");
    CHK(push_check(c, "eppm_batch_push_images", true));
    if (n != c->n_active) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images: %d frames, %d pairs are active", n, c->n_active);
    HostHold hold;
    const int r = push_images_host_impl(c, n, rgb, row_stride, new_clip, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);
    return r;
}

extern "C" int eppm_batch_push_images_device(eppm_ctx* c, int n, const void* const* d_rgba, size_t pitch, const uint8_t* new_clip)
{
    if (!c || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images_device: NULL argument");
    CHK(push_check(c, "eppm_batch_push_images_device", true));
    if (n != c->n_active) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images_device: %d frames, %d pairs are active", n, c->n_active);
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images_device: bad pitch %zu", pitch);
    for (int k = 0; k < n; k++)
        if (!d_rgba[k]) return set_err(EPPM_ERR_ARG, "eppm_batch_push_images_device: NULL image");
    HIPCHK(hipSetDevice(c->device));
    // into the old image 1's raw planes, which the swap then makes image 2's
    for (int k = 0; k < n; k++)
        HIPCHK(hipMemcpy2DAsync(c->of_pair(c->raw1, k), c->raw_pitch, d_rgba[k], pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
    push_swap(c, new_clip);
    return prepare(c, true);
}

// ---- Y'CbCr 4:2:0 frames (include/eppm_yuv.h): the calls above with k_yuv_to_rgba in the place of the RGBA copy
// (device forms) or of k_rgb_to_rgba (host forms).  The kernel writes the slabs' raw planes directly; everything after it is shared. ----
// device planes of slots 0 .. n - 1 (3 pointers each) -> the raw plane `raw` of every slot, a launch per chunk of the pointer table
static void yuv_convert(eppm_ctx* c, uint32_t* raw, int n, const void* const* planes, const size_t* pitches, int layout, const YuvK& k)
{
    for (int k0 = 0; k0 < n; k0 += kYuvChunk) {
        const int m = std::min(kYuvChunk, n - k0);
        YuvSlots S = {};
        for (int i = 0; i < m; i++)
            for (int p = 0; p < 3; p++) S.p[i][p] = planes[3 * (k0 + i) + p];
        launch_yuv_to_rgba(S, m, c->of_pair(raw, k0), c->raw_pitch, c->stride, pitches, c->h, c->w, layout, k, c->stream);
    }
}

extern "C" int eppm_yuv_batch_set_images_device(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* d1, const void* const* d2,
                                                const size_t* pitches)
{
    if (!c || !d1 || !d2) return set_err(EPPM_ERR_ARG, "eppm_yuv_set_images_device: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_yuv_set_images_device: %d pairs, context holds %d", n, c->npairs);
    YuvK k;
    CHK(yuv_check("eppm_yuv_set_images_device", f, d1, n, pitches, c->h, c->w, &k));
    CHK(yuv_check("eppm_yuv_set_images_device", f, d2, n, pitches, c->h, c->w, nullptr));
    HIPCHK(hipSetDevice(c->device));
    yuv_convert(c, c->raw1, n, d1, pitches, f->layout, k);
    yuv_convert(c, c->raw2, n, d2, pitches, f->layout, k);
    c->n_active = n;
    c->tmp_drop();
    return prepare(c);
}
extern "C" int eppm_yuv_set_images_device(eppm_ctx* c, const eppm_yuv_format* f, const void* const* d1, const void* const* d2, const size_t* pitches)
{
    return eppm_yuv_batch_set_images_device(c, f, 1, d1, d2, pitches);
}

extern "C" int eppm_yuv_batch_push_images_device(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* d, const size_t* pitches,
                                                 const uint8_t* new_clip)
{
    if (!c || !d) return set_err(EPPM_ERR_ARG, "eppm_yuv_batch_push_images_device: NULL argument");
    CHK(push_check(c, "eppm_yuv_batch_push_images_device", true));
    if (n != c->n_active) return set_err(EPPM_ERR_ARG, "eppm_yuv_batch_push_images_device: %d frames, %d pairs are active", n, c->n_active);
    YuvK k;
    CHK(yuv_check("eppm_yuv_batch_push_images_device", f, d, n, pitches, c->h, c->w, &k));
    HIPCHK(hipSetDevice(c->device));
    yuv_convert(c, c->raw1, n, d, pitches, f->layout, k);      // the old image 1's raw planes, which the swap then makes image 2's
    push_swap(c, new_clip);
    return prepare(c, true);
}
extern "C" int eppm_yuv_push_image_device(eppm_ctx* c, const eppm_yuv_format* f, const void* const* d, const size_t* pitches)
{
    if (!c || !d) return set_err(EPPM_ERR_ARG, "eppm_yuv_push_image_device: NULL argument");
    CHK(push_check(c, "eppm_yuv_push_image_device"));
    return eppm_yuv_batch_push_images_device(c, f, 1, d, pitches, nullptr);
}

// Where host frames are staged.  Depth 8: frame `fr` of pair k in its half of the slab's d_rgb plane and image 2k + fr of the pinned
// h_rgb (wh + 2 ceil(w/2) ceil(h/2) <= 3wh bytes).  16-bit words: the same slots of d_yuv and h_yuv, made here by the first such call.
// The planes of a frame lie packed one after the other, rows without padding.
struct YuvStage {
    bool wide;
    size_t slot;            // bytes of a frame's slot in both stagings
    size_t off[3], row[3];
    int rows[3], np;
    uint8_t* dev(eppm_ctx* c, int k, int fr) const { return wide ? c->d_yuv + (size_t)(2 * k + fr) * slot : c->of_pair(c->d_rgb, k) + (size_t)fr * slot; }
};
static int yuv_stage(eppm_ctx* c, const eppm_yuv_format& f, YuvStage* st)
{
    st->wide = f.depth > 8;
    st->np = f.layout == EPPM_YUV_NV12 ? 2 : 3;
    size_t off = 0;
    for (int p = 0; p < 3; p++) {
        yuv_plane_size(f, c->h, c->w, p, &st->rows[p], &st->row[p]);
        st->off[p] = off;
        off += st->row[p] * st->rows[p];
    }
    st->slot = st->wide ? off : (size_t)c->w * 3 * c->h;
    if (st->wide && !c->d_yuv) {
        const size_t bytes = st->slot * 2 * c->npairs;
        const hipError_t e = cache_alloc((void**)&c->d_yuv, bytes, false, c->device);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            c->d_yuv = nullptr;
            return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (16-bit frame staging) failed: %s", bytes, hipGetErrorString(e));
        }
        c->d_yuv_bytes = bytes;
    }
    return EPPM_OK;
}
// one host frame -> its staging slot, as upload_rgb sends an image.  A frame whose planes all lie in registered memory is read in place,
// a copy per plane (the planes are the caller's, rows and planes apart as they are); any other frame is packed into its slot of this
// turn's pinned buffer -- the planes one after the other, as they lie in the device slot -- and goes up in ONE copy.  dev[3]: where the
// planes went
static int upload_yuv(eppm_ctx* c, const YuvStage& st, int k, int fr, const void* const* planes, const size_t* strides, HostHold& hold, bool* direct,
                      bool* staged, const void** dev)
{
    uint8_t* base = st.dev(c, k, fr);
    size_t bytes = 0;
    bool in_place = true;
    for (int p = 0; p < 3; p++) {
        dev[p] = p < st.np ? base + st.off[p] : nullptr;
        if (p >= st.np) continue;
        bytes = st.off[p] + st.row[p] * st.rows[p];
        in_place = in_place && hold.add(planes[p], strides[p] * (st.rows[p] - 1) + st.row[p]);       // (blocks held for a frame that is then staged are let go with the call)
    }
    if (in_place) {
        for (int p = 0; p < st.np; p++) {
            const size_t row = st.row[p];
            if (strides[p] == row) HIPCHK(hipMemcpyAsync(base + st.off[p], planes[p], row * st.rows[p], hipMemcpyHostToDevice, c->stream));
            else HIPCHK(hipMemcpy2DAsync(base + st.off[p], row, planes[p], strides[p], row, st.rows[p], hipMemcpyHostToDevice, c->stream));
        }
        *direct = true;
        return EPPM_OK;
    }
    const int q = c->rgb_cur;
    if (!*staged) {
        if (st.wide) HIPCHK(pinned_lazy(&c->h_yuv[q], &c->h_yuv_bytes, st.slot * 2 * c->npairs, c->device));
        else HIPCHK(pinned_lazy(&c->h_rgb[q], &c->h_rgb_bytes, st.slot * 2 * c->npairs, c->device));
        if (!c->ev_rgb[q]) HIPCHK(hipEventCreateWithFlags(&c->ev_rgb[q], hipEventDisableTiming));
        else HIPCHK(hipEventSynchronize(c->ev_rgb[q]));
    }
    uint8_t* h = (st.wide ? c->h_yuv[q] : c->h_rgb[q]) + (size_t)(2 * k + fr) * st.slot;
    for (int p = 0; p < st.np; p++) copy_rows(h + st.off[p], st.row[p], (const uint8_t*)planes[p], strides[p], st.row[p], st.rows[p]);
    HIPCHK(hipMemcpyAsync(base, h, bytes, hipMemcpyHostToDevice, c->stream));
    *staged = true;
    return EPPM_OK;
}

static int yuv_set_images_host_impl(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* p1, const void* const* p2, const size_t* strides,
                                    HostHold& hold)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_set_images", f, p1, n, strides, c->h, c->w, &k));
    CHK(yuv_check("eppm_yuv_set_images", f, p2, n, strides, c->h, c->w, nullptr));
    HIPCHK(hipSetDevice(c->device));
    YuvStage st;
    CHK(yuv_stage(c, *f, &st));
    std::vector<const void*> dev[2] = {std::vector<const void*>(3 * (size_t)n), std::vector<const void*>(3 * (size_t)n)};
    bool staged = false, direct = false;
    for (int i = 0; i < n; i++)
        for (int fr = 0; fr < 2; fr++) CHK(upload_yuv(c, st, i, fr, (fr ? p2 : p1) + 3 * i, strides, hold, &direct, &staged, &dev[fr][3 * i]));
    CHK(upload_done(c, direct, staged));
    c->n_active = n;
    c->tmp_drop();
    yuv_convert(c, c->raw1, n, dev[0].data(), st.row, f->layout, k);
    yuv_convert(c, c->raw2, n, dev[1].data(), st.row, f->layout, k);
    const int r = prepare(c);
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}
extern "C" int eppm_yuv_batch_set_images(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* p1, const void* const* p2, const size_t* strides)
{
    if (!c || !p1 || !p2) return set_err(EPPM_ERR_ARG, "eppm_yuv_set_images: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_yuv_set_images: %d pairs, context holds %d", n, c->npairs);
    HostHold hold;
    const int r = yuv_set_images_host_impl(c, f, n, p1, p2, strides, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);     // nothing may still read the blocks when `hold` lets them go
    return r;
}
extern "C" int eppm_yuv_set_images(eppm_ctx* c, const eppm_yuv_format* f, const void* const* p1, const void* const* p2, const size_t* strides)
{
    return eppm_yuv_batch_set_images(c, f, 1, p1, p2, strides);
}

static int yuv_push_images_host_impl(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* planes, const size_t* strides,
                                     const uint8_t* new_clip, HostHold& hold)
{
    YuvK k;
    CHK(yuv_check("eppm_yuv_push_image", f, planes, n, strides, c->h, c->w, &k));
    HIPCHK(hipSetDevice(c->device));
    YuvStage st;
    CHK(yuv_stage(c, *f, &st));
    std::vector<const void*> dev(3 * (size_t)n);
    bool staged = false, direct = false;
    for (int i = 0; i < n; i++) CHK(upload_yuv(c, st, i, 1, planes + 3 * i, strides, hold, &direct, &staged, &dev[3 * i]));   // image 2's slots
    CHK(upload_done(c, direct, staged));
    push_swap(c, new_clip);
    yuv_convert(c, c->raw2, n, dev.data(), st.row, f->layout, k);
    const int r = prepare(c, true);
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}
extern "C" int eppm_yuv_batch_push_images(eppm_ctx* c, const eppm_yuv_format* f, int n, const void* const* planes, const size_t* strides,
                                          const uint8_t* new_clip)
{
    if (!c || !planes) return set_err(EPPM_ERR_ARG, "eppm_yuv_batch_push_images: NULL argument");
    CHK(push_check(c, "eppm_yuv_batch_push_images", true));
    if (n != c->n_active) return set_err(EPPM_ERR_ARG, "eppm_yuv_batch_push_images: %d frames, %d pairs are active", n, c->n_active);
    HostHold hold;
    const int r = yuv_push_images_host_impl(c, f, n, planes, strides, new_clip, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);
    return r;
}
extern "C" int eppm_yuv_push_image(eppm_ctx* c, const eppm_yuv_format* f, const void* const* planes, const size_t* strides)
{
    if (!c || !planes) return set_err(EPPM_ERR_ARG, "eppm_yuv_push_image: NULL argument");
    CHK(push_check(c, "eppm_yuv_push_image"));
    return eppm_yuv_batch_push_images(c, f, 1, planes, strides, nullptr);
}
