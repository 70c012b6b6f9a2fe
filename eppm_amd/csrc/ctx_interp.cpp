// ctx_interp.cpp -- what reads the results of a context's (context.h) last call: frame interpolation, the synthetic shutter, rolling-shutter
// correction, and the one view of a context that the nine per-clip stage objects share (stage_object.h).
#include "context.h"
#include "stage_object.h"
#include "interp.h"
#include "mblur.h"
#include "rshutter.h"
#include "../../include/eppm_rshutter.h"

using namespace eppm;

// ---- frame interpolation: the raw RGBA frames (written only by set_images, read only by prepare), the level-0
// forward flow and both masks of the last bidirectional call, all still in the context ----

static int itp_alloc(eppm_ctx* c)
{
    if (c->itp) return EPPM_OK;
    const size_t n = (size_t)c->h * c->w, slots = (size_t)c->npairs * kInterpChunk;
    const size_t plane = (n + 63) & ~(size_t)63;
    const size_t keys = slots * plane * 8, fills = slots * plane * 4, rgb = slots * n * 3;
    Carve cv;                           // (every size but the last is a multiple of 256 bytes)
    cv.plane(&c->itp_keys, keys);
    for (int32_t** p : {&c->itp_fill1, &c->itp_fill2}) cv.plane(p, fills);
    cv.plane(&c->itp_rgb, rgb);
    CHK(cv.alloc(&c->itp, &c->itp_bytes, keys + 2 * fills + rgb, c->device, "interpolation scratch"));
    c->itp_plane = plane;
    return EPPM_OK;
}

static int interp_check(eppm_ctx* c, const char* what, int nt, const float* t)
{
    if (nt < 1 || !t) return set_err(EPPM_ERR_ARG, "%s: nt %d, t %p", what, nt, (const void*)t);
    for (int k = 0; k < nt; k++)
        if (!interp_t_ok(t[k])) return set_err(EPPM_ERR_ARG, "%s: t[%d] = %g outside [0, 1]", what, k, t[k]);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (!c->have_bwd || !c->bwd_images) return set_err(EPPM_ERR_STATE, "%s: needs a bidirectional call on the current images", what);
    return EPPM_OK;
}

// times t[k0 .. k0+nt) of the first npairs pairs: splat, fill, blend into the packed RGB scratch (d_rgba NULL) or into d_rgba[k0 + k] (pair 0)
static int interp_chunk(eppm_ctx* c, int npairs, int k0, int nt, const float* t, void* const* d_rgba, size_t pitch)
{
    InterpArgs a{};
    a.img1 = (const uint8_t*)c->raw1; a.img2 = (const uint8_t*)c->raw2; a.img_pitch = c->raw_pitch; a.img_stride = c->stride;
    a.flow = c->flow[0]; a.flow_stride = c->stride;
    a.occ1 = c->occ1; a.occ2 = c->occ2; a.occ_stride = c->bwd_stride;
    a.keys = c->itp_keys; a.fill1 = c->itp_fill1; a.fill2 = c->itp_fill2; a.plane = c->itp_plane;
    a.rgb = d_rgba ? nullptr : c->itp_rgb;
    a.rgba_pitch = pitch;
    a.h = c->h; a.w = c->w; a.nt = nt;
    for (int k = 0; k < kInterpChunk; k++) {
        a.t[k] = k < nt ? t[k0 + k] : 0.0f;
        a.rgba[k] = (d_rgba && k < nt) ? (uint8_t*)d_rgba[k0 + k] : nullptr;
    }
    stage_begin(c, c->ev, "interp_splat");
    launch_interp_splat(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "interp_fill");
    launch_interp_fill(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "interp_blend");
    launch_interp_blend(a, npairs, c->stream);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

// host-pointer forms: each chunk's packed RGB outputs cross PCIe once (3 B/px) into the pinned copy, then into the caller's rows
static int interp_host(eppm_ctx* c, const char* what, int npairs, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    CHK(interp_check(c, what, nt, t));
    if (!rgb) return set_err(EPPM_ERR_ARG, "%s: NULL rgb", what);
    for (int k = 0; k < npairs * nt; k++)
        if (!rgb[k]) return set_err(EPPM_ERR_ARG, "%s: NULL rgb[%d]", what, k);
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "%s: row_stride %zu < 3*w", what, row_stride);
    HIPCHK(hipSetDevice(c->device));
    CHK(itp_alloc(c));
    const size_t img = (size_t)c->h * c->w * 3, row = (size_t)c->w * 3;
    HIPCHK(pinned_lazy(&c->h_itp, &c->h_itp_bytes, img * c->npairs * kInterpChunk, c->device));
    for (int k0 = 0; k0 < nt; k0 += kInterpChunk) {
        const int m = nt - k0 < kInterpChunk ? nt - k0 : kInterpChunk;
        CHK(interp_chunk(c, npairs, k0, m, t, nullptr, 0));
        HIPCHK(hipMemcpyAsync(c->h_itp, c->itp_rgb, img * npairs * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int p = 0; p < npairs; p++)
            for (int k = 0; k < m; k++) copy_rows(rgb[(size_t)p * nt + k0 + k], row_stride, c->h_itp + img * ((size_t)p * m + k), row, row, c->h);
    }
    return EPPM_OK;
}

extern "C" int eppm_interpolate(eppm_ctx* c, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_interpolate: NULL ctx");
    return interp_host(c, "eppm_interpolate", 1, nt, t, rgb, row_stride);
}

extern "C" int eppm_batch_interpolate(eppm_ctx* c, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_interpolate: NULL ctx");
    return interp_host(c, "eppm_batch_interpolate", c->n_active, nt, t, rgb, row_stride);
}

extern "C" int eppm_interpolate_device(eppm_ctx* c, int nt, const float* t, void* const* d_rgba, size_t pitch)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL ctx");
    CHK(interp_check(c, "eppm_interpolate_device", nt, t));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL d_rgba");
    for (int k = 0; k < nt; k++)
        if (!d_rgba[k]) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL d_rgba[%d]", k);
    if (bad_pitch(pitch, c->w)) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    CHK(itp_alloc(c));
    for (int k0 = 0; k0 < nt; k0 += kInterpChunk)
        CHK(interp_chunk(c, 1, k0, nt - k0 < kInterpChunk ? nt - k0 : kInterpChunk, t, d_rgba, pitch));
    return EPPM_OK;
}

// ---- synthetic shutter: one raw RGBA frame and the level-0 flow defined on it.  frame 0: image 1 and the forward
// flow, after any compute of the current images; frame 1: image 2 and the backward flow, in the window of eppm_interpolate* ----

static int mbl_alloc(eppm_ctx* c)
{
    if (c->mbl) return EPPM_OK;
    const size_t n = (size_t)c->h * c->w;
    const size_t plane = (n + 63) & ~(size_t)63;
    const size_t tplane = ((size_t)((c->h + kMBlurTile - 1) / kMBlurTile) * ((c->w + kMBlurTile - 1) / kMBlurTile) + 31) & ~(size_t)31;
    const size_t packed = c->npairs * plane * 4, keys = c->npairs * tplane * 8, rgb = c->npairs * n * 3;
    Carve cv;                           // (every size but the last is a multiple of 256 bytes)
    cv.plane(&c->mbl_packed, packed);
    cv.plane(&c->mbl_tkeys, keys);
    cv.plane(&c->mbl_rgb, rgb);
    CHK(cv.alloc(&c->mbl, &c->mbl_bytes, packed + keys + rgb, c->device, "motion-blur scratch"));
    c->mbl_plane = plane;
    c->mbl_tplane = tplane;
    return EPPM_OK;
}

static int mblur_check(eppm_ctx* c, const char* what, const eppm_mblur_params* p, int frame, eppm_mblur_params* prm)
{
    if (p) *prm = *p;
    else (void)eppm_mblur_default_params(prm);
    if (!mblur_params_ok(prm->shutter, prm->max_radius, prm->taps))
        return set_err(EPPM_ERR_ARG, "%s: shutter %g (0 < s <= 1), max_radius %g (1 .. 31), taps %d (1 .. 32)", what, prm->shutter, prm->max_radius, prm->taps);
    if (frame != 0 && frame != 1) return set_err(EPPM_ERR_ARG, "%s: frame %d (0: image 1, 1: image 2)", what, frame);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (frame == 0 && !c->have_flow) return set_err(EPPM_ERR_STATE, "%s: frame 0 needs a compute on the current images", what);
    if (frame == 1 && (!c->have_flow || !c->have_bwd || !c->bwd_images))
        return set_err(EPPM_ERR_STATE, "%s: frame 1 needs a bidirectional call on the current images", what);
    return EPPM_OK;
}

// the first npairs pairs: pack, gather into the packed RGB scratch (d_rgba NULL) or into d_rgba (pair 0)
static int mblur_run(eppm_ctx* c, const eppm_mblur_params& prm, int frame, int npairs, void* d_rgba, size_t pitch)
{
    MBlurArgs a{};
    a.img = (const uint8_t*)(frame ? c->raw2 : c->raw1); a.img_pitch = c->raw_pitch; a.img_stride = c->stride;
    a.flow = frame ? c->bflow[0] : c->flow[0]; a.flow_stride = frame ? c->bwd_stride : c->stride;
    a.packed = c->mbl_packed; a.tkeys = c->mbl_tkeys; a.plane = c->mbl_plane; a.tplane = c->mbl_tplane;
    a.rgb = d_rgba ? nullptr : c->mbl_rgb;
    a.rgba = (uint8_t*)d_rgba; a.rgba_pitch = pitch;
    a.h = c->h; a.w = c->w;
    a.tiles_x = (c->w + kMBlurTile - 1) / kMBlurTile; a.tiles_y = (c->h + kMBlurTile - 1) / kMBlurTile;
    a.shutter = prm.shutter; a.max_radius = prm.max_radius; a.taps = prm.taps;
    stage_begin(c, c->ev, "mblur_pack");
    launch_mblur_pack(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "mblur_gather");
    launch_mblur_gather(a, npairs, c->stream);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

// host-pointer forms: the packed RGB outputs cross PCIe once (3 B/px) into the pinned copy, then into the caller's rows
static int mblur_host(eppm_ctx* c, const char* what, const eppm_mblur_params* p, int frame, int npairs, uint8_t* const* rgb, size_t row_stride)
{
    eppm_mblur_params prm;
    CHK(mblur_check(c, what, p, frame, &prm));
    if (!rgb) return set_err(EPPM_ERR_ARG, "%s: NULL rgb", what);
    for (int k = 0; k < npairs; k++)
        if (!rgb[k]) return set_err(EPPM_ERR_ARG, "%s: NULL rgb[%d]", what, k);
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "%s: row_stride %zu < 3*w", what, row_stride);
    HIPCHK(hipSetDevice(c->device));
    CHK(mbl_alloc(c));
    const size_t img = (size_t)c->h * c->w * 3, row = (size_t)c->w * 3;
    HIPCHK(pinned_lazy(&c->h_mbl, &c->h_mbl_bytes, img * c->npairs, c->device));
    CHK(mblur_run(c, prm, frame, npairs, nullptr, 0));
    HIPCHK(hipMemcpyAsync(c->h_mbl, c->mbl_rgb, img * npairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < npairs; k++) copy_rows(rgb[k], row_stride, c->h_mbl + img * k, row, row, c->h);
    return EPPM_OK;
}

extern "C" int eppm_motion_blur(eppm_ctx* c, const eppm_mblur_params* p, int frame, uint8_t* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_motion_blur: NULL ctx");
    return mblur_host(c, "eppm_motion_blur", p, frame, 1, &rgb, row_stride);
}

extern "C" int eppm_batch_motion_blur(eppm_ctx* c, const eppm_mblur_params* p, int frame, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_motion_blur: NULL ctx");
    return mblur_host(c, "eppm_batch_motion_blur", p, frame, c->n_active, rgb, row_stride);
}

extern "C" int eppm_motion_blur_device(eppm_ctx* c, const eppm_mblur_params* p, int frame, void* d_rgba, size_t pitch)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_motion_blur_device: NULL ctx");
    eppm_mblur_params prm;
    CHK(mblur_check(c, "eppm_motion_blur_device", p, frame, &prm));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_motion_blur_device: NULL d_rgba");
    if (bad_pitch(pitch, c->w)) return set_err(EPPM_ERR_ARG, "eppm_motion_blur_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    CHK(mbl_alloc(c));
    return mblur_run(c, prm, frame, 1, d_rgba, pitch);
}

// ---- rolling-shutter correction (include/eppm_rshutter.h): the synthetic shutter's inputs and windows.  One block of
// the context's own, made by the first call: per pair the velocity plane (8 B/px), then the packed RGB outputs (3 B/px) ----

static int rs_alloc(eppm_ctx* c)
{
    if (c->rsh) return EPPM_OK;
    const size_t n = (size_t)c->h * c->w;
    const size_t plane = (n + 31) & ~(size_t)31;
    const size_t vel = c->npairs * plane * 8, rgb = c->npairs * n * 3;
    Carve cv;                           // (the first size is a multiple of 256 bytes)
    cv.plane(&c->rsh_vel, vel);
    cv.plane(&c->rsh_rgb, rgb);
    CHK(cv.alloc(&c->rsh, &c->rsh_bytes, vel + rgb, c->device, "rolling-shutter scratch"));
    c->rsh_plane = plane;
    return EPPM_OK;
}

static int rs_check(eppm_ctx* c, const char* what, const eppm_rs_params* p, int frame, eppm_rs_params* prm)
{
    if (p) *prm = *p;
    else (void)eppm_rs_default_params(prm);
    if (!rs_params_ok(prm->readout, prm->anchor, prm->iters, prm->axis))
        return set_err(EPPM_ERR_ARG, "%s: readout %g (-1 .. 1), anchor %g (0 .. 1), iters %d (1 .. 8), axis %d (0, 1)", what, prm->readout, prm->anchor, prm->iters, prm->axis);
    if (frame != 0 && frame != 1) return set_err(EPPM_ERR_ARG, "%s: frame %d (0: image 1, 1: image 2)", what, frame);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (frame == 0 && !c->have_flow) return set_err(EPPM_ERR_STATE, "%s: frame 0 needs a compute on the current images", what);
    if (frame == 1 && (!c->have_flow || !c->have_bwd || !c->bwd_images))
        return set_err(EPPM_ERR_STATE, "%s: frame 1 needs a bidirectional call on the current images", what);
    return EPPM_OK;
}

// the first npairs pairs: velocity, gather into the packed RGB scratch (d_rgba NULL) or into d_rgba (pair 0)
static int rs_run(eppm_ctx* c, const eppm_rs_params& prm, int frame, int npairs, void* d_rgba, size_t pitch)
{
    RShutterArgs a{};
    a.img = (const uint8_t*)(frame ? c->raw2 : c->raw1); a.img_pitch = c->raw_pitch; a.img_stride = c->stride;
    a.flow = frame ? c->bflow[0] : c->flow[0]; a.flow_stride = frame ? c->bwd_stride : c->stride;
    a.vel = c->rsh_vel; a.plane = c->rsh_plane;
    a.rgb = d_rgba ? nullptr : c->rsh_rgb;
    a.rgba = (uint8_t*)d_rgba; a.rgba_pitch = pitch;
    a.h = c->h; a.w = c->w;
    a.readout = prm.readout; a.anchor = prm.anchor; a.iters = prm.iters; a.axis = prm.axis; a.frame = frame;
    stage_begin(c, c->ev, "rs_velocity");
    launch_rs_velocity(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "rs_gather");
    launch_rs_gather(a, npairs, c->stream);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

// host-pointer forms: the packed RGB outputs cross PCIe once (3 B/px) into the pinned copy, then into the caller's rows
static int rs_host(eppm_ctx* c, const char* what, const eppm_rs_params* p, int frame, int npairs, uint8_t* const* rgb, size_t row_stride)
{
    eppm_rs_params prm;
    CHK(rs_check(c, what, p, frame, &prm));
    if (!rgb) return set_err(EPPM_ERR_ARG, "%s: NULL rgb", what);
    for (int k = 0; k < npairs; k++)
        if (!rgb[k]) return set_err(EPPM_ERR_ARG, "%s: NULL rgb[%d]", what, k);
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "%s: row_stride %zu < 3*w", what, row_stride);
    HIPCHK(hipSetDevice(c->device));
    CHK(rs_alloc(c));
    const size_t img = (size_t)c->h * c->w * 3, row = (size_t)c->w * 3;
    HIPCHK(pinned_lazy(&c->h_rsh, &c->h_rsh_bytes, img * c->npairs, c->device));
    CHK(rs_run(c, prm, frame, npairs, nullptr, 0));
    HIPCHK(hipMemcpyAsync(c->h_rsh, c->rsh_rgb, img * npairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < npairs; k++) copy_rows(rgb[k], row_stride, c->h_rsh + img * k, row, row, c->h);
    return EPPM_OK;
}

extern "C" int eppm_rolling_shutter(eppm_ctx* c, const eppm_rs_params* p, int frame, uint8_t* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter: NULL ctx");
    return rs_host(c, "eppm_rolling_shutter", p, frame, 1, &rgb, row_stride);
}

extern "C" int eppm_batch_rolling_shutter(eppm_ctx* c, const eppm_rs_params* p, int frame, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_rolling_shutter: NULL ctx");
    return rs_host(c, "eppm_batch_rolling_shutter", p, frame, c->n_active, rgb, row_stride);
}

extern "C" int eppm_rolling_shutter_device(eppm_ctx* c, const eppm_rs_params* p, int frame, void* d_rgba, size_t pitch)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_device: NULL ctx");
    eppm_rs_params prm;
    CHK(rs_check(c, "eppm_rolling_shutter_device", p, frame, &prm));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_device: NULL d_rgba");
    if (bad_pitch(pitch, c->w)) return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    CHK(rs_alloc(c));
    return rs_run(c, prm, frame, 1, d_rgba, pitch);
}

// ---- the per-clip stage objects (stage_object.h): what the tracker, the temporal filter, the stabiliser, the cut
// detector, the correspondence map, the object detector and the background plate read of a context, in the window of eppm_interpolate* ----

int ctx_stage_inputs(eppm_ctx* c, const StageObject* o, const char* what, CtxPlanes* in, hipStream_t* s, const int* pair)
{
    if (c->h != o->h || c->w != o->w || c->device != o->device)
        return set_err(EPPM_ERR_ARG, "%s: the %s is %dx%d on device %d, the context %dx%d on device %d", what, o->noun, o->w, o->h, o->device, c->w, c->h, c->device);
    if (!pair && c->n_active > o->nslots)
        return set_err(EPPM_ERR_ARG, "%s: the context has %d active pairs, the %s %d slots", what, c->n_active, o->noun, o->nslots);
    if (pair && (*pair < 0 || *pair >= c->n_active)) return set_err(EPPM_ERR_ARG, "%s: pair %d, the context has %d active", what, *pair, c->n_active);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (!c->have_bwd || !c->bwd_images) return set_err(EPPM_ERR_STATE, "%s: needs a bidirectional call on the current images", what);
    HIPCHK(hipSetDevice(c->device));
    const int k = pair ? *pair : 0;
    in->img1 = (const uint8_t*)c->of_pair(c->raw1, k);
    in->img2 = (const uint8_t*)c->of_pair(c->raw2, k);
    in->img_pitch = c->raw_pitch;
    in->img_stride = c->stride;
    in->fwd = c->of_pair(c->flow[0], k);
    in->fwd_stride = c->stride;
    in->bwd = c->of_bwd_pair(c->bflow[0], k);
    in->bwd_stride = c->bwd_stride;
    in->occ1 = c->of_bwd_pair(c->occ1, k);
    in->occ2 = c->of_bwd_pair(c->occ2, k);
    in->occ_stride = c->bwd_stride;
    in->n = pair ? 1 : c->n_active;
    *s = c->stream;
    return EPPM_OK;
}
