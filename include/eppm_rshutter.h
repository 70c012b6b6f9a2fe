/* eppm_rshutter.h -- rolling-shutter correction of a frame along its flow.  Everything here is opt-in: a context
 * that never calls it allocates and launches exactly what it does without this header.
 *
 * A CMOS sensor reads a frame out line by line: the sample at coordinate c along the readout axis (rows; columns for rotated video) of
 * frame k is taken at time k + tau(c), tau(c) = (readout / n) * (c - anchor * (n - 1)) frame intervals, n the frame's length along that
 * axis.  Whatever moves is skewed or squashed.  The correction is a gather: for every pixel q of the output it solves
 * p = q + tau(p) * vel(p) by `iters` fixed-point steps and samples the frame bilinearly at p, so that the output shows every scene point
 * where a global shutter would have seen it at time k.  vel: the level-0 flow the context holds, normalised for the time its vector
 * spans: a pixel with vector (fx, fy) and the component fa along the readout axis has D = sg + (readout / n) * fa (sg = 1 for a flow to
 * the next frame, -1 for a flow to the previous one) and vel = (fx / D, fy / D); an unknown vector and one with sg * D < 0.5 have vel = 0,
 * so a static, unknown or NaN field returns the frame untouched, and so does readout = 0.
 *
 *   frame 0: image 1 along the forward flow, valid after any compute of the current images until the next eppm_set_images* /
 *            eppm_push_image*;
 *   frame 1: image 2 along the backward flow, valid in the window of eppm_interpolate*.
 * EPPM_ERR_STATE outside these windows; EPPM_ERR_ARG for parameters out of range (NaN included), before any GPU call.  params NULL: the
 * defaults.  The first call allocates the context's rolling-shutter scratch (11 bytes per pixel and pair, kept until eppm_destroy).
 * Outputs: h rows of w R,G,B triplets row_stride bytes apart (host), or RGBA words with alpha 255 (device).  A call leaves every plane of
 * the context as it was.  Stage names: "rs_velocity", "rs_gather".  The kernels equal eppm_rolling_shutter_host byte for byte, in both
 * libraries. */
#ifndef EPPM_RSHUTTER_H
#define EPPM_RSHUTTER_H

#include "eppm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eppm_rs_params {
    float readout;               /* share of the frame interval the sensor takes to read a frame, -1 .. 1 (0.5); negative: last line first */
    float anchor;                /* position along the axis whose sampling time is the frame's time, 0 .. 1 (0.5): 0 the first line */
    int   iters;                 /* fixed-point steps, 1 .. 8 (3) */
    int   axis;                  /* 0: rows are read one after another; 1: columns (0) */
} eppm_rs_params;
int  eppm_rs_default_params(eppm_rs_params* p);
/* pair 0; rgb: one host image.  Synchronous. */
int  eppm_rolling_shutter(eppm_ctx* ctx, const eppm_rs_params* params, int frame, uint8_t* rgb, size_t row_stride);
/* pair 0; d_rgba: a device RGBA plane of `pitch` bytes per row.  Asynchronous on the context's stream (no host synchronisation, no
 * allocation after the first call: usable inside stream capture). */
int  eppm_rolling_shutter_device(eppm_ctx* ctx, const eppm_rs_params* params, int frame, void* d_rgba, size_t pitch);
/* every active pair: rgb[pair] receives pair `pair`.  Synchronous. */
int  eppm_batch_rolling_shutter(eppm_ctx* ctx, const eppm_rs_params* params, int frame, uint8_t* const* rgb, size_t row_stride);
/* the kernels alone on caller planes, any size from 1x1 up to 8192x8192 and 2^26 pixels: RGBA input (in_pitch bytes per row, alpha
 * ignored) and output (out_pitch), h*w float2 flow, all device pointers; frame 0: the flow points to the next frame, 1: to the previous
 * one; on the launcher stream, synchronous */
int  eppm_rolling_shutter_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba, size_t in_pitch, const eppm_float2* d_flow,
                                 int h, int w, int frame, const eppm_rs_params* params);
/* host form on a packed RGB image and a planar flow (no GPU needed): byte-identical to the kernels */
int  eppm_rolling_shutter_host(uint8_t* rgb_out, const uint8_t* rgb, const float* u, const float* v, int h, int w, int frame,
                               const eppm_rs_params* params);

#ifdef __cplusplus
}
#endif
#endif
