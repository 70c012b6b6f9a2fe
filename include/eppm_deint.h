/* eppm_deint.h -- motion-compensated deinterlacing.  Everything here is opt-in: a context that never creates a
 * deinterlacer allocates and launches exactly what it does without this header.
 *
 * An interlaced frame of h rows holds two fields taken at two times: field p (0 top, 1 bottom) owns the rows y with (y & 1) == p.  A clip
 * of n frames is processed as 2n FIELD FRAMES of full height at field rate: a field frame's own rows are the field's samples, its other
 * rows the line average of their neighbours (the bob below).  Field frames are what is pushed into a context, and the flows are computed
 * between them.  After the bidirectional call on the pair (field frame k - 1, field frame k) a deinterlacer step makes the progressive
 * frame at the time of field k: its real rows are image 2's bytes; a pixel of a missing row comes from the slot's reference, the previous
 * step's output (image 1 while the slot is empty), gathered along the backward flow, where the gate accepts it, and is the line average
 * of image 2's real rows elsewhere.  The output becomes the reference.  The step never reads the bytes of image 2's missing rows.
 *
 * The gate, all integer.  up / dn: image 2 at the rows y - 1 / y + 1 (a row outside the frame is replaced by the other one);
 * s[c] = (up[c] + dn[c] + 1) >> 1.  The candidate is valid under the temporal filter's conditions: the backward vector is known, the
 * sample position lies inside the frame, occ2 == 0 (unless use_occ == 0).  q[c]: the float32 bilinear sample of the reference, clamped and
 * rounded as the temporal filter's output word.  It is accepted iff it is valid, the step is no cut, and
 * 2 * sum |q[c] - s[c]| <= 2 * thresh + sum |up[c] - dn[c]|.  Mask byte: 0 real row, 1 temporal, 2 spatial.
 * The kernels equal eppm_deint_step_host and eppm_deint_bob_host byte for byte, in both libraries. */
#ifndef EPPM_DEINT_H
#define EPPM_DEINT_H

#include "eppm_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eppm_deint_params {
    int thresh;                  /* the gate's slack, 0 .. 765 (24) */
    int use_occ;                 /* 1: an occluded pixel (occ2 != 0) has no candidate; 0: the mask is ignored (1) */
} eppm_deint_params;
typedef struct eppm_deint_stats {
    int64_t temporal;            /* missing pixels taken from the reference (mask 1) */
    int64_t spatial;             /* missing pixels filled by the line average (mask 2) */
} eppm_deint_stats;
typedef struct eppm_deint eppm_deint;

int  eppm_deint_default_params(eppm_deint_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty.  The frame needs h >= 2. */
int  eppm_deint_create(eppm_ctx* ctx, const eppm_deint_params* p, eppm_deint** out);
/* an object without a context, for eppm_deint_step_frames on caller planes: nslots slots of h x w pixels (h >= 2) */
int  eppm_deint_create_size(int h, int w, int nslots, int device, const eppm_deint_params* p, eppm_deint** out);
int  eppm_deint_destroy(eppm_deint* f);             /* NULL is fine */
int  eppm_deint_reset(eppm_deint* f, int slot);     /* the slot is empty again; slot < 0: every slot */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames, the level-0 backward flow
 * and occ2): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions, another
 * device or more active pairs than the object has slots.  parity: one byte per active pair, 0 or 1: the rows of that pair's image 2 that are
 * real (NULL: EPPM_ERR_ARG).  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair is the first frame of another clip,
 * so nothing is taken from the reference.  A slot the step does not cover keeps its state.  One launch, asynchronous on the context's
 * stream: no copy, no allocation, no host synchronisation. */
int  eppm_deint_step(eppm_deint* f, eppm_ctx* ctx, const uint8_t* cut, const uint8_t* parity);
/* the same step of one slot on caller device planes of the object's size (RGBA images of `pitch` bytes per row, h*w float2 backward flow,
 * h*w mask bytes; the images on a multiple of 4 bytes, the flow of 8: EPPM_ERR_ARG otherwise); on the launcher stream, synchronous.
 * d_rgba1 is read only if the slot is empty.  Whatever the planes hold, nothing
 * outside them is read. */
int  eppm_deint_step_frames(eppm_deint* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                            const uint8_t* d_occ2, int cut, int parity);
/* the slot's progressive frame of the last step (EPPM_ERR_STATE on a slot never stepped): packed RGB to the host, synchronous ... */
int  eppm_deint_get(eppm_deint* f, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the object's last step */
int  eppm_deint_get_device(eppm_deint* f, int slot, void* d_rgba, size_t pitch);
/* synchronous (EPPM_ERR_STATE on a slot never stepped): the last step's mask, h*w bytes, and its counts, added up on the host */
int  eppm_deint_get_mask(eppm_deint* f, int slot, uint8_t* mask);
int  eppm_deint_get_stats(eppm_deint* f, int slot, eppm_deint_stats* stats);
/* synchronous.  The slot's reference frame (packed RGB, h*w*3) and whether the slot is empty (EPPM_ERR_STATE on a slot that was never
 * stepped nor loaded) / load them: a later eppm_deint_get returns the loaded frame */
int  eppm_deint_get_state(eppm_deint* f, int slot, uint8_t* rgb, int* empty);
int  eppm_deint_set_state(eppm_deint* f, int slot, const uint8_t* rgb, int empty);
/* host form (no GPU needed): one step on packed RGB frames; rgb_ref: the reference (image 1 for an empty slot), rgb_cur: image 2 (its
 * missing rows are not read), (bu, bv): the backward flow, occ2: the mask.  mask_out: h*w bytes.  rgb_out must not be rgb_ref. */
int  eppm_deint_step_host(const eppm_deint_params* p, uint8_t* rgb_out, uint8_t* mask_out, eppm_deint_stats* stats, const uint8_t* rgb_ref,
                          const uint8_t* rgb_cur, const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int parity, int cut);

/* The bob: the full h x w frame (h >= 2) of a field picture of fh = (h - parity + 1) / 2 rows.  Row 2i + parity is field row i; every other
 * row is the line average of its neighbours, per colour (up + dn + 1) >> 1.  Device form: RGBA words both sides, rows `pitch` bytes apart (a
 * multiple of 4), alpha 0 as the YUV path's RGBA outputs carry; asynchronous on the launcher stream, or on `stream` (a hipStream_t, NULL:
 * the launcher stream).  Host form: packed RGB both sides. */
int  eppm_deint_bob(void* d_out, size_t out_pitch, const void* d_field, size_t field_pitch, int h, int w, int parity);
int  eppm_deint_bob_stream(void* d_out, size_t out_pitch, const void* d_field, size_t field_pitch, int h, int w, int parity, void* stream);
int  eppm_deint_bob_host(uint8_t* rgb_out, const uint8_t* rgb_field, int h, int w, int parity);

/* eppm_y4m_open_read for files that may be interlaced: Ip (or no I tag), It and Ib are accepted, *interlace is 0 progressive, 1 top field
 * first, 2 bottom field first.  Im (mixed) is refused by name.  An interlaced 4:2:0 file needs h % 4 == 0, so that each field is itself a
 * 4:2:0 picture (EPPM_ERR_ARG with a message otherwise).  Frames are read with eppm_y4m_read_frame: whole frames, both fields woven. */
int  eppm_deint_y4m_open_read(eppm_y4m** out, const char* path, int* h, int* w, eppm_yuv_format* f, int* fps_num, int* fps_den, int* interlace);

#ifdef __cplusplus
}
#endif
#endif
