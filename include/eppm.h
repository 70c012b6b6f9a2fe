/*
 * eppm.h -- C ABI of the MI355X-native EPPM optical-flow engine (libeppm_hip.so).
 *
 * Drop-in boundary for the hot path of linchaobao/EPPM: image pair -> dense flow.
 * Two layers are exported:
 *
 *  (1) the context API (eppm_*): what a host program or an FFI binding uses.  It replaces
 *      class bao_flow_patchmatch_multiscale_cuda (bao_flow_patchmatch_multiscale_cuda.h:33-44):
 *      eppm_create      <- init(h,w)                                   driver .cpp:112-157
 *      eppm_set_images  <- set_data(img1,img2)                         driver .cpp:159-168
 *      eppm_compute     <- compute_flow(disp1_x,disp1_y)               driver .cpp:217-306
 *      eppm_destroy     <- ~bao_flow_patchmatch_multiscale_cuda()      driver .cpp:170-209
 *      The C++ class itself is kept, source compatible, in
 *      include/bao_flow_patchmatch_multiscale_cuda.h on top of this ABI.
 *
 *  (2) the nine live stage launchers of the reference's link-level ABI, with the reference's
 *      names, argument order and meaning (driver .cpp:40-62): see "stage launchers" below.
 *
 * Conventions: plain pointers and sizes only; every function returns an eppm_status
 * (0 = OK) except the reference-signature launchers, which are void like the originals
 * and record their status for eppm_last_error().  Nothing in this library calls exit().
 * One context = one device + one stream; contexts are independent (one per host thread or
 * per GPU); a single context is not thread-safe.
 */
#ifndef EPPM_H_
#define EPPM_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    EPPM_OK = 0,
    EPPM_ERR_ARG = 1,        /* bad argument (NULL, non-positive size, unsupported parameter) */
    EPPM_ERR_HIP = 2,        /* a HIP runtime call failed; see eppm_last_error() */
    EPPM_ERR_STATE = 3,      /* call order: compute before set_images, ... */
    EPPM_ERR_NOMEM = 4
} eppm_status;

/* Pixel / vector element layouts (identical to CUDA's uchar4 / short2 / float2). */
typedef struct { uint8_t x, y, z, w; } eppm_uchar4;
typedef struct { int16_t x, y; } eppm_short2;
typedef struct { float x, y; } eppm_float2;

/* Tunables.  The reference fixes them at compile time (defs.h:31-76); defaults are those values. */
typedef struct {
    int patch_r;        /* PATCH_R 9 (odd, <= 31)                         defs.h:44 */
    int num_iter;       /* NUM_ITER 10                                    defs.h:45 */
    int search_range;   /* SEARCH_RANGE 30                                defs.h:36 */
    int num_guess;      /* NUM_RAND_GUESS 6 (<= 8)                        defs.h:38 */
    int seg_len;        /* PROP_SEG_LENGTH 10              bao_pmflow_kernel.cu:979 */
    int wmf_iters;      /* 20                                         driver .cpp:239 */
    unsigned long long seed; /* 1234                        bao_pmflow_kernel.cu:68 */
    int propagation;    /* 0: segmented scan-line sweeps, baoSegPropagate (live, bao_pmflow_kernel.cu:1812)
                           1: jump flood, baoJumpPropagate (steps 32..1, :800-857; disabled in the reference :1813)
                           2: 4-neighbour propagation, 10x baoParallelPropagate (:720-795; disabled at :1804-1809) */
    int levels;         /* PYR_MAX_DEPTH 3 (1..8): pyramid depth; PatchMatch runs at level levels-1   defs.h:31 */
} eppm_params;

typedef struct eppm_ctx eppm_ctx;

/* ----------------------------------------------------------------------------------------
 * context API
 * -------------------------------------------------------------------------------------- */
int  eppm_default_params(eppm_params* p);
/* Allocates every device buffer for an h x w pair (3-level pyramid, PYR_MAX_DEPTH defs.h:31). */
int  eppm_create(eppm_ctx** out, int h, int w, int device, const eppm_params* params /* NULL = defaults */);
int  eppm_destroy(eppm_ctx* ctx);
/* Use an existing hipStream_t (passed as void*) instead of the context's own stream. */
int  eppm_set_stream(eppm_ctx* ctx, void* hip_stream);

/* Host images: h rows of w RGB triplets, row_stride bytes apart (>= 3*w).  RGB->RGBA, H2D,
 * prefilter, pyramid, census (set_data + _prepare_data, driver .cpp:159-168,212-215). */
int  eppm_set_images(eppm_ctx* ctx, const uint8_t* rgb1, const uint8_t* rgb2, size_t row_stride);
/* Caller memory pinned for DMA.  eppm_set_images / eppm_batch_set_images read an image that lies inside a registered block where
 * it is (no staging copy), and eppm_compute / eppm_compute_begin_into / the batch forms write flow planes that lie inside
 * registered blocks directly; anything else goes through the context's pinned staging buffers (one host copy each way), with
 * identical results.  Register the buffers a program reuses from pair to pair once (hipHostRegister underneath: the cost of a
 * registration is that of pinning the pages, paid once); eppm_host_alloc returns pinned memory that counts as registered.
 * eppm_set_images returns when the images have been read (set_data is a synchronous cudaMemcpy in the reference,
 * driver .cpp:165-166).  Registrations are counted: registering a block (or a range inside a registered block) again adds an owner,
 * eppm_host_unregister removes one, and the pages are unpinned when the last owner unregisters -- after the transfers other contexts
 * have in flight on the block completed (an unregister under one's own pending eppm_compute_begin_into fails with EPPM_ERR_STATE
 * after a bounded wait instead of deadlocking).  Thread-safe. */
int  eppm_host_register(void* p, size_t bytes);
int  eppm_host_unregister(void* p);
int  eppm_host_is_registered(const void* p, size_t bytes);   /* 1 / 0 */
int  eppm_host_alloc(void** p, size_t bytes);
int  eppm_host_free(void* p);

/* Device-resident RGBA (uchar4, alpha ignored/0) images, pitch in bytes: copies them into the context (device to device,
 * in the order of the context's stream) and runs prepare.  The planes must be complete before the call (or produced on
 * that stream) and stay valid until that copy has run (eppm_synchronize, or any later synchronous call on this
 * context); they are never read in place by a kernel. */
int  eppm_set_images_device(eppm_ctx* ctx, const void* d_rgba1, const void* d_rgba2, size_t pitch);

/* ----------------------------------------------------------------------------------------
 * batches of independent pairs of one size (BASELINE.json configs[2]: many pairs per GPU; SURVEY 7 "batch dimension
 * in the kernel grid").  A batch context holds `npairs` pairs; every kernel launch of the path covers all active pairs
 * (the quarter-resolution stages of ONE pair cannot fill 256 CUs, those of 8 pairs can).  Each pair's result is
 * bit-identical to what a single-pair context computes for it.  The single-pair calls above and below work on a batch
 * context too (they address pair 0 and make it the only active pair).
 * -------------------------------------------------------------------------------------- */
int  eppm_create_batch(eppm_ctx** out, int h, int w, int device, const eppm_params* params, int npairs);
int  eppm_batch_size(const eppm_ctx* ctx);
/* set_data for pairs 0..n-1 (n <= npairs; n becomes the number of active pairs): arrays of n host RGB image pointers */
int  eppm_batch_set_images(eppm_ctx* ctx, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride);
/* the same from device-resident RGBA planes (arrays of n device pointers); copied in stream order, never read in place */
int  eppm_batch_set_images_device(eppm_ctx* ctx, int n, const void* const* d_rgba1, const void* const* d_rgba2, size_t pitch);
/* compute_flow for every active pair.  u[k], v[k]: h*w floats of pair k (host); synchronous */
int  eppm_batch_compute(eppm_ctx* ctx, float* const* u, float* const* v);
/* asynchronous; d_flows: NULL, or n device pointers (NULL entries allowed) receiving the interleaved float2 flows */
int  eppm_batch_compute_device(eppm_ctx* ctx, void* const* d_flows);
/* second half of eppm_compute_begin / eppm_batch_compute_begin_into for every active pair */
int  eppm_batch_compute_end(eppm_ctx* ctx, float* const* u, float* const* v);
/* eppm_compute_begin_into for every active pair */
int  eppm_batch_compute_begin_into(eppm_ctx* ctx, float* const* u, float* const* v);
/* eppm_get_plane of pair `pair` */
int  eppm_batch_get_plane(eppm_ctx* ctx, int pair, const char* name, int level, void* dst, size_t dst_bytes);

/* compute_flow (driver .cpp:217-306).  u, v: h*w floats each (host). Synchronous. */
int  eppm_compute(eppm_ctx* ctx, float* u, float* v);
/* The same in two halves, for a host thread that keeps several contexts in flight (PCIe copies of one pair overlap
 * the kernels of another): begin enqueues the path and the device-to-host copy and returns at once; end waits for
 * this context's stream and writes u, v.  eppm_set_images on a context does NOT drain its stream: the staging buffers are
 * double-buffered with an event each, images in registered memory are read by DMA and the call returns once that DMA is done; u, v
 * handed to eppm_compute_begin_into must stay allocated until eppm_compute_end has returned. */
int  eppm_compute_begin(eppm_ctx* ctx);
int  eppm_compute_end(eppm_ctx* ctx, float* u, float* v);
/* eppm_compute_begin with the destination named up front: planes in registered memory (eppm_host_register) are written by the
 * copy engine directly and eppm_compute_end(ctx, u, v) with the same pointers only waits.  eppm_compute = this + eppm_compute_end. */
int  eppm_compute_begin_into(eppm_ctx* ctx, float* u, float* v);
/* Optional colour-coded flow of the last eppm_compute* (compute_flow's color_flow argument, driver .cpp:308-314):
 * Middlebury colour wheel on the device flow (basic/bao_basic_cuda.cuh:776-845), h rows of w R,G,B triplets,
 * row_stride bytes apart.  The reference calls it with max_disp (20,20).  On a batch context: pair 0. */
int  eppm_compute_color(eppm_ctx* ctx, uint8_t* rgb, size_t row_stride, float max_disp_x, float max_disp_y);
/* Same, asynchronous on the context's stream; the interleaved float2 flow stays in HBM.
 * d_flow may be NULL (result kept in the context; fetch with eppm_get_plane("flow",0)). */
int  eppm_compute_device(eppm_ctx* ctx, void* d_flow);
int  eppm_synchronize(eppm_ctx* ctx);

/* Geometry of the pyramid (bao_pyr_init_dim, basic/bao_basic.h:196-211). */
int  eppm_num_levels(const eppm_ctx* ctx);
int  eppm_level_dims(const eppm_ctx* ctx, int level, int* h, int* w);

/* Copy an internal plane to the host, tightly packed (row = w elements).  Names:
 *  "img1","img2" (uchar4), "census1","census2" (u8), "nnf1","nnf2" (short2), "cost1","cost2" (f32),
 *  "flow" (float2).  Valid after the stage that produces it has run.
 *  After a bidirectional call (below) also: "flow_bwd" (float2, every level: the backward flow as that level left it), "occ1", "occ2"
 *  (u8, level 0: the occlusion masks), and "nnf2" at the PatchMatch level is the backward NNF after hole filling.  A later
 *  forward-only compute invalidates "flow_bwd", "occ1" and "occ2" (EPPM_ERR_STATE).
 *  After a compute that started from a temporal prior (below; EPPM_ERR_STATE otherwise), at the PatchMatch level: "prior1", "prior2" (short2:
 *  the advected targets of the forward / backward problem), "nnf_init1", "nnf_init2" (short2) and "cost_init1", "cost_init2" (f32): the
 *  field and its costs as the iterations found them. */
int  eppm_get_plane(eppm_ctx* ctx, const char* name, int level, void* dst, size_t dst_bytes);

/* ----------------------------------------------------------------------------------------
 * bidirectional flow with forward-backward occlusion masks.  Opt-in: a context that never makes one of these
 * calls allocates and launches exactly what it did without them.  The first call on a context allocates its backward planes (npairs
 * of them on a batch context); eppm_destroy frees them.
 *  forward (u, v): bit-identical to eppm_compute's.
 *  backward (bu, bv): image 2 -> image 1, from the backward NNF the coarsest level's PatchMatch computes anyway (the reference's
 *    commented-out branch, driver .cpp:243-245, completed symmetrically): outlier removal, weighted median, hole filling and every
 *    coarse-to-fine level guided by image 2.  NOT the forward flow of the swapped pair (that would draw other random numbers).
 *  occ1 / occ2: h*w bytes each, for image 1's / image 2's pixels: 0 consistent, 1 inconsistent (|F + G(x + F)|^2 > alpha (|F|^2 +
 *    |G|^2) + beta, G bilinear, or a tap of G unknown), 2 the vector leaves the frame, 3 the vector is unknown (|component| > 1e9, NaN).
 * The pipelined eppm_compute_begin / eppm_compute_end forms have no bidirectional counterpart.
 * -------------------------------------------------------------------------------------- */
/* forward-backward: u,v forward (== eppm_compute), bu,bv backward, occ1/occ2 h*w bytes (codes 0..3 above); any of bu,bv,occ1,occ2 may be NULL.
 * Synchronous. */
int  eppm_compute_bidirectional(eppm_ctx* ctx, float* u, float* v, float* bu, float* bv, uint8_t* occ1, uint8_t* occ2);
/* asynchronous; interleaved float2 flows and h*w-byte masks of pair 0 into device memory; NULLs allowed (results stay in the context:
 * eppm_get_plane) */
int  eppm_compute_bidirectional_device(eppm_ctx* ctx, void* d_flow, void* d_flow_bwd, void* d_occ1, void* d_occ2);
/* every active pair; u, v: n plane pointers (required); bu, bv, occ1, occ2: NULL or n pointers (NULL entries allowed).  Synchronous. */
int  eppm_batch_compute_bidirectional(eppm_ctx* ctx, float* const* u, float* const* v, float* const* bu, float* const* bv,
                                      uint8_t* const* occ1, uint8_t* const* occ2);
/* alpha, beta of the masks' criterion (defaults 0.01, 0.5: Sundaram, Brox & Keutzer, ECCV 2010); both finite, >= 0 */
int  eppm_set_occlusion_params(eppm_ctx* ctx, float alpha, float beta);
/* ----------------------------------------------------------------------------------------
 * draft mode: the stop level s of a context, single or batch, 0 <= s <= eppm_num_levels - 1, default 0 = the full
 * path.  With s > 0 the levels eppm_num_levels - 1 .. s run as always (flow[s] is the full path's flow[s], bit for bit), and every level
 * l < s is ONE launch instead of resize + candidate refine + smoothing: flow[l] = the flow smoothing, guided by level l's image, of the
 * doubled and 2x-replicated flow[l + 1] (eppm_flow_upsample); no final smoothing follows.  The backward branch of the bidirectional
 * calls does the same with image 2 as the guide, and the masks, the interpolation, the tracker and the streaming calls work on the
 * draft flows unchanged.  No memory is added.  Takes effect at the next compute; the flows of the last compute stop being valid for
 * eppm_interpolate* / eppm_track_step (EPPM_ERR_STATE until the next compute).  EPPM_ERR_ARG outside 0 .. eppm_num_levels - 1;
 * EPPM_ERR_STATE, and nothing changes, while an eppm_compute_begin is pending.  Stage
 * names: "flow_jbu_L<l>", "flow_jbu_bwd_L<l>".
 * -------------------------------------------------------------------------------------- */
int  eppm_set_stop_level(eppm_ctx* ctx, int level);
int  eppm_stop_level(const eppm_ctx* ctx);           /* -1: NULL context */
/* the kernel alone on unpitched device planes (like eppm_flow_to_color): d_occ h*w bytes for F = d_flow, G = d_other (h*w float2
 * each); on the launcher stream, synchronous like the other launchers */
int  eppm_fb_occlusion(uint8_t* d_occ, const eppm_float2* d_flow, const eppm_float2* d_other, int h, int w, float alpha, float beta);

/* ----------------------------------------------------------------------------------------
 * frame interpolation.  The frame at time t between image 1 (t = 0) and image 2 (t = 1) from the forward flow and
 * the two occlusion masks of the last bidirectional call (Baker et al., IJCV 2011, section 3.3, made deterministic): splat the forward
 * flow to time t (consistent vectors first, then the lowest photo cost, then the lowest source index), fill the holes, sample both frames
 * along the splatted vector and let the masks choose which frame(s) to trust.  t = 0 / t = 1 return the input frames byte for byte; any
 * other t must lie in (0, 1) (else EPPM_ERR_ARG, NaN included).  The context forms are valid after eppm_compute_bidirectional* and until the
 * next eppm_set_images* or forward-only compute (EPPM_ERR_STATE outside that window); they read the images, the forward flow and the masks
 * where the context keeps them.  The first call allocates the context's interpolation scratch (kept until eppm_destroy); times are
 * processed four per launch.  Outputs: h rows of w R,G,B triplets row_stride bytes apart (host), or RGBA words with alpha 255 (device).
 * -------------------------------------------------------------------------------------- */
/* pair 0; rgb: nt host images, one per time t[k].  Synchronous. */
int  eppm_interpolate(eppm_ctx* ctx, int nt, const float* t, uint8_t* const* rgb, size_t row_stride);
/* pair 0; d_rgba: nt device RGBA planes of `pitch` bytes per row.  Asynchronous on the context's stream (no host synchronisation, no
 * allocation after the first call: usable inside stream capture). */
int  eppm_interpolate_device(eppm_ctx* ctx, int nt, const float* t, void* const* d_rgba, size_t pitch);
/* every active pair: rgb[pair * nt + k] receives pair `pair` at time t[k].  Synchronous. */
int  eppm_batch_interpolate(eppm_ctx* ctx, int nt, const float* t, uint8_t* const* rgb, size_t row_stride);
/* the kernels alone on caller planes: RGBA inputs (in_pitch bytes per row, alpha ignored) and output (out_pitch), h*w float2 forward flow,
 * h*w-byte masks, all device pointers; on the launcher stream, synchronous like eppm_fb_occlusion */
int  eppm_interpolate_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba1, const void* d_rgba2, size_t in_pitch,
                             const eppm_float2* d_flow, const uint8_t* d_occ1, const uint8_t* d_occ2, int h, int w, float t);
/* host form on packed RGB images and planar flows: byte-identical to the kernels */
int  eppm_interpolate_host(uint8_t* rgb_out, const uint8_t* rgb1, const uint8_t* rgb2, const float* u, const float* v, const uint8_t* occ1,
                           const uint8_t* occ2, int h, int w, float t);

/* ----------------------------------------------------------------------------------------
 * synthetic shutter: motion blur of a frame along its flow (a depth-free form of the tile-dominant reconstruction
 * filter of McGuire et al., I3D 2012).  The frame as a camera whose shutter stays open for `shutter` of the frame interval, centred on the
 * frame, would have recorded it: every pixel averages 2*taps + 1 single-pixel taps along the longest half-vector (0.5 * shutter * flow,
 * clamped to max_radius) of the up to 3x3 tiles of 32x32 pixels around its own; a tap counts when the pixel there sweeps over the output
 * pixel or the output pixel's own motion sweeps over it, and every other tap counts as the output pixel itself.  A uniform motion gives
 * the box filter along it; where the longest half-vector is below half a pixel (static regions; unknown or NaN flow counts as zero) the
 * frame comes back byte for byte.  Every weight is 0 or 1 and every sum an integer: the kernels, the host form and both libraries give
 * the same bytes.  The context forms read the raw frame and the level-0 flow where the context keeps them and change no plane of it:
 *   frame 0: image 1 along the forward flow, valid after ANY compute of the current images (forward-only included) and until the next
 *            eppm_set_images* / eppm_push_image*;
 *   frame 1: image 2 along the backward flow, valid in the window of eppm_interpolate*.
 * EPPM_ERR_STATE outside these windows; EPPM_ERR_ARG for parameters out of range (NaN included).  params NULL: the defaults.  The first
 * call allocates the context's motion-blur scratch (about 7 bytes per pixel and pair, kept until eppm_destroy).  Outputs: h rows of w
 * R,G,B triplets row_stride bytes apart (host), or RGBA words with alpha 255 (device).  Stage names: "mblur_pack", "mblur_gather".
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_mblur_params {
    float shutter;               /* open fraction of the frame interval, 0 < shutter <= 1 (0.5) */
    float max_radius;            /* longest half-vector in pixels, 1 .. 31 (16) */
    int   taps;                  /* taps to each side of the pixel, 1 .. 32 (8): the filter reads 2*taps + 1 */
} eppm_mblur_params;
int  eppm_mblur_default_params(eppm_mblur_params* p);
/* pair 0; rgb: one host image.  Synchronous. */
int  eppm_motion_blur(eppm_ctx* ctx, const eppm_mblur_params* params, int frame, uint8_t* rgb, size_t row_stride);
/* pair 0; d_rgba: a device RGBA plane of `pitch` bytes per row.  Asynchronous on the context's stream (no host synchronisation, no
 * allocation after the first call: usable inside stream capture). */
int  eppm_motion_blur_device(eppm_ctx* ctx, const eppm_mblur_params* params, int frame, void* d_rgba, size_t pitch);
/* every active pair: rgb[pair] receives pair `pair`.  Synchronous. */
int  eppm_batch_motion_blur(eppm_ctx* ctx, const eppm_mblur_params* params, int frame, uint8_t* const* rgb, size_t row_stride);
/* the kernels alone on caller planes, any size from 1x1 up to 8192x8192 and 2^26 pixels: RGBA input (in_pitch bytes per row, alpha
 * ignored) and output (out_pitch), h*w float2 flow, all device pointers; on the launcher stream, synchronous */
int  eppm_motion_blur_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba, size_t in_pitch, const eppm_float2* d_flow,
                             int h, int w, const eppm_mblur_params* params);
/* host form on a packed RGB image and a planar flow (no GPU needed): byte-identical to the kernels */
int  eppm_motion_blur_host(uint8_t* rgb_out, const uint8_t* rgb, const float* u, const float* v, int h, int w, const eppm_mblur_params* params);

/* ----------------------------------------------------------------------------------------
 * dense point trajectories (Sundaram, Brox & Keutzer, ECCV 2010).  Points seeded on a grid of spacing x spacing
 * cells, where the 5x5 structure tensor of R+G+B has lambda_min >= min_eig (exact integers), move by the bilinearly sampled forward flow;
 * a track ends where the forward flow is unknown (reason 1), where it leaves the frame (2), where the forward-backward check fails (3) or
 * at a motion boundary (4); every uncovered textured cell of the new frame is seeded again.  One step advances a tracker by one pair.
 * A tracker is a separate allocation on its context's device (the context's own allocations do not change).  Tracks are ordered:
 * survivors keep their order, new seeds follow in cell order with consecutive ids; seeds past the capacity are dropped (the highest
 * cells first).  The kernels, the host form and any two runs give the same bytes.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_track_params {
    int     spacing;             /* cell side in pixels, >= 1 (8) */
    int64_t min_eig;             /* texture threshold on lambda_min of the integer structure tensor, 0 .. 2^40 (2500) */
    float   fb_alpha, fb_beta;   /* forward-backward check, as the occlusion masks' (0.01, 0.5) */
    float   mb_alpha, mb_beta;   /* motion boundary: |grad u|^2 + |grad v|^2 > mb_alpha |w|^2 + mb_beta ends a track (0.01, 0.002) */
    int     capacity;            /* track slots, <= 2^26; 0: 4 x the number of cells */
} eppm_track_params;
typedef struct {
    int live;                    /* live tracks (positions in the current frame) */
    int ended, seeded, dropped;  /* of the last step */
    int frame;                   /* the current frame: steps since frame 0 */
    int next_id;                 /* the id of the next seed */
} eppm_track_counts;
typedef struct eppm_tracker eppm_tracker;

int  eppm_track_default_params(eppm_track_params* p);
/* the capacity a tracker of these parameters has on an h x w frame (-1: bad parameters) */
int  eppm_track_capacity(const eppm_track_params* p, int h, int w);
/* p NULL: the defaults.  Frame 0, no track, next id 0. */
int  eppm_tracker_create(eppm_ctx* ctx, const eppm_track_params* p, eppm_tracker** out);
int  eppm_tracker_destroy(eppm_tracker* t);
/* one step on pair `pair` of the context (images, forward and backward flow of its last bidirectional call); valid in the window of
 * eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions or another device, or a pair that is not
 * active.  At frame 0 with no live track the step first seeds image 1.  Asynchronous on the context's stream: no host synchronisation,
 * no allocation.  Consecutive pairs of one batch context stepped 0, 1, ... with one tracker chain them. */
int  eppm_track_step(eppm_tracker* t, eppm_ctx* ctx, int pair);
/* the same kernels on caller planes: RGBA images (pitch bytes per row, alpha ignored), h*w float2 forward and backward flows, all device
 * pointers of the tracker's size; on the launcher stream, synchronous */
int  eppm_track_step_frames(eppm_tracker* t, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow,
                            const eppm_float2* d_flow_bwd, int h, int w);
/* synchronous.  The first min(live, max) live tracks: ids, start frames, positions (x, y pairs) in the current frame; any array may be
 * NULL; counts: NULL or the counters */
int  eppm_tracker_get(eppm_tracker* t, int max, int32_t* ids, int32_t* starts, float* xy, eppm_track_counts* counts);
/* synchronous.  The last step's first min(ended, max) ended tracks: ids, start frames, last positions (in the frame before the step),
 * reasons 1..4 */
int  eppm_tracker_get_ended(eppm_tracker* t, int max, int32_t* ids, int32_t* starts, float* xy, int32_t* reasons, eppm_track_counts* counts);
/* synchronous.  Load a state: n <= capacity tracks at finite positions inside the frame, the next id (>= 0) and the frame (>= 0);
 * the last step's counts become 0 */
int  eppm_tracker_set(eppm_tracker* t, int n, const int32_t* ids, const int32_t* starts, const float* xy, int next_id, int frame);
/* host form of one step on packed RGB images and planar flows (u, v forward; bu, bv backward): sequential loops, byte-identical to the
 * kernels.  In: n tracks (ids, starts, xy), next_id, frame.  Out: arrays of eppm_track_capacity entries (xy: twice that); counts */
int  eppm_track_step_host(const eppm_track_params* p, const uint8_t* rgb1, const uint8_t* rgb2, const float* u, const float* v, const float* bu,
                          const float* bv, int h, int w, int n, const int32_t* ids, const int32_t* starts, const float* xy, int next_id, int frame,
                          int32_t* out_ids, int32_t* out_starts, float* out_xy, int32_t* end_ids, int32_t* end_starts, float* end_xy,
                          int32_t* end_reasons, eppm_track_counts* counts);
/* the seeds of the textured cells of a packed RGB image in cell order: *n of them, the first min(*n, max) written to xy */
int  eppm_track_seeds_host(const eppm_track_params* p, const uint8_t* rgb, int h, int w, int max, float* xy, int* n);

/* ----------------------------------------------------------------------------------------
 * streaming video: one single-pair context walks a clip.  Opt-in: a context that never calls these allocates and
 * launches exactly what it did without them.
 *  frame push: image 2 becomes image 1 and the new frame becomes image 2.  The raw frame, the pyramid, the census and the texel planes of
 *    the old image 2 are kept (the context exchanges its plane pointers); only the new frame is uploaded and prepared.  After
 *    eppm_set_images(A, B), eppm_push_image(C) every plane and every flow equals those after eppm_set_images(B, C), bit for bit.
 *    EPPM_ERR_STATE before the first eppm_set_images*; EPPM_ERR_ARG on a batch context (its pairs run concurrently: there is no previous pair).
 *  temporal mode: every compute keeps two level-L displacement fields (L = the PatchMatch level; an allocation of its own, made by the first
 *    compute with the mode on): the forward field that is converted to the level's flow, and the raw backward NNF.  The next compute moves
 *    each along its own motion (a pixel with displacement d lands on p + d -- p - d for the backward field -- and keeps d; of several
 *    sources the smallest index wins) and starts PatchMatch from that prior wherever its cost is strictly lower than the random match's;
 *    the random field, the random search's numbers and the iterations are those of a cold run.  The prior is armed by eppm_push_image*
 *    directly after a compute: a second compute on the same pair, or a compute after two pushes in a row, is a cold run.  eppm_set_images*
 *    drops the fields (a new pair is a new clip), eppm_temporal_reset drops them by hand; a cold run is bit for bit eppm_compute's.  Works with eppm_compute*, eppm_compute_bidirectional* and therefore eppm_track_step.  EPPM_ERR_ARG on a batch
 *    context.
 * -------------------------------------------------------------------------------------- */
int  eppm_push_image(eppm_ctx* ctx, const uint8_t* rgb, size_t row_stride);
/* device-resident RGBA frame, as eppm_set_images_device's */
int  eppm_push_image_device(eppm_ctx* ctx, const void* d_rgba, size_t pitch);
int  eppm_set_temporal(eppm_ctx* ctx, int on);      /* off (default) also drops the fields */
int  eppm_temporal_reset(eppm_ctx* ctx);            /* the next compute is cold */
int  eppm_temporal_valid(const eppm_ctx* ctx);      /* 1: the next compute will start from a prior; 0 otherwise */
/* The advection rule on host memory (no GPU needed).  prev: h*w displacements (a component <= -10000: unknown vector); prior: h*w absolute
 * targets as an NNF holds them, (-10000, -10000) where a pixel has no prior; backward != 0: the step's sign is flipped (q = p - d). */
int  eppm_temporal_prior_host(eppm_short2* prior, const eppm_short2* prev, int h, int w, int backward);
/* the kernels alone on unpitched device planes; on the launcher stream, like eppm_fb_occlusion */
int  eppm_temporal_prior(eppm_short2* d_prior, const eppm_short2* d_prev, int h, int w, int backward);

/* ----------------------------------------------------------------------------------------
 * batch streaming: one clip per slot of a batch context, every slot advanced by one frame per step.  Valid on any
 * context of eppm_create_batch (npairs = 1 included); eppm_push_image* and eppm_set_temporal keep refusing a batch context.  Opt-in like the
 * single-pair calls: a batch context that never calls these allocates and launches exactly what it did without them.
 *  push: n must equal the number of active pairs (EPPM_ERR_ARG).  Slot k's image 2 becomes its image 1 and rgb[k] its image 2; only the new
 *    frames are uploaded and prepared.  After eppm_batch_set_images(A_k, B_k), eppm_batch_push_images(C_k) every plane and every flow of
 *    slot k equals those after eppm_batch_set_images(B_k, C_k), bit for bit.  EPPM_ERR_STATE before the first eppm_batch_set_images*, or
 *    while an eppm_compute_begin* is pending.  The host form returns when the caller may reuse the images.
 *  new_clip: NULL, or n bytes; non-zero: the frame pushed into slot k is the first frame of another clip.  The pair the slot now holds
 *    (the old clip's last frame, the new clip's first) is computed like any other -- every launch covers every slot; its flow is the
 *    caller's to discard -- but neither starts from a prior nor leaves one: the pair across the cut and the new clip's first pair are cold
 *    runs, its second pair is seeded.
 *  temporal mode, per slot k:   compute: seeded[k] = valid[k], snap[k] = !cut[k], valid[k] = 0
 *                               push:    valid[k] = snap[k] && !new_clip[k], snap[k] = 0, cut[k] = new_clip[k]
 *    eppm_batch_set_images* drops every slot's fields, eppm_batch_temporal_reset(k) those of slot k (k < 0: of every slot).  A slot that is
 *    not seeded gets the cold run's bits whatever its neighbours do: its flows are eppm_batch_compute's.  The temporal planes are npairs
 *    blocks of 40 bytes per PatchMatch-level pixel (each plane rounded up to 256 bytes), allocated by the first compute with the mode on.
 *    Works with eppm_batch_compute, _compute_device, _compute_begin_into / _end, _compute_bidirectional and eppm_track_step(t, ctx, pair).
 *    eppm_batch_get_plane(ctx, k, "prior1" ...) is valid for a slot whose last compute was seeded (EPPM_ERR_STATE otherwise).
 * -------------------------------------------------------------------------------------- */
int  eppm_batch_set_temporal(eppm_ctx* ctx, int on);          /* off (default) also drops every slot's fields */
int  eppm_batch_push_images(eppm_ctx* ctx, int n, const uint8_t* const* rgb, size_t row_stride, const uint8_t* new_clip);
/* device-resident RGBA frames, as eppm_batch_set_images_device's */
int  eppm_batch_push_images_device(eppm_ctx* ctx, int n, const void* const* d_rgba, size_t pitch, const uint8_t* new_clip);
int  eppm_batch_temporal_valid(const eppm_ctx* ctx, int pair);    /* 1: the slot's next compute will start from a prior; 0 otherwise */
int  eppm_batch_temporal_reset(eppm_ctx* ctx, int pair);          /* the slot's next compute is cold; pair < 0: every slot's */
/* the advection kernels alone on caller planes: npairs slots of h*w short2 each, both planes unpitched and slot after slot, one splat and
 * one gather launch for all of them; armed: NULL (all) or npairs bytes (host memory), an unarmed slot gets "no prior" everywhere */
int  eppm_temporal_prior_batch(eppm_short2* d_prior, const eppm_short2* d_prev, int h, int w, int backward, int npairs, const uint8_t* armed);

/* ----------------------------------------------------------------------------------------
 * motion-compensated temporal denoising: a recursive filter that averages every pixel of a streamed clip along its
 * own trajectory.  A filter holds one slot per pair of its context: per pixel the running mean {R, G, B} and the count n of the frames in
 * it (h*w float4, row-major).  One step moves every covered slot from image 1 to image 2 of its pair: a pixel whose backward vector is
 * known, stays inside the frame and is not occluded (occ2 == 0) samples the previous state bilinearly at its source, and if the sample is
 * within thresh of the new pixel (sum of the three absolute differences) blends the new pixel in with weight 1 / n, n = min(n_prev + 1,
 * n_max); every other pixel starts again from the new frame with n = 1.  The kernel equals eppm_tfilter_step_host bit for bit, in both
 * libraries.  A filter is a separate allocation on its context's device (36 bytes per pixel and slot: two states and the RGBA output), made
 * by eppm_tfilter_create and freed by eppm_tfilter_destroy; a context that never creates one allocates and launches exactly what it did
 * without.  A slot that has never been stepped, or after eppm_tfilter_reset, is empty: its first step reads the seed of image 1
 * ({R, G, B, 1}) as the previous state.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_tfilter_params {
    float thresh;                /* largest |dR| + |dG| + |dB| between the new pixel and the compensated mean that still blends (40); finite, >= 0 */
    int   n_max;                 /* the longest average, 1 .. 255 (8) */
} eppm_tfilter_params;
typedef struct eppm_tfilter eppm_tfilter;

int  eppm_tfilter_default_params(eppm_tfilter_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty. */
int  eppm_tfilter_create(eppm_ctx* ctx, const eppm_tfilter_params* p, eppm_tfilter** out);
/* a filter without a context, for eppm_tfilter_step_frames on caller planes: nslots slots of h x w pixels (any size from 1 x 1) on `device` */
int  eppm_tfilter_create_size(int h, int w, int nslots, int device, const eppm_tfilter_params* p, eppm_tfilter** out);
int  eppm_tfilter_destroy(eppm_tfilter* f);                 /* NULL is fine */
int  eppm_tfilter_reset(eppm_tfilter* f, int slot);         /* the slot is empty again; slot < 0: every slot */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames, the level-0 backward flow
 * and occ2): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions, another
 * device or more active pairs than the filter has slots.  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair is the
 * first frame of another clip, the slot's state becomes its seed.  A slot the step does not cover keeps its state.  One launch,
 * asynchronous on the context's stream: no copy, no allocation, no host synchronisation. */
int  eppm_tfilter_step(eppm_tfilter* f, eppm_ctx* ctx, const uint8_t* cut);
/* the same step of one slot on caller device planes of the filter's size (RGBA images of `pitch` bytes per row, h*w float2 backward flow,
 * h*w mask bytes); on the launcher stream, synchronous.  d_rgba1 is read only if the slot is empty.  Whatever the planes hold, nothing
 * outside them is read. */
int  eppm_tfilter_step_frames(eppm_tfilter* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                              const uint8_t* d_occ2, int cut);
/* the slot's filtered frame (EPPM_ERR_STATE on an empty slot): packed RGB to the host, synchronous ... */
int  eppm_tfilter_get(eppm_tfilter* f, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the filter's last step */
int  eppm_tfilter_get_device(eppm_tfilter* f, int slot, void* d_rgba, size_t pitch);
/* synchronous.  The slot's state, h*w*4 floats {R, G, B, n} (EPPM_ERR_STATE on an empty slot) / load one: the slot is no longer empty */
int  eppm_tfilter_get_state(eppm_tfilter* f, int slot, float* acc);
int  eppm_tfilter_set_state(eppm_tfilter* f, int slot, const float* acc);
/* host forms (no GPU needed): the seed of a packed RGB frame, and one step from acc_in (image 1's state) to acc_out and the packed RGB
 * output rgb_out; rgb2: image 2, (bu, bv): the backward flow, occ2: the mask.  acc_out must not be acc_in.  The step of an empty slot is
 * eppm_tfilter_seed_host(image 1) followed by this. */
int  eppm_tfilter_seed_host(float* acc, const uint8_t* rgb, int h, int w);
int  eppm_tfilter_step_host(const eppm_tfilter_params* p, float* acc_out, uint8_t* rgb_out, const float* acc_in, const uint8_t* rgb2,
                            const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int cut);

/* ----------------------------------------------------------------------------------------
 * flicker removal: frame-to-frame brightness fluctuation that varies slowly over the picture (archive film,
 * timelapse, mains lighting) is modelled as a gain and an offset per colour on a grid of cell x cell pixels.  A step runs on a pair and
 * corrects IMAGE 2 towards the slot's reference, the previous step's corrected output (image 1 while the slot is empty).  A pixel whose
 * backward vector is known, stays inside the frame and is not occluded (occ2 == 0) samples the reference bilinearly (p); it is a member of
 * pass 0 if |v - p| summed over the colours is within `reject`, and of a later pass if the previous pass's field brings v within `tau` of
 * p.  Per cell and colour the members' exact integer sums give the regression a = (cov + 64 N^2) / (var + 64 N^2) clamped to [0.5, 2] and
 * b = (sum p - a sum v) / N in float64; a cell with fewer than n_min members is invalid.  The field is the (1, 2, 1) x (1, 2, 1) average
 * over the valid cells of each 3 x 3 neighbourhood (none: gain 1, offset 0), read bilinearly between cell centres; the output is
 * (1 + keep (a - 1)) v + keep b, rounded and clamped, and becomes the slot's next reference.  A cut step returns image 2 itself.  The
 * kernels equal eppm_deflicker_step_host bit for bit, in both libraries.  A deflicker object is a separate allocation on its context's
 * device (8 bytes per pixel and 77 per cell, per slot); a context that never creates one allocates and launches exactly what it did without.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_deflicker_params {
    int   cell;                  /* the grid's cell, 16, 32 or 64 pixels (32) */
    int   iters;                 /* passes, 1 .. 4 (2) */
    float reject;                /* pass 0: largest |dR| + |dG| + |dB| between the new pixel and its sample (60); finite, >= 0 */
    float tau;                   /* later passes: the same after the previous pass's correction (12); finite, >= 0 */
    float keep;                  /* how much of the correction is applied, 0 .. 1 (1) */
    int   n_min;                 /* a cell needs this many members, >= 1 (32) */
} eppm_deflicker_params;
typedef struct eppm_deflicker_stats {
    int64_t used;                /* members of the last pass */
    int32_t valid_cells;         /* cells with at least n_min of them */
    int32_t cells;               /* cells of the grid */
} eppm_deflicker_stats;
typedef struct eppm_deflicker eppm_deflicker;

int  eppm_deflicker_default_params(eppm_deflicker_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty. */
int  eppm_deflicker_create(eppm_ctx* ctx, const eppm_deflicker_params* p, eppm_deflicker** out);
/* an object without a context, for eppm_deflicker_step_frames on caller planes: nslots slots of h x w pixels (any size from 1 x 1) */
int  eppm_deflicker_create_size(int h, int w, int nslots, int device, const eppm_deflicker_params* p, eppm_deflicker** out);
int  eppm_deflicker_destroy(eppm_deflicker* f);             /* NULL is fine */
int  eppm_deflicker_reset(eppm_deflicker* f, int slot);     /* the slot is empty again; slot < 0: every slot */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames, the level-0 backward flow
 * and occ2): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions, another
 * device or more active pairs than the object has slots.  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair is the
 * first frame of another clip.  A slot the step does not cover keeps its state.  2 iters + 1 launches, asynchronous on the context's
 * stream: no copy, no allocation, no host synchronisation. */
int  eppm_deflicker_step(eppm_deflicker* f, eppm_ctx* ctx, const uint8_t* cut);
/* the same step of one slot on caller device planes of the object's size (RGBA images of `pitch` bytes per row, h*w float2 backward flow,
 * h*w mask bytes); on the launcher stream, synchronous.  d_rgba1 is read only if the slot is empty.  Whatever the planes hold, nothing
 * outside them is read. */
int  eppm_deflicker_step_frames(eppm_deflicker* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch,
                                const eppm_float2* d_flow_bwd, const uint8_t* d_occ2, int cut);
/* the slot's corrected image 2 of the last step (EPPM_ERR_STATE on a slot never stepped): packed RGB to the host, synchronous ... */
int  eppm_deflicker_get(eppm_deflicker* f, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the object's last step */
int  eppm_deflicker_get_device(eppm_deflicker* f, int slot, void* d_rgba, size_t pitch);
/* synchronous (EPPM_ERR_STATE on a slot never stepped): the last step's field on the grid of cells_x = (w + cell - 1) / cell by cells_y =
 * (h + cell - 1) / cell cells, cells_y * cells_x * 6 floats {aR, aG, aB, bR, bG, bB}, and
 * a byte per cell, 1 where the last pass's own model was valid (either may be NULL); the last step's counts */
int  eppm_deflicker_get_field(eppm_deflicker* f, int slot, float* field, uint8_t* valid);
int  eppm_deflicker_get_stats(eppm_deflicker* f, int slot, eppm_deflicker_stats* stats);
/* synchronous.  The slot's reference frame (packed RGB, h*w*3) and whether the slot is empty (EPPM_ERR_STATE on a slot that was never
 * stepped nor loaded) / load them: a later eppm_deflicker_get returns the loaded frame */
int  eppm_deflicker_get_state(eppm_deflicker* f, int slot, uint8_t* rgb, int* empty);
int  eppm_deflicker_set_state(eppm_deflicker* f, int slot, const uint8_t* rgb, int empty);
/* host form (no GPU needed): one step on packed RGB frames; rgb_ref: the reference (image 1 for an empty slot), rgb_cur: image 2,
 * (bu, bv): the backward flow, occ2: the mask.  field_out: cells * 6 floats, valid_out: cells bytes.  rgb_out must not be rgb_ref. */
int  eppm_deflicker_step_host(const eppm_deflicker_params* p, uint8_t* rgb_out, float* field_out, uint8_t* valid_out,
                              eppm_deflicker_stats* stats, const uint8_t* rgb_ref, const uint8_t* rgb_cur, const float* bu, const float* bv,
                              const uint8_t* occ2, int h, int w, int cut);

/* ----------------------------------------------------------------------------------------
 * film-defect removal: dust, dirt, dropouts and sparkle live for one frame, so a defective pixel differs from both
 * of its motion-compensated neighbours in time while those agree with each other.  A step runs on the pair (image 1 = F_k, image 2 =
 * F_k+1) and repairs IMAGE 1: its next side is image 2 through the level-0 forward flow, its previous side is F_k-1 through the backward
 * flow of the step before, both of which every step saves per slot (a copy of image 1 and of the backward plane).  Per pixel: p and n are
 * the bilinear samples of the previous and the next frame; with d(a, b) = |dR| + |dG| + |dB| the pixel is DECIDED if both samples exist
 * and d(p, n) <= agree, and a HIT if also d(cur, p) > detect and d(cur, n) > detect.  A pixel its own two vectors do not decide gets a
 * second chance with the component-wise lower median of the vectors of its (2 radius + 1)^2 window (coordinates clamped; a window that
 * holds an unknown vector has no median); a pixel neither chance decides is never touched.  A decided pixel within `grow` pixels of a hit
 * is GROWN.  Hit and grown pixels become the rounded mean of p and n; every other pixel keeps image 1's colour.  The first and the last
 * frame of a clip are never repaired (they have one neighbour only), nor is the frame before or after a cut.  The kernels equal
 * eppm_defect_step_host bit for bit, in both libraries.  A defect filter is a separate allocation on its context's device (34 bytes per
 * pixel and slot), made by eppm_defect_create and freed by eppm_defect_destroy; a context that never creates one allocates and launches
 * exactly what it did without.  A slot has_prev if its saved planes belong to the frame before image 1: a step DETECTS if has_prev and
 * the pair is not cut, otherwise it PASSES (the output is image 1, the mask and the stats are zero); after either has_prev = !cut.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_defect_params {
    float detect;                /* a hit differs from both neighbours by more than this |dR| + |dG| + |dB| (60); finite, >= 0 */
    float agree;                 /* the two neighbours differ by at most this (30); finite, >= 0 */
    int   radius;                /* the median window of the second chance, 0 .. 4 (3); 0: no second chance */
    int   grow;                  /* hits are grown by this many pixels, 0 .. 4 (1) */
} eppm_defect_params;
typedef struct eppm_defect_stats {
    int hit;                     /* pixels with mask 1 */
    int grown;                   /* pixels with mask 2 */
    int second_chance;           /* pixels decided by the median vectors */
    int undecided;               /* pixels decided by neither chance */
} eppm_defect_stats;
typedef struct eppm_defect eppm_defect;

int  eppm_defect_default_params(eppm_defect_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; no slot has_prev. */
int  eppm_defect_create(eppm_ctx* ctx, const eppm_defect_params* p, eppm_defect** out);
/* a defect filter without a context, for eppm_defect_step_frames on caller planes: nslots slots of h x w pixels (any size from 1 x 1) */
int  eppm_defect_create_size(int h, int w, int nslots, int device, const eppm_defect_params* p, eppm_defect** out);
int  eppm_defect_destroy(eppm_defect* f);                  /* NULL is fine */
int  eppm_defect_reset(eppm_defect* f, int slot);          /* the slot's next step passes; slot < 0: every slot's */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames and both level-0 flows):
 * valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions, another device or
 * more active pairs than the filter has slots.  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair is the first frame
 * of another clip.  A slot the step does not cover keeps its state.  Two launches, asynchronous on the context's stream: no copy, no
 * allocation, no host synchronisation. */
int  eppm_defect_step(eppm_defect* f, eppm_ctx* ctx, const uint8_t* cut);
/* the same step of one slot on caller device planes of the filter's size (RGBA images of `pitch` bytes per row, h*w float2 forward and
 * backward flow); on the launcher stream, synchronous.  Whatever the planes hold, nothing outside them is read. */
int  eppm_defect_step_frames(eppm_defect* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow,
                             const eppm_float2* d_flow_bwd, int cut);
/* the slot's repaired image 1 of the last step (EPPM_ERR_STATE on a slot never stepped): packed RGB to the host, synchronous ... */
int  eppm_defect_get(eppm_defect* f, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the filter's last step */
int  eppm_defect_get_device(eppm_defect* f, int slot, void* d_rgba, size_t pitch);
/* synchronous: the last step's mask (h*w bytes: 0 untouched, 1 hit, 2 grown) and counts */
int  eppm_defect_get_mask(eppm_defect* f, int slot, uint8_t* mask);
int  eppm_defect_get_stats(eppm_defect* f, int slot, eppm_defect_stats* stats);
/* synchronous.  The slot's saved frame (packed RGB, h*w*3), saved backward plane (h*w interleaved (x, y) floats) and has_prev
 * (EPPM_ERR_STATE on a slot that holds none) / load them */
int  eppm_defect_get_state(eppm_defect* f, int slot, uint8_t* rgb, float* bwd, int* has_prev);
int  eppm_defect_set_state(eppm_defect* f, int slot, const uint8_t* rgb, const float* bwd, int has_prev);
/* host form (no GPU needed): one step on packed RGB frames; (bu, bv): the vectors from rgb_cur into rgb_prev, (fu, fv): into rgb_next.
 * rgb_prev or rgb_next NULL: the passing step (the flows are not read).  rgb_out must not be rgb_cur. */
int  eppm_defect_step_host(const eppm_defect_params* p, uint8_t* rgb_out, uint8_t* mask_out, eppm_defect_stats* stats, const uint8_t* rgb_prev,
                           const uint8_t* rgb_cur, const uint8_t* rgb_next, const float* bu, const float* bv, const float* fu, const float* fv,
                           int h, int w);

/* ----------------------------------------------------------------------------------------
 * global camera motion and video stabilisation.  One step, after eppm_compute_bidirectional* on a streamed clip's
 * next pair, (a) fits an affine camera motion to the pair's level-0 forward flow by iters passes of least squares on the inliers of the
 * pass before (pixels with occ1 == 0 and a known vector of at most 8192 px; an inlier's residual is at most tau), (b) classifies every
 * pixel of image 1 against the final model (mask bytes: 0 moves with the camera, 1 moves on its own, 2 not valid), (c) appends the model to
 * the slot's camera path C (frame 0 -> current frame), moves the smoothed path S towards it (S = smooth * S + (1 - smooth) * C), and
 * (d) renders image 2 from the smoothed camera: the output pixel (x, y) samples image 2 bilinearly at (C o S^-1)(x, y), {0, 0, 0} where
 * that leaves the frame.  A motion in displacement form is six numbers p: T(x, y) = (x + p0 + p1 X + p2 Y, y + p3 + p4 X + p5 Y) with
 * X = 2x - (w - 1), Y = 2y - (h - 1); a path in (A, t) form is {a00, a01, a10, a11, tx, ty} in coordinates centred on the frame.  The sums of
 * a pass are 64-bit integers (vectors quantised to 1/256 px), so the kernels equal the host forms bit for bit, in both libraries and on
 * every run.  A stabiliser is a separate allocation on its context's device (per slot 5 bytes per pixel -- the RGBA output and the mask --,
 * 128 bytes per tile of 64 x 16 pixels and 256 bytes of model and state), made by eppm_stab_create and freed by eppm_stab_destroy; a
 * context that never creates one allocates and launches exactly what it did without.  Frames of at most 8192 x 8192 and 2^26 pixels.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_stab_params {
    float tau;                   /* largest residual of an inlier in pixels (1); finite, > 0 */
    int   iters;                 /* passes of the fit, 1 .. 8 (3) */
    float smooth;                /* share of the smoothed path that survives a step, 0 .. 1 (0.9); 1: tripod lock, 0: pass-through */
} eppm_stab_params;
typedef struct eppm_gmotion_model {
    double  p[6];                /* displacement form; all 0 when not valid */
    int64_t n_valid;             /* valid pixels (the first pass's) */
    int64_t n_inliers;           /* pixels the last pass summed: the valid inliers of the pass before it */
    int     valid;               /* at least 3 pixels that are not collinear */
    int     passes;              /* passes run: iters, or fewer when one left no valid model */
} eppm_gmotion_model;
typedef struct eppm_stab eppm_stab;

int  eppm_stab_default_params(eppm_stab_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty (its path is the identity). */
int  eppm_stab_create(eppm_ctx* ctx, const eppm_stab_params* p, eppm_stab** out);
/* a stabiliser without a context, for eppm_stab_step_frames on caller planes: nslots slots of h x w pixels on `device` */
int  eppm_stab_create_size(int h, int w, int nslots, int device, const eppm_stab_params* p, eppm_stab** out);
int  eppm_stab_destroy(eppm_stab* stab);                  /* NULL is fine */
int  eppm_stab_reset(eppm_stab* stab, int slot);          /* the slot is empty again; slot < 0: every slot */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw image 2, the level-0 forward
 * flow and occ1): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions,
 * another device or more active pairs than the stabiliser has slots.  cut: NULL, or one flag per active pair; non-zero: image 2 of that
 * pair is the first frame of another clip: the slot's paths become the identity and its output is image 2.  A slot the step does not cover
 * keeps its state.  2 * iters + 1 launches, asynchronous on the context's stream: no copy, no allocation, no host synchronisation. */
int  eppm_stab_step(eppm_stab* stab, eppm_ctx* ctx, const uint8_t* cut);
/* the same step of one slot on caller device planes of the stabiliser's size (an RGBA image of `pitch` bytes per row, h*w float2 forward
 * flow, h*w mask bytes); on the launcher stream, synchronous.  Whatever the planes hold, nothing outside them is read. */
int  eppm_stab_step_frames(eppm_stab* stab, int slot, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow, const uint8_t* d_occ1, int cut);
/* of a slot's last step (EPPM_ERR_STATE on a slot that has none): the stabilised frame as packed RGB to the host, synchronous ... */
int  eppm_stab_get(eppm_stab* stab, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the last step; the h*w mask bytes; the pair's model */
int  eppm_stab_get_device(eppm_stab* stab, int slot, void* d_rgba, size_t pitch);
int  eppm_stab_get_mask(eppm_stab* stab, int slot, uint8_t* mask);
int  eppm_stab_get_model(eppm_stab* stab, int slot, eppm_gmotion_model* model);
/* synchronous.  path: twelve doubles, C then S in (A, t) form (the identity for an empty slot); frames / invalid_steps (NULL: not wanted):
 * the updates since the last cut and how many of them had no valid model.  set_path loads C and S: the slot is no longer empty. */
int  eppm_stab_get_path(eppm_stab* stab, int slot, double* path, int64_t* frames, int64_t* invalid_steps);
int  eppm_stab_set_path(eppm_stab* stab, int slot, const double* path);
/* host forms (no GPU needed).  The fit of one pair: (u, v) the forward flow, occ1 the mask of image 1; mask: NULL or h*w bytes.  One
 * update of a path (twelve doubles, in place; the identity for a clip's first pair) and its counts (NULL, or {frames, invalid_steps}, in
 * place) with a pair's model; wf: the six float32 of the warp in displacement form.  The warp of a packed RGB image 2 by wf. */
int  eppm_gmotion_fit_host(const eppm_stab_params* p, const float* u, const float* v, const uint8_t* occ1, int h, int w,
                           eppm_gmotion_model* model, uint8_t* mask);
int  eppm_stab_update_host(const eppm_stab_params* p, double* path, int64_t* counts, const eppm_gmotion_model* model, int cut, float* wf);
int  eppm_stab_warp_host(const float* wf, const uint8_t* rgb2, int h, int w, uint8_t* rgb_out);

/* ----------------------------------------------------------------------------------------
 * scene-cut detection from the bidirectional flow.  One step, after eppm_compute_bidirectional* on a streamed
 * clip's next pair, counts per slot the pixels of image 1 and image 2 by their occlusion class (mask bytes 0, 1, 2 and 3; a byte above 3
 * counts as 3), the tracked pixels of image 2 -- occ2 == 0, a known backward vector and a source inside the frame -- and over them the sum
 * of |Y(image 2) - Y(image 1 at the nearest pixel of the source)|, Y = (77 R + 150 G + 29 B + 128) >> 8.  With n = h*w and
 * lost = min(n - c1[0], n - n_tracked), the pair is a cut iff lost * 1000 > lost_permille * n, or (residual_max >= 0, n_tracked > 0 and)
 * sad * 16 > rint(residual_max * 16) * n_tracked: equality is not a cut.  Every sum is an integer, so the kernels equal eppm_cutdet_host
 * in every number, in both libraries and on every run.  A detector is a separate allocation on its context's device (per slot 128 bytes of
 * record and 64 bytes per tile of 64 x 16 pixels), made by eppm_cutdet_create and freed by eppm_cutdet_destroy; a context that never
 * creates one allocates and launches exactly what it did without.  Frames of at most 8192 x 8192 and 2^26 pixels.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_cut_params {
    int   lost_permille;         /* a pair that loses more than this share of its pixels on both sides is a cut, 0 .. 1000 (530) */
    float residual_max;          /* largest mean |dY| over the tracked pixels that is not a cut, 0 .. 255; negative: the test is off (-1) */
} eppm_cut_params;
typedef struct eppm_cut_stats {
    int64_t n;                   /* h*w */
    int64_t c1[4], c2[4];        /* pixels of image 1 / image 2 by occlusion class */
    int64_t n_tracked;           /* tracked pixels of image 2 */
    int64_t sad;                 /* sum of their absolute luma differences */
    int32_t cut;                 /* the verdict */
    int32_t stepped;             /* 1 */
} eppm_cut_stats;
typedef struct eppm_cutdet eppm_cutdet;

int  eppm_cutdet_default_params(eppm_cut_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; no slot has a record. */
int  eppm_cutdet_create(eppm_ctx* ctx, const eppm_cut_params* p, eppm_cutdet** out);
/* a detector without a context, for eppm_cutdet_step_frames on caller planes: nslots slots of h x w pixels on `device` */
int  eppm_cutdet_create_size(int h, int w, int nslots, int device, const eppm_cut_params* p, eppm_cutdet** out);
int  eppm_cutdet_destroy(eppm_cutdet* det);                /* NULL is fine */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames, the level-0 backward
 * flow and both masks): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other
 * dimensions, another device or more active pairs than the detector has slots.  A slot the step does not cover keeps its record.  Two
 * launches, asynchronous on the context's stream: no copy, no allocation, no host synchronisation. */
int  eppm_cutdet_step(eppm_cutdet* det, eppm_ctx* ctx);
/* the same step of one slot on caller device planes of the detector's size (RGBA images of `pitch` bytes per row, h*w float2 backward
 * flow, h*w mask bytes each); on the launcher stream, synchronous.  Whatever the planes hold, nothing outside them is read. */
int  eppm_cutdet_step_frames(eppm_cutdet* det, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                             const uint8_t* d_occ1, const uint8_t* d_occ2);
/* synchronous.  The record of a slot's last step (EPPM_ERR_STATE on a slot that has none) / the verdicts of slots 0 .. n - 1 in one small
 * copy (0 for a slot without a step) */
int  eppm_cutdet_get(eppm_cutdet* det, int slot, eppm_cut_stats* stats);
int  eppm_cutdet_cuts(eppm_cutdet* det, int n, uint8_t* cut);
/* host form (no GPU needed): packed RGB images, (bu, bv) the backward flow, the two masks */
int  eppm_cutdet_host(const eppm_cut_params* p, const uint8_t* rgb1, const uint8_t* rgb2, const float* bu, const float* bv,
                      const uint8_t* occ1, const uint8_t* occ2, int h, int w, eppm_cut_stats* stats);

/* ----------------------------------------------------------------------------------------
 * dense correspondence maps to an anchor frame and layer propagation.  A map holds one slot per pair of its
 * context: per pixel of the current frame the position (sx, sy) in the slot's anchor frame that the pixel shows (h*w float2, row-major;
 * a lost pixel holds (1e10, 1e10), and any value with a component above 1e9 in magnitude or NaN reads as lost), the anchor frame, the
 * current frame and a layer (RGBA, straight alpha; by default the anchor frame with alpha 255).  One step moves every covered slot from
 * image 1 to image 2 of its pair by composing the map with the backward flow: a pixel whose backward vector is known, stays inside the
 * frame and (use_occ) is not occluded samples the previous map at its source -- bilinearly where the four taps are known and within
 * `tear` of the nearest tap in both components, otherwise the nearest tap translated --, and is kept if the anchor frame sampled
 * bilinearly at the result is within thresh of the new pixel (sum of the three absolute differences); every other pixel is lost.  The
 * render composites the layer, sampled once at the map, over the current frame; lost pixels show the current frame.  The kernels equal
 * eppm_cmap_step_host and eppm_cmap_render_host bit for bit, in both libraries.  A map is a separate allocation on its context's device
 * (32 bytes per pixel and slot: two maps, the anchor, the frame, the layer and the output), made by eppm_cmap_create and freed by
 * eppm_cmap_destroy; a context that never creates one allocates and launches exactly what it did without.  A slot that has never been
 * stepped, or after eppm_cmap_reset, is empty: its first step reads the identity as the previous map and image 1 as the anchor, which it
 * also stores.  Frames of at most 8192 x 8192 and 2^26 pixels.  Stage names: "cmap_step", "cmap_render".
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_cmap_params {
    float thresh;                /* largest |dR| + |dG| + |dB| between the new pixel and the anchor at the composed position that keeps it (90); finite, >= 0 */
    float tear;                  /* largest difference between a tap of the map and the nearest tap that still blends the four (2); finite, >= 0 */
    int   use_occ;               /* 1: a pixel with occ2 != 0 is lost (1); 0: the mask is not read into the decision */
} eppm_cmap_params;
typedef struct eppm_cmap eppm_cmap;

int  eppm_cmap_default_params(eppm_cmap_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty. */
int  eppm_cmap_create(eppm_ctx* ctx, const eppm_cmap_params* p, eppm_cmap** out);
/* a map without a context, for eppm_cmap_step_frames on caller planes: nslots slots of h x w pixels (any size from 1 x 1) on `device` */
int  eppm_cmap_create_size(int h, int w, int nslots, int device, const eppm_cmap_params* p, eppm_cmap** out);
int  eppm_cmap_destroy(eppm_cmap* cm);                    /* NULL is fine */
int  eppm_cmap_reset(eppm_cmap* cm, int slot);            /* the slot is empty again; slot < 0: every slot */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the raw frames, the level-0 backward flow
 * and occ2): valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other dimensions, another
 * device or more active pairs than the map has slots.  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair is the
 * first frame of another clip: the slot's map becomes the identity and image 2 its anchor.  A slot the step does not cover keeps its
 * state.  Two launches (the step, and the render of the covered slots), asynchronous on the context's stream: no copy, no allocation, no
 * host synchronisation. */
int  eppm_cmap_step(eppm_cmap* cm, eppm_ctx* ctx, const uint8_t* cut);
/* the same step of one slot on caller device planes of the map's size (RGBA images of `pitch` bytes per row, h*w float2 backward flow,
 * h*w mask bytes); on the launcher stream, synchronous.  d_rgba1 is read only if the slot is empty.  Whatever the planes hold, nothing
 * outside them is read. */
int  eppm_cmap_step_frames(eppm_cmap* cm, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                           const uint8_t* d_occ2, int cut);
/* synchronous.  The slot's map, h*w*2 floats (EPPM_ERR_STATE on an empty slot) / load a map and its anchor frame (packed RGB), which also
 * becomes the slot's current frame: the slot is no longer empty and its age is 0 */
int  eppm_cmap_get_state(eppm_cmap* cm, int slot, float* xy);
int  eppm_cmap_set_state(eppm_cmap* cm, int slot, const float* xy, const uint8_t* anchor_rgb, size_t row_stride);
/* synchronous.  The slot's layer: h rows of w RGBA quadruples, straight alpha, in the anchor frame's geometry; NULL: the default layer
 * again (the anchor frame with alpha 255, followed across re-anchoring).  Allowed on an empty slot. */
int  eppm_cmap_set_layer(eppm_cmap* cm, int slot, const uint8_t* rgba, size_t row_stride);
/* the slot's layer composited over its current frame through its map (EPPM_ERR_STATE on a slot that has never been stepped or loaded):
 * packed RGB to the host, synchronous ... */
int  eppm_cmap_render(eppm_cmap* cm, int slot, uint8_t* rgb, size_t row_stride);
/* ... or RGBA words (alpha 255) into a device plane, asynchronous on the stream of the map's last step.  A step renders the slots it
 * covers; these calls launch the render again only if the layer or the state was set since. */
int  eppm_cmap_render_device(eppm_cmap* cm, int slot, void* d_rgba, size_t pitch);
/* steps since the slot's anchor frame (0 after a cut step or eppm_cmap_set_state); -1 and an error for an empty slot or a bad argument */
int  eppm_cmap_age(eppm_cmap* cm, int slot);
/* host forms (no GPU needed).  One step from map_in (image 1's map; NULL: the identity, as an empty slot reads it) to map_out, which must
 * not be map_in; anchor_rgb: the anchor frame (image 1 for an empty slot), rgb2: image 2, (bu, bv): the backward flow, occ2: the mask.
 * After a cut step the caller's anchor is rgb2.  The render of a map over the current frame rgb_cur: layer_rgba, or NULL for the default
 * layer made of anchor_rgb (which is read in that case only). */
int  eppm_cmap_step_host(const eppm_cmap_params* p, float* map_out, const float* map_in, const uint8_t* anchor_rgb, const uint8_t* rgb2,
                         const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int cut);
int  eppm_cmap_render_host(uint8_t* rgb_out, const float* map, const uint8_t* rgb_cur, const uint8_t* layer_rgba, const uint8_t* anchor_rgb,
                           int h, int w);

/* ----------------------------------------------------------------------------------------
 * moving-object detection: the connected components of the stabiliser's motion mask as objects.  A detector holds
 * one slot per pair of its context.  One step fits the camera motion of every active pair with a private stabiliser (tau, iters: section
 * 16's), takes the pixels of image 1 whose mask byte is 1 ("moves on its own") as foreground, labels its components under 4- or
 * 8-connectivity, drops those smaller than min_area, numbers the others 1, 2, ... in increasing order of their root (the smallest linear
 * index y*w + x of a component) and reports the first max_objects of them: a label byte per pixel (0: background, dropped or beyond
 * max_objects) and one integer record per object.  At the end of the step the labels are carried along the backward flow to image 2; at
 * the next step an object inherits the id of the previous object that most of its carried pixels voted for, if it is that object's
 * largest claimant and the overlap is at least min_overlap pixels; every other object takes the slot's next id.  A split leaves the old id
 * with the larger part, a merge keeps the dominant previous object's id.  All results are integers, independent of any summation order:
 * the kernels equal eppm_objects_label_host, eppm_objects_assign_host and eppm_objects_carry_host bit for bit, in both libraries, on
 * every run.  A detector is a separate allocation on its context's device (14 bytes per pixel and slot plus tables, and its stabiliser's
 * 5), made by eppm_objects_create and freed by eppm_objects_destroy; a context that never creates one allocates and launches exactly
 * what it did without.  A slot that has never been stepped, or after eppm_objects_reset, is empty: its carried plane counts as zero and
 * its next id is 1.  Frames of at most 8192 x 8192 and 2^26 pixels.  Stage names: "objects_fit", "objects_label", "objects_assign".
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_objects_params {
    float tau;                   /* the fit's inlier radius in pixels (1); finite, > 0 */
    int   iters;                 /* the fit's passes (3); 1 .. 8 */
    int   connectivity;          /* 4 or 8 (8) */
    int   min_area;              /* smallest component that is an object (16); >= 1 */
    int   max_objects;           /* objects reported per slot (64); 1 .. 255 */
    int   min_overlap;           /* carried pixels an object needs to inherit an id (4); >= 1 */
} eppm_objects_params;
typedef struct eppm_object {
    int32_t id, age;             /* the identity, and the steps it has been inherited for */
    int32_t area;
    int32_t x0, y0, x1, y1;      /* inclusive bounding box */
    int32_t n_flow;              /* pixels of the object with a valid forward vector (known, |u|, |v| <= 8192) */
    int64_t sum_x, sum_y;        /* over the object's pixels: the centroid is sum / area */
    int64_t sum_qu, sum_qv;      /* over the n_flow pixels: (int)rintf(u * 256); the mean velocity is sum / (256 * n_flow) */
} eppm_object;
typedef struct eppm_objects_counts {
    int32_t n;                   /* objects reported: min(n_found, max_objects) */
    int32_t n_found;             /* components with area >= min_area */
    int32_t n_components;        /* components of the foreground */
    int32_t next_id;             /* the id the slot's next new object takes */
} eppm_objects_counts;
typedef struct eppm_objects eppm_objects;

int  eppm_objects_default_params(eppm_objects_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty. */
int  eppm_objects_create(eppm_ctx* ctx, const eppm_objects_params* p, eppm_objects** out);
/* a detector without a context: nslots slots of h x w pixels (any size from 1 x 1) on `device` */
int  eppm_objects_create_size(int h, int w, int nslots, int device, const eppm_objects_params* p, eppm_objects** out);
int  eppm_objects_destroy(eppm_objects* det);             /* NULL is fine */
int  eppm_objects_reset(eppm_objects* det, int slot);     /* the slot is empty again (next_id 1); slot < 0: every slot.  Synchronous */
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional* (the level-0 flows, occ1 and occ2), under
 * eppm_stab_step's rules: valid in the window of eppm_interpolate* (EPPM_ERR_STATE outside it); EPPM_ERR_ARG for a context of other
 * dimensions, another device or more active pairs than the detector has slots.  cut: NULL, or one flag per active pair; non-zero: image 2
 * of that pair is the first frame of another clip, so nothing is carried to it: the slot's carried plane becomes zero and every object of
 * its next step is new (next_id keeps counting).  A slot the step does not cover keeps its state.  A fixed sequence of launches,
 * asynchronous on the context's stream: no copy, no allocation, no host synchronisation. */
int  eppm_objects_step(eppm_objects* det, eppm_ctx* ctx, const uint8_t* cut);
/* the kernels alone, without a fit, for one slot on caller device planes of the detector's size: h*w mask bytes (1: foreground), h*w
 * float2 forward flow, and h*w float2 backward flow with h*w occ2 bytes; either of the last two NULL: no carry, the carried plane becomes
 * zero.  On the launcher stream, synchronous.  Whatever the planes hold, nothing outside them is read. */
int  eppm_objects_step_frames(eppm_objects* det, int slot, const uint8_t* d_mask, const eppm_float2* d_flow, const eppm_float2* d_flow_bwd,
                              const uint8_t* d_occ2, int cut);
/* synchronous; EPPM_ERR_STATE on a slot that has never been stepped, and -- with a message that says so -- if a loop of a kernel hit
 * its iteration cap in the slot's last steps (a defect of the library, never an input's fault; eppm_objects_reset clears it).
 * The first min(n, max) records, in label order, and the counts (either may be NULL) / the h*w label bytes */
int  eppm_objects_get(eppm_objects* det, int slot, int max, eppm_object* records, eppm_objects_counts* counts);
int  eppm_objects_get_labels(eppm_objects* det, int slot, uint8_t* labels);
/* synchronous.  A slot's state between two steps: the carried plane (h*w bytes: the last labels as image 2's pixels see them), the ids
 * and ages of the last objects (256 entries each, indexed by label; entry 0 and those beyond the last n are 0) and next_id.  An empty
 * slot gives zeros and next_id 1.  set_state makes the slot non-empty; next_id outside [1, 2^30] or an age outside [0, 2^30] is
 * EPPM_ERR_ARG.  A carried byte above max_objects counts as 0. */
int  eppm_objects_get_state(eppm_objects* det, int slot, uint8_t* carried, int32_t* prev_id, int32_t* prev_age, int32_t* next_id);
int  eppm_objects_set_state(eppm_objects* det, int slot, const uint8_t* carried, const int32_t* prev_id, const int32_t* prev_age, int32_t next_id);
/* host forms (no GPU needed; plain sequential code).  label: mask, u, v (h*w each) to the label bytes, max_objects records (id and age 0)
 * and counts (next_id is not touched).  carry: the labels to image 2 along the backward flow (bu, bv) and occ2.  assign: the identity
 * rule for the n objects of `labels` against the carried plane (NULL: all zero), reading and rewriting the 256-entry tables and *next_id
 * and setting id and age of the n records. */
int  eppm_objects_label_host(const eppm_objects_params* p, const uint8_t* mask, const float* u, const float* v, int h, int w, uint8_t* labels,
                             eppm_object* records, eppm_objects_counts* counts);
int  eppm_objects_carry_host(const uint8_t* labels, const float* bu, const float* bv, const uint8_t* occ2, int h, int w, uint8_t* carried);
int  eppm_objects_assign_host(const eppm_objects_params* p, const uint8_t* labels, const uint8_t* carried, int h, int w, int n, int32_t* prev_id,
                              int32_t* prev_age, int32_t* next_id, eppm_object* records);

/* ----------------------------------------------------------------------------------------
 * Background plates: the scene behind the moving objects, aligned to the clip's first frame, and frames with the
 * moving objects painted out from it.  A plate is an attachment like the stabiliser: one slot per pair, its own allocation, nothing
 * launched for a context that never creates one.  A slot owns a canvas of (h + 2*margin_y) x (w + 2*margin_x) pixels in the coordinates of
 * the clip's first frame (the anchor), which sits at canvas offset (margin_x, margin_y); per canvas pixel a running mean {R, G, B, n}
 * (float4).  A step on a pair fits the camera's motion (the stabiliser's fit), dilates its mask by `grow` into a blocked plane, and
 * accumulates IMAGE 1 of the pair: every canvas pixel whose position under the slot's camera path P (frame 0 -> image 1) lies inside the
 * frame with no blocked tap takes the bilinear sample c: an empty state (!(n >= 1)) becomes {c, 1}; a sample within `thresh` (sum of
 * absolute differences) of the mean joins it, n' = min(n + 1, n_max); any other lowers n by one, so a value contradicted more often than
 * confirmed empties and is replaced.  Then P advances by the pair's model (unchanged by an invalid one).  A path with !(|det A| > 1e-6)
 * accumulates nothing.  The render fills the blocked pixels of image 1 from the canvas: fill byte 0 = free (the image), 1 = filled (every
 * one of the four canvas taps has n >= min_count), 2 = blocked but not filled (the image).  Whatever the inputs hold -- NaN paths, any
 * mask bytes, any states -- nothing outside the frame or the canvas is read.  Every kernel gathers: the same bits on every run, equal to
 * the host forms below.
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_plate_params {
    float tau;                   /* the fit's inlier radius in pixels (1); finite, > 0 */
    int   iters;                 /* the fit's passes (3); 1 .. 8 */
    int   margin_x, margin_y;    /* canvas margins (0, 0); >= 0, the canvas within 8192 x 8192 and 2^26 pixels */
    int   grow;                  /* dilation radius of the mask (2); 0 .. 8 */
    int   accept_invalid;        /* mask bytes other than 0 and 1 (not valid) count as free (0: they block) */
    float thresh;                /* a sample this close to the mean confirms it (40); finite, >= 0 */
    int   n_max;                 /* the count's cap (64); 1 .. 255 */
    int   min_count;             /* a canvas tap fills with at least this count (2); 1 .. 255 */
} eppm_plate_params;
typedef struct eppm_plate eppm_plate;

int  eppm_plate_default_params(eppm_plate_params* p);
/* p NULL: the defaults.  One slot per pair of ctx (eppm_batch_size), on its device; every slot empty, its path the identity. */
int  eppm_plate_create(eppm_ctx* ctx, const eppm_plate_params* p, eppm_plate** out);
/* a plate without a context: nslots slots of h x w pixels (any size from 1 x 1) on `device` */
int  eppm_plate_create_size(int h, int w, int nslots, int device, const eppm_plate_params* p, eppm_plate** out);
int  eppm_plate_destroy(eppm_plate* plate);               /* NULL is fine */
int  eppm_plate_reset(eppm_plate* plate, int slot);       /* the slot is empty again, its path the identity; slot < 0: every slot.  Synchronous */
int  eppm_plate_canvas_dims(const eppm_plate* plate, int* ch, int* cw);
/* One step of slots 0 .. active pairs - 1 on the pairs of ctx's last eppm_compute_bidirectional*, under eppm_stab_step's window, rules
 * and error codes.  cut: NULL, or one flag per active pair; non-zero: image 2 of that pair starts another clip: image 1 is still
 * accumulated, then the path becomes the identity and the canvas is kept (eppm_plate_reset empties it).  A fixed sequence of launches,
 * asynchronous on the context's stream: no copy, no allocation, no host synchronisation. */
int  eppm_plate_step(eppm_plate* plate, eppm_ctx* ctx, const uint8_t* cut);
/* the kernels alone, without a fit, for one slot on caller device planes: image 1 (RGBA words, pitch bytes per row) and h*w mask bytes
 * (0 free, 1 blocked, others not valid).  path6: the slot's path {a00, a01, a10, a11, tx, ty} for this step (it is stored), NULL: the
 * slot's own; without a model the path does not advance.  On the launcher stream, synchronous. */
int  eppm_plate_step_frames(eppm_plate* plate, int slot, const void* d_rgba, size_t pitch, const uint8_t* d_mask, const double* path6, int cut);
/* image 1 of the last stepped pair of `slot` with its blocked pixels filled from the canvas (h*w*3 bytes, row_stride >= 3*w) and the fill
 * bytes (h*w, or NULL); in eppm_plate_step's window.  Synchronous.  EPPM_ERR_STATE on an empty slot. */
int  eppm_plate_render(eppm_plate* plate, eppm_ctx* ctx, int slot, uint8_t* rgb, size_t row_stride, uint8_t* fill);
/* the render alone on caller device planes, against the slot's canvas as it is: the frame, its mask and its path (NULL: the slot's own)
 * to h*w RGBA words (out_pitch bytes per row) and h*w fill bytes.  The slot's path is not changed.  On the launcher stream, synchronous. */
int  eppm_plate_render_frames(eppm_plate* plate, int slot, const void* d_rgba, size_t pitch, const uint8_t* d_mask, const double* path6,
                              void* d_rgba_out, size_t out_pitch, uint8_t* d_fill);
/* synchronous; EPPM_ERR_STATE on an empty slot.  The canvas as ch*cw*3 bytes (row_stride >= 3*cw) and its coverage (ch*cw bytes:
 * min(n, 255), 0 for !(n >= 1); or NULL) / as RGBA words on the device / the fit's mask of the last step (h*w bytes; EPPM_ERR_STATE when
 * that step had no fit), for the two-pass use: step a clip keeping each pair's mask and path, then eppm_plate_render_frames every frame
 * against the finished plate */
int  eppm_plate_get(eppm_plate* plate, int slot, uint8_t* rgb, size_t row_stride, uint8_t* coverage);
int  eppm_plate_get_device(eppm_plate* plate, int slot, void* d_rgba, size_t pitch);
int  eppm_plate_get_mask(eppm_plate* plate, int slot, uint8_t* mask);
/* synchronous.  The slot's path (six doubles; the identity for an empty slot) and its canvas states (ch*cw float4 {R, G, B, n};
 * get_state: EPPM_ERR_STATE on an empty slot; set_state makes the slot non-empty) */
int  eppm_plate_get_path(eppm_plate* plate, int slot, double* path6);
int  eppm_plate_set_path(eppm_plate* plate, int slot, const double* path6);
int  eppm_plate_get_state(eppm_plate* plate, int slot, float* state);
int  eppm_plate_set_state(eppm_plate* plate, int slot, const float* state);
/* host forms (no GPU needed; plain sequential code; p supplies margins, grow, accept_invalid, thresh, n_max and min_count).  forms: a
 * path's two six-float displacement forms and whether it is valid.  block: the dilated blocked plane of a mask.  accumulate: one frame
 * (h*w*3 bytes) into the canvas states, in place (an empty canvas is all zero).  render: the frame with its blocked pixels filled
 * (h*w*3 bytes) and the fill bytes (or NULL). */
int  eppm_plate_forms_host(const double* path6, float* fwd, float* inv, int* ok);
int  eppm_plate_block_host(const eppm_plate_params* p, const uint8_t* mask, int h, int w, uint8_t* blocked);
int  eppm_plate_accumulate_host(const eppm_plate_params* p, const float* fwd, const uint8_t* rgb, const uint8_t* blocked, int h, int w, float* state);
int  eppm_plate_render_host(const eppm_plate_params* p, const float* inv, int ok, const uint8_t* rgb, const uint8_t* blocked, int h, int w,
                            const float* state, uint8_t* rgb_out, uint8_t* fill);

/* Per-stage device times in ms (hipEvent pairs on the context's stream), one entry per stage per
 * call since the last eppm_clear_stage_times (names repeat across calls; prepare entries first).
 * names[i] points to static strings.  Returns the number of entries written (<= max). */
int  eppm_stage_times(eppm_ctx* ctx, const char** names, float* ms, int max);
int  eppm_clear_stage_times(eppm_ctx* ctx);
/* 0: no events (default); 1: an event pair around every stage; 2: only around the dominant kernel (the candidate
 * refine, entries "c2f_refine_L<l>").  A bidirectional call adds (mode 1) "l2_post_bwd", "upsample_bwd_L<l>", "c2f_refine_bwd_L<l>",
 * "flow_blf_bwd_L<l>", "flow_blf_bwd_final" and "fb_occlusion"; an interpolation call "interp_splat", "interp_fill" and "interp_blend"
 * (mode 1, once per group of four times); a track step "track_advance", "track_seed" and "track_compact" (mode 1; the step that seeds
 * frame 0 adds a "track_seed" before "track_advance"); a compute that starts from a temporal prior "temporal_advect" (before "patchmatch") and
 * "temporal_select" (inside it: "patchmatch" includes its time); a temporal-filter step "tfilter_step"; a stabiliser step "stab_fit" (every accumulate and solve launch) and "stab_warp"; a cut-detector step "cutdet"; a motion-blur call "mblur_pack" and "mblur_gather"; a correspondence-map step "cmap_step" and "cmap_render"; an object-detector step "objects_fit" (its stabiliser's launches), "objects_label" and "objects_assign"; a background-plate step "plate_fit" (its stabiliser's launches), "plate_block" and "plate_accumulate", its render "plate_render"; a defect-filter step "defect_detect" and "defect_apply"; a deflicker step "deflicker_fit" (every accumulate and field launch) and "deflicker_apply".  Events come from a per-context pool: none is created in a steady-state step. */
int  eppm_enable_stage_timing(eppm_ctx* ctx, int on);

const char* eppm_last_error(void);
const char* eppm_version(void);

/* ----------------------------------------------------------------------------------------
 * device-memory plumbing for callers without a HIP runtime binding (tests, FFI hosts)
 * -------------------------------------------------------------------------------------- */
int  eppm_device_count(int* n);
int  eppm_set_device(int device);
int  eppm_malloc_device(void** p, size_t bytes);
int  eppm_malloc_pitched(void** p, size_t* pitch, size_t width_bytes, size_t rows);  /* cudaMallocPitch analogue */
int  eppm_free_device(void* p);
int  eppm_memcpy_h2d(void* dst, const void* src, size_t bytes);
int  eppm_memcpy_d2h(void* dst, const void* src, size_t bytes);
int  eppm_memcpy2d_h2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t rows);
int  eppm_memcpy2d_d2h(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes, size_t rows);
int  eppm_memset_device(void* p, int value, size_t bytes);
int  eppm_device_synchronize(void);
/* PCI address of a device, lower case as sysfs spells it ("0000:c1:00.0"; hipDeviceGetPCIBusId); buf: at least 13 bytes */
int  eppm_device_pci_bus_id(int device, char* buf, size_t len);
/* Multi-GPU hosts (one host thread per GPU, one context each: pair i -> GPU i mod N): binds the CALLING thread, and the threads it
 * creates afterwards, to the CPUs of the NUMA node the device's PCIe slot belongs to (sysfs), within the CPUs the thread may use now.
 * *numa_node = -1, *ncpus = 0 and nothing bound when the topology is not visible; either pointer may be NULL. */
int  eppm_bind_thread_to_device(int device, int* numa_node, int* ncpus);
/* free / total memory of the current device (sizing the number of contexts in flight; leak checks) */
int  eppm_device_mem_info(size_t* free_bytes, size_t* total_bytes);
/* A destroyed context's slab and pinned staging buffers are kept (a few blocks, bounded in bytes) for the next context of the same size:
 * allocation is inside the window the reference's demo times.  This gives them back to the runtime. */
int  eppm_release_cached_memory(void);
/* Stream used by the reference-signature launchers below (default: the null stream). */
int  eppm_set_launcher_stream(void* hip_stream);
/* Parameters used by the reference-signature launchers (default: defs.h values). */
int  eppm_set_launcher_params(const eppm_params* p);
/* Status of the most recent void launcher below (they cannot return one). */
int  eppm_launcher_status(void);

/* ----------------------------------------------------------------------------------------
 * stage launchers: the reference's live extern "C" ABI (driver .cpp:40-62).
 * All pointers are DEVICE pointers, all *_pitch are in BYTES, argument order is (w,h).
 * Pyramid tables (T**, int*, size_t*) are HOST arrays of device pointers
 * (basic/bao_basic_cuda.h:209-229).  uchar4/short2/float2 are the layouts declared above.
 * -------------------------------------------------------------------------------------- */
/* bao_pmflow_refine_kernel.cu:1060-1071 */
void baoCudaPatchMatchMultiscalePrepare(eppm_uchar4** pImgPyr1, eppm_uchar4** pImgPyr2, unsigned char** pCensusPyr1,
        unsigned char** pCensusPyr2, eppm_uchar4** pTempPyr1, eppm_uchar4** pTempPyr2, int* arrH, int* arrW,
        size_t* arrPitchUchar4, size_t* arrPitchUchar1, int nLevels, eppm_uchar4* d_img1, eppm_uchar4* d_img2, int h, int w);
/* bao_pmflow_census_kernel.cu:93-112 */
void baoCudaCensusTransform(unsigned char* d_census1, unsigned char* d_census2, eppm_uchar4* d_img1, eppm_uchar4* d_img2,
        int w, int h, size_t img_pitch, size_t census_pitch);
/* bao_pmflow_kernel.cu:1760-1826 */
void baoCudaPatchMatch(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img1, eppm_uchar4* d_img2,
        unsigned char* d_census1, unsigned char* d_census2, int w, int h, size_t img_pitch, size_t cost_pitch,
        size_t disp_pitch, size_t census_pitch);
/* bao_pmflow_refine_kernel.cu:78-92 */
void baoCudaLeftRightCheck(eppm_short2* d_disp_vec, float* d_cost, eppm_short2* d_disp_vec2, float* d_cost2,
        int w, int h, size_t cost_pitch, size_t disp_pitch);
/* bao_pmflow_refine_kernel.cu:185-193 */
void baoCudaOutlierRemoval(eppm_short2* d_disp_vec, float* d_cost, int w, int h, size_t cost_pitch, size_t disp_pitch);
/* bao_pmflow_refine_kernel.cu:261-286 */
void baoCudaWeightedMedianFilter(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img, int w, int h,
        size_t img_pitch, size_t cost_pitch, size_t disp_pitch, int num_iter, bool is_only_occlusion);
/* bao_pmflow_refine_kernel.cu:373-390 */
void baoCudaFillHole(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img, int w, int h,
        size_t img_pitch, size_t cost_pitch, size_t disp_pitch);
/* bao_pmflow_refine_kernel.cu:724-734 */
void baoCudaNNF2Flow(eppm_float2* d_flow, eppm_short2* d_disp_vec, int w, int h, size_t disp_pitch, size_t flow_pitch);
/* bao_pmflow_refine_kernel.cu:1076-1087 */
void baoCudaBLF_C2F(eppm_float2** pFlowPyr, eppm_uchar4** pImgPyr1, eppm_uchar4** pImgPyr2, unsigned char** pCensusPyr1,
        unsigned char** pCensusPyr2, eppm_float2** pTempPyr1, eppm_float2** pTempPyr2, int* arrH, int* arrW,
        size_t* arrPitchUchar4, size_t* arrPitchUchar1, int nLayerIdx);
/* bao_pmflow_kernel.cu:2042-2069 */
void baoCudaBLFCostFilterRefine(eppm_float2* d_flow_vec, eppm_uchar4* d_img1, eppm_uchar4* d_img2, unsigned char* d_census1,
        unsigned char* d_census2, int w, int h, size_t img_pitch, size_t census_pitch);
/* bao_pmflow_refine_kernel.cu:801-826 */
void baoCudaFlowSmoothing(eppm_float2* d_flow, eppm_uchar4* d_img, int w, int h, size_t img_pitch, size_t flow_pitch);
/* basic/bao_basic_cuda.cuh:839-845 (float2 form): d_rgba h*w uchar4 {R,G,B,0}, d_flow h*w float2, both unpitched.
 * The library also exports the C++-linkage symbol the reference's driver declares at :64,
 *   void bao_cuda_convert_flow_to_colorshow(uchar4*, float2*, int h, int w, float max_disp_x, float max_disp_y)
 * (HIP vector types; a C header cannot declare it). */
int  eppm_flow_to_color(eppm_uchar4* d_rgba, const eppm_float2* d_flow, int h, int w, float max_disp_x, float max_disp_y);

/* ----------------------------------------------------------------------------------------
 * sub-stage entry points of PatchMatch (for parity tests at kernel granularity).  They mirror
 * the reference's inner launchers baoGenerateRandomField / baoComputeCostField / baoSegPropagate /
 * baoRandomSearch (bao_pmflow_kernel.cu:153-165, 689-696, 1167-1181, 1588-1594), with the
 * texture bindings and the global RNG state made explicit arguments.
 * rng: opaque device buffer from eppm_pm_rng_create (one XORWOW stream per 16x16 block).
 * PRECONDITION of the three propagate entry points AND of eppm_pm_random_search: d_cost[p] is the patch cost of d_nnf[p] (as eppm_pm_cost_field,
 * a propagate or a search leaves it).  A candidate equal to the pixel's stored match is rejected without being
 * evaluated -- it would reproduce the stored cost bit for bit, and the reference's strict `<` rejects it too; with a
 * cost plane that is NOT consistent with the NNF the reference would re-evaluate and could lower the cost, these would not
 * (a random guess equal to the stored match likewise sits its evaluation out).
 * -------------------------------------------------------------------------------------- */
typedef struct eppm_pm_rng eppm_pm_rng;
int  eppm_pm_rng_create(eppm_pm_rng** out, int w, int h, const eppm_params* p);
int  eppm_pm_rng_reset(eppm_pm_rng* rng);        /* back to curand_init(seed, block_id, 0) */
int  eppm_pm_rng_destroy(eppm_pm_rng* rng);
/* host copy of the per-block XORWOW state at the current stream position: 6 x uint32 per block (v[5], d) */
int  eppm_pm_rng_block_states(eppm_pm_rng* rng, uint32_t* dst, size_t dst_words);
int  eppm_pm_gen_rand_field(eppm_pm_rng* rng, eppm_short2* d_nnf, int w, int h, size_t disp_pitch);
int  eppm_pm_cost_field(float* d_cost, const eppm_short2* d_nnf, const eppm_uchar4* d_img1, const eppm_uchar4* d_img2,
        const unsigned char* d_census1, const unsigned char* d_census2, int w, int h, size_t img_pitch,
        size_t cost_pitch, size_t disp_pitch, size_t census_pitch);
/* dir: 0 row fwd, 1 col fwd, 2 row rev, 3 col rev; dir < 0: all four in the reference's order */
int  eppm_pm_seg_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* d_img1, const eppm_uchar4* d_img2,
        const unsigned char* d_census1, const unsigned char* d_census2, int w, int h, size_t img_pitch,
        size_t cost_pitch, size_t disp_pitch, size_t census_pitch, int dir);
/* baoJumpPropagate (bao_pmflow_kernel.cu:843-857): six Jacobi launches with step 32,16,8,4,2,1 */
int  eppm_pm_jump_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* d_img1, const eppm_uchar4* d_img2,
        const unsigned char* d_census1, const unsigned char* d_census2, int w, int h, size_t img_pitch,
        size_t cost_pitch, size_t disp_pitch, size_t census_pitch);
/* baoParallelPropagate (bao_pmflow_kernel.cu:720-795): ONE Jacobi launch of the 4-neighbour propagation */
int  eppm_pm_parallel_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* d_img1, const eppm_uchar4* d_img2,
        const unsigned char* d_census1, const unsigned char* d_census2, int w, int h, size_t img_pitch,
        size_t cost_pitch, size_t disp_pitch, size_t census_pitch);
int  eppm_pm_random_search(eppm_pm_rng* rng, float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* d_img1,
        const eppm_uchar4* d_img2, const unsigned char* d_census1, const unsigned char* d_census2, int w, int h,
        size_t img_pitch, size_t cost_pitch, size_t disp_pitch, size_t census_pitch);
/* basic/bao_basic_cuda.cuh:437-481 and :565-615 (uchar4), :511-537 (float2) */
int  eppm_gauss_filter_rgba(eppm_uchar4* d_out, const eppm_uchar4* d_in, size_t pitch, int h, int w, float sigma, int radius);
int  eppm_resize_rgba(eppm_uchar4* d_out, size_t out_pitch, int outH, int outW, const eppm_uchar4* d_in, size_t in_pitch,
        int h, int w, float ratio);
int  eppm_resize_flow(eppm_float2* d_out, int outH, int outW, const eppm_float2* d_in, int h, int w, float ratio);
/* Draft mode's upsampling alone, on unpitched float2 device planes: d_out (h x w) = the flow smoothing, guided by
 * d_guide (h x w RGBA, guide_pitch bytes per row), of the plane whose pixel (x, y) holds 2 * d_coarse[min(y >> 1, hc - 1)][min(x >> 1, wc - 1)]
 * (d_coarse: hc x wc).  One launch; the replicated plane is never written.  On the launcher stream, synchronous. */
int  eppm_flow_upsample(eppm_float2* d_out, int h, int w, const eppm_float2* d_coarse, int hc, int wc, const eppm_uchar4* d_guide,
        size_t guide_pitch);
/* ----------------------------------------------------------------------------------------
 * file formats used by the reference's CLI (main.cpp:56-69)
 * -------------------------------------------------------------------------------------- */
/* P6/P5 reader tolerant of '#' comment lines (basic/bao_basic.cpp:137-218). image: h*w*3 bytes. */
int  eppm_load_ppm(const char* filename, uint8_t* image, int h, int w, int* channels);
int  eppm_ppm_size(const char* filename, int* h, int* w);
/* Middlebury .flo: "PIEH", int32 w, int32 h, interleaved f32 (u,v) rows (flowIO.cpp:122-163). */
int  eppm_save_flo(const char* filename, const float* u, const float* v, int h, int w);
int  eppm_load_flo(const char* filename, float* u, float* v, int h, int w);
int  eppm_flo_size(const char* filename, int* h, int* w);
/* EPE / AAE with the reference's validity rule (basic/bao_flow_tools.cpp:64-111); _border: `border` pixels on every side left out. */
int  eppm_flow_error(const float* u, const float* v, const float* gt_u, const float* gt_v, int h, int w, float* epe, float* aae);
int  eppm_flow_error_border(const float* u, const float* v, const float* gt_u, const float* gt_v, int h, int w, int border, float* epe, float* aae);
/* Fraction of the pixels with known ground truth whose end-point error exceeds error_thresh; error_map: h*w bytes (255 there) or
 * NULL (bao_calc_flow_error_percentage, basic/bao_flow_tools.cpp:114-141). */
int  eppm_flow_error_percentage(const float* u, const float* v, const float* gt_u, const float* gt_v, int h, int w, int error_thresh,
                                uint8_t* error_map, float* fraction);
/* Both components clamped to [-|cutoff|, |cutoff|]; unknown vectors pass through unless cut_invalid (bao_flow_cutoff, :166-197). */
int  eppm_flow_cutoff(float* u_out, float* v_out, const float* u, const float* v, int h, int w, int cutoff, int cut_invalid);
/* The occlusion criterion above on host planes (flows read from .flo files): occ h*w bytes for F = (u, v), G = (bu, bv); bit-identical
 * to eppm_fb_occlusion. */
int  eppm_fb_occlusion_host(uint8_t* occ, const float* u, const float* v, const float* bu, const float* bv, int h, int w,
                            float alpha, float beta);
/* Host colour coding scaled by the field's largest known radius, unknown vectors black; rgb: h*w*3 bytes R,G,B
 * (bao_convert_flow_to_colorshow, :200-231, on Middlebury's computeColor, 3rdparty/middlebury/colorcode.cpp:30-85).  Where the
 * reference is undefined this is defined: a field with no motion or no known vector (largest radius 0: 0/0 there, then
 * colorwheel[(int)NaN]) is scaled by 1 -- a static scene is white --, and a vector with a NaN component is black. */
int  eppm_flow_to_color_host(uint8_t* rgb, const float* u, const float* v, int h, int w);

#ifdef __cplusplus
}
#endif
#endif /* EPPM_H_ */
