/* eppm_yuv.h -- Y'CbCr 4:2:0 frames in and out: NV12 / I420 / P010-style planes to and from the library's RGB and
 * RGBA forms, on the device and on the host, the context calls that take such frames, and y4m files.  Everything here is opt-in: a context
 * that never makes one of these calls allocates and launches exactly what it does without this header.
 *
 * A frame of h rows by w columns is a luma plane of h x w samples and chroma of ch = (h + 1) / 2 rows by cw = (w + 1) / 2 columns (odd
 * sizes are legal): one plane of cw interleaved {Cb, Cr} pairs per row (NV12), or a Cb plane and a Cr plane (I420).  A sample is a byte at
 * depth 8 and a little-endian 16-bit word above.  `planes` is always three pointers -- {Y, CbCr, ignored} or {Y, Cb, Cr} -- and `pitches` /
 * `strides` three byte counts, the distance between the rows of each plane.
 *
 * The arithmetic is integer only (eppm_amd/csrc/yuv.h), so the kernels, the host forms and a restatement agree byte for byte. */
#ifndef EPPM_YUV_H
#define EPPM_YUV_H

#include "eppm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EPPM_YUV_NV12 = 0, EPPM_YUV_I420 = 1 };
enum { EPPM_YUV_BT601 = 0, EPPM_YUV_BT709 = 1, EPPM_YUV_BT2020 = 2 };
enum { EPPM_YUV_LEFT = 0, EPPM_YUV_CENTER = 1 };

typedef struct {
    int layout;       /* EPPM_YUV_NV12 0: Y plane + interleaved CbCr plane;  EPPM_YUV_I420 1: Y, Cb, Cr planes */
    int depth;        /* 8, 10, 12 or 16 bits per sample; above 8: little-endian 16-bit words */
    int msb_aligned;  /* depth > 8 only. 1: value = word >> (16 - depth)  (P010 / P016);  0: value = word & (2^depth - 1)  (yuv420p10le, y4m C420p10) */
    int matrix;       /* EPPM_YUV_BT601 0, EPPM_YUV_BT709 1, EPPM_YUV_BT2020 2 (non-constant luminance) */
    int full_range;   /* 0: Y 16..235, C 16..240, scaled by 2^(depth-8);  1: 0 .. 2^depth - 1 */
    int siting;       /* EPPM_YUV_LEFT 0: chroma co-sited with even luma columns, centred between the two rows (MPEG-2, H.264, HEVC default);
                         EPPM_YUV_CENTER 1: centred both ways (JPEG, MPEG-1) */
} eppm_yuv_format;

/* NV12, 8 bit, BT.709, limited range, LEFT siting */
int eppm_yuv_default_format(eppm_yuv_format* f);
/* rows and bytes per row of plane 0, 1 or 2 of an h x w frame (plane 2 of NV12: 0 and 0).  EPPM_ERR_ARG for a bad format, size or plane */
int eppm_yuv_plane_dims(const eppm_yuv_format* f, int h, int w, int plane, int* rows, int* row_bytes);

/* The kernels alone on caller device planes.  d_rgba: one word {R, G, B, A} per pixel, rows `pitch` bytes apart (a multiple of 4; a base and
 * pitch that are multiples of 16 take the 16-byte stores).  to_rgba writes alpha 0; from_rgba ignores alpha.  Bytes between the rows of a
 * destination are not written.  stream: a hipStream_t, NULL = the launcher stream (eppm_set_launcher_stream); asynchronous on it.
 * Argument errors (EPPM_ERR_ARG with a message, here and in every call below): an unknown enum value, depth outside {8, 10, 12, 16},
 * msb_aligned with depth 8, a pitch below the row's bytes, an odd pitch for 16-bit words, a NULL plane the layout needs. */
int eppm_yuv_to_rgba(const eppm_yuv_format* f, const void* const* d_planes, const size_t* pitches, void* d_rgba, size_t pitch, int h, int w, void* stream);
int eppm_yuv_from_rgba(const eppm_yuv_format* f, const void* d_rgba, size_t pitch, void* const* d_planes, const size_t* pitches, int h, int w, void* stream);

/* Host forms, no GPU needed, byte-identical to the kernels.  rgb: packed {R, G, B} bytes, rows row_stride bytes apart. */
int eppm_yuv_to_rgb_host(const eppm_yuv_format* f, const void* const* planes, const size_t* strides, uint8_t* rgb, size_t row_stride, int h, int w);
int eppm_yuv_from_rgb_host(const eppm_yuv_format* f, const uint8_t* rgb, size_t row_stride, void* const* planes, const size_t* strides, int h, int w);

/* Context forms, mirroring eppm_set_images / eppm_push_image / eppm_batch_* and their *_device forms one for one: after a call every plane
 * and every flow of the context equals, bit for bit, those after the matching RGB call on eppm_yuv_to_rgb_host of the same frames.  State
 * rules, temporal arming, new_clip, the n == active pairs rule, pending computes and the error codes are those of the RGB calls.
 * Host forms: the planes are uploaded as they are (1.5 bytes per pixel at depth 8) and converted on the device straight into the
 * context's raw planes; registered memory (eppm_host_register) is read in place, other memory goes through pinned staging; the call
 * returns when the caller may reuse the planes.  Device forms: the kernel reads the caller's planes in stream order, there is no
 * intermediate RGBA plane and no copy.  Batch forms: 3 * n plane pointers per image (slot k's at [3k .. 3k + 2]), one `strides` triple. */
int eppm_yuv_set_images(eppm_ctx* ctx, const eppm_yuv_format* f, const void* const* planes1, const void* const* planes2, const size_t* strides);
int eppm_yuv_set_images_device(eppm_ctx* ctx, const eppm_yuv_format* f, const void* const* d_planes1, const void* const* d_planes2, const size_t* pitches);
int eppm_yuv_push_image(eppm_ctx* ctx, const eppm_yuv_format* f, const void* const* planes, const size_t* strides);
int eppm_yuv_push_image_device(eppm_ctx* ctx, const eppm_yuv_format* f, const void* const* d_planes, const size_t* pitches);
int eppm_yuv_batch_set_images(eppm_ctx* ctx, const eppm_yuv_format* f, int n, const void* const* planes1, const void* const* planes2, const size_t* strides);
int eppm_yuv_batch_set_images_device(eppm_ctx* ctx, const eppm_yuv_format* f, int n, const void* const* d_planes1, const void* const* d_planes2, const size_t* pitches);
int eppm_yuv_batch_push_images(eppm_ctx* ctx, const eppm_yuv_format* f, int n, const void* const* planes, const size_t* strides, const uint8_t* new_clip);
int eppm_yuv_batch_push_images_device(eppm_ctx* ctx, const eppm_yuv_format* f, int n, const void* const* d_planes, const size_t* pitches, const uint8_t* new_clip);

/* y4m files (YUV4MPEG2): I420 planes, one FRAME per picture.  Colour-space tags: C420jpeg = CENTER siting; C420mpeg2 and a bare C420 (or
 * none) = LEFT; C420p10 / C420p12 / C420p16 = 16-bit words, low-aligned.  XCOLORRANGE=FULL|LIMITED is honoured (default limited).  The
 * matrix is not in the file: BT.601 below 720 rows, BT.709 from 720 rows; overwrite f->matrix after opening to choose another.  Refused with
 * a message that names the tag: C420paldv, C422*, C444*, Cmono*, interlaced It / Ib / Im.  Malformed (EPPM_ERR_ARG): a missing W or H, a
 * missing FRAME line, a truncated frame.  The writer emits the tags the reader maps back to the same format (layout I420, low-aligned). */
typedef struct eppm_y4m eppm_y4m;
int eppm_y4m_open_read(eppm_y4m** out, const char* path, int* h, int* w, eppm_yuv_format* f, int* fps_num, int* fps_den);
/* the next frame into I420 planes; *got = 1, or 0 at a clean end of file (the planes are then not written) */
int eppm_y4m_read_frame(eppm_y4m* y, void* const* planes, const size_t* strides, int* got);
int eppm_y4m_open_write(eppm_y4m** out, const char* path, int h, int w, const eppm_yuv_format* f, int fps_num, int fps_den);
int eppm_y4m_write_frame(eppm_y4m* y, const void* const* planes, const size_t* strides);
int eppm_y4m_close(eppm_y4m* y);

#ifdef __cplusplus
}
#endif
#endif
