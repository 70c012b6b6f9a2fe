// runeppm -- CLI with the I/O contract of the reference's demo (main.cpp:36-79): read two P6 PPMs, run
// init + compute_flow through the drop-in class, print the time of that window, write flow.flo.
//
//   runeppm [options] [img1.ppm img2.ppm [out.flo]]          (defaults: frame10.ppm frame11.ppm flow.flo)
//
//   --size WxH        synthetic pair instead of files: smooth value noise, image 2 = image 1 translated by
//                     (+5,-3) px; the end-point error against that translation is printed
//   --seed N          PatchMatch RNG seed (1234, bao_pmflow_kernel.cu:68); also seeds the synthetic images
//   --levels N        pyramid depth (PYR_MAX_DEPTH 3, defs.h:31)
//   --patch-r N       patch radius (PATCH_R 9, defs.h:44)
//   --iters N         PatchMatch iterations (NUM_ITER 10, defs.h:45)
//   --propagation M   0 segmented sweeps (live in the reference), 1 jump flood, 2 4-neighbour
//   --stop-level N    draft mode: the levels below N are upsampled edge-aware instead of refined; 0 (default) the
//                     full path, at most levels - 1
//   --pairs P         process the pair P times in steady state (set_data + compute_flow); throughput is printed
//   --gpus G          G worker threads, one context per GPU; the P pairs are dealt round-robin (pair i -> GPU i mod G)
//   --batch B         each worker runs its pairs B at a time through a batch context (eppm_create_batch: every kernel launch
//                     covers the B pairs); default 1 = the drop-in class, one pair per launch
//   --pin             set_option("pin_caller_buffers", 1): the class registers the image and flow blocks for DMA, no host copies
//   --out file.flo    output name (same as the third positional argument)
//   --gt file.flo     print EPE / AAE of the result against a ground-truth .flo (bao_flow_tools.cpp:64-111)
//   --backward f.flo  the timed window runs compute_flow_bidirectional instead: also write the backward flow (image 2 -> image 1)
//   --occlusion f.pgm ... and image 1's occlusion mask as a P5 PGM: 0 consistent, 255 inconsistent, 128 leaves the frame, 64 unknown
//   --interpolate T f.ppm  (repeatable) implies the bidirectional call; after the timed window, write the frame at time T in [0, 1]
//                     between image 1 and image 2 (interpolate_frame) as a P6 PPM
//   --motion-blur S f.ppm  after the timed window, write image 1 as a camera whose shutter stays open for S of the frame interval
//                     (0 < S <= 1) would have recorded it: blurred along the forward flow (eppm_motion_blur), as
//                     a P6 PPM.  --blur-radius R (1 .. 31, default 16): the longest half-vector in pixels; --blur-taps N (1 .. 32,
//                     default 8): taps to each side of a pixel
//   --rolling-shutter R f.ppm  after the timed window, write image 1 as a global shutter would have recorded it, R (-1 .. 1) being the
//                     share of the frame interval the sensor takes to read a frame (negative: last line first): corrected along the
//                     forward flow (eppm_rolling_shutter), as a P6 PPM.  --rs-anchor A (0 .. 1, default 0.5): the
//                     position along the readout axis whose sampling time is the frame's; --rs-iters N (1 .. 8, default 3): fixed-point
//                     steps; --rs-columns: columns are read one after another, not rows.  Not together with --motion-blur.
//
//   runeppm [options] --sequence f0.ppm f1.ppm f2.ppm ... --out-prefix P [--temporal 0|1]
//   runeppm [options] --sequence clip.y4m --out-prefix P [--y4m-out] [--yuv-matrix 601|709|2020] ...
//
//                     a single --sequence argument that ends in .y4m is the clip: its 4:2:0 frames go into the
//                     context as they are (eppm_yuv_set_images / eppm_yuv_push_image: half the bytes of RGB over PCIe, converted on the
//                     device).  --y4m-out: every frame product of the run is written as ONE file per product in the input's format and
//                     rate (without a y4m input: 8 bit, BT.709, limited range, 25:1) instead of numbered PPMs -- P_dn.y4m, P_st.y4m,
//                     P_fk.y4m, P_df.y4m, P_mb.y4m, P_pl.y4m, P_ro.y4m; flows, masks and text outputs are unchanged.  --yuv-matrix:
//                     the matrix of input and output instead of the default by size (601 below 720 rows, else 709).
//
//                     a clip through ONE context: the first pair by eppm_set_images, every later frame by
//                     eppm_push_image; the flow of frames k-1 -> k is written to P_<k as four digits>.flo (P_0001.flo ...).
//                     --temporal 1 (default): every pair after the first starts PatchMatch from the previous pair's result moved
//                     along its motion; 0: every pair is a cold run (bit for bit the two-image form's flow).  Of the options above
//                     --seed, --levels, --patch-r, --iters, --propagation and --stop-level apply.
//                     --denoise: every pair runs the bidirectional call (the forward flows written are the same) followed by one step
//                     of the motion-compensated temporal filter; the filtered frames are written to
//                     P_dn_0000.ppm (the first frame itself), P_dn_0001.ppm ...  --denoise-thresh T (default 40) and
//                     --denoise-frames N (the longest average, default 8) set its parameters and imply --denoise.
//                     --remove-defects: every pair runs the bidirectional call followed by one step of the defect filter (DESIGN.md
//                     section 23): single-frame blotches of frame k - 1 are concealed from frames k - 2 and k.  The frames are written
//                     to P_df_0000.ppm ..., their masks (0 untouched, 1 hit, 2 grown) to P_dfm_0000.pgm ..., and P_defects.txt gets one
//                     line per frame: its index and the counts hit, grown, second_chance, undecided.  The first and the last frame of
//                     the clip (and, with --auto-cut, of every shot) are written as they are.  --defect-thresh D A (defaults 60 30),
//                     --defect-radius R (0 .. 4, default 3) and --defect-grow G (0 .. 4, default 1) set its parameters and imply it.
//                     --deflicker: every pair runs the bidirectional call followed by one step of flicker removal (DESIGN.md section
//                     24): frame k is corrected towards the corrected frame k - 1 by a gain and an offset per colour on a grid of cells.
//                     The frames are written to P_fk_0000.ppm (the first frame itself), P_fk_0001.ppm ...  --flicker-cell N (16, 32 or
//                     64, default 32) and --flicker-keep K (0 .. 1, default 1: how much of the correction is applied) imply it.
//                     --stabilize: every pair runs the bidirectional call followed by one step of the stabiliser (DESIGN.md section 16:
//                     the camera motion fitted to the forward flow, the frame re-rendered from the smoothed camera path); the frames are
//                     written to P_st_0000.ppm (the first frame itself), P_st_0001.ppm ...  --smooth S (0 .. 1, default 0.9; 1: tripod
//                     lock) sets the smoothing and implies --stabilize.
//                     --auto-cut: every pair runs the bidirectional call followed by one step of the cut detector (DESIGN.md section
//                     17); a frame that starts another shot restarts the flow's temporal prior and, with --denoise / --stabilize, the
//                     filter and the camera path.  P_cuts.txt gets one line per pair: its index, the verdict and the record's integers
//                     (n, c1[0..3], c2[0..3], n_tracked, sad).  --cut-lost N (0 .. 1000, default 530) sets the share of lost pixels,
//                     in permille, above which a pair is a cut, and implies --auto-cut.
//                     --motion-blur S (no file name here): every frame with the synthetic shutter is written to
//                     P_mb_0000.ppm, P_mb_0001.ppm ...: frame k - 1 blurred along the forward flow of the pair k - 1 -> k; the last pair
//                     runs the bidirectional call and gives the clip's last frame too, blurred along its backward flow.  --blur-radius
//                     and --blur-taps as above.
//                     --rolling-shutter R (no file name here): every frame with its rolling-shutter distortion removed (DESIGN.md section
//                     27) is written to P_rs_0000.ppm, P_rs_0001.ppm ... (P_rs.y4m with --y4m-out), from the same flows as --motion-blur's
//                     frames.  --rs-anchor, --rs-iters and --rs-columns as above.  It is a mode of its own: the other filters,
//                     --auto-cut and --deinterlace do not combine with it.
//                     --propagate layer.ppm alpha.ppm: a layer painted on the first frame follows the surface through the clip
//                     (DESIGN.md section 19): every pair runs the bidirectional call followed by one step of a correspondence map to
//                     the first frame, and the layer (alpha: the first channel of the second file), sampled once at the map, is
//                     composited over every frame: P_pl_0000.ppm (through the identity), P_pl_0001.ppm ...  With --auto-cut a frame
//                     that starts another shot re-anchors the map, and from there on the frames are written as they are.
//                     --objects: every pair runs the bidirectional call followed by one step of the object detector (DESIGN.md section
//                     20: the connected components of what moves against the camera).  P_ob_0001.pgm ... get the label bytes of every
//                     pair's first frame, P_objects.txt one line per object: the pair's index, id, age, area, the box x0 y0 x1 y1, the
//                     centroid and the mean velocity in pixels per frame (nan nan without a valid vector).  --min-area N and
//                     --max-objects N (1 .. 255) set its parameters and imply --objects.  With --auto-cut nothing is carried across a
//                     cut: the objects after it take new ids.
//                     --plate: every pair runs the bidirectional call followed by one step of a background plate (DESIGN.md section
//                     22): P_plate.ppm is the scene behind the moving objects in the first frame's coordinates, with --plate-margin MX
//                     MY on a canvas that much larger on every side (a panning camera), P_plate_cov.pgm how often each of its pixels
//                     was confirmed (0: never seen).  --remove-objects (implies --plate): a second pass renders every frame against
//                     the finished plate: P_ro_0000.ppm ... are the frames with their moving objects painted out; the frames, masks and
//                     paths of the first pass are kept in host memory.  The last frame has no pair of its own and is written unchanged.
//                     --deinterlace: the clip is interlaced.  Every frame is split into its two fields, every
//                     field is bobbed to full height on the host, and the 2n field frames go through the context: every pair runs the
//                     bidirectional call followed by one deinterlacer step.  P_di_0000.ppm (field frame 0 itself), P_di_0001.ppm ... are
//                     the 2n progressive frames at field rate; --single-rate keeps one frame per first field (n frames).  With
//                     --y4m-out they go to P_di.y4m at twice the input's frame rate (--single-rate: at the input's).  The field order
//                     of a y4m clip is its header's (It / Ib; an interlaced y4m clip is accepted only with --deinterlace); a PPM
//                     sequence, or a y4m clip that calls itself progressive, is top field first unless --bff says bottom field first.
//                     --deint-thresh N (0 .. 765, default 24) sets the gate and implies --deinterlace.  It is a mode of its own: the
//                     other filters and --auto-cut do not combine with it, and no .flo files are written.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bao_flow_patchmatch_multiscale_cuda.h"
#include "eppm.h"
#include "eppm_yuv.h"
#include "eppm_deint.h"
#include "eppm_rshutter.h"

template <typename T>
struct Array3 {       // bao_alloc<T>(n,r,c): one contiguous block reachable through row-pointer tables (bao_basic.h:146-162)
    std::vector<T> store;
    std::vector<T*> rows;
    std::vector<T**> planes;
    Array3(int n, int r, int c) : store((size_t)n * r * c), rows((size_t)n * r), planes(n)
    {
        for (int i = 0; i < n; i++)
            for (int j = 0; j < r; j++) rows[(size_t)i * r + j] = &store[((size_t)i * r + j) * c];
        for (int i = 0; i < n; i++) planes[i] = &rows[(size_t)i * r];
    }
    T*** p() { return planes.data(); }
};

struct Options {
    const char *f1 = "frame10.ppm", *f2 = "frame11.ppm", *fo = "flow.flo", *gt = nullptr, *fb = nullptr, *focc = nullptr;
    int sw = 0, sh = 0, pairs = 1, gpus = 1, batch = 1;
    std::vector<std::pair<std::string, long long>> opts;
    std::vector<std::pair<float, const char*>> interp;     // --interpolate T file.ppm
    std::vector<const char*> seq;                           // --sequence frames
    const char* prefix = nullptr;                           // --out-prefix
    int temporal = 1;                                       // --temporal
    int stop_level = 0;                                     // --stop-level
    bool denoise = false;                                   // --denoise
    float dn_thresh = 40.0f;                                // --denoise-thresh
    int dn_frames = 8;                                      // --denoise-frames
    bool defects = false;                                   // --remove-defects
    eppm_defect_params df = {60.0f, 30.0f, 3, 1};           // --defect-thresh, --defect-radius, --defect-grow
    bool deflicker = false;                                 // --deflicker
    int fk_cell = 32;                                       // --flicker-cell
    float fk_keep = 1.0f;                                   // --flicker-keep
    bool stabilize = false;                                 // --stabilize
    float smooth = 0.9f;                                    // --smooth
    bool auto_cut = false;                                  // --auto-cut
    int cut_lost = 530;                                     // --cut-lost
    bool mblur = false;                                     // --motion-blur
    const char* mblur_file = nullptr;                       // ... its file (the two-image form)
    eppm_mblur_params mb = {0.5f, 16.0f, 8};                // --motion-blur S, --blur-radius, --blur-taps
    bool mb_set = false;                                    // --blur-radius or --blur-taps given
    bool rs = false;                                        // --rolling-shutter
    const char* rs_file = nullptr;                          // ... its file (the two-image form)
    eppm_rs_params rsp = {0.5f, 0.5f, 3, 0};                // --rolling-shutter R, --rs-anchor, --rs-iters, --rs-columns
    bool rs_set = false;                                    // --rs-anchor, --rs-iters or --rs-columns given
    const char *pl_layer = nullptr, *pl_alpha = nullptr;    // --propagate layer.ppm alpha.ppm
    bool objects = false;                                   // --objects
    bool plate = false, remove_objects = false;             // --plate, --remove-objects
    int plate_mx = 0, plate_my = 0;                         // --plate-margin
    int ob_min_area = 0, ob_max = 0;                        // --min-area, --max-objects (0: the default)
    bool y4m_out = false;                                   // --y4m-out
    int yuv_matrix = -1;                                    // --yuv-matrix (-1: the default by size)
    bool deint = false, bff = false, single_rate = false;   // --deinterlace, --bff, --single-rate
    int di_thresh = 24;                                     // --deint-thresh
};

static unsigned hash32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// smooth value noise, three octaves, per channel
static void synth_image(unsigned char* rgb, int h, int w, int ox, int oy, unsigned seed)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                float acc = 0.f, amp = 1.f, tot = 0.f;
                for (int o = 0; o < 3; o++) {
                    const int cell = 32 >> (2 * o);
                    const float fx = (float)(x + ox + 4096) / cell, fy = (float)(y + oy + 4096) / cell;
                    const int ix = (int)fx, iy = (int)fy;
                    const float tx = fx - ix, ty = fy - iy;
                    float v[2][2];
                    for (int b = 0; b < 2; b++)
                        for (int a = 0; a < 2; a++)
                            v[b][a] = (hash32((unsigned)(ix + a) * 73856093u ^ (unsigned)(iy + b) * 19349663u ^ (unsigned)(c + 3 * o) * 83492791u ^ seed) & 0xffff) / 65535.f;
                    const float sx = tx * tx * (3 - 2 * tx), sy = ty * ty * (3 - 2 * ty);
                    acc += amp * ((v[0][0] * (1 - sx) + v[0][1] * sx) * (1 - sy) + (v[1][0] * (1 - sx) + v[1][1] * sx) * sy);
                    tot += amp;
                    amp *= 0.5f;
                }
                rgb[((size_t)y * w + x) * 3 + c] = (unsigned char)(255.f * acc / tot);
            }
}

static bool apply_opt(eppm_params& p, const std::string& name, long long v)
{
    if (name == "patch_r") p.patch_r = (int)v;
    else if (name == "num_iter") p.num_iter = (int)v;
    else if (name == "seed") p.seed = (unsigned long long)v;
    else if (name == "propagation") p.propagation = (int)v;
    else if (name == "levels") p.levels = (int)v;
    else if (name == "pin_caller_buffers" || name == "verify_tables_every_call" || name == "trust_verified_tables") return true;      // options of the class, not of eppm_params
    else return false;
    return true;
}

static int usage()
{
    fprintf(stderr, "usage: runeppm [--size WxH] [--seed N] [--levels N] [--patch-r N] [--iters N] [--propagation M] [--stop-level N]\n"
                    "               [--pin] [--pairs P] [--gpus G] [--batch B] [--gt file.flo] [--out file.flo] [--backward file.flo]\n"
                    "               [--occlusion file.pgm] [--interpolate T file.ppm]... [--motion-blur S file.ppm]\n"
                    "               [--blur-radius R] [--blur-taps N] [--rolling-shutter R file.ppm] [--rs-anchor A]\n"
                    "               [--rs-iters N] [--rs-columns] [img1.ppm img2.ppm [out.flo]]\n"
                    "       runeppm [--seed N] [--levels N] [--patch-r N] [--iters N] [--propagation M] [--stop-level N]\n"
                    "               --sequence f0.ppm f1.ppm [f2.ppm ...] --out-prefix P [--temporal 0|1]\n"
                    "               [--denoise] [--denoise-thresh T] [--denoise-frames N] [--stabilize] [--smooth S]\n"
                    "               [--auto-cut] [--cut-lost N] [--motion-blur S] [--blur-radius R] [--blur-taps N]\n"
                    "               [--propagate layer.ppm alpha.ppm] [--objects] [--min-area N] [--max-objects N]\n"
                    "               [--plate] [--plate-margin MX MY] [--remove-objects]\n"
                    "               [--remove-defects] [--defect-thresh D A] [--defect-radius R] [--defect-grow G]\n"
                    "               [--deflicker] [--flicker-cell N] [--flicker-keep K]\n"
                    "               [--deinterlace] [--bff] [--deint-thresh N] [--single-rate]\n"
                    "               [--rolling-shutter R] [--rs-anchor A] [--rs-iters N] [--rs-columns]\n"
                    "               --sequence clip.y4m --out-prefix P [--y4m-out] [--yuv-matrix 601|709|2020] [the options above]\n");
    return 2;
}

static bool write_ppm(const char* name, const unsigned char* rgb, int h, int w)
{
    FILE* f = fopen(name, "wb");
    if (!f) return false;
    bool ok = fprintf(f, "P6\n%d %d\n255\n", w, h) > 0 && fwrite(rgb, 1, (size_t)h * w * 3, f) == (size_t)h * w * 3;
    ok = fclose(f) == 0 && ok;
    return ok;
}

static bool ends_with(const char* s, const char* tail)
{
    const size_t n = strlen(s), m = strlen(tail);
    return n >= m && !strcmp(s + n - m, tail);
}

// One frame of I420 planes in one block, as the y4m calls and the context's YUV calls take them
struct YuvBuf {
    std::vector<unsigned char> mem;
    void* planes[3] = {nullptr, nullptr, nullptr};
    size_t strides[3] = {0, 0, 0};
    bool init(const eppm_yuv_format& f, int h, int w)
    {
        int rows[3], bytes[3];
        size_t total = 0;
        for (int p = 0; p < 3; p++) {
            if (eppm_yuv_plane_dims(&f, h, w, p, &rows[p], &bytes[p]) != EPPM_OK) return false;
            total += (size_t)rows[p] * bytes[p];
        }
        mem.assign(total, 0);
        size_t off = 0;
        for (int p = 0; p < 3; p++) { planes[p] = mem.data() + off; strides[p] = (size_t)bytes[p]; off += (size_t)rows[p] * bytes[p]; }
        return true;
    }
};

// Where the frame products of a clip go: numbered PPMs P_<tag>_<index>.ppm, or with --y4m-out one file P_<tag>.y4m per product, opened by
// the product's first frame and closed with the run.  A product's frames arrive in the order of their indices.
struct FrameOut {
    const char* prefix = nullptr;
    bool y4m = false;
    eppm_yuv_format fmt;
    int h = 0, w = 0, fps_num = 25, fps_den = 1;
    std::vector<std::pair<std::string, eppm_y4m*>> files;
    YuvBuf buf;
    ~FrameOut() { close(); }
    // closes every file; false if one could not be finished (the run then fails: a short file is no result)
    bool close()
    {
        bool ok = true;
        for (auto& f : files) ok = (eppm_y4m_close(f.second) == EPPM_OK) && ok;
        files.clear();
        return ok;
    }
    // the name of a product's first frame, or of its file, for the run's messages
    std::string first(const char* tag) const { return std::string(prefix) + "_" + tag + (y4m ? ".y4m" : "_0000.ppm ..."); }
    // name: the file written (or that could not be), for the caller's message
    bool put(const char* tag, size_t index, const unsigned char* rgb, char* name, size_t name_size)
    {
        if (!y4m) {
            snprintf(name, name_size, "%s_%s_%04zu.ppm", prefix, tag, index);
            return write_ppm(name, rgb, h, w);
        }
        snprintf(name, name_size, "%s_%s.y4m", prefix, tag);
        eppm_y4m* out = nullptr;
        for (auto& f : files) if (f.first == tag) out = f.second;
        if (!out) {
            if (buf.mem.empty() && !buf.init(fmt, h, w)) return false;
            if (eppm_y4m_open_write(&out, name, h, w, &fmt, fps_num, fps_den) != EPPM_OK) return false;
            files.emplace_back(tag, out);
        }
        return eppm_yuv_from_rgb_host(&fmt, rgb, (size_t)w * 3, buf.planes, buf.strides, h, w) == EPPM_OK &&
               eppm_y4m_write_frame(out, buf.planes, buf.strides) == EPPM_OK;
    }
};

// --sequence: the clip through one context of the C ABI (frame push, temporal mode; --denoise: the temporal filter on top; --stabilize:
// the stabiliser on top)
static int run_sequence(const Options& o)
{
    eppm_params prm;
    eppm_default_params(&prm);
    for (auto& kv : o.opts) {
        if (kv.first == "seed") prm.seed = (unsigned long long)kv.second;
        else if (kv.first == "levels") prm.levels = (int)kv.second;
        else if (kv.first == "patch_r") prm.patch_r = (int)kv.second;
        else if (kv.first == "num_iter") prm.num_iter = (int)kv.second;
        else if (kv.first == "propagation") prm.propagation = (int)kv.second;
    }
    int h = 0, w = 0, nch = 3;
    // a y4m clip: counted once (the last pair is told apart from the others), then read frame by frame
    struct Y4mGuard { eppm_y4m* p = nullptr; ~Y4mGuard() { eppm_y4m_close(p); } } yin;
    const bool y4m_in = o.seq.size() == 1;
    FrameOut frames_out;
    eppm_yuv_default_format(&frames_out.fmt);
    frames_out.fmt.layout = EPPM_YUV_I420;
    size_t nframes = o.seq.size();
    YuvBuf yuv[2];
    if (y4m_in) {
        eppm_yuv_format f;
        for (int pass = 0; pass < 2; pass++) {
            if (eppm_y4m_open_read(&yin.p, o.seq[0], &h, &w, &f, &frames_out.fps_num, &frames_out.fps_den) != EPPM_OK) { fprintf(stderr, "%s\n", eppm_last_error()); return 1; }
            if (pass == 1) break;
            if (!yuv[0].init(f, h, w) || !yuv[1].init(f, h, w)) { fprintf(stderr, "%s\n", eppm_last_error()); return 1; }
            int got = 1;
            for (nframes = 0; got; nframes += (size_t)got)
                if (eppm_y4m_read_frame(yin.p, yuv[0].planes, yuv[0].strides, &got) != EPPM_OK) { fprintf(stderr, "%s: %s\n", o.seq[0], eppm_last_error()); return 1; }
            eppm_y4m_close(yin.p);
            yin.p = nullptr;
        }
        if (nframes < 2) { fprintf(stderr, "%s: a clip needs at least two frames\n", o.seq[0]); return 1; }
        if (frames_out.fps_num < 1 || frames_out.fps_den < 1) { frames_out.fps_num = 25; frames_out.fps_den = 1; }
        frames_out.fmt = f;
    } else if (eppm_ppm_size(o.seq[0], &h, &w) != EPPM_OK) { fprintf(stderr, "cannot read %s\n", o.seq[0]); return 1; }
    if (o.yuv_matrix >= 0) frames_out.fmt.matrix = o.yuv_matrix;
    else if (!y4m_in) frames_out.fmt.matrix = EPPM_YUV_BT709;
    const eppm_yuv_format yfmt = frames_out.fmt;        // of the input (a y4m clip) and of --y4m-out
    frames_out.prefix = o.prefix; frames_out.y4m = o.y4m_out; frames_out.h = h; frames_out.w = w;
    std::vector<std::vector<unsigned char>> img(2, std::vector<unsigned char>((size_t)h * w * 3));
    std::vector<float> u((size_t)h * w), v((size_t)h * w);
    eppm_ctx* ctx = nullptr;
    eppm_tfilter* flt = nullptr;
    eppm_stab* stab = nullptr;
    eppm_cutdet* det = nullptr;
    eppm_cmap* cm = nullptr;
    eppm_objects* od = nullptr;
    struct PlateGuard { eppm_plate* p = nullptr; ~PlateGuard() { eppm_plate_destroy(p); } } plt;          // freed on every way out
    struct DefectGuard {                                                                                   // freed and closed on every way out
        eppm_defect* p = nullptr;
        FILE* txt = nullptr;
        ~DefectGuard() { eppm_defect_destroy(p); if (txt) fclose(txt); }
    } dfl;
    std::vector<unsigned char> df_rgb, df_mask;
    struct DeflickerGuard { eppm_deflicker* p = nullptr; ~DeflickerGuard() { eppm_deflicker_destroy(p); } } dfk;       // freed on every way out
    std::vector<unsigned char> fk_rgb;
    std::vector<std::vector<unsigned char>> ro_frames, ro_masks;          // --remove-objects: what the second pass needs of the first
    std::vector<std::vector<double>> ro_paths;
    FILE* cuts = nullptr;
    FILE* obf = nullptr;
    auto fail = [&](const char* what) { fprintf(stderr, "%s: %s\n", what, eppm_last_error()); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); if (ctx) eppm_destroy(ctx); return 1; };
    if (eppm_create(&ctx, h, w, 0, &prm) != EPPM_OK) return fail("eppm_create");
    std::vector<unsigned char> dn, st, mb, pl, layer;
    bool pl_drawn = true;               // --propagate: no cut so far
    if (o.mblur || o.rs) mb.resize((size_t)h * w * 3);
    char name[4096];
    if (o.stabilize) {
        eppm_stab_params sp;
        eppm_stab_default_params(&sp);
        sp.smooth = o.smooth;
        if (eppm_stab_create(ctx, &sp, &stab) != EPPM_OK) return fail("eppm_stab_create");
        st.resize((size_t)h * w * 3);
    }
    if (o.denoise) {
        const eppm_tfilter_params tp = {o.dn_thresh, o.dn_frames};
        if (eppm_tfilter_create(ctx, &tp, &flt) != EPPM_OK) return fail("eppm_tfilter_create");
        dn.resize((size_t)h * w * 3);
    }
    if (o.defects) {
        if (eppm_defect_create(ctx, &o.df, &dfl.p) != EPPM_OK) return fail("eppm_defect_create");
        df_rgb.resize((size_t)h * w * 3);
        df_mask.resize((size_t)h * w);
        snprintf(name, sizeof name, "%s_defects.txt", o.prefix);
        if (!(dfl.txt = fopen(name, "w"))) { fprintf(stderr, "cannot write %s\n", name); return fail("fopen"); }
    }
    if (o.deflicker) {
        eppm_deflicker_params fp;
        eppm_deflicker_default_params(&fp);
        fp.cell = o.fk_cell;
        fp.keep = o.fk_keep;
        if (eppm_deflicker_create(ctx, &fp, &dfk.p) != EPPM_OK) return fail("eppm_deflicker_create");
        fk_rgb.resize((size_t)h * w * 3);
    }
    // one frame of --remove-defects: the frame, its mask and its line of counts
    auto write_defects = [&](size_t frame, const unsigned char* rgb, const unsigned char* mask, const eppm_defect_stats& ds) {
        if (!frames_out.put("df", frame, rgb, name, sizeof name)) return false;
        snprintf(name, sizeof name, "%s_dfm_%04zu.pgm", o.prefix, frame);
        FILE* f = fopen(name, "wb");
        bool ok = f && fprintf(f, "P5\n%d %d\n255\n", w, h) > 0 && fwrite(mask, 1, (size_t)h * w, f) == (size_t)h * w;
        if (f) ok = fclose(f) == 0 && ok;
        return ok && fprintf(dfl.txt, "%zu %d %d %d %d\n", frame, ds.hit, ds.grown, ds.second_chance, ds.undecided) > 0;
    };
    if (o.pl_layer) {
        int hl = 0, wl = 0;
        std::vector<unsigned char> rgb((size_t)h * w * 3), alpha((size_t)h * w * 3);
        for (int j = 0; j < 2; j++) {
            const char* f = j ? o.pl_alpha : o.pl_layer;
            if (eppm_ppm_size(f, &hl, &wl) != EPPM_OK || hl != h || wl != w || eppm_load_ppm(f, (j ? alpha : rgb).data(), h, w, &nch) != EPPM_OK) {
                fprintf(stderr, "cannot read %s (or its size differs from the first frame's)\n", f);
                eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx);
                return 1;
            }
        }
        layer.resize((size_t)h * w * 4);
        for (size_t i = 0; i < (size_t)h * w; i++) {
            for (int c = 0; c < 3; c++) layer[4 * i + c] = rgb[3 * i + c];
            layer[4 * i + 3] = alpha[3 * i];
        }
        if (eppm_cmap_create(ctx, nullptr, &cm) != EPPM_OK) return fail("eppm_cmap_create");
        pl.resize((size_t)h * w * 3);
    }
    if (o.auto_cut) {
        eppm_cut_params cp;
        eppm_cutdet_default_params(&cp);
        cp.lost_permille = o.cut_lost;
        if (eppm_cutdet_create(ctx, &cp, &det) != EPPM_OK) return fail("eppm_cutdet_create");
        snprintf(name, sizeof name, "%s_cuts.txt", o.prefix);
        if (!(cuts = fopen(name, "w"))) { fprintf(stderr, "cannot write %s\n", name); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
    }
    std::vector<unsigned char> ob_labels;
    std::vector<eppm_object> ob_rec;
    if (o.objects) {
        eppm_objects_params op;
        eppm_objects_default_params(&op);
        if (o.ob_min_area) op.min_area = o.ob_min_area;
        if (o.ob_max) op.max_objects = o.ob_max;
        if (eppm_objects_create(ctx, &op, &od) != EPPM_OK) return fail("eppm_objects_create");
        ob_labels.resize((size_t)h * w);
        ob_rec.resize(op.max_objects);
        snprintf(name, sizeof name, "%s_objects.txt", o.prefix);
        if (!(obf = fopen(name, "w"))) { fprintf(stderr, "cannot write %s\n", name); return fail("fopen"); }
    }
    if (o.plate) {
        eppm_plate_params pp;
        eppm_plate_default_params(&pp);
        pp.margin_x = o.plate_mx; pp.margin_y = o.plate_my;
        if (eppm_plate_create(ctx, &pp, &plt.p) != EPPM_OK) return fail("eppm_plate_create");
    }
    if (eppm_set_temporal(ctx, o.temporal) != EPPM_OK) return fail("eppm_set_temporal");
    if (eppm_set_stop_level(ctx, o.stop_level) != EPPM_OK) {
        fprintf(stderr, "--stop-level: %s\n", eppm_last_error());
        if (cuts) fclose(cuts); if (obf) fclose(obf);
        eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx);
        return usage();
    }
    double total = 0;
    for (size_t k = 0; k < nframes; k++) {
        int hk = 0, wk = 0;
        std::vector<unsigned char>& cur = img[k == 0 ? 0 : 1];
        if (y4m_in) {       // the planes for the context, and their RGB form (eppm_yuv_to_rgb_host: the bytes the context holds) for what reads the frame here
            YuvBuf& y = yuv[k == 0 ? 0 : 1];
            int got = 0;
            if (eppm_y4m_read_frame(yin.p, y.planes, y.strides, &got) != EPPM_OK || !got ||
                eppm_yuv_to_rgb_host(&yfmt, y.planes, y.strides, cur.data(), (size_t)w * 3, h, w) != EPPM_OK)
                return fail(o.seq[0]);
        } else if (eppm_ppm_size(o.seq[k], &hk, &wk) != EPPM_OK || hk != h || wk != w || eppm_load_ppm(o.seq[k], cur.data(), h, w, &nch) != EPPM_OK) {
            fprintf(stderr, "cannot read %s (or its size differs from the first frame's)\n", o.seq[k]);
            if (cuts) fclose(cuts); if (obf) fclose(obf);
            eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det);
            eppm_stab_destroy(stab);
            eppm_tfilter_destroy(flt);
            eppm_destroy(ctx);
            return 1;
        }
        if (o.remove_objects) ro_frames.push_back(cur);
        if (k == 0) {
            if (o.denoise) {
                if (!frames_out.put("dn", 0, cur.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
            }
            if (dfk.p) {
                if (!frames_out.put("fk", 0, cur.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
            }
            if (cm) {                  // the layer through the identity map: the first frame is its own anchor
                std::vector<float> seed((size_t)h * w * 2);
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++) { seed[((size_t)y * w + x) * 2] = (float)x; seed[((size_t)y * w + x) * 2 + 1] = (float)y; }
                if (eppm_cmap_set_state(cm, 0, seed.data(), cur.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_cmap_set_state");
                if (eppm_cmap_set_layer(cm, 0, layer.data(), (size_t)w * 4) != EPPM_OK) return fail("eppm_cmap_set_layer");
                if (eppm_cmap_render(cm, 0, pl.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_cmap_render");
                if (!frames_out.put("pl", 0, pl.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
            }
            if (o.stabilize) {
                if (!frames_out.put("st", 0, cur.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
            }
            continue;
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (y4m_in) {
            if (k == 1) { if (eppm_yuv_set_images(ctx, &yfmt, yuv[0].planes, yuv[1].planes, yuv[0].strides) != EPPM_OK) return fail("eppm_yuv_set_images"); }
            else if (eppm_yuv_push_image(ctx, &yfmt, yuv[1].planes, yuv[1].strides) != EPPM_OK) return fail("eppm_yuv_push_image");
        }
        else if (k == 1) { if (eppm_set_images(ctx, img[0].data(), img[1].data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_set_images"); }
        else if (eppm_push_image(ctx, cur.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_push_image");
        const bool last = k + 1 == nframes;
        if (!o.denoise && !o.stabilize && !o.auto_cut && !cm && !od && !plt.p && !dfl.p && !dfk.p && !((o.mblur || o.rs) && last)) { if (eppm_compute(ctx, u.data(), v.data()) != EPPM_OK) return fail("eppm_compute"); }
        else {
            if (eppm_compute_bidirectional(ctx, u.data(), v.data(), nullptr, nullptr, nullptr, nullptr) != EPPM_OK) return fail("eppm_compute_bidirectional");
            uint8_t cut = 0;
            if (o.auto_cut) {
                eppm_cut_stats cs;
                if (eppm_cutdet_step(det, ctx) != EPPM_OK) return fail("eppm_cutdet_step");
                if (eppm_cutdet_cuts(det, 1, &cut) != EPPM_OK) return fail("eppm_cutdet_cuts");
                if (eppm_cutdet_get(det, 0, &cs) != EPPM_OK) return fail("eppm_cutdet_get");
                if (cut && eppm_temporal_reset(ctx) != EPPM_OK) return fail("eppm_temporal_reset");
                fprintf(cuts, "%zu %d %lld", k - 1, (int)cs.cut, (long long)cs.n);
                for (int j = 0; j < 4; j++) fprintf(cuts, " %lld", (long long)cs.c1[j]);
                for (int j = 0; j < 4; j++) fprintf(cuts, " %lld", (long long)cs.c2[j]);
                fprintf(cuts, " %lld %lld\n", (long long)cs.n_tracked, (long long)cs.sad);
            }
            if (o.denoise && eppm_tfilter_step(flt, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_tfilter_step");
            if (o.stabilize && eppm_stab_step(stab, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_stab_step");
            if (dfk.p) {
                if (eppm_deflicker_step(dfk.p, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_deflicker_step");
                if (eppm_deflicker_get(dfk.p, 0, fk_rgb.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_deflicker_get");
                if (!frames_out.put("fk", k, fk_rgb.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
            }
            if (dfl.p) {                // the step of pair (k - 1, k) gives frame k - 1
                eppm_defect_stats ds;
                if (eppm_defect_step(dfl.p, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_defect_step");
                if (eppm_defect_get(dfl.p, 0, df_rgb.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_defect_get");
                if (eppm_defect_get_mask(dfl.p, 0, df_mask.data()) != EPPM_OK) return fail("eppm_defect_get_mask");
                if (eppm_defect_get_stats(dfl.p, 0, &ds) != EPPM_OK) return fail("eppm_defect_get_stats");
                if (!write_defects(k - 1, df_rgb.data(), df_mask.data(), ds)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
                if (last) {             // the clip's last frame has no next neighbour
                    std::fill(df_mask.begin(), df_mask.end(), 0);
                    if (!write_defects(k, cur.data(), df_mask.data(), eppm_defect_stats{0, 0, 0, 0})) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
                }
            }
            if (cm) {
                if (eppm_cmap_step(cm, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_cmap_step");
                if (cut) pl_drawn = false;              // the layer belongs to the first shot
                if (pl_drawn) { if (eppm_cmap_render(cm, 0, pl.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_cmap_render"); }
                else pl = cur;
            }
            if (od) {
                eppm_objects_counts oc;
                if (eppm_objects_step(od, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_objects_step");
                if (eppm_objects_get(od, 0, (int)ob_rec.size(), ob_rec.data(), &oc) != EPPM_OK) return fail("eppm_objects_get");
                if (eppm_objects_get_labels(od, 0, ob_labels.data()) != EPPM_OK) return fail("eppm_objects_get_labels");
                for (int j = 0; j < oc.n; j++) {
                    const eppm_object& r = ob_rec[j];
                    fprintf(obf, "%zu %d %d %d %d %d %d %d %.6f %.6f", k - 1, r.id, r.age, r.area, r.x0, r.y0, r.x1, r.y1, (double)r.sum_x / r.area,
                            (double)r.sum_y / r.area);
                    if (r.n_flow) fprintf(obf, " %.6f %.6f\n", (double)r.sum_qu / (256.0 * r.n_flow), (double)r.sum_qv / (256.0 * r.n_flow));
                    else fprintf(obf, " nan nan\n");
                }
                snprintf(name, sizeof name, "%s_ob_%04zu.pgm", o.prefix, k);
                FILE* f = fopen(name, "wb");
                bool ok = f && fprintf(f, "P5\n%d %d\n255\n", w, h) > 0 && fwrite(ob_labels.data(), 1, ob_labels.size(), f) == ob_labels.size();
                if (f) ok = fclose(f) == 0 && ok;
                if (!ok) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
            }
            if (plt.p) {
                if (o.remove_objects) {              // the path that ends at this pair's image 1, before the step advances it
                    ro_paths.emplace_back(6);
                    if (eppm_plate_get_path(plt.p, 0, ro_paths.back().data()) != EPPM_OK) return fail("eppm_plate_get_path");
                }
                if (eppm_plate_step(plt.p, ctx, o.auto_cut ? &cut : nullptr) != EPPM_OK) return fail("eppm_plate_step");
                if (o.remove_objects) {
                    ro_masks.emplace_back((size_t)h * w);
                    if (eppm_plate_get_mask(plt.p, 0, ro_masks.back().data()) != EPPM_OK) return fail("eppm_plate_get_mask");
                }
            }
            if (o.denoise && eppm_tfilter_get(flt, 0, dn.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_tfilter_get");
            if (o.stabilize && eppm_stab_get(stab, 0, st.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_stab_get");
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        total += ms;
        snprintf(name, sizeof name, "%s_%04zu.flo", o.prefix, k);
        if (eppm_save_flo(name, u.data(), v.data(), h, w) != EPPM_OK) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
        printf("pair %zu: %.3f ms%s -> %s\n", k, ms, (o.temporal && k > 1) ? " (seeded)" : "", name);
        if (o.denoise) {
            if (!frames_out.put("dn", k, dn.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
        }
        if (o.stabilize) {
            if (!frames_out.put("st", k, st.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
        }
        if (cm) {
            if (!frames_out.put("pl", k, pl.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
        }
        for (int fr = 0; o.mblur && fr <= (last ? 1 : 0); fr++) {       // frame k - 1 from the forward flow; the clip's last frame from the backward flow
            if (eppm_motion_blur(ctx, &o.mb, fr, mb.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_motion_blur");
            if (!frames_out.put("mb", k - 1 + fr, mb.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); if (cuts) fclose(cuts); if (obf) fclose(obf); eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det); eppm_stab_destroy(stab); eppm_tfilter_destroy(flt); eppm_destroy(ctx); return 1; }
        }
        for (int fr = 0; o.rs && fr <= (last ? 1 : 0); fr++) {          // the same two windows for the rolling-shutter correction
            if (eppm_rolling_shutter(ctx, &o.rsp, fr, mb.data(), (size_t)w * 3) != EPPM_OK) return fail("eppm_rolling_shutter");
            if (!frames_out.put("rs", k - 1 + fr, mb.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
        }
    }
    printf("%zu pairs, %.3f ms per pair\n", nframes - 1, total / (double)(nframes - 1));
    if (plt.p) {
        int ch = 0, cw = 0;
        if (eppm_plate_canvas_dims(plt.p, &ch, &cw) != EPPM_OK) return fail("eppm_plate_canvas_dims");
        std::vector<unsigned char> canvas((size_t)ch * cw * 3), cov((size_t)ch * cw);
        if (eppm_plate_get(plt.p, 0, canvas.data(), (size_t)cw * 3, cov.data()) != EPPM_OK) return fail("eppm_plate_get");
        snprintf(name, sizeof name, "%s_plate.ppm", o.prefix);
        if (!write_ppm(name, canvas.data(), ch, cw)) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
        snprintf(name, sizeof name, "%s_plate_cov.pgm", o.prefix);
        FILE* f = fopen(name, "wb");
        bool ok = f && fprintf(f, "P5\n%d %d\n255\n", cw, ch) > 0 && fwrite(cov.data(), 1, cov.size(), f) == cov.size();
        if (f) ok = fclose(f) == 0 && ok;
        if (!ok) { fprintf(stderr, "cannot write %s\n", name); return fail("write"); }
        printf("plate %dx%d -> %s_plate.ppm, %s_plate_cov.pgm\n", cw, ch, o.prefix, o.prefix);
    }
    if (o.remove_objects) {              // the second pass: every frame against the finished plate, on device planes of our own
        const size_t px = (size_t)h * w;
        void* d[4] = {nullptr, nullptr, nullptr, nullptr};          // frame (RGBA), mask, output (RGBA), fill
        const size_t bytes[4] = {px * 4, px, px * 4, px};
        auto release = [&]() { for (void* p : d) if (p) eppm_free_device(p); };
        for (int j = 0; j < 4; j++)
            if (eppm_malloc_device(&d[j], bytes[j]) != EPPM_OK) { release(); return fail("eppm_malloc_device"); }
        std::vector<unsigned char> rgba(px * 4), out(px * 3);
        size_t filled = 0;
        for (size_t k = 0; k < ro_frames.size(); k++) {
            out = ro_frames[k];
            if (k < ro_masks.size()) {
                for (size_t i = 0; i < px; i++) { rgba[4 * i] = out[3 * i]; rgba[4 * i + 1] = out[3 * i + 1]; rgba[4 * i + 2] = out[3 * i + 2]; rgba[4 * i + 3] = 0; }
                if (eppm_memcpy_h2d(d[0], rgba.data(), bytes[0]) != EPPM_OK || eppm_memcpy_h2d(d[1], ro_masks[k].data(), bytes[1]) != EPPM_OK ||
                    eppm_plate_render_frames(plt.p, 0, d[0], (size_t)w * 4, (const uint8_t*)d[1], ro_paths[k].data(), d[2], (size_t)w * 4, (uint8_t*)d[3]) != EPPM_OK ||
                    eppm_memcpy_d2h(rgba.data(), d[2], bytes[2]) != EPPM_OK || eppm_memcpy_d2h(ro_masks[k].data(), d[3], bytes[3]) != EPPM_OK) {
                    release();
                    return fail("eppm_plate_render_frames");
                }
                for (size_t i = 0; i < px; i++) { out[3 * i] = rgba[4 * i]; out[3 * i + 1] = rgba[4 * i + 1]; out[3 * i + 2] = rgba[4 * i + 2]; filled += ro_masks[k][i] == 1; }
            }
            if (!frames_out.put("ro", k, out.data(), name, sizeof name)) { fprintf(stderr, "cannot write %s\n", name); release(); return fail("write"); }
        }
        release();
        printf("%zu frames with %zu pixels filled from the plate -> %s\n", ro_frames.size(), filled, frames_out.first("ro").c_str());
    }
    const bool dft_ok = !dfl.txt || fclose(dfl.txt) == 0;
    dfl.txt = nullptr;
    if (!dft_ok) { fprintf(stderr, "cannot write %s_defects.txt\n", o.prefix); return fail("write"); }
    const bool cuts_ok = !cuts || fclose(cuts) == 0;
    const bool obf_ok = !obf || fclose(obf) == 0;
    const bool frames_ok = frames_out.close();
    eppm_plate_destroy(plt.p);
    plt.p = nullptr;
    eppm_defect_destroy(dfl.p);
    dfl.p = nullptr;
    eppm_deflicker_destroy(dfk.p);
    dfk.p = nullptr;
    eppm_objects_destroy(od); eppm_cmap_destroy(cm); eppm_cutdet_destroy(det);
    eppm_stab_destroy(stab);
    eppm_tfilter_destroy(flt);
    eppm_destroy(ctx);
    if (!cuts_ok) { fprintf(stderr, "cannot write %s_cuts.txt\n", o.prefix); return 1; }
    if (!obf_ok) { fprintf(stderr, "cannot write %s_objects.txt\n", o.prefix); return 1; }
    if (!frames_ok) { fprintf(stderr, "cannot finish the y4m files of %s: %s\n", o.prefix, eppm_last_error()); return 1; }
    return 0;
}

// --sequence ... --deinterlace: an interlaced clip as progressive frames at field rate.  The calls are those of
// eppm_amd.deinterlace_sequence: split, bob on the host, set_images / push_image, the bidirectional call, one deinterlacer step per pair
static int run_deinterlace(const Options& o)
{
    eppm_params prm;
    eppm_default_params(&prm);
    for (auto& kv : o.opts) {
        if (kv.first == "seed") prm.seed = (unsigned long long)kv.second;
        else if (kv.first == "levels") prm.levels = (int)kv.second;
        else if (kv.first == "patch_r") prm.patch_r = (int)kv.second;
        else if (kv.first == "num_iter") prm.num_iter = (int)kv.second;
        else if (kv.first == "propagation") prm.propagation = (int)kv.second;
    }
    struct Guard {          // freed on every way out
        eppm_y4m* yin = nullptr;
        eppm_ctx* ctx = nullptr;
        eppm_deint* di = nullptr;
        ~Guard() { eppm_deint_destroy(di); if (ctx) eppm_destroy(ctx); eppm_y4m_close(yin); }
    } g;
    auto fail = [&](const char* what) { fprintf(stderr, "%s: %s\n", what, eppm_last_error()); return 1; };
    int h = 0, w = 0, nch = 3, interlace = 0;
    const bool y4m_in = o.seq.size() == 1 && ends_with(o.seq[0], ".y4m");
    FrameOut out;
    eppm_yuv_default_format(&out.fmt);
    out.fmt.layout = EPPM_YUV_I420;
    YuvBuf yuv;
    if (y4m_in) {
        if (eppm_deint_y4m_open_read(&g.yin, o.seq[0], &h, &w, &out.fmt, &out.fps_num, &out.fps_den, &interlace) != EPPM_OK) { fprintf(stderr, "%s\n", eppm_last_error()); return 1; }
        if (h % 4 != 0) { fprintf(stderr, "%s: --deinterlace needs a 4:2:0 clip whose height is a multiple of 4 (each field is a 4:2:0 picture), not %d\n", o.seq[0], h); return 1; }
        if (!yuv.init(out.fmt, h, w)) return fail("eppm_yuv_plane_dims");
        if (out.fps_num < 1 || out.fps_den < 1) { out.fps_num = 25; out.fps_den = 1; }
    } else {
        if (eppm_ppm_size(o.seq[0], &h, &w) != EPPM_OK) { fprintf(stderr, "cannot read %s\n", o.seq[0]); return 1; }
        out.fmt.matrix = EPPM_YUV_BT709;
    }
    if (h < 2) { fprintf(stderr, "--deinterlace needs frames of at least two rows\n"); return 1; }
    if (o.yuv_matrix >= 0) out.fmt.matrix = o.yuv_matrix;
    const eppm_yuv_format yfmt = out.fmt;
    const int first = interlace == 1 ? 0 : interlace == 2 ? 1 : (o.bff ? 1 : 0);        // the parity of the field that is first in time
    if (!o.single_rate) {
        if (out.fps_num > 0x3fffffff) { fprintf(stderr, "%s: the frame rate cannot be doubled\n", o.seq[0]); return 1; }
        out.fps_num *= 2;
    }
    out.prefix = o.prefix; out.y4m = o.y4m_out; out.h = h; out.w = w;
    const size_t row = (size_t)w * 3;
    std::vector<unsigned char> img((size_t)h * row), field((size_t)((h + 1) / 2) * row), prev((size_t)h * row), cur((size_t)h * row), rgb((size_t)h * row);
    if (eppm_create(&g.ctx, h, w, 0, &prm) != EPPM_OK) return fail("eppm_create");
    const eppm_deint_params dp = {o.di_thresh, 1};
    if (eppm_deint_create(g.ctx, &dp, &g.di) != EPPM_OK) return fail("eppm_deint_create");
    if (eppm_set_temporal(g.ctx, o.temporal) != EPPM_OK) return fail("eppm_set_temporal");
    if (eppm_set_stop_level(g.ctx, o.stop_level) != EPPM_OK) { fprintf(stderr, "--stop-level: %s\n", eppm_last_error()); return usage(); }
    char name[4096];
    size_t k = 0, written = 0;          // field frames so far, frames written
    double total = 0;
    for (size_t n = 0;; n++) {
        if (y4m_in) {
            int got = 0;
            if (eppm_y4m_read_frame(g.yin, yuv.planes, yuv.strides, &got) != EPPM_OK) return fail(o.seq[0]);
            if (!got) break;
        } else {
            if (n == o.seq.size()) break;
            int hk = 0, wk = 0;
            if (eppm_ppm_size(o.seq[n], &hk, &wk) != EPPM_OK || hk != h || wk != w || eppm_load_ppm(o.seq[n], img.data(), h, w, &nch) != EPPM_OK) {
                fprintf(stderr, "cannot read %s (or its size differs from the first frame's)\n", o.seq[n]);
                return 1;
            }
        }
        for (int j = 0; j < 2; j++, k++) {
            const int p = first ^ j, fh = (h - p + 1) / 2;
            if (y4m_in) {           // field p of every plane: its rows p, p + 2, ... (h % 4 == 0: h / 2 luma rows, h / 4 chroma rows)
                const void* planes[3];
                size_t strides[3];
                for (int q = 0; q < 3; q++) { planes[q] = (const unsigned char*)yuv.planes[q] + (size_t)p * yuv.strides[q]; strides[q] = 2 * yuv.strides[q]; }
                if (eppm_yuv_to_rgb_host(&yfmt, planes, strides, field.data(), row, fh, w) != EPPM_OK) return fail("eppm_yuv_to_rgb_host");
            } else
                for (int i = 0; i < fh; i++) memcpy(&field[(size_t)i * row], &img[(size_t)(2 * i + p) * row], row);
            prev.swap(cur);
            if (eppm_deint_bob_host(cur.data(), field.data(), h, w, p) != EPPM_OK) return fail("eppm_deint_bob_host");
            const unsigned char* frame = cur.data();
            if (k > 0) {
                const auto t0 = std::chrono::steady_clock::now();
                if (k == 1) { if (eppm_set_images(g.ctx, prev.data(), cur.data(), row) != EPPM_OK) return fail("eppm_set_images"); }
                else if (eppm_push_image(g.ctx, cur.data(), row) != EPPM_OK) return fail("eppm_push_image");
                if (eppm_compute_bidirectional_device(g.ctx, nullptr, nullptr, nullptr, nullptr) != EPPM_OK) return fail("eppm_compute_bidirectional_device");
                const uint8_t parity = (uint8_t)p;
                if (eppm_deint_step(g.di, g.ctx, nullptr, &parity) != EPPM_OK) return fail("eppm_deint_step");
                if (eppm_deint_get(g.di, 0, rgb.data(), row) != EPPM_OK) return fail("eppm_deint_get");
                total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                frame = rgb.data();
            }
            if (o.single_rate && j == 1) continue;
            if (!out.put("di", written++, frame, name, sizeof name)) { fprintf(stderr, "cannot write %s: %s\n", name, eppm_last_error()); return 1; }
        }
    }
    if (k == 0) { fprintf(stderr, "%s: a clip needs at least one frame\n", o.seq[0]); return 1; }
    if (!out.close()) { fprintf(stderr, "cannot finish the y4m files of %s: %s\n", o.prefix, eppm_last_error()); return 1; }
    printf("%zu field frames (%s field first), %.3f ms per pair, %zu frames -> %s\n", k, first ? "bottom" : "top", total / (double)(k - 1), written, out.first("di").c_str());
    return 0;
}

int main(int argc, char** argv)
{
    Options o;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        auto val = [&](long long* v) { if (i + 1 >= argc) return false; *v = atoll(argv[++i]); return true; };
        long long v = 0;
        if (!strcmp(a, "--size")) {
            if (i + 1 >= argc || sscanf(argv[++i], "%dx%d", &o.sw, &o.sh) != 2) return usage();
        } else if (!strcmp(a, "--seed")) { if (!val(&v)) return usage(); o.opts.push_back({"seed", v}); }
        else if (!strcmp(a, "--levels")) { if (!val(&v)) return usage(); o.opts.push_back({"levels", v}); }
        else if (!strcmp(a, "--patch-r")) { if (!val(&v)) return usage(); o.opts.push_back({"patch_r", v}); }
        else if (!strcmp(a, "--iters")) { if (!val(&v)) return usage(); o.opts.push_back({"num_iter", v}); }
        else if (!strcmp(a, "--propagation")) { if (!val(&v)) return usage(); o.opts.push_back({"propagation", v}); }
        else if (!strcmp(a, "--stop-level")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            const long n = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end || n < 0 || n > 1000) return usage();
            o.stop_level = (int)n;
        }
        else if (!strcmp(a, "--pairs")) { if (!val(&v) || v < 1) return usage(); o.pairs = (int)v; }
        else if (!strcmp(a, "--gpus")) { if (!val(&v) || v < 1) return usage(); o.gpus = (int)v; }
        else if (!strcmp(a, "--batch")) { if (!val(&v) || v < 1) return usage(); o.batch = (int)v; }
        else if (!strcmp(a, "--pin")) o.opts.push_back({"pin_caller_buffers", 1});
        else if (!strcmp(a, "--gt")) { if (i + 1 >= argc) return usage(); o.gt = argv[++i]; }
        else if (!strcmp(a, "--out")) { if (i + 1 >= argc) return usage(); o.fo = argv[++i]; }
        else if (!strcmp(a, "--backward")) { if (i + 1 >= argc) return usage(); o.fb = argv[++i]; }
        else if (!strcmp(a, "--occlusion")) { if (i + 1 >= argc) return usage(); o.focc = argv[++i]; }
        else if (!strcmp(a, "--interpolate")) {
            if (i + 2 >= argc) return usage();
            char* end = nullptr;
            const float t = strtof(argv[++i], &end);
            if (!end || *end || !(t >= 0.0f && t <= 1.0f)) return usage();
            o.interp.push_back({t, argv[++i]});
        }
        else if (!strcmp(a, "--motion-blur")) {       // the value, then (two-image form) the file: resolved once the form is known
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.mb.shutter = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.mb.shutter > 0.0f && o.mb.shutter <= 1.0f)) return usage();
            o.mblur = true;
            if (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-')) o.mblur_file = argv[++i];
        }
        else if (!strcmp(a, "--blur-radius")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.mb.max_radius = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.mb.max_radius >= 1.0f && o.mb.max_radius <= 31.0f)) return usage();
            o.mb_set = true;
        }
        else if (!strcmp(a, "--blur-taps")) { if (!val(&v) || v < 1 || v > 32) return usage(); o.mb.taps = (int)v; o.mb_set = true; }
        else if (!strcmp(a, "--rolling-shutter")) {   // the value, then (two-image form) the file, as --motion-blur
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.rsp.readout = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.rsp.readout >= -1.0f && o.rsp.readout <= 1.0f)) return usage();
            o.rs = true;
            if (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-')) o.rs_file = argv[++i];
        }
        else if (!strcmp(a, "--rs-anchor")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.rsp.anchor = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.rsp.anchor >= 0.0f && o.rsp.anchor <= 1.0f)) return usage();
            o.rs_set = true;
        }
        else if (!strcmp(a, "--rs-iters")) { if (!val(&v) || v < 1 || v > 8) return usage(); o.rsp.iters = (int)v; o.rs_set = true; }
        else if (!strcmp(a, "--rs-columns")) { o.rsp.axis = 1; o.rs_set = true; }
        else if (!strcmp(a, "--sequence")) { while (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-')) o.seq.push_back(argv[++i]); if (o.seq.empty()) return usage(); }
        else if (!strcmp(a, "--out-prefix")) { if (i + 1 >= argc) return usage(); o.prefix = argv[++i]; }
        else if (!strcmp(a, "--denoise")) o.denoise = true;
        else if (!strcmp(a, "--denoise-thresh")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.dn_thresh = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end) return usage();
            o.denoise = true;
        }
        else if (!strcmp(a, "--denoise-frames")) { if (!val(&v) || v < 1 || v > 255) return usage(); o.dn_frames = (int)v; o.denoise = true; }
        else if (!strcmp(a, "--remove-defects")) o.defects = true;
        else if (!strcmp(a, "--defect-thresh")) {
            if (i + 2 >= argc) return usage();
            char *e1 = nullptr, *e2 = nullptr;
            o.df.detect = strtof(argv[i + 1], &e1);
            o.df.agree = strtof(argv[i + 2], &e2);
            if (!e1 || e1 == argv[i + 1] || *e1 || !e2 || e2 == argv[i + 2] || *e2) return usage();
            i += 2;
            o.defects = true;
        }
        else if (!strcmp(a, "--defect-radius")) { if (!val(&v) || v < 0 || v > 4) return usage(); o.df.radius = (int)v; o.defects = true; }
        else if (!strcmp(a, "--defect-grow")) { if (!val(&v) || v < 0 || v > 4) return usage(); o.df.grow = (int)v; o.defects = true; }
        else if (!strcmp(a, "--deflicker")) o.deflicker = true;
        else if (!strcmp(a, "--flicker-cell")) { if (!val(&v) || (v != 16 && v != 32 && v != 64)) return usage(); o.fk_cell = (int)v; o.deflicker = true; }
        else if (!strcmp(a, "--flicker-keep")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.fk_keep = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.fk_keep >= 0.0f && o.fk_keep <= 1.0f)) return usage();
            o.deflicker = true;
        }
        else if (!strcmp(a, "--stabilize")) o.stabilize = true;
        else if (!strcmp(a, "--smooth")) {
            if (i + 1 >= argc) return usage();
            char* end = nullptr;
            o.smooth = strtof(argv[++i], &end);
            if (!end || end == argv[i] || *end || !(o.smooth >= 0.0f && o.smooth <= 1.0f)) return usage();
            o.stabilize = true;
        }
        else if (!strcmp(a, "--auto-cut")) o.auto_cut = true;
        else if (!strcmp(a, "--cut-lost")) { if (!val(&v) || v < 0 || v > 1000) return usage(); o.cut_lost = (int)v; o.auto_cut = true; }
        else if (!strcmp(a, "--propagate")) { if (i + 2 >= argc) return usage(); o.pl_layer = argv[++i]; o.pl_alpha = argv[++i]; }
        else if (!strcmp(a, "--objects")) o.objects = true;
        else if (!strcmp(a, "--plate")) o.plate = true;
        else if (!strcmp(a, "--remove-objects")) o.plate = o.remove_objects = true;
        else if (!strcmp(a, "--plate-margin")) {
            long long mx, my;
            if (!val(&mx) || !val(&my) || mx < 0 || my < 0 || mx > 8192 || my > 8192) return usage();
            o.plate_mx = (int)mx; o.plate_my = (int)my; o.plate = true;
        }
        else if (!strcmp(a, "--min-area")) { if (!val(&v) || v < 1 || v > 0x7fffffff) return usage(); o.ob_min_area = (int)v; o.objects = true; }
        else if (!strcmp(a, "--max-objects")) { if (!val(&v) || v < 1 || v > 255) return usage(); o.ob_max = (int)v; o.objects = true; }
        else if (!strcmp(a, "--deinterlace")) o.deint = true;
        else if (!strcmp(a, "--bff")) o.bff = true;
        else if (!strcmp(a, "--single-rate")) o.single_rate = true;
        else if (!strcmp(a, "--deint-thresh")) { if (!val(&v) || v < 0 || v > 765) return usage(); o.di_thresh = (int)v; o.deint = true; }
        else if (!strcmp(a, "--y4m-out")) o.y4m_out = true;
        else if (!strcmp(a, "--yuv-matrix")) {
            if (!val(&v) || (v != 601 && v != 709 && v != 2020)) return usage();
            o.yuv_matrix = v == 601 ? EPPM_YUV_BT601 : v == 709 ? EPPM_YUV_BT709 : EPPM_YUV_BT2020;
        }
        else if (!strcmp(a, "--temporal")) { if (!val(&v) || (v != 0 && v != 1)) return usage(); o.temporal = (int)v; }
        else if (a[0] == '-' && a[1] == '-') return usage();
        else pos.push_back(a);
    }
    if (!o.seq.empty() || o.prefix) {
        const bool y4m_clip = o.seq.size() == 1 && ends_with(o.seq[0], ".y4m");
        if ((o.seq.size() < 2 && !y4m_clip && !(o.deint && o.seq.size() == 1)) || !o.prefix || !pos.empty()) return usage();
        if ((o.bff || o.single_rate) && !o.deint) return usage();
        if (o.mblur_file || (o.mb_set && !o.mblur)) return usage();       // a clip's blurred frames are named by the prefix
        if (o.rs_file || (o.rs_set && !o.rs)) return usage();
        if (o.rs && (o.deint || o.denoise || o.stabilize || o.auto_cut || o.pl_layer || o.objects || o.plate || o.defects || o.deflicker || o.mblur)) return usage();       // a mode of its own
        // the options of the two-image form that a clip has no meaning for are refused, not ignored
        const Options d;
        bool pin = false;
        for (auto& kv : o.opts) pin = pin || kv.first == "pin_caller_buffers";
        if (pin || o.sw || o.pairs != d.pairs || o.gpus != d.gpus || o.batch != d.batch || o.gt || o.fo != d.fo || o.fb || o.focc || !o.interp.empty())
            return usage();
        if (o.deint) {          // a mode of its own: one interlaced frame is a clip of two field frames
            if (o.denoise || o.stabilize || o.auto_cut || o.pl_layer || o.objects || o.plate || o.defects || o.deflicker || o.mblur) return usage();
            return run_deinterlace(o);
        }
        return run_sequence(o);
    }
    if (o.deint || o.bff || o.single_rate) return usage();
    if (o.denoise || o.stabilize || o.auto_cut || o.pl_layer || o.objects || o.plate || o.defects || o.deflicker || o.y4m_out || o.yuv_matrix >= 0) return usage();     // the filter, the stabiliser, the cut detector, the map and the object detector walk a clip
    if ((o.mblur && !o.mblur_file) || (o.mb_set && !o.mblur)) return usage();
    if ((o.rs && !o.rs_file) || (o.rs_set && !o.rs) || (o.rs && o.mblur)) return usage();
    if (pos.size() == 1 || pos.size() > 3) return usage();
    if (pos.size() >= 2) { o.f1 = pos[0]; o.f2 = pos[1]; }
    if (pos.size() == 3) o.fo = pos[2];

    int h = 0, w = 0, nch = 3;
    if (o.sw > 0) { w = o.sw; h = o.sh; }
    else {
        int h2 = 0, w2 = 0;
        if (eppm_ppm_size(o.f1, &h, &w) != EPPM_OK || eppm_ppm_size(o.f2, &h2, &w2) != EPPM_OK || h != h2 || w != w2) {
            fprintf(stderr, "cannot read %s / %s (or sizes differ)\n", o.f1, o.f2);
            return 1;
        }
    }
    Array3<unsigned char> img1(h, w, 3), img2(h, w, 3);                  // bao_alloc<unsigned char>(h,w,3), main.cpp:42-43
    printf("loading image ... \n");
    if (o.sw > 0) {
        unsigned seed = 1234;
        for (auto& kv : o.opts) if (kv.first == "seed") seed = (unsigned)kv.second;
        synth_image(img1.store.data(), h, w, 0, 0, seed);
        synth_image(img2.store.data(), h, w, -5, 3, seed);              // I2(x,y) = I1(x-5, y+3): flow (+5,-3)
    } else {
        if (eppm_load_ppm(o.f1, img1.store.data(), h, w, &nch) != EPPM_OK || eppm_load_ppm(o.f2, img2.store.data(), h, w, &nch) != EPPM_OK) {
            fprintf(stderr, "cannot read %s / %s\n", o.f1, o.f2);
            return 1;
        }
    }
    std::vector<float> u((size_t)h * w, 0.f), v((size_t)h * w, 0.f);
    std::vector<float*> ur(h), vr(h);
    for (int i = 0; i < h; i++) { ur[i] = &u[(size_t)i * w]; vr[i] = &v[(size_t)i * w]; }
    const bool bidir = o.fb || o.focc || !o.interp.empty();
    std::vector<Array3<unsigned char>> frames;      // --interpolate outputs
    for (size_t k = 0; k < o.interp.size(); k++) frames.emplace_back(h, w, 3);
    std::vector<unsigned char> blurred;             // --motion-blur output
    if (o.mblur) blurred.resize((size_t)h * w * 3);
    std::vector<unsigned char> corrected;           // --rolling-shutter output
    if (o.rs) corrected.resize((size_t)h * w * 3);
    std::vector<float> bu, bv;                      // backward flow and image 1's occlusion mask (--backward / --occlusion)
    std::vector<unsigned char> occ;
    std::vector<float*> bur, bvr;
    std::vector<unsigned char*> occr;
    if (bidir) {
        bu.assign((size_t)h * w, 0.f); bv.assign((size_t)h * w, 0.f); occ.assign((size_t)h * w, 0);
        bur.resize(h); bvr.resize(h); occr.resize(h);
        for (int i = 0; i < h; i++) { bur[i] = &bu[(size_t)i * w]; bvr[i] = &bv[(size_t)i * w]; occr[i] = &occ[(size_t)i * w]; }
    }

    printf("Processing (image size %d * %d * %d)...\n", w, h, nch);
    {
        bao_flow_patchmatch_multiscale_cuda eppm;
        for (auto& kv : o.opts)
            if (!eppm.set_option(kv.first.c_str(), kv.second)) return usage();
        auto t0 = std::chrono::steady_clock::now();
        eppm.init(img1.p(), img2.p(), h, w);                             // main.cpp:63-64: the reference's timed window
        if (!eppm.handle()) return 1;
        if (o.stop_level && !eppm.set_stop_level(o.stop_level)) return usage();
        if (bidir) eppm.compute_flow_bidirectional(ur.data(), vr.data(), bur.data(), bvr.data(), occr.data());
        else eppm.compute_flow(ur.data(), vr.data());
        auto t1 = std::chrono::steady_clock::now();
        printf("GPU: %.3f s (init + %s)\n", std::chrono::duration<double>(t1 - t0).count(), bidir ? "compute_flow_bidirectional" : "compute_flow");
        for (size_t k = 0; k < o.interp.size(); k++)
            if (!eppm.interpolate_frame(o.interp[k].first, frames[k].p())) return 1;
        if (o.mblur && eppm_motion_blur(eppm.handle(), &o.mb, 0, blurred.data(), (size_t)w * 3) != EPPM_OK) {
            fprintf(stderr, "eppm_motion_blur: %s\n", eppm_last_error());
            return 1;
        }
        if (o.rs && eppm_rolling_shutter(eppm.handle(), &o.rsp, 0, corrected.data(), (size_t)w * 3) != EPPM_OK) {
            fprintf(stderr, "eppm_rolling_shutter: %s\n", eppm_last_error());
            return 1;
        }
    }

    // steady state: contexts created once, pairs streamed through set_data + compute_flow
    {
        std::vector<std::thread> workers;
        std::vector<int> failed(o.gpus, 0);
        std::atomic<int> ready(0);
        std::vector<double> t_begin(o.gpus, 0.0), t_end(o.gpus, 0.0);
        const auto epoch = std::chrono::steady_clock::now();
        auto now = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - epoch).count(); };
        int ndev = 1;
        if (eppm_device_count(&ndev) != EPPM_OK || ndev < 1) ndev = 1;
        for (int g = 0; g < o.gpus; g++)
            workers.emplace_back([&, g]() {
                const int dev = g % ndev;          // more workers than devices: they share (one context each; all read the same pinned images)
                if (o.gpus > 1) eppm_bind_thread_to_device(dev, nullptr, nullptr);     // this worker's host side next to its GPU (NUMA node of the PCIe slot)
                if (o.batch > 1) {       // batch context through the C ABI: B pairs per launch sequence
                    eppm_params prm;
                    eppm_default_params(&prm);
                    for (auto& kv : o.opts) apply_opt(prm, kv.first, kv.second);
                    eppm_ctx* c = nullptr;
                    if (eppm_create_batch(&c, h, w, dev, &prm, o.batch) != EPPM_OK) { failed[g] = 1; ready++; return; }
                    if (eppm_set_stop_level(c, o.stop_level) != EPPM_OK) { failed[g] = 1; ready++; eppm_destroy(c); return; }
                    std::vector<std::vector<float>> bu(o.batch, std::vector<float>((size_t)h * w)), bv(o.batch, std::vector<float>((size_t)h * w));
                    std::vector<const uint8_t*> a1(o.batch, img1.store.data()), a2(o.batch, img2.store.data());
                    std::vector<float*> pu(o.batch), pv(o.batch);
                    for (int k = 0; k < o.batch; k++) { pu[k] = bu[k].data(); pv[k] = bv[k].data(); }
                    ready++;
                    while (ready.load() < o.gpus) std::this_thread::yield();
                    t_begin[g] = now();
                    int mine = 0;
                    for (int p = g; p < o.pairs; p += o.gpus) mine++;
                    for (int done = 0; done < mine; done += o.batch) {
                        const int n = (mine - done < o.batch) ? mine - done : o.batch;
                        if (eppm_batch_set_images(c, n, a1.data(), a2.data(), (size_t)w * 3) != EPPM_OK || eppm_batch_compute(c, pu.data(), pv.data()) != EPPM_OK) {
                            failed[g] = 1;
                            eppm_destroy(c);
                            return;
                        }
                        for (int k = 0; k < n; k++)
                            if (bu[k] != u || bv[k] != v) failed[g] = 2;      // every pair of a batch == the single-pair flow
                    }
                    t_end[g] = now();
                    eppm_destroy(c);
                    return;
                }
                bao_flow_patchmatch_multiscale_cuda e;
                e.set_device(dev);
                for (auto& kv : o.opts) e.set_option(kv.first.c_str(), kv.second);
                e.init(h, w);
                if (!e.handle() || !e.set_stop_level(o.stop_level)) { failed[g] = 1; ready++; return; }
                std::vector<float> lu((size_t)h * w), lv((size_t)h * w);
                std::vector<float*> lur(h), lvr(h);
                for (int i = 0; i < h; i++) { lur[i] = &lu[(size_t)i * w]; lvr[i] = &lv[(size_t)i * w]; }
                ready++;
                while (ready.load() < o.gpus) std::this_thread::yield();     // all contexts exist before the window opens
                t_begin[g] = now();
                for (int p = g; p < o.pairs; p += o.gpus) {
                    if (!e.set_data(img1.p(), img2.p())) { failed[g] = 1; return; }
                    e.compute_flow(lur.data(), lvr.data());
                }
                t_end[g] = now();
                if (g == 0 && (lu != u || lv != v)) failed[g] = 2;       // every run of a pair gives the same flow
            });
        for (auto& t : workers) t.join();
        double tb = 1e30, te = 0;
        for (int g = 0; g < o.gpus; g++) { if (t_begin[g] < tb) tb = t_begin[g]; if (t_end[g] > te) te = t_end[g]; }
        const double dt = te - tb;
        for (int g = 0; g < o.gpus; g++)
            if (failed[g]) { fprintf(stderr, "worker %d failed (%s)\n", g, failed[g] == 2 ? "flow differs between runs" : eppm_last_error()); return 1; }
        printf("GPU: %.3f s (%d x (set_data + compute_flow) on %d GPU(s), %d pair(s) per launch, init hoisted): %.2f Mflow-vectors/s\n", dt,
               o.pairs, o.gpus, o.batch, (double)o.pairs * h * w / dt / 1e6);
    }

    if (o.sw > 0) {
        std::vector<float> gu((size_t)h * w, 5.f), gv((size_t)h * w, -3.f);
        float epe = 0, aae = 0;
        eppm_flow_error(u.data(), v.data(), gu.data(), gv.data(), h, w, &epe, &aae);
        printf("EPE %.4f px, AAE %.4f deg against the synthetic translation (+5,-3)\n", epe, aae);
    }
    if (o.gt) {
        int gh = 0, gw = 0;
        std::vector<float> gu((size_t)h * w), gv((size_t)h * w);
        if (eppm_flo_size(o.gt, &gh, &gw) != EPPM_OK || gh != h || gw != w || eppm_load_flo(o.gt, gu.data(), gv.data(), h, w) != EPPM_OK) {
            fprintf(stderr, "cannot read ground truth %s\n", o.gt);
            return 1;
        }
        float epe = 0, aae = 0;
        eppm_flow_error(u.data(), v.data(), gu.data(), gv.data(), h, w, &epe, &aae);
        printf("EPE %.4f px, AAE %.4f deg against %s\n", epe, aae, o.gt);
    }
    printf("Saving flo file...%d*%d\n", h, w);
    if (eppm_save_flo(o.fo, u.data(), v.data(), h, w) != EPPM_OK) { fprintf(stderr, "cannot write %s\n", o.fo); return 1; }
    if (o.fb && eppm_save_flo(o.fb, bu.data(), bv.data(), h, w) != EPPM_OK) { fprintf(stderr, "cannot write %s\n", o.fb); return 1; }
    if (o.focc) {
        static const unsigned char grey[4] = {0, 255, 128, 64};      // consistent, inconsistent, leaves the frame, unknown
        FILE* f = fopen(o.focc, "wb");
        bool ok = f && fprintf(f, "P5\n%d %d\n255\n", w, h) > 0;
        for (size_t i = 0; ok && i < occ.size(); i++) ok = fputc(grey[occ[i] & 3], f) != EOF;
        if (f && fclose(f) != 0) ok = false;
        if (!ok) { fprintf(stderr, "cannot write %s\n", o.focc); return 1; }
    }
    for (size_t k = 0; k < o.interp.size(); k++) {
        FILE* f = fopen(o.interp[k].second, "wb");
        bool ok = f && fprintf(f, "P6\n%d %d\n255\n", w, h) > 0 && fwrite(frames[k].store.data(), 1, frames[k].store.size(), f) == frames[k].store.size();
        if (f && fclose(f) != 0) ok = false;
        if (!ok) { fprintf(stderr, "cannot write %s\n", o.interp[k].second); return 1; }
    }
    if (o.mblur && !write_ppm(o.mblur_file, blurred.data(), h, w)) { fprintf(stderr, "cannot write %s\n", o.mblur_file); return 1; }
    if (o.rs && !write_ppm(o.rs_file, corrected.data(), h, w)) { fprintf(stderr, "cannot write %s\n", o.rs_file); return 1; }
    return 0;
}
