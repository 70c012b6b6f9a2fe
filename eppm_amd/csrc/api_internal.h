// api_internal.h -- what the translation units behind the C ABI of libeppm_hip.so (include/eppm.h) share: error plumbing, parameter
// checks, host-side look-up tables, the PatchMatch generator object, the block / stream cache and the PatchMatch host driver.  Private to
// eppm_amd/csrc; everything here has hidden visibility (the library exports the C ABI, the drop-in class and the kernels, nothing else).
//   api_common.cpp         errors, version, default / checked parameters, host look-up tables, pyramid dimensions
//   host_registry.h/.cpp   caller memory registered for DMA (header-only logic, tested under ThreadSanitizer on the CPU)
//   rng_tables.cpp         XORWOW generator objects and their shared read-only tables
//   mem_cache.cpp          slabs, pinned staging buffers and streams of destroyed contexts, kept for the next one
//   pm_driver.cpp          baoCudaPatchMatch's host loop (sweep forms by iteration, search), shared by contexts and stage launchers
//   context.h              eppm_ctx and what its four translation units share; included by them alone
//   context.cpp            eppm_ctx: create / destroy / planes / stage times (the class's init), the only one of the four that reads opt_*
//   ctx_images.cpp         set_images, push_image, prepare, the host upload of one image (the class's set_data)
//   ctx_compute.cpp        compute in all its forms, the post-PatchMatch branch of both directions, temporal mode (the class's compute_flow)
//   ctx_interp.cpp         frame interpolation, the synthetic shutter, the stage objects' view of a context
//   stage_object.h/.cpp    the core of the nine per-clip stage objects (tracker.cpp, tfilter.cpp, stabilizer.cpp, cutdet.cpp, cmap.cpp,
//                          objects.cpp, plate.cpp, defect.cpp, deflicker.cpp): one allocation and event, the hand-over between streams, shared host helpers
//   device_api.cpp         device-memory plumbing of the ABI (malloc / memcpy / NUMA binding)
//   yuv.cpp                Y'CbCr 4:2:0 frames (include/eppm_yuv.h): format checks, host forms, the context-less device calls
//   launchers_ref_abi.cpp  the reference's live extern "C" stage launchers and the sub-stage entry points of the parity tests
//   test_hooks.cpp         libeppm_hip_test.so only: include/eppm_test.h
#pragma once

#include <ctype.h>
#include <math.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/eppm_yuv.h"
#include "eppm_internal.h"
#include "host_registry.h"

#define EPPM_HIDDEN __attribute__((visibility("hidden")))

// ---- errors (api_common.cpp) ----
EPPM_HIDDEN int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// a failed HIP call leaves a sticky "last error"; it is consumed here so that it cannot surface in a later, unrelated call
#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            (void)hipGetLastError();                                                                         \
            return set_err(EPPM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                                    \
    } while (0)
#define CHK(expr)                     \
    do {                              \
        int r_ = (expr);              \
        if (r_ != EPPM_OK) return r_; \
    } while (0)

// ---- parameters, host look-up tables, pyramid geometry (api_common.cpp) ----
EPPM_HIDDEN int check_params(const eppm_params& p);
EPPM_HIDDEN void host_pm_lut(int R, std::vector<float>& v);       // gs[0..R], cn[0..8] (+ the tolerance library's td[256], ta[256])
EPPM_HIDDEN void host_wmf_lut(std::vector<float>& v);
EPPM_HIDDEN void host_blf_lut(std::vector<float>& v);
EPPM_HIDDEN int pyr_init_dim(int* arrH, int* arrW, int h, int w, int maxDepth, double ratio);
EPPM_HIDDEN int upload_lut(float** dst, const std::vector<float>& v);
// the two-level index of eppm_device.cuh: DeltaTab over the 598 distinct L-inf distances of unorm8 texels: t1[kd] and, per slot of t2, the
// distance it stands for (gaps between the members of a group repeat a neighbour); built once, checked exhaustively
struct DeltaIndex { int32_t t1[256]; std::vector<float> dval; };
EPPM_HIDDEN const DeltaIndex& delta_index();
// `head` followed by a DeltaTab whose values the device computes with the formula they replace (which: see launch_delta_values)
EPPM_HIDDEN int upload_lut_delta(float** dst, const std::vector<float>& head, int which);
EPPM_HIDDEN int upload_pm_lut(float** dst, int R);        // gs[0..R], cn[0..8], then the library's term tables (exact: DeltaTab; tolerance: td, ta)
EPPM_HIDDEN int upload_wmf_lut(float** dst);              // g[0..WMF_RADIUS], DeltaTab of the range weight
EPPM_HIDDEN int upload_blf_lut(float** dst);              // g[0..2*POSTPROC_BLF_SIG_S], DeltaTab of the range weight

// ---- kernel-variant switches of the parity tests ----
// The product library has none: the functions below are constants.  libeppm_hip_test.so (the same objects, with the translation units
// that read a switch compiled once more with -DEPPM_TEST_HOOKS, plus test_hooks.cpp; include/eppm_test.h) exports eppm_test_set_option,
// which sets the DEFAULTS a context copies when it is created (eppm_ctx::opt_*) and what the context-less stage launchers read; a context
// in use is never affected.
#ifdef EPPM_TEST_HOOKS
EPPM_HIDDEN extern std::atomic<int> g_opt_rand_table;       // "rand_table": 0 = contexts created afterwards draw while they search (the form above 512 MB); 2 = 1, and eppm_pm_random_search reads a table too
EPPM_HIDDEN extern std::atomic<int> g_opt_sweep_spec;       // "sweep_spec": -1 by iteration, 0 never, 1 always, 2 always and without the work list, 3 always in the merged form
EPPM_HIDDEN extern std::atomic<int> g_opt_no_split;         // "c2f_no_split"
EPPM_HIDDEN extern std::atomic<int> g_opt_force_split;      // "c2f_force_split": the refine's stage launchers bring the split path's scratch
EPPM_HIDDEN extern std::atomic<int> g_opt_search_pre;       // "search_pre_from": -1 the library's threshold, else the first iteration of the two-phase search
static inline int opt_rand_table() { return g_opt_rand_table.load(); }
static inline int opt_sweep_spec() { return g_opt_sweep_spec.load(); }
static inline int opt_no_split() { return g_opt_no_split.load(); }
static inline int opt_force_split() { return g_opt_force_split.load(); }
static inline int opt_search_pre() { return g_opt_search_pre.load(); }
EPPM_HIDDEN extern std::atomic<int> g_opt_c2f_pre;          // "c2f_pre": -1 the library's EPPM_C2F_PRE, 0 / 1 the window refine's coherent tiles one-phase / two-phase
static inline int opt_c2f_pre() { return g_opt_c2f_pre.load(); }
EPPM_HIDDEN extern std::atomic<int> g_opt_alloc_fill;       // "alloc_fill": -1 off, 0..255 the byte every block is filled with before it is handed out
static inline int opt_alloc_fill() { return g_opt_alloc_fill.load(); }
// The one place that fills (test_hooks.cpp): a no-op while "alloc_fill" is off or e is an error.  Device blocks: hipMemset, then
// hipDeviceSynchronize -- contexts run on non-blocking streams, which the null stream's memset is not ordered against; pinned: memset.
EPPM_HIDDEN hipError_t alloc_fill(hipError_t e, void* p, size_t bytes, bool pinned);
#else
static constexpr int opt_rand_table() { return 1; }
static constexpr int opt_sweep_spec() { return -1; }
static constexpr int opt_no_split() { return 0; }
static constexpr int opt_force_split() { return 0; }
static constexpr int opt_search_pre() { return -1; }
static constexpr int opt_c2f_pre() { return -1; }
static constexpr int opt_alloc_fill() { return -1; }
#endif

// ---- caller memory registered for DMA: host_registry.h (header-only logic), bound to HIP by host_registry.cpp ----

// ---- PatchMatch generator object (rng_tables.cpp) ----
namespace eppm { struct RngTables; }
struct eppm_pm_rng {
    eppm::RngTables* tables = nullptr; // shared, read-only (rngtab_acquire): init_tab, iter_tab, skip_mat point into it
    const int16_t* rand_tab = nullptr; // contexts: the search launches' numbers drawn ahead (rngtab_rand_table), or NULL
    size_t rand_stride = 0;            // shorts per launch
    int device = 0, w = 0, h = 0, gx = 0, gy = 0, G = 0, per_lane = 0;
    unsigned long long seed = 0;
    uint32_t* init_tab = nullptr;
    uint32_t* iter_tab = nullptr;
    uint32_t* work[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [problem][ping-pong]
    bool own_work = true;              // false: the states live in a context's slab (one set per pair of the batch)
    int cur[2] = {0, 0};
    uint32_t* skip_mat = nullptr;
    uint32_t skip_weyl = 0;
    eppm::PmRngDev dev() const
    {
        eppm::PmRngDev d;
        d.init_tab = init_tab; d.iter_tab = iter_tab; d.skip_mat = skip_mat;
        d.skip_weyl = skip_weyl; d.per_lane = per_lane; d.gx = gx; d.gy = gy;
        return d;
    }
};
EPPM_HIDDEN int rng_create(eppm_pm_rng** out, int w, int h, const eppm_params& p, bool alloc_work = true);
EPPM_HIDDEN void rng_free(eppm_pm_rng* r);
EPPM_HIDDEN void rngtab_release_idle();        // eppm_release_cached_memory: the tables no generator uses any more

// ---- blocks and streams of destroyed contexts (mem_cache.cpp) ----
EPPM_HIDDEN hipError_t cache_alloc(void** p, size_t bytes, bool pinned, int device);
EPPM_HIDDEN void cache_free(void* p, size_t bytes, bool pinned, int device);        // the block must be idle
EPPM_HIDDEN hipError_t pooled_stream_create(hipStream_t* out, int device);
EPPM_HIDDEN void pooled_stream_destroy(hipStream_t s, int device);

// ---- baoCudaPatchMatch's host loop (pm_driver.cpp) ----
EPPM_HIDDEN eppm::PmProblem mk_problem(const eppm::PlanesH& P, float* cost, int16_t* nnf, int16_t* nnf_alt, eppm_pm_rng* rng, int k, float* spec = nullptr,
                                       int32_t* scand = nullptr, uint32_t* wl = nullptr, int16_t* seed = nullptr, float* restw = nullptr);
EPPM_HIDDEN void search(eppm::PmBatch& b, eppm_pm_rng* rng, const float* lut, const eppm_params& prm, hipStream_t s, int launch_no = -1, bool pretest = false);
EPPM_HIDDEN bool sweep_list_on(int mode);
// The form of the sweeps of PatchMatch iteration `iteration`: speculative two-launch form by the pixels of the LAUNCH (problem x problems x
// pairs), merged form (one phase A for the four sweeps) from an iteration that depends on the pixels of one PROBLEM; m: the test switch
// "sweep_spec" (-1: the library's own decision).  Asked by pm_iterate and by eppm_probe_dispatch "patchmatch".
EPPM_DECISION bool sweep_speculative(int iteration, long long pixels, int m);
EPPM_DECISION bool sweeps_merged(int iteration, long long pixels, long long problem_pixels, int m);
EPPM_HIDDEN void sweep(eppm::PmBatch& b, const float* lut, const eppm_params& prm, int dir, hipStream_t s, bool speculative = false);
EPPM_HIDDEN void jump(eppm::PmBatch& b, const float* lut, const eppm_params& prm, hipStream_t s);
EPPM_HIDDEN void neighbor(eppm::PmBatch& b, const float* lut, const eppm_params& prm, int launches, hipStream_t s);
// pre_from: -1 the library's own threshold for the two-phase search (eppm_internal.h: pm_search_pretest), else the test switch's
EPPM_HIDDEN void run_patchmatch(eppm::PmBatch& b, eppm_pm_rng* rng, const float* lut, const eppm_params& prm, hipStream_t s, int spec_mode, int pre_from = -1);
// run_patchmatch = pm_start (random field + cost field, the rest-weight planes) then pm_iterate (num_iter x [sweeps + search])
EPPM_HIDDEN void pm_start(eppm::PmBatch& b, eppm_pm_rng* rng, const float* lut, const eppm_params& prm, hipStream_t s, int pre_from = -1);
EPPM_HIDDEN void pm_iterate(eppm::PmBatch& b, eppm_pm_rng* rng, const float* lut, const eppm_params& prm, hipStream_t s, int spec_mode, int pre_from = -1);
#ifndef EPPM_SWEEP_CACHE
#define EPPM_SWEEP_CACHE 1
#endif

// ---- state of the context-less launchers that test_hooks.cpp and the colour entry points share (launchers_ref_abi.cpp) ----
EPPM_HIDDEN int launcher_finish();
EPPM_HIDDEN hipStream_t launcher_stream();        // what eppm_set_launcher_stream set

// ---- Y'CbCr 4:2:0 frames (yuv.cpp; include/eppm_yuv.h) ----
// the argument checks every entry point shares: the format, the pitches, and the planes of nframes frames (3 pointers each); k: the coefficients
EPPM_HIDDEN int yuv_check(const char* what, const eppm_yuv_format* f, const void* const* planes, int nframes, const size_t* pitches, int h, int w,
                          eppm::YuvK* k);

// ---- what the per-clip stage objects read of a context (context.cpp); the objects' shared core: stage_object.h ----
EPPM_HIDDEN int ctx_device(const eppm_ctx* c, int* h, int* w);             // the device; h, w: the context's size
EPPM_HIDDEN void ctx_stage_begin(eppm_ctx* c, const char* name);           // a stage-timing entry on the context's stream (mode 1)
EPPM_HIDDEN void ctx_stage_end(eppm_ctx* c);

// ---- the stabiliser (stabilizer.cpp) as the object detector (objects.cpp) and the background plate (plate.cpp) step their private one ----
// slots slot0 .. slot0 + in.n - 1 on stream s from the input members of in (image 2, the level-0 forward flow, occ1); cut: NULL or one
// flag per pair; timing: the context whose stage-timing entries receive the stages, or NULL
EPPM_HIDDEN int stab_step_on(eppm_stab* f, eppm::StabArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing);
// slot 0's device mask plane (h*w bytes; what eppm_stab_get_mask copies) and the distance in bytes to the next slot's
EPPM_HIDDEN const uint8_t* stab_mask_device(const eppm_stab* f, size_t* slot_stride);
// slot 0's device model (a GmModel; what eppm_stab_get_model copies) and the distance in bytes to the next slot's
EPPM_HIDDEN const char* stab_model_device(const eppm_stab* f, size_t* slot_stride);
