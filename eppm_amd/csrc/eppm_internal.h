// eppm_internal.h -- host-side declarations of the kernel launch wrappers (one per stage).
// All pitches here are in ELEMENTS of the plane's type unless the name says bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../../include/eppm.h"

namespace eppm {

// geometry constants shared by host and device code
constexpr int kMaxLevels = 8;
constexpr int kNumLevels = 3;        // PYR_MAX_DEPTH, defs.h:31
constexpr int kBlock = 16;       // BLOCK_DIM_X/Y, bao_pmflow_kernel.cu:42-43
constexpr int kMaxS = 32;        // samples per patch row: patch_r + 1 <= 32
constexpr int kWmfRadius = 4;    // defs.h:58
constexpr int kBlfRadius = 10;   // 2*POSTPROC_BLF_SIG_S, refine :753
constexpr int kDeltaSlots = 800; // entries of eppm_device.cuh: DeltaTab::t2 (799 are used: api_common.cpp delta_index)

// Batch of independent pairs processed by ONE launch: every device plane of pair k lives at the same offset inside
// pair k's slab, and the slabs are `stride` bytes apart, so a kernel finds pair k's planes by adding k*stride to the
// pointers it was given for pair 0 (blockIdx.z, or .y for 1-D grids, selects the pair).  {1, 0} = a single pair.
struct Batch {
    int n;
    size_t stride;
};
constexpr Batch kOnePair = {1, 0};

// Dispatch decisions: a launcher that chooses between kernels by the size of its launch asks ONE host function below, and the test
// libraries ask the same function (include/eppm_test.h: eppm_probe_dispatch), so that a test can pick shapes on either side of a
// threshold without repeating the constant.  Pure host arithmetic; not exported.
#define EPPM_DECISION __attribute__((visibility("hidden")))
// What a launcher then DID with the answer is noted where a test can read it: one entry per launch -- stage, size of a problem, pairs in
// the launch, the form taken (the decision function's value), and the direction / iteration / level-independent extra the stage has.
// g_launch_note is NULL for ever in the product libraries (nothing in them stores to it, and the log itself is not in them: a launch pays
// one relaxed load); the test libraries point it at their log with the "launch_log" option (test_hooks.cpp) and read the log with
// eppm_probe_launch_log (include/eppm_test.h).
enum LaunchStage { kLaunchSmoothing = 0, kLaunchJbu, kLaunchRefine, kLaunchSearch, kLaunchSweep, kLaunchSweepsMerged };
typedef void (*LaunchNoteFn)(int stage, int w, int h, int npairs, int form, int extra);
extern EPPM_DECISION std::atomic<LaunchNoteFn> g_launch_note;
inline void launch_note(int stage, int w, int h, int npairs, int form, int extra = 0)
{
    if (LaunchNoteFn f = g_launch_note.load(std::memory_order_relaxed)) f(stage, w, h, npairs, form, extra);
}

struct PlanesH {            // host-side mirror of eppm::Planes: float4 texel planes {r,g,b,census bits}, pitch in pixels
    const void* pk1;
    const void* pk2;
    int w, h, pitch;
    // optional (NULL: absent): the same texels in 4 bytes, {R, G, B, census} as one word per pixel, same pitch.  Kernels that stage
    // a whole tile / window in LDS read these and convert while storing (a quarter of the HBM and L2 bytes for the same values)
    const uint32_t* pc1 = nullptr;
    const uint32_t* pc2 = nullptr;
    // optional, tolerance library only (NULL: absent): COLUMN-PARITY planes of the 4-byte texels at the PatchMatch level.  The patch samples
    // every other column, so the S samples of a patch row are S CONSECUTIVE words of the plane of their column parity: 3 gathers per row of 10
    // samples instead of 10 (the kernels that give a lane a whole evaluation run at the L1's lane rate).  Layout: word [p][y][i] = texel
    // (clamp(2i + p - pp_pad, 0, w - 1), y) -- replicate padding = the clamp addressing of the texture model; pp_pitch words per row.
    const uint32_t* pp1 = nullptr;
    const uint32_t* pp2 = nullptr;
    int pp_pitch = 0, pp_pad = 0;
};
inline int parity_pitch(int w, int pad) { return (w + 2 * pad + 1) / 2 + 1; }      // words per row of one parity plane
// the two parity planes of one image (k_prepare.hip); pc = its 4-byte texel plane, pitch pc_pitch words
void launch_parity_planes(uint32_t* pp, int pp_pitch, int pad, const uint32_t* pc, int pc_pitch, int w, int h, hipStream_t s, Batch bt = kOnePair);

// ---- prepare (k_prepare.hip) ----
void launch_gauss_rgba(uint32_t* out, const uint32_t* in, int pitch_px, int h, int w, float sigma, int radius, hipStream_t s, Batch bt = kOnePair);
// blur + exact 2:1 decimation in one kernel (only the kept pixels are blurred); use when gauss_decimate2_ok()
bool gauss_decimate2_ok(int outH, int outW, int h, int w, float ratio, int radius);
void launch_gauss_decimate2(uint32_t* out0, const uint32_t* in0, uint32_t* out1, const uint32_t* in1, int nimg, int out_pitch_px, int outH,
                            int outW, int pitch_px, int h, int w, float sigma, int radius, hipStream_t s, Batch bt = kOnePair);
// the same blur on two images of equal geometry in one launch
void launch_gauss_rgba2(uint32_t* out0, const uint32_t* in0, uint32_t* out1, const uint32_t* in1, int pitch_px, int h, int w, float sigma,
                        int radius, hipStream_t s, Batch bt = kOnePair);
// census (+ texel plane) of several planes in one launch
struct CensusJob { uint8_t* census; int cpitch; void* texels; int tpitch; const uint32_t* img; int ipitch; int w, h; int first_block;
                   uint32_t* packed = nullptr; };   // optional 4-byte texel plane {R,G,B,census}, pitch tpitch
struct CensusBatch { int n; CensusJob job[2 * kMaxLevels]; };
void launch_census_batch(CensusBatch& B, hipStream_t s, Batch bt = kOnePair);
void launch_resize_rgba(uint32_t* out, int out_pitch_px, int outH, int outW, const uint32_t* in, int in_pitch_px, int h, int w,
                        float ratio, hipStream_t s, Batch bt = kOnePair);
// census plane and (optionally, texels != NULL) the float4 texel plane the patch kernels read
void launch_census(uint8_t* census, int cpitch, void* texels, int tpitch, const uint32_t* img, int ipitch, int w, int h, hipStream_t s);
void launch_pack(void* texels, int tpitch, const uint32_t* img, int ipitch, const uint8_t* census, int cpitch, int w, int h, hipStream_t s);
// DeltaTab values (eppm_device.cuh): t2[i] = f(t2[i]) on the device, which = 0 patch data term, 1 smoothing / weighted-median weight
void launch_delta_values(float* t2, int n, int which, hipStream_t s);
void launch_rgb_to_rgba(uint32_t* out, int pitch_px, const uint8_t* rgb, int h, int w, hipStream_t s, Batch bt = kOnePair);

// ---- Y'CbCr 4:2:0 (k_yuv.hip; the arithmetic: yuv.h) ----
struct YuvK;
// The plane pointers of up to kYuvChunk slots, passed to the kernel by value: no device table, no allocation, no synchronisation per call.
constexpr int kYuvChunk = 16;
struct YuvSlots { const void* p[kYuvChunk][3]; };
// slots 0 .. n - 1 (n <= kYuvChunk) of S into the RGBA planes dst + slot * dst_stride (bytes), rows dst_pitch bytes apart; pitches in bytes
void launch_yuv_to_rgba(const YuvSlots& S, int n, uint32_t* dst, size_t dst_pitch, size_t dst_stride, const size_t* pitches, int h, int w, int layout,
                        const YuvK& k, hipStream_t s);
bool yuv_to_rgba_vec(const void* dst, size_t dst_pitch, size_t dst_stride);     // whether that launch takes the 16-byte stores
void launch_rgba_to_yuv(void* const* planes, const size_t* pitches, const uint32_t* src, size_t src_pitch, int h, int w, int layout, const YuvK& k,
                        hipStream_t s);

// ---- PatchMatch (k_pm_field.hip, k_pm_sweep.hip, k_pm_search.hip; shared: pm_device.cuh) ----
// One PatchMatch problem = (source planes, target planes, NNF, cost).  The forward (1->2) and backward (2->1)
// problems of a pair have the same size and run in the same launches (blockIdx.z / blockIdx.y selects one).
struct PmProblem {
    PlanesH P;
    float* cost;
    int16_t* nnf;        // short2, current
    int16_t* nnf_alt;    // short2, ping-pong partner for the sweeps
    // Evaluation cache of the sweeps, one (candidate, cost) entry per pixel and sweep direction: four planes each (cost pitch),
    // direction d at element offset d * PmBatch::cache_plane.  The patch cost is a pure function of (pixel, candidate) while the
    // images stand, so a sweep that meets the candidate it evaluated for this pixel last time -- the neighbour's match did not
    // change between two iterations, the normal case once the field has converged -- takes the cost from here.  spec doubles as
    // phase A's hand-over plane to phase B (k_pm_sweep.hip).  scand == NULL: no cache (every candidate is evaluated).
    float* spec = nullptr;
    int32_t* scand = nullptr;   // x | y << 16 of the cached candidate; -1 = empty (no candidate has both coordinates -1)
    // Work list of the speculative sweeps (k_pm_sweep.hip): phase A names the chains on which some candidate of the rejection path
    // would be ACCEPTED -- every other chain leaves its pixels as they are, and phase B walks the listed chains only.  Layout:
    // word 0, 1: list lengths of the even / odd sweeps of a run (ping-pong: a sweep's phase A clears the other one);
    // [16, 16 + units): stamp per unit (two adjacent segments of a line) = 1 + number of the last sweep that listed it;
    // [16 + units, 16 + 2 * units): the list.  NULL: phase B walks every chain.
    // Merged form (one phase A for the four sweeps of an iteration): words 8 + 4 * (iteration & 1) + d: list length of direction d;
    // [16 + (2 + d) * units, ..): stamps of direction d = 1 + the iteration that listed the unit last; [16 + (6 + d) * units, ..): its list.
    uint32_t* wl = nullptr;
    // Merged form of the speculative sweeps (k_pm_sweep.hip, k_pm_spec_all): the field as it stood before each direction's sweep of the
    // current iteration, four short2 planes (direction d at int16 offset d * PmBatch::seed_plane) -- where the in-place sweeps read their seeds.
    int16_t* seed = nullptr;
    uint32_t* rng_work;       // [nblocks][64][6] XORWOW lane states read by the random search
    uint32_t* rng_work_next;  // ... written by it (ping-pong: four workgroups read each block's state, one advances it)
    // Rest-weight plane of the two-phase search (k_pm_search.hip; cost pitch): per pixel an upper bound, formed from the source image
    // alone, of the weights of the patch rows the search's pre-test leaves out.  NULL: every search runs in the one-phase form.
    float* restw = nullptr;
};
struct PmBatch {
    PmProblem p[2];      // the problems of pair 0; pair k's are `stride` bytes further (every pointer of PmProblem)
    int n;               // problems per pair: 1 or 2
    int cpitch, npitch;  // elements
    int npairs = 1;      // a launch covers n * npairs problems
    size_t stride = 0;
    size_t cache_plane = 0;   // elements per direction plane of PmProblem::spec / scand
    int wl_units = 0;         // capacity of PmProblem::wl (pm_worklist_units)
    int sweep_seq = 0;        // number of the next sweep of this PatchMatch run (0, 1, ..): launch_pm_sweep counts
    size_t seed_plane = 0;    // int16 elements per direction plane of PmProblem::seed
    int merged_it = 0;        // merged form: number of the iteration (list parity, stamps)
    int seg_len = 0, nseg_row = 0, nseg_col = 0;   // merged form: the sweeps' geometry (every kernel lists for every direction)
};
// units (pairs of adjacent segments of a line) of the larger of the row and column sweeps; words of PmProblem::wl
int pm_worklist_units(int w, int h, int seg_len);
// words of PmProblem::wl: 16 counters | stamps, list of the two-launch form (units each) | stamps, lists of the merged form (4 x units each)
inline size_t pm_worklist_words(int w, int h, int seg_len) { return 16 + 10 * (size_t)pm_worklist_units(w, h, seg_len); }
// RNG tables shared by both problems (same seed, same block ids: the reference re-initialises the states on
// every baoCudaPatchMatch call, kernel.cu:160); see xorwow_host.cpp
struct PmRngDev {
    const uint32_t* init_tab;    // [nblocks][64][6] lane l at draw 8*l              (init field)
    const uint32_t* iter_tab;    // [nblocks][64][6] lane l at draw 512 + per_lane*l (first search)
    const uint32_t* skip_mat;    // [160][5] GF(2) matrix: advance by (512*G - per_lane) draws
    uint32_t skip_weyl;          // 362437 * (512*G - per_lane)
    int per_lane;                // draws per lane per search = 512*G/64
    int gx, gy;
    // The numbers of search launch `it` of a run, drawn ahead: [block][G][512] int16 (the shorts the search stores in LDS); NULL: the
    // search draws them itself from rng_work.  The block streams depend on (seed, geometry, num_guess) only -- the reference re-seeds on
    // every call (kernel.cu:68, :160) -- so the numbers every PatchMatch run of a geometry draws are the same constants.
    const int16_t* rand_tab = nullptr;
};
// fills tab[block][512*G] with the draws of ONE search launch from the lane states in `work` and advances `work` (in place) to the
// next launch's position: exactly what wave G of k_pm_random_search does
void launch_pm_rand_table(const PmRngDev& rng, uint32_t* work, int16_t* tab, int G, hipStream_t s);
void launch_pm_init_field(const PmBatch& b, const PmRngDev& rng, hipStream_t s);
void launch_pm_cost_field(const PmBatch& b, const float* lut, int R, hipStream_t s);
// the PatchMatch kernels that read the column-parity planes at patch radius R when the planes exist: 1 random search, 2 phase A of the
// sweeps, 4 cost field
int pm_parity_kernels(int R);
// one directional sweep; returns true when the result is in nnf_alt (caller swaps nnf/nnf_alt)
// speculative: the two-launch form for iterations in which few candidates are accepted (k_pm_sweep.hip, k_pm_sweep_spec); same results
bool launch_pm_sweep(PmBatch& b, const float* lut, int R, int seg_len, int dir, hipStream_t s, bool speculative = false);
// The four sweeps of one iteration in the merged speculative form (k_pm_spec_all + four in-place launches over the listed chains): same
// results, in place in nnf.  Returns false (nothing launched) when the problems lack the planes or the radius has no instantiation.
bool launch_pm_sweeps_merged(PmBatch& b, const float* lut, int R, int seg_len, int iteration, hipStream_t s);
// one jump-flood launch (step = neighbour distance); reads nnf, writes nnf_alt (caller swaps)
void launch_pm_jump(const PmBatch& b, const float* lut, int R, int step, hipStream_t s);
// one 4-neighbour propagation launch (d_neighbor_propagate); reads nnf, writes nnf_alt (caller swaps)
void launch_pm_neighbor(const PmBatch& b, const float* lut, int R, hipStream_t s);
// pretest: the two-phase form (same results; quarter-block workgroups whatever pm_search_rows says: the caller asked pm_search_pretest)
// where the launch has what it needs (pm_search_pretest_ready), the one-phase form otherwise
void launch_pm_random_search(const PmBatch& b, const PmRngDev& rng, const float* lut, int R, int search_range, int num_guess,
                             hipStream_t s, bool pretest = false);
// fills PmProblem::restw of every problem of the batch (radius 9, exact library; nothing otherwise): once per PatchMatch run, after the images stand
void launch_pm_rest_weight(const PmBatch& b, const float* lut, int R, hipStream_t s);
bool pm_search_pretest_ready(const PmBatch& b, const PmRngDev& rng, int R);
// test support: the pre-test's sums N and D_A of every pixel with its stored match as the guess, per direction k into n[k] / d[k] (cost
// pitch; pair 0's planes, pair p's lie p * PmBatch::stride bytes further); needs the parity planes (radius 9, exact library)
struct PmPretestSums { float* n[2]; float* d[2]; };
void launch_pm_pretest_probe(const PmBatch& b, const float* lut, int R, const PmPretestSums& out, hipStream_t s);
// whether a launch of that size has a two-phase form at all: radius 9, quarter-block workgroups (pm_search_rows == 4), exact library; and
// whether the search of PatchMatch iteration `iteration` (0, 1, ..) takes it: from iteration EPPM_SEARCH_PRE_FROM on (negative: never)
EPPM_DECISION bool pm_search_pretest_form(int w, int h, int R, int problems, int npairs);
EPPM_DECISION bool pm_search_pretest(int iteration, int w, int h, int R, int problems, int npairs);
// the build's knobs of the pre-test at patch radius R: first centre row and number of centre rows, threshold iteration, epsilon
EPPM_DECISION void pm_search_pretest_knobs(int R, int* row0, int* rows, int* from, float* eps);
// rows of a 16x16 block per workgroup of the random search: 4 (a quarter block, a wave per guess) or 2 (an eighth block: small launches
// at radius 9 that read numbers drawn ahead, `table`); problems = directions per pair
EPPM_DECISION int pm_search_rows(int w, int h, int R, int problems, int npairs, bool table);
// The classic sweep's kernel for one direction.  lpc: lanes per chain (0: no cooperative kernel at this radius, k_pm_seg_propagate);
// small: the launch cannot fill the chip (radius 9: twice the lanes per chain in the exact library); pre: the chains' pixels are fetched
// before the first step (given the evaluation cache, PmProblem::scand); tile: the source tile fits LDS, otherwise the sweep gathers.
struct SweepForm { int lpc; bool small, pre, tile; };
EPPM_DECISION SweepForm pm_sweep_form(int w, int h, int R, int seg_len, int dir, int problems, int npairs);

// The seeded start of a streaming context's PatchMatch, after launch_pm_init_field + launch_pm_cost_field on the same
// batch: the cost of every pixel's temporal prior (an absolute target like an NNF entry; a component <= kInvalid: none), and the prior
// kept where it exists and its cost is STRICTLY lower than the random match's -- the cost-field kernel with a compare in front of
// its store.  Writes nnf and cost, and copies of both into nnf_init / cost_init (unpitched; what eppm_get_plane shows); the evaluation
// cache, the work lists and the generator states stay as launch_pm_init_field left them.  One launch covers every problem of the batch: the
// planes below are slot 0's, slot k's lie k * stride bytes further.  A slot whose prior holds "none" everywhere keeps the cold start's bits.
struct PmSeed {
    const int16_t* prior[2];     // short2 per pixel of direction k, unpitched
    int16_t* nnf_init[2];
    float* cost_init[2];
    size_t stride = 0;           // bytes between the slots' planes
};
void launch_pm_cost_select(const PmBatch& b, const PmSeed& seed, const float* lut, int R, hipStream_t s);

// ---- temporal prior (k_temporal.hip; the rule itself: temporal.h) ----
// Up to two directions and nslots slots per launch: prev[d] a displacement snapshot, prior[d] the advected targets, keys[d] w*h ints that
// hold kTemporalNoKey between launches (launch_temporal_keys_init once; the gather pass restores them), step[d] +1 forward / -1 backward.
// The pointers are slot 0's; slot k's planes lie k * stride bytes further.  armed: bit k set = slot k has a snapshot to advect; a slot whose
// bit is clear is skipped by the splat and gets "no prior" everywhere from the gather.  The flags travel in the kernel arguments, so
// arming costs no copy, no allocation and no synchronisation.
constexpr int kTemporalMaxSlots = 4096;      // eppm_create_batch's limit on npairs
struct TemporalArgs {
    const int16_t* prev[2];
    int16_t* prior[2];
    int32_t* keys[2];
    int step[2];
    int w, h, ndir;
    int nslots;
    size_t stride;
    uint32_t armed[kTemporalMaxSlots / 32];
};
void launch_temporal_keys_init(int32_t* keys, int n, hipStream_t s);
void launch_temporal_splat(const TemporalArgs& a, hipStream_t s);
void launch_temporal_gather(const TemporalArgs& a, hipStream_t s);
// prev <- the displacements of a field of stored matches (nnf_pitch in short2 elements); pair k's snapshot lies k * prev_stride bytes further
void launch_temporal_snapshot(int16_t* prev, size_t prev_stride, const int16_t* nnf, int nnf_pitch, int w, int h, hipStream_t s, Batch bt = kOnePair);
// launch_nnf2flow and the snapshot of the same field in one launch
void launch_nnf2flow_snapshot(float* flow, int flow_pitch, int16_t* prev, size_t prev_stride, const int16_t* nnf, int nnf_pitch, int w, int h,
                              hipStream_t s, Batch bt = kOnePair);

// ---- level-2 post-processing (k_post.hip) ----
void launch_lr_check(int16_t* nnf1, float* cost1, const int16_t* nnf2, int w, int h, int cost_pitch, int nnf_pitch, hipStream_t s, Batch bt = kOnePair);
void launch_outlier(int16_t* nnf_out, float* cost, const int16_t* nnf_in, int w, int h, int cost_pitch, int nnf_pitch, hipStream_t s, Batch bt = kOnePair);
// all num_iter Jacobi launches; ping-pongs buf_a (input) / buf_b, ws = 2*w*h + num_iter + 2 uint32 words; returns the result buffer
size_t wmf_workspace_words(int w, int h, int num_iter);
int16_t* launch_wmf(int16_t* buf_a, int16_t* buf_b, const uint32_t* img, int ipitch, int w, int h, int nnf_pitch,
                    const float* wmf_lut, int num_iter, int only_occlusion, uint32_t* ws, hipStream_t s, Batch bt = kOnePair);
void launch_fill_holes(int16_t* nnf_out, const int16_t* nnf_in, const uint32_t* img, int ipitch, int w, int h, int nnf_pitch,
                       hipStream_t s, Batch bt = kOnePair);
void launch_nnf2flow(float* flow, int flow_pitch, const int16_t* nnf, int nnf_pitch, int w, int h, hipStream_t s, Batch bt = kOnePair);

// ---- coarse to fine: flow up one level (k_c2f_resize.hip) ----
void launch_resize_flow(float* out, int outH, int outW, const float* in, int h, int w, float ratio, float post_scale, hipStream_t s, Batch bt = kOnePair);
void launch_mul_scalar(float* flow, float scale, int h, int w, hipStream_t s);
// ---- coarse to fine: candidate refine (k_c2f_refine.hip, c2f_device.cuh) ----
// workgroups per tile of the candidate refine: 0 (one launch, no scratch), or 3 / 4 (k_c2f_refine_tiled<R, 3 | 4> + k_c2f_select)
EPPM_DECISION int c2f_refine_split_factor(int w, int h, int R, int npairs = 1, bool no_split = false);
bool c2f_refine_wants_split(int w, int h, int R, int npairs = 1, bool no_split = false);      // c2f_refine_split_factor(..) != 0
bool c2f_window_span(int R, int* span_x, int* span_y);          // test support: admissible centre spread of the LDS-window kernels
// cost9: scratch of 36 floats per pixel for launches that c2f_refine_wants_split(), or NULL
// pre: the two-phase form of the radius-9 window kernel's coherent tiles: -1 as the library was built, 0 off, 1 on;
// stat: NULL, or eight zeroed counters that kernel adds to; probe: NULL, or 73 floats per pixel and pair for the pre-test's sums (two-phase
// form forced; both test support)
void launch_c2f_refine(const PlanesH& P, float* flow, const float* lut, int R, float* cost9, hipStream_t s, Batch bt = kOnePair, bool no_split = false,
                       int pre = -1, unsigned* stat = nullptr, float* probe = nullptr);
void c2f_pretest_knobs(int R, int* on, int* row0, int* rows, int* cap, int* parts, float* eps, float* dmin, float* rhsmin);      // test support: that form's knobs
// ---- coarse to fine: joint-bilateral smoothing (k_flow_blf.hip) ----
void launch_flow_blf(float* out, const float* in, const uint32_t* img, int ipitch, int w, int h, int flow_pitch,
                     const float* blf_lut, hipStream_t s, Batch bt = kOnePair);
EPPM_DECISION int flow_blf_pixels_per_lane(int w, int h, int npairs = 1);      // of the smoothing: 2 (k_flow_blf<2>, large launches) or 1
// ---- draft mode: joint-bilateral upsampling (k_flow_jbu.hip) ----
// out (h x w float2, unpitched) = the smoothing of the doubled, 2x-replicated coarse flow (hc x wc float2, unpitched; rows and columns past
// its edge repeat the last one) guided by img; the replicated plane is never written.  Pixels per lane by flow_blf_pixels_per_lane.
void launch_flow_jbu(float* out, const float* in_coarse, const uint32_t* img, int ipitch, int w, int h, int wc, int hc, const float* blf_lut,
                     hipStream_t s, Batch bt = kOnePair);

// interleaved float2 flow -> planar u | v (2*n floats) on the device: compute_flow's de-interleave, driver :302-306
void launch_split_flow(float* uv, const float* flow, int n, hipStream_t s, Batch bt = kOnePair);

// ---- occlusion masks of a bidirectional call (k_occ.hip; the test itself: fb_occlusion.h) ----
// ndir 2: occ1 <- (F fwd, G bwd) and occ2 <- (F bwd, G fwd) for npairs pairs (fwd at fwd_stride, bwd / occ1 / occ2 at bwd_stride bytes apart);
// ndir 1: occ1 <- (F fwd, G bwd) of one pair (npairs 1).  Fields: h*w float2, masks: h*w bytes, all unpitched.
void launch_fb_occlusion(uint8_t* occ1, uint8_t* occ2, const float* fwd, size_t fwd_stride, const float* bwd, size_t bwd_stride, int h, int w,
                         float alpha, float beta, int npairs, int ndir, hipStream_t s);

// ---- frame interpolation (k_interp.hip; the per-pixel arithmetic: interp.h) ----
// One launch covers npairs pairs x nt times (nt <= kInterpChunk): slot z = pair * nt + k.  Inputs of pair p lie p * (their stride) bytes past
// pair 0's; the scratch planes of slot z lie z * plane ELEMENTS past slot 0's.  Images: RGBA words, img_pitch bytes per row; flow: h*w float2,
// masks: h*w bytes, unpitched.  Output: packed RGB (rgb != NULL, slot z at z*h*w*3 bytes) or RGBA words of pair 0 into rgba[k] (pitch bytes).
constexpr int kInterpChunk = 4;
struct InterpArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* flow;
    size_t flow_stride;
    const uint8_t* occ1;
    const uint8_t* occ2;
    size_t occ_stride;
    uint64_t* keys;              // splat keys (all ones: nothing splatted)
    int32_t* fill1;              // pass 1: source index of the vector, -1 a hole
    int32_t* fill2;              // pass 2: written only where fill1 holds a hole
    size_t plane;
    uint8_t* rgb;
    uint8_t* rgba[kInterpChunk];
    size_t rgba_pitch;
    int h, w, nt;
    float t[kInterpChunk];
};
void launch_interp_splat(const InterpArgs& a, int npairs, hipStream_t s);      // clears the keys, then splats
void launch_interp_fill(const InterpArgs& a, int npairs, hipStream_t s);       // both fill passes
void launch_interp_blend(const InterpArgs& a, int npairs, hipStream_t s);

// ---- synthetic shutter (k_mblur.hip; the per-pixel arithmetic: mblur.h) ----
// One launch covers npairs pairs.  Inputs of pair p lie p * (their stride) bytes past pair 0's; its packed plane p * plane words, its tile
// keys p * tplane keys and its packed RGB output p*h*w*3 bytes past pair 0's.  Image: RGBA words, img_pitch bytes per row; flow: h*w float2,
// unpitched.  Output: packed RGB (rgb != NULL) or RGBA words of pair 0 into rgba (rgba_pitch bytes per row).
struct MBlurArgs {
    const uint8_t* img;
    size_t img_pitch, img_stride;
    const float* flow;
    size_t flow_stride;
    uint32_t* packed;            // {R, G, B, mq} per pixel, unpitched
    uint64_t* tkeys;             // the maximum key of each 32x32 tile, tiles_y rows of tiles_x
    size_t plane, tplane;
    uint8_t* rgb;
    uint8_t* rgba;
    size_t rgba_pitch;
    int h, w, tiles_x, tiles_y;
    float shutter, max_radius;
    int taps;
};
void launch_mblur_pack(const MBlurArgs& a, int npairs, hipStream_t s);
void launch_mblur_gather(const MBlurArgs& a, int npairs, hipStream_t s);

// ---- rolling-shutter correction (k_rshutter.hip; the per-pixel arithmetic: rshutter.h) ----
// One launch covers npairs pairs.  Inputs of pair p lie p * (their stride) bytes past pair 0's; its velocity plane p * plane float2 and its
// packed RGB output p*h*w*3 bytes past pair 0's.  Image: RGBA words, img_pitch bytes per row; flow: h*w float2, unpitched.  Output: packed
// RGB (rgb != NULL) or RGBA words of pair 0 into rgba (rgba_pitch bytes per row).
struct RShutterArgs {
    const uint8_t* img;
    size_t img_pitch, img_stride;
    const float* flow;
    size_t flow_stride;
    float* vel;                  // the velocity of each pixel, float2, unpitched
    size_t plane;
    uint8_t* rgb;
    uint8_t* rgba;
    size_t rgba_pitch;
    int h, w;
    float readout, anchor;
    int iters, axis, frame;
};
void launch_rs_velocity(const RShutterArgs& a, int npairs, hipStream_t s);
void launch_rs_gather(const RShutterArgs& a, int npairs, hipStream_t s);

// ---- dense point trajectories (k_track.hip; the per-point arithmetic: track.h) ----
// The device counters of a tracker (int32 each): the live count, the next id, the frame, the last step's dropped / ended / seeded counts,
// and what the kernels of one step hand to each other.
enum {
    kTrackCntLive, kTrackCntNextId, kTrackCntFrame, kTrackCntDropped, kTrackCntEnded, kTrackCntSeeded,
    kTrackCntIdBase, kTrackCntSurv, kTrackCntPrevLive, kTrackCntSeeded0, kTrackCntDropped0, kTrackCntN = 16
};
struct TrackRec;
struct TrackDev {                   // a tracker's allocation (tracker.cpp) as the kernels see it
    struct {
        int spacing;
        long long min_eig;
        float fb_alpha, fb_beta, mb_alpha, mb_beta;
    } p;
    int cap, ncells, ncx;
    float* npos;                    // cap float2: the advanced positions
    uint8_t* stat;                  // cap: the end reasons of the last advance (0 alive)
    TrackRec* ended;                // cap: the last step's ended tracks
    int32_t* ended_reason;          // cap
    uint8_t* cov;                   // ncells: coverage of frame k+1 (zero between steps)
    uint8_t* flags;                 // ncells: seed flags
    int32_t *blk_s, *blk_e;         // per slot block: survivor / ended counts, then their offsets
    int32_t* blk_c;                 // per cell block: seed counts, then their offsets
    int32_t* cnt;                   // kTrackCntN counters
};
struct TrackIn {                    // the planes of one pair: RGBA images (pitch bytes per row), h*w float2 forward / backward flows
    const uint8_t* img1;
    const uint8_t* img2;
    size_t pitch;
    const float* fwd;
    const float* bwd;
    int h, w;
};
void launch_track_seed0(const TrackDev& d, const TrackIn& in, TrackRec* cur, hipStream_t s);     // frame 0 and no live track: seed image 1
void launch_track_advance(const TrackDev& d, const TrackIn& in, const TrackRec* cur, hipStream_t s);
void launch_track_seed(const TrackDev& d, const TrackIn& in, hipStream_t s);
void launch_track_compact(const TrackDev& d, const TrackIn& in, const TrackRec* cur, TrackRec* next, hipStream_t s);

// ---- motion-compensated temporal filter (k_tfilter.hip; the per-pixel arithmetic: tfilter.h) ----
// One launch steps n pairs: pair k's inputs (image 1 / image 2: RGBA words, img_pitch bytes per row; bwd: h*w float2; occ2: h*w bytes) lie
// k * (their stride) bytes past pair 0's and feed slot slot0 + k, whose block (state 0 | state 1: h*w float4 each | out: h*w RGBA words)
// lies (slot0 + k) * slot_stride bytes past slot 0's.  The per-slot bits travel in the kernel arguments as TemporalArgs::armed does: cur
// (which state is the previous one; the step writes the other), empty (the slot has no state: the previous state is image 1's seed) and
// cut (image 2 starts another clip), so a step costs no copy, no allocation and no synchronisation.
struct TFilterArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ2;
    size_t occ_stride;
    float* st0;
    float* st1;
    uint32_t* out;
    size_t slot_stride;
    int h, w, n, slot0;
    float thresh;
    int n_max;
    uint32_t cur[kTemporalMaxSlots / 32], empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32];
};
void launch_tfilter_step(const TFilterArgs& a, hipStream_t s);

// ---- global camera motion and stabilisation (k_gmotion.hip; the arithmetic: gmotion.h) ----
// One step covers n pairs: pair k's inputs (image 2: RGBA words, img_pitch bytes per row; fwd: h*w float2; occ1: h*w bytes) lie k * (their
// stride) bytes past pair 0's and feed slot slot0 + k, whose block lies (slot0 + k) * slot_stride bytes past `mem`: tiles_x * tiles_y slabs
// of 128 bytes (the twelve sums of one accumulate block, 64 x 16 pixels) | GmModel | GmState (at off_model, 256 bytes together) | out:
// h*w RGBA words (off_out) | mask: h*w bytes (off_mask).  A step is iters x (accumulate, solve) and one warp launch; `pass` is the
// launch's pass.  The per-slot bits travel in the kernel arguments as TFilterArgs' do: empty (the slot's state is the identity whatever
// the block holds) and cut (image 2 starts another clip).  The state is read and written by one lane of one launch, in place.
constexpr int kGmTileW = 64, kGmTileH = 16, kGmSlabBytes = 128;
struct StabArgs {
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* fwd;
    size_t fwd_stride;
    const uint8_t* occ1;
    size_t occ_stride;
    char* mem;
    size_t slot_stride, off_model, off_out, off_mask;
    int h, w, n, slot0, tiles_x, tiles_y, iters, pass;
    float tau2, smooth;
    uint32_t empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32];
};
void launch_gmotion_accumulate(const StabArgs& a, hipStream_t s);
void launch_gmotion_solve(const StabArgs& a, hipStream_t s);
void launch_stab_warp(const StabArgs& a, hipStream_t s);

// ---- scene-cut detection (k_cutdet.hip; the arithmetic: cutdet.h) ----
// One step covers n pairs: pair k's inputs (image 1 / image 2: RGBA words, img_pitch bytes per row; bwd: h*w float2; occ1 / occ2: h*w
// bytes) lie k * (their stride) bytes past pair 0's and feed slot slot0 + k.  The detector's allocation `mem`: one record (CutRecord) per
// slot, 128 bytes apart, then per slot (off_slabs + slot * slab_stride) tiles_x * tiles_y slabs of 64 bytes (the ten uint32 sums of one
// accumulate block, 64 x 16 pixels).  A step is one accumulate and one finish launch; the thresholds travel in the kernel arguments.
constexpr int kCutTileW = 64, kCutTileH = 16, kCutSlabBytes = 64;
struct CutArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ1;
    const uint8_t* occ2;
    size_t occ_stride;
    char* mem;
    size_t off_slabs, slab_stride;
    int h, w, n, slot0, tiles_x, tiles_y;
    int lost_permille;
    long long r16;
};
void launch_cutdet_accumulate(const CutArgs& a, hipStream_t s);
void launch_cutdet_finish(const CutArgs& a, hipStream_t s);

// ---- dense correspondence map to an anchor frame (k_cmap.hip; the arithmetic: cmap.h) ----
// One step covers n pairs: pair k's inputs (TFilterArgs' planes) lie k * (their stride) bytes past pair 0's and feed slot slot0 + k, whose
// block lies (slot0 + k) * slot_stride bytes past `mem`: map 0 | map 1 (h*w float2 each) | anchor | frame | layer | out (h*w RGBA words
// each, from off_anchor on).  The per-slot bits travel in the kernel arguments as TFilterArgs' do: cur (which map
// is the previous one; the step writes the other), empty (the slot has no state: the previous map is the seed, the anchor image 1, which
// the step also stores), cut (image 2 starts another clip: seed, and image 2 becomes the anchor) and deflayer (the render reads the
// anchor with alpha 255 in place of the layer plane).  The render launch covers slots slot0 .. slot0 + n - 1 and reads nothing of a pair.
struct CMapArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ2;
    size_t occ_stride;
    char* mem;
    size_t slot_stride, off_anchor;
    int h, w, n, slot0;
    float thresh, tear;
    int use_occ;
    uint32_t cur[kTemporalMaxSlots / 32], empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32], deflayer[kTemporalMaxSlots / 32];
};
void launch_cmap_step(const CMapArgs& a, hipStream_t s);
void launch_cmap_render(const CMapArgs& a, hipStream_t s);

// ---- moving-object detection (k_objects.hip; the semantics: objects.h) ----
// One step covers n pairs: pair k's inputs (mask: h*w bytes; fwd / bwd: h*w float2; occ2: h*w bytes) lie k * (their stride) bytes past
// pair 0's and feed slot slot0 + k, whose block lies (slot0 + k) * slot_stride bytes past `mem`: parent | root | area (h*w words each) |
// labels | carried (h*w bytes each) | chunk counts (2 words per chunk of 1024 indices) | records (256 x 64 B, entry = label) | votes
// ((max_objects + 1)^2 words) | header (32 B), prev_id, prev_age (256 words each).  bwd NULL: no carry (the carried plane becomes zero).
// The per-slot bits travel in the kernel arguments as TFilterArgs' do: empty (the carried plane counts as zero and next_id as 1) and cut
// (image 2 starts another clip: the carried plane becomes zero).
struct ObjArgs {
    const uint8_t* mask;
    size_t mask_stride;
    const float* fwd;
    size_t fwd_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ2;
    size_t occ_stride;
    char* mem;
    size_t slot_stride, off_root, off_area, off_labels, off_carried, off_chunks, off_rec, off_votes, off_hdr;
    int h, w, n, slot0;
    int tiles_x, tiles_y, nchunks;
    int connectivity, min_area, max_objects, min_overlap;
    uint32_t empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32];
};
// a slot's header on the device; err: a loop of a kernel hit its iteration cap (never, unless the code is wrong)
struct ObjHeader {
    int32_t n, n_found, n_components, next_id;
    uint32_t err, pad[3];
};
void launch_objects_label(const ObjArgs& a, hipStream_t s);       // tile, merge, flatten + areas, count, scan, number, label + records + votes
void launch_objects_assign(const ObjArgs& a, hipStream_t s);      // the identity rule, then the carry

// ---- background plates (k_plate.hip; the arithmetic: plate.h) ----
// One step covers n pairs: pair k's inputs (image 1: RGBA words, img_pitch bytes per row; mask: h*w bytes; model: the pair's GmModel, or
// NULL for a step without a fit) lie k * (their stride) bytes past pair 0's and feed slot slot0 + k, whose block lies (slot0 + k) *
// slot_stride bytes past `mem`: canvas (ch*cw float4, ch = h + 2*my, cw = w + 2*mx) | two blocked planes of h*w bytes each, the dilated
// mask of the last step and of the last render on a caller's mask (off_b: the one this launch writes or reads) | PlateRec (off_rec).  The per-slot bits travel in the kernel arguments
// as TFilterArgs' do: empty (every canvas state counts as n = 0 and is not read) and cut (image 2 starts another clip: the path becomes
// the identity after the step).  A render covers one slot and carries its forms in the arguments.
struct PlateArgs {
    const uint8_t* img1;
    size_t img_pitch, img_stride;
    const uint8_t* mask;
    size_t mask_stride;
    const char* model;
    size_t model_stride;
    char* mem;
    size_t slot_stride, off_b, off_rec;
    int h, w, ch, cw, mx, my, n, slot0;
    int grow, accept_invalid, n_max, min_count, phase;
    float thresh;
    uint32_t empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32];
};
struct PlateRenderArgs {
    const uint8_t* img1;
    size_t img_pitch;
    const char* canvas;             // the slot's ch*cw float4
    const uint8_t* blocked;         // h*w bytes
    uint32_t* out;
    size_t out_pitch;               // bytes per row of out
    uint8_t* fill;                  // h*w bytes
    int h, w, ch, cw, mx, my, min_count, ok;
    float inv[6];
};
void launch_plate_path(const PlateArgs& a, hipStream_t s);          // a.phase 0: the forms of P; 1: P advanced by the model, the identity after a cut
void launch_plate_block(const PlateArgs& a, hipStream_t s);         // mask -> the plane at off_b
void launch_plate_accumulate(const PlateArgs& a, hipStream_t s);
void launch_plate_render(const PlateRenderArgs& a, hipStream_t s);
// the canvas states as RGBA words (cw words per row) and coverage bytes
void launch_plate_word(const char* canvas, uint32_t* words, uint8_t* cov, int ch, int cw, hipStream_t s);

// ---- film-defect removal (k_defect.hip; the arithmetic: defect.h) ----
// One step covers n pairs: pair k's inputs (image 1 / image 2: RGBA words, img_pitch bytes per row; fwd / bwd: h*w float2) lie k * (their
// stride) bytes past pair 0's and feed slot slot0 + k, whose block lies (slot0 + k) * slot_stride bytes past `mem`: saved backward plane 0
// | 1 (h*w float2 each) | saved frame 0 | 1 | replacement | out (h*w RGBA words each) | code | mask (h*w bytes each); the slot's four
// counters (eppm_defect_stats) lie (slot0 + k) * 16 bytes past `stats`.  The per-slot bits travel in the kernel arguments as TFilterArgs'
// do: cur (which saved set is the previous frame's; the step writes the other) and detect (the saved set belongs to the frame before
// image 1 and no cut follows: the step detects; otherwise it passes image 1 through).
struct DefectArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* fwd;
    size_t fwd_stride;
    const float* bwd;
    size_t bwd_stride;
    char* mem;
    size_t slot_stride;
    int32_t* stats;
    int h, w, n, slot0;
    float detect, agree;
    int radius, grow;
    uint32_t cur[kTemporalMaxSlots / 32], active[kTemporalMaxSlots / 32];
};
// the planes of a slot's block, in bytes from its start (px = h*w)
constexpr size_t defect_off_bwd(size_t px, int which) { return (size_t)which * px * 8; }
constexpr size_t defect_off_img(size_t px, int which) { return px * 16 + (size_t)which * px * 4; }
constexpr size_t defect_off_repl(size_t px) { return px * 24; }
constexpr size_t defect_off_out(size_t px) { return px * 28; }
constexpr size_t defect_off_code(size_t px) { return px * 32; }
constexpr size_t defect_off_mask(size_t px) { return px * 33; }
void launch_defect_detect(const DefectArgs& a, hipStream_t s);
void launch_defect_apply(const DefectArgs& a, hipStream_t s);

// ---- flicker removal (k_deflicker.hip; the arithmetic: deflicker.h) ----
// One step covers n pairs: pair k's inputs (TFilterArgs' planes) lie k * (their stride) bytes past pair 0's and feed slot slot0 + k, whose
// block lies (slot0 + k) * slot_stride bytes past `mem`: reference 0 | 1 (h*w RGBA words each) | sums (13 words per cell) | field (6 floats
// per cell: the three gains, the three offsets) | valid (a byte per cell).  A step is iters x (accumulate, field) and one apply launch;
// `pass` and `bound` are the launch's.  The per-slot bits travel in the kernel arguments as TFilterArgs' do: cur (which reference is the
// previous output; the apply writes the other), empty (the reference is image 1) and cut (no pixel is sampled, so the output is image 2).
struct DeflickerArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ2;
    size_t occ_stride;
    char* mem;
    size_t slot_stride;
    int h, w, n, slot0;
    int cell, cx, cy, pass, n_min;
    float bound, keep;
    uint32_t cur[kTemporalMaxSlots / 32], empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32];
};
// the planes of a slot's block, in bytes from its start (px = h*w, cells = cx*cy); sums, field and valid start on a multiple of 16
constexpr size_t deflicker_off_ref(size_t px, int which) { return (size_t)which * px * 4; }
constexpr size_t deflicker_off_sums(size_t px) { return (px * 8 + 15) & ~(size_t)15; }
constexpr size_t deflicker_off_field(size_t px, size_t cells) { return deflicker_off_sums(px) + ((cells * 52 + 15) & ~(size_t)15); }
constexpr size_t deflicker_off_valid(size_t px, size_t cells) { return deflicker_off_field(px, cells) + ((cells * 24 + 15) & ~(size_t)15); }
constexpr size_t deflicker_slot_bytes(size_t px, size_t cells) { return deflicker_off_valid(px, cells) + cells; }
void launch_deflicker_accumulate(const DeflickerArgs& a, hipStream_t s);
void launch_deflicker_field(const DeflickerArgs& a, hipStream_t s);
void launch_deflicker_apply(const DeflickerArgs& a, hipStream_t s);

// ---- deinterlacing (k_deint.hip; the arithmetic: deint.h) ----
// One step covers n pairs, laid out as DeflickerArgs' are; a slot's block: reference 0 | 1 (h*w RGBA words each) | mask (a byte per pixel).
// The per-slot bits: cur (which reference is the previous output; the step writes the other), empty (the reference is image 1), cut (no
// candidate is accepted) and parity (which rows of image 2 are real: bit set = the odd rows).
struct DeintArgs {
    const uint8_t* img1;
    const uint8_t* img2;
    size_t img_pitch, img_stride;
    const float* bwd;
    size_t bwd_stride;
    const uint8_t* occ2;
    size_t occ_stride;
    char* mem;
    size_t slot_stride;
    int h, w, n, slot0;
    int thresh, use_occ;
    uint32_t cur[kTemporalMaxSlots / 32], empty[kTemporalMaxSlots / 32], cut[kTemporalMaxSlots / 32], parity[kTemporalMaxSlots / 32];
};
constexpr size_t deint_off_ref(size_t px, int which) { return (size_t)which * px * 4; }
constexpr size_t deint_off_mask(size_t px) { return px * 8; }
constexpr size_t deint_slot_bytes(size_t px) { return px * 9; }
void launch_deint_step(const DeintArgs& a, hipStream_t s);
// the full h x w frame of a field picture of parity p (fh = (h - p + 1) / 2 rows), both on caller planes; pitches in bytes
void launch_deint_bob(uint32_t* out, size_t out_pitch, const uint32_t* field, size_t field_pitch, int h, int w, int parity, hipStream_t s);

// ---- flow colour coding (k_color.hip) ----
// rgba: h*w packed R | G<<8 | B<<16 (alpha 0); flow: h*w float2
void launch_flow_to_color(uint32_t* rgba, const float* flow, int h, int w, float max_disp_x, float max_disp_y, hipStream_t s, Batch bt = kOnePair);

// ---- probes (k_prepare.hip) ----
void launch_probe_delta(const float* x, float* y, int n, const float* delta_tab, hipStream_t s);
void launch_probe(const float* x, float* y, int n, int which, hipStream_t s);
void launch_probe_unpack(const uint32_t* w, float* y, int n, hipStream_t s);

// ---- host XORWOW (xorwow_host.cpp) ----
struct XorwowState { uint32_t v[5]; uint32_t d; };
void xorwow_init(XorwowState* s, unsigned long long seed, unsigned long long subsequence);
uint32_t xorwow_next(XorwowState* s);
// out[160*5]: row-vector GF(2) matrix advancing the xorshift words by n draws
void xorwow_skip_matrix(unsigned long long n, uint32_t* out);

}  // namespace eppm
