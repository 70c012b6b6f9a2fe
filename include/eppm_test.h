/*
 * eppm_test.h -- test support of the EPPM engine: exported by libeppm_hip_test.so ONLY.
 *
 * libeppm_hip_test.so is libeppm_hip.so's own objects (every kernel, the launchers, the C++ class: the same .o files) with
 * eppm_api.cpp compiled once more with -DEPPM_TEST_HOOKS and k_probe.hip added (eppm_amd/csrc/Makefile).  It exports everything
 * include/eppm.h declares plus the entry points below; the product library exports none of them and has no switch a host
 * program could flip: `nm -D libeppm_hip.so | grep -c "eppm_test\|eppm_probe"` is 0 (tests/test_abi_cpu.py).
 * The parity tests load the test library; bench.py, smoke(), the CLI and the C++ class link the product library.
 *
 * libeppm_hip_tol_test.so is the same construction on the tolerance library's objects (-DEPPM_TOL): the stage parity tests of the
 * tolerance kernels load it in child processes.  Everything below works there -- eppm_probe_c2f_window reports that build's own window
 * (50 rows) --, except that eppm_probe_delta_table(which = 0) returns EPPM_ERR_ARG: the tolerance patch term has no such table.
 * Its window refine has no two-phase form either: eppm_probe_c2f_pretest reports it off, eppm_test_c2f_refine_pre with pre = 1 and
 * eppm_test_c2f_refine_probe return EPPM_ERR_ARG.
 */
#ifndef EPPM_TEST_H_
#define EPPM_TEST_H_

#include "eppm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* switches with which the parity tests steer launches onto a specific kernel variant (a host program never needs them;
 * every variant computes the same bits).  A call sets the DEFAULT that contexts created afterwards copy, and what the context-less stage
 * launchers below read; a context that exists already is not affected.  "c2f_no_split" = 1: the candidate refine is never split over
 * several workgroups per tile, so that small images run the LDS-window kernels too.  "c2f_force_split" = 1: the context-less stage launchers
 * of the candidate refine (baoCudaBLFCostFilterRefine, baoCudaBLF_C2F), which otherwise never split, bring the scratch of 36 costs per
 * pixel and split wherever the library's decision (eppm_probe_dispatch "refine") says so; "c2f_no_split" still wins.  "sweep_spec": -1 (default) the sweeps of PatchMatch
 * iterations >= 2 (the third on) run in the speculative two-launch form when a launch covers at least 100 000 pixels (two 1024x436 pairs,
 * one 1920x1080 pair), 0 never, 1 always (also in eppm_pm_seg_propagate, which otherwise runs the classic form), 2 always and without
 * the work list (phase B walks every chain), 3 always and in the merged form (one phase A for the four sweeps of an iteration, the form the
 * library takes by itself from the sixth iteration on -- from the eighth on problems of more than 65 536 pixels, i.e. the quarter-resolution
 * level of 1920x1080 and 3840x2160 pairs).  "rand_table": 1 (default) a context's random searches read numbers drawn ahead per geometry,
 * 0 they draw while they search -- the form a context takes by itself when the table would exceed 512 MB; 2: as 1, and the stand-alone
 * eppm_pm_random_search, which otherwise draws while it searches, reads its launch's numbers drawn ahead as well (radius 9 and 17).
 * "search_pre_from": -1 (default) a context's random searches take the two-phase form (pre-test on the centre rows, then the survivors
 * in full) from the iteration the library itself chooses (eppm_probe_search_pretest), k >= 0: from iteration k on -- beyond the last
 * iteration: never --, wherever the launch has a two-phase form at all (patch radius 9, quarter-block workgroups).
 * "c2f_pre": -1 (default) the radius-9 window refine treats its coherent tiles as the library was built (eppm_probe_c2f_pretest), 0 in the
 * one-phase form, 1 in the two-phase form (pre-test on the centre rows, the best estimate in full, then the survivors).
 * "launch_log": 1 starts an empty record of what the launchers decide from now on (eppm_probe_launch_log), 0 (default) drops it.
 * "alloc_fill" is of another kind: it selects no kernel, it poisons memory.  -1 (default) off; 0..255: every block the library allocates
 * from then on -- a context's slab and its lazily made blocks (backward flow, interpolation, motion blur, streaming), the pinned staging
 * buffers, the state blocks of the attachments (tracker, temporal filter, stabiliser, cut detector, correspondence map, object detector),
 * whether fresh, taken from the cache of destroyed contexts' blocks or allocated again after that cache was emptied, and the generator
 * tables, generator work states and the stage launchers' scratch (at every call that asks for a slot) -- is filled with that byte before its pointer is handed out (device
 * blocks: hipMemset + hipDeviceSynchronize; pinned blocks: memset); any other value: EPPM_ERR_ARG.  Every result must be the same bits
 * under every fill: nothing may read what nothing wrote ("Write-before-read of every allocation"; tests/test_alloc_fill_gpu.py). */
int  eppm_test_set_option(const char* name, int value);
/* admissible spread (max - min, pixels) of a 16x16 tile's candidate centres for which the LDS-window refine kernels stage the
 * target window; wider tiles take the per-access path inside the same launch (patch_r 9 or 17) */
int  eppm_probe_c2f_window(int patch_r, int* span_x, int* span_y);
/* the candidate refine (baoCudaBLFCostFilterRefine) of npairs pairs of one size in ONE launch, as a batch context issues it: device planes
 * unpitched and pair after pair -- flow npairs x h x w float2 (refined in place), images npairs x h x w RGBA words, census npairs x h x w
 * bytes.  Patch radius from eppm_set_launcher_params; never split ("c2f_no_split" or not: this entry brings no cost scratch). */
int  eppm_test_c2f_refine_batch(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
                                const uint8_t* d_census2, int w, int h, int npairs);
/* The same launch with the form of the window kernel's coherent tiles chosen here (pre = 0 one-phase, 1 two-phase, -1 as built) and with
 * that kernel's counters, summed over the launch, in stat[0..7] (host memory): tiles in the two-phase form with one survivor list, tiles sent
 * to the one-phase loop because a centre-row weight sum was too small, tiles whose survivors exceeded one list -- drained in parts, still in
 * the two-phase form, or, in a library built without that (eppm_probe_c2f_pretest), sent to the one-phase loop --, tiles one-phase for any
 * other reason (incoherent, no known pixel, pre = 0), (candidate, pass) pairs tested, pairs rejected, tiles drained in halves, in quarters. */
int  eppm_test_c2f_refine_pre(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
                              const uint8_t* d_census2, int w, int h, int npairs, int pre, unsigned* stat);
/* The same launch in the two-phase form by the kernel's probing instantiation (the same code, which also stores what its pre-test formed):
 * d_probe, npairs x h x w x 73 floats of device memory, receives per pixel N[pass][candidate] (36), D_A[pass][candidate] (36) and U --
 * pass 0 the plain grid, candidate = 3 * x offset + y offset; NaN (all bits set) where the kernel formed nothing: unknown pixels, tiles that
 * are incoherent; 0 for candidate columns outside the image.  Patch radius 9, exact library. */
int  eppm_test_c2f_refine_probe(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
                                const uint8_t* d_census2, int w, int h, int npairs, float* d_probe);
/* The knobs the two-phase window refine was built with (pure host code): out[0] = on by default (0 in the tolerance library, whose kernel has no such form), out[1] the first and out[2] the number of
 * the patch rows its pre-test evaluates, out[3] the items a tile's survivor list holds, out[4] = 1 if a tile with more survivors is drained in
 * parts (0: it takes the one-phase loop); fl[0] = eps (the lower bound is shrunk by 1 - eps),
 * fl[1] = the weight sum at or below which a tile takes the one-phase loop, fl[2] = the smallest right-hand side that may reject. */
int  eppm_probe_c2f_pretest(int patch_r, int* out, float* fl);
/* ONE random-search launch over npairs x ndir problems of one size, as a context issues it: the entry builds the census and texel planes,
 * the column-parity planes and the launch's numbers drawn ahead from r's current states (which it advances by one launch, as
 * eppm_pm_random_search does).  Device planes unpitched: images npairs x h x w RGBA words; d_nnf (short2) and d_cost, searched in place,
 * (npairs * ndir) x h x w with pair p's direction k at p * ndir + k -- direction 0 matches image 1 against image 2, direction 1 image 2
 * against image 1.  pretest = 0: the one-phase kernel; 1: the rest-weight planes are filled (copied to d_restw, laid out as d_cost, unless
 * NULL) and the launch takes the two-phase form in quarter-block workgroups whatever its size -- EPPM_ERR_ARG at patch radius 17.  Patch radius (9 or 17),
 * search range and guesses from eppm_set_launcher_params.  d_pre_n, d_pre_d (both or neither; laid out as d_cost; pretest = 1 only): the
 * pre-test's two sums -- cost-weighted and plain weight sum over the centre rows -- of every pixel with its match in d_nnf AS PASSED IN as the
 * guess, formed by the search kernel's own helper on its own tile before the search runs. */
int  eppm_test_pm_search(eppm_pm_rng* r, float* d_cost, eppm_short2* d_nnf, const uint32_t* d_img1, const uint32_t* d_img2, int w, int h,
                         int ndir, int npairs, int pretest, float* d_restw, float* d_pre_n, float* d_pre_d);
/* Whether the random search of PatchMatch iteration `iteration` (0, 1, ..) of a launch of that size takes the two-phase form (the driver's
 * own decision function; pure host code): out[0] = 1 / 0; and the knobs this build's pre-test was compiled with: out[1] the first and
 * out[2] the number of the patch rows it evaluates, out[3] the threshold iteration (negative: never), *eps the factor 1 - eps that
 * shrinks its lower bound; out[4] = 1 / 0: a launch of that size has a two-phase form at all (what "search_pre_from" can switch on). */
int  eppm_probe_search_pretest(int iteration, int w, int h, int patch_r, int problems, int npairs, int* out, float* eps);
/* What the launchers decide by the size of a launch, answered by the functions the launchers themselves ask; pure host code, no GPU
 * needed.  stage, args -> out:
 *   "smoothing"  w, h, npairs                            -> pixels per lane: 1 (k_flow_blf<1>) or 2 (k_flow_blf<2>)
 *   "refine"     w, h, patch_r, npairs, no_split         -> workgroups per tile of the candidate refine: 0 (no split), 3 or 4
 *   "search"     w, h, patch_r, problems, npairs, table  -> rows of a 16x16 block per workgroup: 4 (quarter block) or 2 (eighth block)
 *   "sweep"      w, h, patch_r, seg_len, dir, problems, npairs -> classic sweep: lanes per chain (0: generic kernel), up-front fetch
 *                                                           (given an evaluation cache), source tile in LDS (0: the sweep gathers)
 *   "levels"     w, h, levels, level                     -> the pyramid a context of that size and eppm_params::levels builds: number of
 *                                                           levels, and w, h of that level (what eppm_level_dims answers, without a context)
 *   "patchmatch" w, h, iteration, problems, npairs       -> the sweeps of that PatchMatch iteration (0, 1, ..) with "sweep_spec" at its
 *                                                           default: speculative two-launch form 1 / 0, merged form 1 / 0
 * problems = directions per pair in the launch (1 or 2).  EPPM_ERR_ARG for another stage or argument count. */
int  eppm_probe_dispatch(const char* stage, const int* args, int nargs, int* out, int nout);
/* What the launchers DID since "launch_log" was set to 1, in launch order: returns the number of entries and copies the first `cap` of them,
 * six ints each: stage, w, h of one problem, pairs in the launch, form, extra --
 *   0 smoothing       form = pixels per lane                                        extra 0
 *   1 draft upsample  form = pixels per lane (k_flow_jbu<1 / 2>)                    extra 0
 *   2 refine          form = workgroups per tile (0: not split)                     extra = patch radius
 *   3 search          form = rows per workgroup (numbers drawn ahead only)          extra = 1: two-phase form
 *   4 sweep           form = 4 x lanes per chain + 2 x up-front fetch + tile, or -1: speculative two-launch form;   extra = direction
 *   5 merged sweeps   form = 1                                                      extra = iteration
 * Entries beyond 65 536 are not recorded.  0 while the log is off. */
int  eppm_probe_launch_log(int* out, int cap);
/* device-side arithmetic probes (parity of the shared float formulas): y[i] = f(x[i]) for n host floats */
int  eppm_probe_fast_exp(const float* x, float* y, int n);
int  eppm_probe_div_const(const float* x, float* y, int n, int which); /* 0: /(.1f*.1f) 1: /(.02f*.02f) 2: unorm8 (x = 0..255) */
/* the range terms that are read from a table of the 598 possible L-inf distances of unorm8 texels instead of being evaluated
 * (eppm_device.cuh: DeltaTab): y[i] = table(x[i]); which = 0: 1 - exp(-d^2/(.1f*.1f)) of the patch data term, 1: exp(-d^2/(.02f*.02f)) of
 * the smoothing and weighted-median weights.  x must be such distances (|a/255 - b/255| of two bytes, as floats). */
int  eppm_probe_delta_table(const float* x, float* y, int n, int which);
/* a word {R, G, B, census} of the 4-byte texel planes read as the exact library's PatchMatch kernels read a column-parity plane word
 * (eppm_device.cuh: unpack_texel) and as the float4 plane is built from it (make_texel): y[8i .. 8i+3] and y[8i+4 .. 8i+7], n words */
int  eppm_probe_unpack_texel(const uint32_t* w, float* y, int n);
/* the column-parity planes of a context's PatchMatch level: words per row of one parity plane and padding columns (0, 0: none), and
 * which kernels read them (bit 0 random search, bit 1 phase A of the sweeps, bit 2 cost field; 0 without planes) */
int  eppm_probe_pm_parity(const eppm_ctx* ctx, int* pitch, int* pad, int* kernels);
/* the per-block XORWOW states of a context's PatchMatch generator where its last run left them: 6 x uint32 per 16x16 block of the
 * PatchMatch level, as eppm_pm_rng_block_states (a seeded run of a streaming context must leave what a cold run leaves) */
int  eppm_probe_ctx_rng_states(eppm_ctx* ctx, uint32_t* dst, size_t dst_words);

#ifdef __cplusplus
}
#endif
#endif /* EPPM_TEST_H_ */
