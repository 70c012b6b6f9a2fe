// test_hooks.cpp -- libeppm_hip_test.so only (include/eppm_test.h): the kernel-variant switches and arithmetic probes of the parity
// tests.  The product libraries are linked without this file and export none of it (with -DEPPM_TOL=1: libeppm_hip_tol_test.so).
#define EPPM_TEST_HOOKS 1
#include "api_internal.h"

#include <array>

using namespace eppm;

std::atomic<int> g_opt_rand_table{1};
std::atomic<int> g_opt_sweep_spec{-1};
std::atomic<int> g_opt_no_split{0};
std::atomic<int> g_opt_force_split{0};
std::atomic<int> g_opt_search_pre{-1};
std::atomic<int> g_opt_c2f_pre{-1};
std::atomic<int> g_opt_alloc_fill{-1};

// "launch_log": the record behind eppm::g_launch_note; entries of six ints, capped so that a forgotten log cannot grow without bound
static struct { std::mutex mu; std::vector<std::array<int, 6>> v; bool on = false; } g_log;
static void launch_log_add(int stage, int w, int h, int npairs, int form, int extra)
{
    std::lock_guard<std::mutex> lk(g_log.mu);
    if (g_log.on && g_log.v.size() < (size_t)1 << 16) g_log.v.push_back({stage, w, h, npairs, form, extra});
}

// "alloc_fill": the block an allocation site is about to hand out, filled with the chosen byte (api_internal.h)
hipError_t alloc_fill(hipError_t e, void* p, size_t bytes, bool pinned)
{
    const int v = opt_alloc_fill();
    if (e != hipSuccess || v < 0 || !p || !bytes) return e;
    if (pinned) { memset(p, v, bytes); return hipSuccess; }
    e = hipMemset(p, v, bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}

static int probe(const float* x, float* y, int n, int which)
{
    float *dx = nullptr, *dy = nullptr;
    HIPCHK(hipMalloc(&dx, (size_t)n * 4));
    HIPCHK(hipMalloc(&dy, (size_t)n * 4));
    HIPCHK(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_probe(dx, dy, n, which, nullptr);
    HIPCHK(hipMemcpy(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy);
    return launcher_finish();
}
extern "C" int eppm_test_set_option(const char* name, int value)
{
    if (!name) return set_err(EPPM_ERR_ARG, "eppm_test_set_option: NULL name");
    if (!strcmp(name, "c2f_no_split")) { g_opt_no_split.store(value); return EPPM_OK; }
    if (!strcmp(name, "c2f_force_split")) { g_opt_force_split.store(value); return EPPM_OK; }
    if (!strcmp(name, "sweep_spec")) { g_opt_sweep_spec.store(value); return EPPM_OK; }
    if (!strcmp(name, "rand_table")) { g_opt_rand_table.store(value); return EPPM_OK; }
    if (!strcmp(name, "search_pre_from")) { g_opt_search_pre.store(value); return EPPM_OK; }
    if (!strcmp(name, "c2f_pre")) {
        if (value < -1 || value > 1) return set_err(EPPM_ERR_ARG, "eppm_test_set_option: c2f_pre %d is none of -1, 0, 1", value);
        g_opt_c2f_pre.store(value);
        return EPPM_OK;
    }
    if (!strcmp(name, "launch_log")) {          // 1: an empty log from now on; 0: none (the entries are dropped)
        g_launch_note.store(nullptr);
        { std::lock_guard<std::mutex> lk(g_log.mu); g_log.v.clear(); g_log.on = value != 0; }
        if (value) g_launch_note.store(launch_log_add);
        return EPPM_OK;
    }
    if (!strcmp(name, "alloc_fill")) {
        if (value < -1 || value > 255) return set_err(EPPM_ERR_ARG, "eppm_test_set_option: alloc_fill %d is neither -1 (off) nor a byte", value);
        g_opt_alloc_fill.store(value);
        return EPPM_OK;
    }
    return set_err(EPPM_ERR_ARG, "eppm_test_set_option: unknown option '%s'", name);
}
extern "C" int eppm_probe_c2f_window(int patch_r, int* span_x, int* span_y)
{
    if (!span_x || !span_y) return set_err(EPPM_ERR_ARG, "eppm_probe_c2f_window: NULL argument");
    if (!c2f_window_span(patch_r, span_x, span_y)) return set_err(EPPM_ERR_ARG, "no LDS-window refine kernel for patch_r %d", patch_r);
    return EPPM_OK;
}
// the launchers' own decision functions (eppm_internal.h: EPPM_DECISION), on the host alone
extern "C" int eppm_probe_dispatch(const char* stage, const int* args, int nargs, int* out, int nout)
{
    if (!stage || !args || !out) return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: NULL argument");
    auto shape = [&](int want_args, int want_out) -> int {
        if (nargs == want_args && nout == want_out && args[0] >= 1 && args[1] >= 1) return EPPM_OK;
        return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: '%s' takes %d arguments (w, h >= 1 first) and gives %d results", stage, want_args, want_out);
    };
    if (!strcmp(stage, "smoothing")) {          // w, h, npairs -> pixels per lane
        CHK(shape(3, 1));
        out[0] = flow_blf_pixels_per_lane(args[0], args[1], args[2]);
        return EPPM_OK;
    }
    if (!strcmp(stage, "refine")) {             // w, h, R, npairs, no_split -> split factor
        CHK(shape(5, 1));
        out[0] = c2f_refine_split_factor(args[0], args[1], args[2], args[3], args[4] != 0);
        return EPPM_OK;
    }
    if (!strcmp(stage, "search")) {             // w, h, R, problems, npairs, table -> rows per workgroup
        CHK(shape(6, 1));
        out[0] = pm_search_rows(args[0], args[1], args[2], args[3], args[4], args[5] != 0);
        return EPPM_OK;
    }
    if (!strcmp(stage, "sweep")) {              // w, h, R, seg_len, dir, problems, npairs -> lanes per chain, up-front fetch, source tile in LDS
        CHK(shape(7, 3));
        if (args[3] < 1) return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: seg_len %d", args[3]);
        const SweepForm f = pm_sweep_form(args[0], args[1], args[2], args[3], args[4], args[5], args[6]);
        out[0] = f.lpc; out[1] = f.pre; out[2] = f.tile;
        return EPPM_OK;
    }
    if (!strcmp(stage, "levels")) {             // w, h, levels, level -> number of levels, and that level's w, h (eppm_level_dims of such a context)
        CHK(shape(4, 3));
        int H[kMaxLevels], W[kMaxLevels];
        if (args[2] < 1 || args[2] > kMaxLevels) return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: levels %d", args[2]);
        const int nl = pyr_init_dim(H, W, args[1], args[0], args[2], 0.5f);
        if (args[3] < 0 || args[3] >= nl) return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: level %d of %d", args[3], nl);
        out[0] = nl; out[1] = W[args[3]]; out[2] = H[args[3]];
        return EPPM_OK;
    }
    if (!strcmp(stage, "patchmatch")) {        // w, h, iteration, problems, npairs -> sweeps speculative, sweeps merged ("sweep_spec" at -1)
        CHK(shape(5, 2));
        if (args[2] < 0 || args[3] < 1 || args[4] < 1) return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: iteration %d, problems %d, npairs %d", args[2], args[3], args[4]);
        const long long problem_pixels = (long long)args[0] * args[1], pixels = problem_pixels * args[3] * args[4];
        out[0] = sweep_speculative(args[2], pixels, -1) ? 1 : 0;
        out[1] = sweeps_merged(args[2], pixels, problem_pixels, -1) ? 1 : 0;
        return EPPM_OK;
    }
    return set_err(EPPM_ERR_ARG, "eppm_probe_dispatch: unknown stage '%s'", stage);
}
// the launches noted since "launch_log" was switched on (eppm_internal.h: launch_note): returns their number, the first `cap` of them in out
extern "C" int eppm_probe_launch_log(int* out, int cap)
{
    if (cap > 0 && !out) return 0;
    std::lock_guard<std::mutex> lk(g_log.mu);
    for (size_t i = 0; i < g_log.v.size() && (int)i < cap; i++) memcpy(out + 6 * i, g_log.v[i].data(), 6 * sizeof(int));
    return (int)g_log.v.size();
}
// the two-phase search's decision (eppm_internal.h: pm_search_pretest) and the knobs its pre-test was built with
extern "C" int eppm_probe_search_pretest(int iteration, int w, int h, int patch_r, int problems, int npairs, int* out, float* eps)
{
    if (!out || !eps || iteration < 0 || w < 1 || h < 1 || patch_r < 1 || problems < 1 || npairs < 1) return set_err(EPPM_ERR_ARG, "eppm_probe_search_pretest: bad argument");
    out[0] = pm_search_pretest(iteration, w, h, patch_r, problems, npairs) ? 1 : 0;
    pm_search_pretest_knobs(patch_r, &out[1], &out[2], &out[3], eps);
    out[4] = pm_search_pretest_form(w, h, patch_r, problems, npairs) ? 1 : 0;
    return EPPM_OK;
}
// the knobs of the two-phase window refine (eppm_internal.h: c2f_pretest_knobs)
extern "C" int eppm_probe_c2f_pretest(int patch_r, int* out, float* fl)
{
    if (!out || !fl || patch_r != 9) return set_err(EPPM_ERR_ARG, "eppm_probe_c2f_pretest: bad argument (the two-phase form exists at patch_r 9)");
    c2f_pretest_knobs(patch_r, &out[0], &out[1], &out[2], &out[3], &out[4], &fl[0], &fl[1], &fl[2]);
    return EPPM_OK;
}
extern "C" int eppm_probe_fast_exp(const float* x, float* y, int n) { return probe(x, y, n, 0); }
extern "C" int eppm_probe_div_const(const float* x, float* y, int n, int which) { return probe(x, y, n, 1 + which); }
// y[i] = the table form of a range term at the distance x[i] (which = 0: 1 - exp(-d^2 / LAMBDA_AD^2) of the patch data term -- exact
// library only, the tolerance library has no such table --, 1: exp(-d^2 / SIG_R^2) of the smoothing / weighted-median weights)
extern "C" int eppm_probe_delta_table(const float* x, float* y, int n, int which)
{
    if (!x || !y || n < 1 || which < 0 || which > 1) return set_err(EPPM_ERR_ARG, "eppm_probe_delta_table: bad argument");
    float *lut = nullptr, *dx = nullptr, *dy = nullptr;
    size_t head = 0;
    if (which == 0) {
#ifdef EPPM_TOL
        return set_err(EPPM_ERR_ARG, "eppm_probe_delta_table: the tolerance library's patch term has no delta table");
#else
        CHK(upload_pm_lut(&lut, 9));
        head = 9 + 1 + 9;
#endif
    } else {
        CHK(upload_blf_lut(&lut));
        head = kBlfRadius + 1;
    }
    HIPCHK(hipMalloc(&dx, (size_t)n * 4));
    HIPCHK(hipMalloc(&dy, (size_t)n * 4));
    HIPCHK(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_probe_delta(dx, dy, n, lut + head, nullptr);
    HIPCHK(hipMemcpy(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(lut);
    return launcher_finish();
}
// y[8i .. 8i+3] = unpack_texel(w[i]), y[8i+4 .. 8i+7] = make_texel(w[i], w[i] >> 24)
extern "C" int eppm_probe_unpack_texel(const uint32_t* w, float* y, int n)
{
    if (!w || !y || n < 1) return set_err(EPPM_ERR_ARG, "eppm_probe_unpack_texel: bad argument");
    uint32_t* dw = nullptr;
    float* dy = nullptr;
    HIPCHK(hipMalloc(&dw, (size_t)n * 4));
    HIPCHK(hipMalloc(&dy, (size_t)n * 32));
    HIPCHK(hipMemcpy(dw, w, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_probe_unpack(dw, dy, n, nullptr);
    HIPCHK(hipMemcpy(y, dy, (size_t)n * 32, hipMemcpyDeviceToHost));
    (void)hipFree(dw); (void)hipFree(dy);
    return launcher_finish();
}
