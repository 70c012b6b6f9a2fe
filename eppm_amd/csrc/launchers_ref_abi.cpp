// launchers_ref_abi.cpp -- the reference's live extern "C" stage launchers with their exact argument lists (driver :40-62) and the
// sub-stage entry points the parity tests drive, all on per-device state kept here (the reference keeps the equivalent in file-scope
// textures, __constant__ tables and g_d_rand_states: SURVEY F12).  The launcher stream lives here; the caller-plane steps of the per-clip
// stage objects (each in its object's module) borrow it through launcher_run.
#include "stage_object.h"
#include "mblur.h"
#include "rshutter.h"
#include "../../include/eppm_rshutter.h"

using namespace eppm;

// ---------------------------------------------------------------------------------------------------
// state of the context-less, reference-signature launchers (the reference keeps the equivalent in
// file-scope textures, __constant__ tables and g_d_rand_states: SURVEY F12)
// ---------------------------------------------------------------------------------------------------
namespace {
struct DevState {
    float *lut_pm = nullptr, *lut_wmf = nullptr, *lut_blf = nullptr;
    int lut_R = -1;
    void* scratch[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t scratch_bytes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::map<std::tuple<int, int, int, unsigned long long>, eppm_pm_rng*> rngs;
};
std::mutex g_mu;
std::map<int, DevState> g_dev;
hipStream_t g_stream = nullptr;
eppm_params g_prm = {9, 10, 30, 6, 10, 20, 1234ULL, 0, kNumLevels};
int g_launch_status = EPPM_OK;

int dev_state(DevState** out)
{
    int d = 0;
    HIPCHK(hipGetDevice(&d));
    DevState& s = g_dev[d];
    if (s.lut_R != g_prm.patch_r) {
        (void)hipFree(s.lut_pm); s.lut_pm = nullptr;
        CHK(upload_pm_lut(&s.lut_pm, g_prm.patch_r));
        s.lut_R = g_prm.patch_r;
    }
    if (!s.lut_wmf) CHK(upload_wmf_lut(&s.lut_wmf));
    if (!s.lut_blf) CHK(upload_blf_lut(&s.lut_blf));
    *out = &s;
    return EPPM_OK;
}
int get_scratch(DevState* s, size_t bytes, void** out, int slot = 0)
{
    if (s->scratch_bytes[slot] < bytes) {
        (void)hipStreamSynchronize(g_stream);
        (void)hipFree(s->scratch[slot]);
        s->scratch[slot] = nullptr; s->scratch_bytes[slot] = 0;
        hipError_t e = hipMalloc(&s->scratch[slot], bytes);
#ifdef EPPM_TEST_HOOKS
        e = alloc_fill(e, s->scratch[slot], bytes, false);      // test library: "alloc_fill"
#endif
        HIPCHK(e);
        s->scratch_bytes[slot] = bytes;
    }
#ifdef EPPM_TEST_HOOKS
    // a slot's contents live for one call, but the block lives as long as the process: under "alloc_fill" every hand-out is a new block
    else if (opt_alloc_fill() >= 0) {
        (void)hipStreamSynchronize(g_stream);
        HIPCHK(alloc_fill(hipSuccess, s->scratch[slot], s->scratch_bytes[slot], false));
    }
#endif
    *out = s->scratch[slot];
    return EPPM_OK;
}
int get_rng(DevState* s, int w, int h, eppm_pm_rng** out)
{
    auto key = std::make_tuple(w, h, g_prm.num_guess, g_prm.seed);
    auto it = s->rngs.find(key);
    if (it == s->rngs.end()) {
        eppm_pm_rng* r = nullptr;
        CHK(rng_create(&r, w, h, g_prm));
        it = s->rngs.emplace(key, r).first;
    }
    *out = it->second;
    return EPPM_OK;
}
// The reference-signature launchers receive image and census planes apart (they were separate textures,
// kernel.cu:1770-1781); the kernels read the packed plane, built here into per-device scratch (slots 2,3).
int mk_planes(DevState* ds, PlanesH* out, const void* i1, const void* i2, const void* c1, const void* c2, int w, int h, size_t ip, size_t cp)
{
    void *a = nullptr, *b = nullptr;
    CHK(get_scratch(ds, (size_t)w * h * 16, &a, 2));
    CHK(get_scratch(ds, (size_t)w * h * 16, &b, 3));
    launch_pack(a, w, (const uint32_t*)i1, (int)(ip / 4), (const uint8_t*)c1, (int)cp, w, h, g_stream);
    launch_pack(b, w, (const uint32_t*)i2, (int)(ip / 4), (const uint8_t*)c2, (int)cp, w, h, g_stream);
    out->pk1 = a; out->pk2 = b; out->w = w; out->h = h; out->pitch = w;
    return EPPM_OK;
}
int finish() { HIPCHK(hipGetLastError()); return EPPM_OK; }
// the split refine's scratch of 36 costs per pixel (slot 8) under the test switch "c2f_force_split", else NULL: the stage launchers
// of the candidate refine have no such plane of their own and never split
int split_scratch(DevState* ds, int w, int h, float** out)
{
    *out = nullptr;
    if (!opt_force_split()) return EPPM_OK;
    void* p = nullptr;
    CHK(get_scratch(ds, (size_t)w * h * 36 * 4, &p, 8));
    *out = (float*)p;
    return EPPM_OK;
}
// device-to-device copy on the launcher stream whose failure reaches eppm_launcher_status()
int copy_d2d(void* dst, const void* src, size_t bytes)
{
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g_stream));
    return EPPM_OK;
}
}  // namespace

#define LAUNCHER_BEGIN std::lock_guard<std::mutex> lk_(g_mu); DevState* ds = nullptr; g_launch_status = dev_state(&ds); if (g_launch_status != EPPM_OK) return
#define LAUNCHER_BEGIN_INT std::lock_guard<std::mutex> lk_(g_mu); DevState* ds = nullptr; CHK(dev_state(&ds))

extern "C" int eppm_set_launcher_stream(void* s) { std::lock_guard<std::mutex> lk(g_mu); g_stream = (hipStream_t)s; return EPPM_OK; }
extern "C" int eppm_set_launcher_params(const eppm_params* p)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!p) return eppm_default_params(&g_prm);
    CHK(check_params(*p));
    g_prm = *p;
    return EPPM_OK;
}

// ---- PatchMatch sub-stages ----
extern "C" int eppm_pm_rng_create(eppm_pm_rng** out, int w, int h, const eppm_params* p)
{
    if (!out || w < 1 || h < 1) return set_err(EPPM_ERR_ARG, "eppm_pm_rng_create: bad argument");
    eppm_params q;
    eppm_default_params(&q);
    if (p) q = *p;
    CHK(check_params(q));
    return rng_create(out, w, h, q);
}
extern "C" int eppm_pm_rng_reset(eppm_pm_rng* r)
{
    if (!r) return set_err(EPPM_ERR_ARG, "NULL rng");
    const size_t bytes = (size_t)r->gx * r->gy * 64 * 6 * 4;
    HIPCHK(hipMemcpy(r->work[0][r->cur[0]], r->iter_tab, bytes, hipMemcpyDeviceToDevice));
    return EPPM_OK;
}
extern "C" int eppm_pm_rng_destroy(eppm_pm_rng* r) { rng_free(r); return EPPM_OK; }
extern "C" int eppm_pm_rng_block_states(eppm_pm_rng* r, uint32_t* dst, size_t dst_words)
{
    if (!r || !dst) return set_err(EPPM_ERR_ARG, "NULL argument");
    const int nb = r->gx * r->gy;
    if (dst_words < (size_t)nb * 6) return set_err(EPPM_ERR_ARG, "dst too small");
    HIPCHK(hipDeviceSynchronize());
    // lane 0 of each block sits at the block's sequential stream position
    HIPCHK(hipMemcpy2D(dst, 24, r->work[0][r->cur[0]], 64 * 24, 24, nb, hipMemcpyDeviceToHost));
    return EPPM_OK;
}
extern "C" int eppm_pm_gen_rand_field(eppm_pm_rng* r, eppm_short2* d_nnf, int w, int h, size_t disp_pitch)
{
    if (!r || !d_nnf || w != r->w || h != r->h) return set_err(EPPM_ERR_ARG, "eppm_pm_gen_rand_field: bad argument");
    std::lock_guard<std::mutex> lk(g_mu);
    PmBatch b;
    b.n = 1; b.cpitch = w; b.npitch = (int)(disp_pitch / 4);
    PlanesH P0;
    P0.pk1 = P0.pk2 = nullptr; P0.w = w; P0.h = h; P0.pitch = w;
    b.p[0] = mk_problem(P0, nullptr, (int16_t*)d_nnf, nullptr, r, 0);
    launch_pm_init_field(b, r->dev(), g_stream);
    return finish();
}
extern "C" int eppm_pm_cost_field(float* d_cost, const eppm_short2* d_nnf, const eppm_uchar4* i1, const eppm_uchar4* i2,
                                  const unsigned char* c1, const unsigned char* c2, int w, int h, size_t img_pitch,
                                  size_t cost_pitch, size_t disp_pitch, size_t census_pitch)
{
    LAUNCHER_BEGIN_INT;
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    CHK(mk_planes(ds, &P, i1, i2, c1, c2, w, h, img_pitch, census_pitch));
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_nnf, nullptr, nullptr, 0);
    launch_pm_cost_field(b, ds->lut_pm, g_prm.patch_r, g_stream);
    return finish();
}
extern "C" int eppm_pm_seg_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* i1, const eppm_uchar4* i2,
                                     const unsigned char* c1, const unsigned char* c2, int w, int h, size_t img_pitch,
                                     size_t cost_pitch, size_t disp_pitch, size_t census_pitch, int dir)
{
    LAUNCHER_BEGIN_INT;
    void* tmp = nullptr;
    CHK(get_scratch(ds, disp_pitch * h, &tmp));
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    CHK(mk_planes(ds, &P, i1, i2, c1, c2, w, h, img_pitch, census_pitch));
    void* spec = nullptr;
    const bool speculative = opt_sweep_spec() >= 1;         // the stand-alone entry point has no iteration count: classic unless forced
    // the evaluation cache of the sweeps lives for ONE call here (the planes of the next call may be other images): emptied first
    const size_t plane_bytes = cost_pitch * h;
    CHK(get_scratch(ds, plane_bytes * 8, &spec, 4));
    HIPCHK(hipMemsetAsync((char*)spec + plane_bytes * 4, 0xff, plane_bytes * 4, g_stream));
    b.cache_plane = plane_bytes / 4;
    void* wl = nullptr;                                        // work list of the speculative form: lengths and stamps cleared per call
    if (speculative && sweep_list_on(opt_sweep_spec())) {
        b.wl_units = pm_worklist_units(w, h, g_prm.seg_len);
        const size_t wl_bytes = pm_worklist_words(w, h, g_prm.seg_len) * 4;
        CHK(get_scratch(ds, wl_bytes, &wl, 5));
        HIPCHK(hipMemsetAsync(wl, 0, wl_bytes, g_stream));
    }
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_nnf, (int16_t*)tmp, nullptr, 0, (float*)spec, (int32_t*)((char*)spec + plane_bytes * 4), (uint32_t*)wl);
    for (int d = 0; d < 4; d++)
        if (dir < 0 || dir == d) sweep(b, ds->lut_pm, g_prm, d, g_stream, speculative);
    if (b.p[0].nnf != (int16_t*)d_nnf) HIPCHK(hipMemcpyAsync(d_nnf, b.p[0].nnf, disp_pitch * h, hipMemcpyDeviceToDevice, g_stream));
    return finish();
}
extern "C" int eppm_pm_jump_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* i1, const eppm_uchar4* i2,
                                      const unsigned char* c1, const unsigned char* c2, int w, int h, size_t img_pitch,
                                      size_t cost_pitch, size_t disp_pitch, size_t census_pitch)
{
    LAUNCHER_BEGIN_INT;
    void* tmp = nullptr;
    CHK(get_scratch(ds, disp_pitch * h, &tmp));
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    CHK(mk_planes(ds, &P, i1, i2, c1, c2, w, h, img_pitch, census_pitch));
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_nnf, (int16_t*)tmp, nullptr, 0);
    jump(b, ds->lut_pm, g_prm, g_stream);
    if (b.p[0].nnf != (int16_t*)d_nnf) HIPCHK(hipMemcpyAsync(d_nnf, b.p[0].nnf, disp_pitch * h, hipMemcpyDeviceToDevice, g_stream));
    return finish();
}
extern "C" int eppm_pm_parallel_propagate(float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* i1, const eppm_uchar4* i2,
                                          const unsigned char* c1, const unsigned char* c2, int w, int h, size_t img_pitch,
                                          size_t cost_pitch, size_t disp_pitch, size_t census_pitch)
{
    LAUNCHER_BEGIN_INT;
    void* tmp = nullptr;
    CHK(get_scratch(ds, disp_pitch * h, &tmp));
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    CHK(mk_planes(ds, &P, i1, i2, c1, c2, w, h, img_pitch, census_pitch));
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_nnf, (int16_t*)tmp, nullptr, 0);
    neighbor(b, ds->lut_pm, g_prm, 1, g_stream);
    if (b.p[0].nnf != (int16_t*)d_nnf) HIPCHK(hipMemcpyAsync(d_nnf, b.p[0].nnf, disp_pitch * h, hipMemcpyDeviceToDevice, g_stream));
    return finish();
}
extern "C" int eppm_pm_random_search(eppm_pm_rng* r, float* d_cost, eppm_short2* d_nnf, const eppm_uchar4* i1, const eppm_uchar4* i2,
                                     const unsigned char* c1, const unsigned char* c2, int w, int h, size_t img_pitch,
                                     size_t cost_pitch, size_t disp_pitch, size_t census_pitch)
{
    if (!r || w != r->w || h != r->h) return set_err(EPPM_ERR_ARG, "eppm_pm_random_search: bad rng");
    LAUNCHER_BEGIN_INT;
    if (r->G != g_prm.num_guess) return set_err(EPPM_ERR_ARG, "rng was created for num_guess=%d", r->G);
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    CHK(mk_planes(ds, &P, i1, i2, c1, c2, w, h, img_pitch, census_pitch));
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_nnf, nullptr, r, 0);
    if (opt_rand_table() == 2 && (g_prm.patch_r == 9 || g_prm.patch_r == 17)) {
        // test switch: this launch reads its numbers drawn ahead, as a context's searches do -- one launch's table (slot 7) drawn from
        // the generator's current states, which k_pm_rand_table leaves where the streaming search would have left them
        void* tab = nullptr;
        CHK(get_scratch(ds, (size_t)r->gx * r->gy * 512 * r->G * sizeof(int16_t), &tab, 7));
        PmRngDev d = r->dev();
        launch_pm_rand_table(d, r->work[0][r->cur[0]], (int16_t*)tab, r->G, g_stream);
        d.rand_tab = (const int16_t*)tab;
        launch_pm_random_search(b, d, ds->lut_pm, g_prm.patch_r, g_prm.search_range, g_prm.num_guess, g_stream);
        return finish();
    }
    search(b, r, ds->lut_pm, g_prm, g_stream);
    return finish();
}
extern "C" int eppm_gauss_filter_rgba(eppm_uchar4* d_out, const eppm_uchar4* d_in, size_t pitch, int h, int w, float sigma, int radius)
{
    if (radius < 0 || radius > 6) return set_err(EPPM_ERR_ARG, "radius %d out of range [0,6]", radius);
    std::lock_guard<std::mutex> lk(g_mu);
    launch_gauss_rgba((uint32_t*)d_out, (const uint32_t*)d_in, (int)(pitch / 4), h, w, sigma, radius, g_stream);
    return finish();
}
extern "C" int eppm_resize_rgba(eppm_uchar4* d_out, size_t out_pitch, int outH, int outW, const eppm_uchar4* d_in, size_t in_pitch,
                                int h, int w, float ratio)
{
    std::lock_guard<std::mutex> lk(g_mu);
    launch_resize_rgba((uint32_t*)d_out, (int)(out_pitch / 4), outH, outW, (const uint32_t*)d_in, (int)(in_pitch / 4), h, w, ratio, g_stream);
    return finish();
}
extern "C" int eppm_resize_flow(eppm_float2* d_out, int outH, int outW, const eppm_float2* d_in, int h, int w, float ratio)
{
    std::lock_guard<std::mutex> lk(g_mu);
    launch_resize_flow((float*)d_out, outH, outW, (const float*)d_in, h, w, ratio, 1.0f, g_stream);
    return finish();
}
// draft mode's upsampling (k_flow_jbu.hip) on caller planes; synchronous
extern "C" int eppm_flow_upsample(eppm_float2* d_out, int h, int w, const eppm_float2* d_coarse, int hc, int wc, const eppm_uchar4* d_guide,
                                  size_t guide_pitch)
{
    if (!d_out || !d_coarse || !d_guide || h < 1 || w < 1 || hc < 1 || wc < 1) return set_err(EPPM_ERR_ARG, "eppm_flow_upsample: bad argument");
    if (bad_pitch(guide_pitch, w)) return set_err(EPPM_ERR_ARG, "eppm_flow_upsample: bad pitch %zu", guide_pitch);
    if ((unsigned long long)h * (unsigned long long)guide_pitch >= (1ULL << 32) || (unsigned long long)h * (unsigned long long)w >= (1ULL << 30))
        return set_err(EPPM_ERR_ARG, "eppm_flow_upsample: size %dx%d out of range", w, h);
    LAUNCHER_BEGIN_INT;
    launch_flow_jbu((float*)d_out, (const float*)d_coarse, (const uint32_t*)d_guide, (int)(guide_pitch / 4), w, h, wc, hc, ds->lut_blf, g_stream);
    HIPCHK(hipStreamSynchronize(g_stream));
    return finish();
}

// ---------------------------------------------------------------------------------------------------
// the reference's live extern "C" launchers (driver :40-62)
// ---------------------------------------------------------------------------------------------------
extern "C" void baoCudaCensusTransform(unsigned char* d_census1, unsigned char* d_census2, eppm_uchar4* d_img1, eppm_uchar4* d_img2,
                                       int w, int h, size_t img_pitch, size_t census_pitch)
{
    std::lock_guard<std::mutex> lk(g_mu);
    launch_census(d_census1, (int)census_pitch, nullptr, 0, (const uint32_t*)d_img1, (int)(img_pitch / 4), w, h, g_stream);
    launch_census(d_census2, (int)census_pitch, nullptr, 0, (const uint32_t*)d_img2, (int)(img_pitch / 4), w, h, g_stream);
    g_launch_status = finish();
}

extern "C" void baoCudaPatchMatchMultiscalePrepare(eppm_uchar4** pImgPyr1, eppm_uchar4** pImgPyr2, unsigned char** pCensusPyr1,
        unsigned char** pCensusPyr2, eppm_uchar4** pTempPyr1, eppm_uchar4** pTempPyr2, int* arrH, int* arrW,
        size_t* arrPitchUchar4, size_t* arrPitchUchar1, int nLevels, eppm_uchar4* d_img1, eppm_uchar4* d_img2, int h, int w)
{
    std::lock_guard<std::mutex> lk(g_mu);
    hipStream_t s = g_stream;
    const float ratio = 0.5f;
    const float baseSigma = (1 / ratio - 1);
    const int n = (int)(log(0.25) / (double)logf(ratio));   // C++ float overload in the reference: n = 1
    const float nSigma = baseSigma * n;
    for (int k = 0; k < 2; k++) {
        uint32_t** pyr = (uint32_t**)(k ? pImgPyr2 : pImgPyr1);
        uint32_t** tmp = (uint32_t**)(k ? pTempPyr2 : pTempPyr1);
        const uint32_t* raw = (const uint32_t*)(k ? d_img2 : d_img1);
        // NOTE: the reference allocates its temp pyramid unpitched (driver :155-156) yet addresses it with the
        // pitched stride; here temp planes are addressed with arrPitchUchar4 as well, so they must be pitched.
        launch_gauss_rgba(pyr[0], raw, (int)(arrPitchUchar4[0] / 4), h, w, .5f, 2, s);
        for (int i = 1; i < nLevels; i++) {
            if (i <= n) {
                const float sigma = baseSigma * i;
                launch_gauss_rgba(tmp[0], pyr[0], (int)(arrPitchUchar4[0] / 4), arrH[0], arrW[0], sigma, (int)(sigma * 3), s);
                launch_resize_rgba(pyr[i], (int)(arrPitchUchar4[i] / 4), arrH[i], arrW[i], tmp[0], (int)(arrPitchUchar4[0] / 4), arrH[0], arrW[0], (float)pow(ratio, i), s);
            } else {
                const int j = i - n;
                launch_gauss_rgba(tmp[j], pyr[j], (int)(arrPitchUchar4[j] / 4), arrH[j], arrW[j], nSigma, (int)(nSigma * 3), s);
                launch_resize_rgba(pyr[i], (int)(arrPitchUchar4[i] / 4), arrH[i], arrW[i], tmp[j], (int)(arrPitchUchar4[j] / 4), arrH[j], arrW[j],
                                   (float)pow(ratio, i) * arrW[0] / arrW[j], s);
            }
        }
    }
    for (int i = 0; i < nLevels; i++) {
        launch_census(pCensusPyr1[i], (int)arrPitchUchar1[i], nullptr, 0, (const uint32_t*)pImgPyr1[i], (int)(arrPitchUchar4[i] / 4), arrW[i], arrH[i], s);
        launch_census(pCensusPyr2[i], (int)arrPitchUchar1[i], nullptr, 0, (const uint32_t*)pImgPyr2[i], (int)(arrPitchUchar4[i] / 4), arrW[i], arrH[i], s);
    }
    g_launch_status = finish();
}

extern "C" void baoCudaPatchMatch(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img1, eppm_uchar4* d_img2,
        unsigned char* d_census1, unsigned char* d_census2, int w, int h, size_t img_pitch, size_t cost_pitch,
        size_t disp_pitch, size_t census_pitch)
{
    LAUNCHER_BEGIN;
    eppm_pm_rng* r = nullptr;
    g_launch_status = get_rng(ds, w, h, &r);
    if (g_launch_status != EPPM_OK) return;
    void* tmp = nullptr;
    g_launch_status = get_scratch(ds, disp_pitch * h, &tmp);
    if (g_launch_status != EPPM_OK) return;
    PmBatch b;
    b.n = 1; b.cpitch = (int)(cost_pitch / 4); b.npitch = (int)(disp_pitch / 4);
    PlanesH P;
    g_launch_status = mk_planes(ds, &P, d_img1, d_img2, d_census1, d_census2, w, h, img_pitch, census_pitch);
    if (g_launch_status != EPPM_OK) return;
    void* spec = nullptr;
    const size_t plane_bytes = cost_pitch * h;
    g_launch_status = get_scratch(ds, plane_bytes * 8, &spec, 4);
    if (g_launch_status != EPPM_OK) return;
    b.cache_plane = plane_bytes / 4;          // (k_pm_init_field empties the cache)
    void* wl = nullptr;
    b.wl_units = pm_worklist_units(w, h, g_prm.seg_len);
    g_launch_status = get_scratch(ds, pm_worklist_words(w, h, g_prm.seg_len) * 4, &wl, 5);       // (k_pm_init_field clears it)
    if (g_launch_status != EPPM_OK) return;
    b.p[0] = mk_problem(P, d_cost, (int16_t*)d_disp_vec, (int16_t*)tmp, r, 0, (float*)spec, (int32_t*)((char*)spec + plane_bytes * 4), sweep_list_on(opt_sweep_spec()) ? (uint32_t*)wl : nullptr);
    run_patchmatch(b, r, ds->lut_pm, g_prm, g_stream, opt_sweep_spec());
    if (b.p[0].nnf != (int16_t*)d_disp_vec && (g_launch_status = copy_d2d(d_disp_vec, b.p[0].nnf, disp_pitch * h)) != EPPM_OK) return;
    g_launch_status = finish();
}

extern "C" void baoCudaLeftRightCheck(eppm_short2* d_disp_vec, float* d_cost, eppm_short2* d_disp_vec2, float* d_cost2,
        int w, int h, size_t cost_pitch, size_t disp_pitch)
{
    std::lock_guard<std::mutex> lk(g_mu);
    launch_lr_check((int16_t*)d_disp_vec, d_cost, (const int16_t*)d_disp_vec2, w, h, (int)(cost_pitch / 4), (int)(disp_pitch / 4), g_stream);
    launch_lr_check((int16_t*)d_disp_vec2, d_cost2, (const int16_t*)d_disp_vec, w, h, (int)(cost_pitch / 4), (int)(disp_pitch / 4), g_stream);
    g_launch_status = finish();
}

extern "C" void baoCudaOutlierRemoval(eppm_short2* d_disp_vec, float* d_cost, int w, int h, size_t cost_pitch, size_t disp_pitch)
{
    LAUNCHER_BEGIN;
    void* tmp = nullptr;
    g_launch_status = get_scratch(ds, disp_pitch * h, &tmp);
    if (g_launch_status != EPPM_OK) return;
    if ((g_launch_status = copy_d2d(tmp, d_disp_vec, disp_pitch * h)) != EPPM_OK) return;
    launch_outlier((int16_t*)d_disp_vec, d_cost, (const int16_t*)tmp, w, h, (int)(cost_pitch / 4), (int)(disp_pitch / 4), g_stream);
    g_launch_status = finish();
}

extern "C" void baoCudaWeightedMedianFilter(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img, int w, int h,
        size_t img_pitch, size_t cost_pitch, size_t disp_pitch, int num_iter, bool is_only_occlusion)
{
    (void)d_cost; (void)cost_pitch;
    LAUNCHER_BEGIN;
    void* tmp = nullptr;
    g_launch_status = get_scratch(ds, disp_pitch * h, &tmp);
    if (g_launch_status != EPPM_OK) return;
    void* ws = nullptr;
    g_launch_status = get_scratch(ds, wmf_workspace_words(w, h, num_iter) * 4, &ws, 1);
    if (g_launch_status != EPPM_OK) return;
    int16_t* res = launch_wmf((int16_t*)d_disp_vec, (int16_t*)tmp, (const uint32_t*)d_img, (int)(img_pitch / 4), w, h, (int)(disp_pitch / 4),
                              ds->lut_wmf, num_iter, is_only_occlusion ? 1 : 0, (uint32_t*)ws, g_stream);
    if (res != (int16_t*)d_disp_vec && (g_launch_status = copy_d2d(d_disp_vec, res, disp_pitch * h)) != EPPM_OK) return;
    g_launch_status = finish();
}

extern "C" void baoCudaFillHole(eppm_short2* d_disp_vec, float* d_cost, eppm_uchar4* d_img, int w, int h,
        size_t img_pitch, size_t cost_pitch, size_t disp_pitch)
{
    (void)d_cost; (void)cost_pitch;
    LAUNCHER_BEGIN;
    void* tmp = nullptr;
    g_launch_status = get_scratch(ds, disp_pitch * h, &tmp);
    if (g_launch_status != EPPM_OK) return;
    if ((g_launch_status = copy_d2d(tmp, d_disp_vec, disp_pitch * h)) != EPPM_OK) return;
    launch_fill_holes((int16_t*)d_disp_vec, (const int16_t*)tmp, (const uint32_t*)d_img, (int)(img_pitch / 4), w, h, (int)(disp_pitch / 4), g_stream);
    g_launch_status = finish();
}

extern "C" void baoCudaNNF2Flow(eppm_float2* d_flow, eppm_short2* d_disp_vec, int w, int h, size_t disp_pitch, size_t flow_pitch)
{
    std::lock_guard<std::mutex> lk(g_mu);
    launch_nnf2flow((float*)d_flow, (int)(flow_pitch / 8), (const int16_t*)d_disp_vec, (int)(disp_pitch / 4), w, h, g_stream);
    g_launch_status = finish();
}

extern "C" void baoCudaBLFCostFilterRefine(eppm_float2* d_flow_vec, eppm_uchar4* d_img1, eppm_uchar4* d_img2, unsigned char* d_census1,
        unsigned char* d_census2, int w, int h, size_t img_pitch, size_t census_pitch)
{
    LAUNCHER_BEGIN;
    PlanesH P;
    g_launch_status = mk_planes(ds, &P, d_img1, d_img2, d_census1, d_census2, w, h, img_pitch, census_pitch);
    if (g_launch_status != EPPM_OK) return;
    float* cost9 = nullptr;
    if ((g_launch_status = split_scratch(ds, w, h, &cost9)) != EPPM_OK) return;
    launch_c2f_refine(P, (float*)d_flow_vec, ds->lut_pm, g_prm.patch_r, cost9, g_stream, kOnePair, opt_no_split() != 0, opt_c2f_pre());
    g_launch_status = finish();
}

extern "C" void baoCudaBLF_C2F(eppm_float2** pFlowPyr, eppm_uchar4** pImgPyr1, eppm_uchar4** pImgPyr2, unsigned char** pCensusPyr1,
        unsigned char** pCensusPyr2, eppm_float2** pTempPyr1, eppm_float2** pTempPyr2, int* arrH, int* arrW,
        size_t* arrPitchUchar4, size_t* arrPitchUchar1, int nLayerIdx)
{
    (void)pTempPyr1; (void)pTempPyr2;
    LAUNCHER_BEGIN;
    const int l = nLayerIdx;
    launch_resize_flow((float*)pFlowPyr[l], arrH[l], arrW[l], (const float*)pFlowPyr[l + 1], arrH[l + 1], arrW[l + 1], 2.0f, 1.0f, g_stream);  // refine :1082
    launch_mul_scalar((float*)pFlowPyr[l], 2.0f, arrH[l], arrW[l], g_stream);                                                                  // refine :1083
    PlanesH P;
    g_launch_status = mk_planes(ds, &P, pImgPyr1[l], pImgPyr2[l], pCensusPyr1[l], pCensusPyr2[l], arrW[l], arrH[l], arrPitchUchar4[l], arrPitchUchar1[l]);
    if (g_launch_status != EPPM_OK) return;
    float* cost9 = nullptr;
    if ((g_launch_status = split_scratch(ds, arrW[l], arrH[l], &cost9)) != EPPM_OK) return;
    launch_c2f_refine(P, (float*)pFlowPyr[l], ds->lut_pm, g_prm.patch_r, cost9, g_stream, kOnePair, opt_no_split() != 0, opt_c2f_pre());                         // refine :1086
    g_launch_status = finish();
}

#ifdef EPPM_TEST_HOOKS
// include/eppm_test.h: the candidate refine of npairs pairs of one size in ONE launch, as a batch context issues it (blockIdx.y = pair).
// Caller planes unpitched, pair after pair.  A Batch has one byte stride for the texel planes and the flow, so the flow fields are spread
// to the texel planes' stride in scratch (slot 0) for the launch and gathered back.
static int c2f_refine_batch(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
        const uint8_t* d_census2, int w, int h, int npairs, int pre, unsigned* stat, float* d_probe = nullptr)
{
#ifdef EPPM_TOL
    if (pre == 1 || d_probe) return set_err(EPPM_ERR_ARG, "the tolerance library's window refine has no two-phase form");
#endif
    if (!d_flow || !d_img1 || !d_img2 || !d_census1 || !d_census2 || w < 1 || h < 1 || npairs < 1)
        return set_err(EPPM_ERR_ARG, "eppm_test_c2f_refine_batch: bad argument");
    LAUNCHER_BEGIN_INT;
    const size_t n = (size_t)w * h, stride = n * 16;
    void *a = nullptr, *b = nullptr, *f = nullptr, *st = nullptr;
    CHK(get_scratch(ds, stride * npairs, &a, 2));
    CHK(get_scratch(ds, stride * npairs, &b, 3));
    CHK(get_scratch(ds, stride * npairs + 32, &f, 0));          // + the window kernel's eight counters, after the flow fields
    if (stat) {
        st = (char*)f + stride * npairs;
        HIPCHK(hipMemsetAsync(st, 0, 32, g_stream));
    }
    for (int p = 0; p < npairs; p++) {
        launch_pack((char*)a + p * stride, w, d_img1 + p * n, w, d_census1 + p * n, w, w, h, g_stream);
        launch_pack((char*)b + p * stride, w, d_img2 + p * n, w, d_census2 + p * n, w, w, h, g_stream);
        CHK(copy_d2d((char*)f + p * stride, d_flow + p * n * 2, n * 8));
    }
    PlanesH P;
    P.pk1 = a; P.pk2 = b; P.w = w; P.h = h; P.pitch = w;
    if (d_probe) HIPCHK(hipMemsetAsync(d_probe, 0xff, n * npairs * 73 * 4, g_stream));          // what the kernel leaves unwritten reads as NaN
    launch_c2f_refine(P, (float*)f, ds->lut_pm, g_prm.patch_r, nullptr, g_stream, Batch{npairs, stride}, opt_no_split() != 0, pre, (unsigned*)st, d_probe);
    for (int p = 0; p < npairs; p++) CHK(copy_d2d(d_flow + p * n * 2, (char*)f + p * stride, n * 8));
    if (stat) { HIPCHK(hipMemcpyAsync(stat, st, 32, hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream)); }
    return finish();
}
extern "C" int eppm_test_c2f_refine_batch(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
        const uint8_t* d_census2, int w, int h, int npairs)
{
    return c2f_refine_batch(d_flow, d_img1, d_img2, d_census1, d_census2, w, h, npairs, opt_c2f_pre(), nullptr);
}
extern "C" int eppm_test_c2f_refine_pre(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
        const uint8_t* d_census2, int w, int h, int npairs, int pre, unsigned* stat)
{
    if (!stat || pre < -1 || pre > 1) return set_err(EPPM_ERR_ARG, "eppm_test_c2f_refine_pre: bad argument");
    return c2f_refine_batch(d_flow, d_img1, d_img2, d_census1, d_census2, w, h, npairs, pre, stat);
}
extern "C" int eppm_test_c2f_refine_probe(float* d_flow, const uint32_t* d_img1, const uint32_t* d_img2, const uint8_t* d_census1,
        const uint8_t* d_census2, int w, int h, int npairs, float* d_probe)
{
    if (!d_probe || g_prm.patch_r != 9) return set_err(EPPM_ERR_ARG, "eppm_test_c2f_refine_probe: bad argument (patch radius 9 only)");
    return c2f_refine_batch(d_flow, d_img1, d_img2, d_census1, d_census2, w, h, npairs, 1, nullptr, d_probe);
}
#endif

#ifdef EPPM_TEST_HOOKS
// include/eppm_test.h: ONE random-search launch over npairs x ndir problems as a context issues it -- census and texel planes, the
// column-parity planes, numbers drawn ahead (slot 7) and, for pretest != 0, the rest-weight planes, laid out pair after pair in a slab of
// one stride (slot 0).  Caller planes unpitched: images pair after pair, fields and costs problem after problem (pair p, direction k at
// p * ndir + k; direction 1 matches image 2 against image 1).
extern "C" int eppm_test_pm_search(eppm_pm_rng* r, float* d_cost, eppm_short2* d_nnf, const uint32_t* d_img1, const uint32_t* d_img2, int w, int h,
                                   int ndir, int npairs, int pretest, float* d_restw, float* d_pre_n, float* d_pre_d)
{
    if (!r || !d_cost || !d_nnf || !d_img1 || !d_img2 || w != r->w || h != r->h || ndir < 1 || ndir > 2 || npairs < 1)
        return set_err(EPPM_ERR_ARG, "eppm_test_pm_search: bad argument");
    LAUNCHER_BEGIN_INT;
    const int R = g_prm.patch_r;
    if (r->G != g_prm.num_guess || (R != 9 && R != 17)) return set_err(EPPM_ERR_ARG, "eppm_test_pm_search: num_guess %d / patch_r %d", r->G, R);
    const size_t n = (size_t)w * h;
    const int pad = (R + 2) & ~1, ppitch = parity_pitch(w, pad);
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    size_t o_img[2], o_cen[2], o_pk[2], o_pc[2], o_pp[2], o_cost[2], o_nnf[2], o_rw[2], o_pn[2], o_pd[2];
    for (int k = 0; k < 2; k++) { o_img[k] = carve(n * 4); o_cen[k] = carve(n); o_pk[k] = carve(n * 16); o_pc[k] = carve(n * 4); o_pp[k] = carve((size_t)2 * h * ppitch * 4); }
    for (int k = 0; k < ndir; k++) { o_cost[k] = carve(n * 4); o_nnf[k] = carve(n * 4); o_rw[k] = carve(n * 4); o_pn[k] = carve(n * 4); o_pd[k] = carve(n * 4); }
    const size_t stride = (off + 4095) & ~(size_t)4095;
    void *slab = nullptr, *tab = nullptr;
    CHK(get_scratch(ds, stride * npairs, &slab, 0));
    CHK(get_scratch(ds, (size_t)r->gx * r->gy * 512 * r->G * sizeof(int16_t), &tab, 7));
    char* S = (char*)slab;
    for (int p = 0; p < npairs; p++) {
        CHK(copy_d2d(S + p * stride + o_img[0], d_img1 + p * n, n * 4));
        CHK(copy_d2d(S + p * stride + o_img[1], d_img2 + p * n, n * 4));
        for (int k = 0; k < ndir; k++) {
            CHK(copy_d2d(S + p * stride + o_cost[k], d_cost + (p * ndir + k) * n, n * 4));
            CHK(copy_d2d(S + p * stride + o_nnf[k], (const char*)d_nnf + (p * ndir + k) * n * 4, n * 4));
        }
    }
    const Batch bt{npairs, stride};
    CensusBatch cb;
    cb.n = 2;
    for (int k = 0; k < 2; k++) {
        CensusJob& J = cb.job[k];
        J.census = (uint8_t*)(S + o_cen[k]); J.cpitch = w; J.texels = S + o_pk[k]; J.tpitch = w; J.img = (const uint32_t*)(S + o_img[k]); J.ipitch = w;
        J.w = w; J.h = h; J.first_block = 0; J.packed = (uint32_t*)(S + o_pc[k]);
    }
    launch_census_batch(cb, g_stream, bt);
    for (int k = 0; k < 2; k++) launch_parity_planes((uint32_t*)(S + o_pp[k]), ppitch, pad, (const uint32_t*)(S + o_pc[k]), w, w, h, g_stream, bt);
    PmBatch b;
    b.n = ndir; b.cpitch = w; b.npitch = w; b.npairs = npairs; b.stride = stride;
    for (int k = 0; k < ndir; k++) {
        PlanesH P;
        P.pk1 = S + o_pk[k]; P.pk2 = S + o_pk[k ^ 1]; P.w = w; P.h = h; P.pitch = w;
        P.pc1 = (const uint32_t*)(S + o_pc[k]); P.pc2 = (const uint32_t*)(S + o_pc[k ^ 1]);
        P.pp1 = (const uint32_t*)(S + o_pp[k]); P.pp2 = (const uint32_t*)(S + o_pp[k ^ 1]); P.pp_pitch = ppitch; P.pp_pad = pad;
        b.p[k] = mk_problem(P, (float*)(S + o_cost[k]), (int16_t*)(S + o_nnf[k]), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, (float*)(S + o_rw[k]));
    }
    PmRngDev d = r->dev();
    launch_pm_rand_table(d, r->work[0][r->cur[0]], (int16_t*)tab, r->G, g_stream);
    d.rand_tab = (const int16_t*)tab;
    if (pretest) {
        if (!pm_search_pretest_ready(b, d, R)) return set_err(EPPM_ERR_ARG, "eppm_test_pm_search: no two-phase search at patch_r %d", R);
        launch_pm_rest_weight(b, ds->lut_pm, R, g_stream);
        if (d_pre_n && d_pre_d) {          // the sums of the fields as they stand BEFORE the search
            PmPretestSums ps{};
            for (int k = 0; k < ndir; k++) { ps.n[k] = (float*)(S + o_pn[k]); ps.d[k] = (float*)(S + o_pd[k]); }
            launch_pm_pretest_probe(b, ds->lut_pm, R, ps, g_stream);
        }
    }
    launch_pm_random_search(b, d, ds->lut_pm, R, g_prm.search_range, g_prm.num_guess, g_stream, pretest != 0);
    for (int p = 0; p < npairs; p++)
        for (int k = 0; k < ndir; k++) {
            CHK(copy_d2d(d_cost + (p * ndir + k) * n, S + p * stride + o_cost[k], n * 4));
            CHK(copy_d2d((char*)d_nnf + (p * ndir + k) * n * 4, S + p * stride + o_nnf[k], n * 4));
            if (pretest && d_restw) CHK(copy_d2d(d_restw + (p * ndir + k) * n, S + p * stride + o_rw[k], n * 4));
            if (pretest && d_pre_n && d_pre_d) {
                CHK(copy_d2d(d_pre_n + (p * ndir + k) * n, S + p * stride + o_pn[k], n * 4));
                CHK(copy_d2d(d_pre_d + (p * ndir + k) * n, S + p * stride + o_pd[k], n * 4));
            }
        }
    return finish();
}
#endif

extern "C" void baoCudaFlowSmoothing(eppm_float2* d_flow, eppm_uchar4* d_img, int w, int h, size_t img_pitch, size_t flow_pitch)
{
    LAUNCHER_BEGIN;
    void* tmp = nullptr;
    g_launch_status = get_scratch(ds, flow_pitch * h, &tmp);
    if (g_launch_status != EPPM_OK) return;
    if ((g_launch_status = copy_d2d(tmp, d_flow, flow_pitch * h)) != EPPM_OK) return;
    launch_flow_blf((float*)d_flow, (const float*)tmp, (const uint32_t*)d_img, (int)(img_pitch / 4), w, h, (int)(flow_pitch / 8), ds->lut_blf, g_stream);
    g_launch_status = finish();
}

// ---- flow colour coding (basic/bao_basic_cuda.cuh:776-845; driver :308-314) ----
extern "C" int eppm_flow_to_color(eppm_uchar4* d_rgba, const eppm_float2* d_flow, int h, int w, float max_disp_x, float max_disp_y)
{
    if (!d_rgba || !d_flow || h < 1 || w < 1) return set_err(EPPM_ERR_ARG, "eppm_flow_to_color: bad argument");
    LAUNCHER_BEGIN_INT;
    (void)ds;
    launch_flow_to_color((uint32_t*)d_rgba, (const float*)d_flow, h, w, max_disp_x, max_disp_y, g_stream);
    return finish();
}
// ---- the occlusion kernel of a bidirectional call on caller planes (k_occ.hip; eppm_fb_occlusion_host is its host form) ----
extern "C" int eppm_fb_occlusion(uint8_t* d_occ, const eppm_float2* d_flow, const eppm_float2* d_other, int h, int w, float alpha, float beta)
{
    if (!d_occ || !d_flow || !d_other || h < 1 || w < 1) return set_err(EPPM_ERR_ARG, "eppm_fb_occlusion: bad argument");
    if (!(alpha >= 0 && isfinite(alpha)) || !(beta >= 0 && isfinite(beta)))
        return set_err(EPPM_ERR_ARG, "eppm_fb_occlusion: alpha %g, beta %g must be finite and >= 0", alpha, beta);
    LAUNCHER_BEGIN_INT;
    (void)ds;
    launch_fb_occlusion(d_occ, nullptr, (const float*)d_flow, 0, (const float*)d_other, 0, h, w, alpha, beta, 1, 1, g_stream);
    return finish();
}
// ---- the temporal prior on caller planes (k_temporal.hip; eppm_temporal_prior_host is its host form): one direction ----
extern "C" int eppm_temporal_prior(eppm_short2* d_prior, const eppm_short2* d_prev, int h, int w, int backward)
{
    if (!d_prior || !d_prev || h < 1 || w < 1 || h > 32767 || w > 32767) return set_err(EPPM_ERR_ARG, "eppm_temporal_prior: bad argument");
    if ((unsigned long long)h * (unsigned long long)w >= (1ULL << 30)) return set_err(EPPM_ERR_ARG, "eppm_temporal_prior: size %dx%d out of range", w, h);
    LAUNCHER_BEGIN_INT;
    void* keys = nullptr;
    CHK(get_scratch(ds, (size_t)w * h * 4, &keys, 6));
    TemporalArgs a{};
    a.prev[0] = (const int16_t*)d_prev; a.prior[0] = (int16_t*)d_prior; a.keys[0] = (int32_t*)keys; a.step[0] = backward ? -1 : 1;
    a.w = w; a.h = h; a.ndir = 1; a.nslots = 1; a.armed[0] = 1u;
    launch_temporal_keys_init(a.keys[0], w * h, g_stream);
    launch_temporal_splat(a, g_stream);
    launch_temporal_gather(a, g_stream);
    return finish();
}
// the same on npairs slots in one launch each (slot k's planes lie k*h*w short2 after slot 0's); armed: NULL (all) or a byte per slot
extern "C" int eppm_temporal_prior_batch(eppm_short2* d_prior, const eppm_short2* d_prev, int h, int w, int backward, int npairs, const uint8_t* armed)
{
    if (!d_prior || !d_prev || h < 1 || w < 1 || h > 32767 || w > 32767 || npairs < 1 || npairs > kTemporalMaxSlots)
        return set_err(EPPM_ERR_ARG, "eppm_temporal_prior_batch: bad argument");
    if ((unsigned long long)h * (unsigned long long)w * (unsigned long long)npairs >= (1ULL << 30))
        return set_err(EPPM_ERR_ARG, "eppm_temporal_prior_batch: %d slots of %dx%d out of range", npairs, w, h);
    LAUNCHER_BEGIN_INT;
    void* keys = nullptr;
    CHK(get_scratch(ds, (size_t)w * h * 4 * npairs, &keys, 6));
    TemporalArgs a{};
    a.prev[0] = (const int16_t*)d_prev; a.prior[0] = (int16_t*)d_prior; a.keys[0] = (int32_t*)keys; a.step[0] = backward ? -1 : 1;
    a.w = w; a.h = h; a.ndir = 1; a.nslots = npairs; a.stride = (size_t)w * h * 4;
    for (int k = 0; k < npairs; k++)
        if (!armed || armed[k]) a.armed[k >> 5] |= 1u << (k & 31);
    launch_temporal_keys_init(a.keys[0], w * h * npairs, g_stream);
    launch_temporal_splat(a, g_stream);
    launch_temporal_gather(a, g_stream);
    return finish();
}
// ---- frame interpolation on caller planes (k_interp.hip; eppm_interpolate_host is its host form): one pair, one time ----
extern "C" int eppm_interpolate_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba1, const void* d_rgba2, size_t in_pitch,
                                       const eppm_float2* d_flow, const uint8_t* d_occ1, const uint8_t* d_occ2, int h, int w, float t)
{
    if (!d_rgba_out || !d_rgba1 || !d_rgba2 || !d_flow || !d_occ1 || !d_occ2 || h < 1 || w < 1) return set_err(EPPM_ERR_ARG, "eppm_interpolate_frames: bad argument");
    if (!(t >= 0.0f && t <= 1.0f)) return set_err(EPPM_ERR_ARG, "eppm_interpolate_frames: t = %g outside [0, 1]", t);
    if (bad_pitch(in_pitch, w) || bad_pitch(out_pitch, w))
        return set_err(EPPM_ERR_ARG, "eppm_interpolate_frames: bad pitch %zu / %zu", in_pitch, out_pitch);
    if ((unsigned long long)h * (unsigned long long)w >= (1ULL << 31)) return set_err(EPPM_ERR_ARG, "eppm_interpolate_frames: size %dx%d out of range", w, h);
    LAUNCHER_BEGIN_INT;
    const size_t plane = ((size_t)h * w + 63) & ~(size_t)63;
    void* scr = nullptr;
    CHK(get_scratch(ds, plane * 16, &scr, 6));          // keys | fill1 | fill2
    InterpArgs a{};
    a.img1 = (const uint8_t*)d_rgba1; a.img2 = (const uint8_t*)d_rgba2; a.img_pitch = in_pitch;
    a.flow = (const float*)d_flow;
    a.occ1 = d_occ1; a.occ2 = d_occ2;
    a.keys = (uint64_t*)scr; a.fill1 = (int32_t*)((char*)scr + plane * 8); a.fill2 = (int32_t*)((char*)scr + plane * 12); a.plane = plane;
    a.rgba[0] = (uint8_t*)d_rgba_out; a.rgba_pitch = out_pitch;
    a.h = h; a.w = w; a.nt = 1; a.t[0] = t;
    launch_interp_splat(a, 1, g_stream);
    launch_interp_fill(a, 1, g_stream);
    launch_interp_blend(a, 1, g_stream);
    return finish();
}
// ---- the synthetic shutter on caller planes (k_mblur.hip; eppm_motion_blur_host is its host form): one frame ----
extern "C" int eppm_motion_blur_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba, size_t in_pitch, const eppm_float2* d_flow, int h, int w,
                                       const eppm_mblur_params* params)
{
    eppm_mblur_params prm;
    if (params) prm = *params;
    else (void)eppm_mblur_default_params(&prm);
    if (!d_rgba_out || !d_rgba || !d_flow || h < 1 || w < 1) return set_err(EPPM_ERR_ARG, "eppm_motion_blur_frames: bad argument");
    if (!mblur_params_ok(prm.shutter, prm.max_radius, prm.taps))
        return set_err(EPPM_ERR_ARG, "eppm_motion_blur_frames: shutter %g (0 < s <= 1), max_radius %g (1 .. 31), taps %d (1 .. 32)", prm.shutter, prm.max_radius, prm.taps);
    if (bad_pitch(in_pitch, w) || bad_pitch(out_pitch, w))
        return set_err(EPPM_ERR_ARG, "eppm_motion_blur_frames: bad pitch %zu / %zu", in_pitch, out_pitch);
    if (h > 8192 || w > 8192 || (unsigned long long)h * (unsigned long long)w > (1ULL << 26))
        return set_err(EPPM_ERR_ARG, "eppm_motion_blur_frames: size %dx%d out of range", w, h);
    LAUNCHER_BEGIN_INT;
    MBlurArgs a{};
    a.tiles_x = (w + kMBlurTile - 1) / kMBlurTile; a.tiles_y = (h + kMBlurTile - 1) / kMBlurTile;
    a.plane = ((size_t)h * w + 63) & ~(size_t)63; a.tplane = (size_t)a.tiles_x * a.tiles_y;
    void* scr = nullptr;
    CHK(get_scratch(ds, a.plane * 4 + a.tplane * 8, &scr, 6));          // packed | tile keys
    a.img = (const uint8_t*)d_rgba; a.img_pitch = in_pitch;
    a.flow = (const float*)d_flow;
    a.packed = (uint32_t*)scr; a.tkeys = (uint64_t*)((char*)scr + a.plane * 4);
    a.rgba = (uint8_t*)d_rgba_out; a.rgba_pitch = out_pitch;
    a.h = h; a.w = w;
    a.shutter = prm.shutter; a.max_radius = prm.max_radius; a.taps = prm.taps;
    launch_mblur_pack(a, 1, g_stream);
    launch_mblur_gather(a, 1, g_stream);
    HIPCHK(hipStreamSynchronize(g_stream));
    return finish();
}
// ---- rolling-shutter correction on caller planes (k_rshutter.hip; eppm_rolling_shutter_host is its host form): one frame ----
extern "C" int eppm_rolling_shutter_frames(void* d_rgba_out, size_t out_pitch, const void* d_rgba, size_t in_pitch, const eppm_float2* d_flow, int h, int w,
                                           int frame, const eppm_rs_params* params)
{
    eppm_rs_params prm;
    if (params) prm = *params;
    else (void)eppm_rs_default_params(&prm);
    if (!d_rgba_out || !d_rgba || !d_flow || h < 1 || w < 1 || (frame != 0 && frame != 1)) return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_frames: bad argument");
    if (!rs_params_ok(prm.readout, prm.anchor, prm.iters, prm.axis))
        return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_frames: readout %g (-1 .. 1), anchor %g (0 .. 1), iters %d (1 .. 8), axis %d (0, 1)", prm.readout, prm.anchor, prm.iters, prm.axis);
    if (bad_pitch(in_pitch, w) || bad_pitch(out_pitch, w))
        return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_frames: bad pitch %zu / %zu", in_pitch, out_pitch);
    if (h > 8192 || w > 8192 || (unsigned long long)h * (unsigned long long)w > (1ULL << 26))
        return set_err(EPPM_ERR_ARG, "eppm_rolling_shutter_frames: size %dx%d out of range", w, h);
    LAUNCHER_BEGIN_INT;
    RShutterArgs a{};
    a.plane = (size_t)h * w;
    void* scr = nullptr;
    CHK(get_scratch(ds, a.plane * 8, &scr, 6));          // the velocity plane
    a.img = (const uint8_t*)d_rgba; a.img_pitch = in_pitch;
    a.flow = (const float*)d_flow;
    a.vel = (float*)scr;
    a.rgba = (uint8_t*)d_rgba_out; a.rgba_pitch = out_pitch;
    a.h = h; a.w = w;
    a.readout = prm.readout; a.anchor = prm.anchor; a.iters = prm.iters; a.axis = prm.axis; a.frame = frame;
    launch_rs_velocity(a, 1, g_stream);
    launch_rs_gather(a, 1, g_stream);
    HIPCHK(hipStreamSynchronize(g_stream));
    return finish();
}
// ---- the caller-plane steps of the per-clip stage objects (eppm_*_step_frames, eppm_plate_render_frames: each in its object's module)
// reach the launcher stream through this ----
int launcher_run(const StageObject* o, const char* what, const std::function<int(hipStream_t)>& fn, bool sync)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int d = 0;
    HIPCHK(hipGetDevice(&d));
    if (d != o->device) return set_err(EPPM_ERR_ARG, "%s: the %s lives on device %d, the current device is %d", what, o->noun, o->device, d);
    CHK(fn(g_stream));
    if (sync) HIPCHK(hipStreamSynchronize(g_stream));
    return finish();
}
// the C++-linkage symbol the reference's driver declares at :64 (defaults 100,100 there; the live call passes 20,20)
void bao_cuda_convert_flow_to_colorshow(uchar4* rgbflow, float2* flow_vec, int h, int w, float max_disp_x, float max_disp_y)
{
    g_launch_status = eppm_flow_to_color((eppm_uchar4*)rgbflow, (const eppm_float2*)flow_vec, h, w, max_disp_x, max_disp_y);
}

extern "C" int eppm_launcher_status(void) { return g_launch_status; }

int launcher_finish() { return finish(); }
hipStream_t launcher_stream() { std::lock_guard<std::mutex> lk(g_mu); return g_stream; }
