// context.cpp -- eppm_ctx (context.h): create / destroy (init, _destroy: driver :112-157, :170-209), stream, level dimensions, planes, stage
// times, the colour-coded flow.  The only one of the context's files that reads a kernel-variant switch (api_internal.h: opt_*).
#include "context.h"

using namespace eppm;

extern "C" int eppm_destroy(eppm_ctx* c)
{
    if (!c) return EPPM_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->out_hold.release();
    clear_events(c, c->ev);
    clear_events(c, c->ev_prep);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    cache_free(c->slab, c->slab_bytes, false, c->device);
    if (c->h_color) (void)hipHostFree(c->h_color);
    for (int q = 0; q < 2; q++) {
        cache_free(c->h_rgb[q], c->h_rgb_bytes, true, c->device);
        if (c->ev_rgb[q]) (void)hipEventDestroy(c->ev_rgb[q]);
    }
    if (c->ev_h2d) (void)hipEventDestroy(c->ev_h2d);
    cache_free(c->d_yuv, c->d_yuv_bytes, false, c->device);
    for (int q = 0; q < 2; q++) cache_free(c->h_yuv[q], c->h_yuv_bytes, true, c->device);
    cache_free(c->h_flow, c->h_flow_bytes, true, c->device);
    cache_free(c->bwd, c->bwd_bytes, false, c->device);
    cache_free(c->h_bwd, c->h_bwd_bytes, true, c->device);
    cache_free(c->itp, c->itp_bytes, false, c->device);
    cache_free(c->h_itp, c->h_itp_bytes, true, c->device);
    cache_free(c->mbl, c->mbl_bytes, false, c->device);
    cache_free(c->h_mbl, c->h_mbl_bytes, true, c->device);
    cache_free(c->rsh, c->rsh_bytes, false, c->device);
    cache_free(c->h_rsh, c->h_rsh_bytes, true, c->device);
    cache_free(c->tmp, c->tmp_bytes, false, c->device);
    rng_free(c->rng);
    if (c->own_stream && c->stream) pooled_stream_destroy(c->stream, c->device);
    delete c;
    return EPPM_OK;
}

// The three look-up tables (a few hundred bytes, functions of the patch radius only) are uploaded once per (device, radius) and shared by
// every context: three hipMalloc + three synchronous copies + three hipFree per context were a millisecond of the create / destroy pair.
static int shared_luts(int device, int R, float** pm, float** wmf, float** blf)
{
    struct Entry { int device, R; float *pm, *wmf, *blf; };
    static std::mutex mu;
    static std::vector<Entry> tab;
    std::lock_guard<std::mutex> lk(mu);
    for (const Entry& e : tab)
        if (e.device == device && e.R == R) { *pm = e.pm; *wmf = e.wmf; *blf = e.blf; return EPPM_OK; }
    Entry e{device, R, nullptr, nullptr, nullptr};
    CHK(upload_pm_lut(&e.pm, R));
    CHK(upload_wmf_lut(&e.wmf));
    CHK(upload_blf_lut(&e.blf));
    tab.push_back(e);
    *pm = e.pm; *wmf = e.wmf; *blf = e.blf;
    return EPPM_OK;
}

// Lays the planes of ONE pair out in a slab (256-byte aligned offsets, pitched rows padded to 256 bytes), allocates
// npairs slabs in one block and points the context's members at pair 0's planes.
static int ctx_alloc(eppm_ctx* c)
{
    const int h = c->h, w = c->w;
    Carve cv;
    auto pitch_of = [](size_t row_bytes) { return (row_bytes + 255) & ~(size_t)255; };
    c->raw_pitch = pitch_of((size_t)w * 4);
    for (uint32_t** p : {&c->raw1, &c->raw2}) cv.plane(p, c->raw_pitch * h);
    for (int i = 0; i < c->nl; i++) {
        c->ipitch[i] = pitch_of((size_t)c->W[i] * 4);
        c->cpitch[i] = pitch_of((size_t)c->W[i]);
        const size_t n = (size_t)c->W[i] * c->H[i];
        for (uint32_t** p : {&c->img1[i], &c->img2[i], &c->tmpu[i]}) cv.plane(p, c->ipitch[i] * c->H[i]);
        for (void** p : {&c->pk1[i], &c->pk2[i]}) cv.plane(p, n * 16);
        for (uint32_t** p : {&c->pc1[i], &c->pc2[i]}) cv.plane(p, n * 4);      // (the refine levels' window kernels and the PatchMatch level's random search)
        for (uint8_t** p : {&c->cen1[i], &c->cen2[i]}) cv.plane(p, c->cpitch[i] * c->H[i]);
        for (float** p : {&c->flow[i], &c->flow_tmp[i]}) cv.plane(p, n * 8);
        if (i < c->nl - 1 && c2f_refine_wants_split(c->W[i], c->H[i], c->prm.patch_r, 1, c->opt_no_split != 0)) cv.plane(&c->c2f_cost9[i], n * 36 * 4);
    }
    const int L = c->nl - 1;
    const size_t n2 = (size_t)c->W[L] * c->H[L];
    // column-parity planes: the tolerance library reads them at both radii, the exact library at radius 9 (pm_device.cuh: pm_has_parity)
#ifndef EPPM_TOL
    if (c->prm.patch_r == 9)
#endif
    {
        c->pp_pad = (c->prm.patch_r + 2) & ~1;              // even and >= R + 1: a target column is in [0, w], a sample within R of it
        c->pp_pitch = parity_pitch(c->W[L], c->pp_pad);
        for (uint32_t** p : {&c->pp1, &c->pp2}) cv.plane(p, (size_t)2 * c->H[L] * c->pp_pitch * 4);
    }
    for (int16_t** p : {&c->nnf1, &c->nnf2, &c->nnf_tmp, &c->nnf_tmp2}) cv.plane(p, n2 * 4);
    for (float** p : {&c->cost1, &c->cost2}) cv.plane(p, n2 * 4);
    for (float** p : {&c->spec1, &c->spec2}) cv.plane(p, n2 * 4 * 4);
    // rest-weight planes of the two-phase search (PmProblem::restw): only where a launch of this context can take that form -- the decision
    // is monotone in the pairs per launch, so the full batch answers for every smaller one
    if (pm_search_pretest_form(c->W[L], c->H[L], c->prm.patch_r, 2, c->npairs))
        for (float** p : {&c->restw1, &c->restw2}) cv.plane(p, n2 * 4);
    for (int32_t** p : {&c->scand1, &c->scand2}) cv.plane(p, n2 * 4 * 4);
    for (uint32_t** p : {&c->wl1, &c->wl2}) cv.plane(p, pm_worklist_words(c->W[L], c->H[L], c->prm.seg_len) * 4);
    for (int16_t** p : {&c->seed1, &c->seed2}) cv.plane(p, n2 * 4 * 4);
    cv.plane(&c->wmf_ws, wmf_workspace_words(c->W[L], c->H[L], c->prm.wmf_iters) * 4);
    cv.plane(&c->d_rgb, (size_t)h * w * 3 * 2);
    cv.plane(&c->d_color, (size_t)h * w * 4);
    cv.plane(&c->d_uv, (size_t)h * w * 8);
    CHK(rng_create(&c->rng, c->W[L], c->H[L], c->prm, false));
    const size_t rng_bytes = (size_t)c->rng->gx * c->rng->gy * 64 * 6 * 4;
    for (int k = 0; k < 2; k++)
        for (int q = 0; q < 2; q++) cv.plane(&c->rng->work[k][q], rng_bytes);
    c->stride = (cv.off + 4095) & ~(size_t)4095;
    // every texel plane is addressed with 32-bit byte offsets from ITS OWN base; the slab stride itself is 64-bit
    CHK(cv.alloc(&c->slab, &c->slab_bytes, c->stride * c->npairs, c->device, (std::to_string(c->npairs) + " slab(s)").c_str()));
    CHK(shared_luts(c->device, c->prm.patch_r, &c->lut_pm, &c->lut_wmf, &c->lut_blf));
    c->out_u.assign(c->npairs, nullptr);
    c->out_v.assign(c->npairs, nullptr);
    for (auto* v : {&c->tmp_snap, &c->tmp_valid, &c->tmp_seeded, &c->tmp_cut}) v->assign(c->npairs, 0);
    return EPPM_OK;
}

extern "C" int eppm_create_batch(eppm_ctx** out, int h, int w, int device, const eppm_params* params, int npairs)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_create: NULL out");
    *out = nullptr;
    if (npairs < 1 || npairs > 4096) return set_err(EPPM_ERR_ARG, "eppm_create_batch: npairs %d out of range [1,4096]", npairs);
    if (h < 4 || w < 4 || h > 32767 || w > 32767) return set_err(EPPM_ERR_ARG, "eppm_create: size %dx%d out of range (NNF coordinates are int16)", w, h);
    if ((unsigned long long)h * (unsigned long long)w * 16ULL >= (1ULL << 32))
        return set_err(EPPM_ERR_ARG, "eppm_create: size %dx%d out of range (texel planes are addressed with 32-bit byte offsets)", w, h);
    eppm_params p;
    eppm_default_params(&p);
    if (params) p = *params;
    CHK(check_params(p));
    HIPCHK(hipSetDevice(device));
    eppm_ctx* c = new eppm_ctx();
    c->device = device; c->prm = p; c->h = h; c->w = w; c->npairs = npairs; c->n_active = 1;
    c->opt_sweep_spec = opt_sweep_spec(); c->opt_no_split = opt_no_split(); c->opt_search_pre = opt_search_pre(); c->opt_c2f_pre = opt_c2f_pre();
    c->nl = pyr_init_dim(c->H, c->W, h, w, p.levels, 0.5f);
    const int L = c->nl - 1;
    if (c->H[L] < 1 || c->W[L] < 1 || (c->W[L] + p.seg_len - 1) / p.seg_len > 1024 || (c->H[L] + p.seg_len - 1) / p.seg_len > 1024) {
        delete c;
        return set_err(EPPM_ERR_ARG, "eppm_create: unsupported size %dx%d", w, h);
    }
    const hipError_t e = pooled_stream_create(&c->stream, c->device);
    if (e != hipSuccess) { delete c; return set_err(EPPM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->own_stream = true;
    int r = ctx_alloc(c);
    if (r != EPPM_OK) { eppm_destroy(c); return r; }
    *out = c;
    return EPPM_OK;
}

extern "C" int eppm_create(eppm_ctx** out, int h, int w, int device, const eppm_params* params)
{
    return eppm_create_batch(out, h, w, device, params, 1);
}

extern "C" int eppm_batch_size(const eppm_ctx* c) { return c ? c->npairs : 0; }

extern "C" int eppm_set_stream(eppm_ctx* c, void* s)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); pooled_stream_destroy(c->stream, c->device); }
    c->stream = (hipStream_t)s;
    c->own_stream = false;
    return EPPM_OK;
}

extern "C" int eppm_num_levels(const eppm_ctx* c) { return c ? c->nl : 0; }
extern "C" int eppm_level_dims(const eppm_ctx* c, int level, int* h, int* w)
{
    if (!c || level < 0 || level >= c->nl) return set_err(EPPM_ERR_ARG, "bad level");
    if (h) *h = c->H[level];
    if (w) *w = c->W[level];
    return EPPM_OK;
}
extern "C" int eppm_enable_stage_timing(eppm_ctx* c, int on)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    c->timing = (on == 2) ? 2 : (on != 0);
    return EPPM_OK;
}

int ctx_device(const eppm_ctx* c, int* h, int* w)
{
    *h = c->h;
    *w = c->w;
    return c->device;
}

void ctx_stage_begin(eppm_ctx* c, const char* name) { stage_begin(c, c->ev, name); }
void ctx_stage_end(eppm_ctx* c) { stage_end(c, c->ev); }

extern "C" int eppm_synchronize(eppm_ctx* c)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    HIPCHK(hipStreamSynchronize(c->stream));
    return EPPM_OK;
}

extern "C" int eppm_stage_times(eppm_ctx* c, const char** names, float* ms, int max)
{
    if (!c) return 0;
    (void)hipStreamSynchronize(c->stream);
    int n = 0;
    for (auto* v : {&c->ev_prep, &c->ev})
        for (auto& e : *v) {
            if (n >= max) return n;
            float t = 0;
            if (hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) t = -1;
            names[n] = e.name; ms[n] = t; n++;
        }
    return n;
}

extern "C" int eppm_clear_stage_times(eppm_ctx* c)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    (void)hipStreamSynchronize(c->stream);
    clear_events(c, c->ev);
    clear_events(c, c->ev_prep);
    return EPPM_OK;
}

extern "C" int eppm_batch_get_plane(eppm_ctx* c, int pair, const char* name, int level, void* dst, size_t dst_bytes)
{
    if (!c || !name || !dst) return set_err(EPPM_ERR_ARG, "eppm_get_plane: NULL argument");
    if (level < 0 || level >= c->nl) return set_err(EPPM_ERR_ARG, "eppm_get_plane: bad level %d", level);
    if (pair < 0 || pair >= c->npairs) return set_err(EPPM_ERR_ARG, "eppm_get_plane: bad pair %d", pair);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int w = c->W[level], h = c->H[level], L = c->nl - 1;
    const void* src = nullptr;
    size_t esz = 0, pitch = 0, pstride = c->stride;
    std::string n(name);
    if (n == "img1" || n == "img2") { src = (n == "img1") ? c->img1[level] : c->img2[level]; esz = 4; pitch = c->ipitch[level]; }
    else if (n == "census1" || n == "census2") { src = (n == "census1") ? c->cen1[level] : c->cen2[level]; esz = 1; pitch = c->cpitch[level]; }
    else if (n == "flow") { src = c->flow[level]; esz = 8; pitch = (size_t)w * 8; }
    else if (level == L && (n == "nnf1" || n == "nnf2")) { src = (n == "nnf1") ? c->nnf1 : c->nnf2; esz = 4; pitch = (size_t)w * 4; }
    else if (level == L && (n == "cost1" || n == "cost2")) { src = (n == "cost1") ? c->cost1 : c->cost2; esz = 4; pitch = (size_t)w * 4; }
    else if (n == "flow_bwd" || (level == 0 && (n == "occ1" || n == "occ2"))) {
        if (!c->have_bwd) return set_err(EPPM_ERR_STATE, "eppm_get_plane: '%s' needs a bidirectional call first", name);
        if (n == "flow_bwd") { src = c->bflow[level]; esz = 8; }
        else { src = (n == "occ1") ? c->occ1 : c->occ2; esz = 1; }
        pitch = (size_t)w * esz;
        pstride = c->bwd_stride;
    }
    else if (level == L && (n == "prior1" || n == "prior2" || n == "nnf_init1" || n == "nnf_init2" || n == "cost_init1" || n == "cost_init2")) {
        if (!c->tmp_seeded[pair]) return set_err(EPPM_ERR_STATE, "eppm_get_plane: '%s' needs a compute that started from a temporal prior", name);
        src = n == "prior1" ? (void*)c->prior1 : n == "prior2" ? (void*)c->prior2 : n == "nnf_init1" ? (void*)c->nnf_init1 : n == "nnf_init2" ? (void*)c->nnf_init2
            : n == "cost_init1" ? (void*)c->cost_init1 : (void*)c->cost_init2;
        esz = 4; pitch = (size_t)w * 4;
        pstride = c->tmp_stride;
    }
    else return set_err(EPPM_ERR_ARG, "eppm_get_plane: unknown plane '%s' at level %d", name, level);
    if (dst_bytes < (size_t)w * h * esz) return set_err(EPPM_ERR_ARG, "eppm_get_plane: dst too small");
    HIPCHK(hipMemcpy2D(dst, (size_t)w * esz, (const char*)src + (size_t)pair * pstride, pitch, (size_t)w * esz, h, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_get_plane(eppm_ctx* c, const char* name, int level, void* dst, size_t dst_bytes)
{
    return eppm_batch_get_plane(c, 0, name, level, dst, dst_bytes);
}

extern "C" int eppm_compute_color(eppm_ctx* c, uint8_t* rgb, size_t row_stride, float max_disp_x, float max_disp_y)
{
    if (!c || !rgb) return set_err(EPPM_ERR_ARG, "eppm_compute_color: NULL argument");
    if (!c->have_flow) return set_err(EPPM_ERR_STATE, "eppm_compute_color: no flow computed yet");
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_compute_color: row_stride %zu < 3*w", row_stride);
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->h * c->w;
    if (!c->h_color) HIPCHK(hipHostMalloc((void**)&c->h_color, n * 4, hipHostMallocDefault));
    launch_flow_to_color(c->d_color, c->flow[0], c->h, c->w, max_disp_x, max_disp_y, c->stream);       // driver :311
    HIPCHK(hipMemcpyAsync(c->h_color, c->d_color, n * 4, hipMemcpyDeviceToHost, c->stream));           // driver :312
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int y = 0; y < c->h; y++)                                                                         // bao_rgba2rgb, driver :313
        for (int x = 0; x < c->w; x++) {
            const uint32_t p = c->h_color[(size_t)y * c->w + x];
            uint8_t* o = rgb + (size_t)y * row_stride + (size_t)x * 3;
            o[0] = (uint8_t)(p & 0xff); o[1] = (uint8_t)((p >> 8) & 0xff); o[2] = (uint8_t)((p >> 16) & 0xff);
        }
    return EPPM_OK;
}

#ifdef EPPM_TEST_HOOKS
// test library (include/eppm_test.h): the column-parity planes of a context's PatchMatch level and which kernels read them
extern "C" int eppm_probe_pm_parity(const eppm_ctx* c, int* pitch, int* pad, int* kernels)
{
    if (!c || !pitch || !pad || !kernels) return set_err(EPPM_ERR_ARG, "eppm_probe_pm_parity: NULL argument");
    *pitch = c->pp1 ? c->pp_pitch : 0;
    *pad = c->pp1 ? c->pp_pad : 0;
    *kernels = c->pp1 ? pm_parity_kernels(c->prm.patch_r) : 0;
    return EPPM_OK;
}
// the per-block XORWOW states of a context's PatchMatch generator where its last run left them (as eppm_pm_rng_block_states)
extern "C" int eppm_probe_ctx_rng_states(eppm_ctx* c, uint32_t* dst, size_t dst_words)
{
    if (!c || !dst) return set_err(EPPM_ERR_ARG, "eppm_probe_ctx_rng_states: NULL argument");
    const int nb = c->rng->gx * c->rng->gy;
    if (dst_words < (size_t)nb * 6) return set_err(EPPM_ERR_ARG, "eppm_probe_ctx_rng_states: dst too small");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy2D(dst, 24, c->rng->work[0][c->rng->cur[0]], 64 * 24, 24, nb, hipMemcpyDeviceToHost));
    return EPPM_OK;
}
#endif
