// context.cpp -- eppm_ctx, the object behind class bao_flow_patchmatch_multiscale_cuda: create / destroy (init, _destroy: driver
// :112-157, :170-209), set_images (set_data :159-168 + _prepare_data :212-215), compute (compute_flow :217-306), planes, stage times.
#include "api_internal.h"
#include "interp.h"
#include "temporal.h"

using namespace eppm;

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------

struct StageEv { const char* name; hipEvent_t a, b; };

// One context = a batch of `npairs` independent pairs of one size (1 for the plain eppm_create).  Every device plane of
// pair k lives at the same offset inside pair k's SLAB and the slabs are `stride` bytes apart in one allocation, so every
// launch covers all active pairs: it gets pair 0's pointers and {n_active, stride} (eppm_internal.h: Batch), and
// blockIdx.z / .y selects the pair.  The pointer members below are pair 0's; ping-pong swaps apply to every pair alike.
struct eppm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int opt_sweep_spec = -1, opt_no_split = 0;     // kernel-variant switches, copied from the process defaults at creation (test support)
    eppm_params prm;
    int h = 0, w = 0, nl = 0;
    int npairs = 1, n_active = 1;
    char* slab = nullptr;
    size_t stride = 0;
    int H[kMaxLevels], W[kMaxLevels];
    size_t ipitch[kMaxLevels], cpitch[kMaxLevels];   // bytes
    uint32_t *raw1 = nullptr, *raw2 = nullptr;
    size_t raw_pitch = 0;
    uint32_t *img1[kMaxLevels] = {}, *img2[kMaxLevels] = {}, *tmpu[kMaxLevels] = {};
    uint8_t *cen1[kMaxLevels] = {}, *cen2[kMaxLevels] = {};
    void *pk1[kMaxLevels] = {}, *pk2[kMaxLevels] = {};       // float4 texel planes {r,g,b,census}, linear (pitch = w)
    uint32_t *pc1[kMaxLevels] = {}, *pc2[kMaxLevels] = {};   // the same texels in 4 bytes, at the levels the LDS-window refine runs on
    uint32_t *pp1 = nullptr, *pp2 = nullptr;                 // column-parity planes of pc at the PatchMatch level (PlanesH::pp1)
    int pp_pitch = 0, pp_pad = 0;
    int16_t *nnf1 = nullptr, *nnf2 = nullptr, *nnf_tmp = nullptr, *nnf_tmp2 = nullptr;
    float *cost1 = nullptr, *cost2 = nullptr;
    float *spec1 = nullptr, *spec2 = nullptr;   // evaluation cache of the sweeps (PmProblem::spec / scand): four direction planes each
    int32_t *scand1 = nullptr, *scand2 = nullptr;
    uint32_t *wl1 = nullptr, *wl2 = nullptr;    // work lists of the speculative sweeps (PmProblem::wl)
    int16_t *seed1 = nullptr, *seed2 = nullptr; // merged form: the field before each direction's sweep (PmProblem::seed), four planes each
    uint32_t* wmf_ws = nullptr;        // work lists + counters of the weighted median
    bool flow_pending = false;         // eppm_compute_begin issued, eppm_compute_end not yet
    float *flow[kMaxLevels] = {}, *flow_tmp[kMaxLevels] = {};
    float* c2f_cost9[kMaxLevels] = {};  // 9 candidates x 4 passes costs per pixel, only for levels whose refine launch is split
    float *lut_pm = nullptr, *lut_wmf = nullptr, *lut_blf = nullptr;
    eppm_pm_rng* rng = nullptr;
    float* d_uv = nullptr;              // planar u | v of the final flow (host-pointer boundary), in the slab
    uint32_t* d_color = nullptr;        // colour-coded flow (optional output), in the slab
    uint32_t* h_color = nullptr;        // pinned, allocated on first use
    uint8_t* d_rgb = nullptr;           // staging for host RGB input (both frames), in the slab
    // pinned staging for images / flows in memory the caller did NOT register (eppm_host_register), allocated on the first such
    // call; the image staging is double-buffered (an event per buffer marks its H2D done), so staging pair i+1 never waits for
    // the stream to drain
    size_t slab_bytes = 0, h_rgb_bytes = 0, h_flow_bytes = 0;      // sizes of the cacheable blocks (cache_alloc / cache_free)
    uint8_t* h_rgb[2] = {nullptr, nullptr};   // each npairs x both frames
    hipEvent_t ev_rgb[2] = {nullptr, nullptr};
    hipEvent_t ev_h2d = nullptr;        // marks the DMA reads of registered caller images
    int rgb_cur = 0;
    float* h_flow = nullptr;            // npairs x (u plane | v plane)
    std::vector<float*> out_u, out_v;   // per active pair: where eppm_compute_begin_into sent the planes directly (NULL: staging)
    HostHold out_hold;                  // the registered blocks those planes lie in, in use until eppm_compute_end
    bool have_images = false, have_flow = false;
    // Bidirectional calls (eppm_compute_bidirectional*): their own allocation, made by the first such call -- a forward-only context never
    // has it.  npairs blocks bwd_stride bytes apart, each: the backward flow pyramid, then the host boundary's planar bu | bv (h*w*8 bytes)
    // followed by occ1 and occ2 (h*w bytes each).  The backward path itself runs in slab planes the forward path has finished with
    // (flow_tmp, d_uv, nnf2 / nnf_tmp2, wmf_ws, c2f_cost9); each level's result is copied into bflow.
    char* bwd = nullptr;
    size_t bwd_stride = 0, bwd_bytes = 0, h_bwd_bytes = 0;
    float* bflow[kMaxLevels] = {};
    float* d_buv = nullptr;
    uint8_t *occ1 = nullptr, *occ2 = nullptr;
    uint8_t* h_bwd = nullptr;           // pinned, npairs x (bu | bv | occ1 | occ2), allocated on the first host-boundary bidirectional call
    float occ_alpha = 0.01f, occ_beta = 0.5f;
    bool have_bwd = false;              // the planes above hold the last call's results
    bool bwd_images = false;            // ... and the raw images they were computed from are still the context's (no set_images since)
    // Frame interpolation (eppm_interpolate*): its own allocation, made by the first such call, for npairs x
    // kInterpChunk slots: the splat keys, the two fill planes (itp_plane elements per slot each) and the packed RGB outputs of the
    // host-pointer forms (h*w*3 bytes per slot); h_itp: pinned copy of those outputs, allocated on the first host-pointer call.
    char* itp = nullptr;
    size_t itp_bytes = 0, itp_plane = 0, h_itp_bytes = 0;
    uint64_t* itp_keys = nullptr;
    int32_t *itp_fill1 = nullptr, *itp_fill2 = nullptr;
    uint8_t* itp_rgb = nullptr;
    uint8_t* h_itp = nullptr;
    // Streaming mode (eppm_set_temporal; single-pair contexts only): its own allocation, made by the first compute
    // with the mode on.  Level-L planes, unpitched: the two displacement snapshots of the last compute (prev_fwd: the field nnf2flow
    // converted, prev_bwd: the raw backward NNF), the two advected priors, the seeded start as the select kernel left it, and the landing
    // keys of both directions (kTemporalNoKey between launches).
    bool temporal = false;
    bool tmp_snap = false;              // the snapshots hold the last compute's pair, and no frame has been pushed since
    bool tmp_valid = false;             // armed by a push that found such snapshots: the next compute starts from their prior
    bool tmp_seeded = false;            // the last compute started from a prior: prior*, nnf_init*, cost_init* are its planes
    char* tmp = nullptr;
    size_t tmp_bytes = 0;
    int16_t *prev_fwd = nullptr, *prev_bwd = nullptr, *prior1 = nullptr, *prior2 = nullptr, *nnf_init1 = nullptr, *nnf_init2 = nullptr;
    float *cost_init1 = nullptr, *cost_init2 = nullptr;
    int32_t* tmp_keys = nullptr;        // 2 x W[L]*H[L]
    int timing = 0;                     // 0 off, 1 every stage, 2 only the dominant kernel (the candidate refine)
    std::vector<StageEv> ev;
    std::vector<StageEv> ev_prep;
    std::vector<hipEvent_t> ev_pool;    // events are created once and reused: no hipEventCreate in a steady-state step
    Batch bt() const { return Batch{n_active, stride}; }
    template <class T> T* of_pair(T* p, int k) const { return (T*)((char*)p + (size_t)k * stride); }
};

static PlanesH planes(const eppm_ctx* c, int l, bool swap)
{
    PlanesH p;
    p.pk1 = swap ? c->pk2[l] : c->pk1[l];
    p.pk2 = swap ? c->pk1[l] : c->pk2[l];
    p.w = c->W[l]; p.h = c->H[l];
    p.pitch = c->W[l];
    p.pc1 = swap ? c->pc2[l] : c->pc1[l];
    p.pc2 = swap ? c->pc1[l] : c->pc2[l];
    if (l == c->nl - 1 && c->pp1) {
        p.pp1 = swap ? c->pp2 : c->pp1;
        p.pp2 = swap ? c->pp1 : c->pp2;
        p.pp_pitch = c->pp_pitch; p.pp_pad = c->pp_pad;
    }
    return p;
}

static hipEvent_t pool_event(eppm_ctx* c)
{
    hipEvent_t e = nullptr;
    if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
}
static bool stage_on(const eppm_ctx* c, bool dominant) { return c->timing == 1 || (c->timing == 2 && dominant); }
static void stage_begin(eppm_ctx* c, std::vector<StageEv>& v, const char* name, bool dominant = false)
{
    if (!stage_on(c, dominant)) return;
    StageEv e;
    e.name = name;
    e.a = pool_event(c);
    e.b = pool_event(c);
    (void)hipEventRecord(e.a, c->stream);
    v.push_back(e);
}
static void stage_end(eppm_ctx* c, std::vector<StageEv>& v, bool dominant = false)
{
    if (!stage_on(c, dominant)) return;
    (void)hipEventRecord(v.back().b, c->stream);
}
// closes entry `idx` (stages opened after it have been closed: a stage inside a stage)
static void stage_end_at(eppm_ctx* c, std::vector<StageEv>& v, size_t idx)
{
    if (!stage_on(c, false)) return;
    (void)hipEventRecord(v[idx].b, c->stream);
}
static void clear_events(eppm_ctx* c, std::vector<StageEv>& v)
{
    for (auto& e : v) { c->ev_pool.push_back(e.a); c->ev_pool.push_back(e.b); }
    v.clear();
}

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
    cache_free(c->h_flow, c->h_flow_bytes, true, c->device);
    cache_free(c->bwd, c->bwd_bytes, false, c->device);
    cache_free(c->h_bwd, c->h_bwd_bytes, true, c->device);
    cache_free(c->itp, c->itp_bytes, false, c->device);
    cache_free(c->h_itp, c->h_itp_bytes, true, c->device);
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
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    auto pitch_of = [](size_t row_bytes) { return (row_bytes + 255) & ~(size_t)255; };
    struct Fix { void** dst; size_t off; };
    std::vector<Fix> fix;
    auto plane = [&](void** dst, size_t bytes) { fix.push_back(Fix{dst, take(bytes)}); };
    c->raw_pitch = pitch_of((size_t)w * 4);
    plane((void**)&c->raw1, c->raw_pitch * h);
    plane((void**)&c->raw2, c->raw_pitch * h);
    for (int i = 0; i < c->nl; i++) {
        c->ipitch[i] = pitch_of((size_t)c->W[i] * 4);
        c->cpitch[i] = pitch_of((size_t)c->W[i]);
        const size_t n = (size_t)c->W[i] * c->H[i];
        plane((void**)&c->img1[i], c->ipitch[i] * c->H[i]);
        plane((void**)&c->img2[i], c->ipitch[i] * c->H[i]);
        plane((void**)&c->tmpu[i], c->ipitch[i] * c->H[i]);
        plane(&c->pk1[i], n * 16);
        plane(&c->pk2[i], n * 16);
        plane((void**)&c->pc1[i], n * 4);      // (the refine levels' window kernels and the PatchMatch level's random search)
        plane((void**)&c->pc2[i], n * 4);
        plane((void**)&c->cen1[i], c->cpitch[i] * c->H[i]);
        plane((void**)&c->cen2[i], c->cpitch[i] * c->H[i]);
        plane((void**)&c->flow[i], n * 8);
        plane((void**)&c->flow_tmp[i], n * 8);
        if (i < c->nl - 1 && c2f_refine_wants_split(c->W[i], c->H[i], c->prm.patch_r, 1, c->opt_no_split != 0)) plane((void**)&c->c2f_cost9[i], n * 36 * 4);
    }
    const int L = c->nl - 1;
    const size_t n2 = (size_t)c->W[L] * c->H[L];
    // column-parity planes: the tolerance library reads them at both radii, the exact library at radius 9 (k_patchmatch.hip: pm_has_parity)
#ifndef EPPM_TOL
    if (c->prm.patch_r == 9)
#endif
    {
        c->pp_pad = (c->prm.patch_r + 2) & ~1;              // even and >= R + 1: a target column is in [0, w], a sample within R of it
        c->pp_pitch = parity_pitch(c->W[L], c->pp_pad);
        plane((void**)&c->pp1, (size_t)2 * c->H[L] * c->pp_pitch * 4);
        plane((void**)&c->pp2, (size_t)2 * c->H[L] * c->pp_pitch * 4);
    }
    plane((void**)&c->nnf1, n2 * 4);
    plane((void**)&c->nnf2, n2 * 4);
    plane((void**)&c->nnf_tmp, n2 * 4);
    plane((void**)&c->nnf_tmp2, n2 * 4);
    plane((void**)&c->cost1, n2 * 4);
    plane((void**)&c->cost2, n2 * 4);
    plane((void**)&c->spec1, n2 * 4 * 4);
    plane((void**)&c->spec2, n2 * 4 * 4);
    plane((void**)&c->scand1, n2 * 4 * 4);
    plane((void**)&c->scand2, n2 * 4 * 4);
    plane((void**)&c->wl1, pm_worklist_words(c->W[L], c->H[L], c->prm.seg_len) * 4);
    plane((void**)&c->wl2, pm_worklist_words(c->W[L], c->H[L], c->prm.seg_len) * 4);
    plane((void**)&c->seed1, n2 * 4 * 4);
    plane((void**)&c->seed2, n2 * 4 * 4);
    plane((void**)&c->wmf_ws, wmf_workspace_words(c->W[L], c->H[L], c->prm.wmf_iters) * 4);
    plane((void**)&c->d_rgb, (size_t)h * w * 3 * 2);
    plane((void**)&c->d_color, (size_t)h * w * 4);
    plane((void**)&c->d_uv, (size_t)h * w * 8);
    CHK(rng_create(&c->rng, c->W[L], c->H[L], c->prm, false));
    const size_t rng_bytes = (size_t)c->rng->gx * c->rng->gy * 64 * 6 * 4;
    for (int k = 0; k < 2; k++)
        for (int q = 0; q < 2; q++) plane((void**)&c->rng->work[k][q], rng_bytes);
    c->stride = (off + 4095) & ~(size_t)4095;
    // every texel plane is addressed with 32-bit byte offsets from ITS OWN base; the slab stride itself is 64-bit
    c->slab_bytes = c->stride * c->npairs;
    {
        const hipError_t e = cache_alloc((void**)&c->slab, c->slab_bytes, false, c->device);
        if (e != hipSuccess) { (void)hipGetLastError(); return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (%d slab(s)) failed: %s", c->slab_bytes, c->npairs, hipGetErrorString(e)); }
    }
    for (const Fix& f : fix) *f.dst = c->slab + f.off;
    CHK(shared_luts(c->device, c->prm.patch_r, &c->lut_pm, &c->lut_wmf, &c->lut_blf));
    c->out_u.assign(c->npairs, nullptr);
    c->out_v.assign(c->npairs, nullptr);
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
    c->opt_sweep_spec = opt_sweep_spec(); c->opt_no_split = opt_no_split();
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

// ---- prepare: refine :1060-1071 + .cuh:642-664.  The two frames of every active pair share every launch; the raw
// RGBA planes of the active pairs are in the slabs already.  only2: image 2 alone (eppm_push_image: image 1's planes are the previous
// pair's image-2 planes); every kernel is per pixel of one image, so its planes equal those of a launch that covers both images. ----
static int prepare(eppm_ctx* c, bool only2 = false)
{
    stage_begin(c, c->ev_prep, "prepare");
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    uint32_t **p1 = c->img1, **p2 = c->img2, **tmp = c->tmpu;
    const int p0 = (int)(c->ipitch[0] / 4);
    if (only2) launch_gauss_rgba(p2[0], c->raw2, p0, c->H[0], c->W[0], .5f, 2, s, bt);
    else launch_gauss_rgba2(p1[0], c->raw1, p2[0], c->raw2, p0, c->H[0], c->W[0], .5f, 2, s, bt);    // refine :1063-1064
    const float ratio = 0.5f;                                                             // PYR_RATIO
    const float baseSigma = (1 / ratio - 1);
    const int n = (int)(log(0.25) / (double)logf(ratio));   // C++ float overload in the reference: n = 1
    const float nSigma = baseSigma * n;
    for (int i = 1; i < c->nl; i++) {
        // source level j, blur (sigma, radius), resize ratio r: .cuh:647-663
        const int j = (i <= n) ? 0 : i - n;
        const float sigma = (i <= n) ? baseSigma * i : nSigma;
        const float r = (i <= n) ? (float)pow(ratio, i) : (float)pow(ratio, i) * c->W[0] / c->W[j];
        const int radius = (int)(sigma * 3);
        const int pj = (int)(c->ipitch[j] / 4), pi = (int)(c->ipitch[i] / 4);
        if (gauss_decimate2_ok(c->H[i], c->W[i], c->H[j], c->W[j], r, radius)) {
            // exact 2:1 step: blur only the pixels the decimation keeps (a quarter of the level)
            if (only2) launch_gauss_decimate2(p2[i], p2[j], p2[i], p2[j], 1, pi, c->H[i], c->W[i], pj, c->H[j], c->W[j], sigma, radius, s, bt);
            else launch_gauss_decimate2(p1[i], p1[j], p2[i], p2[j], 2, pi, c->H[i], c->W[i], pj, c->H[j], c->W[j], sigma, radius, s, bt);
        } else {
            for (int k = only2 ? 1 : 0; k < 2; k++) {
                uint32_t** pyr = k ? p2 : p1;
                launch_gauss_rgba(tmp[j], pyr[j], pj, c->H[j], c->W[j], sigma, radius, s, bt);
                launch_resize_rgba(pyr[i], pi, c->H[i], c->W[i], tmp[j], pj, c->H[j], c->W[j], r, s, bt);
            }
        }
    }
    CensusBatch cb;
    cb.n = 0;
    for (int k = only2 ? 1 : 0; k < 2; k++)
        for (int i = 0; i < c->nl; i++) {
            CensusJob& J = cb.job[cb.n++];
            J.census = k ? c->cen2[i] : c->cen1[i]; J.cpitch = (int)c->cpitch[i];
            J.texels = k ? c->pk2[i] : c->pk1[i];   J.tpitch = c->W[i];
            J.img = k ? c->img2[i] : c->img1[i];    J.ipitch = (int)(c->ipitch[i] / 4);
            J.w = c->W[i]; J.h = c->H[i]; J.first_block = 0;
            J.packed = k ? c->pc2[i] : c->pc1[i];
        }
    launch_census_batch(cb, s, bt);
    if (c->pp1) {
        const int L = c->nl - 1;
        if (!only2) launch_parity_planes(c->pp1, c->pp_pitch, c->pp_pad, c->pc1[L], c->W[L], c->W[L], c->H[L], s, bt);
        launch_parity_planes(c->pp2, c->pp_pitch, c->pp_pad, c->pc2[L], c->W[L], c->W[L], c->H[L], s, bt);
    }
    stage_end(c, c->ev_prep);
    HIPCHK(hipGetLastError());
    c->have_images = true;
    c->have_flow = false;
    c->bwd_images = false;
    return EPPM_OK;
}

// host RGB of pairs 0..n-1 -> H2D -> RGBA planes (bao_rgb2rgba, alpha = 0) -> prepare.  An image inside memory registered with
// eppm_host_register / eppm_host_alloc is read by the copy engine where it lies; any other image goes through the context's pinned
// staging (one host copy), which is double-buffered.
static int set_images_host_impl(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride, HostHold& hold)
{
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_set_images: row_stride %zu < 3*w", row_stride);
    HIPCHK(hipSetDevice(c->device));
    const size_t row = (size_t)c->w * 3, img = row * c->h, span = row_stride * (c->h - 1) + row;
    for (int k = 0; k < n; k++)
        if (!rgb1[k] || !rgb2[k]) return set_err(EPPM_ERR_ARG, "eppm_set_images: NULL image");
    uint8_t* stage = nullptr;
    bool staged = false, direct = false;
    // (`hold`: registered blocks read in place stay in use until their DMA has completed -- the end of the call)
    for (int k = 0; k < n; k++)
        for (int f = 0; f < 2; f++) {
            const uint8_t* src = f ? rgb2[k] : rgb1[k];
            uint8_t* dst = c->of_pair(c->d_rgb, k) + (size_t)f * img;
            if (hold.add(src, span)) {
                if (row_stride == row) HIPCHK(hipMemcpyAsync(dst, src, img, hipMemcpyHostToDevice, c->stream));
                else HIPCHK(hipMemcpy2DAsync(dst, row, src, row_stride, row, c->h, hipMemcpyHostToDevice, c->stream));
                direct = true;
                continue;
            }
            if (!stage) {
                const int q = c->rgb_cur;
                if (!c->h_rgb[q]) {
                    c->h_rgb_bytes = img * 2 * c->npairs;
                    HIPCHK(cache_alloc((void**)&c->h_rgb[q], c->h_rgb_bytes, true, c->device));
                    HIPCHK(hipEventCreateWithFlags(&c->ev_rgb[q], hipEventDisableTiming));
                } else {
                    HIPCHK(hipEventSynchronize(c->ev_rgb[q]));      // the H2D that last read this buffer (two set_images ago)
                }
                stage = c->h_rgb[q];
            }
            uint8_t* h = stage + ((size_t)k * 2 + f) * img;
            if (row_stride == row) memcpy(h, src, img);
            else
                for (int y = 0; y < c->h; y++) memcpy(h + (size_t)y * row, src + (size_t)y * row_stride, row);
            HIPCHK(hipMemcpyAsync(dst, h, img, hipMemcpyHostToDevice, c->stream));
            staged = true;
        }
    if (staged) {
        HIPCHK(hipEventRecord(c->ev_rgb[c->rgb_cur], c->stream));
        c->rgb_cur ^= 1;
    }
    if (direct) {
        if (!c->ev_h2d) HIPCHK(hipEventCreateWithFlags(&c->ev_h2d, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_h2d, c->stream));
    }
    c->n_active = n;
    c->tmp_valid = c->tmp_snap = false; // a new pair is a new clip
    const int p0 = (int)(c->raw_pitch / 4);
    launch_rgb_to_rgba(c->raw1, p0, c->d_rgb, c->h, c->w, c->stream, c->bt());
    launch_rgb_to_rgba(c->raw2, p0, c->d_rgb + img, c->h, c->w, c->stream, c->bt());
    const int r = prepare(c);
    // set_data's contract (a synchronous cudaMemcpy in the reference, driver :165-166): when the call returns the caller may reuse
    // its images.  Staged images were copied above; for images read in place, wait for their DMA (the kernels are queued already).
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}
static int set_images_host(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride)
{
    HostHold hold;
    const int r = set_images_host_impl(c, n, rgb1, rgb2, row_stride, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);     // nothing may still read the blocks when `hold` lets them go
    return r;
}

extern "C" int eppm_set_images(eppm_ctx* c, const uint8_t* rgb1, const uint8_t* rgb2, size_t row_stride)
{
    if (!c || !rgb1 || !rgb2) return set_err(EPPM_ERR_ARG, "eppm_set_images: NULL argument");
    return set_images_host(c, 1, &rgb1, &rgb2, row_stride);
}

extern "C" int eppm_batch_set_images(eppm_ctx* c, int n, const uint8_t* const* rgb1, const uint8_t* const* rgb2, size_t row_stride)
{
    if (!c || !rgb1 || !rgb2) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images: %d pairs, context holds %d", n, c->npairs);
    return set_images_host(c, n, rgb1, rgb2, row_stride);
}

// device-resident RGBA of pairs 0..n-1: copied into the slabs' raw planes in stream order (the caller's planes are not
// read after the copies complete, and never in place), then prepare
static int set_images_device(eppm_ctx* c, int n, const void* const* d1, const void* const* d2, size_t pitch)
{
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    for (int k = 0; k < n; k++) {
        if (!d1[k] || !d2[k]) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: NULL image");
        HIPCHK(hipMemcpy2DAsync(c->of_pair(c->raw1, k), c->raw_pitch, d1[k], pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpy2DAsync(c->of_pair(c->raw2, k), c->raw_pitch, d2[k], pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
    }
    c->n_active = n;
    c->tmp_valid = c->tmp_snap = false;
    return prepare(c);
}

extern "C" int eppm_set_images_device(eppm_ctx* c, const void* d1, const void* d2, size_t pitch)
{
    if (!c || !d1 || !d2) return set_err(EPPM_ERR_ARG, "eppm_set_images_device: NULL argument");
    return set_images_device(c, 1, &d1, &d2, pitch);
}

extern "C" int eppm_batch_set_images_device(eppm_ctx* c, int n, const void* const* d_rgba1, const void* const* d_rgba2, size_t pitch)
{
    if (!c || !d_rgba1 || !d_rgba2) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images_device: NULL argument");
    if (n < 1 || n > c->npairs) return set_err(EPPM_ERR_ARG, "eppm_batch_set_images_device: %d pairs, context holds %d", n, c->npairs);
    return set_images_device(c, n, d_rgba1, d_rgba2, pitch);
}

// ---- frame push: image 2 becomes image 1 by exchanging the context's plane pointers -- the raw frame, every
// pyramid level, census plane and texel plane of the old image 2 are kept --, the new frame becomes image 2 and is prepared alone ----
static int push_check(eppm_ctx* c, const char* what)
{
    if (c->npairs != 1) return set_err(EPPM_ERR_ARG, "%s: a batch context has no previous pair (its pairs run concurrently)", what);
    if (!c->have_images) return set_err(EPPM_ERR_STATE, "%s: no pair set yet (eppm_set_images first)", what);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    return EPPM_OK;
}
// also arms the temporal prior: the snapshots describe the pair that ends in the new image 1 only directly after that pair's compute
static void push_swap(eppm_ctx* c)
{
    c->tmp_valid = c->temporal && c->tmp_snap;
    c->tmp_snap = false;
    std::swap(c->raw1, c->raw2);
    for (int l = 0; l < c->nl; l++) {
        std::swap(c->img1[l], c->img2[l]);
        std::swap(c->cen1[l], c->cen2[l]);
        std::swap(c->pk1[l], c->pk2[l]);
        std::swap(c->pc1[l], c->pc2[l]);
    }
    std::swap(c->pp1, c->pp2);
}

static int push_image_host_impl(eppm_ctx* c, const uint8_t* rgb, size_t row_stride, HostHold& hold)
{
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "eppm_push_image: row_stride %zu < 3*w", row_stride);
    HIPCHK(hipSetDevice(c->device));
    const size_t row = (size_t)c->w * 3, img = row * c->h, span = row_stride * (c->h - 1) + row;
    uint8_t* dst = c->d_rgb + img;                       // image 2's half of the RGB staging plane
    bool direct = false;
    if (hold.add(rgb, span)) {
        if (row_stride == row) HIPCHK(hipMemcpyAsync(dst, rgb, img, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(hipMemcpy2DAsync(dst, row, rgb, row_stride, row, c->h, hipMemcpyHostToDevice, c->stream));
        direct = true;
    } else {
        const int q = c->rgb_cur;
        if (!c->h_rgb[q]) {
            c->h_rgb_bytes = img * 2 * c->npairs;
            HIPCHK(cache_alloc((void**)&c->h_rgb[q], c->h_rgb_bytes, true, c->device));
            HIPCHK(hipEventCreateWithFlags(&c->ev_rgb[q], hipEventDisableTiming));
        } else {
            HIPCHK(hipEventSynchronize(c->ev_rgb[q]));
        }
        uint8_t* h = c->h_rgb[q] + img;
        if (row_stride == row) memcpy(h, rgb, img);
        else
            for (int y = 0; y < c->h; y++) memcpy(h + (size_t)y * row, rgb + (size_t)y * row_stride, row);
        HIPCHK(hipMemcpyAsync(dst, h, img, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->ev_rgb[q], c->stream));
        c->rgb_cur ^= 1;
    }
    if (direct) {
        if (!c->ev_h2d) HIPCHK(hipEventCreateWithFlags(&c->ev_h2d, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_h2d, c->stream));
    }
    push_swap(c);
    launch_rgb_to_rgba(c->raw2, (int)(c->raw_pitch / 4), dst, c->h, c->w, c->stream, c->bt());
    const int r = prepare(c, true);
    if (direct) HIPCHK(hipEventSynchronize(c->ev_h2d));
    return r;
}

extern "C" int eppm_push_image(eppm_ctx* c, const uint8_t* rgb, size_t row_stride)
{
    if (!c || !rgb) return set_err(EPPM_ERR_ARG, "eppm_push_image: NULL argument");
    CHK(push_check(c, "eppm_push_image"));
    HostHold hold;
    const int r = push_image_host_impl(c, rgb, row_stride, hold);
    if (r != EPPM_OK && !hold.v.empty()) (void)hipStreamSynchronize(c->stream);
    return r;
}

extern "C" int eppm_push_image_device(eppm_ctx* c, const void* d_rgba, size_t pitch)
{
    if (!c || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_push_image_device: NULL argument");
    CHK(push_check(c, "eppm_push_image_device"));
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_push_image_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    // into the old image 1's raw plane, which the swap then makes image 2's: a copy that fails leaves the context on its old pair
    HIPCHK(hipMemcpy2DAsync(c->raw1, c->raw_pitch, d_rgba, pitch, (size_t)c->w * 4, c->h, hipMemcpyDeviceToDevice, c->stream));
    push_swap(c);
    return prepare(c, true);
}

// ---- temporal mode ----
static int tmp_alloc(eppm_ctx* c)
{
    if (c->tmp) return EPPM_OK;
    const int L = c->nl - 1;
    const size_t n2 = (size_t)c->W[L] * c->H[L];
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    size_t o[9];
    for (int k = 0; k < 8; k++) o[k] = take(n2 * 4);       // six short2 planes, two float planes
    o[8] = take(n2 * 4 * 2);                               // the keys of both directions
    const hipError_t e = cache_alloc((void**)&c->tmp, off, false, c->device);
    if (e != hipSuccess) { (void)hipGetLastError(); c->tmp = nullptr; return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (temporal planes) failed: %s", off, hipGetErrorString(e)); }
    c->tmp_bytes = off;
    c->prev_fwd = (int16_t*)(c->tmp + o[0]); c->prev_bwd = (int16_t*)(c->tmp + o[1]);
    c->prior1 = (int16_t*)(c->tmp + o[2]);   c->prior2 = (int16_t*)(c->tmp + o[3]);
    c->nnf_init1 = (int16_t*)(c->tmp + o[4]); c->nnf_init2 = (int16_t*)(c->tmp + o[5]);
    c->cost_init1 = (float*)(c->tmp + o[6]);  c->cost_init2 = (float*)(c->tmp + o[7]);
    c->tmp_keys = (int32_t*)(c->tmp + o[8]);
    launch_temporal_keys_init(c->tmp_keys, (int)(2 * n2), c->stream);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

extern "C" int eppm_set_temporal(eppm_ctx* c, int on)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_set_temporal: NULL ctx");
    if (on && c->npairs != 1) return set_err(EPPM_ERR_ARG, "eppm_set_temporal: a batch context has no previous pair (its pairs run concurrently)");
    c->temporal = on != 0;
    if (!on) c->tmp_valid = c->tmp_snap = false;
    return EPPM_OK;
}
extern "C" int eppm_temporal_reset(eppm_ctx* c)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_temporal_reset: NULL ctx");
    c->tmp_valid = c->tmp_snap = false;
    return EPPM_OK;
}
extern "C" int eppm_temporal_valid(const eppm_ctx* c) { return c && c->temporal && c->tmp_valid ? 1 : 0; }

static int compute_all(eppm_ctx* c)
{
    if (!c->have_images) return set_err(EPPM_ERR_STATE, "eppm_compute: no images set");
    HIPCHK(hipSetDevice(c->device));
    c->have_bwd = false;
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    const int L = c->nl - 1;                                            // pm_layer, driver :219
    const int lw = c->W[L], lh = c->H[L];

    // temporal mode: the snapshots of the previous pair of the clip, advected, seed this pair's PatchMatch; without them the run is cold
    const bool tmode = c->temporal, seeded = tmode && c->tmp_valid;
    c->tmp_seeded = false;
    if (tmode) CHK(tmp_alloc(c));
    if (seeded) {
        TemporalArgs a;
        a.prev[0] = c->prev_fwd; a.prior[0] = c->prior1; a.keys[0] = c->tmp_keys; a.step[0] = 1;
        a.prev[1] = c->prev_bwd; a.prior[1] = c->prior2; a.keys[1] = c->tmp_keys + (size_t)lw * lh; a.step[1] = -1;
        a.w = lw; a.h = lh; a.ndir = 2;
        stage_begin(c, c->ev, "temporal_advect");
        launch_temporal_splat(a, s);
        launch_temporal_gather(a, s);
        stage_end(c, c->ev);
    }
    c->tmp_valid = c->tmp_snap = false;

    const size_t pm_entry = c->ev.size();
    stage_begin(c, c->ev, "patchmatch");
    {
        PmBatch b;
        b.n = 2; b.cpitch = lw; b.npitch = lw; b.npairs = bt.n; b.stride = bt.stride;
        b.cache_plane = (size_t)lw * lh;
        b.seed_plane = (size_t)lw * lh * 2;
        b.wl_units = pm_worklist_units(lw, lh, c->prm.seg_len);
        b.p[0] = mk_problem(planes(c, L, false), c->cost1, c->nnf1, c->nnf_tmp, c->rng, 0, c->spec1, EPPM_SWEEP_CACHE ? c->scand1 : nullptr, sweep_list_on(c->opt_sweep_spec) ? c->wl1 : nullptr, c->seed1);     // driver :223
        b.p[1] = mk_problem(planes(c, L, true), c->cost2, c->nnf2, c->nnf_tmp2, c->rng, 1, c->spec2, EPPM_SWEEP_CACHE ? c->scand2 : nullptr, sweep_list_on(c->opt_sweep_spec) ? c->wl2 : nullptr, c->seed2);     // driver :224
        if (!seeded) run_patchmatch(b, c->rng, c->lut_pm, c->prm, s, c->opt_sweep_spec);
        else {
            // the random field and its costs as in a cold run (the generator states too), then the prior where it is strictly cheaper
            pm_start(b, c->rng, c->lut_pm, c->prm, s);
            PmSeed sd;
            sd.prior[0] = c->prior1; sd.nnf_init[0] = c->nnf_init1; sd.cost_init[0] = c->cost_init1;
            sd.prior[1] = c->prior2; sd.nnf_init[1] = c->nnf_init2; sd.cost_init[1] = c->cost_init2;
            stage_begin(c, c->ev, "temporal_select");
            launch_pm_cost_select(b, sd, c->lut_pm, c->prm.patch_r, s);
            stage_end(c, c->ev);
            pm_iterate(b, c->rng, c->lut_pm, c->prm, s, c->opt_sweep_spec);
        }
    }
    stage_end_at(c, c->ev, pm_entry);
    if (tmode) launch_temporal_snapshot(c->prev_bwd, c->nnf2, lw, lw, lh, s);          // the raw backward NNF, before the left-right check

    stage_begin(c, c->ev, "l2_post");
    launch_lr_check(c->nnf1, c->cost1, c->nnf2, lw, lh, lw, lw, s, bt);                                      // driver :233
    launch_lr_check(c->nnf2, c->cost2, c->nnf1, lw, lh, lw, lw, s, bt);
    launch_outlier(c->nnf_tmp, c->cost1, c->nnf1, lw, lh, lw, lw, s, bt);                                    // driver :237
    std::swap(c->nnf1, c->nnf_tmp);
    if (launch_wmf(c->nnf1, c->nnf_tmp, c->img1[L], (int)(c->ipitch[L] / 4), lw, lh, lw, c->lut_wmf, c->prm.wmf_iters, 1,      // driver :239
                   c->wmf_ws, s, bt) != c->nnf1)
        std::swap(c->nnf1, c->nnf_tmp);
    launch_fill_holes(c->nnf_tmp, c->nnf1, c->img1[L], (int)(c->ipitch[L] / 4), lw, lh, lw, s, bt);          // driver :240
    std::swap(c->nnf1, c->nnf_tmp);
    if (tmode) launch_nnf2flow_snapshot(c->flow[L], lw, c->prev_fwd, c->nnf1, lw, lw, lh, s);
    else launch_nnf2flow(c->flow[L], lw, c->nnf1, lw, lw, lh, s, bt);                                        // driver :258
    stage_end(c, c->ev);

    static const char* up_names[] = {"upsample_L0", "upsample_L1", "upsample_L2", "upsample_L3", "upsample_L4", "upsample_L5", "upsample_L6"};
    static const char* rf_names[] = {"c2f_refine_L0", "c2f_refine_L1", "c2f_refine_L2", "c2f_refine_L3", "c2f_refine_L4", "c2f_refine_L5", "c2f_refine_L6"};
    static const char* bl_names[] = {"flow_blf_L0", "flow_blf_L1", "flow_blf_L2", "flow_blf_L3", "flow_blf_L4", "flow_blf_L5", "flow_blf_L6"};
    for (int l = L - 1; l >= 0; l--) {                                                                       // driver :275-282
        stage_begin(c, c->ev, up_names[l]);
        launch_resize_flow(c->flow[l], c->H[l], c->W[l], c->flow[l + 1], c->H[l + 1], c->W[l + 1], 2.0f, 2.0f, s, bt);   // refine :1082-1083
        stage_end(c, c->ev);
        stage_begin(c, c->ev, rf_names[l], true);
        launch_c2f_refine(planes(c, l, false), c->flow[l], c->lut_pm, c->prm.patch_r, c->c2f_cost9[l], s, bt, c->opt_no_split != 0);   // refine :1086
        stage_end(c, c->ev, true);
        stage_begin(c, c->ev, bl_names[l]);
        launch_flow_blf(c->flow_tmp[l], c->flow[l], c->img1[l], (int)(c->ipitch[l] / 4), c->W[l], c->H[l], c->W[l], c->lut_blf, s, bt);  // driver :280
        std::swap(c->flow[l], c->flow_tmp[l]);
        stage_end(c, c->ev);
    }
    stage_begin(c, c->ev, "flow_blf_final");
    launch_flow_blf(c->flow_tmp[0], c->flow[0], c->img1[0], (int)(c->ipitch[0] / 4), c->W[0], c->H[0], c->W[0], c->lut_blf, s, bt);      // driver :289
    std::swap(c->flow[0], c->flow_tmp[0]);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    c->have_flow = true;
    c->tmp_snap = tmode;                // a prior is armed by the next push, not by another compute on this pair
    c->tmp_seeded = seeded;
    return EPPM_OK;
}

// ---- bidirectional calls: the backward flow (the reference's commented-out branch, driver :243-245, completed symmetrically) and the
// forward-backward occlusion masks.  DESIGN.md section 10. ----

// the backward planes of every pair: one allocation, made on the first bidirectional call and kept until eppm_destroy
static int bwd_alloc(eppm_ctx* c)
{
    if (c->bwd) return EPPM_OK;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    size_t flow_off[kMaxLevels];
    for (int l = 0; l < c->nl; l++) flow_off[l] = take((size_t)c->W[l] * c->H[l] * 8);
    const size_t n = (size_t)c->h * c->w;
    const size_t out_off = take(n * 10);                 // bu | bv | occ1 | occ2: one device-to-host copy per pair
    c->bwd_stride = (off + 4095) & ~(size_t)4095;
    const size_t bytes = c->bwd_stride * c->npairs;
    const hipError_t e = cache_alloc((void**)&c->bwd, bytes, false, c->device);
    if (e != hipSuccess) { (void)hipGetLastError(); c->bwd = nullptr; return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (backward planes) failed: %s", bytes, hipGetErrorString(e)); }
    c->bwd_bytes = bytes;
    for (int l = 0; l < c->nl; l++) c->bflow[l] = (float*)(c->bwd + flow_off[l]);
    c->d_buv = (float*)(c->bwd + out_off);
    c->occ1 = (uint8_t*)(c->bwd + out_off + n * 8);
    c->occ2 = c->occ1 + n;
    return EPPM_OK;
}

// level l's backward flow of every active pair: from a slab plane (pairs `stride` apart) into bflow[l] (pairs `bwd_stride` apart)
static int keep_bwd(eppm_ctx* c, int l, const float* src)
{
    const size_t bytes = (size_t)c->W[l] * c->H[l] * 8;
    for (int k = 0; k < c->n_active; k++)
        HIPCHK(hipMemcpyAsync(c->bwd + (size_t)k * c->bwd_stride + ((char*)c->bflow[l] - c->bwd), c->of_pair(src, k), bytes, hipMemcpyDeviceToDevice, c->stream));
    return EPPM_OK;
}

// After compute_all, on the same stream: the backward branch from (nnf2, cost2) as the two-pass left-right check left them, then both
// occlusion masks.  Every kernel is the forward path's, with image 2 as the guide and the refine's planes swapped.
static int backward_all(eppm_ctx* c)
{
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    const int L = c->nl - 1;
    const int lw = c->W[L], lh = c->H[L];

    stage_begin(c, c->ev, "l2_post_bwd");
    launch_outlier(c->nnf_tmp2, c->cost2, c->nnf2, lw, lh, lw, lw, s, bt);
    std::swap(c->nnf2, c->nnf_tmp2);
    if (launch_wmf(c->nnf2, c->nnf_tmp2, c->img2[L], (int)(c->ipitch[L] / 4), lw, lh, lw, c->lut_wmf, c->prm.wmf_iters, 1, c->wmf_ws, s, bt) != c->nnf2)
        std::swap(c->nnf2, c->nnf_tmp2);
    launch_fill_holes(c->nnf_tmp2, c->nnf2, c->img2[L], (int)(c->ipitch[L] / 4), lw, lh, lw, s, bt);
    std::swap(c->nnf2, c->nnf_tmp2);
    float* cur = c->flow_tmp[L];                     // the flow so far, in a slab plane
    launch_nnf2flow(cur, lw, c->nnf2, lw, lw, lh, s, bt);
    if (L > 0) CHK(keep_bwd(c, L, cur));
    stage_end(c, c->ev);

    // level l: resize + refine in flow_tmp[l], smoothing into d_uv (h*w float2: room for any level; the forward flow is split into it
    // only after this branch)
    float* scratch = c->d_uv;
    static const char* up_names[] = {"upsample_bwd_L0", "upsample_bwd_L1", "upsample_bwd_L2", "upsample_bwd_L3", "upsample_bwd_L4", "upsample_bwd_L5", "upsample_bwd_L6"};
    static const char* rf_names[] = {"c2f_refine_bwd_L0", "c2f_refine_bwd_L1", "c2f_refine_bwd_L2", "c2f_refine_bwd_L3", "c2f_refine_bwd_L4", "c2f_refine_bwd_L5", "c2f_refine_bwd_L6"};
    static const char* bl_names[] = {"flow_blf_bwd_L0", "flow_blf_bwd_L1", "flow_blf_bwd_L2", "flow_blf_bwd_L3", "flow_blf_bwd_L4", "flow_blf_bwd_L5", "flow_blf_bwd_L6"};
    for (int l = L - 1; l >= 0; l--) {
        stage_begin(c, c->ev, up_names[l]);
        launch_resize_flow(c->flow_tmp[l], c->H[l], c->W[l], cur, c->H[l + 1], c->W[l + 1], 2.0f, 2.0f, s, bt);
        stage_end(c, c->ev);
        stage_begin(c, c->ev, rf_names[l]);
        launch_c2f_refine(planes(c, l, true), c->flow_tmp[l], c->lut_pm, c->prm.patch_r, c->c2f_cost9[l], s, bt, c->opt_no_split != 0);
        stage_end(c, c->ev);
        stage_begin(c, c->ev, bl_names[l]);
        launch_flow_blf(scratch, c->flow_tmp[l], c->img2[l], (int)(c->ipitch[l] / 4), c->W[l], c->H[l], c->W[l], c->lut_blf, s, bt);
        cur = scratch;
        if (l > 0) CHK(keep_bwd(c, l, cur));
        stage_end(c, c->ev);
    }
    stage_begin(c, c->ev, "flow_blf_bwd_final");
    float* out = (cur == scratch) ? c->flow_tmp[0] : scratch;
    launch_flow_blf(out, cur, c->img2[0], (int)(c->ipitch[0] / 4), c->W[0], c->H[0], c->W[0], c->lut_blf, s, bt);
    CHK(keep_bwd(c, 0, out));
    stage_end(c, c->ev);

    stage_begin(c, c->ev, "fb_occlusion");
    launch_fb_occlusion(c->occ1, c->occ2, c->flow[0], c->stride, c->bflow[0], c->bwd_stride, c->h, c->w, c->occ_alpha, c->occ_beta, bt.n, 2, s);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    c->have_bwd = true;
    c->bwd_images = true;
    return EPPM_OK;
}

static int compute_bidir_all(eppm_ctx* c)
{
    if (!c->have_images) return set_err(EPPM_ERR_STATE, "eppm_compute_bidirectional: no images set");
    HIPCHK(hipSetDevice(c->device));
    CHK(bwd_alloc(c));
    CHK(compute_all(c));
    return backward_all(c);
}

extern "C" int eppm_compute_device(eppm_ctx* c, void* d_flow)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    CHK(compute_all(c));
    if (d_flow) HIPCHK(hipMemcpyAsync(d_flow, c->flow[0], (size_t)c->h * c->w * 8, hipMemcpyDeviceToDevice, c->stream));
    return EPPM_OK;
}

extern "C" int eppm_batch_compute_device(eppm_ctx* c, void* const* d_flows)
{
    if (!c) return set_err(EPPM_ERR_ARG, "NULL ctx");
    CHK(compute_all(c));
    if (d_flows)
        for (int k = 0; k < c->n_active; k++)
            if (d_flows[k]) HIPCHK(hipMemcpyAsync(d_flows[k], c->of_pair(c->flow[0], k), (size_t)c->h * c->w * 8, hipMemcpyDeviceToDevice, c->stream));
    return EPPM_OK;
}

// compute_flow split in two so that a host thread can keep several contexts in flight: begin enqueues the whole path, the
// de-interleave (on the device) and the device-to-host copies and returns; end waits.  When begin knows the destination planes
// and they lie in registered memory, the copy engine writes them directly; otherwise the planes land in the context's pinned
// staging and end copies them out.
static int compute_begin_impl(eppm_ctx* c, int n_out, float* const* u, float* const* v, bool bidir)
{
    CHK(bidir ? compute_bidir_all(c) : compute_all(c));
    const size_t n = (size_t)c->h * c->w;
    launch_split_flow(c->d_uv, c->flow[0], (int)n, c->stream, c->bt());                                                           // driver :302-306, on the device
    if (bidir) {
        // bu | bv | occ1 | occ2 of every active pair into the pinned staging (one copy each)
        launch_split_flow(c->d_buv, c->bflow[0], (int)n, c->stream, Batch{c->n_active, c->bwd_stride});
        if (!c->h_bwd) {
            HIPCHK(cache_alloc((void**)&c->h_bwd, n * 10 * c->npairs, true, c->device));
            c->h_bwd_bytes = n * 10 * c->npairs;
        }
        for (int k = 0; k < c->n_active; k++)
            HIPCHK(hipMemcpyAsync(c->h_bwd + (size_t)k * n * 10, c->bwd + (size_t)k * c->bwd_stride + ((char*)c->d_buv - c->bwd), n * 10, hipMemcpyDeviceToHost, c->stream));
    }
    for (int k = 0; k < c->n_active; k++) {                                                                                       // driver :299
        float* du = (u && k < n_out) ? u[k] : nullptr;
        float* dv = (v && k < n_out) ? v[k] : nullptr;
        const float* src = c->of_pair(c->d_uv, k);
        if (du && dv && c->out_hold.add2(du, dv, n * 4)) {          // both planes in registered memory, held until eppm_compute_end
            HIPCHK(hipMemcpyAsync(du, src, n * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(dv, src + n, n * 4, hipMemcpyDeviceToHost, c->stream));
            c->out_u[k] = du; c->out_v[k] = dv;
            continue;
        }
        if (!c->h_flow) {
            c->h_flow_bytes = n * 8 * c->npairs;
            HIPCHK(cache_alloc((void**)&c->h_flow, c->h_flow_bytes, true, c->device));
        }
        HIPCHK(hipMemcpyAsync(c->h_flow + (size_t)k * n * 2, src, n * 8, hipMemcpyDeviceToHost, c->stream));
        c->out_u[k] = c->out_v[k] = nullptr;
    }
    c->flow_pending = true;
    return EPPM_OK;
}
static int compute_begin(eppm_ctx* c, int n_out, float* const* u, float* const* v, bool bidir = false)
{
    const int r = compute_begin_impl(c, n_out, u, v, bidir);
    if (r != EPPM_OK && !c->out_hold.v.empty()) {
        // eppm_compute_end will refuse to run (nothing is pending): the planes held so far must not stay in use until the context dies.
        // Copies already queued into them drain first.
        (void)hipStreamSynchronize(c->stream);
        c->out_hold.release();
    }
    return r;
}

extern "C" int eppm_compute_begin(eppm_ctx* c)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_compute_begin: NULL ctx");
    return compute_begin(c, 0, nullptr, nullptr);
}

extern "C" int eppm_compute_begin_into(eppm_ctx* c, float* u, float* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_compute_begin_into: NULL argument");
    return compute_begin(c, 1, &u, &v);
}

extern "C" int eppm_batch_compute_begin_into(eppm_ctx* c, float* const* u, float* const* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_batch_compute_begin_into: NULL argument");
    return compute_begin(c, c->n_active, u, v);
}

static int compute_end(eppm_ctx* c, int n_out, float* const* u, float* const* v)
{
    if (!c->flow_pending) return set_err(EPPM_ERR_STATE, "eppm_compute_end without eppm_compute_begin");
    HIPCHK(hipSetDevice(c->device));
    const hipError_t es = hipStreamSynchronize(c->stream);
    c->out_hold.release();              // the copy engine has left the caller's planes (or the stream is broken)
    HIPCHK(es);
    c->flow_pending = false;
    const size_t n = (size_t)c->h * c->w;
    for (int k = 0; k < n_out && k < c->n_active; k++) {
        if (!u[k] || !v[k]) continue;
        // the planes are in the caller's memory already (begin_into, registered), or in the staging buffer: u plane, then v plane
        const float* fu = c->out_u[k] ? c->out_u[k] : c->h_flow + (size_t)k * n * 2;
        const float* fv = c->out_v[k] ? c->out_v[k] : c->h_flow + (size_t)k * n * 2 + n;
        if (u[k] != fu) memcpy(u[k], fu, n * sizeof(float));
        if (v[k] != fv) memcpy(v[k], fv, n * sizeof(float));
    }
    return EPPM_OK;
}

extern "C" int eppm_compute_end(eppm_ctx* c, float* u, float* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_compute_end: NULL argument");
    return compute_end(c, 1, &u, &v);
}

extern "C" int eppm_batch_compute_end(eppm_ctx* c, float* const* u, float* const* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_batch_compute_end: NULL argument");
    return compute_end(c, c->n_active, u, v);
}

extern "C" int eppm_compute(eppm_ctx* c, float* u, float* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_compute: NULL argument");
    CHK(compute_begin(c, 1, &u, &v));
    return compute_end(c, 1, &u, &v);
}

extern "C" int eppm_batch_compute(eppm_ctx* c, float* const* u, float* const* v)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_batch_compute: NULL argument");
    CHK(compute_begin(c, c->n_active, u, v));
    return compute_end(c, c->n_active, u, v);
}

// the backward outputs of a finished bidirectional call, from the pinned staging; NULL tables / entries are skipped
static void bwd_copy_out(eppm_ctx* c, int n_out, float* const* bu, float* const* bv, uint8_t* const* o1, uint8_t* const* o2)
{
    const size_t n = (size_t)c->h * c->w;
    for (int k = 0; k < n_out && k < c->n_active; k++) {
        const uint8_t* src = c->h_bwd + (size_t)k * n * 10;
        if (bu && bu[k]) memcpy(bu[k], src, n * 4);
        if (bv && bv[k]) memcpy(bv[k], src + n * 4, n * 4);
        if (o1 && o1[k]) memcpy(o1[k], src + n * 8, n);
        if (o2 && o2[k]) memcpy(o2[k], src + n * 9, n);
    }
}

static int compute_bidir(eppm_ctx* c, int n_out, float* const* u, float* const* v, float* const* bu, float* const* bv, uint8_t* const* o1,
                         uint8_t* const* o2)
{
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "eppm_compute_bidirectional: an eppm_compute_begin is pending");
    CHK(compute_begin(c, n_out, u, v, true));
    CHK(compute_end(c, n_out, u, v));
    bwd_copy_out(c, n_out, bu, bv, o1, o2);
    return EPPM_OK;
}

extern "C" int eppm_compute_bidirectional(eppm_ctx* c, float* u, float* v, float* bu, float* bv, uint8_t* occ1, uint8_t* occ2)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_compute_bidirectional: NULL argument");
    return compute_bidir(c, 1, &u, &v, &bu, &bv, &occ1, &occ2);
}

extern "C" int eppm_batch_compute_bidirectional(eppm_ctx* c, float* const* u, float* const* v, float* const* bu, float* const* bv,
                                                uint8_t* const* occ1, uint8_t* const* occ2)
{
    if (!c || !u || !v) return set_err(EPPM_ERR_ARG, "eppm_batch_compute_bidirectional: NULL argument");
    return compute_bidir(c, c->n_active, u, v, bu, bv, occ1, occ2);
}

extern "C" int eppm_compute_bidirectional_device(eppm_ctx* c, void* d_flow, void* d_flow_bwd, void* d_occ1, void* d_occ2)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_compute_bidirectional_device: NULL ctx");
    CHK(compute_bidir_all(c));
    const size_t n = (size_t)c->h * c->w;
    if (d_flow) HIPCHK(hipMemcpyAsync(d_flow, c->flow[0], n * 8, hipMemcpyDeviceToDevice, c->stream));
    if (d_flow_bwd) HIPCHK(hipMemcpyAsync(d_flow_bwd, c->bflow[0], n * 8, hipMemcpyDeviceToDevice, c->stream));
    if (d_occ1) HIPCHK(hipMemcpyAsync(d_occ1, c->occ1, n, hipMemcpyDeviceToDevice, c->stream));
    if (d_occ2) HIPCHK(hipMemcpyAsync(d_occ2, c->occ2, n, hipMemcpyDeviceToDevice, c->stream));
    return EPPM_OK;
}

extern "C" int eppm_set_occlusion_params(eppm_ctx* c, float alpha, float beta)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_set_occlusion_params: NULL ctx");
    if (!(alpha >= 0 && isfinite(alpha)) || !(beta >= 0 && isfinite(beta)))
        return set_err(EPPM_ERR_ARG, "eppm_set_occlusion_params: alpha %g, beta %g must be finite and >= 0", alpha, beta);
    c->occ_alpha = alpha;
    c->occ_beta = beta;
    return EPPM_OK;
}

// ---- frame interpolation: the raw RGBA frames (written only by set_images, read only by prepare), the level-0
// forward flow and both masks of the last bidirectional call, all still in the context ----

static int itp_alloc(eppm_ctx* c)
{
    if (c->itp) return EPPM_OK;
    const size_t n = (size_t)c->h * c->w, slots = (size_t)c->npairs * kInterpChunk;
    const size_t plane = (n + 63) & ~(size_t)63;
    const size_t keys = slots * plane * 8, fills = slots * plane * 4, rgb = slots * n * 3;
    const size_t bytes = keys + 2 * fills + rgb;
    const hipError_t e = cache_alloc((void**)&c->itp, bytes, false, c->device);
    if (e != hipSuccess) { (void)hipGetLastError(); c->itp = nullptr; return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (interpolation scratch) failed: %s", bytes, hipGetErrorString(e)); }
    c->itp_bytes = bytes;
    c->itp_plane = plane;
    c->itp_keys = (uint64_t*)c->itp;
    c->itp_fill1 = (int32_t*)(c->itp + keys);
    c->itp_fill2 = (int32_t*)(c->itp + keys + fills);
    c->itp_rgb = (uint8_t*)(c->itp + keys + 2 * fills);
    return EPPM_OK;
}

static int interp_check(eppm_ctx* c, const char* what, int nt, const float* t)
{
    if (nt < 1 || !t) return set_err(EPPM_ERR_ARG, "%s: nt %d, t %p", what, nt, (const void*)t);
    for (int k = 0; k < nt; k++)
        if (!interp_t_ok(t[k])) return set_err(EPPM_ERR_ARG, "%s: t[%d] = %g outside [0, 1]", what, k, t[k]);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (!c->have_bwd || !c->bwd_images) return set_err(EPPM_ERR_STATE, "%s: needs a bidirectional call on the current images", what);
    return EPPM_OK;
}

// times t[k0 .. k0+nt) of the first npairs pairs: splat, fill, blend into the packed RGB scratch (d_rgba NULL) or into d_rgba[k0 + k] (pair 0)
static int interp_chunk(eppm_ctx* c, int npairs, int k0, int nt, const float* t, void* const* d_rgba, size_t pitch)
{
    InterpArgs a{};
    a.img1 = (const uint8_t*)c->raw1; a.img2 = (const uint8_t*)c->raw2; a.img_pitch = c->raw_pitch; a.img_stride = c->stride;
    a.flow = c->flow[0]; a.flow_stride = c->stride;
    a.occ1 = c->occ1; a.occ2 = c->occ2; a.occ_stride = c->bwd_stride;
    a.keys = c->itp_keys; a.fill1 = c->itp_fill1; a.fill2 = c->itp_fill2; a.plane = c->itp_plane;
    a.rgb = d_rgba ? nullptr : c->itp_rgb;
    a.rgba_pitch = pitch;
    a.h = c->h; a.w = c->w; a.nt = nt;
    for (int k = 0; k < kInterpChunk; k++) {
        a.t[k] = k < nt ? t[k0 + k] : 0.0f;
        a.rgba[k] = (d_rgba && k < nt) ? (uint8_t*)d_rgba[k0 + k] : nullptr;
    }
    stage_begin(c, c->ev, "interp_splat");
    launch_interp_splat(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "interp_fill");
    launch_interp_fill(a, npairs, c->stream);
    stage_end(c, c->ev);
    stage_begin(c, c->ev, "interp_blend");
    launch_interp_blend(a, npairs, c->stream);
    stage_end(c, c->ev);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

// host-pointer forms: each chunk's packed RGB outputs cross PCIe once (3 B/px) into the pinned copy, then into the caller's rows
static int interp_host(eppm_ctx* c, const char* what, int npairs, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    CHK(interp_check(c, what, nt, t));
    if (!rgb) return set_err(EPPM_ERR_ARG, "%s: NULL rgb", what);
    for (int k = 0; k < npairs * nt; k++)
        if (!rgb[k]) return set_err(EPPM_ERR_ARG, "%s: NULL rgb[%d]", what, k);
    if (row_stride < (size_t)c->w * 3) return set_err(EPPM_ERR_ARG, "%s: row_stride %zu < 3*w", what, row_stride);
    HIPCHK(hipSetDevice(c->device));
    CHK(itp_alloc(c));
    const size_t img = (size_t)c->h * c->w * 3, row = (size_t)c->w * 3;
    if (!c->h_itp) {
        HIPCHK(cache_alloc((void**)&c->h_itp, img * c->npairs * kInterpChunk, true, c->device));
        c->h_itp_bytes = img * c->npairs * kInterpChunk;
    }
    for (int k0 = 0; k0 < nt; k0 += kInterpChunk) {
        const int m = nt - k0 < kInterpChunk ? nt - k0 : kInterpChunk;
        CHK(interp_chunk(c, npairs, k0, m, t, nullptr, 0));
        HIPCHK(hipMemcpyAsync(c->h_itp, c->itp_rgb, img * npairs * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int p = 0; p < npairs; p++)
            for (int k = 0; k < m; k++) {
                const uint8_t* src = c->h_itp + img * ((size_t)p * m + k);
                uint8_t* dst = rgb[(size_t)p * nt + k0 + k];
                if (row_stride == row) memcpy(dst, src, img);
                else
                    for (int y = 0; y < c->h; y++) memcpy(dst + (size_t)y * row_stride, src + (size_t)y * row, row);
            }
    }
    return EPPM_OK;
}

extern "C" int eppm_interpolate(eppm_ctx* c, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_interpolate: NULL ctx");
    return interp_host(c, "eppm_interpolate", 1, nt, t, rgb, row_stride);
}

extern "C" int eppm_batch_interpolate(eppm_ctx* c, int nt, const float* t, uint8_t* const* rgb, size_t row_stride)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_interpolate: NULL ctx");
    return interp_host(c, "eppm_batch_interpolate", c->n_active, nt, t, rgb, row_stride);
}

extern "C" int eppm_interpolate_device(eppm_ctx* c, int nt, const float* t, void* const* d_rgba, size_t pitch)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL ctx");
    CHK(interp_check(c, "eppm_interpolate_device", nt, t));
    if (!d_rgba) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL d_rgba");
    for (int k = 0; k < nt; k++)
        if (!d_rgba[k]) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: NULL d_rgba[%d]", k);
    if (pitch < (size_t)c->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_interpolate_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(c->device));
    CHK(itp_alloc(c));
    for (int k0 = 0; k0 < nt; k0 += kInterpChunk)
        CHK(interp_chunk(c, 1, k0, nt - k0 < kInterpChunk ? nt - k0 : kInterpChunk, t, d_rgba, pitch));
    return EPPM_OK;
}

// ---- dense point trajectories (tracker.cpp): the raw frames, the level-0 forward flow and the level-0 backward flow
// of one pair, in the window of eppm_interpolate* ----

int ctx_track_inputs(eppm_ctx* c, int pair, int h, int w, int device, const char* what, TrackIn* in, hipStream_t* s)
{
    if (c->h != h || c->w != w || c->device != device)
        return set_err(EPPM_ERR_ARG, "%s: the tracker is %dx%d on device %d, the context %dx%d on device %d", what, w, h, device, c->w, c->h, c->device);
    if (pair < 0 || pair >= c->n_active) return set_err(EPPM_ERR_ARG, "%s: pair %d, the context has %d active", what, pair, c->n_active);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "%s: an eppm_compute_begin is pending", what);
    if (!c->have_bwd || !c->bwd_images) return set_err(EPPM_ERR_STATE, "%s: needs a bidirectional call on the current images", what);
    HIPCHK(hipSetDevice(c->device));
    in->img1 = (const uint8_t*)c->of_pair(c->raw1, pair);
    in->img2 = (const uint8_t*)c->of_pair(c->raw2, pair);
    in->pitch = c->raw_pitch;
    in->fwd = c->of_pair(c->flow[0], pair);
    in->bwd = (const float*)(c->bwd + (size_t)pair * c->bwd_stride + ((char*)c->bflow[0] - c->bwd));
    in->h = c->h;
    in->w = c->w;
    *s = c->stream;
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
        if (!c->tmp_seeded) return set_err(EPPM_ERR_STATE, "eppm_get_plane: '%s' needs a compute that started from a temporal prior", name);
        src = n == "prior1" ? (void*)c->prior1 : n == "prior2" ? (void*)c->prior2 : n == "nnf_init1" ? (void*)c->nnf_init1 : n == "nnf_init2" ? (void*)c->nnf_init2
            : n == "cost_init1" ? (void*)c->cost_init1 : (void*)c->cost_init2;
        esz = 4; pitch = (size_t)w * 4;
        pstride = 0;
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
