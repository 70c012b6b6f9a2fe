// ctx_compute.cpp -- what a context (context.h) computes: compute (compute_flow, driver :217-306) in its host, device, begin / end and
// bidirectional forms, the temporal mode's switches, and the post-PatchMatch branch that the forward and the backward flow share.
#include "context.h"
#include "temporal.h"

using namespace eppm;

// ---- temporal mode ----
// one block per slot (context.h): 40 bytes per level-L pixel, every plane at a 256-byte aligned offset
static int tmp_alloc(eppm_ctx* c)
{
    if (c->tmp) return EPPM_OK;
    const int L = c->nl - 1;
    const size_t n2 = (size_t)c->W[L] * c->H[L];
    Carve cv;
    for (int16_t** p : {&c->prev_fwd, &c->prev_bwd, &c->prior1, &c->prior2, &c->nnf_init1, &c->nnf_init2}) cv.plane(p, n2 * 4);
    for (float** p : {&c->cost_init1, &c->cost_init2}) cv.plane(p, n2 * 4);
    cv.plane(&c->tmp_keys, n2 * 4 * 2);                    // the keys of both directions
    c->tmp_stride = cv.off;
    CHK(cv.alloc(&c->tmp, &c->tmp_bytes, c->tmp_stride * c->npairs, c->device, "temporal planes"));
    for (int k = 0; k < c->npairs; k++) launch_temporal_keys_init((int32_t*)((char*)c->tmp_keys + (size_t)k * c->tmp_stride), (int)(2 * n2), c->stream);
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

static int set_temporal(eppm_ctx* c, int on)
{
    c->temporal = on != 0;
    if (!on) c->tmp_drop();
    return EPPM_OK;
}
extern "C" int eppm_set_temporal(eppm_ctx* c, int on)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_set_temporal: NULL ctx");
    if (on && c->npairs != 1) return set_err(EPPM_ERR_ARG, "eppm_set_temporal: a batch context streams through eppm_batch_set_temporal (one clip per slot)");
    return set_temporal(c, on);
}
extern "C" int eppm_temporal_reset(eppm_ctx* c)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_temporal_reset: NULL ctx");
    return eppm_batch_temporal_reset(c, 0);
}
extern "C" int eppm_temporal_valid(const eppm_ctx* c) { return eppm_batch_temporal_valid(c, 0); }

// the batch forms: one clip per slot (include/eppm.h)
extern "C" int eppm_batch_set_temporal(eppm_ctx* c, int on)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_set_temporal: NULL ctx");
    return set_temporal(c, on);
}
extern "C" int eppm_batch_temporal_reset(eppm_ctx* c, int pair)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_batch_temporal_reset: NULL ctx");
    if (pair >= c->npairs) return set_err(EPPM_ERR_ARG, "eppm_batch_temporal_reset: pair %d, context holds %d", pair, c->npairs);
    for (int k = pair < 0 ? 0 : pair; k < (pair < 0 ? c->npairs : pair + 1); k++) c->tmp_valid[k] = c->tmp_snap[k] = 0;
    return EPPM_OK;
}
extern "C" int eppm_batch_temporal_valid(const eppm_ctx* c, int pair)
{
    return c && pair >= 0 && pair < c->npairs && c->temporal && c->tmp_valid[pair] ? 1 : 0;
}

// ---- the post-PatchMatch branch (driver :237-289): outlier vote, weighted median, hole fill, NNF -> flow at the PatchMatch level, then
// per level upsample, candidate refine, smoothing, then the final smoothing.  One direction of it: ----
struct Branch {
    int16_t *&nnf, *&nnf_alt;       // the direction's field and its ping-pong partner (members of the context: they are exchanged)
    float* cost;
    uint32_t* const* guide;         // the pyramid of the image the field is defined on
    bool swap, bwd, dominant;       // planes(): image 2 against image 1; stage names carry "_bwd"; the refine is timing mode 2's stage
    int16_t* snapshot;              // not NULL: the converted field of every pair is kept as well (launch_nnf2flow_snapshot), tmp_stride apart
    // level l is resized and refined in a[l] and smoothed into b[l]; the final smoothing writes level 0's plane that does not hold its input
    float *a[kMaxLevels], *b[kMaxLevels];
};

// "upsample_L2", "c2f_refine_bwd_L0", ...: the per-level stage names of both directions, built once when the library is loaded
enum { kStageUp, kStageRefine, kStageBlf, kStageJbu };
static const struct EPPM_HIDDEN LevelStageNames {
    char s[4][2][kMaxLevels][24];       // [stage][backward][level]
    LevelStageNames()
    {
        const char* base[4] = {"upsample", "c2f_refine", "flow_blf", "flow_jbu"};
        for (int k = 0; k < 4; k++)
            for (int b = 0; b < 2; b++)
                for (int l = 0; l < kMaxLevels; l++) snprintf(s[k][b][l], sizeof s[k][b][l], "%s%s_L%d", base[k], b ? "_bwd" : "", l);
    }
} level_stage;

// the PatchMatch level, inside the caller's stage: the field after the left-right check -> the flow in a[L]
static void branch_nnf2flow(eppm_ctx* c, Branch& d)
{
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    const int L = c->nl - 1, lw = c->W[L], lh = c->H[L], gp = (int)(c->ipitch[L] / 4);
    launch_outlier(d.nnf_alt, d.cost, d.nnf, lw, lh, lw, lw, s, bt);                                         // driver :237
    std::swap(d.nnf, d.nnf_alt);
    if (launch_wmf(d.nnf, d.nnf_alt, d.guide[L], gp, lw, lh, lw, c->lut_wmf, c->prm.wmf_iters, 1, c->wmf_ws, s, bt) != d.nnf)   // driver :239
        std::swap(d.nnf, d.nnf_alt);
    launch_fill_holes(d.nnf_alt, d.nnf, d.guide[L], gp, lw, lh, lw, s, bt);                                  // driver :240
    std::swap(d.nnf, d.nnf_alt);
    if (d.snapshot) launch_nnf2flow_snapshot(d.a[L], lw, d.snapshot, c->tmp_stride, d.nnf, lw, lw, lh, s, bt);
    else launch_nnf2flow(d.a[L], lw, d.nnf, lw, lw, lh, s, bt);                                              // driver :258
}

// The levels below it (driver :275-289).  keep(c, l, r): r holds level l's result -- what level l's smoothing wrote for l > 0, what the
// final smoothing wrote for level 0 --; called inside that stage, before anything overwrites r.
// Draft mode (stop_level s > 0): the levels below s are one upsampling launch each, written into the level's plane
// that is not the launch's input (the backward branch smooths every level into the same plane), and no final smoothing follows.
static int branch_c2f(eppm_ctx* c, Branch& d, int (*keep)(eppm_ctx*, int, float*))
{
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    const int L = c->nl - 1;
    auto blf = [&](float* dst, const float* src, int l) { launch_flow_blf(dst, src, d.guide[l], (int)(c->ipitch[l] / 4), c->W[l], c->H[l], c->W[l], c->lut_blf, s, bt); };
    const int stop = c->stop_level;
    float* r = d.a[L];
    for (int l = L - 1; l >= 0; l--) {
        if (l < stop) {
            stage_begin(c, c->ev, level_stage.s[kStageJbu][d.bwd][l]);
            float* out = (r == d.b[l]) ? d.a[l] : d.b[l];
            launch_flow_jbu(out, r, d.guide[l], (int)(c->ipitch[l] / 4), c->W[l], c->H[l], c->W[l + 1], c->H[l + 1], c->lut_blf, s, bt);
            r = out;
            CHK(keep(c, l, r));
            stage_end(c, c->ev);
            continue;
        }
        stage_begin(c, c->ev, level_stage.s[kStageUp][d.bwd][l]);
        launch_resize_flow(d.a[l], c->H[l], c->W[l], r, c->H[l + 1], c->W[l + 1], 2.0f, 2.0f, s, bt);        // refine :1082-1083
        stage_end(c, c->ev);
        stage_begin(c, c->ev, level_stage.s[kStageRefine][d.bwd][l], d.dominant);
        launch_c2f_refine(planes(c, l, d.swap), d.a[l], c->lut_pm, c->prm.patch_r, c->c2f_cost9[l], s, bt, c->opt_no_split != 0, c->opt_c2f_pre);   // refine :1086
        stage_end(c, c->ev, d.dominant);
        stage_begin(c, c->ev, level_stage.s[kStageBlf][d.bwd][l]);
        blf(d.b[l], d.a[l], l);                                                                              // driver :280
        r = d.b[l];
        if (l > 0) CHK(keep(c, l, r));
        stage_end(c, c->ev);
    }
    if (stop > 0) return EPPM_OK;
    stage_begin(c, c->ev, d.bwd ? "flow_blf_bwd_final" : "flow_blf_final");
    float* out = (r == d.b[0]) ? d.a[0] : d.b[0];
    blf(out, r, 0);                                                                                          // driver :289
    CHK(keep(c, 0, out));
    stage_end(c, c->ev);
    return EPPM_OK;
}

// flow[l] names level l's result, whichever of the level's two planes it was written into
static int keep_fwd(eppm_ctx* c, int l, float* r)
{
    if (r != c->flow[l]) std::swap(c->flow[l], c->flow_tmp[l]);
    return EPPM_OK;
}

static int compute_all(eppm_ctx* c)
{
    if (!c->have_images) return set_err(EPPM_ERR_STATE, "eppm_compute: no images set");
    HIPCHK(hipSetDevice(c->device));
    c->have_bwd = false;
    hipStream_t s = c->stream;
    const Batch bt = c->bt();
    const int L = c->nl - 1, lw = c->W[L], lh = c->H[L];                // pm_layer, driver :219

    // temporal mode: per slot, the snapshots of the previous pair of the slot's clip, advected, seed this pair's PatchMatch; a slot without
    // them gets "no prior" everywhere, which leaves it a cold run's bits; no slot with them: the run is the cold one
    const bool tmode = c->temporal;
    bool seeded = false;
    std::fill(c->tmp_seeded.begin(), c->tmp_seeded.end(), 0);
    if (tmode) {
        CHK(tmp_alloc(c));
        TemporalArgs a{};
        for (int k = 0; k < bt.n; k++)
            if (c->tmp_valid[k]) { a.armed[k >> 5] |= 1u << (k & 31); seeded = true; }
        if (seeded) {
            a.prev[0] = c->prev_fwd; a.prior[0] = c->prior1; a.keys[0] = c->tmp_keys; a.step[0] = 1;
            a.prev[1] = c->prev_bwd; a.prior[1] = c->prior2; a.keys[1] = c->tmp_keys + (size_t)lw * lh; a.step[1] = -1;
            a.w = lw; a.h = lh; a.ndir = 2; a.nslots = bt.n; a.stride = c->tmp_stride;
            stage_begin(c, c->ev, "temporal_advect");
            launch_temporal_splat(a, s);
            launch_temporal_gather(a, s);
            stage_end(c, c->ev);
        }
    }
    std::fill(c->tmp_snap.begin(), c->tmp_snap.end(), 0);

    const size_t pm_entry = c->ev.size();
    stage_begin(c, c->ev, "patchmatch");
    {
        PmBatch b;
        b.n = 2; b.cpitch = lw; b.npitch = lw; b.npairs = bt.n; b.stride = bt.stride;
        b.cache_plane = (size_t)lw * lh;
        b.seed_plane = (size_t)lw * lh * 2;
        b.wl_units = pm_worklist_units(lw, lh, c->prm.seg_len);
        b.p[0] = mk_problem(planes(c, L, false), c->cost1, c->nnf1, c->nnf_tmp, c->rng, 0, c->spec1, EPPM_SWEEP_CACHE ? c->scand1 : nullptr, sweep_list_on(c->opt_sweep_spec) ? c->wl1 : nullptr, c->seed1, c->restw1);     // driver :223
        b.p[1] = mk_problem(planes(c, L, true), c->cost2, c->nnf2, c->nnf_tmp2, c->rng, 1, c->spec2, EPPM_SWEEP_CACHE ? c->scand2 : nullptr, sweep_list_on(c->opt_sweep_spec) ? c->wl2 : nullptr, c->seed2, c->restw2);     // driver :224
        if (!seeded) run_patchmatch(b, c->rng, c->lut_pm, c->prm, s, c->opt_sweep_spec, c->opt_search_pre);
        else {
            // the random field and its costs as in a cold run (the generator states too), then the prior where it is strictly cheaper
            pm_start(b, c->rng, c->lut_pm, c->prm, s, c->opt_search_pre);
            PmSeed sd;
            sd.prior[0] = c->prior1; sd.nnf_init[0] = c->nnf_init1; sd.cost_init[0] = c->cost_init1;
            sd.prior[1] = c->prior2; sd.nnf_init[1] = c->nnf_init2; sd.cost_init[1] = c->cost_init2;
            sd.stride = c->tmp_stride;
            stage_begin(c, c->ev, "temporal_select");
            launch_pm_cost_select(b, sd, c->lut_pm, c->prm.patch_r, s);
            stage_end(c, c->ev);
            pm_iterate(b, c->rng, c->lut_pm, c->prm, s, c->opt_sweep_spec, c->opt_search_pre);
        }
    }
    stage_end_at(c, c->ev, pm_entry);
    if (tmode) launch_temporal_snapshot(c->prev_bwd, c->tmp_stride, c->nnf2, lw, lw, lh, s, bt);     // the raw backward NNF, before the left-right check

    stage_begin(c, c->ev, "l2_post");
    launch_lr_check(c->nnf1, c->cost1, c->nnf2, lw, lh, lw, lw, s, bt);                                      // driver :233
    launch_lr_check(c->nnf2, c->cost2, c->nnf1, lw, lh, lw, lw, s, bt);
    Branch d{c->nnf1, c->nnf_tmp, c->cost1, c->img1, false, false, true, tmode ? c->prev_fwd : nullptr};
    for (int l = 0; l <= L; l++) { d.a[l] = c->flow[l]; d.b[l] = c->flow_tmp[l]; }
    branch_nnf2flow(c, d);
    stage_end(c, c->ev);
    CHK(branch_c2f(c, d, keep_fwd));
    HIPCHK(hipGetLastError());
    c->have_flow = true;
    // a prior is armed by the next push, not by another compute on this pair; the pair across a cut leaves none
    for (int k = 0; k < bt.n; k++) {
        c->tmp_snap[k] = tmode && !c->tmp_cut[k];
        c->tmp_seeded[k] = tmode && c->tmp_valid[k];
    }
    std::fill(c->tmp_valid.begin(), c->tmp_valid.end(), 0);
    return EPPM_OK;
}

// ---- bidirectional calls: the backward flow (the reference's commented-out branch, driver :243-245, completed symmetrically) and the
// forward-backward occlusion masks.  DESIGN.md section 10. ----

// the backward planes of every pair: one allocation, made on the first bidirectional call and kept until eppm_destroy
static int bwd_alloc(eppm_ctx* c)
{
    if (c->bwd) return EPPM_OK;
    Carve cv;
    for (int l = 0; l < c->nl; l++) cv.plane(&c->bflow[l], (size_t)c->W[l] * c->H[l] * 8);
    const size_t n = (size_t)c->h * c->w;
    cv.plane(&c->d_buv, n * 10);                         // bu | bv | occ1 | occ2: one device-to-host copy per pair
    c->bwd_stride = (cv.off + 4095) & ~(size_t)4095;
    CHK(cv.alloc(&c->bwd, &c->bwd_bytes, c->bwd_stride * c->npairs, c->device, "backward planes"));
    c->occ1 = (uint8_t*)c->d_buv + n * 8;
    c->occ2 = c->occ1 + n;
    return EPPM_OK;
}

// level l's backward flow of every active pair: from a slab plane (pairs `stride` apart) into bflow[l] (pairs `bwd_stride` apart)
static int keep_bwd(eppm_ctx* c, int l, float* src)
{
    const size_t bytes = (size_t)c->W[l] * c->H[l] * 8;
    for (int k = 0; k < c->n_active; k++)
        HIPCHK(hipMemcpyAsync(c->of_bwd_pair(c->bflow[l], k), c->of_pair(src, k), bytes, hipMemcpyDeviceToDevice, c->stream));
    return EPPM_OK;
}

// After compute_all, on the same stream: the backward branch from (nnf2, cost2) as the two-pass left-right check left them, then both
// occlusion masks.  Image 2 is the guide, the refine's planes are swapped; level l's resize + refine run in flow_tmp[l], every smoothing
// writes d_uv (h*w float2: room for any level; the forward flow is split into it only after this branch) and is copied into bflow.
static int backward_all(eppm_ctx* c)
{
    const int L = c->nl - 1;
    Branch d{c->nnf2, c->nnf_tmp2, c->cost2, c->img2, true, true, false, nullptr};
    for (int l = 0; l <= L; l++) { d.a[l] = c->flow_tmp[l]; d.b[l] = c->d_uv; }
    stage_begin(c, c->ev, "l2_post_bwd");
    branch_nnf2flow(c, d);
    if (L > 0) CHK(keep_bwd(c, L, d.a[L]));
    stage_end(c, c->ev);
    CHK(branch_c2f(c, d, keep_bwd));

    stage_begin(c, c->ev, "fb_occlusion");
    launch_fb_occlusion(c->occ1, c->occ2, c->flow[0], c->stride, c->bflow[0], c->bwd_stride, c->h, c->w, c->occ_alpha, c->occ_beta, c->n_active, 2, c->stream);
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
        HIPCHK(pinned_lazy(&c->h_bwd, &c->h_bwd_bytes, n * 10 * c->npairs, c->device));
        for (int k = 0; k < c->n_active; k++)
            HIPCHK(hipMemcpyAsync(c->h_bwd + (size_t)k * n * 10, c->of_bwd_pair(c->d_buv, k), n * 10, hipMemcpyDeviceToHost, c->stream));
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
        HIPCHK(pinned_lazy(&c->h_flow, &c->h_flow_bytes, n * 8 * c->npairs, c->device));
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

// ---- draft mode ----
extern "C" int eppm_set_stop_level(eppm_ctx* c, int level)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_set_stop_level: NULL ctx");
    if (level < 0 || level > c->nl - 1) return set_err(EPPM_ERR_ARG, "eppm_set_stop_level: level %d outside 0 .. %d", level, c->nl - 1);
    if (c->flow_pending) return set_err(EPPM_ERR_STATE, "eppm_set_stop_level: an eppm_compute_begin is pending");
    c->stop_level = level;
    c->have_flow = c->have_bwd = false;          // the planes are another setting's: interpolate / track wait for the next compute
    return EPPM_OK;
}
extern "C" int eppm_stop_level(const eppm_ctx* c) { return c ? c->stop_level : -1; }

extern "C" int eppm_set_occlusion_params(eppm_ctx* c, float alpha, float beta)
{
    if (!c) return set_err(EPPM_ERR_ARG, "eppm_set_occlusion_params: NULL ctx");
    if (!(alpha >= 0 && isfinite(alpha)) || !(beta >= 0 && isfinite(beta)))
        return set_err(EPPM_ERR_ARG, "eppm_set_occlusion_params: alpha %g, beta %g must be finite and >= 0", alpha, beta);
    c->occ_alpha = alpha;
    c->occ_beta = beta;
    return EPPM_OK;
}
