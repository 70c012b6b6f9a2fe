// context.h -- eppm_ctx, the object behind class bao_flow_patchmatch_multiscale_cuda, and the helpers its translation units share.
// Private to context.cpp and ctx_*.cpp (api_internal.h lists them); everything else goes through the ctx_* accessors of api_internal.h.
// No member may depend on EPPM_TEST_HOOKS: the test library links context_test.o against the product's other objects.
#pragma once

#include <algorithm>

#include "api_internal.h"

struct StageEv { const char* name; hipEvent_t a, b; };

// One context = a batch of `npairs` independent pairs of one size (1 for the plain eppm_create).  Every device plane of
// pair k lives at the same offset inside pair k's SLAB and the slabs are `stride` bytes apart in one allocation, so every
// launch covers all active pairs: it gets pair 0's pointers and {n_active, stride} (eppm_internal.h: Batch), and
// blockIdx.z / .y selects the pair.  The pointer members below are pair 0's; ping-pong swaps apply to every pair alike.
struct eppm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int opt_sweep_spec = -1, opt_no_split = 0, opt_search_pre = -1, opt_c2f_pre = -1;     // kernel-variant switches, copied from the process defaults at creation (test support)
    eppm_params prm;
    int h = 0, w = 0, nl = 0;
    int stop_level = 0;                 // draft mode (eppm_set_stop_level): levels below it are upsampled, not refined
    int npairs = 1, n_active = 1;
    char* slab = nullptr;
    size_t stride = 0;
    int H[eppm::kMaxLevels], W[eppm::kMaxLevels];
    size_t ipitch[eppm::kMaxLevels], cpitch[eppm::kMaxLevels];   // bytes
    uint32_t *raw1 = nullptr, *raw2 = nullptr;
    size_t raw_pitch = 0;
    uint32_t *img1[eppm::kMaxLevels] = {}, *img2[eppm::kMaxLevels] = {}, *tmpu[eppm::kMaxLevels] = {};
    uint8_t *cen1[eppm::kMaxLevels] = {}, *cen2[eppm::kMaxLevels] = {};
    void *pk1[eppm::kMaxLevels] = {}, *pk2[eppm::kMaxLevels] = {};       // float4 texel planes {r,g,b,census}, linear (pitch = w)
    uint32_t *pc1[eppm::kMaxLevels] = {}, *pc2[eppm::kMaxLevels] = {};   // the same texels in 4 bytes, at the levels the LDS-window refine runs on
    uint32_t *pp1 = nullptr, *pp2 = nullptr;                 // column-parity planes of pc at the PatchMatch level (PlanesH::pp1)
    int pp_pitch = 0, pp_pad = 0;
    int16_t *nnf1 = nullptr, *nnf2 = nullptr, *nnf_tmp = nullptr, *nnf_tmp2 = nullptr;
    float *cost1 = nullptr, *cost2 = nullptr;
    float *spec1 = nullptr, *spec2 = nullptr;   // evaluation cache of the sweeps (PmProblem::spec / scand): four direction planes each
    int32_t *scand1 = nullptr, *scand2 = nullptr;
    uint32_t *wl1 = nullptr, *wl2 = nullptr;    // work lists of the speculative sweeps (PmProblem::wl)
    float *restw1 = nullptr, *restw2 = nullptr; // rest-weight planes of the two-phase search (PmProblem::restw), radius 9
    int16_t *seed1 = nullptr, *seed2 = nullptr; // merged form: the field before each direction's sweep (PmProblem::seed), four planes each
    uint32_t* wmf_ws = nullptr;        // work lists + counters of the weighted median
    bool flow_pending = false;         // eppm_compute_begin issued, eppm_compute_end not yet
    float *flow[eppm::kMaxLevels] = {}, *flow_tmp[eppm::kMaxLevels] = {};
    float* c2f_cost9[eppm::kMaxLevels] = {};  // 9 candidates x 4 passes costs per pixel, only for levels whose refine launch is split
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
    // Y'CbCr frames from the host (eppm_yuv_set_images* / eppm_yuv_push_image*).  Frames of depth 8 are staged in d_rgb
    // and h_rgb (a frame is never larger than its RGB form); frames of 16-bit words in allocations of their own, made by the first such call:
    // d_yuv, npairs x both frames, and the pinned h_yuv, double-buffered with h_rgb's events and turn (rgb_cur)
    uint8_t* d_yuv = nullptr;
    uint8_t* h_yuv[2] = {nullptr, nullptr};
    size_t d_yuv_bytes = 0, h_yuv_bytes = 0;
    float* h_flow = nullptr;            // npairs x (u plane | v plane)
    std::vector<float*> out_u, out_v;   // per active pair: where eppm_compute_begin_into sent the planes directly (NULL: staging)
    eppm::HostHold out_hold;            // the registered blocks those planes lie in, in use until eppm_compute_end
    bool have_images = false, have_flow = false;
    // Bidirectional calls (eppm_compute_bidirectional*): their own allocation, made by the first such call -- a forward-only context never
    // has it.  npairs blocks bwd_stride bytes apart, each: the backward flow pyramid, then the host boundary's planar bu | bv (h*w*8 bytes)
    // followed by occ1 and occ2 (h*w bytes each).  The backward path itself runs in slab planes the forward path has finished with
    // (flow_tmp, d_uv, nnf2 / nnf_tmp2, wmf_ws, c2f_cost9); each level's result is copied into bflow.
    char* bwd = nullptr;
    size_t bwd_stride = 0, bwd_bytes = 0, h_bwd_bytes = 0;
    float* bflow[eppm::kMaxLevels] = {};
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
    // Synthetic shutter (eppm_motion_blur*): its own allocation, made by the first such call, for npairs pairs: the
    // packed planes (mbl_plane words per pair), the tile keys (mbl_tplane per pair) and the packed RGB outputs of the host-pointer forms
    // (h*w*3 bytes per pair); h_mbl: pinned copy of those outputs, allocated on the first host-pointer call.
    char* mbl = nullptr;
    size_t mbl_bytes = 0, mbl_plane = 0, mbl_tplane = 0, h_mbl_bytes = 0;
    uint32_t* mbl_packed = nullptr;
    uint64_t* mbl_tkeys = nullptr;
    uint8_t* mbl_rgb = nullptr;
    uint8_t* h_mbl = nullptr;
    // Rolling-shutter correction (eppm_rolling_shutter*): its own allocation, made by the first such call, for npairs
    // pairs: the velocity planes (rsh_plane float2 per pair) and the packed RGB outputs of the host-pointer forms (h*w*3 bytes per pair);
    // h_rsh: pinned copy of those outputs, allocated on the first host-pointer call.
    char* rsh = nullptr;
    size_t rsh_bytes = 0, rsh_plane = 0, h_rsh_bytes = 0;
    float* rsh_vel = nullptr;
    uint8_t* rsh_rgb = nullptr;
    uint8_t* h_rsh = nullptr;
    // Streaming mode (eppm_set_temporal / eppm_batch_set_temporal): its own allocation, made by the first compute
    // with the mode on: npairs blocks tmp_stride bytes apart, one per slot (the members below are slot 0's).  Level-L planes, unpitched: the
    // two displacement snapshots of the last compute (prev_fwd: the field nnf2flow converted, prev_bwd: the raw backward NNF), the two
    // advected priors, the seeded start as the select kernel left it, and the landing keys of both directions (kTemporalNoKey between
    // launches).  The state is per slot (npairs entries each; a single-pair context has one):
    bool temporal = false;
    std::vector<uint8_t> tmp_snap;      // the snapshots hold the last compute's pair of this slot's clip, and no frame has been pushed since
    std::vector<uint8_t> tmp_valid;     // armed by a push that found such snapshots: the next compute starts the slot from their prior
    std::vector<uint8_t> tmp_seeded;    // the slot's last compute started from a prior: prior*, nnf_init*, cost_init* are its planes
    std::vector<uint8_t> tmp_cut;       // the slot's image 2 is the first frame of another clip: its pair leaves no snapshot
    char* tmp = nullptr;
    size_t tmp_bytes = 0, tmp_stride = 0;
    int16_t *prev_fwd = nullptr, *prev_bwd = nullptr, *prior1 = nullptr, *prior2 = nullptr, *nnf_init1 = nullptr, *nnf_init2 = nullptr;
    float *cost_init1 = nullptr, *cost_init2 = nullptr;
    int32_t* tmp_keys = nullptr;        // 2 x W[L]*H[L]
    // every slot starts a new clip (set_images*, the mode switched off)
    void tmp_drop() { std::fill(tmp_valid.begin(), tmp_valid.end(), 0); std::fill(tmp_snap.begin(), tmp_snap.end(), 0); std::fill(tmp_cut.begin(), tmp_cut.end(), 0); }
    int timing = 0;                     // 0 off, 1 every stage, 2 only the dominant kernel (the candidate refine)
    std::vector<StageEv> ev;
    std::vector<StageEv> ev_prep;
    std::vector<hipEvent_t> ev_pool;    // events are created once and reused: no hipEventCreate in a steady-state step
    eppm::Batch bt() const { return eppm::Batch{n_active, stride}; }
    template <class T> T* of_pair(T* p, int k) const { return (T*)((char*)p + (size_t)k * stride); }
    template <class T> T* of_bwd_pair(T* p, int k) const { return (T*)((char*)p + (size_t)k * bwd_stride); }      // ... of the backward block
};

static inline eppm::PlanesH planes(const eppm_ctx* c, int l, bool swap)
{
    eppm::PlanesH p;
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

// ---- stage timing: a pair of pooled events per stage, on the context's stream ----
static inline hipEvent_t pool_event(eppm_ctx* c)
{
    hipEvent_t e = nullptr;
    if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
}
static inline bool stage_on(const eppm_ctx* c, bool dominant) { return c->timing == 1 || (c->timing == 2 && dominant); }
static inline void stage_begin(eppm_ctx* c, std::vector<StageEv>& v, const char* name, bool dominant = false)
{
    if (!stage_on(c, dominant)) return;
    StageEv e;
    e.name = name;
    e.a = pool_event(c);
    e.b = pool_event(c);
    (void)hipEventRecord(e.a, c->stream);
    v.push_back(e);
}
static inline void stage_end(eppm_ctx* c, std::vector<StageEv>& v, bool dominant = false)
{
    if (!stage_on(c, dominant)) return;
    (void)hipEventRecord(v.back().b, c->stream);
}
// closes entry `idx` (stages opened after it have been closed: a stage inside a stage)
static inline void stage_end_at(eppm_ctx* c, std::vector<StageEv>& v, size_t idx)
{
    if (!stage_on(c, false)) return;
    (void)hipEventRecord(v[idx].b, c->stream);
}
static inline void clear_events(eppm_ctx* c, std::vector<StageEv>& v)
{
    for (auto& e : v) { c->ev_pool.push_back(e.a); c->ev_pool.push_back(e.b); }
    v.clear();
}

// ---- allocation ----
// Lays planes out in one block at 256-byte aligned offsets: plane() while `off` grows, then alloc() of the final size
struct EPPM_HIDDEN Carve {
    struct Fix { void** dst; size_t off; };
    std::vector<Fix> fix;
    size_t off = 0;
    template <class T> void plane(T** dst, size_t bytes) { fix.push_back(Fix{(void**)dst, off}); off = (off + bytes + 255) & ~(size_t)255; }
    // `bytes` of device memory through the block cache (*held: the size, for cache_free) and every plane's pointer into its start
    int alloc(char** base, size_t* held, size_t bytes, int device, const char* what) const
    {
        const hipError_t e = cache_alloc((void**)base, bytes, false, device);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *base = nullptr;
            return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (%s) failed: %s", bytes, what, hipGetErrorString(e));
        }
        *held = bytes;
        for (const Fix& f : fix) *f.dst = *base + f.off;
        return EPPM_OK;
    }
};

// a pinned buffer that is allocated by its first use (*held: the size, for cache_free)
template <class T> static inline hipError_t pinned_lazy(T** p, size_t* held, size_t bytes, int device)
{
    if (*p) return hipSuccess;
    *held = bytes;
    return cache_alloc((void**)p, bytes, true, device);
}

// h rows of `row` bytes between images whose rows are dst_stride / src_stride bytes apart
static inline void copy_rows(uint8_t* dst, size_t dst_stride, const uint8_t* src, size_t src_stride, size_t row, int h)
{
    if (dst_stride == row && src_stride == row) { memcpy(dst, src, row * h); return; }
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * dst_stride, src + (size_t)y * src_stride, row);
}
