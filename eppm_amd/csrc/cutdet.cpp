// cutdet.cpp -- scene-cut detection from the bidirectional flow: eppm_cutdet (a stage object, stage_object.h), its
// step on a context's pairs or on caller planes (the kernels: k_cutdet.hip), the synchronous getters, and the host form eppm_cutdet_host.  The host form shares cutdet.h's
// arithmetic with the kernels.
#include "stage_object.h"
#include "cutdet.h"

using namespace eppm;

static_assert(sizeof(CutRecord) == sizeof(eppm_cut_stats) && sizeof(CutRecord) == 96 && sizeof(CutRecord) <= kCutRecordStride, "the record is eppm_cut_stats");
static_assert(offsetof(CutRecord, cut) == offsetof(eppm_cut_stats, cut) && offsetof(CutRecord, sad) == offsetof(eppm_cut_stats, sad), "the record is eppm_cut_stats");
static_assert(kCutSums * 4 <= kCutSlabBytes, "a slab holds the ten sums");

struct eppm_cutdet : StageObject {      // mem: nslots records 128 bytes apart | nslots blocks of slabs `slab_stride` bytes apart
    int lost_permille = 0;
    int64_t r16 = -1;
    int tiles_x = 0, tiles_y = 0;
    size_t off_slabs = 0, slab_stride = 0;
    std::vector<uint8_t> stepped;       // per slot: it has a record
};

namespace {

int cutdet_params(const eppm_cut_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (p->lost_permille < 0 || p->lost_permille > 1000) return set_err(EPPM_ERR_ARG, "%s: lost_permille %d outside [0, 1000]", what, p->lost_permille);
    if (!cut_params_ok(p->lost_permille, p->residual_max)) return set_err(EPPM_ERR_ARG, "%s: residual_max must be negative (off) or lie in [0, 255]", what);
    return EPPM_OK;
}

int size_check(int h, int w, const char* what)
{
    if (!cut_size_ok(h, w)) return set_err(EPPM_ERR_ARG, "%s: size %dx%d out of range (w, h <= %d, h*w <= 2^26)", what, w, h, kCutMaxDim);
    return EPPM_OK;
}

}  // namespace

extern "C" int eppm_cutdet_default_params(eppm_cut_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_cutdet_default_params: NULL");
    p->lost_permille = 530;      // the geometric mean of the measured shares
    p->residual_max = -1.0f;
    return EPPM_OK;
}

static int cutdet_new(int device, int h, int w, int nslots, const eppm_cut_params* in, eppm_cutdet** out)
{
    eppm_cut_params def;
    eppm_cutdet_default_params(&def);
    const eppm_cut_params* p = in ? in : &def;
    CHK(cutdet_params(p, "eppm_cutdet_create"));
    CHK(size_check(h, w, "eppm_cutdet_create"));
    eppm_cutdet* f = new eppm_cutdet;
    f->noun = "detector";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->lost_permille = p->lost_permille; f->r16 = cut_r16(p->residual_max);
    f->tiles_x = (w + kCutTileW - 1) / kCutTileW;
    f->tiles_y = (h + kCutTileH - 1) / kCutTileH;
    f->off_slabs = up256((size_t)nslots * kCutRecordStride);
    f->slab_stride = up256((size_t)f->tiles_x * f->tiles_y * kCutSlabBytes);
    f->bytes = f->off_slabs + f->slab_stride * nslots;
    // the records start as zeros: a slot without a step reports no cut
    const int rc = stage_open(f, "eppm_cutdet_create", [f] { return hipMemsetAsync(f->mem, 0, f->off_slabs, nullptr); });
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->stepped.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_cutdet_create(eppm_ctx* ctx, const eppm_cut_params* in, eppm_cutdet** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_cutdet_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return cutdet_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_cutdet_create_size(int h, int w, int nslots, int device, const eppm_cut_params* in, eppm_cutdet** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_cutdet_create_size: NULL argument");
    *out = nullptr;
    return cutdet_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_cutdet_destroy(eppm_cutdet* f)
{
    if (!f) return EPPM_OK;
    stage_close(f);
    delete f;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the other members are filled in here).  timing: the
// context whose stage-timing entries receive the stage, or NULL
static int step_on(eppm_cutdet* f, CutArgs& in, int slot0, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.off_slabs = f->off_slabs; in.slab_stride = f->slab_stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.tiles_x = f->tiles_x; in.tiles_y = f->tiles_y;
    in.lost_permille = f->lost_permille; in.r16 = f->r16;
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "cutdet");
        launch_cutdet_accumulate(in, s);
        launch_cutdet_finish(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) f->stepped[k] = 1;
    return EPPM_OK;
}

extern "C" int eppm_cutdet_step(eppm_cutdet* f, eppm_ctx* ctx)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_cutdet_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_cutdet_step", &c, &s));
    CutArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ1 = c.occ1; in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return step_on(f, in, 0, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_cutdet_step_frames(eppm_cutdet* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                                       const uint8_t* d_occ1, const uint8_t* d_occ2)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow_bwd || !d_occ1 || !d_occ2) return set_err(EPPM_ERR_ARG, "eppm_cutdet_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_cutdet_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_cutdet_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_cutdet_step_frames", [&](hipStream_t s) {
        CutArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.bwd = (const float*)d_flow_bwd; in.occ1 = d_occ1; in.occ2 = d_occ2;
        in.n = 1;
        return step_on(f, in, slot, s, nullptr);
    });
}

extern "C" int eppm_cutdet_get(eppm_cutdet* f, int slot, eppm_cut_stats* stats)
{
    if (!f || !stats) return set_err(EPPM_ERR_ARG, "eppm_cutdet_get: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_cutdet_get"));
    if (!f->stepped[slot]) return set_err(EPPM_ERR_STATE, "eppm_cutdet_get: slot %d has not been stepped", slot);
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(stats, f->mem + (size_t)slot * kCutRecordStride, sizeof *stats, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_cutdet_cuts(eppm_cutdet* f, int n, uint8_t* cut)
{
    if (!f || !cut) return set_err(EPPM_ERR_ARG, "eppm_cutdet_cuts: NULL argument");
    if (n < 1 || n > f->nslots) return set_err(EPPM_ERR_ARG, "eppm_cutdet_cuts: %d slots, the detector has %d", n, f->nslots);
    CHK(stage_wait(f));
    std::vector<char> rec((size_t)n * kCutRecordStride);
    HIPCHK(hipMemcpy(rec.data(), f->mem, rec.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++) {
        CutRecord r;
        memcpy(&r, rec.data() + (size_t)k * kCutRecordStride, sizeof r);
        cut[k] = (f->stepped[k] && r.cut) ? 1 : 0;
    }
    return EPPM_OK;
}

// ---- host form: the same step as a sequential loop ----
extern "C" int eppm_cutdet_host(const eppm_cut_params* p, const uint8_t* rgb1, const uint8_t* rgb2, const float* bu, const float* bv,
                                const uint8_t* occ1, const uint8_t* occ2, int h, int w, eppm_cut_stats* stats)
{
    CHK(cutdet_params(p, "eppm_cutdet_host"));
    if (!rgb1 || !rgb2 || !bu || !bv || !occ1 || !occ2 || !stats) return set_err(EPPM_ERR_ARG, "eppm_cutdet_host: NULL argument");
    CHK(size_check(h, w, "eppm_cutdet_host"));
    auto word = [](const uint8_t* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16; };
    auto P1 = [rgb1, w, word](int x, int y) { return word(rgb1 + ((size_t)y * w + x) * 3); };
    int64_t s[kCutSums] = {};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            cut_pixel(s, x, y, occ1[i], word(rgb2 + 3 * i), bu[i], bv[i], occ2[i], h, w, P1);
        }
    CutRecord r;
    cut_record(&r, s, (int64_t)h * w, p->lost_permille, cut_r16(p->residual_max));
    memcpy(stats, &r, sizeof r);
    return EPPM_OK;
}
