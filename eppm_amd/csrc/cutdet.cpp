// cutdet.cpp -- scene-cut detection from the bidirectional flow: eppm_cutdet, its one allocation, its step on a
// context's pairs (the kernels: k_cutdet.hip), the synchronous getters, and the host form eppm_cutdet_host.  The host form shares cutdet.h's
// arithmetic with the kernels.
#include "api_internal.h"
#include "cutdet.h"

using namespace eppm;

static_assert(sizeof(CutRecord) == sizeof(eppm_cut_stats) && sizeof(CutRecord) == 96 && sizeof(CutRecord) <= kCutRecordStride, "the record is eppm_cut_stats");
static_assert(offsetof(CutRecord, cut) == offsetof(eppm_cut_stats, cut) && offsetof(CutRecord, sad) == offsetof(eppm_cut_stats, sad), "the record is eppm_cut_stats");
static_assert(kCutSums * 4 <= kCutSlabBytes, "a slab holds the ten sums");

struct eppm_cutdet {
    int device = 0, h = 0, w = 0, nslots = 0;
    int lost_permille = 0;
    int64_t r16 = -1;
    int tiles_x = 0, tiles_y = 0;
    char* mem = nullptr;                // nslots records 128 bytes apart | nslots blocks of slabs `slab_stride` bytes apart
    size_t bytes = 0, off_slabs = 0, slab_stride = 0;
    std::vector<uint8_t> stepped;       // per slot: it has a record
    hipEvent_t done = nullptr;          // recorded after every step: the synchronous calls wait for it
    hipStream_t last = nullptr;         // the stream of the last step: a step on another stream waits for `done` first
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

// the detector's last step is complete (the synchronous calls read its records on the null stream)
int wait(eppm_cutdet* f)
{
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipEventSynchronize(f->done));
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
    if (nslots < 1 || nslots > kTemporalMaxSlots) return set_err(EPPM_ERR_ARG, "eppm_cutdet_create: %d slots outside [1, %d]", nslots, kTemporalMaxSlots);
    HIPCHK(hipSetDevice(device));
    eppm_cutdet* f = new eppm_cutdet;
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->lost_permille = p->lost_permille; f->r16 = cut_r16(p->residual_max);
    f->tiles_x = (w + kCutTileW - 1) / kCutTileW;
    f->tiles_y = (h + kCutTileH - 1) / kCutTileH;
    f->off_slabs = ((size_t)nslots * kCutRecordStride + 255) & ~(size_t)255;
    f->slab_stride = ((size_t)f->tiles_x * f->tiles_y * kCutSlabBytes + 255) & ~(size_t)255;
    f->bytes = f->off_slabs + f->slab_stride * nslots;
    f->stepped.assign(nslots, 0);
    hipError_t e = cache_alloc((void**)&f->mem, f->bytes, false, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const size_t bytes = f->bytes;
        delete f;
        return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (cut detector) failed: %s", bytes, hipGetErrorString(e));
    }
    // the records start as zeros: a slot without a step reports no cut
    e = hipMemsetAsync(f->mem, 0, f->off_slabs, nullptr);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(f->done, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (f->done) (void)hipEventDestroy(f->done);
        (void)hipDeviceSynchronize();
        cache_free(f->mem, f->bytes, false, device);
        delete f;
        return set_err(EPPM_ERR_HIP, "eppm_cutdet_create: %s", hipGetErrorString(e));
    }
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
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->done);
    (void)hipEventDestroy(f->done);
    cache_free(f->mem, f->bytes, false, f->device);
    delete f;
    return EPPM_OK;
}

int cutdet_device(const eppm_cutdet* f, int* h, int* w, int* nslots)
{
    *h = f->h;
    *w = f->w;
    *nslots = f->nslots;
    return f->device;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the other members are filled in here).  timing: the
// context whose stage-timing entries receive the stage, or NULL
int cutdet_step_on(eppm_cutdet* f, CutArgs& in, int slot0, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.off_slabs = f->off_slabs; in.slab_stride = f->slab_stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.tiles_x = f->tiles_x; in.tiles_y = f->tiles_y;
    in.lost_permille = f->lost_permille; in.r16 = f->r16;
    if (s != f->last) HIPCHK(hipStreamWaitEvent(s, f->done, 0));
    if (timing) ctx_stage_begin(timing, "cutdet");
    launch_cutdet_accumulate(in, s);
    launch_cutdet_finish(in, s);
    if (timing) ctx_stage_end(timing);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(f->done, s));
    f->last = s;
    for (int k = slot0; k < slot0 + in.n; k++) f->stepped[k] = 1;
    return EPPM_OK;
}

extern "C" int eppm_cutdet_step(eppm_cutdet* f, eppm_ctx* ctx)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_cutdet_step: NULL argument");
    CutArgs in{};
    hipStream_t s;
    CHK(ctx_cutdet_inputs(ctx, f->h, f->w, f->device, f->nslots, "eppm_cutdet_step", &in, &s));
    return cutdet_step_on(f, in, 0, s, ctx);
}

extern "C" int eppm_cutdet_get(eppm_cutdet* f, int slot, eppm_cut_stats* stats)
{
    if (!f || !stats) return set_err(EPPM_ERR_ARG, "eppm_cutdet_get: NULL argument");
    if (slot < 0 || slot >= f->nslots) return set_err(EPPM_ERR_ARG, "eppm_cutdet_get: slot %d, the detector has %d", slot, f->nslots);
    if (!f->stepped[slot]) return set_err(EPPM_ERR_STATE, "eppm_cutdet_get: slot %d has not been stepped", slot);
    CHK(wait(f));
    HIPCHK(hipMemcpy(stats, f->mem + (size_t)slot * kCutRecordStride, sizeof *stats, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_cutdet_cuts(eppm_cutdet* f, int n, uint8_t* cut)
{
    if (!f || !cut) return set_err(EPPM_ERR_ARG, "eppm_cutdet_cuts: NULL argument");
    if (n < 1 || n > f->nslots) return set_err(EPPM_ERR_ARG, "eppm_cutdet_cuts: %d slots, the detector has %d", n, f->nslots);
    CHK(wait(f));
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
