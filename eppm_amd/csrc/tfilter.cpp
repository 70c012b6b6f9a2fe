// tfilter.cpp -- motion-compensated temporal denoising: eppm_tfilter, its one allocation, its step on a context's
// pairs (the kernel: k_tfilter.hip), the synchronous state calls, and the host forms eppm_tfilter_seed_host / eppm_tfilter_step_host.  The
// host form shares tfilter.h's per-pixel arithmetic with the kernel.
#include "api_internal.h"
#include "tfilter.h"

using namespace eppm;

struct eppm_tfilter {
    int device = 0, h = 0, w = 0, nslots = 0;
    float thresh = 0.0f;
    int n_max = 0;
    char* mem = nullptr;                // nslots blocks `stride` bytes apart: state 0 | state 1 (h*w float4 each) | out (h*w RGBA words)
    size_t bytes = 0, stride = 0;
    std::vector<uint8_t> cur, empty;    // per slot: which state is current, and whether the slot has one at all
    hipEvent_t done = nullptr;          // recorded after every step: the synchronous calls wait for it
    hipStream_t last = nullptr;         // the stream of the last step: a step on another stream waits for `done` first
    size_t px() const { return (size_t)h * w; }
    float* state(int slot, int which) const { return (float*)(mem + (size_t)slot * stride + (size_t)which * px() * 16); }
    uint32_t* out(int slot) const { return (uint32_t*)(mem + (size_t)slot * stride + px() * 32); }
};

namespace {

int tfilter_params(const eppm_tfilter_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->thresh >= 0.0f && p->thresh <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: thresh must be finite and >= 0", what);
    if (p->n_max < 1 || p->n_max > 255) return set_err(EPPM_ERR_ARG, "%s: n_max %d outside [1, 255]", what, p->n_max);
    return EPPM_OK;
}

// the filter's last step is complete (the synchronous calls read and write its planes on the null stream)
int wait(eppm_tfilter* f)
{
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipEventSynchronize(f->done));
    return EPPM_OK;
}

int slot_check(const eppm_tfilter* f, int slot, bool need_state, const char* what)
{
    if (slot < 0 || slot >= f->nslots) return set_err(EPPM_ERR_ARG, "%s: slot %d, the filter has %d", what, slot, f->nslots);
    if (need_state && f->empty[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d is empty", what, slot);
    return EPPM_OK;
}

}  // namespace

extern "C" int eppm_tfilter_default_params(eppm_tfilter_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_tfilter_default_params: NULL");
    p->thresh = 40.0f;
    p->n_max = 8;
    return EPPM_OK;
}

static int tfilter_new(int device, int h, int w, int nslots, const eppm_tfilter_params* in, eppm_tfilter** out)
{
    eppm_tfilter_params def;
    eppm_tfilter_default_params(&def);
    const eppm_tfilter_params* p = in ? in : &def;
    CHK(tfilter_params(p, "eppm_tfilter_create"));
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_create: size %dx%d out of range", w, h);
    if (nslots < 1 || nslots > kTemporalMaxSlots) return set_err(EPPM_ERR_ARG, "eppm_tfilter_create: %d slots outside [1, %d]", nslots, kTemporalMaxSlots);
    HIPCHK(hipSetDevice(device));
    eppm_tfilter* f = new eppm_tfilter;
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->thresh = p->thresh; f->n_max = p->n_max;
    f->stride = (f->px() * 36 + 255) & ~(size_t)255;
    f->bytes = f->stride * nslots;
    f->cur.assign(nslots, 0);
    f->empty.assign(nslots, 1);
    hipError_t e = cache_alloc((void**)&f->mem, f->bytes, false, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const size_t bytes = f->bytes;
        delete f;
        return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (temporal filter) failed: %s", bytes, hipGetErrorString(e));
    }
    e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(f->done, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (f->done) (void)hipEventDestroy(f->done);
        cache_free(f->mem, f->bytes, false, device);
        delete f;
        return set_err(EPPM_ERR_HIP, "eppm_tfilter_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_tfilter_create(eppm_ctx* ctx, const eppm_tfilter_params* in, eppm_tfilter** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_tfilter_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return tfilter_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_tfilter_create_size(int h, int w, int nslots, int device, const eppm_tfilter_params* in, eppm_tfilter** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_tfilter_create_size: NULL argument");
    *out = nullptr;
    return tfilter_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_tfilter_destroy(eppm_tfilter* f)
{
    if (!f) return EPPM_OK;
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->done);
    (void)hipEventDestroy(f->done);
    cache_free(f->mem, f->bytes, false, f->device);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_tfilter_reset(eppm_tfilter* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_tfilter_reset: NULL filter");
    if (slot >= f->nslots) return set_err(EPPM_ERR_ARG, "eppm_tfilter_reset: slot %d, the filter has %d", slot, f->nslots);
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1;
    return EPPM_OK;
}

int tfilter_device(const eppm_tfilter* f, int* h, int* w, int* nslots)
{
    *h = f->h;
    *w = f->w;
    *nslots = f->nslots;
    return f->device;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the state members are filled in here); cut: NULL or
// one flag per pair.  timing: the context whose stage-timing entries receive the stage, or NULL
int tfilter_step_on(eppm_tfilter* f, TFilterArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.st0 = f->state(0, 0);
    in.st1 = f->state(0, 1);
    in.out = f->out(0);
    in.slot_stride = f->stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.thresh = f->thresh; in.n_max = f->n_max;
    memset(in.cur, 0, sizeof(in.cur));
    memset(in.empty, 0, sizeof(in.empty));
    memset(in.cut, 0, sizeof(in.cut));
    for (int k = slot0; k < slot0 + in.n; k++) {
        const uint32_t bit = 1u << (k & 31);
        if (f->cur[k]) in.cur[k >> 5] |= bit;
        if (f->empty[k]) in.empty[k >> 5] |= bit;
        if (cut && cut[k - slot0]) in.cut[k >> 5] |= bit;
    }
    if (s != f->last) HIPCHK(hipStreamWaitEvent(s, f->done, 0));
    if (timing) ctx_stage_begin(timing, "tfilter_step");
    launch_tfilter_step(in, s);
    if (timing) ctx_stage_end(timing);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(f->done, s));
    f->last = s;
    for (int k = slot0; k < slot0 + in.n; k++) {
        f->cur[k] ^= 1;
        f->empty[k] = 0;
    }
    return EPPM_OK;
}

extern "C" int eppm_tfilter_step(eppm_tfilter* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step: NULL argument");
    TFilterArgs in{};
    hipStream_t s;
    CHK(ctx_tfilter_inputs(ctx, f->h, f->w, f->device, f->nslots, "eppm_tfilter_step", &in, &s));
    return tfilter_step_on(f, in, 0, cut, s, ctx);
}

extern "C" int eppm_tfilter_get(eppm_tfilter* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get: row_stride %zu < 3*w", row_stride);
    CHK(wait(f));
    std::vector<uint32_t> words(f->px());
    HIPCHK(hipMemcpy(words.data(), f->out(slot), f->px() * 4, hipMemcpyDeviceToHost));
    for (int y = 0; y < f->h; y++) {
        uint8_t* o = rgb + (size_t)y * row_stride;
        const uint32_t* q = words.data() + (size_t)y * f->w;
        for (int x = 0; x < f->w; x++) {
            o[3 * x] = (uint8_t)q[x]; o[3 * x + 1] = (uint8_t)(q[x] >> 8); o[3 * x + 2] = (uint8_t)(q[x] >> 16);
        }
    }
    return EPPM_OK;
}

extern "C" int eppm_tfilter_get_device(eppm_tfilter* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get_device"));
    if (pitch < (size_t)f->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(f->device));
    // on the stream of the last step, behind it; the next step on any stream waits for the copy
    HIPCHK(hipMemcpy2DAsync(d_rgba, pitch, f->out(slot), (size_t)f->w * 4, (size_t)f->w * 4, f->h, hipMemcpyDeviceToDevice, f->last));
    HIPCHK(hipEventRecord(f->done, f->last));
    return EPPM_OK;
}

extern "C" int eppm_tfilter_get_state(eppm_tfilter* f, int slot, float* acc)
{
    if (!f || !acc) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_state: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get_state"));
    CHK(wait(f));
    HIPCHK(hipMemcpy(acc, f->state(slot, f->cur[slot]), f->px() * 16, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_tfilter_set_state(eppm_tfilter* f, int slot, const float* acc)
{
    if (!f || !acc) return set_err(EPPM_ERR_ARG, "eppm_tfilter_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_tfilter_set_state"));
    CHK(wait(f));
    std::vector<uint32_t> words(f->px());
    for (size_t i = 0; i < f->px(); i++) words[i] = tfilter_word(TfState{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]});
    HIPCHK(hipMemcpy(f->state(slot, f->cur[slot]), acc, f->px() * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->out(slot), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipEventRecord(f->done, nullptr));
    f->last = nullptr;
    f->empty[slot] = 0;
    return EPPM_OK;
}

// ---- host forms: the same step as a sequential loop ----
extern "C" int eppm_tfilter_seed_host(float* acc, const uint8_t* rgb, int h, int w)
{
    if (!acc || !rgb) return set_err(EPPM_ERR_ARG, "eppm_tfilter_seed_host: NULL argument");
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_seed_host: size %dx%d out of range", w, h);
    for (size_t i = 0; i < (size_t)h * w; i++) {
        const TfState s = tfilter_seed((uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16);
        acc[4 * i] = s.r; acc[4 * i + 1] = s.g; acc[4 * i + 2] = s.b; acc[4 * i + 3] = s.n;
    }
    return EPPM_OK;
}

extern "C" int eppm_tfilter_step_host(const eppm_tfilter_params* p, float* acc_out, uint8_t* rgb_out, const float* acc_in, const uint8_t* rgb2,
                                      const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int cut)
{
    CHK(tfilter_params(p, "eppm_tfilter_step_host"));
    if (!acc_out || !rgb_out || !acc_in || !rgb2 || !bu || !bv || !occ2) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step_host: NULL argument");
    if (acc_out == acc_in) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step_host: the step gathers, acc_out must not be acc_in");
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step_host: size %dx%d out of range", w, h);
    auto A = [acc_in, w](int x, int y) {
        const float* q = acc_in + ((size_t)y * w + x) * 4;
        return TfState{q[0], q[1], q[2], q[3]};
    };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint32_t word = (uint32_t)rgb2[3 * i] | (uint32_t)rgb2[3 * i + 1] << 8 | (uint32_t)rgb2[3 * i + 2] << 16;
            const TfState s = tfilter_step_pixel(x, y, word, bu[i], bv[i], occ2[i], cut != 0, h, w, p->thresh, p->n_max, A);
            acc_out[4 * i] = s.r; acc_out[4 * i + 1] = s.g; acc_out[4 * i + 2] = s.b; acc_out[4 * i + 3] = s.n;
            const uint32_t o = tfilter_word(s);
            rgb_out[3 * i] = (uint8_t)o; rgb_out[3 * i + 1] = (uint8_t)(o >> 8); rgb_out[3 * i + 2] = (uint8_t)(o >> 16);
        }
    return EPPM_OK;
}
