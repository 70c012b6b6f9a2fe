// stabilizer.cpp -- global camera motion and video stabilisation: eppm_stab, its one allocation, its step on a
// context's pairs (the kernels: k_gmotion.hip), the synchronous calls, and the host forms eppm_gmotion_fit_host / eppm_stab_update_host /
// eppm_stab_warp_host.  The host forms share gmotion.h's arithmetic with the kernels.
#include "api_internal.h"
#include "gmotion.h"

using namespace eppm;

static_assert(sizeof(GmModel) == 96 && sizeof(GmState) == 144, "the model and the state fill 240 of their 256 bytes");
static_assert(kGmSums * 8 <= kGmSlabBytes, "a slab holds the twelve sums");

struct eppm_stab {
    int device = 0, h = 0, w = 0, nslots = 0;
    float tau = 0.0f, tau2 = 0.0f, smooth = 0.0f;
    int iters = 0;
    int tiles_x = 0, tiles_y = 0;
    char* mem = nullptr;                // nslots blocks `stride` bytes apart: slabs | model, state (256 B) | out (h*w RGBA words) | mask (h*w bytes)
    size_t bytes = 0, stride = 0, off_model = 0, off_out = 0, off_mask = 0;
    std::vector<uint8_t> empty, stepped;    // per slot: it has no path (its state counts as the identity) / it has an output, a mask and a model
    hipEvent_t done = nullptr;          // recorded after every step: the synchronous calls wait for it
    hipStream_t last = nullptr;         // the stream of the last step: a step on another stream waits for `done` first
    size_t px() const { return (size_t)h * w; }
    char* block(int slot) const { return mem + (size_t)slot * stride; }
    GmModel* model(int slot) const { return (GmModel*)(block(slot) + off_model); }
    GmState* state(int slot) const { return (GmState*)(block(slot) + off_model + sizeof(GmModel)); }
    uint32_t* out(int slot) const { return (uint32_t*)(block(slot) + off_out); }
    uint8_t* mask(int slot) const { return (uint8_t*)(block(slot) + off_mask); }
};

namespace {

int stab_params(const eppm_stab_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->tau > 0.0f && p->tau <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: tau must be finite and > 0", what);
    if (p->iters < 1 || p->iters > kGmMaxIters) return set_err(EPPM_ERR_ARG, "%s: iters %d outside [1, %d]", what, p->iters, kGmMaxIters);
    if (!(p->smooth >= 0.0f && p->smooth <= 1.0f)) return set_err(EPPM_ERR_ARG, "%s: smooth must lie in [0, 1]", what);
    return EPPM_OK;
}

int size_check(int h, int w, const char* what)
{
    if (!gm_size_ok(h, w)) return set_err(EPPM_ERR_ARG, "%s: size %dx%d out of range (w, h <= %d, h*w <= 2^26)", what, w, h, kGmMaxDim);
    return EPPM_OK;
}

// the stabiliser's last step is complete (the synchronous calls read and write its planes on the null stream)
int wait(eppm_stab* f)
{
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipEventSynchronize(f->done));
    return EPPM_OK;
}

int slot_check(const eppm_stab* f, int slot, bool need_step, const char* what)
{
    if (slot < 0 || slot >= f->nslots) return set_err(EPPM_ERR_ARG, "%s: slot %d, the stabiliser has %d", what, slot, f->nslots);
    if (need_step && !f->stepped[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has not been stepped", what, slot);
    return EPPM_OK;
}

void model_out(eppm_gmotion_model* o, const GmModel& m)
{
    for (int k = 0; k < 6; k++) o->p[k] = m.p[k];
    o->n_valid = m.n_valid; o->n_inliers = m.n_inliers; o->valid = m.valid; o->passes = m.passes;
}

}  // namespace

extern "C" int eppm_stab_default_params(eppm_stab_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_stab_default_params: NULL");
    p->tau = 1.0f;
    p->iters = 3;
    p->smooth = 0.9f;
    return EPPM_OK;
}

static int stab_new(int device, int h, int w, int nslots, const eppm_stab_params* in, eppm_stab** out)
{
    eppm_stab_params def;
    eppm_stab_default_params(&def);
    const eppm_stab_params* p = in ? in : &def;
    CHK(stab_params(p, "eppm_stab_create"));
    CHK(size_check(h, w, "eppm_stab_create"));
    if (nslots < 1 || nslots > kTemporalMaxSlots) return set_err(EPPM_ERR_ARG, "eppm_stab_create: %d slots outside [1, %d]", nslots, kTemporalMaxSlots);
    HIPCHK(hipSetDevice(device));
    eppm_stab* f = new eppm_stab;
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->tau = p->tau; f->tau2 = p->tau * p->tau; f->iters = p->iters; f->smooth = p->smooth;
    f->tiles_x = (w + kGmTileW - 1) / kGmTileW;
    f->tiles_y = (h + kGmTileH - 1) / kGmTileH;
    f->off_model = ((size_t)f->tiles_x * f->tiles_y * kGmSlabBytes + 255) & ~(size_t)255;
    f->off_out = f->off_model + 256;
    f->off_mask = f->off_out + f->px() * 4;
    f->stride = (f->off_mask + f->px() + 255) & ~(size_t)255;
    f->bytes = f->stride * nslots;
    f->empty.assign(nslots, 1);
    f->stepped.assign(nslots, 0);
    hipError_t e = cache_alloc((void**)&f->mem, f->bytes, false, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const size_t bytes = f->bytes;
        delete f;
        return set_err(EPPM_ERR_HIP, "hipMalloc of %zu bytes (stabiliser) failed: %s", bytes, hipGetErrorString(e));
    }
    e = hipEventCreateWithFlags(&f->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(f->done, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (f->done) (void)hipEventDestroy(f->done);
        cache_free(f->mem, f->bytes, false, device);
        delete f;
        return set_err(EPPM_ERR_HIP, "eppm_stab_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_stab_create(eppm_ctx* ctx, const eppm_stab_params* in, eppm_stab** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_stab_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return stab_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_stab_create_size(int h, int w, int nslots, int device, const eppm_stab_params* in, eppm_stab** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_stab_create_size: NULL argument");
    *out = nullptr;
    return stab_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_stab_destroy(eppm_stab* f)
{
    if (!f) return EPPM_OK;
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->done);
    (void)hipEventDestroy(f->done);
    cache_free(f->mem, f->bytes, false, f->device);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_stab_reset(eppm_stab* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_stab_reset: NULL stabiliser");
    if (slot >= f->nslots) return set_err(EPPM_ERR_ARG, "eppm_stab_reset: slot %d, the stabiliser has %d", slot, f->nslots);
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1, f->stepped[k] = 0;
    return EPPM_OK;
}

int stab_device(const eppm_stab* f, int* h, int* w, int* nslots)
{
    *h = f->h;
    *w = f->w;
    *nslots = f->nslots;
    return f->device;
}

const uint8_t* stab_mask_device(const eppm_stab* f, size_t* slot_stride)
{
    *slot_stride = f->stride;
    return f->mask(0);
}

const char* stab_model_device(const eppm_stab* f, size_t* slot_stride)
{
    *slot_stride = f->stride;
    return (const char*)f->model(0);
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the other members are filled in here); cut: NULL or one
// flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
int stab_step_on(eppm_stab* f, StabArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride; in.off_model = f->off_model; in.off_out = f->off_out; in.off_mask = f->off_mask;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.tiles_x = f->tiles_x; in.tiles_y = f->tiles_y;
    in.iters = f->iters; in.tau2 = f->tau2; in.smooth = f->smooth;
    memset(in.empty, 0, sizeof(in.empty));
    memset(in.cut, 0, sizeof(in.cut));
    for (int k = slot0; k < slot0 + in.n; k++) {
        const uint32_t bit = 1u << (k & 31);
        if (f->empty[k]) in.empty[k >> 5] |= bit;
        if (cut && cut[k - slot0]) in.cut[k >> 5] |= bit;
    }
    if (s != f->last) HIPCHK(hipStreamWaitEvent(s, f->done, 0));
    if (timing) ctx_stage_begin(timing, "stab_fit");
    for (in.pass = 0; in.pass < f->iters; in.pass++) {
        launch_gmotion_accumulate(in, s);
        launch_gmotion_solve(in, s);
    }
    if (timing) ctx_stage_end(timing);
    if (timing) ctx_stage_begin(timing, "stab_warp");
    launch_stab_warp(in, s);
    if (timing) ctx_stage_end(timing);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(f->done, s));
    f->last = s;
    for (int k = slot0; k < slot0 + in.n; k++) f->empty[k] = 0, f->stepped[k] = 1;
    return EPPM_OK;
}

extern "C" int eppm_stab_step(eppm_stab* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_stab_step: NULL argument");
    StabArgs in{};
    hipStream_t s;
    CHK(ctx_stab_inputs(ctx, f->h, f->w, f->device, f->nslots, "eppm_stab_step", &in, &s));
    return stab_step_on(f, in, 0, cut, s, ctx);
}

extern "C" int eppm_stab_get(eppm_stab* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_stab_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_stab_get: row_stride %zu < 3*w", row_stride);
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

extern "C" int eppm_stab_get_device(eppm_stab* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_stab_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_device"));
    if (pitch < (size_t)f->w * 4 || (pitch & 3)) return set_err(EPPM_ERR_ARG, "eppm_stab_get_device: bad pitch %zu", pitch);
    HIPCHK(hipSetDevice(f->device));
    // on the stream of the last step, behind it; the next step on any stream waits for the copy
    HIPCHK(hipMemcpy2DAsync(d_rgba, pitch, f->out(slot), (size_t)f->w * 4, (size_t)f->w * 4, f->h, hipMemcpyDeviceToDevice, f->last));
    HIPCHK(hipEventRecord(f->done, f->last));
    return EPPM_OK;
}

extern "C" int eppm_stab_get_mask(eppm_stab* f, int slot, uint8_t* mask)
{
    if (!f || !mask) return set_err(EPPM_ERR_ARG, "eppm_stab_get_mask: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_mask"));
    CHK(wait(f));
    HIPCHK(hipMemcpy(mask, f->mask(slot), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_stab_get_model(eppm_stab* f, int slot, eppm_gmotion_model* model)
{
    if (!f || !model) return set_err(EPPM_ERR_ARG, "eppm_stab_get_model: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_model"));
    CHK(wait(f));
    GmModel m;
    HIPCHK(hipMemcpy(&m, f->model(slot), sizeof m, hipMemcpyDeviceToHost));
    model_out(model, m);
    return EPPM_OK;
}

extern "C" int eppm_stab_get_path(eppm_stab* f, int slot, double* path, int64_t* frames, int64_t* invalid_steps)
{
    if (!f || !path) return set_err(EPPM_ERR_ARG, "eppm_stab_get_path: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_stab_get_path"));
    GmState st;
    if (f->empty[slot]) gm_identity(&st);
    else {
        CHK(wait(f));
        HIPCHK(hipMemcpy(&st, f->state(slot), sizeof st, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < 6; k++) path[k] = st.c[k], path[6 + k] = st.s[k];
    if (frames) *frames = st.frames;
    if (invalid_steps) *invalid_steps = st.invalid_steps;
    return EPPM_OK;
}

extern "C" int eppm_stab_set_path(eppm_stab* f, int slot, const double* path)
{
    if (!f || !path) return set_err(EPPM_ERR_ARG, "eppm_stab_set_path: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_stab_set_path"));
    CHK(wait(f));
    GmState st;
    gm_identity(&st);
    for (int k = 0; k < 6; k++) st.c[k] = path[k], st.s[k] = path[6 + k], st.wf[k] = 0.0f;
    st.pad[0] = st.pad[1] = 0;
    HIPCHK(hipMemcpy(f->state(slot), &st, sizeof st, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipEventRecord(f->done, nullptr));
    f->last = nullptr;
    f->empty[slot] = 0;
    return EPPM_OK;
}

// ---- host forms: the same step as sequential loops ----
extern "C" int eppm_gmotion_fit_host(const eppm_stab_params* p, const float* u, const float* v, const uint8_t* occ1, int h, int w,
                                     eppm_gmotion_model* model, uint8_t* mask)
{
    CHK(stab_params(p, "eppm_gmotion_fit_host"));
    if (!u || !v || !occ1 || !model) return set_err(EPPM_ERR_ARG, "eppm_gmotion_fit_host: NULL argument");
    CHK(size_check(h, w, "eppm_gmotion_fit_host"));
    const float tau2 = p->tau * p->tau;
    GmModel m{};
    for (int pass = 0; pass < p->iters; pass++) {
        if (pass > 0 && !m.valid) break;
        int64_t s[kGmSums] = {};
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const int X = gm_X(x, w), Y = gm_Y(y, h);
                if (gm_valid(u[i], v[i], occ1[i]) && (pass == 0 || gm_inlier(u[i], v[i], X, Y, m.pf, tau2))) gm_accumulate(s, X, Y, u[i], v[i]);
            }
        gm_model_from_sums(&m, s, pass);
    }
    model_out(model, m);
    if (mask)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                mask[i] = gm_mask(u[i], v[i], occ1[i], gm_X(x, w), gm_Y(y, h), m, tau2);
            }
    return EPPM_OK;
}

extern "C" int eppm_stab_update_host(const eppm_stab_params* p, double* path, int64_t* counts, const eppm_gmotion_model* model, int cut, float* wf)
{
    CHK(stab_params(p, "eppm_stab_update_host"));
    if (!path || !model || !wf) return set_err(EPPM_ERR_ARG, "eppm_stab_update_host: NULL argument");
    GmState st;
    for (int k = 0; k < 6; k++) st.c[k] = path[k], st.s[k] = path[6 + k];
    st.frames = counts ? counts[0] : 0;
    st.invalid_steps = counts ? counts[1] : 0;
    gm_update(&st, model->p, model->valid != 0, p->smooth, false, cut != 0);
    for (int k = 0; k < 6; k++) path[k] = st.c[k], path[6 + k] = st.s[k], wf[k] = st.wf[k];
    if (counts) counts[0] = st.frames, counts[1] = st.invalid_steps;
    return EPPM_OK;
}

extern "C" int eppm_stab_warp_host(const float* wf, const uint8_t* rgb2, int h, int w, uint8_t* rgb_out)
{
    if (!wf || !rgb2 || !rgb_out) return set_err(EPPM_ERR_ARG, "eppm_stab_warp_host: NULL argument");
    if (rgb2 == rgb_out) return set_err(EPPM_ERR_ARG, "eppm_stab_warp_host: the warp gathers, rgb_out must not be rgb2");
    CHK(size_check(h, w, "eppm_stab_warp_host"));
    auto P = [rgb2, w](int x, int y) {
        const uint8_t* q = rgb2 + ((size_t)y * w + x) * 3;
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t o = gm_warp_pixel(x, y, wf, h, w, P);
            uint8_t* q = rgb_out + ((size_t)y * w + x) * 3;
            q[0] = (uint8_t)o; q[1] = (uint8_t)(o >> 8); q[2] = (uint8_t)(o >> 16);
        }
    return EPPM_OK;
}
