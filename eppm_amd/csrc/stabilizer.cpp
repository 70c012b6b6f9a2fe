// stabilizer.cpp -- global camera motion and video stabilisation: eppm_stab (a stage object, stage_object.h), its step on a
// context's pairs or on caller planes (the kernels: k_gmotion.hip), the synchronous calls, and the host forms eppm_gmotion_fit_host / eppm_stab_update_host /
// eppm_stab_warp_host.  The host forms share gmotion.h's arithmetic with the kernels.
#include "stage_object.h"
#include "gmotion.h"

using namespace eppm;

static_assert(sizeof(GmModel) == 96 && sizeof(GmState) == 144, "the model and the state fill 240 of their 256 bytes");
static_assert(kGmSums * 8 <= kGmSlabBytes, "a slab holds the twelve sums");

struct eppm_stab : StageObject {        // mem: nslots blocks `stride` bytes apart: slabs | model, state (256 B) | out (h*w RGBA words) | mask (h*w bytes)
    float tau = 0.0f, tau2 = 0.0f, smooth = 0.0f;
    int iters = 0;
    int tiles_x = 0, tiles_y = 0;
    size_t stride = 0, off_model = 0, off_out = 0, off_mask = 0;
    std::vector<uint8_t> empty, stepped;    // per slot: it has no path (its state counts as the identity) / it has an output, a mask and a model
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

int slot_check(const eppm_stab* f, int slot, bool need_step, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
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
    eppm_stab* f = new eppm_stab;
    f->noun = "stabiliser";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->tau = p->tau; f->tau2 = p->tau * p->tau; f->iters = p->iters; f->smooth = p->smooth;
    f->tiles_x = (w + kGmTileW - 1) / kGmTileW;
    f->tiles_y = (h + kGmTileH - 1) / kGmTileH;
    f->off_model = up256((size_t)f->tiles_x * f->tiles_y * kGmSlabBytes);
    f->off_out = f->off_model + 256;
    f->off_mask = f->off_out + f->px() * 4;
    f->stride = up256(f->off_mask + f->px());
    f->bytes = f->stride * nslots;
    const int rc = stage_open(f, "eppm_stab_create");
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->empty.assign(nslots, 1);
    f->stepped.assign(nslots, 0);
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
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_stab_reset(eppm_stab* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_stab_reset: NULL stabiliser");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_stab_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1, f->stepped[k] = 0;
    return EPPM_OK;
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

// what a stabiliser reads of a context: image 2, the forward flow and occ1 of every active pair
StabArgs stab_ctx_args(const CtxPlanes& c)
{
    StabArgs in{};
    in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.fwd = c.fwd; in.fwd_stride = c.fwd_stride;
    in.occ1 = c.occ1; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return in;
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
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "stab_fit");
        for (in.pass = 0; in.pass < f->iters; in.pass++) {
            launch_gmotion_accumulate(in, s);
            launch_gmotion_solve(in, s);
        }
    }
    {
        StageTimer t(timing, "stab_warp");
        launch_stab_warp(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) f->empty[k] = 0, f->stepped[k] = 1;
    return EPPM_OK;
}

extern "C" int eppm_stab_step(eppm_stab* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_stab_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_stab_step", &c, &s));
    StabArgs in = stab_ctx_args(c);
    return stab_step_on(f, in, 0, cut, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_stab_step_frames(eppm_stab* f, int slot, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow, const uint8_t* d_occ1, int cut)
{
    if (!f || !d_rgba2 || !d_flow || !d_occ1) return set_err(EPPM_ERR_ARG, "eppm_stab_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_stab_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_stab_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_stab_step_frames", [&](hipStream_t s) {
        StabArgs in{};
        in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.fwd = (const float*)d_flow; in.occ1 = d_occ1;
        in.n = 1;
        const uint8_t c = cut != 0;
        return stab_step_on(f, in, slot, &c, s, nullptr);
    });
}

extern "C" int eppm_stab_get(eppm_stab* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_stab_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_stab_get: row_stride %zu < 3*w", row_stride);
    return stage_get_rgb(f, f->out(slot), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_stab_get_device(eppm_stab* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_stab_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_stab_get_device: bad pitch %zu", pitch);
    return stage_get_rgba_device(f, f->out(slot), f->h, f->w, d_rgba, pitch);
}

extern "C" int eppm_stab_get_mask(eppm_stab* f, int slot, uint8_t* mask)
{
    if (!f || !mask) return set_err(EPPM_ERR_ARG, "eppm_stab_get_mask: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_mask"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(mask, f->mask(slot), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_stab_get_model(eppm_stab* f, int slot, eppm_gmotion_model* model)
{
    if (!f || !model) return set_err(EPPM_ERR_ARG, "eppm_stab_get_model: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_stab_get_model"));
    CHK(stage_wait(f));
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
        CHK(stage_wait(f));
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
    CHK(stage_wait(f));
    GmState st;
    gm_identity(&st);
    for (int k = 0; k < 6; k++) st.c[k] = path[k], st.s[k] = path[6 + k], st.wf[k] = 0.0f;
    st.pad[0] = st.pad[1] = 0;
    HIPCHK(hipMemcpy(f->state(slot), &st, sizeof st, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
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
