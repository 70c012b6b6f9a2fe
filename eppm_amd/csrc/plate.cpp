// plate.cpp -- background plates: eppm_plate (a stage object, stage_object.h), its private stabiliser, its step
// on a context's pairs or on caller planes (the kernels: k_plate.hip), the synchronous calls, and the host forms eppm_plate_forms_host / eppm_plate_block_host /
// eppm_plate_accumulate_host / eppm_plate_render_host, which are plate.h's sequential code behind argument checks.
#include "stage_object.h"
#include "plate.h"

using namespace eppm;

static_assert(sizeof(PlateRec) == 128 && sizeof(TfState) == 16, "a path record is 128 bytes, a canvas state one float4");

struct eppm_plate : StageObject {       // mem: nslots blocks `stride` bytes apart (PlateArgs' layout), then the scratch of the synchronous calls
    int ch = 0, cw = 0;
    eppm_plate_params prm{};
    eppm_stab* stab = nullptr;          // the private stabiliser whose mask and model the context form uses
    size_t stride = 0, off_b = 0, off_br = 0, off_rec = 0, off_scratch = 0;
    std::vector<uint8_t> empty, stepped, fitted;    // per slot: its canvas has no states / it has forms and a blocked plane / its last step had a fit
    size_t cpx() const { return (size_t)ch * cw; }
    char* block(int slot) const { return mem + (size_t)slot * stride; }
    PlateRec* rec(int slot) const { return (PlateRec*)(block(slot) + off_rec); }
    uint32_t* scratch_words() const { return (uint32_t*)(mem + off_scratch); }
    uint8_t* scratch_bytes() const { return (uint8_t*)(mem + off_scratch + cpx() * 4); }
};

namespace {

int plate_params(const eppm_plate_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->tau > 0.0f && p->tau <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: tau must be finite and > 0", what);
    if (p->iters < 1 || p->iters > kGmMaxIters) return set_err(EPPM_ERR_ARG, "%s: iters %d outside [1, %d]", what, p->iters, kGmMaxIters);
    if (!plate_params_ok(p->margin_x, p->margin_y, p->grow, p->thresh, p->n_max, p->min_count))
        return set_err(EPPM_ERR_ARG, "%s: margins >= 0, grow in [0, %d], thresh finite and >= 0, n_max and min_count in [1, %d]", what, kPlateMaxGrow,
                       kPlateMaxCount);
    return EPPM_OK;
}

int size_check(int h, int w, int mx, int my, const char* what)
{
    if (!plate_size_ok(h, w, mx, my))
        return set_err(EPPM_ERR_ARG, "%s: size %dx%d with margins %d, %d out of range (canvas w, h <= %d, h*w <= 2^26)", what, w, h, mx, my, kGmMaxDim);
    return EPPM_OK;
}

int slot_check(const eppm_plate* f, int slot, bool need_states, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_states && f->empty[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d is empty", what, slot);
    return EPPM_OK;
}

int write_path(eppm_plate* f, int slot, const double* p)
{
    HIPCHK(hipMemcpy(f->rec(slot)->p, p, 6 * sizeof(double), hipMemcpyHostToDevice));
    return EPPM_OK;
}

}  // namespace

extern "C" int eppm_plate_default_params(eppm_plate_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_plate_default_params: NULL");
    p->tau = 1.0f;
    p->iters = 3;
    p->margin_x = p->margin_y = 0;
    p->grow = 2;
    p->accept_invalid = 0;
    p->thresh = 40.0f;
    p->n_max = 64;
    p->min_count = 2;
    return EPPM_OK;
}

static int plate_new(int device, int h, int w, int nslots, const eppm_plate_params* in, eppm_plate** out)
{
    eppm_plate_params def;
    eppm_plate_default_params(&def);
    const eppm_plate_params* p = in ? in : &def;
    CHK(plate_params(p, "eppm_plate_create"));
    CHK(size_check(h, w, p->margin_x, p->margin_y, "eppm_plate_create"));
    eppm_plate* f = new eppm_plate;
    f->noun = "plate";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->ch = h + 2 * p->margin_y; f->cw = w + 2 * p->margin_x;
    f->prm = *p;
    f->off_b = up256(f->cpx() * sizeof(TfState));
    f->off_br = f->off_b + up256(f->px());
    f->off_rec = f->off_br + up256(f->px());
    f->stride = f->off_rec + up256(sizeof(PlateRec));
    f->off_scratch = f->stride * nslots;
    f->bytes = f->off_scratch + up256(f->cpx() * 4) + up256(f->cpx());
    eppm_stab_params sp;
    eppm_stab_default_params(&sp);
    sp.tau = p->tau;
    sp.iters = p->iters;
    int rc = stage_open(f, "eppm_plate_create", [f] {           // every slot's path starts as the identity
        PlateRec r{};
        plate_identity(r.p);
        hipError_t e = hipSuccess;
        for (int k = 0; k < f->nslots && e == hipSuccess; k++) e = hipMemcpy(f->rec(k), &r, sizeof r, hipMemcpyHostToDevice);
        return e;
    });
    if (rc == EPPM_OK) rc = eppm_stab_create_size(h, w, nslots, device, &sp, &f->stab);
    if (rc != EPPM_OK) {
        eppm_plate_destroy(f);
        return rc;
    }
    f->empty.assign(nslots, 1);
    f->stepped.assign(nslots, 0);
    f->fitted.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_plate_create(eppm_ctx* ctx, const eppm_plate_params* in, eppm_plate** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_plate_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return plate_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_plate_create_size(int h, int w, int nslots, int device, const eppm_plate_params* in, eppm_plate** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_plate_create_size: NULL argument");
    *out = nullptr;
    return plate_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_plate_destroy(eppm_plate* f)
{
    if (!f) return EPPM_OK;
    eppm_stab_destroy(f->stab);
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_plate_reset(eppm_plate* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_plate_reset: NULL plate");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_plate_reset"));
    CHK(stage_wait(f));
    double id[6];
    plate_identity(id);
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) {
            CHK(write_path(f, k, id));
            f->empty[k] = 1;
            f->stepped[k] = 0;
            f->fitted[k] = 0;
        }
    CHK(eppm_stab_reset(f->stab, slot));
    return stage_settle(f);
}

extern "C" int eppm_plate_canvas_dims(const eppm_plate* f, int* ch, int* cw)
{
    if (!f || !ch || !cw) return set_err(EPPM_ERR_ARG, "eppm_plate_canvas_dims: NULL argument");
    *ch = f->ch;
    *cw = f->cw;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the other members are filled in here); cut: NULL or one
// flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_plate* f, PlateArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride; in.off_b = f->off_b; in.off_rec = f->off_rec;
    in.h = f->h; in.w = f->w; in.ch = f->ch; in.cw = f->cw; in.mx = f->prm.margin_x; in.my = f->prm.margin_y; in.slot0 = slot0;
    in.grow = f->prm.grow; in.accept_invalid = f->prm.accept_invalid; in.n_max = f->prm.n_max; in.min_count = f->prm.min_count;
    in.thresh = f->prm.thresh;
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "plate_block");
        launch_plate_block(in, s);
    }
    {
        StageTimer t(timing, "plate_accumulate");
        in.phase = 0;
        launch_plate_path(in, s);
        launch_plate_accumulate(in, s);
        in.phase = 1;
        launch_plate_path(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) f->empty[k] = 0, f->stepped[k] = 1, f->fitted[k] = in.model != nullptr;
    return EPPM_OK;
}

extern "C" int eppm_plate_step(eppm_plate* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_plate_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_plate_step", &c, &s));
    PlateArgs in{};
    in.img1 = c.img1; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.n = c.n;
    {
        StageTimer t(ctx, "plate_fit");
        StabArgs sin = stab_ctx_args(c);
        CHK(stab_step_on(f->stab, sin, 0, cut, s, nullptr));
    }
    in.mask = stab_mask_device(f->stab, &in.mask_stride);
    in.model = stab_model_device(f->stab, &in.model_stride);
    return step_on(f, in, 0, cut, s, ctx);
}

// the kernels alone for one slot on caller planes, without a fit, on the launcher stream; path NULL: the slot's own
extern "C" int eppm_plate_step_frames(eppm_plate* f, int slot, const void* d_rgba, size_t pitch, const uint8_t* d_mask, const double* path, int cut)
{
    if (!f || !d_rgba || !d_mask) return set_err(EPPM_ERR_ARG, "eppm_plate_step_frames: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_plate_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_plate_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_plate_step_frames", [&](hipStream_t s) {
        if (path) {
            CHK(stage_wait(f));
            CHK(write_path(f, slot, path));
            CHK(stage_settle(f));
        }
        PlateArgs in{};
        in.img1 = (const uint8_t*)d_rgba; in.img_pitch = pitch;
        in.mask = d_mask;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    });
}

// a render of one slot on stream s into (out, fill); path NULL: the forms of the slot's last step with its blocked plane (mask NULL), or
// of the slot's own path (mask given)
static int render_on(eppm_plate* f, int slot, const uint8_t* img1, size_t pitch, const uint8_t* d_mask, const double* path, uint32_t* out, size_t out_pitch,
                     uint8_t* fill, hipStream_t s, eppm_ctx* timing)
{
    CHK(stage_wait(f));
    PlateRec r;
    HIPCHK(hipMemcpy(&r, f->rec(slot), sizeof r, hipMemcpyDeviceToHost));
    PlateRenderArgs a{};
    if (path || d_mask) {
        float fwd[6];
        a.ok = plate_forms(path ? path : r.p, fwd, a.inv) ? 1 : 0;
    } else {
        a.ok = r.ok;
        for (int k = 0; k < 6; k++) a.inv[k] = r.inv[k];
    }
    a.img1 = img1; a.img_pitch = pitch;
    a.canvas = f->block(slot);
    a.blocked = (const uint8_t*)(f->block(slot) + (d_mask ? f->off_br : f->off_b));
    a.out = out; a.out_pitch = out_pitch; a.fill = fill;
    a.h = f->h; a.w = f->w; a.ch = f->ch; a.cw = f->cw; a.mx = f->prm.margin_x; a.my = f->prm.margin_y; a.min_count = f->prm.min_count;
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "plate_render");
        if (d_mask) {
            PlateArgs b{};
            b.mask = d_mask;
            b.mem = f->mem; b.slot_stride = f->stride; b.off_b = f->off_br;
            b.h = f->h; b.w = f->w; b.n = 1; b.slot0 = slot;
            b.grow = f->prm.grow; b.accept_invalid = f->prm.accept_invalid;
            launch_plate_block(b, s);
        }
        launch_plate_render(a, s);
    }
    CHK(stage_leave(f, s));
    HIPCHK(hipStreamSynchronize(s));
    return EPPM_OK;
}

// the render alone on caller planes against the slot's canvas, on the launcher stream (render_on waits for it itself)
extern "C" int eppm_plate_render_frames(eppm_plate* f, int slot, const void* d_rgba, size_t pitch, const uint8_t* d_mask, const double* path, void* d_rgba_out,
                                        size_t out_pitch, uint8_t* d_fill)
{
    if (!f || !d_rgba || !d_mask || !d_rgba_out || !d_fill) return set_err(EPPM_ERR_ARG, "eppm_plate_render_frames: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_render_frames"));
    if (bad_pitch(pitch, f->w) || bad_pitch(out_pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_plate_render_frames: bad pitch %zu / %zu", pitch, out_pitch);
    return launcher_run(f, "eppm_plate_render_frames", [&](hipStream_t s) {
        return render_on(f, slot, (const uint8_t*)d_rgba, pitch, d_mask, path, (uint32_t*)d_rgba_out, out_pitch, d_fill, s, nullptr);
    }, false);
}

extern "C" int eppm_plate_render(eppm_plate* f, eppm_ctx* ctx, int slot, uint8_t* rgb, size_t row_stride, uint8_t* fill)
{
    if (!f || !ctx || !rgb) return set_err(EPPM_ERR_ARG, "eppm_plate_render: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_render"));
    if (!f->stepped[slot]) return set_err(EPPM_ERR_STATE, "eppm_plate_render: slot %d has not been stepped", slot);
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_plate_render: row_stride %zu < 3*w", row_stride);
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_plate_render", &c, &s));
    if (slot >= c.n) return set_err(EPPM_ERR_ARG, "eppm_plate_render: slot %d, the context has %d active pairs", slot, c.n);
    CHK(render_on(f, slot, c.img1 + (size_t)slot * c.img_stride, c.img_pitch, nullptr, nullptr, f->scratch_words(), (size_t)f->w * 4, f->scratch_bytes(), s, ctx));
    CHK(stage_get_rgb(f, f->scratch_words(), f->h, f->w, rgb, row_stride));
    if (fill) HIPCHK(hipMemcpy(fill, f->scratch_bytes(), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_plate_get(eppm_plate* f, int slot, uint8_t* rgb, size_t row_stride, uint8_t* coverage)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_plate_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_get"));
    if (row_stride < (size_t)f->cw * 3) return set_err(EPPM_ERR_ARG, "eppm_plate_get: row_stride %zu < 3 * canvas width", row_stride);
    CHK(stage_wait(f));
    launch_plate_word(f->block(slot), f->scratch_words(), f->scratch_bytes(), f->ch, f->cw, nullptr);
    HIPCHK(hipGetLastError());
    CHK(stage_get_rgb(f, f->scratch_words(), f->ch, f->cw, rgb, row_stride));
    if (coverage) HIPCHK(hipMemcpy(coverage, f->scratch_bytes(), f->cpx(), hipMemcpyDeviceToHost));
    return stage_settle(f);
}

extern "C" int eppm_plate_get_device(eppm_plate* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_plate_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_get_device"));
    if (bad_pitch(pitch, f->cw)) return set_err(EPPM_ERR_ARG, "eppm_plate_get_device: bad pitch %zu", pitch);
    CHK(stage_wait(f));
    launch_plate_word(f->block(slot), f->scratch_words(), f->scratch_bytes(), f->ch, f->cw, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2D(d_rgba, pitch, f->scratch_words(), (size_t)f->cw * 4, (size_t)f->cw * 4, f->ch, hipMemcpyDeviceToDevice));
    return stage_settle(f);
}

extern "C" int eppm_plate_get_mask(eppm_plate* f, int slot, uint8_t* mask)
{
    if (!f || !mask) return set_err(EPPM_ERR_ARG, "eppm_plate_get_mask: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_get_mask"));
    if (!f->fitted[slot]) return set_err(EPPM_ERR_STATE, "eppm_plate_get_mask: the last step of slot %d had no fit", slot);
    CHK(stage_wait(f));
    return eppm_stab_get_mask(f->stab, slot, mask);
}

extern "C" int eppm_plate_get_path(eppm_plate* f, int slot, double* path)
{
    if (!f || !path) return set_err(EPPM_ERR_ARG, "eppm_plate_get_path: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_plate_get_path"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(path, f->rec(slot)->p, 6 * sizeof(double), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_plate_set_path(eppm_plate* f, int slot, const double* path)
{
    if (!f || !path) return set_err(EPPM_ERR_ARG, "eppm_plate_set_path: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_plate_set_path"));
    CHK(stage_wait(f));
    CHK(write_path(f, slot, path));
    return stage_settle(f);
}

extern "C" int eppm_plate_get_state(eppm_plate* f, int slot, float* state)
{
    if (!f || !state) return set_err(EPPM_ERR_ARG, "eppm_plate_get_state: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_plate_get_state"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(state, f->block(slot), f->cpx() * sizeof(TfState), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_plate_set_state(eppm_plate* f, int slot, const float* state)
{
    if (!f || !state) return set_err(EPPM_ERR_ARG, "eppm_plate_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_plate_set_state"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(f->block(slot), state, f->cpx() * sizeof(TfState), hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->empty[slot] = 0;
    return EPPM_OK;
}

// ---- host forms: plate.h's sequential code ----
extern "C" int eppm_plate_forms_host(const double* path, float* fwd, float* inv, int* ok)
{
    if (!path || !fwd || !inv || !ok) return set_err(EPPM_ERR_ARG, "eppm_plate_forms_host: NULL argument");
    *ok = plate_forms(path, fwd, inv) ? 1 : 0;
    return EPPM_OK;
}

extern "C" int eppm_plate_block_host(const eppm_plate_params* p, const uint8_t* mask, int h, int w, uint8_t* blocked)
{
    CHK(plate_params(p, "eppm_plate_block_host"));
    if (!mask || !blocked) return set_err(EPPM_ERR_ARG, "eppm_plate_block_host: NULL argument");
    if (mask == blocked) return set_err(EPPM_ERR_ARG, "eppm_plate_block_host: the dilation gathers, blocked must not be mask");
    CHK(size_check(h, w, p->margin_x, p->margin_y, "eppm_plate_block_host"));
    plate_block_host(mask, h, w, p->grow, p->accept_invalid != 0, blocked);
    return EPPM_OK;
}

extern "C" int eppm_plate_accumulate_host(const eppm_plate_params* p, const float* fwd, const uint8_t* rgb, const uint8_t* blocked, int h, int w, float* state)
{
    CHK(plate_params(p, "eppm_plate_accumulate_host"));
    if (!fwd || !rgb || !blocked || !state) return set_err(EPPM_ERR_ARG, "eppm_plate_accumulate_host: NULL argument");
    CHK(size_check(h, w, p->margin_x, p->margin_y, "eppm_plate_accumulate_host"));
    plate_accumulate_host(fwd, rgb, blocked, h, w, p->margin_x, p->margin_y, p->thresh, p->n_max, reinterpret_cast<TfState*>(state));
    return EPPM_OK;
}

extern "C" int eppm_plate_render_host(const eppm_plate_params* p, const float* inv, int ok, const uint8_t* rgb, const uint8_t* blocked, int h, int w,
                                      const float* state, uint8_t* rgb_out, uint8_t* fill)
{
    CHK(plate_params(p, "eppm_plate_render_host"));
    if (!inv || !rgb || !blocked || !state || !rgb_out) return set_err(EPPM_ERR_ARG, "eppm_plate_render_host: NULL argument");
    CHK(size_check(h, w, p->margin_x, p->margin_y, "eppm_plate_render_host"));
    plate_render_host(inv, ok != 0, rgb, blocked, h, w, p->margin_x, p->margin_y, p->min_count, reinterpret_cast<const TfState*>(state), rgb_out, fill);
    return EPPM_OK;
}
