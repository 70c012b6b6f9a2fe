// tfilter.cpp -- motion-compensated temporal denoising: eppm_tfilter (a stage object, stage_object.h), its step on
// a context's pairs or on caller planes (the kernel: k_tfilter.hip), the synchronous state calls, and the host forms
// eppm_tfilter_seed_host / eppm_tfilter_step_host.  The host form shares tfilter.h's per-pixel arithmetic with the kernel.
#include "stage_object.h"
#include "tfilter.h"

using namespace eppm;

struct eppm_tfilter : StageObject {     // mem: nslots blocks `stride` bytes apart: state 0 | state 1 (h*w float4 each) | out (h*w RGBA words)
    float thresh = 0.0f;
    int n_max = 0;
    size_t stride = 0;
    std::vector<uint8_t> cur, empty;    // per slot: which state is current, and whether the slot has one at all
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

int slot_check(const eppm_tfilter* f, int slot, bool need_state, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
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
    eppm_tfilter* f = new eppm_tfilter;
    f->noun = "filter";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->thresh = p->thresh; f->n_max = p->n_max;
    f->stride = up256(f->px() * 36);
    f->bytes = f->stride * nslots;
    const int rc = stage_open(f, "eppm_tfilter_create");
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->cur.assign(nslots, 0);
    f->empty.assign(nslots, 1);
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
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_tfilter_reset(eppm_tfilter* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_tfilter_reset: NULL filter");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_tfilter_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the state members are filled in here); cut: NULL or
// one flag per pair.  timing: the context whose stage-timing entries receive the stage, or NULL
static int step_on(eppm_tfilter* f, TFilterArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.st0 = f->state(0, 0);
    in.st1 = f->state(0, 1);
    in.out = f->out(0);
    in.slot_stride = f->stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.thresh = f->thresh; in.n_max = f->n_max;
    slot_mask(in.cur, f->cur.data() + slot0, slot0, in.n);
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "tfilter_step");
        launch_tfilter_step(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) {
        f->cur[k] ^= 1;
        f->empty[k] = 0;
    }
    return EPPM_OK;
}

extern "C" int eppm_tfilter_step(eppm_tfilter* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_tfilter_step", &c, &s));
    TFilterArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return step_on(f, in, 0, cut, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_tfilter_step_frames(eppm_tfilter* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch,
                                        const eppm_float2* d_flow_bwd, const uint8_t* d_occ2, int cut)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow_bwd || !d_occ2) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_tfilter_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_tfilter_step_frames", [&](hipStream_t s) {
        TFilterArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.bwd = (const float*)d_flow_bwd; in.occ2 = d_occ2;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    });
}

extern "C" int eppm_tfilter_get(eppm_tfilter* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get: row_stride %zu < 3*w", row_stride);
    return stage_get_rgb(f, f->out(slot), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_tfilter_get_device(eppm_tfilter* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_device: bad pitch %zu", pitch);
    return stage_get_rgba_device(f, f->out(slot), f->h, f->w, d_rgba, pitch);
}

extern "C" int eppm_tfilter_get_state(eppm_tfilter* f, int slot, float* acc)
{
    if (!f || !acc) return set_err(EPPM_ERR_ARG, "eppm_tfilter_get_state: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_tfilter_get_state"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(acc, f->state(slot, f->cur[slot]), f->px() * 16, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_tfilter_set_state(eppm_tfilter* f, int slot, const float* acc)
{
    if (!f || !acc) return set_err(EPPM_ERR_ARG, "eppm_tfilter_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_tfilter_set_state"));
    CHK(stage_wait(f));
    std::vector<uint32_t> words(f->px());
    for (size_t i = 0; i < f->px(); i++) words[i] = tfilter_word(TfState{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]});
    HIPCHK(hipMemcpy(f->state(slot, f->cur[slot]), acc, f->px() * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->out(slot), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
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
