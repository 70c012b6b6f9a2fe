// deint.cpp -- motion-compensated deinterlacing: eppm_deint (a stage object, stage_object.h), its step on a
// context's pairs or on caller planes and the bob on caller planes (the kernels: k_deint.hip), the synchronous getters and state calls.
// The host forms and the interlaced y4m reader are eppm_io.cpp's; the arithmetic is deint.h's.
#include "stage_object.h"
#include "deint.h"
#include "../../include/eppm_deint.h"

using namespace eppm;

struct eppm_deint : StageObject {   // mem: nslots blocks `stride` bytes apart (DeintArgs)
    eppm_deint_params p{};
    size_t stride = 0;
    std::vector<uint8_t> cur, empty, stepped, saved;    // per slot: which reference is current, whether the slot counts as empty, whether the
                                                        // mask plane / the current reference hold anything
    char* plane(int slot, size_t off) const { return mem + (size_t)slot * stride + off; }
    uint32_t* ref(int slot) const { return (uint32_t*)plane(slot, deint_off_ref(px(), cur[slot])); }
};

static int deint_params(const eppm_deint_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (const char* why = deint_params_bad(p->thresh, p->use_occ)) return set_err(EPPM_ERR_ARG, "%s: %s", what, why);
    return EPPM_OK;
}

static int slot_check(const eppm_deint* f, int slot, bool need_out, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_out && !f->stepped[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has not been stepped", what, slot);
    return EPPM_OK;
}

static int deint_new(int device, int h, int w, int nslots, const eppm_deint_params* in, eppm_deint** out)
{
    eppm_deint_params def;
    eppm_deint_default_params(&def);
    const eppm_deint_params* p = in ? in : &def;
    CHK(deint_params(p, "eppm_deint_create"));
    if (h < 2 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_deint_create: size %dx%d out of range (h >= 2)", w, h);
    eppm_deint* f = new eppm_deint;
    f->noun = "deinterlacer";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->p = *p;
    f->stride = up256(deint_slot_bytes(f->px()));
    f->bytes = f->stride * nslots;
    const int rc = stage_open(f, "eppm_deint_create");
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->cur.assign(nslots, 0);
    f->empty.assign(nslots, 1);
    f->stepped.assign(nslots, 0);
    f->saved.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_deint_create(eppm_ctx* ctx, const eppm_deint_params* in, eppm_deint** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_deint_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return deint_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_deint_create_size(int h, int w, int nslots, int device, const eppm_deint_params* in, eppm_deint** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_deint_create_size: NULL argument");
    *out = nullptr;
    return deint_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_deint_destroy(eppm_deint* f)
{
    if (!f) return EPPM_OK;
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_deint_reset(eppm_deint* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_deint_reset: NULL object");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_deint_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the object's members are filled in here); cut: NULL or
// one flag per pair; parity: one byte per pair.  timing: the context whose stage-timing entries receive the stage, or NULL
static int step_on(eppm_deint* f, DeintArgs& in, int slot0, const uint8_t* cut, const uint8_t* parity, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.thresh = f->p.thresh; in.use_occ = f->p.use_occ;
    slot_mask(in.cur, f->cur.data() + slot0, slot0, in.n);
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    slot_mask(in.parity, parity, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "deint_step");
        launch_deint_step(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) {
        f->cur[k] ^= 1;
        f->empty[k] = 0;
        f->stepped[k] = 1;
        f->saved[k] = 1;
    }
    return EPPM_OK;
}

static int parity_check(const uint8_t* parity, int n, const char* what)
{
    if (!parity) return set_err(EPPM_ERR_ARG, "%s: NULL parity", what);
    for (int k = 0; k < n; k++)
        if (parity[k] > 1) return set_err(EPPM_ERR_ARG, "%s: parity %d of pair %d is not 0 or 1", what, parity[k], k);
    return EPPM_OK;
}

extern "C" int eppm_deint_step(eppm_deint* f, eppm_ctx* ctx, const uint8_t* cut, const uint8_t* parity)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_deint_step: NULL argument");
    if (!parity) return set_err(EPPM_ERR_ARG, "eppm_deint_step: NULL parity");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_deint_step", &c, &s));
    CHK(parity_check(parity, c.n, "eppm_deint_step"));
    DeintArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return step_on(f, in, 0, cut, parity, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_deint_step_frames(eppm_deint* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                                      const uint8_t* d_occ2, int cut, int parity)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow_bwd || !d_occ2) return set_err(EPPM_ERR_ARG, "eppm_deint_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_deint_step_frames"));
    if (bad_pitch(pitch, f->w) || ((uintptr_t)d_rgba1 & 3) || ((uintptr_t)d_rgba2 & 3) || ((uintptr_t)d_flow_bwd & 7))
        return set_err(EPPM_ERR_ARG, "eppm_deint_step_frames: bad pitch %zu, or an image not on a multiple of 4 bytes or a flow not on a multiple of 8", pitch);
    if (parity != 0 && parity != 1) return set_err(EPPM_ERR_ARG, "eppm_deint_step_frames: parity %d is not 0 or 1", parity);
    return launcher_run(f, "eppm_deint_step_frames", [&](hipStream_t s) {
        DeintArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.bwd = (const float*)d_flow_bwd; in.occ2 = d_occ2;
        in.n = 1;
        const uint8_t c = cut != 0, p = (uint8_t)parity;
        return step_on(f, in, slot, &c, &p, s, nullptr);
    });
}

extern "C" int eppm_deint_get(eppm_deint* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_deint_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deint_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_deint_get: row_stride %zu < 3*w", row_stride);
    return stage_get_rgb(f, f->ref(slot), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_deint_get_device(eppm_deint* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_deint_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deint_get_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_deint_get_device: bad pitch %zu", pitch);
    return stage_get_rgba_device(f, f->ref(slot), f->h, f->w, d_rgba, pitch);
}

extern "C" int eppm_deint_get_mask(eppm_deint* f, int slot, uint8_t* mask)
{
    if (!f || !mask) return set_err(EPPM_ERR_ARG, "eppm_deint_get_mask: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deint_get_mask"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(mask, f->plane(slot, deint_off_mask(f->px())), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

// the counts are sums over the mask the step leaves in the slot's block: added here, not on the device
extern "C" int eppm_deint_get_stats(eppm_deint* f, int slot, eppm_deint_stats* stats)
{
    if (!f || !stats) return set_err(EPPM_ERR_ARG, "eppm_deint_get_stats: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deint_get_stats"));
    CHK(stage_wait(f));
    std::vector<uint8_t> mask(f->px());
    HIPCHK(hipMemcpy(mask.data(), f->plane(slot, deint_off_mask(f->px())), f->px(), hipMemcpyDeviceToHost));
    *stats = eppm_deint_stats{0, 0};
    for (const uint8_t m : mask) {
        stats->temporal += m == 1;
        stats->spatial += m == 2;
    }
    return EPPM_OK;
}

extern "C" int eppm_deint_get_state(eppm_deint* f, int slot, uint8_t* rgb, int* empty)
{
    if (!f || !rgb || !empty) return set_err(EPPM_ERR_ARG, "eppm_deint_get_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_deint_get_state"));
    if (!f->saved[slot]) return set_err(EPPM_ERR_STATE, "eppm_deint_get_state: slot %d holds no reference", slot);
    CHK(stage_get_rgb(f, f->ref(slot), f->h, f->w, rgb, (size_t)f->w * 3));
    *empty = f->empty[slot];
    return EPPM_OK;
}

extern "C" int eppm_deint_set_state(eppm_deint* f, int slot, const uint8_t* rgb, int empty)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_deint_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_deint_set_state"));
    CHK(stage_wait(f));
    std::vector<uint32_t> words(f->px());
    for (size_t i = 0; i < f->px(); i++) words[i] = (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16 | 255u << 24;
    HIPCHK(hipMemcpy(f->ref(slot), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->empty[slot] = empty != 0;
    f->saved[slot] = 1;
    return EPPM_OK;
}

// ---- the bob on caller planes ----
extern "C" int eppm_deint_bob_stream(void* d_out, size_t out_pitch, const void* d_field, size_t field_pitch, int h, int w, int parity, void* stream)
{
    if (!d_out || !d_field) return set_err(EPPM_ERR_ARG, "eppm_deint_bob: NULL argument");
    if (h < 2 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_deint_bob: size %dx%d out of range (h >= 2)", w, h);
    if (parity != 0 && parity != 1) return set_err(EPPM_ERR_ARG, "eppm_deint_bob: parity %d is not 0 or 1", parity);
    if (bad_pitch(out_pitch, w) || bad_pitch(field_pitch, w) || ((uintptr_t)d_out & 3) || ((uintptr_t)d_field & 3))
        return set_err(EPPM_ERR_ARG, "eppm_deint_bob: bad pitch %zu / %zu or address", out_pitch, field_pitch);
    launch_deint_bob((uint32_t*)d_out, out_pitch, (const uint32_t*)d_field, field_pitch, h, w, parity, stream ? (hipStream_t)stream : launcher_stream());
    HIPCHK(hipGetLastError());
    return EPPM_OK;
}

extern "C" int eppm_deint_bob(void* d_out, size_t out_pitch, const void* d_field, size_t field_pitch, int h, int w, int parity)
{
    return eppm_deint_bob_stream(d_out, out_pitch, d_field, field_pitch, h, w, parity, nullptr);
}
