// deflicker.cpp -- flicker removal: eppm_deflicker (a stage object, stage_object.h), its step on a context's pairs
// or on caller planes (the kernels: k_deflicker.hip), the synchronous getters and state calls, and the host form
// eppm_deflicker_step_host.  The host form shares deflicker.h's arithmetic with the kernels.
#include "stage_object.h"
#include "deflicker.h"

using namespace eppm;

struct eppm_deflicker : StageObject {   // mem: nslots blocks `stride` bytes apart (DeflickerArgs)
    eppm_deflicker_params p{};
    int cx = 0, cy = 0;
    size_t stride = 0;
    std::vector<uint8_t> cur, empty, stepped, saved;    // per slot: which reference is current, whether the slot counts as empty, whether the
                                                        // field, sums and valid planes / the current reference hold anything
    size_t cells() const { return (size_t)cx * cy; }
    char* plane(int slot, size_t off) const { return mem + (size_t)slot * stride + off; }
    uint32_t* ref(int slot) const { return (uint32_t*)plane(slot, deflicker_off_ref(px(), cur[slot])); }
};

namespace {

int deflicker_params(const eppm_deflicker_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (p->cell != 16 && p->cell != 32 && p->cell != 64) return set_err(EPPM_ERR_ARG, "%s: cell %d is not 16, 32 or 64", what, p->cell);
    if (p->iters < 1 || p->iters > 4) return set_err(EPPM_ERR_ARG, "%s: iters %d outside [1, 4]", what, p->iters);
    if (!(p->reject >= 0.0f && p->reject <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: reject must be finite and >= 0", what);
    if (!(p->tau >= 0.0f && p->tau <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: tau must be finite and >= 0", what);
    if (!(p->keep >= 0.0f && p->keep <= 1.0f)) return set_err(EPPM_ERR_ARG, "%s: keep must lie in [0, 1]", what);
    if (p->n_min < 1) return set_err(EPPM_ERR_ARG, "%s: n_min %d < 1", what, p->n_min);
    return EPPM_OK;
}

int slot_check(const eppm_deflicker* f, int slot, bool need_out, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_out && !f->stepped[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has not been stepped", what, slot);
    return EPPM_OK;
}

uint32_t word_of(const uint8_t* rgb, size_t i) { return (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16; }

}  // namespace

extern "C" int eppm_deflicker_default_params(eppm_deflicker_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_deflicker_default_params: NULL");
    p->cell = 32;
    p->iters = 2;
    p->reject = 60.0f;
    p->tau = 12.0f;
    p->keep = 1.0f;
    p->n_min = 32;
    return EPPM_OK;
}

static int deflicker_new(int device, int h, int w, int nslots, const eppm_deflicker_params* in, eppm_deflicker** out)
{
    eppm_deflicker_params def;
    eppm_deflicker_default_params(&def);
    const eppm_deflicker_params* p = in ? in : &def;
    CHK(deflicker_params(p, "eppm_deflicker_create"));
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_deflicker_create: size %dx%d out of range", w, h);
    eppm_deflicker* f = new eppm_deflicker;
    f->noun = "deflicker object";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->p = *p;
    f->cx = (w + p->cell - 1) / p->cell;
    f->cy = (h + p->cell - 1) / p->cell;
    f->stride = up256(deflicker_slot_bytes(f->px(), f->cells()));
    f->bytes = f->stride * nslots;
    const int rc = stage_open(f, "eppm_deflicker_create");
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

extern "C" int eppm_deflicker_create(eppm_ctx* ctx, const eppm_deflicker_params* in, eppm_deflicker** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_deflicker_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return deflicker_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_deflicker_create_size(int h, int w, int nslots, int device, const eppm_deflicker_params* in, eppm_deflicker** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_deflicker_create_size: NULL argument");
    *out = nullptr;
    return deflicker_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_deflicker_destroy(eppm_deflicker* f)
{
    if (!f) return EPPM_OK;
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_deflicker_reset(eppm_deflicker* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_deflicker_reset: NULL object");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_deflicker_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->empty[k] = 1;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the object's members are filled in here); cut: NULL or
// one flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_deflicker* f, DeflickerArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.cell = f->p.cell; in.cx = f->cx; in.cy = f->cy; in.n_min = f->p.n_min;
    in.keep = f->p.keep;
    slot_mask(in.cur, f->cur.data() + slot0, slot0, in.n);
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "deflicker_fit");
        for (int k = 0; k < f->p.iters; k++) {
            in.pass = k;
            in.bound = k == 0 ? f->p.reject : f->p.tau;
            launch_deflicker_accumulate(in, s);
            launch_deflicker_field(in, s);
        }
    }
    {
        StageTimer t(timing, "deflicker_apply");
        launch_deflicker_apply(in, s);
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

extern "C" int eppm_deflicker_step(eppm_deflicker* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_deflicker_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_deflicker_step", &c, &s));
    DeflickerArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return step_on(f, in, 0, cut, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_deflicker_step_frames(eppm_deflicker* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch,
                                          const eppm_float2* d_flow_bwd, const uint8_t* d_occ2, int cut)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow_bwd || !d_occ2) return set_err(EPPM_ERR_ARG, "eppm_deflicker_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_deflicker_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_deflicker_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_deflicker_step_frames", [&](hipStream_t s) {
        DeflickerArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.bwd = (const float*)d_flow_bwd; in.occ2 = d_occ2;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    });
}

extern "C" int eppm_deflicker_get(eppm_deflicker* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deflicker_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get: row_stride %zu < 3*w", row_stride);
    return stage_get_rgb(f, f->ref(slot), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_deflicker_get_device(eppm_deflicker* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deflicker_get_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get_device: bad pitch %zu", pitch);
    return stage_get_rgba_device(f, f->ref(slot), f->h, f->w, d_rgba, pitch);
}

extern "C" int eppm_deflicker_get_field(eppm_deflicker* f, int slot, float* field, uint8_t* valid)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get_field: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deflicker_get_field"));
    CHK(stage_wait(f));
    if (field) HIPCHK(hipMemcpy(field, f->plane(slot, deflicker_off_field(f->px(), f->cells())), f->cells() * kDkField * 4, hipMemcpyDeviceToHost));
    if (valid) HIPCHK(hipMemcpy(valid, f->plane(slot, deflicker_off_valid(f->px(), f->cells())), f->cells(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

// the counts are sums over the cells' records of the last pass, which the step leaves in the slot's block: added here, not on the device
extern "C" int eppm_deflicker_get_stats(eppm_deflicker* f, int slot, eppm_deflicker_stats* stats)
{
    if (!f || !stats) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get_stats: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_deflicker_get_stats"));
    CHK(stage_wait(f));
    std::vector<uint32_t> sums(f->cells() * kDkSums);
    HIPCHK(hipMemcpy(sums.data(), f->plane(slot, deflicker_off_sums(f->px())), sums.size() * 4, hipMemcpyDeviceToHost));
    *stats = eppm_deflicker_stats{0, 0, (int32_t)f->cells()};
    for (size_t c = 0; c < f->cells(); c++) {
        stats->used += sums[c * kDkSums];
        stats->valid_cells += (int)sums[c * kDkSums] >= f->p.n_min;
    }
    return EPPM_OK;
}

extern "C" int eppm_deflicker_get_state(eppm_deflicker* f, int slot, uint8_t* rgb, int* empty)
{
    if (!f || !rgb || !empty) return set_err(EPPM_ERR_ARG, "eppm_deflicker_get_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_deflicker_get_state"));
    if (!f->saved[slot]) return set_err(EPPM_ERR_STATE, "eppm_deflicker_get_state: slot %d holds no reference", slot);
    CHK(stage_get_rgb(f, f->ref(slot), f->h, f->w, rgb, (size_t)f->w * 3));
    *empty = f->empty[slot];
    return EPPM_OK;
}

extern "C" int eppm_deflicker_set_state(eppm_deflicker* f, int slot, const uint8_t* rgb, int empty)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_deflicker_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_deflicker_set_state"));
    CHK(stage_wait(f));
    std::vector<uint32_t> words(f->px());
    for (size_t i = 0; i < f->px(); i++) words[i] = word_of(rgb, i) | 255u << 24;
    HIPCHK(hipMemcpy(f->ref(slot), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->empty[slot] = empty != 0;
    f->saved[slot] = 1;
    return EPPM_OK;
}

// ---- host form: the same step as sequential loops ----
extern "C" int eppm_deflicker_step_host(const eppm_deflicker_params* p, uint8_t* rgb_out, float* field_out, uint8_t* valid_out,
                                        eppm_deflicker_stats* stats, const uint8_t* rgb_ref, const uint8_t* rgb_cur, const float* bu,
                                        const float* bv, const uint8_t* occ2, int h, int w, int cut)
{
    CHK(deflicker_params(p, "eppm_deflicker_step_host"));
    if (!rgb_out || !field_out || !valid_out || !stats || !rgb_ref || !rgb_cur || !bu || !bv || !occ2)
        return set_err(EPPM_ERR_ARG, "eppm_deflicker_step_host: NULL argument");
    if (rgb_out == rgb_ref) return set_err(EPPM_ERR_ARG, "eppm_deflicker_step_host: the step gathers, rgb_out must not be rgb_ref");
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_deflicker_step_host: size %dx%d out of range", w, h);
    const int cell = p->cell, cx = (w + cell - 1) / cell, cy = (h + cell - 1) / cell;
    const size_t cells = (size_t)cx * cy;
    std::vector<uint32_t> sums(cells * kDkSums);
    auto R = [&](int x, int y) { return word_of(rgb_ref, (size_t)y * w + x); };
    auto F = [&](int i, int j) { return (const float*)field_out + ((size_t)j * cx + i) * kDkField; };
    auto S = [&](int i, int j) { return (const uint32_t*)sums.data() + ((size_t)j * cx + i) * kDkSums; };
    for (int k = 0; k < p->iters; k++) {
        const float bound = k == 0 ? p->reject : p->tau;
        std::fill(sums.begin(), sums.end(), 0u);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const uint32_t word = word_of(rgb_cur, i);
                float s[3], g[kDkField] = {1.0f, 1.0f, 1.0f, 0.0f, 0.0f, 0.0f};
                if (!deflicker_sample(x, y, bu[i], bv[i], occ2[i], cut != 0, h, w, R, s)) continue;
                if (k > 0) deflicker_field_at(x, y, cell, cx, cy, F, g);
                if (deflicker_member(word, s, g, g + 3, bound)) deflicker_add(&sums[((size_t)(y / cell) * cx + x / cell) * kDkSums], word, s);
            }
        std::vector<float> field(cells * kDkField);         // pass k's field reads pass k's sums only; field_out holds pass k - 1's until here
        for (int j = 0; j < cy; j++)
            for (int i = 0; i < cx; i++) valid_out[(size_t)j * cx + i] = deflicker_smooth(i, j, cx, cy, p->n_min, S, &field[((size_t)j * cx + i) * kDkField]);
        std::copy(field.begin(), field.end(), field_out);
    }
    *stats = eppm_deflicker_stats{0, 0, (int32_t)cells};
    for (size_t c = 0; c < cells; c++) {
        stats->used += sums[c * kDkSums];
        stats->valid_cells += valid_out[c];
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            float g[kDkField];
            deflicker_field_at(x, y, cell, cx, cy, F, g);
            const uint32_t o = deflicker_out(word_of(rgb_cur, i), g, p->keep);
            rgb_out[3 * i] = (uint8_t)o; rgb_out[3 * i + 1] = (uint8_t)(o >> 8); rgb_out[3 * i + 2] = (uint8_t)(o >> 16);
        }
    return EPPM_OK;
}
