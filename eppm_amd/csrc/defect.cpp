// defect.cpp -- film-defect removal: eppm_defect (a stage object, stage_object.h), its step on a context's pairs
// or on caller planes (the kernels: k_defect.hip), the synchronous getters and state calls, and the host form eppm_defect_step_host.  The
// host form shares defect.h's per-pixel arithmetic with the kernels.
#include "stage_object.h"
#include "defect.h"

using namespace eppm;

struct eppm_defect : StageObject {      // mem: nslots blocks `stride` bytes apart (DefectArgs), then one eppm_defect_stats per slot
    eppm_defect_params p{};
    size_t stride = 0;
    std::vector<uint8_t> cur, has_prev, stepped, saved;    // per slot: which saved set is current, whether it is the frame before image 1,
                                                           // whether the output planes / the saved set hold anything
    char* plane(int slot, size_t off) const { return mem + (size_t)slot * stride + off; }
    int32_t* stats() const { return (int32_t*)(mem + stride * nslots); }
};

namespace {

int defect_params(const eppm_defect_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->detect >= 0.0f && p->detect <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: detect must be finite and >= 0", what);
    if (!(p->agree >= 0.0f && p->agree <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: agree must be finite and >= 0", what);
    if (p->radius < 0 || p->radius > 4) return set_err(EPPM_ERR_ARG, "%s: radius %d outside [0, 4]", what, p->radius);
    if (p->grow < 0 || p->grow > 4) return set_err(EPPM_ERR_ARG, "%s: grow %d outside [0, 4]", what, p->grow);
    return EPPM_OK;
}

int slot_check(const eppm_defect* f, int slot, bool need_out, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_out && !f->stepped[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has not been stepped", what, slot);
    return EPPM_OK;
}

}  // namespace

extern "C" int eppm_defect_default_params(eppm_defect_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_defect_default_params: NULL");
    p->detect = 60.0f;
    p->agree = 30.0f;
    p->radius = 3;
    p->grow = 1;
    return EPPM_OK;
}

static int defect_new(int device, int h, int w, int nslots, const eppm_defect_params* in, eppm_defect** out)
{
    eppm_defect_params def;
    eppm_defect_default_params(&def);
    const eppm_defect_params* p = in ? in : &def;
    CHK(defect_params(p, "eppm_defect_create"));
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_defect_create: size %dx%d out of range", w, h);
    eppm_defect* f = new eppm_defect;
    f->noun = "defect filter";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->p = *p;
    f->stride = up256(f->px() * 34);
    f->bytes = f->stride * nslots + up256((size_t)(nslots > 0 ? nslots : 0) * sizeof(eppm_defect_stats));
    const int rc = stage_open(f, "eppm_defect_create");
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->cur.assign(nslots, 0);
    f->has_prev.assign(nslots, 0);
    f->stepped.assign(nslots, 0);
    f->saved.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_defect_create(eppm_ctx* ctx, const eppm_defect_params* in, eppm_defect** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_defect_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return defect_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_defect_create_size(int h, int w, int nslots, int device, const eppm_defect_params* in, eppm_defect** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_defect_create_size: NULL argument");
    *out = nullptr;
    return defect_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_defect_destroy(eppm_defect* f)
{
    if (!f) return EPPM_OK;
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_defect_reset(eppm_defect* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_defect_reset: NULL filter");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_defect_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) f->has_prev[k] = 0;
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the object's members are filled in here); cut: NULL or
// one flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_defect* f, DefectArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride;
    in.stats = f->stats();
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.detect = f->p.detect; in.agree = f->p.agree; in.radius = f->p.radius; in.grow = f->p.grow;
    std::vector<uint8_t> active(in.n);
    for (int k = 0; k < in.n; k++) active[k] = f->has_prev[slot0 + k] && !(cut && cut[k]);
    slot_mask(in.cur, f->cur.data() + slot0, slot0, in.n);
    slot_mask(in.active, active.data(), slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "defect_detect");
        launch_defect_detect(in, s);
    }
    {
        StageTimer t(timing, "defect_apply");
        launch_defect_apply(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) {
        f->cur[k] ^= 1;
        f->has_prev[k] = !(cut && cut[k - slot0]);
        f->stepped[k] = 1;
        f->saved[k] = 1;
    }
    return EPPM_OK;
}

extern "C" int eppm_defect_step(eppm_defect* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_defect_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_defect_step", &c, &s));
    DefectArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.fwd = c.fwd; in.fwd_stride = c.fwd_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.n = c.n;
    return step_on(f, in, 0, cut, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_defect_step_frames(eppm_defect* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch,
                                       const eppm_float2* d_flow, const eppm_float2* d_flow_bwd, int cut)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow || !d_flow_bwd) return set_err(EPPM_ERR_ARG, "eppm_defect_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_defect_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_defect_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_defect_step_frames", [&](hipStream_t s) {
        DefectArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.fwd = (const float*)d_flow; in.bwd = (const float*)d_flow_bwd;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    });
}

extern "C" int eppm_defect_get(eppm_defect* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_defect_get: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_defect_get"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_defect_get: row_stride %zu < 3*w", row_stride);
    return stage_get_rgb(f, (const uint32_t*)f->plane(slot, defect_off_out(f->px())), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_defect_get_device(eppm_defect* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_defect_get_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_defect_get_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_defect_get_device: bad pitch %zu", pitch);
    return stage_get_rgba_device(f, (const uint32_t*)f->plane(slot, defect_off_out(f->px())), f->h, f->w, d_rgba, pitch);
}

extern "C" int eppm_defect_get_mask(eppm_defect* f, int slot, uint8_t* mask)
{
    if (!f || !mask) return set_err(EPPM_ERR_ARG, "eppm_defect_get_mask: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_defect_get_mask"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(mask, f->plane(slot, defect_off_mask(f->px())), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_defect_get_stats(eppm_defect* f, int slot, eppm_defect_stats* stats)
{
    if (!f || !stats) return set_err(EPPM_ERR_ARG, "eppm_defect_get_stats: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_defect_get_stats"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(stats, f->stats() + (size_t)slot * 4, sizeof(*stats), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_defect_get_state(eppm_defect* f, int slot, uint8_t* rgb, float* bwd, int* has_prev)
{
    if (!f || !rgb || !bwd || !has_prev) return set_err(EPPM_ERR_ARG, "eppm_defect_get_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_defect_get_state"));
    if (!f->saved[slot]) return set_err(EPPM_ERR_STATE, "eppm_defect_get_state: slot %d holds no saved frame", slot);
    CHK(stage_get_rgb(f, (const uint32_t*)f->plane(slot, defect_off_img(f->px(), f->cur[slot])), f->h, f->w, rgb, (size_t)f->w * 3));
    HIPCHK(hipMemcpy(bwd, f->plane(slot, defect_off_bwd(f->px(), f->cur[slot])), f->px() * 8, hipMemcpyDeviceToHost));
    *has_prev = f->has_prev[slot];
    return EPPM_OK;
}

extern "C" int eppm_defect_set_state(eppm_defect* f, int slot, const uint8_t* rgb, const float* bwd, int has_prev)
{
    if (!f || !rgb || !bwd) return set_err(EPPM_ERR_ARG, "eppm_defect_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_defect_set_state"));
    CHK(stage_wait(f));
    std::vector<uint32_t> words(f->px());
    for (size_t i = 0; i < f->px(); i++) words[i] = (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16 | 255u << 24;
    HIPCHK(hipMemcpy(f->plane(slot, defect_off_img(f->px(), f->cur[slot])), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->plane(slot, defect_off_bwd(f->px(), f->cur[slot])), bwd, f->px() * 8, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->has_prev[slot] = has_prev != 0;
    f->saved[slot] = 1;
    return EPPM_OK;
}

// ---- host form: the same step as two sequential loops ----
extern "C" int eppm_defect_step_host(const eppm_defect_params* p, uint8_t* rgb_out, uint8_t* mask_out, eppm_defect_stats* stats,
                                     const uint8_t* rgb_prev, const uint8_t* rgb_cur, const uint8_t* rgb_next, const float* bu, const float* bv,
                                     const float* fu, const float* fv, int h, int w)
{
    CHK(defect_params(p, "eppm_defect_step_host"));
    if (!rgb_out || !mask_out || !stats || !rgb_cur) return set_err(EPPM_ERR_ARG, "eppm_defect_step_host: NULL argument");
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "eppm_defect_step_host: size %dx%d out of range", w, h);
    const bool active = rgb_prev && rgb_next;
    if (active && (!bu || !bv || !fu || !fv)) return set_err(EPPM_ERR_ARG, "eppm_defect_step_host: NULL flow plane");
    if (rgb_out == rgb_cur) return set_err(EPPM_ERR_ARG, "eppm_defect_step_host: rgb_out must not be rgb_cur");
    *stats = eppm_defect_stats{0, 0, 0, 0};
    const size_t px = (size_t)h * w;
    auto word_of = [](const uint8_t* rgb, size_t i) { return (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16; };
    std::vector<uint8_t> code(px, 0);
    std::vector<uint32_t> repl(px);
    for (size_t i = 0; i < px; i++) repl[i] = word_of(rgb_cur, i) | 0xff000000u;
    if (active) {
        auto P = [&](int x, int y) { return word_of(rgb_prev, (size_t)y * w + x); };
        auto N = [&](int x, int y) { return word_of(rgb_next, (size_t)y * w + x); };
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                const uint32_t cur = word_of(rgb_cur, i);
                const DfChance c1 = defect_chance(x, y, cur, bu[i], bv[i], fu[i], fv[i], h, w, p->detect, p->agree, P, N);
                code[i] = defect_code(c1, nullptr, &repl[i]);
                if (c1.decided || p->radius <= 0) continue;
                auto K = [&](int dx, int dy) {
                    const int gx = x + dx < 0 ? 0 : (x + dx > w - 1 ? w - 1 : x + dx), gy = y + dy < 0 ? 0 : (y + dy > h - 1 ? h - 1 : y + dy);
                    const size_t g = (size_t)gy * w + gx;
                    return defect_keys(fu[g], fv[g], bu[g], bv[g]);
                };
                float m[4];
                if (!defect_median(p->radius, K, m)) continue;
                const DfChance c2 = defect_chance(x, y, cur, m[2], m[3], m[0], m[1], h, w, p->detect, p->agree, P, N);
                code[i] = defect_code(c1, &c2, &repl[i]);
            }
    }
    auto C = [&](int x, int y) { return code[(size_t)y * w + x]; };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint8_t m = defect_mask(x, y, h, w, p->grow, C);
            const uint32_t o = m ? repl[i] : word_of(rgb_cur, i);
            rgb_out[3 * i] = (uint8_t)o; rgb_out[3 * i + 1] = (uint8_t)(o >> 8); rgb_out[3 * i + 2] = (uint8_t)(o >> 16);
            mask_out[i] = m;
            stats->hit += m == 1;
            stats->grown += m == 2;
            stats->second_chance += (code[i] & kDfSecond) != 0;
            stats->undecided += (code[i] & kDfUndecided) != 0;
        }
    return EPPM_OK;
}
