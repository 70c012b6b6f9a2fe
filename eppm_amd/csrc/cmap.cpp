// cmap.cpp -- dense correspondence maps to an anchor frame: eppm_cmap (a stage object, stage_object.h), its step on a
// context's pairs or on caller planes and its render (the kernels: k_cmap.hip), the synchronous state calls, and the host forms eppm_cmap_step_host /
// eppm_cmap_render_host.  The host forms share cmap.h's per-pixel arithmetic with the kernels.
#include "stage_object.h"
#include "cmap.h"
#include "gmotion.h"

using namespace eppm;

struct eppm_cmap : StageObject {        // mem: nslots blocks `stride` bytes apart: map 0 | map 1 (h*w float2 each) | anchor | frame | layer | out (h*w words each)
    eppm_cmap_params prm{};
    size_t stride = 0;
    std::vector<uint8_t> cur, empty;    // per slot: which map is current, and whether the slot has a state at all
    std::vector<uint8_t> deflayer;      // per slot: the layer is the anchor with alpha 255 (the layer plane is not read)
    std::vector<uint8_t> rendered;      // per slot: `out` is the render of the current map, frame and layer
    std::vector<int> age;               // per slot: steps since the anchor
    char* block(int slot) const { return mem + (size_t)slot * stride; }
    float* map(int slot, int which) const { return (float*)(block(slot) + (size_t)which * px() * 8); }
    uint32_t* words(int slot, int plane) const { return (uint32_t*)(block(slot) + px() * 16 + (size_t)plane * px() * 4); }   // 0 anchor, 1 frame, 2 layer, 3 out
};

namespace {

int cmap_params(const eppm_cmap_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->thresh >= 0.0f && p->thresh <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: thresh must be finite and >= 0", what);
    if (!(p->tear >= 0.0f && p->tear <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: tear must be finite and >= 0", what);
    if (p->use_occ != 0 && p->use_occ != 1) return set_err(EPPM_ERR_ARG, "%s: use_occ %d is neither 0 nor 1", what, p->use_occ);
    return EPPM_OK;
}

int cmap_size(int h, int w, const char* what)
{
    if (!gm_size_ok(h, w)) return set_err(EPPM_ERR_ARG, "%s: size %dx%d out of range (w, h <= %d, h*w <= 2^26)", what, w, h, kGmMaxDim);
    return EPPM_OK;
}

int slot_check(const eppm_cmap* f, int slot, bool need_state, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_state && f->empty[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has never been stepped", what, slot);
    return EPPM_OK;
}

void fill_args(const eppm_cmap* f, CMapArgs& a, int slot0, int n, const uint8_t* cut)
{
    a.mem = f->mem;
    a.slot_stride = f->stride;
    a.off_anchor = f->px() * 16;
    a.h = f->h; a.w = f->w; a.n = n; a.slot0 = slot0;
    a.thresh = f->prm.thresh; a.tear = f->prm.tear; a.use_occ = f->prm.use_occ;
    slot_mask(a.cur, f->cur.data() + slot0, slot0, n);
    slot_mask(a.empty, f->empty.data() + slot0, slot0, n);
    slot_mask(a.deflayer, f->deflayer.data() + slot0, slot0, n);
    slot_mask(a.cut, cut, slot0, n);
}

// `out` of one slot is its render: a launch on the stream of the last step, behind it, if something changed since the last one
int render_slot(eppm_cmap* f, int slot)
{
    HIPCHK(hipSetDevice(f->device));
    if (f->rendered[slot]) return EPPM_OK;
    CMapArgs a{};
    fill_args(f, a, slot, 1, nullptr);
    CHK(stage_enter(f, f->last));
    launch_cmap_render(a, f->last);
    CHK(stage_leave(f, f->last));
    f->rendered[slot] = 1;
    return EPPM_OK;
}

void pack_words(std::vector<uint32_t>& words, const uint8_t* src, size_t row_stride, int h, int w, int channels)
{
    words.resize((size_t)h * w);
    for (int y = 0; y < h; y++) {
        const uint8_t* q = src + (size_t)y * row_stride;
        for (int x = 0; x < w; x++, q += channels) {
            uint32_t v = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
            if (channels == 4) v |= (uint32_t)q[3] << 24;
            words[(size_t)y * w + x] = v;
        }
    }
}

}  // namespace

extern "C" int eppm_cmap_default_params(eppm_cmap_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_cmap_default_params: NULL");
    p->thresh = 90.0f;
    p->tear = 2.0f;
    p->use_occ = 1;
    return EPPM_OK;
}

static int cmap_new(int device, int h, int w, int nslots, const eppm_cmap_params* in, eppm_cmap** out)
{
    eppm_cmap_params def;
    eppm_cmap_default_params(&def);
    const eppm_cmap_params* p = in ? in : &def;
    CHK(cmap_params(p, "eppm_cmap_create"));
    CHK(cmap_size(h, w, "eppm_cmap_create"));
    eppm_cmap* f = new eppm_cmap;
    f->noun = "map";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->prm = *p;
    f->stride = up256(f->px() * 32);
    f->bytes = f->stride * nslots;
    const int rc = stage_open(f, "eppm_cmap_create");
    if (rc != EPPM_OK) {
        delete f;
        return rc;
    }
    f->cur.assign(nslots, 0);
    f->empty.assign(nslots, 1);
    f->deflayer.assign(nslots, 1);
    f->rendered.assign(nslots, 0);
    f->age.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_cmap_create(eppm_ctx* ctx, const eppm_cmap_params* in, eppm_cmap** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_cmap_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return cmap_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_cmap_create_size(int h, int w, int nslots, int device, const eppm_cmap_params* in, eppm_cmap** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_cmap_create_size: NULL argument");
    *out = nullptr;
    return cmap_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_cmap_destroy(eppm_cmap* f)
{
    if (!f) return EPPM_OK;
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_cmap_reset(eppm_cmap* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_cmap_reset: NULL map");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_cmap_reset"));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) {
            f->empty[k] = 1;
            f->rendered[k] = 0;
            f->age[k] = 0;
        }
    return EPPM_OK;
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s, and their render; in: the pairs' planes (the other members are filled in
// here); cut: NULL or one flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_cmap* f, CMapArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    const int n = in.n;
    fill_args(f, in, slot0, n, cut);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "cmap_step");
        launch_cmap_step(in, s);
    }
    HIPCHK(hipGetLastError());
    for (int k = slot0; k < slot0 + n; k++) {
        const bool c = cut && cut[k - slot0];
        f->cur[k] ^= 1;
        f->empty[k] = 0;
        f->age[k] = c ? 0 : f->age[k] + 1;
        f->rendered[k] = 1;
    }
    fill_args(f, in, slot0, n, nullptr);    // the render reads the map the step wrote
    {
        StageTimer t(timing, "cmap_render");
        launch_cmap_render(in, s);
    }
    return stage_leave(f, s);
}

extern "C" int eppm_cmap_step(eppm_cmap* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_cmap_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_cmap_step", &c, &s));
    CMapArgs in{};
    in.img1 = c.img1; in.img2 = c.img2; in.img_pitch = c.img_pitch; in.img_stride = c.img_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    return step_on(f, in, 0, cut, s, ctx);
}

// one step of one slot on caller planes, on the launcher stream
extern "C" int eppm_cmap_step_frames(eppm_cmap* f, int slot, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow_bwd,
                                     const uint8_t* d_occ2, int cut)
{
    if (!f || !d_rgba1 || !d_rgba2 || !d_flow_bwd || !d_occ2) return set_err(EPPM_ERR_ARG, "eppm_cmap_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_cmap_step_frames"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_cmap_step_frames: bad pitch %zu", pitch);
    return launcher_run(f, "eppm_cmap_step_frames", [&](hipStream_t s) {
        CMapArgs in{};
        in.img1 = (const uint8_t*)d_rgba1; in.img2 = (const uint8_t*)d_rgba2; in.img_pitch = pitch;
        in.bwd = (const float*)d_flow_bwd; in.occ2 = d_occ2;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    });
}

extern "C" int eppm_cmap_age(eppm_cmap* f, int slot)
{
    if (!f) {
        set_err(EPPM_ERR_ARG, "eppm_cmap_age: NULL map");
        return -1;
    }
    if (slot_check(f, slot, true, "eppm_cmap_age") != EPPM_OK) return -1;
    return f->age[slot];
}

extern "C" int eppm_cmap_get_state(eppm_cmap* f, int slot, float* xy)
{
    if (!f || !xy) return set_err(EPPM_ERR_ARG, "eppm_cmap_get_state: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_cmap_get_state"));
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(xy, f->map(slot, f->cur[slot]), f->px() * 8, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_cmap_set_state(eppm_cmap* f, int slot, const float* xy, const uint8_t* anchor_rgb, size_t row_stride)
{
    if (!f || !xy || !anchor_rgb) return set_err(EPPM_ERR_ARG, "eppm_cmap_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_cmap_set_state"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_cmap_set_state: row_stride %zu < 3*w", row_stride);
    CHK(stage_wait(f));
    std::vector<uint32_t> words;
    pack_words(words, anchor_rgb, row_stride, f->h, f->w, 3);
    HIPCHK(hipMemcpy(f->map(slot, f->cur[slot]), xy, f->px() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->words(slot, 0), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->words(slot, 1), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->empty[slot] = 0;
    f->rendered[slot] = 0;
    f->age[slot] = 0;
    return EPPM_OK;
}

extern "C" int eppm_cmap_set_layer(eppm_cmap* f, int slot, const uint8_t* rgba, size_t row_stride)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_cmap_set_layer: NULL map");
    CHK(slot_check(f, slot, false, "eppm_cmap_set_layer"));
    if (!rgba) {
        f->deflayer[slot] = 1;
        f->rendered[slot] = 0;
        return EPPM_OK;
    }
    if (row_stride < (size_t)f->w * 4) return set_err(EPPM_ERR_ARG, "eppm_cmap_set_layer: row_stride %zu < 4*w", row_stride);
    CHK(stage_wait(f));
    std::vector<uint32_t> words;
    pack_words(words, rgba, row_stride, f->h, f->w, 4);
    HIPCHK(hipMemcpy(f->words(slot, 2), words.data(), f->px() * 4, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->deflayer[slot] = 0;
    f->rendered[slot] = 0;
    return EPPM_OK;
}

extern "C" int eppm_cmap_render(eppm_cmap* f, int slot, uint8_t* rgb, size_t row_stride)
{
    if (!f || !rgb) return set_err(EPPM_ERR_ARG, "eppm_cmap_render: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_cmap_render"));
    if (row_stride < (size_t)f->w * 3) return set_err(EPPM_ERR_ARG, "eppm_cmap_render: row_stride %zu < 3*w", row_stride);
    CHK(render_slot(f, slot));
    return stage_get_rgb(f, f->words(slot, 3), f->h, f->w, rgb, row_stride);
}

extern "C" int eppm_cmap_render_device(eppm_cmap* f, int slot, void* d_rgba, size_t pitch)
{
    if (!f || !d_rgba) return set_err(EPPM_ERR_ARG, "eppm_cmap_render_device: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_cmap_render_device"));
    if (bad_pitch(pitch, f->w)) return set_err(EPPM_ERR_ARG, "eppm_cmap_render_device: bad pitch %zu", pitch);
    CHK(render_slot(f, slot));
    return stage_get_rgba_device(f, f->words(slot, 3), f->h, f->w, d_rgba, pitch);
}

// ---- host forms: the same step and render as sequential loops ----
namespace {

struct HostRgb {          // a packed RGB image as words
    const uint8_t* rgb;
    int w;
    uint32_t operator()(int x, int y) const
    {
        const uint8_t* q = rgb + ((size_t)y * w + x) * 3;
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    }
};

struct HostLayer {        // RGBA bytes, or a packed RGB image with alpha 255
    const uint8_t* rgba;
    const uint8_t* rgb;
    int w;
    uint32_t operator()(int x, int y) const
    {
        if (!rgba) return HostRgb{rgb, w}(x, y) | 255u << 24;
        const uint8_t* q = rgba + ((size_t)y * w + x) * 4;
        return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
};

struct HostMap {          // h*w (x, y) floats, or the seed
    const float* xy;
    int w;
    CmPt operator()(int x, int y) const
    {
        if (!xy) return CmPt{(float)x, (float)y};
        const float* q = xy + ((size_t)y * w + x) * 2;
        return CmPt{q[0], q[1]};
    }
};

}  // namespace

extern "C" int eppm_cmap_step_host(const eppm_cmap_params* p, float* map_out, const float* map_in, const uint8_t* anchor_rgb, const uint8_t* rgb2,
                                   const float* bu, const float* bv, const uint8_t* occ2, int h, int w, int cut)
{
    CHK(cmap_params(p, "eppm_cmap_step_host"));
    if (!map_out || !anchor_rgb || !rgb2 || !bu || !bv || !occ2) return set_err(EPPM_ERR_ARG, "eppm_cmap_step_host: NULL argument");
    if (map_out == map_in) return set_err(EPPM_ERR_ARG, "eppm_cmap_step_host: the step gathers, map_out must not be map_in");
    CHK(cmap_size(h, w, "eppm_cmap_step_host"));
    const HostMap M{map_in, w};
    const HostRgb A{anchor_rgb, w}, cur{rgb2, w};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const CmPt s = cmap_step_pixel(x, y, cur(x, y), bu[i], bv[i], occ2[i], cut != 0, h, w, p->thresh, p->tear, p->use_occ, M, A);
            map_out[2 * i] = s.x; map_out[2 * i + 1] = s.y;
        }
    return EPPM_OK;
}

extern "C" int eppm_cmap_render_host(uint8_t* rgb_out, const float* map, const uint8_t* rgb_cur, const uint8_t* layer_rgba, const uint8_t* anchor_rgb,
                                     int h, int w)
{
    if (!rgb_out || !map || !rgb_cur || (!layer_rgba && !anchor_rgb)) return set_err(EPPM_ERR_ARG, "eppm_cmap_render_host: NULL argument");
    CHK(cmap_size(h, w, "eppm_cmap_render_host"));
    const HostLayer L{layer_rgba, anchor_rgb, w};
    const HostRgb cur{rgb_cur, w};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            const uint32_t o = cmap_render_pixel(cur(x, y), CmPt{map[2 * i], map[2 * i + 1]}, h, w, L);
            rgb_out[3 * i] = (uint8_t)o; rgb_out[3 * i + 1] = (uint8_t)(o >> 8); rgb_out[3 * i + 2] = (uint8_t)(o >> 16);
        }
    return EPPM_OK;
}
