// objects.cpp -- moving-object detection: eppm_objects (a stage object, stage_object.h), its private stabiliser,
// its step on a context's pairs or on caller planes (the kernels: k_objects.hip), the synchronous calls, and the host forms eppm_objects_label_host /
// eppm_objects_carry_host / eppm_objects_assign_host, which are objects.h's sequential code behind argument checks.
#include "stage_object.h"
#include "objects.h"

using namespace eppm;

static_assert(sizeof(ObjRecord) == 64 && sizeof(eppm_object) == sizeof(ObjRecord), "a record is the public eppm_object");
static_assert(sizeof(ObjCounts) == sizeof(eppm_objects_counts) && sizeof(ObjHeader) == 32, "the counts head a slot's 32-byte header");

struct eppm_objects : StageObject {     // mem: nslots blocks `stride` bytes apart: ObjArgs' layout
    eppm_objects_params prm{};
    eppm_stab* stab = nullptr;          // the private stabiliser whose mask the context form labels
    size_t stride = 0, off_root = 0, off_area = 0, off_labels = 0, off_carried = 0, off_chunks = 0, off_rec = 0, off_votes = 0, off_hdr = 0;
    int tiles_x = 0, tiles_y = 0, nchunks = 0;
    std::vector<uint8_t> empty, stepped;    // per slot: it has no state (carried plane zero, next_id 1) / it has labels and records
    char* block(int slot) const { return mem + (size_t)slot * stride; }
    ObjHeader* hdr(int slot) const { return (ObjHeader*)(block(slot) + off_hdr); }
    int32_t* prev(int slot, int which) const { return (int32_t*)(block(slot) + off_hdr + sizeof(ObjHeader)) + which * kObjTable; }
    uint8_t* labels(int slot) const { return (uint8_t*)(block(slot) + off_labels); }
    uint8_t* carried(int slot) const { return (uint8_t*)(block(slot) + off_carried); }
    ObjRecord* rec(int slot) const { return (ObjRecord*)(block(slot) + off_rec); }
};

namespace {

int objects_params(const eppm_objects_params* p, const char* what)
{
    if (!p) return set_err(EPPM_ERR_ARG, "%s: NULL parameters", what);
    if (!(p->tau > 0.0f && p->tau <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "%s: tau must be finite and > 0", what);
    if (p->iters < 1 || p->iters > 8) return set_err(EPPM_ERR_ARG, "%s: iters %d outside [1, 8]", what, p->iters);
    if (!obj_params_ok(p->connectivity, p->min_area, p->max_objects, p->min_overlap))
        return set_err(EPPM_ERR_ARG, "%s: connectivity 4 or 8, min_area >= 1, max_objects in [1, %d], min_overlap >= 1", what, kObjMaxObjects);
    return EPPM_OK;
}

int size_check(int h, int w, const char* what)
{
    if (!obj_size_ok(h, w)) return set_err(EPPM_ERR_ARG, "%s: size %dx%d out of range (w, h <= %d, h*w <= 2^26)", what, w, h, kObjMaxDim);
    return EPPM_OK;
}

int slot_check(const eppm_objects* f, int slot, bool need_step, const char* what)
{
    CHK(stage_slot_check(f, slot, what));
    if (need_step && !f->stepped[slot]) return set_err(EPPM_ERR_STATE, "%s: slot %d has not been stepped", what, slot);
    return EPPM_OK;
}

// the slot's header, after the last step; an error word that is set is the call's failure
int header(eppm_objects* f, int slot, ObjHeader* hd, const char* what)
{
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(hd, f->hdr(slot), sizeof *hd, hipMemcpyDeviceToHost));
    if (hd->err)
        return set_err(EPPM_ERR_STATE, "%s: a labelling loop hit its iteration cap in slot %d (a defect of the library): its results are invalid until eppm_objects_reset", what, slot);
    return EPPM_OK;
}

}  // namespace

extern "C" int eppm_objects_default_params(eppm_objects_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_objects_default_params: NULL");
    p->tau = 1.0f;
    p->iters = 3;
    p->connectivity = 8;
    p->min_area = 16;
    p->max_objects = 64;
    p->min_overlap = 4;
    return EPPM_OK;
}

static int objects_new(int device, int h, int w, int nslots, const eppm_objects_params* in, eppm_objects** out)
{
    eppm_objects_params def;
    eppm_objects_default_params(&def);
    const eppm_objects_params* p = in ? in : &def;
    CHK(objects_params(p, "eppm_objects_create"));
    CHK(size_check(h, w, "eppm_objects_create"));
    eppm_objects* f = new eppm_objects;
    f->noun = "detector";
    f->device = device; f->h = h; f->w = w; f->nslots = nslots;
    f->prm = *p;
    f->tiles_x = (w + kObjTileW - 1) / kObjTileW;
    f->tiles_y = (h + kObjTileH - 1) / kObjTileH;
    f->nchunks = (int)((f->px() + kObjChunk - 1) / kObjChunk);
    const size_t words = up256(f->px() * 4), bytes = up256(f->px()), votes = (size_t)(p->max_objects + 1) * (p->max_objects + 1) * 4;
    f->off_root = words;
    f->off_area = 2 * words;
    f->off_labels = 3 * words;
    f->off_carried = f->off_labels + bytes;
    f->off_chunks = f->off_carried + bytes;
    f->off_rec = f->off_chunks + up256((size_t)f->nchunks * 8);
    f->off_votes = f->off_rec + (size_t)kObjTable * sizeof(ObjRecord);
    f->off_hdr = f->off_votes + up256(votes);
    f->stride = f->off_hdr + up256(sizeof(ObjHeader) + 2 * kObjTable * sizeof(int32_t));
    f->bytes = f->stride * nslots;
    eppm_stab_params sp;
    eppm_stab_default_params(&sp);
    sp.tau = p->tau;
    sp.iters = p->iters;
    int rc = stage_open(f, "eppm_objects_create", [f] {
        hipError_t e = hipSuccess;
        for (int k = 0; k < f->nslots && e == hipSuccess; k++) e = hipMemsetAsync(f->hdr(k), 0, sizeof(ObjHeader) + 2 * kObjTable * sizeof(int32_t), nullptr);
        return e;
    });
    if (rc == EPPM_OK) rc = eppm_stab_create_size(h, w, nslots, device, &sp, &f->stab);
    if (rc != EPPM_OK) {
        eppm_objects_destroy(f);
        return rc;
    }
    f->empty.assign(nslots, 1);
    f->stepped.assign(nslots, 0);
    *out = f;
    return EPPM_OK;
}

extern "C" int eppm_objects_create(eppm_ctx* ctx, const eppm_objects_params* in, eppm_objects** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_objects_create: NULL argument");
    *out = nullptr;
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    return objects_new(device, h, w, eppm_batch_size(ctx), in, out);
}

extern "C" int eppm_objects_create_size(int h, int w, int nslots, int device, const eppm_objects_params* in, eppm_objects** out)
{
    if (!out) return set_err(EPPM_ERR_ARG, "eppm_objects_create_size: NULL argument");
    *out = nullptr;
    return objects_new(device, h, w, nslots, in, out);
}

extern "C" int eppm_objects_destroy(eppm_objects* f)
{
    if (!f) return EPPM_OK;
    eppm_stab_destroy(f->stab);
    stage_close(f);
    delete f;
    return EPPM_OK;
}

extern "C" int eppm_objects_reset(eppm_objects* f, int slot)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_objects_reset: NULL detector");
    if (slot >= 0) CHK(stage_slot_check(f, slot, "eppm_objects_reset"));
    CHK(stage_wait(f));
    for (int k = 0; k < f->nslots; k++)
        if (slot < 0 || k == slot) {
            HIPCHK(hipMemset(f->hdr(k), 0, sizeof(ObjHeader)));      // the error word too
            f->empty[k] = 1;
            f->stepped[k] = 0;
        }
    CHK(eppm_stab_reset(f->stab, slot));
    return stage_settle(f);
}

// one step of slots slot0 .. slot0 + in.n - 1 on stream s; in: the pairs' planes (the other members are filled in here); cut: NULL or one
// flag per pair.  timing: the context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_objects* f, ObjArgs& in, int slot0, const uint8_t* cut, hipStream_t s, eppm_ctx* timing)
{
    in.mem = f->mem;
    in.slot_stride = f->stride;
    in.off_root = f->off_root; in.off_area = f->off_area; in.off_labels = f->off_labels; in.off_carried = f->off_carried;
    in.off_chunks = f->off_chunks; in.off_rec = f->off_rec; in.off_votes = f->off_votes; in.off_hdr = f->off_hdr;
    in.h = f->h; in.w = f->w; in.slot0 = slot0;
    in.tiles_x = f->tiles_x; in.tiles_y = f->tiles_y; in.nchunks = f->nchunks;
    in.connectivity = f->prm.connectivity; in.min_area = f->prm.min_area; in.max_objects = f->prm.max_objects; in.min_overlap = f->prm.min_overlap;
    slot_mask(in.empty, f->empty.data() + slot0, slot0, in.n);
    slot_mask(in.cut, cut, slot0, in.n);
    CHK(stage_enter(f, s));
    {
        StageTimer t(timing, "objects_label");
        launch_objects_label(in, s);
    }
    {
        StageTimer t(timing, "objects_assign");
        launch_objects_assign(in, s);
    }
    CHK(stage_leave(f, s));
    for (int k = slot0; k < slot0 + in.n; k++) f->empty[k] = 0, f->stepped[k] = 1;
    return EPPM_OK;
}

extern "C" int eppm_objects_step(eppm_objects* f, eppm_ctx* ctx, const uint8_t* cut)
{
    if (!f || !ctx) return set_err(EPPM_ERR_ARG, "eppm_objects_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, f, "eppm_objects_step", &c, &s));
    ObjArgs in{};
    in.fwd = c.fwd; in.fwd_stride = c.fwd_stride;
    in.bwd = c.bwd; in.bwd_stride = c.bwd_stride;
    in.occ2 = c.occ2; in.occ_stride = c.occ_stride;
    in.n = c.n;
    {
        StageTimer t(ctx, "objects_fit");
        StabArgs sin = stab_ctx_args(c);
        CHK(stab_step_on(f->stab, sin, 0, cut, s, nullptr));
    }
    in.mask = stab_mask_device(f->stab, &in.mask_stride);
    return step_on(f, in, 0, cut, s, ctx);
}

// the kernels alone for one slot on caller planes, without a fit, on the launcher stream; then the slot's error word
extern "C" int eppm_objects_step_frames(eppm_objects* f, int slot, const uint8_t* d_mask, const eppm_float2* d_flow, const eppm_float2* d_flow_bwd,
                                        const uint8_t* d_occ2, int cut)
{
    if (!f || !d_mask || !d_flow) return set_err(EPPM_ERR_ARG, "eppm_objects_step_frames: NULL argument");
    CHK(stage_slot_check(f, slot, "eppm_objects_step_frames"));
    CHK(launcher_run(f, "eppm_objects_step_frames", [&](hipStream_t s) {
        ObjArgs in{};
        in.mask = d_mask; in.fwd = (const float*)d_flow;
        if (d_flow_bwd && d_occ2) in.bwd = (const float*)d_flow_bwd, in.occ2 = d_occ2;
        in.n = 1;
        const uint8_t c = cut != 0;
        return step_on(f, in, slot, &c, s, nullptr);
    }));
    ObjHeader hd;
    return header(f, slot, &hd, "eppm_objects_step_frames");
}

extern "C" int eppm_objects_get(eppm_objects* f, int slot, int max, eppm_object* records, eppm_objects_counts* counts)
{
    if (!f) return set_err(EPPM_ERR_ARG, "eppm_objects_get: NULL detector");
    if (max < 0 || (max > 0 && !records)) return set_err(EPPM_ERR_ARG, "eppm_objects_get: %d records into a NULL array", max);
    CHK(slot_check(f, slot, true, "eppm_objects_get"));
    ObjHeader hd;
    CHK(header(f, slot, &hd, "eppm_objects_get"));
    const int n = hd.n < max ? hd.n : max;
    if (n > 0 && records) HIPCHK(hipMemcpy(records, f->rec(slot) + 1, (size_t)n * sizeof(ObjRecord), hipMemcpyDeviceToHost));
    if (counts) {
        counts->n = hd.n; counts->n_found = hd.n_found; counts->n_components = hd.n_components; counts->next_id = hd.next_id;
    }
    return EPPM_OK;
}

extern "C" int eppm_objects_get_labels(eppm_objects* f, int slot, uint8_t* labels)
{
    if (!f || !labels) return set_err(EPPM_ERR_ARG, "eppm_objects_get_labels: NULL argument");
    CHK(slot_check(f, slot, true, "eppm_objects_get_labels"));
    ObjHeader hd;
    CHK(header(f, slot, &hd, "eppm_objects_get_labels"));
    HIPCHK(hipMemcpy(labels, f->labels(slot), f->px(), hipMemcpyDeviceToHost));
    return EPPM_OK;
}

extern "C" int eppm_objects_get_state(eppm_objects* f, int slot, uint8_t* carried, int32_t* prev_id, int32_t* prev_age, int32_t* next_id)
{
    if (!f || !carried || !prev_id || !prev_age || !next_id) return set_err(EPPM_ERR_ARG, "eppm_objects_get_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_objects_get_state"));
    if (f->empty[slot]) {
        memset(carried, 0, f->px());
        memset(prev_id, 0, kObjTable * sizeof(int32_t));
        memset(prev_age, 0, kObjTable * sizeof(int32_t));
        *next_id = 1;
        return EPPM_OK;
    }
    ObjHeader hd;
    CHK(header(f, slot, &hd, "eppm_objects_get_state"));
    HIPCHK(hipMemcpy(carried, f->carried(slot), f->px(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(prev_id, f->prev(slot, 0), kObjTable * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(prev_age, f->prev(slot, 1), kObjTable * sizeof(int32_t), hipMemcpyDeviceToHost));
    *next_id = hd.next_id;
    return EPPM_OK;
}

extern "C" int eppm_objects_set_state(eppm_objects* f, int slot, const uint8_t* carried, const int32_t* prev_id, const int32_t* prev_age, int32_t next_id)
{
    if (!f || !carried || !prev_id || !prev_age) return set_err(EPPM_ERR_ARG, "eppm_objects_set_state: NULL argument");
    CHK(slot_check(f, slot, false, "eppm_objects_set_state"));
    if (next_id < 1 || next_id > kObjMaxNextId) return set_err(EPPM_ERR_ARG, "eppm_objects_set_state: next_id %d outside [1, 2^30]", next_id);
    for (int k = 0; k < kObjTable; k++)
        if (prev_age[k] < 0 || prev_age[k] > kObjMaxNextId) return set_err(EPPM_ERR_ARG, "eppm_objects_set_state: age %d outside [0, 2^30]", prev_age[k]);
    CHK(stage_wait(f));
    HIPCHK(hipMemcpy(f->carried(slot), carried, f->px(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->prev(slot, 0), prev_id, kObjTable * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->prev(slot, 1), prev_age, kObjTable * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(&f->hdr(slot)->next_id, &next_id, sizeof next_id, hipMemcpyHostToDevice));
    CHK(stage_settle(f));
    f->empty[slot] = 0;
    return EPPM_OK;
}

// ---- host forms: objects.h's sequential code ----
extern "C" int eppm_objects_label_host(const eppm_objects_params* p, const uint8_t* mask, const float* u, const float* v, int h, int w, uint8_t* labels,
                                       eppm_object* records, eppm_objects_counts* counts)
{
    CHK(objects_params(p, "eppm_objects_label_host"));
    if (!mask || !u || !v || !labels || !records || !counts) return set_err(EPPM_ERR_ARG, "eppm_objects_label_host: NULL argument");
    CHK(size_check(h, w, "eppm_objects_label_host"));
    ObjCounts c{0, 0, 0, counts->next_id};
    obj_label_host(mask, u, v, h, w, p->connectivity, p->min_area, p->max_objects, labels, reinterpret_cast<ObjRecord*>(records), &c);
    counts->n = c.n; counts->n_found = c.n_found; counts->n_components = c.n_components;
    return EPPM_OK;
}

extern "C" int eppm_objects_carry_host(const uint8_t* labels, const float* bu, const float* bv, const uint8_t* occ2, int h, int w, uint8_t* carried)
{
    if (!labels || !bu || !bv || !occ2 || !carried) return set_err(EPPM_ERR_ARG, "eppm_objects_carry_host: NULL argument");
    if (labels == carried) return set_err(EPPM_ERR_ARG, "eppm_objects_carry_host: the carry gathers, carried must not be labels");
    CHK(size_check(h, w, "eppm_objects_carry_host"));
    obj_carry_host(labels, bu, bv, occ2, h, w, carried);
    return EPPM_OK;
}

extern "C" int eppm_objects_assign_host(const eppm_objects_params* p, const uint8_t* labels, const uint8_t* carried, int h, int w, int n, int32_t* prev_id,
                                        int32_t* prev_age, int32_t* next_id, eppm_object* records)
{
    CHK(objects_params(p, "eppm_objects_assign_host"));
    if (!labels || !prev_id || !prev_age || !next_id || (n > 0 && !records)) return set_err(EPPM_ERR_ARG, "eppm_objects_assign_host: NULL argument");
    CHK(size_check(h, w, "eppm_objects_assign_host"));
    if (n < 0 || n > p->max_objects) return set_err(EPPM_ERR_ARG, "eppm_objects_assign_host: %d objects outside [0, max_objects]", n);
    if (*next_id < 1 || *next_id > kObjMaxNextId) return set_err(EPPM_ERR_ARG, "eppm_objects_assign_host: next_id %d outside [1, 2^30]", *next_id);
    for (int k = 0; k < kObjTable; k++)
        if (prev_age[k] < 0 || prev_age[k] > kObjMaxNextId) return set_err(EPPM_ERR_ARG, "eppm_objects_assign_host: age %d outside [0, 2^30]", prev_age[k]);
    obj_assign_host(labels, carried, (size_t)h * w, n, p->max_objects, p->min_overlap, prev_id, prev_age, next_id, reinterpret_cast<ObjRecord*>(records));
    return EPPM_OK;
}
