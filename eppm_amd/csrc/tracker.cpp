// tracker.cpp -- dense point trajectories: eppm_tracker (a stage object of one slot, stage_object.h), its steps on a
// context's pair or on caller planes (the kernels: k_track.hip), the synchronous state calls, and the host form eppm_track_step_host.  The host form shares track.h's per-point
// arithmetic with the kernels; its lists are built by sequential loops with running counters, independent of the kernels' scans.
#include "stage_object.h"
#include "track.h"

using namespace eppm;

struct eppm_tracker : StageObject {
    int cap = 0, ncells = 0, ncx = 0;
    int cur = 0;                        // which of the two lists holds the live tracks
    int frame = 0;                      // the device frame counter as the steps enqueued so far leave it (the frame-0 pass is skipped otherwise)
    TrackRec* list[2] = {nullptr, nullptr};
    TrackDev d{};
};

namespace {

constexpr long long kMaxMinEig = 1LL << 40;
constexpr int kMaxCapacity = 1 << 26;

// checked parameters; *cap: the capacity after the default
int track_params(const eppm_track_params* in, int h, int w, TrackParams* p, int* cap, int* ncx, int* ncy)
{
    if (!in) return set_err(EPPM_ERR_ARG, "track: NULL parameters");
    if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return set_err(EPPM_ERR_ARG, "track: size %dx%d out of range", w, h);
    if (in->spacing < 1) return set_err(EPPM_ERR_ARG, "track: spacing %d < 1", in->spacing);
    if (in->min_eig < 0 || in->min_eig > kMaxMinEig) return set_err(EPPM_ERR_ARG, "track: min_eig %lld outside [0, 2^40]", (long long)in->min_eig);
    const float f[4] = {in->fb_alpha, in->fb_beta, in->mb_alpha, in->mb_beta};
    for (float x : f)
        if (!(x >= 0.0f && x <= 3.4e38f)) return set_err(EPPM_ERR_ARG, "track: the check parameters must be finite and >= 0");
    const long long cx = (w + (long long)in->spacing - 1) / in->spacing, cy = (h + (long long)in->spacing - 1) / in->spacing;
    const long long c = in->capacity ? in->capacity : 4 * cx * cy;
    if (in->capacity < 0 || c > kMaxCapacity) return set_err(EPPM_ERR_ARG, "track: capacity %lld outside [1, 2^26]", c);
    p->spacing = in->spacing;
    p->min_eig = in->min_eig;
    p->fb_alpha = in->fb_alpha; p->fb_beta = in->fb_beta; p->mb_alpha = in->mb_alpha; p->mb_beta = in->mb_beta;
    *cap = (int)c;
    *ncx = (int)cx;
    *ncy = (int)cy;
    return EPPM_OK;
}

bool in_frame(float x, float y, int h, int w) { return x >= 0.0f && x <= (float)(w - 1) && y >= 0.0f && y <= (float)(h - 1); }

int read_counts(eppm_tracker* t, int32_t* cnt)
{
    HIPCHK(hipMemcpy(cnt, t->d.cnt, kTrackCntN * 4, hipMemcpyDeviceToHost));
    return EPPM_OK;
}

void to_counts(const int32_t* cnt, eppm_track_counts* out)
{
    out->live = cnt[kTrackCntLive];
    out->ended = cnt[kTrackCntEnded];
    out->seeded = cnt[kTrackCntSeeded];
    out->dropped = cnt[kTrackCntDropped];
    out->frame = cnt[kTrackCntFrame];
    out->next_id = cnt[kTrackCntNextId];
}

}  // namespace

extern "C" int eppm_track_default_params(eppm_track_params* p)
{
    if (!p) return set_err(EPPM_ERR_ARG, "eppm_track_default_params: NULL");
    p->spacing = 8;
    p->min_eig = 2500;
    p->fb_alpha = 0.01f;
    p->fb_beta = 0.5f;
    p->mb_alpha = 0.01f;
    p->mb_beta = 0.002f;
    p->capacity = 0;
    return EPPM_OK;
}

extern "C" int eppm_track_capacity(const eppm_track_params* in, int h, int w)
{
    TrackParams p;
    int cap, ncx, ncy;
    return track_params(in, h, w, &p, &cap, &ncx, &ncy) == EPPM_OK ? cap : -1;
}

extern "C" int eppm_tracker_create(eppm_ctx* ctx, const eppm_track_params* in, eppm_tracker** out)
{
    if (!ctx || !out) return set_err(EPPM_ERR_ARG, "eppm_tracker_create: NULL argument");
    *out = nullptr;
    eppm_track_params def;
    eppm_track_default_params(&def);
    int h, w;
    const int device = ctx_device(ctx, &h, &w);
    TrackParams p;
    int cap, ncx, ncy;
    CHK(track_params(in ? in : &def, h, w, &p, &cap, &ncx, &ncy));
    const int ncells = ncx * ncy, nbs = (cap + 255) / 256, nbc = (ncells + 255) / 256;
    // list | list | ended | ended_reason | npos | stat | cov | flags | blk_s | blk_e | blk_c | counters, each 256-byte aligned
    const size_t sz[12] = {(size_t)cap * 16, (size_t)cap * 16, (size_t)cap * 16, (size_t)cap * 4, (size_t)cap * 8, (size_t)cap, (size_t)ncells,
                           (size_t)ncells, (size_t)nbs * 4, (size_t)nbs * 4, (size_t)nbc * 4, (size_t)kTrackCntN * 4};
    size_t off[12], bytes = 0;
    for (int i = 0; i < 12; i++) {
        off[i] = bytes;
        bytes += up256(sz[i]);
    }
    eppm_tracker* t = new eppm_tracker;
    t->noun = "tracker";
    t->device = device; t->h = h; t->w = w; t->nslots = 1; t->bytes = bytes;
    t->cap = cap; t->ncells = ncells; t->ncx = ncx;
    const int rc = stage_open(t, "eppm_tracker_create", [t] {
        const hipError_t e = hipMemsetAsync(t->mem, 0, t->bytes, nullptr);
        return e == hipSuccess ? hipStreamSynchronize(nullptr) : e;
    });
    if (rc != EPPM_OK) {
        delete t;
        return rc;
    }
    char* m = t->mem;
    t->list[0] = (TrackRec*)(m + off[0]);
    t->list[1] = (TrackRec*)(m + off[1]);
    TrackDev& d = t->d;
    d.p.spacing = p.spacing; d.p.min_eig = p.min_eig;
    d.p.fb_alpha = p.fb_alpha; d.p.fb_beta = p.fb_beta; d.p.mb_alpha = p.mb_alpha; d.p.mb_beta = p.mb_beta;
    d.cap = cap; d.ncells = ncells; d.ncx = ncx;
    d.ended = (TrackRec*)(m + off[2]);
    d.ended_reason = (int32_t*)(m + off[3]);
    d.npos = (float*)(m + off[4]);
    d.stat = (uint8_t*)(m + off[5]);
    d.cov = (uint8_t*)(m + off[6]);
    d.flags = (uint8_t*)(m + off[7]);
    d.blk_s = (int32_t*)(m + off[8]);
    d.blk_e = (int32_t*)(m + off[9]);
    d.blk_c = (int32_t*)(m + off[10]);
    d.cnt = (int32_t*)(m + off[11]);
    *out = t;
    return EPPM_OK;
}

extern "C" int eppm_tracker_destroy(eppm_tracker* t)
{
    if (!t) return EPPM_OK;
    stage_close(t);
    delete t;
    return EPPM_OK;
}

// one step on stream s: the frame-0 seeding pass (only while the frame counter is 0), advance, seed flags, compaction.  timing: the
// context whose stage-timing entries receive the stages, or NULL
static int step_on(eppm_tracker* t, const TrackIn& in, hipStream_t s, eppm_ctx* timing)
{
    TrackRec* cur = t->list[t->cur];
    TrackRec* next = t->list[t->cur ^ 1];
    CHK(stage_enter(t, s));
    if (t->frame == 0) {
        StageTimer tm(timing, "track_seed");
        launch_track_seed0(t->d, in, cur, s);
    }
    {
        StageTimer tm(timing, "track_advance");
        launch_track_advance(t->d, in, cur, s);
    }
    {
        StageTimer tm(timing, "track_seed");
        launch_track_seed(t->d, in, s);
    }
    {
        StageTimer tm(timing, "track_compact");
        launch_track_compact(t->d, in, cur, next, s);
    }
    CHK(stage_leave(t, s));
    t->cur ^= 1;
    t->frame++;
    return EPPM_OK;
}

extern "C" int eppm_track_step(eppm_tracker* t, eppm_ctx* ctx, int pair)
{
    if (!t || !ctx) return set_err(EPPM_ERR_ARG, "eppm_track_step: NULL argument");
    CtxPlanes c;
    hipStream_t s;
    CHK(ctx_stage_inputs(ctx, t, "eppm_track_step", &c, &s, &pair));
    return step_on(t, TrackIn{c.img1, c.img2, c.img_pitch, c.fwd, c.bwd, t->h, t->w}, s, ctx);
}

// one step on caller planes, on the launcher stream
extern "C" int eppm_track_step_frames(eppm_tracker* t, const void* d_rgba1, const void* d_rgba2, size_t pitch, const eppm_float2* d_flow,
                                      const eppm_float2* d_flow_bwd, int h, int w)
{
    if (!t || !d_rgba1 || !d_rgba2 || !d_flow || !d_flow_bwd) return set_err(EPPM_ERR_ARG, "eppm_track_step_frames: NULL argument");
    if (h != t->h || w != t->w) return set_err(EPPM_ERR_ARG, "eppm_track_step_frames: %dx%d planes, the tracker is %dx%d", w, h, t->w, t->h);
    if (bad_pitch(pitch, w)) return set_err(EPPM_ERR_ARG, "eppm_track_step_frames: bad pitch %zu", pitch);
    return launcher_run(t, "eppm_track_step_frames", [&](hipStream_t s) {
        return step_on(t, TrackIn{(const uint8_t*)d_rgba1, (const uint8_t*)d_rgba2, pitch, (const float*)d_flow, (const float*)d_flow_bwd, h, w}, s, nullptr);
    });
}

extern "C" int eppm_tracker_get(eppm_tracker* t, int max, int32_t* ids, int32_t* starts, float* xy, eppm_track_counts* counts)
{
    if (!t || max < 0) return set_err(EPPM_ERR_ARG, "eppm_tracker_get: bad argument");
    CHK(stage_wait(t));
    int32_t cnt[kTrackCntN];
    CHK(read_counts(t, cnt));
    if (counts) to_counts(cnt, counts);
    const int n = cnt[kTrackCntLive] < max ? cnt[kTrackCntLive] : max;
    if (n > 0 && (ids || starts || xy)) {
        std::vector<TrackRec> r(n);
        HIPCHK(hipMemcpy(r.data(), t->list[t->cur], (size_t)n * sizeof(TrackRec), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            if (ids) ids[i] = r[i].id;
            if (starts) starts[i] = r[i].start;
            if (xy) { xy[2 * i] = r[i].x; xy[2 * i + 1] = r[i].y; }
        }
    }
    return EPPM_OK;
}

extern "C" int eppm_tracker_get_ended(eppm_tracker* t, int max, int32_t* ids, int32_t* starts, float* xy, int32_t* reasons, eppm_track_counts* counts)
{
    if (!t || max < 0) return set_err(EPPM_ERR_ARG, "eppm_tracker_get_ended: bad argument");
    CHK(stage_wait(t));
    int32_t cnt[kTrackCntN];
    CHK(read_counts(t, cnt));
    if (counts) to_counts(cnt, counts);
    const int n = cnt[kTrackCntEnded] < max ? cnt[kTrackCntEnded] : max;
    if (n > 0 && (ids || starts || xy || reasons)) {
        std::vector<TrackRec> r(n);
        std::vector<int32_t> why(n);
        HIPCHK(hipMemcpy(r.data(), t->d.ended, (size_t)n * sizeof(TrackRec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(why.data(), t->d.ended_reason, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            if (ids) ids[i] = r[i].id;
            if (starts) starts[i] = r[i].start;
            if (xy) { xy[2 * i] = r[i].x; xy[2 * i + 1] = r[i].y; }
            if (reasons) reasons[i] = why[i];
        }
    }
    return EPPM_OK;
}

extern "C" int eppm_tracker_set(eppm_tracker* t, int n, const int32_t* ids, const int32_t* starts, const float* xy, int next_id, int frame)
{
    if (!t) return set_err(EPPM_ERR_ARG, "eppm_tracker_set: NULL tracker");
    if (n < 0 || n > t->cap) return set_err(EPPM_ERR_ARG, "eppm_tracker_set: %d tracks, capacity %d", n, t->cap);
    if (n > 0 && (!ids || !starts || !xy)) return set_err(EPPM_ERR_ARG, "eppm_tracker_set: NULL arrays");
    if (next_id < 0 || frame < 0) return set_err(EPPM_ERR_ARG, "eppm_tracker_set: next_id %d, frame %d", next_id, frame);
    std::vector<TrackRec> r(n);
    for (int i = 0; i < n; i++) {
        if (!in_frame(xy[2 * i], xy[2 * i + 1], t->h, t->w))
            return set_err(EPPM_ERR_ARG, "eppm_tracker_set: track %d at (%g, %g) outside the frame", i, xy[2 * i], xy[2 * i + 1]);
        r[i] = TrackRec{ids[i], starts[i], xy[2 * i], xy[2 * i + 1]};
    }
    CHK(stage_wait(t));
    if (n > 0) HIPCHK(hipMemcpy(t->list[t->cur], r.data(), (size_t)n * sizeof(TrackRec), hipMemcpyHostToDevice));
    int32_t cnt[kTrackCntN] = {};
    cnt[kTrackCntLive] = n;
    cnt[kTrackCntNextId] = next_id;
    cnt[kTrackCntFrame] = frame;
    HIPCHK(hipMemcpy(t->d.cnt, cnt, sizeof(cnt), hipMemcpyHostToDevice));
    CHK(stage_settle(t));
    t->frame = frame;
    return EPPM_OK;
}

// ---- host form: the same step as sequential loops ----
extern "C" int eppm_track_step_host(const eppm_track_params* pin, const uint8_t* rgb1, const uint8_t* rgb2, const float* u, const float* v,
                                    const float* bu, const float* bv, int h, int w, int n, const int32_t* ids, const int32_t* starts,
                                    const float* xy, int next_id, int frame, int32_t* out_ids, int32_t* out_starts, float* out_xy,
                                    int32_t* end_ids, int32_t* end_starts, float* end_xy, int32_t* end_reasons, eppm_track_counts* counts)
{
    TrackParams p;
    int cap, ncx, ncy;
    CHK(track_params(pin, h, w, &p, &cap, &ncx, &ncy));
    if (!rgb1 || !rgb2 || !u || !v || !bu || !bv || !out_ids || !out_starts || !out_xy || !end_ids || !end_starts || !end_xy || !end_reasons ||
        !counts)
        return set_err(EPPM_ERR_ARG, "eppm_track_step_host: NULL argument");
    if (n < 0 || n > cap || (n > 0 && (!ids || !starts || !xy)) || next_id < 0 || frame < 0)
        return set_err(EPPM_ERR_ARG, "eppm_track_step_host: bad state (n %d, capacity %d)", n, cap);
    for (int i = 0; i < n; i++)
        if (!in_frame(xy[2 * i], xy[2 * i + 1], h, w)) return set_err(EPPM_ERR_ARG, "eppm_track_step_host: track %d outside the frame", i);
    const int s = p.spacing, ncells = ncx * ncy;
    auto grey = [w](const uint8_t* img) {
        return [img, w](int x, int y) { const uint8_t* q = img + ((size_t)y * w + x) * 3; return (int)q[0] + (int)q[1] + (int)q[2]; };
    };
    const auto g1 = grey(rgb1), g2 = grey(rgb2);
    auto F = [u, v, w](int x, int y, float* a, float* b) { *a = u[(size_t)y * w + x]; *b = v[(size_t)y * w + x]; };
    auto G = [bu, bv, w](int x, int y, float* a, float* b) { *a = bu[(size_t)y * w + x]; *b = bv[(size_t)y * w + x]; };

    std::vector<TrackRec> cur;
    cur.reserve(cap);
    for (int i = 0; i < n; i++) cur.push_back(TrackRec{ids[i], starts[i], xy[2 * i], xy[2 * i + 1]});
    int next = next_id, seeded = 0, dropped = 0;
    if (frame == 0 && n == 0)
        for (int c = 0; c < ncells; c++) {
            int x, y;
            track_seed_xy(c, ncx, s, h, w, &x, &y);
            if (!track_textured(x, y, h, w, p.min_eig, g1)) continue;
            if ((int)cur.size() < cap) { cur.push_back(TrackRec{next++, 0, (float)x, (float)y}); seeded++; }
            else dropped++;
        }
    std::vector<uint8_t> cov(ncells, 0);
    int live = 0, ended = 0;
    for (const TrackRec& t : cur) {
        float nx = t.x, ny = t.y;
        const int st = track_advance(t.x, t.y, h, w, p, F, G, &nx, &ny);
        if (st == kTrackAlive) {
            out_ids[live] = t.id; out_starts[live] = t.start; out_xy[2 * live] = nx; out_xy[2 * live + 1] = ny;
            live++;
            cov[track_cell(nx, ny, ncx, s)] = 1;
        } else {
            end_ids[ended] = t.id; end_starts[ended] = t.start; end_xy[2 * ended] = t.x; end_xy[2 * ended + 1] = t.y; end_reasons[ended] = st;
            ended++;
        }
    }
    for (int c = 0; c < ncells; c++) {
        if (cov[c]) continue;
        int x, y;
        track_seed_xy(c, ncx, s, h, w, &x, &y);
        if (!track_textured(x, y, h, w, p.min_eig, g2)) continue;
        if (live < cap) {
            out_ids[live] = next++; out_starts[live] = frame + 1; out_xy[2 * live] = (float)x; out_xy[2 * live + 1] = (float)y;
            live++;
            seeded++;
        } else dropped++;
    }
    counts->live = live;
    counts->ended = ended;
    counts->seeded = seeded;
    counts->dropped = dropped;
    counts->frame = frame + 1;
    counts->next_id = next;
    return EPPM_OK;
}

extern "C" int eppm_track_seeds_host(const eppm_track_params* pin, const uint8_t* rgb, int h, int w, int max, float* xy, int* n)
{
    TrackParams p;
    int cap, ncx, ncy;
    CHK(track_params(pin, h, w, &p, &cap, &ncx, &ncy));
    if (!rgb || !n || max < 0 || (max > 0 && !xy)) return set_err(EPPM_ERR_ARG, "eppm_track_seeds_host: bad argument");
    auto g = [rgb, w](int x, int y) { const uint8_t* q = rgb + ((size_t)y * w + x) * 3; return (int)q[0] + (int)q[1] + (int)q[2]; };
    int k = 0;
    for (int c = 0; c < ncx * ncy; c++) {
        int x, y;
        track_seed_xy(c, ncx, p.spacing, h, w, &x, &y);
        if (!track_textured(x, y, h, w, p.min_eig, g)) continue;
        if (k < max) { xy[2 * k] = (float)x; xy[2 * k + 1] = (float)y; }
        k++;
    }
    *n = k;
    return EPPM_OK;
}
