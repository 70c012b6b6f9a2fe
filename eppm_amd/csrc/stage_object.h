// stage_object.h -- the core the ten per-clip stage objects share: the tracker, the temporal filter, the
// stabiliser, the cut detector, the correspondence map, the object detector, the background plate, the defect filter, the deflicker object
// and the deinterlacer.  Each is one allocation on a device
// with one slot per pair of a batch, stepped from a context on the context's stream or on caller planes on the launcher stream, with
// synchronous getters and setters on the null stream.  Host code only: no kernel and no header a kernel includes knows this file.
#pragma once

#include <functional>

#include "api_internal.h"

struct EPPM_HIDDEN StageObject {
    const char* noun = "object";        // what the object calls itself in messages: "filter", "stabiliser", "detector", "map", "plate", "tracker", "defect filter", "deflicker object", "deinterlacer"
    int device = 0, h = 0, w = 0, nslots = 0;
    char* mem = nullptr;                // the one allocation
    size_t bytes = 0;
    hipEvent_t done = nullptr;          // recorded after every launch and copy: the synchronous calls wait for it
    hipStream_t last = nullptr;         // the stream of the last step: a step on another stream waits for `done` first
    size_t px() const { return (size_t)h * w; }
};

// device, h, w, nslots and bytes are set: the slots range (EPPM_ERR_ARG, before any HIP call), the block from the cache, `init` (work
// on the null stream that the block needs before its first step, or none), the event, recorded on the null stream.  A failure waits for
// the device, returns the block and leaves *o closed
EPPM_HIDDEN int stage_open(StageObject* o, const char* what, const std::function<hipError_t()>& init = nullptr);
// waits for `done`, then the event and the block go; harmless on an object that never opened
EPPM_HIDDEN void stage_close(StageObject* o);
// the object's last launch or copy is complete (the synchronous calls read and write its planes on the null stream); sets the device
EPPM_HIDDEN int stage_wait(StageObject* o);
// a synchronous call's work on the null stream is complete; the next step on any stream starts behind it
EPPM_HIDDEN int stage_settle(StageObject* o);
// 0 <= slot < nslots; the object's own condition ("is empty", "has not been stepped") stays with the object
EPPM_HIDDEN int stage_slot_check(const StageObject* o, int slot, const char* what);
// a step's launches on stream s go between these: enter waits for `done` if s is not the stream of the last step; leave consumes the
// launches' error, records `done` on s and makes s the stream of the last step.  The asynchronous getters run between
// stage_enter(o, o->last) and stage_leave(o, o->last): on the stream of the last step, behind it; the next step on any stream waits
EPPM_HIDDEN int stage_enter(StageObject* o, hipStream_t s);
EPPM_HIDDEN int stage_leave(StageObject* o, hipStream_t s);
// one plane of h x w RGBA words of the object: to the caller's packed RGB rows after stage_wait, or to a caller's device plane on the
// stream of the last step
EPPM_HIDDEN int stage_get_rgb(StageObject* o, const uint32_t* d_words, int h, int w, uint8_t* rgb, size_t row_stride);
EPPM_HIDDEN int stage_get_rgba_device(StageObject* o, const uint32_t* d_words, int h, int w, void* d_rgba, size_t pitch);

// "run this on the launcher stream, for the object o" (launchers_ref_abi.cpp, which owns that stream): under the launchers' lock, the
// current device must be the object's; fn(stream); the stream is synchronised unless sync is false; the launches' error
EPPM_HIDDEN int launcher_run(const StageObject* o, const char* what, const std::function<int(hipStream_t)>& fn, bool sync = true);

// every plane of a context's last bidirectional call that an object may read, for every active pair (ctx_interp.cpp)
struct EPPM_HIDDEN CtxPlanes {
    const uint8_t *img1 = nullptr, *img2 = nullptr;     // the raw RGBA frames, img_stride bytes from pair to pair
    size_t img_pitch = 0, img_stride = 0;
    const float *fwd = nullptr, *bwd = nullptr;         // the level-0 flows
    size_t fwd_stride = 0, bwd_stride = 0;
    const uint8_t *occ1 = nullptr, *occ2 = nullptr;
    size_t occ_stride = 0;
    int n = 0;                                          // active pairs
};
// the window of eppm_interpolate*, once for all ten objects.  EPPM_ERR_ARG: other dimensions / device, more active pairs than slots
// (pair NULL) or a pair that is not active (pair given: the tracker's one pair, whose planes *in then holds); EPPM_ERR_STATE: outside the
// window.  Sets the context's device current; *s: the context's stream
EPPM_HIDDEN int ctx_stage_inputs(eppm_ctx* c, const StageObject* o, const char* what, CtxPlanes* in, hipStream_t* s, const int* pair = nullptr);
// what a stabiliser reads of these planes (stabilizer.cpp): the object detector and the background plate step a private one
EPPM_HIDDEN eppm::StabArgs stab_ctx_args(const CtxPlanes& c);

// a named stage-timing entry of the context around a scope; nothing when the context is NULL
struct EPPM_HIDDEN StageTimer {
    eppm_ctx* c;
    StageTimer(eppm_ctx* ctx, const char* name) : c(ctx) { if (c) ctx_stage_begin(c, name); }
    ~StageTimer() { if (c) ctx_stage_end(c); }
    StageTimer(const StageTimer&) = delete;
};

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline bool bad_pitch(size_t pitch, int w) { return pitch < (size_t)w * 4 || (pitch & 3); }
// rows of RGBA words to rows of packed RGB
EPPM_HIDDEN void words_to_rgb(const uint32_t* words, int h, int w, uint8_t* rgb, size_t row_stride);
// an *Args bit mask over slots: bit k = flags[k - slot0] != 0 for slot0 <= k < slot0 + n, every other bit 0; flags NULL: all 0
template <size_t N> static inline void slot_mask(uint32_t (&mask)[N], const uint8_t* flags, int slot0, int n)
{
    memset(mask, 0, sizeof(mask));
    for (int k = slot0; flags && k < slot0 + n; k++)
        if (flags[k - slot0]) mask[k >> 5] |= 1u << (k & 31);
}
