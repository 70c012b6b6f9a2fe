// stage_object.cpp -- the core of the per-clip stage objects (stage_object.h): the one open and close of their
// allocation and event, the hand-over of an object between streams, and the small host helpers the nine modules share.
#include "stage_object.h"

using namespace eppm;

// the one way out: a failed open waits for the device (work on the null stream may still touch the block), a close for the last step
static void release(StageObject* o, bool failed)
{
    if (!o->done && !o->mem) return;    // never opened: no HIP call
    (void)hipSetDevice(o->device);
    if (o->done && !failed) (void)hipEventSynchronize(o->done);
    if (o->done) (void)hipEventDestroy(o->done);
    if (failed) (void)hipDeviceSynchronize();
    if (o->mem) cache_free(o->mem, o->bytes, false, o->device);
    o->done = nullptr;
    o->mem = nullptr;
}

int stage_open(StageObject* o, const char* what, const std::function<hipError_t()>& init)
{
    if (o->nslots < 1 || o->nslots > kTemporalMaxSlots) return set_err(EPPM_ERR_ARG, "%s: %d slots outside [1, %d]", what, o->nslots, kTemporalMaxSlots);
    HIPCHK(hipSetDevice(o->device));
    hipError_t e = cache_alloc((void**)&o->mem, o->bytes, false, o->device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        o->mem = nullptr;
        return set_err(EPPM_ERR_HIP, "%s: hipMalloc of %zu bytes (%s) failed: %s", what, o->bytes, o->noun, hipGetErrorString(e));
    }
    if (init) e = init();
    if (e == hipSuccess) e = hipEventCreateWithFlags(&o->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(o->done, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release(o, true);
        return set_err(EPPM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    o->last = nullptr;
    return EPPM_OK;
}

void stage_close(StageObject* o) { release(o, false); }

int stage_wait(StageObject* o)
{
    HIPCHK(hipSetDevice(o->device));
    HIPCHK(hipEventSynchronize(o->done));
    return EPPM_OK;
}

int stage_settle(StageObject* o)
{
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipEventRecord(o->done, nullptr));
    o->last = nullptr;
    return EPPM_OK;
}

int stage_slot_check(const StageObject* o, int slot, const char* what)
{
    if (slot < 0 || slot >= o->nslots) return set_err(EPPM_ERR_ARG, "%s: slot %d, the %s has %d", what, slot, o->noun, o->nslots);
    return EPPM_OK;
}

int stage_enter(StageObject* o, hipStream_t s)
{
    if (s != o->last) HIPCHK(hipStreamWaitEvent(s, o->done, 0));
    return EPPM_OK;
}

int stage_leave(StageObject* o, hipStream_t s)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(o->done, s));
    o->last = s;
    return EPPM_OK;
}

void words_to_rgb(const uint32_t* words, int h, int w, uint8_t* rgb, size_t row_stride)
{
    for (int y = 0; y < h; y++) {
        uint8_t* o = rgb + (size_t)y * row_stride;
        const uint32_t* q = words + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            o[3 * x] = (uint8_t)q[x]; o[3 * x + 1] = (uint8_t)(q[x] >> 8); o[3 * x + 2] = (uint8_t)(q[x] >> 16);
        }
    }
}

int stage_get_rgb(StageObject* o, const uint32_t* d_words, int h, int w, uint8_t* rgb, size_t row_stride)
{
    CHK(stage_wait(o));
    std::vector<uint32_t> words((size_t)h * w);
    HIPCHK(hipMemcpy(words.data(), d_words, words.size() * 4, hipMemcpyDeviceToHost));
    words_to_rgb(words.data(), h, w, rgb, row_stride);
    return EPPM_OK;
}

int stage_get_rgba_device(StageObject* o, const uint32_t* d_words, int h, int w, void* d_rgba, size_t pitch)
{
    HIPCHK(hipSetDevice(o->device));
    CHK(stage_enter(o, o->last));
    HIPCHK(hipMemcpy2DAsync(d_rgba, pitch, d_words, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyDeviceToDevice, o->last));
    return stage_leave(o, o->last);
}
