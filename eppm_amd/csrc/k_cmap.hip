// k_cmap.hip -- the dense correspondence map to an anchor frame (cmap.h): k_cmap_step moves every covered slot's
// map from image 1 to image 2 of its pair, k_cmap_render composites a slot's layer through its map.  Both have k_tfilter_step's shape: one
// launch for every slot it covers (blockIdx.z), one lane per pixel.  A wave is 64 consecutive pixels of one row, so the frame word (4 B),
// the backward vector (8 B), the mask byte, the new map value (8 B: 512 B per wave and store) and the words written are coalesced, and
// the four float2 taps of the map and the four words of the anchor that neighbouring lanes gather are neighbours wherever the flow and
// the map are smooth.  The step gathers, so it reads one of the slot's two maps and writes the other; which is which, and whether the
// slot is empty or cut, are bits of the kernel arguments.  An empty slot's step reads image 1 in place of the anchor plane and only
// writes that plane, so no lane reads what another writes.  The arithmetic has no EPPM_TOL branch: both libraries compile the same
// operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "cmap.h"

namespace eppm {

namespace {

__device__ __forceinline__ bool cm_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct CmPrevMap {        // the previous map of a slot: its current plane, or the seed while the slot is empty
    const float2* __restrict__ map;
    int w;
    bool empty;
    __device__ CmPt operator()(int x, int y) const
    {
        if (empty) return CmPt{(float)x, (float)y};
        const float2 v = map[(size_t)y * w + x];
        return CmPt{v.x, v.y};
    }
};

struct CmWords {          // RGBA words: a plane of the slot (pitch = 4 * w), or a caller image
    const uint8_t* __restrict__ base;
    size_t pitch;
    uint32_t force;       // ORed into every word (the default layer's alpha)
    __device__ uint32_t operator()(int x, int y) const
    {
        return *reinterpret_cast<const uint32_t*>(base + (size_t)y * pitch + (size_t)x * 4) | force;
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_cmap_step(CMapArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t i = (size_t)y * A.w + x, px = (size_t)A.h * A.w;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const bool cur = cm_bit(A.cur, slot), empty = cm_bit(A.empty, slot), cut = cm_bit(A.cut, slot);
    const float2* __restrict__ prev = reinterpret_cast<const float2*>(blk) + (cur ? px : 0);
    float2* __restrict__ next = reinterpret_cast<float2*>(blk) + (cur ? 0 : px);
    uint32_t* anchor = reinterpret_cast<uint32_t*>(blk + A.off_anchor);
    uint32_t* frame = anchor + px;
    const uint8_t* img1 = pair_ptr(A.img1, A.img_stride, pair);
    const uint32_t word = *reinterpret_cast<const uint32_t*>(pair_ptr(A.img2, A.img_stride, pair) + (size_t)y * A.img_pitch + (size_t)x * 4);
    const float2 f = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair))[i];
    const uint8_t o = pair_ptr(A.occ2, A.occ_stride, pair)[i];
    const CmPrevMap M{prev, A.w, empty};
    const CmWords Anc{empty ? img1 : reinterpret_cast<const uint8_t*>(anchor), empty ? A.img_pitch : (size_t)A.w * 4, 0u};
    const CmPt s = cmap_step_pixel(x, y, word, f.x, f.y, o, cut, A.h, A.w, A.thresh, A.tear, A.use_occ, M, Anc);
    next[i] = make_float2(s.x, s.y);
    frame[i] = word;
    // a cut re-anchors on image 2 (nothing of the anchor was read); an empty slot that is not cut takes image 1 (read from the image)
    if (cut) anchor[i] = word;
    else if (empty) anchor[i] = *reinterpret_cast<const uint32_t*>(img1 + (size_t)y * A.img_pitch + (size_t)x * 4);
}

__global__ __launch_bounds__(256) void k_cmap_render(CMapArgs A)
{
    const unsigned slot = A.slot0 + blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t i = (size_t)y * A.w + x, px = (size_t)A.h * A.w;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const float2 v = (reinterpret_cast<const float2*>(blk) + (cm_bit(A.cur, slot) ? px : 0))[i];
    uint32_t* anchor = reinterpret_cast<uint32_t*>(blk + A.off_anchor);      // then frame, layer, out: px words each
    const bool def = cm_bit(A.deflayer, slot);
    const CmWords L{reinterpret_cast<const uint8_t*>(def ? anchor : anchor + 2 * px), (size_t)A.w * 4, def ? 255u << 24 : 0u};
    anchor[3 * px + i] = cmap_render_pixel(anchor[px + i], CmPt{v.x, v.y}, A.h, A.w, L);
}

void launch_cmap_step(const CMapArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_cmap_step, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

void launch_cmap_render(const CMapArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_cmap_render, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

}  // namespace eppm
