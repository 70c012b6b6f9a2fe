// k_deint.hip -- motion-compensated deinterlacing (deint.h).
//   step   one lane per pixel in 64 x 4 blocks, for every slot the step covers (blockIdx.z), as k_tfilter_step and k_deflicker_apply.  A
//          lane on a real row of image 2 copies its word; a lane on a missing row reads the words above and below (coalesced rows), the
//          backward vector, the mask byte and the four reference taps, and writes the output word into the slot's other reference plane
//          and the mask byte.  The bytes of image 2's missing rows are never read.
//   bob    one lane per output pixel of caller planes, a launch per call.
// No LDS, no atomics.  The arithmetic has no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "deint.h"

namespace eppm {

namespace {

__device__ __forceinline__ bool di_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct DiRef {            // the reference of a slot: its current plane, or image 1 while the slot is empty
    const uint32_t* __restrict__ ref;
    const uint8_t* __restrict__ img1;
    size_t pitch;
    int w;
    bool empty;
    __device__ uint32_t operator()(int x, int y) const
    {
        if (empty) return *reinterpret_cast<const uint32_t*>(img1 + (size_t)y * pitch + (size_t)x * 4);
        return ref[(size_t)y * w + x];
    }
};

struct DiField {
    const uint8_t* __restrict__ f;
    size_t pitch;
    __device__ uint32_t operator()(int x, int i) const { return *reinterpret_cast<const uint32_t*>(f + (size_t)i * pitch + (size_t)x * 4); }
};

}  // namespace

__global__ __launch_bounds__(256) void k_deint_step(DeintArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t px = (size_t)A.h * A.w, i = (size_t)y * A.w + x;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const bool cur = di_bit(A.cur, slot);
    uint32_t* __restrict__ next = reinterpret_cast<uint32_t*>(blk + deint_off_ref(px, cur ? 0 : 1));
    uint8_t* __restrict__ mask = reinterpret_cast<uint8_t*>(blk + deint_off_mask(px));
    const uint8_t* __restrict__ img2 = pair_ptr(A.img2, A.img_stride, pair);
    const int parity = di_bit(A.parity, slot) ? 1 : 0;
    if ((y & 1) == parity) {
        next[i] = *reinterpret_cast<const uint32_t*>(img2 + (size_t)y * A.img_pitch + (size_t)x * 4) | 255u << 24;
        mask[i] = 0;
        return;
    }
    const uint32_t up = *reinterpret_cast<const uint32_t*>(img2 + (size_t)deint_row_up(y) * A.img_pitch + (size_t)x * 4);
    const uint32_t dn = *reinterpret_cast<const uint32_t*>(img2 + (size_t)deint_row_dn(y, A.h) * A.img_pitch + (size_t)x * 4);
    const float2 f = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair))[i];
    const uint8_t o = pair_ptr(A.occ2, A.occ_stride, pair)[i];
    const DiRef R{reinterpret_cast<const uint32_t*>(blk + deint_off_ref(px, cur ? 1 : 0)), pair_ptr(A.img1, A.img_stride, pair), A.img_pitch, A.w,
                  di_bit(A.empty, slot)};
    uint8_t m;
    next[i] = deint_missing_pixel(x, y, up, dn, f.x, f.y, o, di_bit(A.cut, slot), A.use_occ, A.thresh, A.h, A.w, R, &m);
    mask[i] = m;
}

__global__ __launch_bounds__(256) void k_deint_bob(uint8_t* __restrict__ out, size_t out_pitch, const uint8_t* __restrict__ field, size_t field_pitch,
                                                   int h, int w, int parity)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const DiField F{field, field_pitch};
    *reinterpret_cast<uint32_t*>(out + (size_t)y * out_pitch + (size_t)x * 4) = deint_bob_pixel(x, y, parity, h, F);
}

void launch_deint_step(const DeintArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_deint_step, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

void launch_deint_bob(uint32_t* out, size_t out_pitch, const uint32_t* field, size_t field_pitch, int h, int w, int parity, hipStream_t s)
{
    hipLaunchKernelGGL(k_deint_bob, dim3((w + 63) / 64, (h + 3) / 4, 1), dim3(64, 4), 0, s, reinterpret_cast<uint8_t*>(out), out_pitch,
                       reinterpret_cast<const uint8_t*>(field), field_pitch, h, w, parity);
}

}  // namespace eppm
