// k_plate.hip -- background plates (plate.h): every launch covers the slots of a step (blockIdx.z, or one lane per
// slot in k_plate_path).  Every kernel gathers: a lane reads what earlier launches wrote and writes only its own pixel, so there are no
// atomics, fences or tickets, and the results are the same bits on every run and equal the host forms.
//   k_plate_path        one lane per slot.  Phase 0, before the accumulation: the forms of the slot's path P.  Phase 1, after it: P advanced
//                       by the pair's model, or the identity after a cut.  Two launches, so no block reads what another block of its launch writes.
//   k_plate_block       the blocked plane: the mask's bytes classified and dilated by `grow`, separable (rows, then columns) through an LDS
//                       tile of 64 x 16 pixels with a halo of `grow`; byte loads and stores of consecutive lanes are consecutive.
//   k_plate_accumulate  one lane per canvas pixel, a wave is 64 consecutive pixels of a canvas row: one 16-byte load and one 16-byte store of
//                       the state per lane (1 KiB per wave), in place; the four image taps and four blocked bytes of neighbouring lanes are
//                       neighbours under any near-identity path.  A lane whose pixel is unchanged stores nothing, except in an empty slot,
//                       whose states it must not read and therefore has to define: there it stores n = 0.
//   k_plate_render      one lane per frame pixel: the RGBA word and the fill byte.
//   k_plate_word        the canvas states as RGBA words and coverage bytes.
// The arithmetic has no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "plate.h"

namespace eppm {

namespace {

constexpr int kPlTileW = 64, kPlTileH = 16;

__device__ __forceinline__ bool pl_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct PlPx {             // an RGBA image, pitch bytes per row
    const uint8_t* __restrict__ img;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(img + (size_t)y * pitch + (size_t)x * 4); }
};

struct PlBk {             // a blocked plane
    const uint8_t* __restrict__ b;
    int w;
    __device__ uint8_t operator()(int x, int y) const { return b[(size_t)y * w + x]; }
};

struct PlSt {             // a canvas
    const float4* __restrict__ st;
    int cw;
    __device__ TfState operator()(int x, int y) const
    {
        const float4 v = st[(size_t)y * cw + x];
        return TfState{v.x, v.y, v.z, v.w};
    }
};

}  // namespace

__global__ __launch_bounds__(64) void k_plate_path(PlateArgs A)
{
    const unsigned pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= (unsigned)A.n) return;
    const unsigned slot = A.slot0 + pair;
    PlateRec* rec = reinterpret_cast<PlateRec*>(pair_ptr(A.mem, A.slot_stride, slot) + A.off_rec);
    double p[6];
#pragma unroll
    for (int k = 0; k < 6; k++) p[k] = rec->p[k];
    if (A.phase == 0) {
        float fwd[6], inv[6];
        const bool ok = plate_forms(p, fwd, inv);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            rec->fwd[k] = fwd[k];
            rec->inv[k] = inv[k];
        }
        rec->ok = ok ? 1 : 0;
        return;
    }
    if (pl_bit(A.cut, slot)) plate_identity(p);
    else if (A.model) {
        const GmModel* m = reinterpret_cast<const GmModel*>(pair_ptr(A.model, A.model_stride, pair));
        double mp[6];
#pragma unroll
        for (int k = 0; k < 6; k++) mp[k] = m->p[k];
        plate_advance(p, mp, m->valid != 0);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) rec->p[k] = p[k];
}

__global__ __launch_bounds__(256) void k_plate_block(PlateArgs A)
{
    __shared__ uint8_t raw[kPlTileH + 2 * kPlateMaxGrow][kPlTileW + 2 * kPlateMaxGrow];
    __shared__ uint8_t rows[kPlTileH + 2 * kPlateMaxGrow][kPlTileW];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const uint8_t* __restrict__ mask = pair_ptr(A.mask, A.mask_stride, pair);
    uint8_t* __restrict__ out = reinterpret_cast<uint8_t*>(pair_ptr(A.mem, A.slot_stride, slot) + A.off_b);
    const int g = A.grow, tw = kPlTileW + 2 * g, th = kPlTileH + 2 * g;
    const int x0 = blockIdx.x * kPlTileW, y0 = blockIdx.y * kPlTileH;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const bool acc = A.accept_invalid != 0;
    for (int i = tid; i < tw * th; i += 256) {
        const int ry = i / tw, rx = i - ry * tw;
        const int gx = x0 - g + rx, gy = y0 - g + ry;
        raw[ry][rx] = (gx >= 0 && gx < A.w && gy >= 0 && gy < A.h) ? plate_blocked(mask[(size_t)gy * A.w + gx], acc) : 0;
    }
    __syncthreads();
    for (int i = tid; i < th * kPlTileW; i += 256) {
        const int ry = i >> 6, x = i & 63;
        uint8_t b = 0;
        for (int k = 0; k <= 2 * g; k++) b |= raw[ry][x + k];
        rows[ry][x] = b;
    }
    __syncthreads();
    for (int i = tid; i < kPlTileH * kPlTileW; i += 256) {
        const int y = i >> 6, x = i & 63;
        uint8_t b = 0;
        for (int k = 0; k <= 2 * g; k++) b |= rows[y + k][x];
        if (x0 + x < A.w && y0 + y < A.h) out[(size_t)(y0 + y) * A.w + (x0 + x)] = b;
    }
}

__global__ __launch_bounds__(256) void k_plate_accumulate(PlateArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int xc = blockIdx.x * blockDim.x + threadIdx.x, yc = blockIdx.y * blockDim.y + threadIdx.y;
    if (xc >= A.cw || yc >= A.ch) return;
    char* __restrict__ blk = pair_ptr(A.mem, A.slot_stride, slot);
    const PlateRec* rec = reinterpret_cast<const PlateRec*>(blk + A.off_rec);
    float4* st = reinterpret_cast<float4*>(blk) + ((size_t)yc * A.cw + xc);
    const bool empty = pl_bit(A.empty, slot);
    float fwd[6];
#pragma unroll
    for (int k = 0; k < 6; k++) fwd[k] = rec->fwd[k];
    const PlPx P{pair_ptr(A.img1, A.img_stride, pair), A.img_pitch};
    const PlBk B{reinterpret_cast<const uint8_t*>(blk + A.off_b), A.w};
    float c[3];
    if (!(rec->ok != 0 && plate_sample(xc, yc, A.mx, A.my, fwd, A.h, A.w, P, B, c))) {
        if (empty) *st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    TfState s{0.0f, 0.0f, 0.0f, 0.0f};
    if (!empty) {
        const float4 v = *st;
        s = TfState{v.x, v.y, v.z, v.w};
    }
    s = plate_update(s, c, A.thresh, A.n_max);
    *st = make_float4(s.r, s.g, s.b, s.n);
}

__global__ __launch_bounds__(256) void k_plate_render(PlateRenderArgs A)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const size_t i = (size_t)y * A.w + x;
    const PlPx P{A.img1, A.img_pitch};
    const PlSt S{reinterpret_cast<const float4*>(A.canvas), A.cw};
    float inv[6];
#pragma unroll
    for (int k = 0; k < 6; k++) inv[k] = A.inv[k];
    uint8_t f;
    const uint32_t o = plate_render_pixel(x, y, P(x, y), A.blocked[i], A.ok != 0, inv,A.mx, A.my, A.h, A.w, A.ch, A.cw, A.min_count, S, &f);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(A.out) + (size_t)y * A.out_pitch + (size_t)x * 4) = o;
    A.fill[i] = f;
}

__global__ __launch_bounds__(256) void k_plate_word(const float4* __restrict__ canvas, uint32_t* __restrict__ words, uint8_t* __restrict__ cov, int ch, int cw)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= cw || y >= ch) return;
    const size_t i = (size_t)y * cw + x;
    const float4 v = canvas[i];
    words[i] = tfilter_word(TfState{v.x, v.y, v.z, v.w});
    cov[i] = plate_coverage(v.w);
}

void launch_plate_path(const PlateArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_plate_path, dim3((a.n + 63) / 64), dim3(64), 0, s, a); }

void launch_plate_block(const PlateArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_plate_block, dim3((a.w + kPlTileW - 1) / kPlTileW, (a.h + kPlTileH - 1) / kPlTileH, a.n), dim3(64, 4), 0, s, a);
}

void launch_plate_accumulate(const PlateArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_plate_accumulate, dim3((a.cw + 63) / 64, (a.ch + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

void launch_plate_render(const PlateRenderArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_plate_render, dim3((a.w + 63) / 64, (a.h + 3) / 4, 1), dim3(64, 4), 0, s, a);
}

void launch_plate_word(const char* canvas, uint32_t* words, uint8_t* cov, int ch, int cw, hipStream_t s)
{
    hipLaunchKernelGGL(k_plate_word, dim3((cw + 63) / 64, (ch + 3) / 4, 1), dim3(64, 4), 0, s, reinterpret_cast<const float4*>(canvas), words, cov, ch, cw);
}

}  // namespace eppm
