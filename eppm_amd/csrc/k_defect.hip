// k_defect.hip -- film-defect removal (defect.h): one detect and one apply launch per step for every slot it covers
// (blockIdx.z), one lane per pixel of image 1.  A wave is 64 consecutive pixels of one row, as in k_tfilter_step, so the frame word, the
// two vectors, the saved set the lane writes, the code byte, the replacement and the output word are coalesced.
//
// The window median of the four vector components (the second chance) is wanted by under 1 % of the pixels of natural content, but by
// some pixel of almost every block of 256, so a lane that selects its own medians makes its whole wave wait for it.  The detect kernel
// therefore does nothing for the median unless a lane of its block is undecided after the first chance; then the block stages the keys of
// its 64 x 4 pixels and their halo (16 bytes per pixel, at most 72 x 12 of them: 13.5 KiB) in LDS once and takes one of two forms by
// the number of its undecided lanes.  Up to kDfWaveFormMax of them: the lanes append themselves to a list in LDS and a WAVE selects the
// medians of one listed pixel at a time, two window elements per lane, counting with ballots (32 passes of eight ballots: about a
// twentieth of what a lane alone needs).  More: every undecided lane selects its own (defect_median: 32 passes of one 16-byte LDS read
// per window pixel, eight registers of state whatever the radius -- a sorting network over 81 x 4 values would not fit the register
// file), which is the cheaper form once most lanes of a wave want one.  Both forms select the element of rank (n - 1) / 2 of the same
// integer keys, as the host form does, so all three agree at every share of undecided pixels.  The arithmetic has no EPPM_TOL branch.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "defect.h"

namespace eppm {

namespace {

constexpr int kDfBlockW = 64, kDfBlockH = 4, kDfMaxRadius = 4;
constexpr int kDfTileMax = (kDfBlockW + 2 * kDfMaxRadius) * (kDfBlockH + 2 * kDfMaxRadius);
constexpr int kDfWaveFormMax = 64;      // undecided lanes of a block up to which a wave selects each pixel's medians

__device__ __forceinline__ bool df_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct DfWords {            // an unpitched plane of h*w RGBA words
    const uint32_t* __restrict__ p;
    int w;
    __device__ uint32_t operator()(int x, int y) const { return p[(size_t)y * w + x]; }
};
struct DfPitched {          // a frame of `pitch` bytes per row
    const uint8_t* __restrict__ p;
    size_t pitch;
    __device__ uint32_t operator()(int x, int y) const { return *reinterpret_cast<const uint32_t*>(p + (size_t)y * pitch + (size_t)x * 4); }
};
struct DfTile {             // the block's staged keys, seen from one lane
    const uint4* t;
    int tw, at;             // the tile's width and the lane's own element
    __device__ DfKeys operator()(int dx, int dy) const
    {
        const uint4 v = t[at + dy * tw + dx];
        return DfKeys{v.x, v.y, v.z, v.w};
    }
};
// defect_median for the window centred on tile element `at`, by the 64 lanes of a wave together: lane j holds the window's elements j and
// j + 64.  Every lane returns the same answer
__device__ __forceinline__ bool df_wave_median(const uint4* t, int tw, int at, int r, float* out)
{
    const int side = 2 * r + 1, n = side * side, lane = threadIdx.x;
    const bool v0 = lane < n, v1 = lane + 64 < n;
    const int e0 = v0 ? lane : 0, e1 = v1 ? lane + 64 : 0;
    const uint4 k0 = t[at + (e0 / side - r) * tw + (e0 % side - r)], k1 = t[at + (e1 / side - r) * tw + (e1 % side - r)];
    if (__ballot((v0 && k0.x == kDfUnknown) || (v1 && k1.x == kDfUnknown))) return false;
    const uint32_t rank = (uint32_t)(n - 1) / 2;
    uint32_t pa = 0, pb = 0, pc = 0, pd = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t ta = pa | 1u << bit, tb = pb | 1u << bit, tc = pc | 1u << bit, td = pd | 1u << bit;
        const uint32_t na = __popcll(__ballot(v0 && k0.x < ta)) + __popcll(__ballot(v1 && k1.x < ta));
        const uint32_t nb = __popcll(__ballot(v0 && k0.y < tb)) + __popcll(__ballot(v1 && k1.y < tb));
        const uint32_t nc = __popcll(__ballot(v0 && k0.z < tc)) + __popcll(__ballot(v1 && k1.z < tc));
        const uint32_t nd = __popcll(__ballot(v0 && k0.w < td)) + __popcll(__ballot(v1 && k1.w < td));
        if (na <= rank) pa = ta;
        if (nb <= rank) pb = tb;
        if (nc <= rank) pc = tc;
        if (nd <= rank) pd = td;
    }
    out[0] = defect_unkey(pa); out[1] = defect_unkey(pb); out[2] = defect_unkey(pc); out[3] = defect_unkey(pd);
    return true;
}

struct DfCodes {
    const uint8_t* __restrict__ p;
    int w;
    __device__ uint8_t operator()(int x, int y) const { return p[(size_t)y * w + x]; }
};

}  // namespace

__global__ __launch_bounds__(256) void k_defect_detect(DefectArgs A)
{
    __shared__ uint4 tile[kDfTileMax];
    __shared__ float4 s_med[kDfWaveFormMax];
    __shared__ uint16_t s_at[kDfWaveFormMax];
    __shared__ uint8_t s_ok[kDfWaveFormMax];
    __shared__ int s_n;
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int bx0 = blockIdx.x * kDfBlockW, by0 = blockIdx.y * kDfBlockH;
    const int x = bx0 + threadIdx.x, y = by0 + threadIdx.y;
    const bool inside = x < A.w && y < A.h;
    const size_t px = (size_t)A.h * A.w, i = (size_t)y * A.w + x;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const int cur = df_bit(A.cur, slot) ? 1 : 0;
    const bool active = df_bit(A.active, slot);
    const float2* __restrict__ prev_bwd = reinterpret_cast<const float2*>(blk + defect_off_bwd(px, cur));
    const uint32_t* __restrict__ prev_img = reinterpret_cast<const uint32_t*>(blk + defect_off_img(px, cur));
    const float2* __restrict__ fwd = reinterpret_cast<const float2*>(pair_ptr(A.fwd, A.fwd_stride, pair));
    const uint8_t* img1 = pair_ptr(A.img1, A.img_stride, pair);

    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4 && threadIdx.y == 0) A.stats[(size_t)slot * 4 + threadIdx.x] = 0;

    uint32_t cur_word = 0, word = 0;
    float2 own_bwd = make_float2(0.0f, 0.0f);
    uint8_t code = 0;
    DfChance c1{false, false, 0};
    const DfWords P{prev_img, A.w};
    const DfPitched N{pair_ptr(A.img2, A.img_stride, pair), A.img_pitch};
    if (inside) {
        cur_word = *reinterpret_cast<const uint32_t*>(img1 + (size_t)y * A.img_pitch + (size_t)x * 4);
        own_bwd = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair))[i];
        word = cur_word | 0xff000000u;
    }
    if (active) {           // uniform over the block
        if (inside) {
            const float2 f = fwd[i], b = prev_bwd[i];
            c1 = defect_chance(x, y, cur_word, b.x, b.y, f.x, f.y, A.h, A.w, A.detect, A.agree, P, N);
            code = defect_code(c1, nullptr, &word);
        }
        const bool need = inside && !c1.decided && A.radius > 0;
        if (threadIdx.x == 0 && threadIdx.y == 0) s_n = 0;
        const int wanted = __syncthreads_count(need);
        if (wanted) {
            const int r = A.radius, tw = kDfBlockW + 2 * r, th = kDfBlockH + 2 * r;
            for (int k = threadIdx.y * kDfBlockW + threadIdx.x; k < tw * th; k += kDfBlockW * kDfBlockH) {
                const int gx = min(max(bx0 - r + k % tw, 0), A.w - 1), gy = min(max(by0 - r + k / tw, 0), A.h - 1);
                const size_t g = (size_t)gy * A.w + gx;
                const float2 f = fwd[g], b = prev_bwd[g];
                const DfKeys q = defect_keys(f.x, f.y, b.x, b.y);
                tile[k] = make_uint4(q.a, q.b, q.c, q.d);
            }
            const int at = ((int)threadIdx.y + r) * tw + (int)threadIdx.x + r;
            float m[4];
            bool have = false;
            if (wanted <= kDfWaveFormMax) {
                int mine = -1;
                if (need) {
                    mine = atomicAdd(&s_n, 1);                  // any order: an entry's result does not depend on its place
                    s_at[mine] = (uint16_t)at;
                }
                __syncthreads();
                for (int k = threadIdx.y; k < wanted; k += kDfBlockH) {
                    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    const bool ok = df_wave_median(tile, tw, s_at[k], r, q);
                    if (threadIdx.x == 0) {
                        s_med[k] = make_float4(q[0], q[1], q[2], q[3]);
                        s_ok[k] = ok;
                    }
                }
                __syncthreads();
                if (need) {
                    const float4 v = s_med[mine];
                    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
                    have = s_ok[mine] != 0;
                }
            } else {
                __syncthreads();
                if (need) have = defect_median(r, DfTile{tile, tw, at}, m);
            }
            if (need && have) {
                const DfChance c2 = defect_chance(x, y, cur_word, m[2], m[3], m[0], m[1], A.h, A.w, A.detect, A.agree, P, N);
                code = defect_code(c1, &c2, &word);
            }
        }
    }
    if (!inside) return;
    reinterpret_cast<float2*>(blk + defect_off_bwd(px, cur ^ 1))[i] = own_bwd;
    reinterpret_cast<uint32_t*>(blk + defect_off_img(px, cur ^ 1))[i] = cur_word | 0xff000000u;
    reinterpret_cast<uint32_t*>(blk + defect_off_repl(px))[i] = word;
    reinterpret_cast<uint8_t*>(blk + defect_off_code(px))[i] = code;
}

// a block covers 64 x 16 pixels in four passes of its four waves, so that the slot's four counters see four adds per 1024 pixels: adds
// to one address serialise, and one per wave made them the launch's whole time
constexpr int kDfApplyRows = 16;

__global__ __launch_bounds__(256) void k_defect_apply(DefectArgs A)
{
    __shared__ int s_cnt[4];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * kDfBlockW + threadIdx.x;
    const size_t px = (size_t)A.h * A.w;
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    const DfCodes C{reinterpret_cast<const uint8_t*>(blk + defect_off_code(px)), A.w};
    const int cur = df_bit(A.cur, slot) ? 1 : 0;            // the set the detect launch wrote holds image 1 with alpha 255
    if (threadIdx.y == 0 && threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int n_hit = 0, n_grown = 0, n_second = 0, n_und = 0;    // of the wave (rows of 64 pixels): integer counts, order-free
    for (int pass = 0; pass < kDfApplyRows / kDfBlockH; pass++) {
        const int y = blockIdx.y * kDfApplyRows + pass * kDfBlockH + threadIdx.y;
        const bool inside = x < A.w && y < A.h;
        const size_t i = (size_t)y * A.w + x;
        uint8_t code = 0, mask = 0;
        if (inside) {
            code = C(x, y);
            mask = defect_mask(x, y, A.h, A.w, A.grow, C);
            const uint32_t word = mask ? reinterpret_cast<const uint32_t*>(blk + defect_off_repl(px))[i]
                                       : reinterpret_cast<const uint32_t*>(blk + defect_off_img(px, cur ^ 1))[i];
            reinterpret_cast<uint32_t*>(blk + defect_off_out(px))[i] = word;
            reinterpret_cast<uint8_t*>(blk + defect_off_mask(px))[i] = mask;
        }
        n_hit += __popcll(__ballot(mask == 1)); n_grown += __popcll(__ballot(mask == 2));
        n_second += __popcll(__ballot((code & kDfSecond) != 0)); n_und += __popcll(__ballot((code & kDfUndecided) != 0));
    }
    if (threadIdx.x == 0) {
        if (n_hit) atomicAdd(&s_cnt[0], n_hit);
        if (n_grown) atomicAdd(&s_cnt[1], n_grown);
        if (n_second) atomicAdd(&s_cnt[2], n_second);
        if (n_und) atomicAdd(&s_cnt[3], n_und);
    }
    __syncthreads();
    if (threadIdx.y == 0 && threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(A.stats + (size_t)slot * 4 + threadIdx.x, s_cnt[threadIdx.x]);
}

void launch_defect_detect(const DefectArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_defect_detect, dim3((a.w + kDfBlockW - 1) / kDfBlockW, (a.h + kDfBlockH - 1) / kDfBlockH, a.n), dim3(kDfBlockW, kDfBlockH), 0, s, a);
}

void launch_defect_apply(const DefectArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_defect_apply, dim3((a.w + kDfBlockW - 1) / kDfBlockW, (a.h + kDfApplyRows - 1) / kDfApplyRows, a.n), dim3(kDfBlockW, kDfBlockH), 0, s, a);
}

}  // namespace eppm
