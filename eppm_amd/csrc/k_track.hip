// k_track.hip -- one step of dense point trajectories: seed flags, advance, and a stable compaction of survivors,
// ended tracks and new seeds.  The per-point arithmetic is track.h's, shared with the host form; the order of every list comes from
// per-block ballot counts, one workgroup's exclusive scan of those counts, and a scatter that ranks again inside each block.  No atomics:
// the result is one bit pattern.  The counters (TrackCnt) live on the device, so a step needs no host round trip.
// Blocks of 256 lanes (four waves of 64).  Slot kernels run over the capacity, cell kernels over the cells; both grids are fixed at create.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "track.h"

namespace eppm {

namespace {

constexpr int kTB = 256;            // lanes per block of the slot and cell kernels
constexpr int kScanT = 1024;        // lanes of the scan workgroup

struct RgbaGrey {                   // g = R + G + B of an RGBA word, pitch in bytes
    const uint8_t* __restrict__ p;
    size_t pitch;
    __device__ int operator()(int x, int y) const
    {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (size_t)y * pitch + (size_t)x * 4);
        return (int)(v & 255u) + (int)((v >> 8) & 255u) + (int)((v >> 16) & 255u);
    }
};
struct Float2Field {                // interleaved float2, w vectors per row
    const float2* __restrict__ p;
    int w;
    __device__ void operator()(int x, int y, float* u, float* v) const
    {
        const float2 f = p[(size_t)y * w + x];
        *u = f.x;
        *v = f.y;
    }
};

// this lane's rank among the lanes of its block whose flag is set, and the block's count; sh: 4 ints of LDS (one per wave)
__device__ __forceinline__ int block_rank(bool f, int* sh, int* total)
{
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sh[wv] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < kTB / 64; k++) {
        const int c = sh[k];
        off += k < wv ? c : 0;
        tot += c;
    }
    *total = tot;
    return off + __popcll(m & ((1ull << lane) - 1ull));
}

// exclusive scan of a[0..n) in place by one workgroup of kScanT lanes (each a contiguous chunk); returns the total to every lane
__device__ int wg_exclusive_scan(int* __restrict__ a, int n, int* lds)
{
    const int t = threadIdx.x, per = (n + kScanT - 1) / kScanT;
    const int b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    int s = 0;
    for (int i = b; i < e; i++) s += a[i];
    lds[t] = s;
    __syncthreads();
    for (int d = 1; d < kScanT; d <<= 1) {
        const int v = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += v;
        __syncthreads();
    }
    int run = lds[t] - s;           // exclusive prefix of this chunk
    const int total = lds[kScanT - 1];
    for (int i = b; i < e; i++) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    __syncthreads();                // lds is reused by the caller's next scan
    return total;
}

__device__ __forceinline__ int seed_cell_flag(int c, int ncells, int ncx, int s, int h, int w, long long min_eig, const RgbaGrey& g)
{
    if (c >= ncells) return 0;
    int x, y;
    track_seed_xy(c, ncx, s, h, w, &x, &y);
    return track_textured(x, y, h, w, min_eig, g) ? 1 : 0;
}

}  // namespace

// (seed0 a) frame 0 and no live track: flag the textured cells of image 1; per-block counts into blk_c
__global__ __launch_bounds__(kTB) void k_track_seed0_flags(const uint8_t* __restrict__ img1, size_t pitch, int h, int w, int s, long long min_eig,
                                                           int ncx, int ncells, const int32_t* __restrict__ cnt, uint8_t* __restrict__ flags,
                                                           int32_t* __restrict__ blk_c)
{
    __shared__ int sh[kTB / 64];
    const int c = blockIdx.x * kTB + threadIdx.x;
    const bool on = cnt[kTrackCntFrame] == 0 && cnt[kTrackCntLive] == 0;
    const int f = on ? seed_cell_flag(c, ncells, ncx, s, h, w, min_eig, RgbaGrey{img1, pitch}) : 0;
    if (c < ncells) flags[c] = (uint8_t)f;
    int tot;
    block_rank(f != 0, sh, &tot);
    if (threadIdx.x == 0) blk_c[blockIdx.x] = tot;
}

// (seed0 b) one workgroup: offsets of the frame-0 seeds, how many fit, their first id
__global__ __launch_bounds__(kScanT) void k_track_scan0(int32_t* __restrict__ blk_c, int nbc, int cap, int32_t* __restrict__ cnt)
{
    __shared__ int lds[kScanT];
    const int n = wg_exclusive_scan(blk_c, nbc, lds);
    if (threadIdx.x == 0) {
        const int live = cnt[kTrackCntLive], room = cap - live;
        const int acc = n < room ? n : room;
        cnt[kTrackCntIdBase] = cnt[kTrackCntNextId];
        cnt[kTrackCntNextId] = cnt[kTrackCntNextId] + acc;
        cnt[kTrackCntLive] = live + acc;
        cnt[kTrackCntSeeded0] = acc;
        cnt[kTrackCntDropped0] = n - acc;
    }
}

// (seed0 c) the accepted frame-0 seeds, appended to the current list in cell order
__global__ __launch_bounds__(kTB) void k_track_seed0_scatter(int h, int w, int s, int ncx, int ncells, const uint8_t* __restrict__ flags,
                                                             const int32_t* __restrict__ blk_c, const int32_t* __restrict__ cnt,
                                                             TrackRec* __restrict__ list)
{
    __shared__ int sh[kTB / 64];
    const int c = blockIdx.x * kTB + threadIdx.x;
    const bool f = c < ncells && flags[c] != 0;
    int tot;
    const int r = blk_c[blockIdx.x] + block_rank(f, sh, &tot);
    const int acc = cnt[kTrackCntSeeded0];
    if (!f || r >= acc) return;
    int x, y;
    track_seed_xy(c, ncx, s, h, w, &x, &y);
    TrackRec t;
    t.id = cnt[kTrackCntIdBase] + r;
    t.start = cnt[kTrackCntFrame];
    t.x = (float)x;
    t.y = (float)y;
    list[cnt[kTrackCntLive] - acc + r] = t;
}

// advance: one lane per slot of the capacity; slots at or past the live count take no part.  A survivor marks its cell of frame k+1 in
// the coverage plane (always the value 1: the order of the stores does not matter).  Per-block counts of survivors and ended tracks.
__global__ __launch_bounds__(kTB) void k_track_advance(const float2* __restrict__ fwd, const float2* __restrict__ bwd, int h, int w, int s, int ncx,
                                                       float fb_alpha, float fb_beta, float mb_alpha, float mb_beta, const int32_t* __restrict__ cnt,
                                                       const TrackRec* __restrict__ list, float2* __restrict__ npos, uint8_t* __restrict__ stat,
                                                       uint8_t* __restrict__ cov, int32_t* __restrict__ blk_s, int32_t* __restrict__ blk_e)
{
    __shared__ int sh_s[kTB / 64], sh_e[kTB / 64];
    const int i = blockIdx.x * kTB + threadIdx.x;
    const bool active = i < cnt[kTrackCntLive];
    int st = kTrackAlive;
    if (active) {
        const TrackRec t = list[i];
        const TrackParams p{s, 0, fb_alpha, fb_beta, mb_alpha, mb_beta};
        float nx = t.x, ny = t.y;
        st = track_advance(t.x, t.y, h, w, p, Float2Field{fwd, w}, Float2Field{bwd, w}, &nx, &ny);
        npos[i] = make_float2(nx, ny);
        stat[i] = (uint8_t)st;
        if (st == kTrackAlive) cov[track_cell(nx, ny, ncx, s)] = 1;
    }
    int ts, te;
    block_rank(active && st == kTrackAlive, sh_s, &ts);
    block_rank(active && st != kTrackAlive, sh_e, &te);
    if (threadIdx.x == 0) {
        blk_s[blockIdx.x] = ts;
        blk_e[blockIdx.x] = te;
    }
}

// seed flags: one lane per cell; uncovered cells whose seed passes the texture test on image 2.  Per-block counts into blk_c
__global__ __launch_bounds__(kTB) void k_track_seed_flags(const uint8_t* __restrict__ img2, size_t pitch, int h, int w, int s, long long min_eig,
                                                          int ncx, int ncells, const uint8_t* __restrict__ cov, uint8_t* __restrict__ flags,
                                                          int32_t* __restrict__ blk_c)
{
    __shared__ int sh[kTB / 64];
    const int c = blockIdx.x * kTB + threadIdx.x;
    const int f = (c < ncells && cov[c] == 0) ? seed_cell_flag(c, ncells, ncx, s, h, w, min_eig, RgbaGrey{img2, pitch}) : 0;
    if (c < ncells) flags[c] = (uint8_t)f;
    int tot;
    block_rank(f != 0, sh, &tot);
    if (threadIdx.x == 0) blk_c[blockIdx.x] = tot;
}

// one workgroup: offsets of survivors, ended tracks and seeds; the new counters
__global__ __launch_bounds__(kScanT) void k_track_scan(int32_t* __restrict__ blk_s, int32_t* __restrict__ blk_e, int nbs, int32_t* __restrict__ blk_c,
                                                       int nbc, int cap, int32_t* __restrict__ cnt)
{
    __shared__ int lds[kScanT];
    const int S = wg_exclusive_scan(blk_s, nbs, lds);
    const int E = wg_exclusive_scan(blk_e, nbs, lds);
    const int N = wg_exclusive_scan(blk_c, nbc, lds);
    if (threadIdx.x == 0) {
        const int room = cap - S, acc = N < room ? N : room;
        cnt[kTrackCntPrevLive] = cnt[kTrackCntLive];
        cnt[kTrackCntSurv] = S;
        cnt[kTrackCntLive] = S + acc;
        cnt[kTrackCntEnded] = E;
        cnt[kTrackCntSeeded] = cnt[kTrackCntSeeded0] + acc;
        cnt[kTrackCntDropped] = cnt[kTrackCntDropped0] + (N - acc);
        cnt[kTrackCntSeeded0] = 0;
        cnt[kTrackCntDropped0] = 0;
        cnt[kTrackCntIdBase] = cnt[kTrackCntNextId];
        cnt[kTrackCntNextId] = cnt[kTrackCntNextId] + acc;
        cnt[kTrackCntFrame] = cnt[kTrackCntFrame] + 1;
    }
}

// scatter: blocks [0, nbs) one lane per slot (survivors into the next list, ended tracks into the ended list, both in slot order); blocks
// [nbs, nbs + nbc) one lane per cell (the accepted seeds after the survivors, in cell order; every lane clears its coverage byte for the
// next step)
__global__ __launch_bounds__(kTB) void k_track_scatter(int h, int w, int s, int ncx, int ncells, int nbs, const int32_t* __restrict__ cnt,
                                                       const TrackRec* __restrict__ list, const float2* __restrict__ npos,
                                                       const uint8_t* __restrict__ stat, const int32_t* __restrict__ blk_s,
                                                       const int32_t* __restrict__ blk_e, const uint8_t* __restrict__ flags,
                                                       const int32_t* __restrict__ blk_c, uint8_t* __restrict__ cov, TrackRec* __restrict__ next,
                                                       TrackRec* __restrict__ ended, int32_t* __restrict__ ended_reason)
{
    __shared__ int sh_a[kTB / 64], sh_b[kTB / 64];
    int tot;
    if ((int)blockIdx.x < nbs) {
        const int i = blockIdx.x * kTB + threadIdx.x;
        const bool active = i < cnt[kTrackCntPrevLive];
        const int st = active ? (int)stat[i] : kTrackAlive;
        const bool surv = active && st == kTrackAlive, end = active && st != kTrackAlive;
        const int rs = blk_s[blockIdx.x] + block_rank(surv, sh_a, &tot);
        const int re = blk_e[blockIdx.x] + block_rank(end, sh_b, &tot);
        if (!active) return;
        TrackRec t = list[i];
        if (surv) {
            const float2 q = npos[i];
            t.x = q.x;
            t.y = q.y;
            next[rs] = t;
        } else {
            ended[re] = t;
            ended_reason[re] = st;
        }
        return;
    }
    const int b = blockIdx.x - nbs, c = b * kTB + threadIdx.x;
    const bool f = c < ncells && flags[c] != 0;
    const int r = blk_c[b] + block_rank(f, sh_a, &tot);
    if (c < ncells) cov[c] = 0;
    const int S = cnt[kTrackCntSurv];
    if (!f || S + r >= cnt[kTrackCntLive]) return;
    int x, y;
    track_seed_xy(c, ncx, s, h, w, &x, &y);
    TrackRec t;
    t.id = cnt[kTrackCntIdBase] + r;
    t.start = cnt[kTrackCntFrame];
    t.x = (float)x;
    t.y = (float)y;
    next[S + r] = t;
}

static int nblocks(int n) { return (n + kTB - 1) / kTB; }

void launch_track_seed0(const TrackDev& d, const TrackIn& in, TrackRec* cur, hipStream_t st)
{
    const int nbc = nblocks(d.ncells);
    hipLaunchKernelGGL(k_track_seed0_flags, dim3(nbc), dim3(kTB), 0, st, in.img1, in.pitch, in.h, in.w, d.p.spacing, d.p.min_eig, d.ncx, d.ncells,
                       (const int32_t*)d.cnt, d.flags, d.blk_c);
    hipLaunchKernelGGL(k_track_scan0, dim3(1), dim3(kScanT), 0, st, d.blk_c, nbc, d.cap, d.cnt);
    hipLaunchKernelGGL(k_track_seed0_scatter, dim3(nbc), dim3(kTB), 0, st, in.h, in.w, d.p.spacing, d.ncx, d.ncells, (const uint8_t*)d.flags,
                       (const int32_t*)d.blk_c, (const int32_t*)d.cnt, cur);
}

void launch_track_advance(const TrackDev& d, const TrackIn& in, const TrackRec* cur, hipStream_t st)
{
    hipLaunchKernelGGL(k_track_advance, dim3(nblocks(d.cap)), dim3(kTB), 0, st, (const float2*)in.fwd, (const float2*)in.bwd, in.h, in.w,
                       d.p.spacing, d.ncx, d.p.fb_alpha, d.p.fb_beta, d.p.mb_alpha, d.p.mb_beta, (const int32_t*)d.cnt, cur, (float2*)d.npos,
                       d.stat, d.cov, d.blk_s, d.blk_e);
}

void launch_track_seed(const TrackDev& d, const TrackIn& in, hipStream_t st)
{
    hipLaunchKernelGGL(k_track_seed_flags, dim3(nblocks(d.ncells)), dim3(kTB), 0, st, in.img2, in.pitch, in.h, in.w, d.p.spacing, d.p.min_eig,
                       d.ncx, d.ncells, (const uint8_t*)d.cov, d.flags, d.blk_c);
}

void launch_track_compact(const TrackDev& d, const TrackIn& in, const TrackRec* cur, TrackRec* next, hipStream_t st)
{
    const int nbs = nblocks(d.cap), nbc = nblocks(d.ncells);
    hipLaunchKernelGGL(k_track_scan, dim3(1), dim3(kScanT), 0, st, d.blk_s, d.blk_e, nbs, d.blk_c, nbc, d.cap, d.cnt);
    hipLaunchKernelGGL(k_track_scatter, dim3(nbs + nbc), dim3(kTB), 0, st, in.h, in.w, d.p.spacing, d.ncx, d.ncells, nbs, (const int32_t*)d.cnt, cur,
                       (const float2*)d.npos, (const uint8_t*)d.stat, (const int32_t*)d.blk_s, (const int32_t*)d.blk_e, (const uint8_t*)d.flags,
                       (const int32_t*)d.blk_c, d.cov, next, d.ended, d.ended_reason);
}

}  // namespace eppm
