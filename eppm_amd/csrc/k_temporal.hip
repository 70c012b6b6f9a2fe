// k_temporal.hip -- the temporal prior of a streaming context (temporal.h): snapshots of a pair's level-L fields as
// displacements, and their advection into the next pair's initial guess.  The fields have ~28 k pixels (1024x436: 256x109), so every
// kernel here costs its launch: one lane per pixel in 256-lane workgroups (four full waves, coalesced short2 / int rows), both
// directions of the advection (blockIdx.y) and every slot of a batch context (blockIdx.z) in one launch.  The landing competition is an
// integer atomicMin on the source index -- the minimum does not depend on the order of the lanes -- and the gather pass that reads the
// winner puts the key back to "none", so the key planes are written once when they are allocated and never cleared by a launch of their
// own.  Indices are per slot (y * w + x inside the slot's planes): per slot the rule and its result are temporal.h's.  A slot that is not
// armed (TemporalArgs::armed) competes for nothing and gets "no prior" everywhere.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "temporal.h"

namespace eppm {

static_assert(kTemporalUnknown == kInvalid, "the prior's 'no prior' is the NNF's INVALID_LOCATION");

__global__ __launch_bounds__(256) void k_temporal_keys_init(int32_t* __restrict__ keys, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = kTemporalNoKey;
}

__device__ __forceinline__ bool temporal_armed(const TemporalArgs& A, unsigned slot) { return (A.armed[slot >> 5] >> (slot & 31)) & 1u; }

// pass 1: every source pixel with a known displacement competes for the pixel it lands on
__global__ __launch_bounds__(256) void k_temporal_splat(TemporalArgs A)
{
    const int dir = blockIdx.y, n = A.w * A.h;
    const unsigned slot = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !temporal_armed(A, slot)) return;
    const short2 d = reinterpret_cast<const short2*>(pair_ptr(A.prev[dir], A.stride, slot))[i];
    const int x = i % A.w, y = i / A.w;
    int qx, qy;
    if (temporal_landing(x, y, d.x, d.y, A.step[dir], A.w, A.h, &qx, &qy)) atomicMin(pair_ptr(A.keys[dir], A.stride, slot) + qy * A.w + qx, i);
}

// pass 2: every pixel reads its winner's displacement, writes its prior and leaves its key as it found the plane
__global__ __launch_bounds__(256) void k_temporal_gather(TemporalArgs A)
{
    const int dir = blockIdx.y, n = A.w * A.h;
    const unsigned slot = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t* keys = pair_ptr(A.keys[dir], A.stride, slot);
    const int k = keys[i];                      // a slot that is not armed was skipped by pass 1: its keys are all "none"
    const bool won = k != kTemporalNoKey;
    short2 d = make_short2(0, 0);
    if (won) {
        d = reinterpret_cast<const short2*>(pair_ptr(A.prev[dir], A.stride, slot))[k];
        keys[i] = kTemporalNoKey;
    }
    short2 t;
    temporal_target(i % A.w, i / A.w, won, d.x, d.y, A.w, A.h, &t.x, &t.y);
    reinterpret_cast<short2*>(pair_ptr(A.prior[dir], A.stride, slot))[i] = t;
}

void launch_temporal_keys_init(int32_t* keys, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_temporal_keys_init, dim3((n + 255) / 256), dim3(256), 0, s, keys, n);
}
void launch_temporal_splat(const TemporalArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_temporal_splat, dim3((a.w * a.h + 255) / 256, a.ndir, a.nslots), dim3(256), 0, s, a);
}
void launch_temporal_gather(const TemporalArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_temporal_gather, dim3((a.w * a.h + 255) / 256, a.ndir, a.nslots), dim3(256), 0, s, a);
}

// the displacement snapshot of a field of stored matches (pitch in short2 elements; the snapshot is unpitched), every pair of the batch in
// one launch (blockIdx.y): pair k's field lies k * pstride bytes after pair 0's, its snapshot k * prev_stride bytes
__global__ __launch_bounds__(256) void k_temporal_snapshot(int16_t* __restrict__ prev_, size_t prev_stride, const int16_t* __restrict__ nnf_,
                                                           int npitch, int w, int h, size_t pstride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= w * h) return;
    const int x = i % w, y = i / w;
    const short2 t = reinterpret_cast<const short2*>(pair_ptr(nnf_, pstride, blockIdx.y))[y * npitch + x];
    short2 d;
    temporal_displacement(x, y, t.x, t.y, &d.x, &d.y);
    reinterpret_cast<short2*>(pair_ptr(prev_, prev_stride, blockIdx.y))[i] = d;
}
void launch_temporal_snapshot(int16_t* prev, size_t prev_stride, const int16_t* nnf, int nnf_pitch, int w, int h, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_temporal_snapshot, dim3((w * h + 255) / 256, bt.n), dim3(256), 0, s, prev, prev_stride, nnf, nnf_pitch, w, h, bt.stride);
}

// k_nnf2flow (k_post.hip; refine :724-734) and the snapshot of the same field in one launch, every pair of the batch (blockIdx.z): the flow
// values are k_nnf2flow's, and the snapshot is their rintf (they are integers) with unknown vectors marked
__global__ __launch_bounds__(256) void k_nnf2flow_snapshot(float* __restrict__ flow_, int fpitch, int16_t* __restrict__ prev_, size_t prev_stride,
                                                           const int16_t* __restrict__ nnf_, int npitch, int w, int h, size_t pstride)
{
    float* __restrict__ flow = pair_ptr(flow_, pstride, blockIdx.z);
    const int16_t* __restrict__ nnf = pair_ptr(nnf_, pstride, blockIdx.z);
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    const int dx = nnf[(y * npitch + x) * 2], dy = nnf[(y * npitch + x) * 2 + 1];
    float fx, fy;
    if (dx <= kInvalid || dy <= kInvalid) { fx = kUnknownFlow; fy = kUnknownFlow; }
    else { fx = (float)(dx - x); fy = (float)(dy - y); }
    flow[(y * fpitch + x) * 2] = fx;
    flow[(y * fpitch + x) * 2 + 1] = fy;
    short2 d;
    temporal_displacement(x, y, dx, dy, &d.x, &d.y);
    reinterpret_cast<short2*>(pair_ptr(prev_, prev_stride, blockIdx.z))[y * w + x] = d;
}
void launch_nnf2flow_snapshot(float* flow, int flow_pitch, int16_t* prev, size_t prev_stride, const int16_t* nnf, int nnf_pitch, int w, int h,
                              hipStream_t s, Batch bt)
{
    dim3 block(64, 4), grid((w + 63) / 64, (h + 3) / 4, bt.n);
    hipLaunchKernelGGL(k_nnf2flow_snapshot, grid, block, 0, s, flow, flow_pitch, prev, prev_stride, nnf, nnf_pitch, w, h, bt.stride);
}

}  // namespace eppm
