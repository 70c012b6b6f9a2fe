// temporal.h -- the temporal prior of a streaming context: the previous pair's level-L displacement field moved
// along its own motion, shared by the kernels (k_temporal.hip) and the host form (eppm_io.cpp: eppm_temporal_prior_host) so that both state
// the same rule.  Integers only: nothing here rounds.
//
// A snapshot is a field of short2 DISPLACEMENTS on the grid of the previous pair's source image; a vector with a component <=
// kTemporalUnknown is unknown.  The prior is a field of short2 absolute TARGETS (what an NNF holds) on the grid of the new pair's source
// image; a pixel without a prior holds (kTemporalUnknown, kTemporalUnknown).
//   forward  (step +1): the snapshot lives on A's grid, the prior on B's.  A pixel p with displacement d lands on q = p + d and keeps d
//                       there (steady motion), so q's prior target is q + d.
//   backward (step -1): the snapshot lives on B's grid with targets in A, the prior on C's grid with targets in B.  A pixel p of B with
//                       backward displacement d moves to q = p - d in C and keeps d: prior target q + d (which is p).
// Several sources may land on one q: the smallest linear index y * w + x wins (an atomicMin on the device, whatever the order of the
// lanes).  q outside the level: the source is dropped.  Target outside the level: q has no prior.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define EPPM_HD __host__ __device__
#else
#define EPPM_HD
#endif

namespace eppm {

constexpr int kTemporalUnknown = -10000;     // INVALID_LOCATION (eppm_device.cuh: kInvalid)
constexpr int kTemporalNoKey = 0x7fffffff;   // INT_MAX: no source landed here

EPPM_HD inline bool temporal_known(int dx, int dy) { return dx > kTemporalUnknown && dy > kTemporalUnknown; }
EPPM_HD inline bool temporal_inside(int x, int y, int w, int h) { return x >= 0 && x < w && y >= 0 && y < h; }

// where the source pixel (x, y) with displacement (dx, dy) lands; false: it competes for no pixel
EPPM_HD inline bool temporal_landing(int x, int y, int dx, int dy, int step, int w, int h, int* qx, int* qy)
{
    if (!temporal_known(dx, dy)) return false;
    *qx = x + step * dx;
    *qy = y + step * dy;
    return temporal_inside(*qx, *qy, w, h);
}

// the prior of pixel (qx, qy) whose winning source carries (dx, dy); has_winner false: nothing landed
EPPM_HD inline void temporal_target(int qx, int qy, bool has_winner, int dx, int dy, int w, int h, int16_t* tx, int16_t* ty)
{
    const int x = qx + dx, y = qy + dy;
    const bool ok = has_winner && temporal_inside(x, y, w, h);
    *tx = (int16_t)(ok ? x : kTemporalUnknown);
    *ty = (int16_t)(ok ? y : kTemporalUnknown);
}

// displacement of a stored match (an NNF entry: absolute target, unknown where a component <= kTemporalUnknown) of pixel (x, y)
EPPM_HD inline void temporal_displacement(int x, int y, int tx, int ty, int16_t* dx, int16_t* dy)
{
    const bool ok = temporal_known(tx, ty);
    *dx = (int16_t)(ok ? tx - x : kTemporalUnknown);
    *dy = (int16_t)(ok ? ty - y : kTemporalUnknown);
}

}  // namespace eppm
