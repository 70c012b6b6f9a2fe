// k_objects.hip -- moving-object detection (objects.h): connected-component labelling of the motion mask, one
// integer record per object, the identity rule and the carry of the labels to image 2.  A step of every slot it covers (blockIdx.z, or
// blockIdx.x of the one-wave kernels) is nine launches:
//   tile      a block of 64 x 4 lanes labels a tile of 64 x 16 pixels in LDS (label equivalence: link the root of a pixel's label to the
//             smallest neighbouring label with an LDS atomic, then flatten every label to its root, until nothing changes) and writes each
//             foreground pixel's parent -- the global linear index of its tile-local root -- and the sentinel for background, and at
//             every tile-local root's area word the pixels of its component in the tile (0 elsewhere).  It also clears the record table
//             and the vote table.
//   merge     one lane per foreground pixel of a tile's right or bottom border unions its tree with those of its neighbours across the
//             border.  The parent plane is read with relaxed agent-scope atomic loads and written with atomicMin only; a decision is taken
//             only on the value an atomic returned.
//   flatten   every foreground pixel follows its parents to the root and writes it to the root plane; a tile-local root that is not the
//             root adds its tile's count (left by the tile launch at its area word) to the root's area word.
//   count     a block per chunk of 1024 linear indices counts the roots and the roots with area >= min_area.
//   scan      one wave per slot: the exclusive scan of the chunk counts, n_components, n_found, n.
//   number    a block per chunk numbers its found roots in index order (ballot + lane prefix) and stores the label at the root's word of
//             the parent plane (0: dropped or beyond max_objects), with the object's area into its record.
//   label     a block per tile: the label bytes, the record sums (by label in LDS, then one set of atomics per label and tile), the vote
//             table V[label][carried].
//   assign    one wave per slot: the identity rule over V; ids, ages, prev tables, next_id.
//   carry     one lane per pixel of image 2: the label its backward vector points at.
// Every combine is at a launch boundary; no lane waits for another workgroup.  Every integer sum is exact, so the atomics' order does not
// show in the result: the same bits on every run, equal to the host forms'.  Adds to one address are pre-reduced: areas and record sums
// per tile in LDS, votes across the wave when all its active lanes share the address (a wave is 64 consecutive pixels of one row: the
// common case inside an object).
//
// Loops whose trip count depends on the data carry a cap derived from the invariant next to them; a lane that hits one stores 1 to the
// slot's error word and leaves the loop.  There is no EPPM_TOL branch: both libraries compile the same operations.
#include "eppm_device.cuh"
#include "eppm_internal.h"
#include "objects.h"

namespace eppm {

namespace {

constexpr uint32_t kBg = kObjBackground;
constexpr int kTilePx = kObjTileW * kObjTileH;

__device__ __forceinline__ bool ob_bit(const uint32_t* bits, unsigned slot) { return (bits[slot >> 5] >> (slot & 31)) & 1u; }

struct ObSlot {
    uint32_t* parent;
    uint32_t* root;
    uint32_t* area;
    uint8_t* labels;
    uint8_t* carried;
    uint32_t* chunks;
    ObjRecord* rec;
    uint32_t* votes;
    ObjHeader* hdr;
    int32_t* prev_id;
    int32_t* prev_age;
};

__device__ __forceinline__ ObSlot ob_slot(const ObjArgs& A, unsigned slot)
{
    char* blk = pair_ptr(A.mem, A.slot_stride, slot);
    ObSlot S;
    S.parent = reinterpret_cast<uint32_t*>(blk);
    S.root = reinterpret_cast<uint32_t*>(blk + A.off_root);
    S.area = reinterpret_cast<uint32_t*>(blk + A.off_area);
    S.labels = reinterpret_cast<uint8_t*>(blk + A.off_labels);
    S.carried = reinterpret_cast<uint8_t*>(blk + A.off_carried);
    S.chunks = reinterpret_cast<uint32_t*>(blk + A.off_chunks);
    S.rec = reinterpret_cast<ObjRecord*>(blk + A.off_rec);
    S.votes = reinterpret_cast<uint32_t*>(blk + A.off_votes);
    S.hdr = reinterpret_cast<ObjHeader*>(blk + A.off_hdr);
    S.prev_id = reinterpret_cast<int32_t*>(blk + A.off_hdr + sizeof(ObjHeader));
    S.prev_age = S.prev_id + kObjTable;
    return S;
}

__device__ __forceinline__ void ob_fail(ObjHeader* hdr) { hdr->err = 1u; }

__device__ __forceinline__ uint32_t ob_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a tile label in LDS that other lanes of the block rewrite meanwhile: relaxed workgroup-scope atomics, so that every access is made
__device__ __forceinline__ uint32_t ob_lds(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void ob_lds_set(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// base[key] += 1 for every lane with `has`, by one atomic per wave when the lanes share the key.  Called by whole waves.
__device__ __forceinline__ void ob_count(uint32_t* base, bool has, uint32_t key)
{
    const unsigned long long act = __ballot(has);
    if (!act) return;
    const int first = __ffsll(act) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)key, first, 64);
    if (__ballot(has && key != k0) == 0) {
        if ((int)threadIdx.x == first) atomicAdd(&base[k0], (uint32_t)__popcll(act));
    } else if (has)
        atomicAdd(&base[key], 1u);
}

__device__ __forceinline__ int ob_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void ob_add64(int64_t* p, int64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

}  // namespace

// ---- 1. tile labelling ----
__global__ __launch_bounds__(256) void k_obj_tile(ObjArgs A)
{
    __shared__ uint32_t lab[kTilePx], cnt[kTilePx];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const ObSlot S = ob_slot(A, slot);
    const uint8_t* __restrict__ mask = pair_ptr(A.mask, A.mask_stride, pair);
    const int lx = threadIdx.x, ty = threadIdx.y, x = blockIdx.x * kObjTileW + lx;
    const bool c8 = A.connectivity == 8;
    {   // the tables of the step, cleared by the whole grid of the slot
        const unsigned nthreads = gridDim.x * gridDim.y * 256u, t = (blockIdx.y * gridDim.x + blockIdx.x) * 256u + ty * 64u + lx;
        const unsigned nv = (unsigned)(A.max_objects + 1) * (unsigned)(A.max_objects + 1);
        for (unsigned i = t; i < nv; i += nthreads) S.votes[i] = 0u;
        for (unsigned i = t; i < (unsigned)kObjTable; i += nthreads) {
            ObjRecord r;
            obj_record_clear(&r);
            S.rec[i] = r;
        }
    }
    bool in[4], fg[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int ly = r * 4 + ty, y = blockIdx.y * kObjTileH + ly;
        in[r] = x < A.w && y < A.h;
        fg[r] = false;
        if (in[r]) {
            const size_t i = (size_t)y * A.w + x;
            fg[r] = obj_foreground(mask[i]);
        }
        lab[ly * kObjTileW + lx] = fg[r] ? (uint32_t)(ly * kObjTileW + lx) : kBg;
        cnt[ly * kObjTileW + lx] = 0u;
    }
    __syncthreads();
    // Invariant: lab[p] <= p, and an entry only ever decreases.  After a flatten every label is a root (lab[l] == l); a link makes one
    // root stop being one and none is ever created, so at most kTilePx rounds change anything.  Cap: kTilePx + 1 rounds.
    int round = 0;
    for (; round <= kTilePx; round++) {
        int changed = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (!fg[r]) continue;
            const int ly = r * 4 + ty, p = ly * kObjTileW + lx;
            const uint32_t l = ob_lds(lab + p);
            uint32_t m = l;
            const bool xl = lx > 0, xr = lx < kObjTileW - 1, yu = ly > 0, yd = ly < kObjTileH - 1;
            if (xl) m = min(m, ob_lds(lab + p - 1));
            if (xr) m = min(m, ob_lds(lab + p + 1));
            if (yu) m = min(m, ob_lds(lab + p - kObjTileW));
            if (yd) m = min(m, ob_lds(lab + p + kObjTileW));
            if (c8) {
                if (yu && xl) m = min(m, ob_lds(lab + p - kObjTileW - 1));
                if (yu && xr) m = min(m, ob_lds(lab + p - kObjTileW + 1));
                if (yd && xl) m = min(m, ob_lds(lab + p + kObjTileW - 1));
                if (yd && xr) m = min(m, ob_lds(lab + p + kObjTileW + 1));
            }
            if (m < l) {
                atomicMin(&lab[l], m);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (!fg[r]) continue;
            const int p = (r * 4 + ty) * kObjTileW + lx;
            // a chase visits strictly decreasing indices below kTilePx.  Cap: kTilePx steps.  An entry another lane rewrites meanwhile
            // holds an ancestor before and after, and a root is only rewritten by its own lane, with itself.
            uint32_t l = ob_lds(lab + p);
            int k = 0;
            for (; k < kTilePx; k++) {
                const uint32_t n = ob_lds(lab + l);
                if (n == l) break;
                l = n;
            }
            if (k == kTilePx) ob_fail(S.hdr);
            ob_lds_set(lab + p, l);
        }
        __syncthreads();
    }
    if (round > kTilePx) ob_fail(S.hdr);
    // the pixels of every tile-local component, counted at its root
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (fg[r]) atomicAdd(&cnt[lab[(r * 4 + ty) * kObjTileW + lx]], 1u);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (!in[r]) continue;
        const int ly = r * 4 + ty, y = blockIdx.y * kObjTileH + ly, p = ly * kObjTileW + lx;
        uint32_t out = kBg;
        if (fg[r]) {
            const uint32_t l = lab[p];
            out = (uint32_t)(blockIdx.y * kObjTileH + l / kObjTileW) * (uint32_t)A.w + (blockIdx.x * kObjTileW + l % kObjTileW);
        }
        S.parent[(size_t)y * A.w + x] = out;
        S.area[(size_t)y * A.w + x] = cnt[p];          // a tile-local root: its component's pixels in this tile; every other pixel: 0
    }
}

namespace {

// Invariant of the parent plane: parent[i] <= i for a foreground index and a word only ever decreases, so a chase visits strictly
// decreasing indices.  Cap: npx steps (an index is below npx).
__device__ __forceinline__ uint32_t ob_find_atomic(const uint32_t* parent, uint32_t i, uint32_t npx, ObjHeader* hdr)
{
    uint32_t r = i, k = 0;
    for (; k <= npx; k++) {
        const uint32_t p = ob_load(parent + r);
        if (p == r) return r;
        r = p;
    }
    ob_fail(hdr);
    return r;
}

// Union of the trees of a and b.  ra and rb start as hints (a stale parent is still an ancestor); the only decision -- "ra was a root and
// now hangs below rb" -- is taken on the value atomicMin returned.  Otherwise the word held old < ra, ra's parent: the obligation that is
// left is the union of old and rb, whichever of the two the word holds now.  max(ra, rb) strictly decreases from round to round.  Cap: npx
// rounds.
__device__ __forceinline__ void ob_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t npx, ObjHeader* hdr)
{
    uint32_t ra = ob_find_atomic(parent, a, npx, hdr), rb = ob_find_atomic(parent, b, npx, hdr), k = 0;
    for (; k <= npx; k++) {
        if (ra == rb) return;
        if (ra < rb) {
            const uint32_t t = ra;
            ra = rb;
            rb = t;
        }
        const uint32_t old = atomicMin(&parent[ra], rb);
        if (old == ra) return;
        ra = old;
    }
    ob_fail(hdr);
}

}  // namespace

// ---- 2. border merge ----
__global__ __launch_bounds__(256) void k_obj_merge(ObjArgs A)
{
    const unsigned slot = A.slot0 + blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const bool right = (x & (kObjTileW - 1)) == kObjTileW - 1 && x + 1 < A.w, bottom = (y & (kObjTileH - 1)) == kObjTileH - 1 && y + 1 < A.h;
    if (!right && !bottom) return;
    const ObSlot S = ob_slot(A, slot);
    const uint32_t npx = (uint32_t)A.h * (uint32_t)A.w, i = (uint32_t)y * (uint32_t)A.w + x;
    if (ob_load(S.parent + i) == kBg) return;
    const bool c8 = A.connectivity == 8;
    // a background word holds the sentinel throughout (only words reached from a foreground pixel are ever written), so whether a pixel is
    // foreground is a fact, not a hint
    auto is_fg = [&](int nx, int ny) {
        return nx >= 0 && nx < A.w && ny >= 0 && ny < A.h && ob_load(S.parent + ((uint32_t)ny * (uint32_t)A.w + nx)) != kBg;
    };
    auto join = [&](int nx, int ny) { ob_union(S.parent, i, (uint32_t)ny * (uint32_t)A.w + nx, npx, S.hdr); };
    // A union is left out where the tile labelling implies it.  The pair straight across the border, if the pair before it along the
    // border (in the same two tiles) is foreground too: those two pairs are neighbours inside their tiles, so one union joins all four.
    // The diagonal pairs, if the pixel straight across is foreground: it is a 4-neighbour of both diagonal pixels inside its tile.
    if (right) {
        if (is_fg(x + 1, y)) {
            if (!((y & (kObjTileH - 1)) != 0 && is_fg(x, y - 1) && is_fg(x + 1, y - 1))) join(x + 1, y);
        } else if (c8) {
            if (is_fg(x + 1, y - 1)) join(x + 1, y - 1);
            if (is_fg(x + 1, y + 1)) join(x + 1, y + 1);
        }
    }
    if (bottom) {
        if (is_fg(x, y + 1)) {
            if (!((x & (kObjTileW - 1)) != 0 && is_fg(x - 1, y) && is_fg(x - 1, y + 1))) join(x, y + 1);
        } else if (c8) {
            if (is_fg(x - 1, y + 1)) join(x - 1, y + 1);
            if (is_fg(x + 1, y + 1)) join(x + 1, y + 1);
        }
    }
}

// ---- 3. + 4. flatten, areas ----
__global__ __launch_bounds__(256) void k_obj_flatten(ObjArgs A)
{
    const unsigned slot = A.slot0 + blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    const bool in = x < A.w && y < A.h;
    const ObSlot S = ob_slot(A, slot);
    const uint32_t* __restrict__ parent = S.parent;          // not written in this launch
    const uint32_t npx = (uint32_t)A.h * (uint32_t)A.w;
    const size_t i = in ? (size_t)y * A.w + x : 0;
    uint32_t r = in ? parent[i] : kBg;
    const bool fg = r != kBg;
    if (fg) {
        // strictly decreasing indices below npx.  Cap: npx steps
        uint32_t k = 0;
        for (; k <= npx; k++) {
            const uint32_t p = parent[r];
            if (p == r) break;
            r = p;
        }
        if (k > npx) ob_fail(S.hdr);
    }
    if (in) S.root[i] = r;
    // the area of a component is the sum over its tile-local roots, which the tile launch left at their words: one add per tile-local
    // root that is not the root.  Only roots' words are added to, and only non-roots' words are read
    if (fg && r != (uint32_t)i) {
        const uint32_t local = S.area[i];
        if (local) atomicAdd(&S.area[r], local);
    }
}

// ---- 5a. roots per chunk ----
__global__ __launch_bounds__(256) void k_obj_count(ObjArgs A)
{
    __shared__ uint32_t part[4][2];
    const unsigned slot = A.slot0 + blockIdx.z, chunk = blockIdx.x, tid = threadIdx.x;
    const ObSlot S = ob_slot(A, slot);
    const uint32_t npx = (uint32_t)A.h * (uint32_t)A.w;
    uint32_t nf = 0, nc = 0;
#pragma unroll
    for (int k = 0; k < kObjChunk / 256; k++) {
        const uint32_t i = chunk * kObjChunk + k * 256 + tid;
        const bool isroot = i < npx && S.root[i] == i;
        const bool found = isroot && S.area[i] >= (uint32_t)A.min_area;
        nc += (uint32_t)__popcll(__ballot(isroot));
        nf += (uint32_t)__popcll(__ballot(found));
    }
    if ((tid & 63) == 0) part[tid >> 6][0] = nf, part[tid >> 6][1] = nc;
    __syncthreads();
    if (tid < 2) S.chunks[2 * chunk + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
}

// ---- 5b. the scan of the chunk counts ----
__global__ __launch_bounds__(64) void k_obj_scan(ObjArgs A)
{
    const unsigned slot = A.slot0 + blockIdx.x, lane = threadIdx.x;
    const ObSlot S = ob_slot(A, slot);
    uint32_t f = 0, c = 0;
    for (int base = 0; base < A.nchunks; base += 64) {
        const int k = base + (int)lane;
        const uint32_t cf = k < A.nchunks ? S.chunks[2 * k] : 0u, cc = k < A.nchunks ? S.chunks[2 * k + 1] : 0u;
        uint32_t incl = cf;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64);
            if ((int)lane >= off) incl += t;
        }
        if (k < A.nchunks) S.chunks[2 * k] = f + incl - cf;          // the chunk's first number - 1; nobody else reads this word here
        f += (uint32_t)__shfl((int)incl, 63, 64);
        c += (uint32_t)ob_wave_sum((int)cc);
    }
    if (lane == 0) {
        S.hdr->n_found = (int32_t)f;
        S.hdr->n_components = (int32_t)c;
        S.hdr->n = (int32_t)min(f, (uint32_t)A.max_objects);
    }
}

// ---- 5c. numbering ----
__global__ __launch_bounds__(256) void k_obj_number(ObjArgs A)
{
    __shared__ uint32_t wsum[4];
    const unsigned slot = A.slot0 + blockIdx.z, chunk = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ObSlot S = ob_slot(A, slot);
    const uint32_t npx = (uint32_t)A.h * (uint32_t)A.w;
    uint32_t run = S.chunks[2 * chunk];
#pragma unroll
    for (int k = 0; k < kObjChunk / 256; k++) {
        const uint32_t i = chunk * kObjChunk + k * 256 + tid;
        const bool isroot = i < npx && S.root[i] == i;
        const uint32_t a = isroot ? S.area[i] : 0u;
        const bool found = isroot && a >= (uint32_t)A.min_area;
        const unsigned long long bal = __ballot(found);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (unsigned q = 0; q < 4; q++) {
            tot += wsum[q];
            if (q < wave) pre += wsum[q];
        }
        if (isroot) {
            uint32_t num = 0;
            if (found) {
                num = run + pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)) + 1u;
                if (num > (uint32_t)A.max_objects) num = 0;
            }
            S.parent[i] = num;               // the flatten is done with the parent plane: a root's word now holds its label
            if (num) S.rec[num].area = (int32_t)a;
        }
        run += tot;
        __syncthreads();
    }
}

// ---- 6. label bytes, records, votes ----
__global__ __launch_bounds__(256) void k_obj_label(ObjArgs A)
{
    // the records' sums of one tile, by label: LDS atomics, then one set of global atomics per label the tile holds.  Inside a tile of
    // 1024 pixels |sum_x|, |sum_y| < 2^23; the vector sums are 64-bit
    __shared__ int tx0[kObjTable], tx1[kObjTable], ty0[kObjTable], ty1[kObjTable], tnf[kObjTable], tsx[kObjTable], tsy[kObjTable];
    __shared__ unsigned long long tqu[kObjTable], tqv[kObjTable];
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair, t = threadIdx.y * 64 + threadIdx.x;
    const ObSlot S = ob_slot(A, slot);
    const bool fresh = ob_bit(A.empty, slot);
    const float2* __restrict__ flow = reinterpret_cast<const float2*>(pair_ptr(A.fwd, A.fwd_stride, pair));
    tx0[t] = ty0[t] = 0x7fffffff;
    tx1[t] = ty1[t] = -1;
    tnf[t] = tsx[t] = tsy[t] = 0;
    tqu[t] = tqv[t] = 0ull;
    __syncthreads();
    const int x = blockIdx.x * kObjTileW + threadIdx.x;
#pragma unroll
    for (int r = 0; r < kObjTileH / 4; r++) {
        const int y = blockIdx.y * kObjTileH + r * 4 + threadIdx.y;
        const bool in = x < A.w && y < A.h;
        const size_t i = in ? (size_t)y * A.w + x : 0;
        const uint32_t root = in ? S.root[i] : kBg;
        const uint32_t lab = root != kBg ? S.parent[root] : 0u;
        if (in) S.labels[i] = (uint8_t)lab;
        int p = 0;
        if (lab) {
            atomicMin(&tx0[lab], x); atomicMax(&tx1[lab], x);
            atomicMin(&ty0[lab], y); atomicMax(&ty1[lab], y);
            atomicAdd(&tsx[lab], x); atomicAdd(&tsy[lab], y);
            const float2 f = flow[i];
            if (obj_flow_ok(f.x, f.y)) {
                atomicAdd(&tnf[lab], 1);
                atomicAdd(&tqu[lab], (unsigned long long)(long long)obj_quant(f.x));
                atomicAdd(&tqv[lab], (unsigned long long)(long long)obj_quant(f.y));
            }
            if (!fresh) p = obj_carried(S.carried[i], A.max_objects);
        }
        ob_count(S.votes, p != 0, lab * (uint32_t)(A.max_objects + 1) + (uint32_t)p);
    }
    __syncthreads();
    if (tx1[t] >= 0) {                           // label t has pixels in this tile
        ObjRecord* o = S.rec + t;
        atomicMin(&o->x0, tx0[t]); atomicMax(&o->x1, tx1[t]);
        atomicMin(&o->y0, ty0[t]); atomicMax(&o->y1, ty1[t]);
        ob_add64(&o->sum_x, tsx[t]); ob_add64(&o->sum_y, tsy[t]);
        if (tnf[t]) {
            atomicAdd(&o->n_flow, tnf[t]);
            atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_qu), tqu[t]);
            atomicAdd(reinterpret_cast<unsigned long long*>(&o->sum_qv), tqv[t]);
        }
    }
}

// ---- 7. the identity rule ----
__global__ __launch_bounds__(64) void k_obj_assign(ObjArgs A)
{
    __shared__ int32_t pid[kObjTable], page[kObjTable], nid[kObjTable], nage[kObjTable];
    __shared__ int best[kObjTable], winner[kObjTable];
    __shared__ uint32_t bestv[kObjTable];
    const unsigned slot = A.slot0 + blockIdx.x, lane = threadIdx.x;
    const ObSlot S = ob_slot(A, slot);
    const bool fresh = ob_bit(A.empty, slot);
    const int n = S.hdr->n, M = A.max_objects, stride = M + 1;
    int32_t next = fresh ? 1 : S.hdr->next_id;
    for (int k = lane; k < kObjTable; k += 64) {
        pid[k] = fresh ? 0 : S.prev_id[k];
        page[k] = fresh ? 0 : S.prev_age[k];
        nid[k] = nage[k] = 0;
        best[k] = winner[k] = 0;
        bestv[k] = 0u;
    }
    __syncthreads();
    for (int c = 1 + (int)lane; c <= n; c += 64) {
        uint32_t bv = 0;
        int bp = 0;
        for (int p = 1; p <= M; p++) {
            const uint32_t v = S.votes[c * stride + p];
            if (v > bv) bv = v, bp = p;          // ties to the lower p
        }
        best[c] = bp;
        bestv[c] = bv;
    }
    __syncthreads();
    for (int p = 1 + (int)lane; p <= M; p += 64) {
        uint32_t wv = 0;
        int wc = 0;
        for (int c = 1; c <= n; c++)
            if (best[c] == p && bestv[c] > wv) wv = bestv[c], wc = c;          // ties to the lower c
        winner[p] = wc;
    }
    __syncthreads();
    for (int base = 0; base < n; base += 64) {
        const int c = base + (int)lane + 1;
        const bool valid = c <= n;
        const int p = valid ? best[c] : 0;
        const bool inherit = valid && p != 0 && winner[p] == c && bestv[c] >= (uint32_t)A.min_overlap;
        const unsigned long long fresh_ids = __ballot(valid && !inherit);
        if (valid) {
            const int32_t id = inherit ? pid[p] : next + (int32_t)__popcll(fresh_ids & ((1ull << lane) - 1ull));
            const int32_t age = inherit ? page[p] + 1 : 0;
            nid[c] = id;
            nage[c] = age;
            S.rec[c].id = id;
            S.rec[c].age = age;
        }
        next += (int32_t)__popcll(fresh_ids);
    }
    __syncthreads();
    for (int k = lane; k < kObjTable; k += 64) {
        S.prev_id[k] = nid[k];
        S.prev_age[k] = nage[k];
    }
    if (lane == 0) S.hdr->next_id = obj_next_wrap(next);
}

namespace {

struct ObLabels {
    const uint8_t* __restrict__ labels;
    int w;
    __device__ uint8_t operator()(int x, int y) const { return labels[(size_t)y * w + x]; }
};

}  // namespace

// ---- 8. carry ----
__global__ __launch_bounds__(256) void k_obj_carry(ObjArgs A)
{
    const unsigned pair = blockIdx.z, slot = A.slot0 + pair;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= A.w || y >= A.h) return;
    const ObSlot S = ob_slot(A, slot);
    const size_t i = (size_t)y * A.w + x;
    uint8_t c = 0;
    if (A.bwd && A.occ2 && !ob_bit(A.cut, slot)) {
        const float2 f = reinterpret_cast<const float2*>(pair_ptr(A.bwd, A.bwd_stride, pair))[i];
        const uint8_t o = pair_ptr(A.occ2, A.occ_stride, pair)[i];
        c = obj_carry_pixel(x, y, f.x, f.y, o, A.h, A.w, ObLabels{S.labels, A.w});
    }
    S.carried[i] = c;
}

void launch_objects_label(const ObjArgs& a, hipStream_t s)
{
    const dim3 px((a.w + 63) / 64, (a.h + 3) / 4, a.n), blk(64, 4);
    hipLaunchKernelGGL(k_obj_tile, dim3(a.tiles_x, a.tiles_y, a.n), blk, 0, s, a);
    hipLaunchKernelGGL(k_obj_merge, px, blk, 0, s, a);
    hipLaunchKernelGGL(k_obj_flatten, px, blk, 0, s, a);
    hipLaunchKernelGGL(k_obj_count, dim3(a.nchunks, 1, a.n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_obj_scan, dim3(a.n), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_obj_number, dim3(a.nchunks, 1, a.n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_obj_label, dim3(a.tiles_x, a.tiles_y, a.n), blk, 0, s, a);
}

void launch_objects_assign(const ObjArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_obj_assign, dim3(a.n), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_obj_carry, dim3((a.w + 63) / 64, (a.h + 3) / 4, a.n), dim3(64, 4), 0, s, a);
}

}  // namespace eppm
