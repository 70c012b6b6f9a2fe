// k_pm_sweep.hip -- PatchMatch, propagation: the segmented sweeps in their classic, two-launch speculative and merged forms, and the
// reference's two alternative schemes (jump flood, neighbour).  Shared helpers and the tuning knobs: pm_device.cuh.
#include "pm_device.cuh"

namespace eppm {

// ---------------------------------------------------------------------------------------------------
// Segmented scan-line propagation (kernel.cu:1049-1181), cooperative form.
//
// A chain = (line, segment): up to L sequential steps, each one patch evaluation whose candidate depends
// on the previous step's outcome.  The reference gives a chain ONE thread; at quarter resolution that is
// ~45 waves on the whole chip.  Here one chain owns a DPP row of 16 lanes.  Per step the S*S samples of
// the patch (row-major, the reference's order) are dealt to the lanes in contiguous chunks of CH; every
// lane computes the (cost*w, w) terms of its chunk, then the two running sums travel lane to lane
// (row_ror:1) while every lane adds its chunk in order: the sums are formed in exactly the reference's
// sequential order, only the expensive per-sample terms are computed in parallel.
//
// Ordering points of the lockstep semantics:
//  (a) seeds are read from nnf_in, all writes go to nnf_out (ping-pong) -- no cross-workgroup hazard;
//  (b) forward pixel L: segment 1's first step precedes segment 0's last step; segments 0 and 1 of a
//      line are always in one workgroup (chains per line padded to an even count, 16 chains per
//      workgroup) and a workgroup barrier follows step 0.
// cost is updated in place: a pixel's cost is touched only by its visitor(s).
// ---------------------------------------------------------------------------------------------------
// LPC = lanes per chain (16, 32 or 64)
// TILE: the workgroup's CPB chains are SEGS consecutive segments of LINES lines of equal parity (y, y+2, ..): the sampled rows of
// neighbouring lines of one parity coincide (offsets -R, -R+2, .. R), so S + LINES - 1 rows of SEGS*L + 2R texels, plus the LINES
// lines themselves (patch centres), hold every source texel the workgroup's patches can touch.  They are staged in LDS once,
// clamped at load; the source half of the sample gathers then never reaches the L1 (which these launches load to 60 % at one
// 16-byte lane-fetch per clock, tools/ubench/gather_rate.hip).  TW = tile row length (odd: spreads a chain's ds_read_b128 over the banks).
// SPEC: phase B of the speculative form (see k_pm_sweep_spec below): a step that follows a rejection takes its cost from
// pr.spec; the stored match, cost and speculative cost of a chain's pixels are fetched once, before the first step, and
// handed to the steps through LDS (they are the only memory a cheap step needs).  Requires L_ <= kSpecMaxSteps.
// PRE (always with SPEC): the per-step global loads happen before the first step.  The classic form uses it for launches that cannot
// fill the chip (one 1024x436 pair): once the field has converged nearly every step is answered by the evaluation cache, and what a
// step then waits for is the round trip of its own loads -- 1.3 us per step, ten steps deep; fetched up front they cost one round trip.
// MERGED (classic form, PRE, no tile): one of the four in-place launches of the merged speculative form (k_pm_spec_all below): the
// workgroup's chains are listed units of this direction, seeds come from PmProblem::seed (the field as it stood before this sweep), a
// step's cost comes from the evaluation cache when the cache holds its candidate and is evaluated otherwise, only accepted candidates are
// written (in place: a pixel is written by its own visitors only), and an accepted candidate is passed on to the later directions of the
// iteration: their seed planes, and the unit of the pixel whose candidate it changes.
template <int R, int LPC, bool IS_ROW, bool REVERSE, bool TILE, bool SPEC = false, bool PRE = SPEC, bool MERGED = false>
__global__ __launch_bounds__(256) EPPM_SWEEP_OCC void k_pm_sweep(PmBatch B, const float* __restrict__ lut, int L_, int nseg, int nseg_pad, int TW)
{
    static_assert(PRE || !SPEC, "phase B fetches its chains' pixels up front");
    static_assert(!MERGED || (PRE && !SPEC && !TILE), "the merged form's sweeps are the classic form with up-front fetches, without a tile");
    // SPEC with a work list (pr.wl): the workgroup's CPB chains are CPB / 2 listed units (a unit = segments 2u, 2u + 1 of a line, so
    // that segments 0 and 1 -- the two visitors of pixel L -- always sit in one workgroup); a workgroup past the end of the list
    // returns at once.  Chains that are not listed keep their pixels: phase A has copied the whole field to the output plane.
    constexpr int S = R + 1, NS = S * S, CH = coop_chunk<R, LPC>(), CPB = 256 / LPC;
    static_assert((NS + CH - 1) / CH <= LPC, "a lane per chunk");
    constexpr int SEGS = SweepTile<LPC>::SEGS, LINES = SweepTile<LPC>::LINES, TROWS = S + LINES - 1;
    static_assert(!(SPEC && TILE), "phase B evaluates rarely: it gathers its source samples");
    extern __shared__ float4 s_tile[];          // TILE: TROWS sample rows + LINES centre rows of TW texels
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    __shared__ int s_own[PRE ? CPB * kSpecMaxSteps : 1];       // PRE: per chain and step, the pixel's stored match (x | y << 16),
    __shared__ float s_cst[PRE ? CPB * kSpecMaxSteps : 1];     //      its stored cost,
    __shared__ float s_spc[PRE ? CPB * kSpecMaxSteps : 1];     //      phase A's cost of the rejection-path candidate (classic form: the cached cost)
    __shared__ int s_ccd[(PRE && !SPEC) ? CPB * kSpecMaxSteps : 1];   // classic form: and the cached candidate
    load_patch_lut(L, lut, R, threadIdx.x, 256);
    // 1-D grid, problem = id mod nprob: workgroups are dealt to the 8 XCDs by id mod 8, so with 8 problems (4 pairs x 2 directions)
    // each problem's planes stay in ONE XCD's L2 instead of all problems' planes competing for every L2
    const unsigned nprob = B.n * B.npairs, bq = blockIdx.x % nprob, bxx = blockIdx.x / nprob;
    const PmProblem pr = pm_problem(B, bq);
    const Planes P = to_dev(pr.P);
    // (MERGED reads and writes one plane: no __restrict__ on either pointer then)
    typename std::conditional<MERGED, const int16_t*, const int16_t* __restrict__>::type nin = pr.nnf;
    typename std::conditional<MERGED, int16_t*, int16_t* __restrict__>::type nout = MERGED ? pr.nnf : pr.nnf_alt;
    float* __restrict__ cost = pr.cost;
    // this direction's planes of the evaluation cache (eppm_internal.h: PmProblem::spec / scand)
    constexpr int DIR = IS_ROW ? (REVERSE ? 2 : 0) : (REVERSE ? 3 : 1);
    const int16_t* __restrict__ seeds = MERGED ? pr.seed + DIR * B.seed_plane : nullptr;
    float* __restrict__ cval = pr.spec ? pr.spec + DIR * B.cache_plane : nullptr;
    int32_t* __restrict__ ccand = pr.scand ? pr.scand + DIR * B.cache_plane : nullptr;
    const int len = IS_ROW ? P.w : P.h, lines = IS_ROW ? P.h : P.w;
    const int grp = threadIdx.x / LPC, r = threadIdx.x % LPC;
    int line, seg, li = 0, line0 = 0, seg0 = 0;
    if (TILE) {
        // workgroup -> (group of 2*LINES lines, parity, group of SEGS segments); chain grp -> line li of the group, segment grp % SEGS
        const int nsg = nseg_pad / SEGS, sg = bxx % nsg, lp = bxx / nsg;
        line0 = (lp >> 1) * (2 * LINES) + (lp & 1);
        seg0 = sg * SEGS;
        li = grp / SEGS;
        line = line0 + 2 * li;
        seg = seg0 + grp % SEGS;
    } else {
        const int chain = bxx * CPB + grp;
        line = chain / nseg_pad;
        seg = chain % nseg_pad;
    }
    bool listed = true;
    if ((SPEC && pr.wl) || MERGED) {
        const uint32_t nlist = MERGED ? pr.wl[8 + 4 * (B.merged_it & 1) + DIR] : pr.wl[B.sweep_seq & 1];
        if (bxx * (CPB / 2) >= nlist) return;                         // (uniform over the workgroup, before any barrier)
        const unsigned slot = bxx * CPB + grp, upl = (unsigned)(nseg + 1) >> 1;
        listed = (slot >> 1) < nlist;
        const unsigned unit = listed ? pr.wl[(MERGED ? 16 + (6 + DIR) * B.wl_units : 16 + B.wl_units) + (slot >> 1)] : 0u;
        line = (int)(unit / upl);
        seg = (int)(unit % upl) * 2 + (int)(slot & 1);
    }
    const bool active = listed && (line < lines) && (seg < nseg);
    int start, count, i, step;
    if (!REVERSE) {
        start = (seg == 0) ? 0 : seg * L_ - 1;
        const int end = min(len - 1, start + L_);
        count = end - start;
        i = start + 1;
        step = 1;
    } else {
        start = (seg + 1) * L_;
        if (start >= len) start = len - 1;
        count = start - seg * L_;
        i = start - 1;
        step = -1;
    }
    const int abase = seg0 * L_ - R;                                  // TILE: along-line coordinate of tile column 0
    if (TILE) {
        if (line0 >= lines) return;                                   // the whole workgroup is past the last line
        for (int t = threadIdx.x; t < (TROWS + LINES) * TW; t += 256) {
            const int row = t / TW, c = t - row * TW;
            const int across = iclamp(row < TROWS ? line0 - R + 2 * row : line0 + 2 * (row - TROWS), 0, lines - 1);
            const int along = iclamp(abase + c, 0, len - 1);
            s_tile[t] = P.pk1[(unsigned)(IS_ROW ? across * P.pitch + along : along * P.pitch + across)];
        }
    }
    int px = 0, py = 0;
    if (active) {
        const int sidx = IS_ROW ? (line * B.npitch + start) : (start * B.npitch + line);
        px = MERGED ? seeds[sidx * 2] : nin[sidx * 2];
        py = MERGED ? seeds[sidx * 2 + 1] : nin[sidx * 2 + 1];
        // the one pixel of the line no chain visits keeps its value
        const bool copier = (REVERSE ? (seg == nseg - 1) : (seg == 0)) && !(SPEC && pr.wl) && !MERGED;     // (work list: phase A copied every pixel; merged: in place)
        if (copier && r == 0) {
            const int u = REVERSE ? len - 1 : 0;
            const int uidx = IS_ROW ? (line * B.npitch + u) : (u * B.npitch + line);
            nout[uidx * 2] = nin[uidx * 2];
            nout[uidx * 2 + 1] = nin[uidx * 2 + 1];
        }
    }
    if (PRE) {
        // the lanes of a chain fetch what its steps need: lane r the steps r, r + LPC, ...
        for (int sr = r; sr < L_; sr += LPC) {
            int own = 0, ccd = -1;
            float cst = 0.0f, spc = 0.0f;
            if (active && sr < count) {
                const int ir = i + sr * step;
                const int xr = IS_ROW ? ir : line, yr = IS_ROW ? line : ir;
                own = (int)(uint16_t)nin[(yr * B.npitch + xr) * 2] | ((int)nin[(yr * B.npitch + xr) * 2 + 1] << 16);
                cst = cost[yr * B.cpitch + xr];
                if (cval) spc = cval[yr * B.cpitch + xr];
                if (!SPEC && ccand) ccd = ccand[yr * B.cpitch + xr];
            }
            const int sl = grp * kSpecMaxSteps + sr;
            s_own[sl] = own; s_cst[sl] = cst; s_spc[sl] = spc;
            if (!SPEC) s_ccd[sl] = ccd;
        }
    }
    bool from_nin = true;                  // SPEC: the chain carries a stored match (seed, or the own match of a pixel that rejected)
    float cost_L = 0.0f;                   // SPEC: see the barrier after step 0
    __syncthreads();   // LUT ready
    const int t0 = r * CH;
    const int pitch16 = P.pitch << 4, wmax16 = (P.w - 1) << 4;
    // this lane's sample offsets (column in bytes), the same at every step: kept in registers by the classic form; phase B, which
    // evaluates rarely and runs up to 25 samples per lane, recomputes them at use (registers are what limits its waves)
    constexpr int NOFF = SPEC ? 1 : CH;
    int dj16[NOFF], di_[NOFF];
    int lo_[NOFF];                         // TILE: tile index of the sample when the chain stands at along-line coordinate 0
#pragma unroll
    for (int k = 0; k < NOFF; k++) {
        const int t = min(t0 + k, NS - 1);
        di_[k] = 2 * (t / S) - R;
        dj16[k] = (2 * (t % S) - R) * 16;
        lo_[k] = IS_ROW ? (li + t / S) * TW + (2 * (t % S) - R) - abase : (li + t % S) * TW + (2 * (t / S) - R) - abase;
    }
    const int lc = (TROWS + li) * TW - abase;                          // TILE: the same for the patch centre
    for (int s = 0; s < L_; s++) {
        if (active && s < count) {
            const int x = IS_ROW ? i : line, y = IS_ROW ? line : i;
            const int nidx = y * B.npitch + x, cidx = y * B.cpitch + x;
            const bool second_visit = (!REVERSE) && (seg == 0) && (s == L_ - 1) && (nseg > 1);   // pixel L, after segment 1
            float cur_best;
            int ox, oy;
            if (PRE) {
                const int sl = grp * kSpecMaxSteps + s, e = s_own[sl];
                ox = (int)(int16_t)(e & 0xffff); oy = e >> 16;
                cur_best = second_visit ? cost_L : s_cst[sl];         // segment 1 may have lowered pixel L's cost at its first step
            } else {
                cur_best = cost[cidx];
                ox = nin[nidx * 2]; oy = nin[nidx * 2 + 1];           // the pixel's own match, needed on rejection: fetched with the rest
            }
            int hit_cand = -1;                                        // classic form: this pixel's cached evaluation, fetched with the rest
            float hit_val = 0.0f;
            if (!PRE && ccand) { hit_cand = ccand[cidx]; hit_val = cval[cidx]; }
            // (fetched up front: at pixel L's second visit the entry may predate segment 1's evaluation; a stale entry is still a
            // valid (candidate, cost) pair -- at worst this step evaluates what the entry written meanwhile would have answered)
            if (PRE && !SPEC) { hit_cand = s_ccd[grp * kSpecMaxSteps + s]; hit_val = s_spc[grp * kSpecMaxSteps + s]; }
            if (IS_ROW) px = REVERSE ? max(px - 1, 0) : min(px + 1, P.w - 1);
            else        py = REVERSE ? max(py - 1, 0) : min(py + 1, P.h - 1);
            // A candidate equal to the pixel's current match would reproduce the stored cost bit for bit
            // (every cost in the plane was produced by this same sum), so "cv < cur_best" is false: the
            // reference evaluates and rejects it, here the evaluation is skipped.  Converged regions --
            // neighbours sharing one offset -- make this the common case after the first iterations.
            float cv = cur_best;
            const bool differs = !(px == ox && py == oy);
            const int cpack = (px & 0xffff) | (py << 16);
            if (SPEC && differs && from_nin) cv = s_spc[grp * kSpecMaxSteps + s];           // phase A evaluated exactly this candidate (now or earlier)
            else if (!SPEC && differs && hit_cand == cpack) cv = hit_val;                   // evaluated in an earlier sweep of this direction
            else if (differs) {
            const rgbf c1 = texel_rgb(TILE ? s_tile[lc + i] : tex_px(P.pk1, P.pitch, P.w, P.h, x, y));
            const rgbf c2 = texel_rgb(tex_px(P.pk2, P.pitch, P.w, P.h, px, py));
            float tc[CH], tw[CH];
            // gathers in flight per lane (EPPM_SWEEP_GB, EPPM_SWEEP_GB_SPEC)
            constexpr int GBW = SPEC ? EPPM_SWEEP_GB_SPEC : EPPM_SWEEP_GB;
            constexpr int GB = (CH < GBW) ? CH : GBW;
#pragma unroll
            for (int q0 = 0; q0 < CH; q0 += GB) {
                float4 q1[GB], q2[GB];
#pragma unroll
                for (int k = 0; k < GB; k++) {
                    const int qk = (q0 + k < CH) ? q0 + k : CH - 1;       // (the last batch may be partial: its spare slots repeat the last sample)
                    int dj, di;
                    if (SPEC) {
                        int t0v = t0;
                        asm volatile("" : "+v"(t0v));          // keeps the 25 offset pairs from being hoisted out of the step loop into registers
                        const int t = min(t0v + qk, NS - 1);
                        di = 2 * (t / S) - R; dj = (2 * (t % S) - R) * 16;
                    } else { di = di_[qk]; dj = dj16[qk]; }
                    q1[k] = TILE ? s_tile[lo_[SPEC ? 0 : qk] + i]
                                 : texel_at(P.pk1, texel_off16(pitch16, wmax16, P.h - 1, (x << 4) + dj, y + di));
                    q2[k] = texel_at(P.pk2, texel_off16(pitch16, wmax16, P.h - 1, (px << 4) + dj, py + di));
                }
#pragma unroll
                for (int k = 0; k < GB; k++) {
                    const int q = q0 + k;
                    if (q < CH) {
                        const int t = t0 + q;
                        tc[q] = 0.0f; tw[q] = 0.0f;
                        if (t < NS) patch_terms(q1[k], q2[k], c1, c2, L.gsp[t], L.tab(), tc[q], tw[q]);
                    }
                }
            }
            // the sums in their defined order (coop_chain_sum): complete in the lane of the last chunk
            float ac = 0.0f, aw = 0.0f;
            constexpr int NL = (NS + CH - 1) / CH;       // lanes that own samples
            coop_chain_sum<LPC, CH, NS, NL>(tc, tw, ac, aw);
            const int src = ((threadIdx.x & 63) / LPC) * LPC + (NL - 1);   // lane holding the complete sums (wave-relative)
            const float cs = __shfl(ac, src, 64), ws = __shfl(aw, src, 64);
            cv = cs / ws;
            if (!SPEC && ccand && r == 0) { ccand[cidx] = cpack; cval[cidx] = cv; }
            }
            if (cv < cur_best) {
                if (r == 0) {
                    nout[nidx * 2] = (int16_t)px;
                    nout[nidx * 2 + 1] = (int16_t)py;
                    cost[cidx] = cv;
                    if (MERGED) {
                        // the later sweeps of this iteration start from the field this sweep leaves: their seeds, and the chain whose
                        // candidate at the next pixel in THEIR direction has just changed
#pragma unroll
                        for (int d2 = DIR + 1; d2 < 4; d2++) {
                            int16_t* sd = pr.seed + d2 * B.seed_plane;
                            sd[nidx * 2] = (int16_t)px; sd[nidx * 2 + 1] = (int16_t)py;
                            const int qx = (d2 == 2) ? x - 1 : x, qy = (d2 == 1) ? y + 1 : (d2 == 3) ? y - 1 : y;
                            if (qx >= 0 && qy >= 0 && qx < P.w && qy < P.h) merged_list_unit(pr.wl, B, d2, qx, qy);
                        }
                    }
                }
                from_nin = false;
            } else {
                if (r == 0 && !second_visit && !MERGED) {
                    nout[nidx * 2] = (int16_t)ox;
                    nout[nidx * 2 + 1] = (int16_t)oy;
                }
                px = ox; py = oy;
                from_nin = true;
            }
            i += step;
        }
        if (!REVERSE && s == 0) {
            __syncthreads();   // (b)
            // SPEC: pixel L's cost as segment 1's first step left it, for segment 0's last step (fetched here, by value: a select
            // between this global address and the LDS copy at the point of use would turn both loads into flat_load)
            if (PRE && active && seg == 0 && nseg > 1 && L_ < len) cost_L = cost[IS_ROW ? line * B.cpitch + L_ : L_ * B.cpitch + line];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Speculative form of a sweep, for the iterations in which few candidates are accepted (from the third iteration on fewer
// than one step in ten, tools/sweep_stats.py): phase A + phase B, same results bit for bit.
//
// The candidate a chain tries at pixel i is shift(p) where p is what the chain carries out of pixel i-1: the match it accepted
// there, or -- when pixel i-1 REJECTED its candidate (and at a segment's first step, whose seed is pixel i-1) -- pixel i-1's own
// match nin[i-1].  So for every visited pixel the candidate on the rejection path, shift(nin[i-1]), is known before the sweep
// starts and its cost does not depend on the chain's history (the patch cost is a pure function of (pixel, candidate)):
//  phase A (k_pm_sweep_spec): evaluates E(i, shift(nin[i-1])) for every visited pixel in parallel -- no dependent steps, one
//      evaluation per lane with the source samples from an LDS tile; pixels whose candidate equals their own match are skipped
//      (the skip rule), the rest are compacted inside the workgroup so that whole waves work or exit;
//  phase B (k_pm_sweep<.., SPEC>): the chains walk their pixels in the reference's order as before, but a step that follows a
//      rejection takes its cost from phase A's plane; only a step that follows an ACCEPTED candidate evaluates (cooperatively,
//      as in the classic form).  In the converged iterations phase B is ten compare-and-select steps.
// ---------------------------------------------------------------------------------------------------
//
// Work list (pr.wl): phase A also knows which chains can change anything.  A chain leaves the rejection path only where a
// rejection-path candidate is ACCEPTED, i.e. where E(i, shift(nin[i-1])) < cost[i]; a chain without such a pixel rejects at every
// step (by induction it never carries anything but stored matches) and writes back what it read.  So phase A copies the field to
// the output plane, tests every visited pixel (evaluated now, taken from the cache, or skipped by the skip rule: never accepted)
// and appends the UNIT of a pixel that would accept -- segments 2u and 2u + 1 of its line, so that segments 0 and 1, the two
// visitors of pixel L, are always listed together -- to the list, once (a stamp per unit holds the number of the last sweep that
// listed it).  Phase B walks the listed chains only: from the fifth iteration on that is one chain in ten.
template <int RT, bool IS_ROW, bool REVERSE, int PK = 0>
__global__ __launch_bounds__(256) void k_pm_sweep_spec(PmBatch B, const float* __restrict__ lut, int R, int gx, int L_, int nseg)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = (RT == 0) ? 1 : kBlock + 2 * RT;
    constexpr int DIR = IS_ROW ? (REVERSE ? 2 : 0) : (REVERSE ? 3 : 1);
    __shared__ float4 s_src[TW * TW];
    __shared__ EPPM_LUT_ALIGN LUT L;
    __shared__ uint32_t s_list[256];       // compacted work: pixel index inside the block
    __shared__ int s_cand[256];            // its candidate, x | y << 16
    __shared__ int s_wcount[4];
    const unsigned nprob = B.n * B.npairs, bq = blockIdx.x % nprob, brest = blockIdx.x / nprob;
    const int bxx = brest % gx, byy = brest / gx;
    const PmProblem pr = pm_problem(B, bq);
    const Planes P = to_dev(pr.P);
    float* __restrict__ cval = pr.spec + DIR * B.cache_plane;
    int32_t* __restrict__ ccand = pr.scand ? pr.scand + DIR * B.cache_plane : nullptr;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x = bxx * kBlock + (tid & 15), y = byy * kBlock + (tid >> 4);
    // the pixel the chain comes from: one step against the sweep direction; the first pixel of a line is never visited
    const int qx = IS_ROW ? (REVERSE ? x + 1 : x - 1) : x, qy = IS_ROW ? y : (REVERSE ? y + 1 : y - 1);
    bool need = false;
    int cpack = 0;
    uint32_t* __restrict__ wl = pr.wl;
    const unsigned upl = (unsigned)(nseg + 1) >> 1, seq1 = (unsigned)B.sweep_seq + 1u;
    // lists the unit of pixel (px, py) for this sweep, once
    auto list_unit = [&](int px, int py) {
        const int along = IS_ROW ? px : py, ln = IS_ROW ? py : px;
        const unsigned seg = (!REVERSE && along < L_) ? 0u : (unsigned)(along / L_);
        const unsigned unit = (unsigned)ln * upl + (seg >> 1);
        if (atomicMax(&wl[16 + unit], seq1) < seq1) wl[16 + B.wl_units + atomicAdd(&wl[B.sweep_seq & 1], 1u)] = unit;
    };
    if (wl && blockIdx.x < nprob && tid == 0) wl[(B.sweep_seq + 1) & 1] = 0u;        // the next sweep's list length (the previous sweep is done with it)
    if (x < P.w && y < P.h) {
        const int ni = (y * B.npitch + x) * 2;
        const int ox = pr.nnf[ni], oy = pr.nnf[ni + 1];
        if (wl) { pr.nnf_alt[ni] = (int16_t)ox; pr.nnf_alt[ni + 1] = (int16_t)oy; }   // a pixel no listed chain visits keeps its match
        if (qx >= 0 && qy >= 0 && qx < P.w && qy < P.h) {
            const int qi = (qy * B.npitch + qx) * 2;
            int cx = pr.nnf[qi], cy = pr.nnf[qi + 1];
            if (IS_ROW) cx = REVERSE ? max(cx - 1, 0) : min(cx + 1, P.w - 1);
            else        cy = REVERSE ? max(cy - 1, 0) : min(cy + 1, P.h - 1);
            cpack = (cx & 0xffff) | (cy << 16);
            need = !(cx == ox && cy == oy);                              // equal to the pixel's own match: rejected unevaluated
            if (need && ccand && ccand[y * B.cpitch + x] == cpack) {     // evaluated in an earlier sweep of this direction: the cost stands
                need = false;
                if (wl && cval[y * B.cpitch + x] < pr.cost[y * B.cpitch + x]) list_unit(x, y);
            }
        }
    }
    // compaction: wave-level ballot + prefix, then the four wave counts: whole waves work or exit
    const unsigned long long bal = __ballot(need);
    if (lane == 0) s_wcount[wv] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const int c = s_wcount[k]; if (k < wv) base += c; total += c; }
    if (total == 0) return;                   // every candidate of the block is known (converged field): no tile, no table
    load_patch_lut(L, lut, R, tid, 256);
    if (RT != 0) pm_stage_tile<RT>(s_src, P, bxx, byy, tid);
    if (need) {
        const int slot = base + __popcll(bal & ((1ull << lane) - 1ull));
        s_list[slot] = (uint32_t)tid;
        s_cand[slot] = cpack;
    }
    __syncthreads();                          // LUT, tile, list
    if (RT == 17 && total <= EPPM_SPEC_COOP17_MAX) {          // few evaluations: a wave each, four at a time (pm_device.cuh)
        for (int slot = tid >> 6; slot < total; slot += 4) {
            const int pix = (int)s_list[slot], e = s_cand[slot];
            const int px = bxx * kBlock + (pix & 15), py = byy * kBlock + (pix >> 4);
            const float cv = coop_patch_dist<(RT == 17 ? 17 : 1), 64>(P, L, s_src, TW, pix & 15, pix >> 4, (int)(int16_t)(e & 0xffff), e >> 16, tid & 63);
            if ((tid & 63) == 0) {
                cval[py * B.cpitch + px] = cv;
                if (ccand) ccand[py * B.cpitch + px] = e;
                if (wl && cv < pr.cost[py * B.cpitch + px]) list_unit(px, py);
            }
        }
        return;
    }
    if (tid >= total) return;
    const int pix = (int)s_list[tid], e = s_cand[tid];
    const int tx = pix & 15, ty = pix >> 4;
    const int px = bxx * kBlock + tx, py = byy * kBlock + ty;
    // (radius 17: gathering the 4-byte target plane here as the search does changes nothing: 57.5 vs 57.6 ms PatchMatch at 3840x2160)
    const float cv = search_patch_dist<RT, PK>(P, L, R, s_src, TW, tx, ty, px, py, (int)(int16_t)(e & 0xffff), e >> 16, pr.P);
    cval[py * B.cpitch + px] = cv;
    if (ccand) ccand[py * B.cpitch + px] = e;
    if (wl && cv < pr.cost[py * B.cpitch + px]) list_unit(px, py);
}

// ---------------------------------------------------------------------------------------------------
// Merged form: ONE phase A for the four sweeps of an iteration (late iterations: nearly every candidate is answered by the cache, and
// what a phase-A launch then costs is the launch).  From the field F0 the iteration starts with, for every pixel and every direction d the
// rejection-path candidate shift_d(F0[i - 1_d]) is tested exactly as k_pm_sweep_spec tests it (skip rule, cache, evaluation) and the unit
// is listed when the candidate would be accepted against the pixel's cost.  The four sweeps then run as in-place launches over their lists
// (k_pm_sweep<.., MERGED>).  Why the lists stay complete although sweeps 1..3 see a field the earlier sweeps have changed:
//  * a chain leaves the rejection path first at a pixel i whose candidate shift_d(F[i - 1_d]) is accepted.  If pixel i - 1_d still holds its
//    F0 match, that candidate is the one tested here, against a cost that can only have fallen since: listed.  If an earlier sweep of the
//    iteration changed pixel i - 1_d, that sweep listed the unit of pixel i for direction d when it accepted (k_pm_sweep, MERGED);
//  * the cache answers by candidate, so an entry written here for a candidate the field no longer proposes is simply not used;
//  * seeds: PmProblem::seed[d] = F0 here, kept current by the earlier sweeps' accepted candidates, never by sweep d itself.
// ---------------------------------------------------------------------------------------------------
template <int RT, int PK = 0>
__global__ __launch_bounds__(256) void k_pm_spec_all(PmBatch B, const float* __restrict__ lut, int R, int gx)
{
    using LUT = typename SearchLut<RT>::type;
    constexpr int TW = kBlock + 2 * RT;
    __shared__ float4 s_src[TW * TW];
    __shared__ EPPM_LUT_ALIGN LUT L;
    __shared__ uint16_t s_list[1024];      // compacted work: pixel index inside the block | direction << 8
    __shared__ int s_cand[1024];           // its candidate, x | y << 16
    __shared__ int s_wcount[16];           // [direction][wave]
    const unsigned nprob = B.n * B.npairs, bq = blockIdx.x % nprob, brest = blockIdx.x / nprob;
    const int bxx = brest % gx, byy = brest / gx;
    const PmProblem pr = pm_problem(B, bq);
    const Planes P = to_dev(pr.P);
    uint32_t* __restrict__ wl = pr.wl;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x = bxx * kBlock + (tid & 15), y = byy * kBlock + (tid >> 4);
    if (blockIdx.x < nprob && tid < 4) wl[8 + 4 * ((B.merged_it + 1) & 1) + tid] = 0u;      // the next iteration's list lengths
    unsigned needmask = 0;
    int cpack[4] = {0, 0, 0, 0};
    if (x < P.w && y < P.h) {
        const int ni = (y * B.npitch + x) * 2, ci = y * B.cpitch + x;
        const uint32_t* __restrict__ nnf32 = reinterpret_cast<const uint32_t*>(pr.nnf);       // a match as one word: x | y << 16
        const uint32_t own = nnf32[ni >> 1];
        const int ox = (int)(int16_t)(own & 0xffffu), oy = (int)(int16_t)(own >> 16);
        const float c0 = pr.cost[ci];
#pragma unroll
        for (int d = 0; d < 4; d++) {
            reinterpret_cast<uint32_t*>(pr.seed + d * B.seed_plane)[ni >> 1] = own;
            const int qx = (d == 0) ? x - 1 : (d == 2) ? x + 1 : x, qy = (d == 1) ? y - 1 : (d == 3) ? y + 1 : y;
            if (qx >= 0 && qy >= 0 && qx < P.w && qy < P.h) {
                const uint32_t qm = nnf32[qy * B.npitch + qx];
                int cx = (int)(int16_t)(qm & 0xffffu), cy = (int)(int16_t)(qm >> 16);
                if (d == 0) cx = min(cx + 1, P.w - 1);
                else if (d == 1) cy = min(cy + 1, P.h - 1);
                else if (d == 2) cx = max(cx - 1, 0);
                else cy = max(cy - 1, 0);
                const int cp = (cx & 0xffff) | (cy << 16);
                bool need = !(cx == ox && cy == oy);                             // equal to the pixel's own match: rejected unevaluated
                if (need && pr.scand[d * B.cache_plane + ci] == cp) {            // evaluated before: the cost stands
                    need = false;
                    if (pr.spec[d * B.cache_plane + ci] < c0) merged_list_unit(wl, B, d, x, y);
                }
                if (need) { needmask |= 1u << d; cpack[d] = cp; }
            }
        }
    }
    unsigned long long bal[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        bal[d] = __ballot((needmask >> d) & 1u);
        if (lane == 0) s_wcount[d * 4 + wv] = __popcll(bal[d]);
    }
    __syncthreads();
    int total = 0, base[4];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if ((k & 3) == 0) base[k >> 2] = total;              // start of direction k/4 ...
        const int c = s_wcount[k];
        if ((k & 3) < wv) base[k >> 2] += c;                 // ... plus the lower waves of that direction
        total += c;
    }
    if (total == 0) return;
    load_patch_lut(L, lut, R, tid, 256);
    pm_stage_tile<RT>(s_src, P, bxx, byy, tid);
#pragma unroll
    for (int d = 0; d < 4; d++)
        if ((needmask >> d) & 1u) {
            const int slot = base[d] + __popcll(bal[d] & ((1ull << lane) - 1ull));
            s_list[slot] = (uint16_t)(tid | (d << 8));
            s_cand[slot] = cpack[d];
        }
    __syncthreads();                          // table, tile, list
    if (RT == 17 && total <= EPPM_SPEC_COOP17_MAX) {          // few evaluations: a wave each (see k_pm_sweep_spec)
        for (int slot = tid >> 6; slot < total; slot += 4) {
            const int pix = (int)s_list[slot] & 255, d = (int)s_list[slot] >> 8, e = s_cand[slot];
            const int px = bxx * kBlock + (pix & 15), py = byy * kBlock + (pix >> 4), ci = py * B.cpitch + px;
            const float cv = coop_patch_dist<(RT == 17 ? 17 : 1), 64>(P, L, s_src, TW, pix & 15, pix >> 4, (int)(int16_t)(e & 0xffff), e >> 16, tid & 63);
            if ((tid & 63) == 0) {
                pr.spec[d * B.cache_plane + ci] = cv;
                pr.scand[d * B.cache_plane + ci] = e;
                if (cv < pr.cost[ci]) merged_list_unit(wl, B, d, px, py);
            }
        }
        return;
    }
    if (RT == 9 && total <= EPPM_MERGED_COOP9_MAX) {          // few evaluations: 16 lanes each, all at once (pm_device.cuh)
        constexpr int CL = EPPM_LPC9_SPEC;            // lanes per evaluation: 16 (tolerance library: 32, a lane = a chunk)
        for (int slot = tid / CL; slot < total; slot += 256 / CL) {
            const int pix = (int)s_list[slot] & 255, d = (int)s_list[slot] >> 8, e = s_cand[slot];
            const int px = bxx * kBlock + (pix & 15), py = byy * kBlock + (pix >> 4), ci = py * B.cpitch + px;
            const float cv = coop_patch_dist<(RT == 9 ? 9 : 1), CL>(P, L, s_src, TW, pix & 15, pix >> 4, (int)(int16_t)(e & 0xffff), e >> 16, tid % CL);
            if ((tid % CL) == 0) {
                pr.spec[d * B.cache_plane + ci] = cv;
                pr.scand[d * B.cache_plane + ci] = e;
                if (cv < pr.cost[ci]) merged_list_unit(wl, B, d, px, py);
            }
        }
        return;
    }
    for (int slot = tid; slot < total; slot += 256) {
        const int pix = (int)s_list[slot] & 255, d = (int)s_list[slot] >> 8, e = s_cand[slot];
        const int tx = pix & 15, ty = pix >> 4;
        const int px = bxx * kBlock + tx, py = byy * kBlock + ty, ci = py * B.cpitch + px;
        const float cv = search_patch_dist<RT, PK>(P, L, R, s_src, TW, tx, ty, px, py, (int)(int16_t)(e & 0xffff), e >> 16, pr.P);
        pr.spec[d * B.cache_plane + ci] = cv;
        pr.scand[d * B.cache_plane + ci] = e;
        if (cv < pr.cost[ci]) merged_list_unit(wl, B, d, px, py);
    }
}

// Fallback for patch radii without a cooperative instantiation: the reference's one-thread-per-chain form,
// in place, all segments of a line in one workgroup (seed reads / pixel-L order by workgroup barriers).
template <bool IS_ROW, bool REVERSE>
__global__ __launch_bounds__(1024) void k_pm_seg_propagate(PmBatch B, const float* __restrict__ lut, int R, int L_, int nseg,
                                                           int lines_per_block)
{
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    load_patch_lut(L, lut, R, threadIdx.x, blockDim.x);
    const PmProblem pr = pm_problem(B, blockIdx.y);
    const Planes P = to_dev(pr.P);
    int16_t* __restrict__ nnf = pr.nnf;
    float* __restrict__ cost = pr.cost;
    const int len = IS_ROW ? P.w : P.h, lines = IS_ROW ? P.h : P.w;
    const int lline = threadIdx.x / nseg, seg = threadIdx.x % nseg;
    const int line = blockIdx.x * lines_per_block + lline;
    const bool active = (lline < lines_per_block) && (line < lines);
    int start, count, i, step;
    if (!REVERSE) {
        start = (seg == 0) ? 0 : seg * L_ - 1;
        const int end = min(len - 1, start + L_);
        count = end - start;
        i = start + 1;
        step = 1;
    } else {
        start = (seg + 1) * L_;
        if (start >= len) start = len - 1;
        count = start - seg * L_;
        i = start - 1;
        step = -1;
    }
    int px = 0, py = 0;
    if (active) {
        const int sidx = IS_ROW ? (line * B.npitch + start) : (start * B.npitch + line);
        px = nnf[sidx * 2];
        py = nnf[sidx * 2 + 1];
    }
    __syncthreads();   // LUT ready; (a) all seeds read
    for (int s = 0; s < L_; s++) {
        if (active && s < count) {
            const int x = IS_ROW ? i : line, y = IS_ROW ? line : i;
            const int nidx = y * B.npitch + x, cidx = y * B.cpitch + x;
            const float cur_best = cost[cidx];
            if (IS_ROW) px = REVERSE ? max(px - 1, 0) : min(px + 1, P.w - 1);
            else        py = REVERSE ? max(py - 1, 0) : min(py + 1, P.h - 1);
            const bool same = (px == nnf[nidx * 2]) && (py == nnf[nidx * 2 + 1]);   // would reproduce cur_best: rejected
            const float cv = same ? cur_best : patch_dist(P, L, R, x, y, px, py);
            if (cv < cur_best) {
                nnf[nidx * 2] = (int16_t)px;
                nnf[nidx * 2 + 1] = (int16_t)py;
                cost[cidx] = cv;
            } else {
                px = nnf[nidx * 2];
                py = nnf[nidx * 2 + 1];
            }
            i += step;
        }
        if (!REVERSE && s == 0) __syncthreads();   // (b)
    }
}

// dir (0 row forward, 1 column forward, 2 row reverse, 3 column reverse) as the kernels' <IS_ROW, REVERSE>: f(row, rev) gets two std::bool_constant
template <class F>
static void with_dir(int dir, F&& f)
{
    switch (dir) {
        case 0: f(std::true_type{}, std::false_type{}); break;
        case 1: f(std::false_type{}, std::false_type{}); break;
        case 2: f(std::true_type{}, std::true_type{}); break;
        default: f(std::false_type{}, std::true_type{}); break;
    }
}
// the chains of one direction: `lines` lines of len pixels, each cut into nseg segments of seg_len steps
struct SweepGeom {
    int len, lines, nseg;
    SweepGeom(int w, int h, int dir, int seg_len)
    {
        const bool is_row = (dir == 0 || dir == 2);
        len = is_row ? w : h; lines = is_row ? h : w;
        nseg = (len + seg_len - 1) / seg_len;
    }
    SweepGeom(const PmBatch& b, int dir, int seg_len) : SweepGeom(b.p[0].P.w, b.p[0].P.h, dir, seg_len) {}
    int nseg_pad() const { return (nseg + 1) & ~1; }                                    // segments 0 and 1 of a line in one workgroup
    int wgs(int cpb) const { return (lines * nseg_pad() + cpb - 1) / cpb; }             // workgroups of cpb chains, without a tile
};

// phase A of the speculative form for one direction
template <int RT>
static void launch_sweep_spec(const PmBatch& b, const float* lut, int R, int dir, int seg_len, int nseg, hipStream_t s)
{
    const int w = b.p[0].P.w, h = b.p[0].P.h, gx = (w + kBlock - 1) / kBlock, gy = (h + kBlock - 1) / kBlock;
    dim3 grid(gx * gy * (b.n * b.npairs)), block(256);
    if (pm_has_parity(b, RT, EPPM_PARITY_SPEC))
        with_dir(dir, [&](auto row, auto rev) { hipLaunchKernelGGL((k_pm_sweep_spec<RT, row(), rev(), 2>), grid, block, 0, s, b, lut, R, gx, seg_len, nseg); });
    else
        with_dir(dir, [&](auto row, auto rev) { hipLaunchKernelGGL((k_pm_sweep_spec<RT, row(), rev()>), grid, block, 0, s, b, lut, R, gx, seg_len, nseg); });
}
int pm_worklist_units(int w, int h, int seg_len)
{
    const int ur = h * (((w + seg_len - 1) / seg_len + 1) / 2), uc = w * (((h + seg_len - 1) / seg_len + 1) / 2);
    return ur > uc ? ur : uc;
}
// the sweeps over listed chains: phase B of the two-launch form, or (MERGED) one of the merged form's four in-place sweeps
template <int R, int LPC, bool MERGED = false>
static void launch_sweep_b(const PmBatch& b, const float* lut, int seg_len, int dir, const SweepGeom& g, hipStream_t s)
{
    dim3 grid(g.wgs(256 / LPC) * (b.n * b.npairs)), block(256);
    with_dir(dir, [&](auto row, auto rev) {
        hipLaunchKernelGGL((k_pm_sweep<R, LPC, row(), rev(), false, !MERGED, true, MERGED>), grid, block, 0, s, b, lut, seg_len, g.nseg, g.nseg_pad(), 0);
    });
}
template <int R, int LPC, bool TILE, bool PRE = false>
static void launch_sweep_t(const PmBatch& b, const float* lut, int seg_len, int dir, const SweepGeom& g, hipStream_t s)
{
    constexpr int SEGS = SweepTile<LPC>::SEGS, LINES = SweepTile<LPC>::LINES;
    const int nseg_pad = TILE ? (g.nseg + SEGS - 1) / SEGS * SEGS : g.nseg_pad();
    const int wgs = TILE ? ((g.lines + 2 * LINES - 1) / (2 * LINES)) * 2 * (nseg_pad / SEGS) : g.wgs(256 / LPC);
    const int TW = (SEGS * seg_len + 2 * R) | 1;
    const size_t lds = TILE ? (size_t)(R + 1 + 2 * LINES - 1) * TW * 16 : 0;
    dim3 grid(wgs * (b.n * b.npairs)), block(256);
    with_dir(dir, [&](auto row, auto rev) {
        hipLaunchKernelGGL((k_pm_sweep<R, LPC, row(), rev(), TILE, false, PRE>), grid, block, lds, s, b, lut, seg_len, g.nseg, nseg_pad, TW);
    });
}
// the classic form: source tile in LDS while it stays small (EPPM_SWEEP_TILE); very long segments gather
template <int R, int LPC, bool PRE = false>
static void launch_sweep_r(const PmBatch& b, const float* lut, int seg_len, int dir, const SweepGeom& g, const SweepForm& f, hipStream_t s)
{
    if (PRE && f.pre && b.p[0].scand) {
        if (f.tile) launch_sweep_t<R, LPC, true, PRE>(b, lut, seg_len, dir, g, s);
        else launch_sweep_t<R, LPC, false, PRE>(b, lut, seg_len, dir, g, s);
        return;
    }
    if (f.tile) launch_sweep_t<R, LPC, true>(b, lut, seg_len, dir, g, s);
    else launch_sweep_t<R, LPC, false>(b, lut, seg_len, dir, g, s);
}

#ifdef EPPM_TOL
constexpr int kLpc9Small = EPPM_LPC9;          // one dealing of the samples (coop_chunk): small launches only fetch up front
#else
constexpr int kLpc9Small = 2 * EPPM_LPC9;
#endif
SweepForm pm_sweep_form(int w, int h, int R, int seg_len, int dir, int problems, int npairs)
{
    SweepForm f = {0, false, false, false};
    if (!(R == 9 || R == 17) || seg_len < 1) return f;
    f.lpc = EPPM_LPC17;
    if (R == 9) {
        // 16 lanes per chain, or twice as many for launches that cannot fill the chip (EPPM_LPC_SWITCH_WAVES)
        const SweepGeom g(w, h, dir, seg_len);
        const int chains = g.lines * g.nseg_pad() * problems * npairs;
        f.small = chains * 16 / 64 < EPPM_LPC_SWITCH_WAVES;
        f.lpc = f.small ? kLpc9Small : EPPM_LPC9;
        f.pre = (EPPM_SWEEP_PRE >= (f.small ? 1 : 2)) && seg_len <= kSpecMaxSteps;
    }
    const int cpb = 256 / f.lpc, segs = (cpb >= 16) ? 4 : 2, lines = cpb / segs;           // SweepTile<LPC>
    const size_t lds = (size_t)(R + 2 * lines) * ((segs * seg_len + 2 * R) | 1) * 16;
    f.tile = EPPM_SWEEP_TILE && lds <= 32 * 1024;
    return f;
}

bool launch_pm_sweep(PmBatch& b, const float* lut, int R, int seg_len, int dir, hipStream_t s, bool speculative)
{
    struct Count { PmBatch& b; ~Count() { b.sweep_seq++; } } count{b};      // every sweep of a run has its number (the work list's stamps)
    const SweepGeom g(b, dir, seg_len);
    if (speculative && b.p[0].spec && (R == 9 || R == 17) && seg_len <= kSpecMaxSteps) {
        if (R == 9) { launch_sweep_spec<9>(b, lut, R, dir, seg_len, g.nseg, s); launch_sweep_b<9, EPPM_LPC9_SPEC>(b, lut, seg_len, dir, g, s); }
        else { launch_sweep_spec<17>(b, lut, R, dir, seg_len, g.nseg, s); launch_sweep_b<17, EPPM_LPC17_SPEC>(b, lut, seg_len, dir, g, s); }
        launch_note(kLaunchSweep, b.p[0].P.w, b.p[0].P.h, b.npairs, -1, dir);
        return true;
    }
    const SweepForm f = pm_sweep_form(b.p[0].P.w, b.p[0].P.h, R, seg_len, dir, b.n, b.npairs);
    launch_note(kLaunchSweep, b.p[0].P.w, b.p[0].P.h, b.npairs, f.lpc * 4 + f.pre * 2 + f.tile, dir);      // (speculative: -1)
    if (R == 9) {
        if (f.small) launch_sweep_r<9, kLpc9Small, (EPPM_SWEEP_PRE >= 1)>(b, lut, seg_len, dir, g, f, s);
        else launch_sweep_r<9, EPPM_LPC9, (EPPM_SWEEP_PRE >= 2)>(b, lut, seg_len, dir, g, f, s);
        return true;
    }
    if (R == 17) { launch_sweep_r<17, EPPM_LPC17>(b, lut, seg_len, dir, g, f, s); return true; }
    if (g.nseg > 1024) return false;   // eppm_create / the launchers validate sizes
    const int lpb = g.nseg < 256 ? 256 / g.nseg : 1;
    const int threads = ((g.nseg * lpb + 63) / 64) * 64;
    dim3 grid((g.lines + lpb - 1) / lpb, b.n * b.npairs), block(threads);
    with_dir(dir, [&](auto row, auto rev) { hipLaunchKernelGGL((k_pm_seg_propagate<row(), rev()>), grid, block, 0, s, b, lut, R, seg_len, g.nseg, lpb); });
    return false;
}

bool launch_pm_sweeps_merged(PmBatch& b, const float* lut, int R, int seg_len, int iteration, hipStream_t s)
{
    for (int k = 0; k < b.n; k++)
        if (!b.p[k].seed || !b.p[k].wl || !b.p[k].spec || !b.p[k].scand) return false;
    if (!(R == 9 || R == 17) || seg_len > kSpecMaxSteps || seg_len < 1) return false;
    const int w = b.p[0].P.w, h = b.p[0].P.h, gx = (w + kBlock - 1) / kBlock, gy = (h + kBlock - 1) / kBlock;
    launch_note(kLaunchSweepsMerged, w, h, b.npairs, 1, iteration);
    b.merged_it = iteration;
    b.seg_len = seg_len;
    b.nseg_row = (w + seg_len - 1) / seg_len;
    b.nseg_col = (h + seg_len - 1) / seg_len;
    dim3 grid(gx * gy * (b.n * b.npairs)), block(256);
    if (R == 9 && pm_has_parity(b, R, EPPM_PARITY_SPEC)) hipLaunchKernelGGL((k_pm_spec_all<9, 2>), grid, block, 0, s, b, lut, R, gx);
    else if (pm_has_parity(b, R, EPPM_PARITY_SPEC)) hipLaunchKernelGGL((k_pm_spec_all<17, 2>), grid, block, 0, s, b, lut, R, gx);
    else if (R == 9) hipLaunchKernelGGL(k_pm_spec_all<9>, grid, block, 0, s, b, lut, R, gx);
    else hipLaunchKernelGGL(k_pm_spec_all<17>, grid, block, 0, s, b, lut, R, gx);
    for (int dir = 0; dir < 4; dir++) {
        if (R == 9) launch_sweep_b<9, EPPM_LPC9_SPEC, true>(b, lut, seg_len, dir, SweepGeom(b, dir, seg_len), s);
        else launch_sweep_b<17, EPPM_LPC17_SPEC, true>(b, lut, seg_len, dir, SweepGeom(b, dir, seg_len), s);
        b.sweep_seq++;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------
// Jump-flood propagation (d_jump_propagate, kernel.cu:800-841; launcher :843-857, disabled in the reference).
// Each pixel tries the matches of its neighbours at distance `step` (left, right, up, down), shifted by that
// distance, in order with strict <; candidates outside the image are skipped.  Jacobi: reads nnf, writes
// nnf_alt.  No serial chains: workgroup = 64 pixels x 4 candidates, wave k = candidate k, costs meet in
// LDS and wave 0 replays the in-order selection.  A candidate equal to the pixel's own match is rejected
// without evaluation (it would reproduce the stored cost).
//
// NEIGHBOR = true is d_neighbor_propagate (kernel.cu:720-787; ten launches per iteration at the disabled call
// site :1804-1809): distance 1, order upper, lower, left, right, the neighbour's match is copied UNSHIFTED
// and unchecked, and a neighbour outside the image is the clamped border pixel.
// ---------------------------------------------------------------------------------------------------
template <bool NEIGHBOR>
__global__ __launch_bounds__(256) void k_pm_jump(PmBatch B, const float* __restrict__ lut, int R, int step)
{
    __shared__ EPPM_LUT_ALIGN PatchLut L;
    __shared__ float s_cost[4][64];
    __shared__ int s_cand[4][64];
    const PmProblem pr = pm_problem(B, blockIdx.z);
    const int tid = threadIdx.x, lane = tid & 63, k = tid >> 6;
    load_patch_lut(L, lut, R, tid, 256);
    __syncthreads();
    const Planes P = to_dev(pr.P);
    const int x = blockIdx.x * kBlock + (lane & 15), y = blockIdx.y * 4 + (lane >> 4);
    const bool inimg = (x < P.w && y < P.h);
    const int nidx = y * B.npitch + x, cidx = y * B.cpitch + x;
    int bx = 0, by = 0;
    float cv = FLT_MAX;
    int cand = -1;
    if (inimg) {
        bx = pr.nnf[nidx * 2]; by = pr.nnf[nidx * 2 + 1];
        if (NEIGHBOR) {
            const int nx = iclamp(x + ((k == 2) ? -1 : (k == 3) ? 1 : 0), 0, P.w - 1);
            const int ny = iclamp(y + ((k == 0) ? -1 : (k == 1) ? 1 : 0), 0, P.h - 1);
            const int dx = pr.nnf[(ny * B.npitch + nx) * 2], dy = pr.nnf[(ny * B.npitch + nx) * 2 + 1];
            if (!(dx == bx && dy == by)) {
                cand = (dx & 0xffff) | (dy << 16);
                cv = patch_dist(P, L, R, x, y, dx, dy);
            }
        }
        const int nx = x + ((k == 0) ? -step : (k == 1) ? step : 0);
        const int ny = y + ((k == 2) ? -step : (k == 3) ? step : 0);
        if (!NEIGHBOR && nx >= 0 && nx < P.w && ny >= 0 && ny < P.h) {
            int dx = pr.nnf[(ny * B.npitch + nx) * 2], dy = pr.nnf[(ny * B.npitch + nx) * 2 + 1];
            if (k == 0) dx = (int)(int16_t)(dx - step);
            else if (k == 1) dx = (int)(int16_t)(dx + step);
            else if (k == 2) dy = (int)(int16_t)(dy - step);
            else dy = (int)(int16_t)(dy + step);
            if (!(dx < 0 || dy < 0 || dx >= P.w || dy >= P.h)) {
                cand = (dx & 0xffff) | (dy << 16);
                if (!(dx == bx && dy == by)) cv = patch_dist(P, L, R, x, y, dx, dy);
                else cand = -1;                                   // equals the current match: never accepted
            }
        }
    }
    s_cost[k][lane] = cv;
    s_cand[k][lane] = cand;
    __syncthreads();
    if (k == 0 && inimg) {
        float best_cost = pr.cost[cidx];
        for (int g = 0; g < 4; g++) {
            const int e = s_cand[g][lane];
            if (e == -1) continue;
            const float c = s_cost[g][lane];
            if (c < best_cost) { bx = (int)(int16_t)(e & 0xffff); by = e >> 16; best_cost = c; }
        }
        pr.nnf_alt[nidx * 2] = (int16_t)bx;
        pr.nnf_alt[nidx * 2 + 1] = (int16_t)by;
        pr.cost[cidx] = best_cost;
    }
}

void launch_pm_jump(const PmBatch& b, const float* lut, int R, int step, hipStream_t s)
{
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    dim3 grid((w + kBlock - 1) / kBlock, (h + 3) / 4, b.n * b.npairs), block(256);
    hipLaunchKernelGGL(k_pm_jump<false>, grid, block, 0, s, b, lut, R, step);
}

void launch_pm_neighbor(const PmBatch& b, const float* lut, int R, hipStream_t s)
{
    const int w = b.p[0].P.w, h = b.p[0].P.h;
    dim3 grid((w + kBlock - 1) / kBlock, (h + 3) / 4, b.n * b.npairs), block(256);
    hipLaunchKernelGGL(k_pm_jump<true>, grid, block, 0, s, b, lut, R, 1);
}

}  // namespace eppm
