"""GPU half of tests/test_batch_forms_cpu.py: batches of 83x61 pairs at every size n at which a launcher changes its kernel, each slot
against the CPU oracle, bit for bit.

One context of 512 pairs per patch radius serves every n (kernels cover only the active pairs of set_data).  Slot k of a batch of n holds
clip perm_n[k] % 13 of thirteen distinct clips, perm_n a seeded permutation: a kernel that reads a neighbouring slot's planes, or the slot
8 or 64 further on, meets other data.  Every case asserts through the launch log (include/eppm_test.h) that its launches TOOK the forms
the probe answers for its (level, n) -- the "reached" half of the ledger -- and, on a mismatch, names the first stage plane of the first
failing slot that differs from the oracle's dump, so that the failing kernel is named."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_batch_forms_cpu as T
from conftest import ROOT
from test_bidirectional_gpu import eq, oracle_backward, uv
from test_draft_cpu import oracle_jbu
from test_temporal_cpu import UNKNOWN, displacement, make_clip
from test_temporal_gpu import free_bytes, oracle_forward_from, oracle_planes, oracle_seeded_patchmatch

pytestmark = pytest.mark.gpu

H, W = T.H, T.W
NCLIPS = 13
FLOW_NAMES = ("u", "v", "bu", "bv", "occ1", "occ2")


@functools.lru_cache(None)
def clip(s):
    return make_clip(H, W, 500 + s, n=3, max_flow=4.0)[0]


def slots(n, nclips=NCLIPS):
    """the clip in every slot of a batch of n"""
    return [int(p) % nclips for p in np.random.default_rng(7000 + n).permutation(n)]


@functools.lru_cache(None)
def reference(R, s, a=0):
    """The oracle on frames (a, a + 1) of clip s, once: the flows, the dump, the level-2 planes a context shows after a forward call, and
    the backward chain with both occlusion masks.  Nothing may write into what this returns."""
    from eppm_amd import io
    from oracle import oracle as O
    prm = O.default_params(patch_r=R)
    f = clip(s)
    u, v, st = O.compute_flow(f[a], f[a + 1], prm, dump=True)
    n1, c1, n2, c2 = O.left_right_check(st["nnf1_pm"], st["cost1_pm"], st["nnf2_pm"], st["cost2_pm"])
    n2_fill, blev = oracle_backward(st, prm)
    bu, bv = uv(blev[0])
    return dict(u=u, v=v, st=st, lr=dict(nnf2=n2, cost2=c2, cost1=c1), n2_fill=n2_fill, blev=blev, bu=bu, bv=bv,
                occ1=io.fb_occlusion(u, v, bu, bv), occ2=io.fb_occlusion(bu, bv, u, v))


@pytest.fixture(scope="module")
def refs():
    """{R: [reference of clip s]}; filled per radius on first use, shared by every test of the module"""
    cache = {}

    def get(R):
        if R not in cache:
            cache[R] = [reference(R, s) for s in range(NCLIPS)]
            flows = [r["u"].tobytes() + r["v"].tobytes() for r in cache[R]]
            assert len(set(flows)) == NCLIPS and all(np.abs(r["u"]).max() > 0 for r in cache[R]), "thirteen distinct, non-zero oracle flows"
        return cache[R]
    return get


@pytest.fixture(scope="module")
def contexts():
    """{R: EPPMBatch(61, 83, 512)}, made on first use; the device bytes each holds are printed (and those of its first bidirectional call)"""
    import eppm_amd
    made = {}

    def get(R):
        if R not in made:
            eppm_amd.lib().eppm_release_cached_memory()
            before = free_bytes()
            b = eppm_amd.EPPMBatch(H, W, T.CAPACITY, params=eppm_amd.Params(patch_r=R))
            held = before - free_bytes()
            print(f"EPPMBatch({H}, {W}, {T.CAPACITY}) R = {R}: {held} device bytes, {held / T.CAPACITY / 2 ** 20:.3f} MiB per pair")
            assert held < (2 << 30), "above 2 GiB the largest case gets a context of its own"
            dims = [(w, h) for h, w in _level_dims(b)]
            assert tuple(dims) == T.level_dims(), "eppm_level_dims == the probe's pyramid"
            made[R] = (b, before)
        return made[R][0]
    yield get
    for R, (b, before) in made.items():
        eppm_amd.lib().eppm_release_cached_memory()
        f0 = free_bytes()
        b.close()
        eppm_amd.lib().eppm_release_cached_memory()
        print(f"R = {R}: {free_bytes() - f0} device bytes with the planes of the bidirectional calls")


def _level_dims(b):
    import eppm_amd
    out = []
    for l in range(eppm_amd.lib().eppm_num_levels(b._ctx)):
        h, w = C.c_int(), C.c_int()
        eppm_amd._lib.check(eppm_amd.lib().eppm_level_dims(b._ctx, l, C.byref(h), C.byref(w)), "eppm_level_dims")
        out.append((h.value, w.value))
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(b, k, r, bidirectional):
    """the first stage plane of slot k, in pipeline order, that differs from the oracle's"""
    L = len(T.level_dims()) - 1
    st = r["st"]
    order = []
    if bidirectional:                   # (the backward branch has rewritten nnf2 / cost2)
        order += [("nnf1", L, st["nnf1_fill"]), ("nnf2", L, r["n2_fill"])]
    else:
        order += [("nnf2", L, r["lr"]["nnf2"]), ("cost2", L, r["lr"]["cost2"]), ("cost1", L, r["lr"]["cost1"]), ("nnf1", L, st["nnf1_fill"])]
    for l in range(L, -1, -1):
        order.append(("flow", l, st[f"flow_L{l}"]))
        if bidirectional:
            order.append(("flow_bwd", l, r["blev"][l]))
    for name, l, want in order:
        got = b.plane(k, name, l)
        if not same(got, want):
            bad = int((got.view(np.uint8).reshape(got.shape + (-1,)) != np.ascontiguousarray(want).view(np.uint8).reshape(got.shape + (-1,))).any(axis=-1).sum())
            return f"first differing plane: {name} at level {l} ({bad} of {got.size} elements)"
    return "every stage plane equals the oracle's: the difference is in the output copy"


def check_slots(b, res, who, ref, R, n, bidirectional):
    want_names = FLOW_NAMES if bidirectional else FLOW_NAMES[:2]
    for k in range(n):
        r = ref[who[k]]
        if not all(same(res[k][j], r[name]) for j, name in enumerate(want_names)):
            what = [name for j, name in enumerate(want_names) if not same(res[k][j], r[name])]
            pytest.fail(f"R = {R}, n = {n}: slot {k} (clip {who[k]}) differs from the oracle in {what}; {first_difference(b, k, r, bidirectional)}")
    for j, name in enumerate(want_names):             # (and once through the helper every other parity test uses)
        eq(res[n - 1][j], ref[who[n - 1]][name], f"slot {n - 1} {name}")


def run_case(b, ref, R, n, bidirectional, who=None):
    from eppm_amd._lib import launch_log
    who = who or slots(n)
    b.set_data([(clip(s)[0], clip(s)[1]) for s in who])
    with launch_log() as log:
        res = b.compute_flow_bidirectional() if bidirectional else b.compute_flow()
    T.check_reached(log.entries(), R, n)
    check_slots(b, res, who, ref, R, n, bidirectional)


CASES = [(R, n) for R in T.RADII for n in T.batch_sizes(R)]
CHANGES = [(R, n) for R in T.RADII for n in T.change_sizes(R)]


@pytest.mark.parametrize("R,n", CASES, ids=[T.case_id(R, n) for R, n in CASES])
def test_forward_every_slot_equals_the_oracle(R, n, refs, contexts):
    run_case(contexts(R), refs(R), R, n, False)


@pytest.mark.parametrize("R,n", CHANGES, ids=[T.case_id(R, n) for R, n in CHANGES])
def test_bidirectional_every_slot_equals_the_oracle(R, n, refs, contexts):
    run_case(contexts(R), refs(R), R, n, True)


def test_slot_assignment_meets_other_data_at_the_strides_a_kernel_could_confuse():
    """the premise of every case above: in every batch the slots 1, 8 and 64 further on hold, somewhere, another clip"""
    for R, n in CASES:
        who = slots(n)
        assert len(set(who)) == min(n, NCLIPS)
        for d in (1, 8, 64):
            if n > d:
                assert any(who[k] != who[k + d] for k in range(n - d)), (n, d)


def test_draft_two_pixels_per_lane_upsampling(refs, contexts):
    """stop level 1 at the smallest n whose level-0 launch takes two pixels per lane: k_flow_jbu<2> on 83x61 with the pair index up to
    n - 1; level 1 is the full path's, level 0 the oracle's smoothing of the doubled, replicated level-1 flow (test_draft_gpu.py)"""
    from eppm_amd._lib import launch_log
    R = 9
    n = min(m for m in T.batch_sizes(R) if T.forms(R, m)["smoothing_L0"] == 2)
    assert T.forms(R, n - 1)["smoothing_L0"] == 1
    b, ref, who = contexts(R), refs(R), slots(n)
    want = [oracle_jbu(r["st"]["flow_L1"], r["st"]["img1_L0"]) for r in ref]
    b.set_stop_level(1)
    try:
        b.set_data([(clip(s)[0], clip(s)[1]) for s in who])
        with launch_log() as log:
            res = b.compute_flow()
        T.check_reached(log.entries(), R, n, draft=True)
        for k in range(n):
            wu, wv = uv(want[who[k]])
            if not (same(res[k][0], wu) and same(res[k][1], wv)):
                eq(b.plane(k, "flow", 1), ref[who[k]]["st"]["flow_L1"], f"slot {k}: flow level 1 == the full path's")
                eq(b.plane(k, "flow", 0), want[who[k]], f"slot {k}: flow level 0 == oracle composition")
                eq(res[k][0], wu, f"slot {k}: u"); eq(res[k][1], wv, f"slot {k}: v")
        eq(b.plane(n - 1, "flow", 0), want[who[n - 1]], f"slot {n - 1}: flow level 0 == oracle composition")
    finally:
        b.set_stop_level(0)


# ---- seeded start ------------------------------------------------------------------------------------------------------------------------

SEEDED_CLIPS = 5
ALL_FLAGGED = (31, 32, 33, 64)


@pytest.fixture(scope="module")
def seeded_refs(refs):
    """per clip 0..4: the oracle's seeded chain of pair (1, 2) from its own pair (0, 1), and the cold oracle run of pair (1, 2)"""
    from eppm_amd import io
    from oracle import oracle as O
    prm = O.default_params(patch_r=9)
    out = []
    for s in range(SEEDED_CLIPS):
        st0 = refs(9)[s]["st"]
        prior1 = io.temporal_prior(displacement(st0["nnf1_fill"]), False)
        prior2 = io.temporal_prior(displacement(st0["nnf2_pm"]), True)
        known = float((prior1["x"] > UNKNOWN).mean())
        assert known > 0.9, (s, known)
        f = clip(s)
        st = oracle_planes(f[1], f[2], prm.levels)
        (n1, c1, init1, _), (n2, c2, init2, _) = oracle_seeded_patchmatch(st, prior1, prior2, prm)
        _, levels = oracle_forward_from(n1, c1, n2, c2, st, prm)
        out.append(dict(prior1=prior1, nnf_init1=init1[0], cost_init1=init1[1], levels=levels, uv=uv(levels[0]), cold=reference(9, s, 1)))
    return out


def seeded_sizes():
    cps = T.change_points(9)
    L = len(T.level_dims()) - 1
    return [cps[f"search_rows_L{L}"][0], cps[f"speculative_L{L}"][0]]


@pytest.mark.parametrize("which", [0, 1], ids=["search_change_point", "speculative_change_point"])
def test_seeded_start_per_slot(which, refs, seeded_refs):
    """set_data of frames 0 / 1, compute, push of frame 2 with new_clip set for slots 31, 32, 33 and 64 (those the batch has: the search
    changes form at a size that ends one slot short of 64), compute: every other slot equals the oracle's seeded chain in prior1, nnf_init1,
    cost_init1 and the flow, the flagged ones its cold run of frames 1 / 2"""
    import eppm_amd
    from eppm_amd._lib import launch_log
    n = seeded_sizes()[which]
    FLAGGED = tuple(k for k in ALL_FLAGGED if k < n)
    assert len(FLAGGED) >= 3 and (which == 0 or FLAGGED == ALL_FLAGGED)
    L = len(T.level_dims()) - 1
    who = [k % SEEDED_CLIPS for k in range(n)]
    b = eppm_amd.EPPMBatch(H, W, n)
    try:
        b.set_temporal(True)
        b.set_data([(clip(s)[0], clip(s)[1]) for s in who])
        res = b.compute_flow()
        for k in (0, 31, 32, n - 1):
            eq(res[k][0], refs(9)[who[k]]["u"], f"first pair, slot {k}: u"); eq(res[k][1], refs(9)[who[k]]["v"], f"first pair, slot {k}: v")
        b.push_frames([clip(s)[2] for s in who], new_clip=[k in FLAGGED for k in range(n)])
        assert [k for k in range(n) if not b.temporal_valid(k)] == list(FLAGGED)
        with launch_log() as log:
            res = b.compute_flow()
        T.check_reached(log.entries(), 9, n)
        for k in range(n):
            r = seeded_refs[who[k]]
            if k in FLAGGED:
                with pytest.raises(eppm_amd.EppmError):
                    b.plane(k, "prior1", L)
                want = (r["cold"]["u"], r["cold"]["v"])
            else:
                want = r["uv"]
            if k not in FLAGGED:
                for p in ("prior1", "nnf_init1", "cost_init1"):
                    if not same(b.plane(k, p, L), r[p]):
                        eq(b.plane(k, p, L), r[p], f"slot {k}: {p}")
            if same(res[k][0], want[0]) and same(res[k][1], want[1]):
                continue
            if k not in FLAGGED:
                for l in range(L, -1, -1):
                    eq(b.plane(k, "flow", l), r["levels"][l], f"slot {k}: flow level {l}")
            eq(res[k][0], want[0], f"slot {k} ({'cold' if k in FLAGGED else 'seeded'}): u")
            eq(res[k][1], want[1], f"slot {k} ({'cold' if k in FLAGGED else 'seeded'}): v")
    finally:
        b.close()


# ---- the tolerance library -----------------------------------------------------------------------------------------------------------------

def test_tolerance_library_batch_equals_its_single_pair_contexts():
    """DESIGN.md section 9.2 at the change-point sizes: in a child process that loads the tolerance library, every slot equals that library's
    own single-pair context on the same pair, bit for bit"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "batch_forms_tol_child.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert lines and "tolerance arithmetic" in lines[0] and lines[-1] == "PART OK", p.stdout[-2000:]
