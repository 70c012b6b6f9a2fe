"""Slots beyond 31: every word of the slot masks but the first.

TemporalArgs::armed and the cur / empty / cut / deflayer masks of the stage objects are uint32_t[kTemporalMaxSlots / 32], filled by
slot_mask() (stage_object.h) or by hand and read by the kernels as bits[slot >> 5] >> (slot & 31).  No other test has more than 8
slots, so word 0 is the only one they set or read, and k_plate_path (one lane per slot, 64 per block) never runs its second block.  Here
the temporal-prior kernels run on 70 and on 4096 slots with set and clear bits in every word, and the six per-clip objects run on a batch
of 70 pairs with cut flags, resets and empty slots that differ inside words 1 and 2: every checked slot equals the host forms fed with
that slot's own planes from the context, in every number."""
import functools

import numpy as np
import pytest

from test_bidirectional_gpu import eq, uv
from test_cutdet_cpu import differences as cutdet_differences
from test_objects_gpu import HostDetector
from test_plate_gpu import HostPlate
from test_stabilize_cpu import same_bits, same_model
from test_stabilize_gpu import host_walk
from test_temporal_cpu import UNKNOWN, make_clip, random_field

pytestmark = pytest.mark.gpu

WALK = (0, 31, 32, 33, 63, 64, 69)          # both sides of the boundaries between words 0 / 1 and 1 / 2, and the last slot


# ---- 1. the temporal-prior kernels ---------------------------------------------------------------------------------------------------------

def check_prior_batch(prevs, armed, backward):
    from eppm_amd import io, stages
    first, second = stages.temporal_prior_batch(prevs, backward, armed=armed, calls=2)
    host = {}
    for k in range(len(prevs)):
        if armed[k]:
            key = prevs[k].tobytes()
            if key not in host:
                host[key] = io.temporal_prior(prevs[k], backward)
            if not np.array_equal(first[k], host[key]):
                eq(first[k], host[key], f"slot {k} (armed) == eppm_temporal_prior_host")
        elif not ((first[k]["x"] == UNKNOWN).all() and (first[k]["y"] == UNKNOWN).all()):
            pytest.fail(f"slot {k} is not armed and has a prior")
    eq(second, first, "a second call on the same planes: the keys were restored")


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_prior_batch_70_slots_armed_pattern_over_three_words(backward):
    h, w, n = 37, 23, 70
    rng = np.random.default_rng(70 + int(backward))
    prevs = np.stack([random_field(rng, h, w, 5, 0.2) for _ in range(n)])
    armed = [k % 3 != 1 for k in range(n)]
    for k, flag in ((31, 1), (32, 0), (33, 1), (63, 0), (64, 1), (0, 0), (30, 0), (34, 0), (62, 1), (65, 0), (69, 1)):
        armed[k] = bool(flag)
    check_prior_batch(prevs, armed, backward)
    armed = [not a for a in armed]                   # 31, 32, 33, 63, 64 among both kinds
    for word in range(3):
        bits = armed[32 * word:32 * word + 32]
        assert any(bits) and not all(bits), word
    check_prior_batch(prevs, armed, backward)


def test_prior_batch_4096_slots_every_word_mixed():
    h, w, n = 12, 16, 4096
    rng = np.random.default_rng(4096)
    fields = np.stack([random_field(rng, h, w, 4, 0.15) for _ in range(64)])
    prevs = fields[rng.integers(0, 64, n)]           # 64 distinct fields: a slot that reads another slot's plane meets other data
    assert all(prevs[k].tobytes() != prevs[k + 1].tobytes() for k in (31, 63, 4094))
    armed = rng.random(n) < 0.5
    words = armed.reshape(128, 32)
    assert words.any(axis=1).all() and not words.all(axis=1).any(), "every one of the 128 words has a set and a clear bit"
    check_prior_batch(prevs, [bool(a) for a in armed], False)


# ---- 2. the six objects on a batch of 70 pairs -----------------------------------------------------------------------------------------------

H, W, N, NCLIPS = 61, 83, 70, 13
CUT = (31, 32, 64)           # the cut list of the first step
RESET = (33, 63)             # reset between the steps: empty slots beside stepped ones inside words 1 and 2


@functools.lru_cache(None)
def clip(s):
    return make_clip(H, W, 500 + s, n=3, max_flow=4.0)[0]


def slot_planes(b, k):
    u, v = uv(b.plane(k, "flow", 0))
    bu, bv = uv(b.plane(k, "flow_bwd", 0))
    return u, v, bu, bv, b.plane(k, "occ1", 0), b.plane(k, "occ2", 0)


class HostSlot:
    """the host forms of the six objects along one slot's clip"""

    def __init__(self):
        self.empty()

    def empty(self):
        self.acc = self.path = self.map = self.anchor = None
        self.det, self.plate = HostDetector(), HostPlate(H, W)

    def step(self, img1, img2, planes, cut):
        from eppm_amd import io
        u, v, bu, bv, o1, o2 = planes
        if self.acc is None:
            self.acc = io.tfilter_seed_host(img1)
        self.acc, self.rgb = io.tfilter_step_host(self.acc, img2, bu, bv, o2, cut=cut)
        self.stab = host_walk(img2, u, v, o1, self.path, cut=cut)
        self.path = (self.stab["C"], self.stab["S"])
        self.record = io.cutdet_host(img1, img2, bu, bv, o1, o2)
        if self.map is None:
            self.anchor = img1
        self.map = io.cmap_step_host(self.map, self.anchor, img2, bu, bv, o2, cut=cut)
        if cut:
            self.anchor = img2
        self.render = io.cmap_render_host(self.map, img2, None, self.anchor)
        self.objects = self.det.step(u, v, bu, bv, o1, o2, cut=cut)
        self.plate.step(img1, u, v, o1, cut=cut)

    def same(self, objs, k, what, ctx):
        flt, stab, det, cm, od, pl = objs
        assert same_bits(flt.state(k), self.acc) and np.array_equal(flt.frame(k), self.rgb), f"{what}: temporal filter"
        cc, ss = stab.path(k)
        assert same_model(stab.model(k), self.stab["model"]), f"{what}: stabiliser model"
        assert same_bits(cc, self.stab["C"]) and same_bits(ss, self.stab["S"]), f"{what}: stabiliser path"
        assert np.array_equal(stab.mask(k), self.stab["mask"]) and np.array_equal(stab.frame(k), self.stab["rgb"]), f"{what}: stabiliser planes"
        assert not cutdet_differences(self.record, det.stats(k)), f"{what}: cut detector"
        assert same_bits(cm.map(k), self.map) and np.array_equal(cm.render(k), self.render), f"{what}: correspondence map"
        self.det.same(od, k, self.objects, f"{what}: object detector")
        self.plate.same(pl, k, f"{what}: background plate", ctx)


def test_six_objects_on_a_batch_of_70_pairs():
    """a.n = 70, blockIdx.z up to 69, k_plate_path's second block; step 1 with cut flags on 31, 32 and 64 and every slot empty, then a
    reset of 33 and 63 and step 2 without flags: cut, empty and cur bits differ inside words 1 and 2"""
    import eppm_amd
    who = [k % NCLIPS for k in range(N)]
    b = eppm_amd.EPPMBatch(H, W, N)
    objs = (eppm_amd.TemporalFilter(b), eppm_amd.Stabilizer(b), eppm_amd.CutDetector(b), eppm_amd.CorrespondenceMap(b),
            eppm_amd.ObjectDetector(b), eppm_amd.BackgroundPlate(b))
    flt, stab, det, cm, od, pl = objs
    host = {k: HostSlot() for k in WALK}
    try:
        assert all(o.nslots == N for o in objs)
        for step in (1, 2):
            if step == 1:
                b.set_data([(clip(s)[0], clip(s)[1]) for s in who])
            else:
                b.push_frames([clip(s)[2] for s in who])
                for o in (flt, stab, cm, od, pl):
                    for k in RESET:
                        o.reset(k)
                for k in RESET:
                    host[k].empty()
            b.compute_flow_bidirectional_device()
            cut = [k in CUT for k in range(N)] if step == 1 else None
            for o in (flt, stab, cm, od, pl):
                o.step(cut, b)
            det.step(b)
            for k in WALK:
                f = clip(who[k])
                host[k].step(f[step - 1], f[step], slot_planes(b, k), bool(cut and cut[k]))
                host[k].same(objs, k, f"step {step}, slot {k}", b)
            assert det.cuts() == [bool(det.stats(k)["cut"]) for k in range(N)]
        # the cut at step 1 left slots 31, 32 and 64 one step behind their neighbours; the reset slots restarted
        assert [cm.age(k) for k in WALK] == [2, 1, 1, 1, 1, 1, 2]
        # thirteen clips cycled: a slot equals the slot 13 further on exactly when the flags of both agree
        assert same_bits(flt.state(0), flt.state(13)) and not same_bits(flt.state(31), flt.state(31 + 13))
    finally:
        for o in objs:
            o.close()
        b.close()


# ---- 3. the objects on caller planes: one slot per call, slot0 = the slot --------------------------------------------------------------------
# A step_frames call covers ONE slot, so its masks hold at most the slot's own bit -- in word slot >> 5.  Seven slots of a 70-slot object take
# the inputs of seven different cases of the feature's case table, all at one size and under one set of parameters (an object has one); then
# the same slots are stepped again on other inputs, 33 and 63 after a reset (their `empty` bit set, their neighbours' clear) and 32 and 64
# with cut = True.  The expectation is the feature's host form walked along the same two steps; the slots in between were never stepped.
# The sizes are the smallest of each case table with more than one row and column and at least seven usable cases.

UNTOUCHED = (1, 30, 34, 62, 65, 68)
CUT2, RESET2 = (32, 64), (33, 63)
SLOTS = 70


def never_stepped(call):
    import eppm_amd
    for k in UNTOUCHED:
        with pytest.raises(eppm_amd.EppmError):
            call(k)


def pool_of(cases, w, h, need):
    pool = [c for c in cases if (c["w"], c["h"]) == (w, h)]
    assert len(pool) >= need, (len(pool), need)
    return pool


def walk_two_steps(pool, step):
    """step(slot, case, cut, reset_first) for the seven slots, twice: the second time on the inputs of the case three further on"""
    for i, k in enumerate(WALK):
        step(k, pool[i], False, False)
    for i, k in enumerate(WALK):
        step(k, pool[(i + 3) % len(pool)], k in CUT2, k in RESET2)


def test_temporal_filter_and_correspondence_map_slots_on_caller_planes():
    import eppm_amd
    from eppm_amd import io
    from eppm_amd._lib import lib
    from test_tfilter_cpu import tfilter_cases
    from tfilter_tol_child import rgba, to_device
    w, h = 64, 4
    pool = pool_of(tfilter_cases(), w, h, 7)          # (the map reads the same planes: two frames, the backward flow, occ2)
    dev = {id(c): [to_device(rgba(c["img1"])), to_device(rgba(c["img2"])), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
                   to_device(c["occ"])] for c in pool}
    flt = eppm_amd.TemporalFilter(None, 40.0, 8, size=(h, w), slots=SLOTS)
    cm = eppm_amd.CorrespondenceMap(None, size=(h, w), slots=SLOTS)
    acc, M, anchor = {}, {}, {}

    def step(k, c, cut, reset):
        p = [x.value for x in dev[id(c)]]
        if reset:
            flt.reset(k); cm.reset(k)
            acc.pop(k, None); M.pop(k, None)
        flt.step_frames(k, p[0], p[1], w * 4, p[2], p[3], cut)
        cm.step_frames(k, p[0], p[1], w * 4, p[2], p[3], cut)
        a0 = acc[k] if k in acc else io.tfilter_seed_host(c["img1"])
        acc[k], rgb = io.tfilter_step_host(a0, c["img2"], c["bu"], c["bv"], c["occ"], cut=cut)
        assert same_bits(flt.state(k), acc[k]) and np.array_equal(flt.frame(k), rgb), f"filter slot {k}"
        if k not in M:
            anchor[k] = c["img1"]
        M[k] = io.cmap_step_host(M.get(k), anchor[k], c["img2"], c["bu"], c["bv"], c["occ"], cut=cut)
        if cut:
            anchor[k] = c["img2"]
        assert same_bits(cm.map(k), M[k]), f"map slot {k}"
    try:
        walk_two_steps(pool, step)
        for k in WALK:                                 # every slot still holds its own after all the others were stepped
            assert same_bits(flt.state(k), acc[k]) and same_bits(cm.map(k), M[k]), k
        assert [cm.age(k) for k in WALK] == [2, 2, 0, 1, 1, 0, 2]
        never_stepped(flt.state); never_stepped(cm.map)
    finally:
        flt.close(); cm.close()
        for planes in dev.values():
            for p in planes:
                lib().eppm_free_device(p)


def test_stabilizer_slots_on_caller_planes():
    import eppm_amd
    from eppm_amd._lib import lib
    from stabilize_tol_child import rgba, to_device
    from eppm_amd import io
    from test_stabilize_cpu import stab_cases
    w, h = 64, 4
    pool = pool_of(stab_cases(), w, h, 7)
    dev = {id(c): [to_device(rgba(c["img2"])), to_device(np.stack([c["u"], c["v"]], -1).astype(np.float32)), to_device(c["occ"])] for c in pool}
    stab = eppm_amd.Stabilizer(None, 1.0, 3, 0.9, size=(h, w), slots=SLOTS)
    path = {}

    def step(k, c, cut, reset):
        p = [x.value for x in dev[id(c)]]
        if reset:
            stab.reset(k)
            path.pop(k, None)
        stab.step_frames(k, p[0], w * 4, p[1], p[2], cut)
        C0, S0, n0 = path.get(k) or (io.stab_identity() + ((0, 0),))           # (the frame and invalid-step counts go along with the paths)
        model, mask = io.gmotion_fit_host(c["u"], c["v"], c["occ"], 1.0, 3)
        Cn, Sn, wf, counts_want = io.stab_update_host(C0, S0, model, 0.9, cut, n0)
        want = dict(model=model, mask=mask, C=Cn, S=Sn, counts=counts_want, rgb=io.stab_warp_host(wf, c["img2"]))
        path[k] = (Cn, Sn, counts_want)
        cc, ss, counts = stab.path(k, counts=True)
        assert same_model(stab.model(k), want["model"]) and same_bits(cc, want["C"]) and same_bits(ss, want["S"]), f"stabiliser slot {k}: model, path"
        assert tuple(counts) == tuple(want["counts"]), f"stabiliser slot {k}: counts {counts} {want['counts']}"
        assert np.array_equal(stab.mask(k), want["mask"]) and np.array_equal(stab.frame(k), want["rgb"]), f"stabiliser slot {k}: planes"
    try:
        walk_two_steps(pool, step)
        for k in WALK:
            cc, ss = stab.path(k)
            assert same_bits(cc, path[k][0]) and same_bits(ss, path[k][1]), k
        never_stepped(stab.model)
    finally:
        stab.close()
        for planes in dev.values():
            for p in planes:
                lib().eppm_free_device(p)


def test_cut_detector_slots_on_caller_planes():
    """no mask: the seven-slot walk for its slot0 arithmetic alone; the verdicts of all 70 slots in one copy"""
    import eppm_amd
    from eppm_amd import io
    from eppm_amd._lib import lib
    from cutdet_tol_child import rgba, to_device
    from test_cutdet_cpu import cutdet_cases
    w, h = 64, 4
    pool = pool_of(cutdet_cases(), w, h, 7)
    det = eppm_amd.CutDetector(None, size=(h, w), slots=SLOTS)
    want = {}
    try:
        for rnd in (0, 3):
            for i, k in enumerate(WALK):
                c = pool[(i + rnd) % len(pool)]
                planes = [to_device(rgba(c["img1"], 0)), to_device(rgba(c["img2"], 0)), to_device(np.stack([c["bu"], c["bv"]], -1).astype(np.float32)),
                          to_device(c["occ1"]), to_device(c["occ2"])]
                det.step_frames(k, planes[0].value, planes[1].value, w * 4, *[p.value for p in planes[2:]])
                want[k] = io.cutdet_host(c["img1"], c["img2"], c["bu"], c["bv"], c["occ1"], c["occ2"])
                assert not cutdet_differences(want[k], det.stats(k)), f"detector slot {k}"
                for p in planes:
                    lib().eppm_free_device(p)
        for k in WALK:
            assert not cutdet_differences(want[k], det.stats(k)), k
        assert det.cuts(SLOTS) == [k in want and bool(want[k]["cut"]) for k in range(SLOTS)]
        never_stepped(det.stats)
    finally:
        det.close()


def test_object_detector_slots_on_caller_planes():
    import eppm_amd
    from objects_tol_child import case_planes, free_planes, load_case, read_slot, step_case
    from test_objects_cpu import differences, finish_case, objects_cases
    w, h = 65, 17
    common = dict(conn=8, min_area=4, max_objects=64, min_overlap=4)
    KINDS = ("rand45", "spiral", "comb", "bytes", "identity", "ushapes", "stripes_dashed", "blocks", "checker", "diag")
    picked = []
    for c in objects_cases():
        if (c["w"], c["h"]) == (w, h) and c["kind"] in KINDS and c["kind"] not in [p["kind"] for p in picked]:
            picked.append(finish_case(dict(c, **common)))
    cuts = [c for c in picked if c["cut"]]
    empties = [c for c in picked if c["prev"] == "empty" and not c["cut"]]
    rest = [c for c in picked if not c["cut"] and c["prev"] != "empty"]
    assert len(picked) >= 7 and cuts and empties and len(rest) >= 3, (len(picked), len(cuts), len(empties), len(rest))
    det = eppm_amd.ObjectDetector(None, size=(h, w), slots=SLOTS, connectivity=8, min_area=4, max_objects=64, min_overlap=4)
    planes = {id(c): case_planes(c) for c in picked}
    try:
        held = {}
        for i, k in enumerate(WALK):
            held[k] = picked[i]
        for k, c in held.items():
            load_case(det, k, c)
        for k, c in held.items():
            step_case(det, k, c, planes[id(c)])
        for k, c in held.items():
            assert not differences(c, *read_slot(det, k)), (k, c["name"])
        for i, k in enumerate(WALK):                   # 32, 64: a case stepped with cut; 33, 63: one that starts from a reset slot
            c = cuts[i % len(cuts)] if k in CUT2 else empties[i % len(empties)] if k in RESET2 else rest[i % len(rest)]
            held[k] = c
            load_case(det, k, c)
            step_case(det, k, c, planes[id(c)])
        for k, c in held.items():
            assert not differences(c, *read_slot(det, k)), (k, c["name"])
        never_stepped(det.labels)
    finally:
        det.close()
        for p in planes.values():
            free_planes(p)


def test_background_plate_slots_on_caller_planes():
    import eppm_amd
    from plate_tol_child import case_params, case_planes, device_case, device_differences, free_planes
    from eppm_amd import io
    from test_plate_cpu import F, IDENT, expected, np_coverage, np_word, plate_cases
    w, h = 65, 17
    common = dict(mx=3, my=2, grow=1, accept=False, thresh=40.0, n_max=64, min_count=2)
    picked = []
    for c in plate_cases():
        if (c["w"], c["h"], c["mx"], c["my"]) == (w, h, 3, 2) and c["pname"] in ("identity", "int", "sub", "sub2", "rotzoom"):
            d = {k: v for k, v in c.items() if k != "want"}
            d.update(common, name=c["name"] + "_common")
            picked.append(d)
    assert len(picked) >= 10
    pl = eppm_amd.BackgroundPlate(None, size=(h, w), slots=SLOTS, **case_params(picked[0]))
    planes = {id(c): case_planes(c) for c in picked}
    try:
        res = {k: device_case(picked[i], pl, k, planes[id(picked[i])]) for i, k in enumerate(WALK)}
        for i, k in enumerate(WALK):
            assert not device_differences(picked[i], res[k]), (k, picked[i]["name"])
        # the same seven slots stepped again on another case's frame and mask with the slot's OWN path (path = NULL), 33 and 63 after a
        # reset (identity path, empty canvas), 32 and 64 with cut = True: the host forms from the slot's state -- the canvas accumulates
        # under the path the slot had; a cut then makes the path the identity and keeps the canvas
        m = (common["mx"], common["my"])
        for i, k in enumerate(WALK):
            first, c = picked[i], picked[(i + 3) % len(picked)]
            if k in RESET2:
                pl.reset(k)
                st, path = np.zeros((h + 2 * m[1], w + 2 * m[0], 4), F), np.array(IDENT, np.float64)
            else:
                st, path = expected(first)["states"][1], np.asarray(first["path"], np.float64)
            cut = k in CUT2
            pl.step_frames(k, planes[id(c)][0].value, w * 4, planes[id(c)][2].value, None, cut)
            fwd, inv, ok = io.plate_forms_host(path)
            blocked = io.plate_block_host(c["mask"], common["grow"], common["accept"])
            want = io.plate_accumulate_host(st, fwd, c["img"], blocked, margins=m, thresh=common["thresh"], n_max=common["n_max"]) if ok else st
            after = np.array(IDENT, np.float64) if cut else path
            assert same_bits(pl.state(k), np.asarray(want, F)), f"slot {k}: canvas after the second step (cut {cut}, reset {k in RESET2})"
            assert same_bits(np.asarray(pl.path(k), np.float64), after), f"slot {k}: path after the second step (cut {cut})"
            assert same_bits(pl.plate(k), np_word(np.asarray(want, F)[..., :3])) and same_bits(pl.coverage(k), np_coverage(np.asarray(want, F))), k
        assert [bool((np.asarray(pl.path(k)) == np.array(IDENT)).all()) for k in (32, 64)] == [True, True]
        assert any(not (np.asarray(picked[i]["path"]) == np.array(IDENT)).all() for i, k in enumerate(WALK) if k in CUT2), "a cut slot had another path"
        never_stepped(pl.state)
    finally:
        pl.close()
        for p in planes.values():
            free_planes(p)
