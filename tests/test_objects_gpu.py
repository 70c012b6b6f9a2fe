"""GPU tests of moving-object detection: the kernels against the numpy restatement (which
tests/test_objects_cpu.py holds equal to the host forms) in every number on objects_cases() and objects_large_cases() (more than 64
chunks, thin frames 8192 long), slot independence, the context and batch
forms against the host forms fed with the context's own planes, the tolerance library, and the end-to-end helpers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_objects_cpu import FIELDS, LARGE_IDS, LARGE_SIZES, SIZES, differences, finish_case, host_case, objects_cases, objects_large_cases
from test_stabilize_cpu import moving_clip
from objects_tol_child import case_planes, free_planes, load_case, mismatches, read_slot, step_case

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


def plain(recs):
    return [{k: r[k] for k in FIELDS + ("id", "age")} for r in recs]


# ---- the kernels equal the host forms ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_host_forms(size):
    """every case through set_state (or reset) + eppm_objects_step_frames + get + get_labels + get_state, twice in a row on one detector:
    labels, records, counts and state are the restatement's.  Every read of a slot fails if its error word is set, so the word is clear
    after every case."""
    cases = [c for c in objects_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad[:3]
    c = cases[len(cases) // 2]                    # and against the host forms directly
    assert not differences(c, *host_case(c))


@pytest.mark.parametrize("size", range(len(LARGE_SIZES)), ids=LARGE_IDS)
def test_kernels_equal_the_host_forms_on_large_frames(size):
    """objects_large_cases(): more than 64 chunks (k_obj_scan's carry from round to round, k_obj_number's start value of a chunk >= 64),
    up to 128 x 2 and 1 x 512 tiles under one component, coordinates up to 8191.  Stepped twice on one detector, read with the error word
    checked, as above."""
    cases = objects_large_cases(size)
    bad = mismatches(cases)
    assert not bad, bad[:3]
    c = cases[len(cases) // 2]
    assert not differences(c, *host_case(c))


@pytest.mark.parametrize("size", range(len(LARGE_SIZES)), ids=LARGE_IDS)
def test_tolerance_library_runs_the_same_kernels_on_large_frames(size):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "objects_tol_child.py"), "large", str(size)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_eight_slots_hold_eight_large_cases():
    """eight slots of one 8192 x 20 detector take eight different large cases, so that every slot's chunk counts, parent plane and tables
    meet other data than its neighbours'; all are stepped before any is read, then stepped again in another order"""
    import eppm_amd
    w, h = 8192, 20
    common = dict(conn=8, min_area=6, max_objects=64, min_overlap=4)
    pool = objects_large_cases(LARGE_SIZES.index((w, h)))
    picked = [finish_case(dict(c, **common)) for c in pool if c["conn"] == 8 or c["kind"] in ("late", "cap", "spread")][:8]
    assert len(picked) == 8 and len({c["want_counts"]["n_found"] for c in picked}) >= 4
    assert any(c["want_counts"]["n_found"] > 64 for c in picked)
    det = eppm_amd.ObjectDetector(None, size=(h, w), slots=8, **{"connectivity" if k == "conn" else k: v for k, v in common.items()})
    planes = [case_planes(c) for c in picked]
    try:
        for order in (range(8), (5, 2, 7, 0, 3, 6, 1, 4)):
            for slot in order:
                load_case(det, slot, picked[slot])
            for slot in order:
                step_case(det, slot, picked[slot], planes[slot])
            for slot in range(8):
                assert not differences(picked[slot], *read_slot(det, slot)), (slot, picked[slot]["name"])
    finally:
        det.close()
        for p in planes:
            free_planes(p)


def test_slots_are_independent():
    """eight slots of one detector hold eight different cases; a slot keeps what it has while the others are stepped, loaded and reset"""
    import eppm_amd
    w, h = 65, 17
    common = dict(conn=8, min_area=4, max_objects=64, min_overlap=4)
    pool = [c for c in objects_cases() if (c["w"], c["h"]) == (w, h) and c["kind"] in ("rand45", "spiral", "comb", "bytes", "identity", "ushapes",
                                                                                         "stripes_dashed", "blocks", "checker", "diag")]
    picked = []
    for c in pool:
        if c["kind"] not in [p["kind"] for p in picked]:
            picked.append(finish_case(dict(c, **common)))
    assert len(picked) >= 8
    first, second = picked[:8], picked[2:10] if len(picked) >= 10 else picked[::-1][:8]
    det = eppm_amd.ObjectDetector(None, size=(h, w), slots=8, connectivity=8, min_area=4, max_objects=64, min_overlap=4)
    planes = {id(c): case_planes(c) for c in picked}
    try:
        for slot, c in enumerate(first):
            load_case(det, slot, c)
        for slot, c in enumerate(first):
            step_case(det, slot, c, planes[id(c)])
        for slot, c in enumerate(first):
            assert not differences(c, *read_slot(det, slot)), (slot, c["name"])
        for slot in (1, 3, 6):                     # three slots take other cases, one is reset: the rest keep theirs
            load_case(det, slot, second[slot])
            step_case(det, slot, second[slot], planes[id(second[slot])])
        det.reset(4)
        assert status(lambda: det.labels(4)) == STATE
        for slot, c in enumerate(first):
            if slot != 4:
                want = second[slot] if slot in (1, 3, 6) else c
                assert not differences(want, *read_slot(det, slot)), (slot, want["name"])
        assert det.state(4)[3] == 1 and not det.state(4)[0].any()
    finally:
        det.close()
        for p in planes.values():
            free_planes(p)


def test_tolerance_library_runs_the_same_kernels():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "objects_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- the context form ----

class HostDetector:
    """the host forms along a clip, fed with a context's planes: what a slot of an ObjectDetector must hold"""

    def __init__(self, **params):
        from eppm_amd import io
        self.p = dict(connectivity=8, min_area=16, max_objects=64, min_overlap=4)
        self.p.update(params)
        self.carried = None
        self.pid, self.page, self.nxt = io.objects_state()

    def step(self, u, v, bu, bv, o1, o2, cut=False):
        from eppm_amd import io
        _, mask = io.gmotion_fit_host(u, v, o1)
        p = self.p
        labels, recs, counts = io.objects_label_host(mask, u, v, p["connectivity"], p["min_area"], p["max_objects"])
        ids, ages, self.pid, self.page, self.nxt = io.objects_assign_host(labels, counts["n"], self.carried, self.pid, self.page, self.nxt,
                                                                          p["max_objects"], p["min_overlap"])
        for r, i, a in zip(recs, ids, ages):
            r["id"], r["age"] = i, a
        self.carried = np.zeros_like(labels) if cut else io.objects_carry_host(labels, bu, bv, o2)
        return labels, recs, dict(counts, next_id=self.nxt)

    def same(self, det, slot, want, what):
        labels, recs, counts = want
        assert np.array_equal(det.labels(slot), labels), f"{what}: labels"
        assert plain(det.objects(slot)) == plain(recs), f"{what}: records"
        assert det.counts(slot) == counts, f"{what}: counts"
        car, pid, page, nxt = det.state(slot)
        assert np.array_equal(car, self.carried) and np.array_equal(pid, self.pid) and np.array_equal(page, self.page) and nxt == self.nxt, f"{what}: state"


def test_context_form_equals_the_host_forms_and_leaves_the_flows_alone():
    import eppm_amd
    h, w = 192, 256
    noisy = moving_clip(h, w, 3)
    e, ref = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); ref.init(h, w)
    det = eppm_amd.ObjectDetector(e)
    host = HostDetector()
    e.enable_stage_timing(True)
    ids = []
    try:
        assert status(lambda: det.objects(0)) == STATE and status(lambda: det.labels(0)) == STATE          # never stepped
        assert status(det.step) == STATE                       # before any bidirectional call
        for k in (1, 2):
            for ctx in (e, ref):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[2])
            planes = e.compute_flow_bidirectional()
            det.step()
            want = host.step(*planes)
            host.same(det, 0, want, f"pair {k}")
            for a, b in zip(planes, ref.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the planes with a detector attached differ"
            # measured, not asserted: how well the engine's own flow finds the square
            sq = np.zeros((h, w), bool)
            sq[h // 4 + 2 * (k - 1): h // 4 + 2 * (k - 1) + 24, w // 2 - (k - 1): w // 2 - (k - 1) + 24] = True
            objs = det.objects(0)
            if objs:
                big = max(range(len(objs)), key=lambda j: objs[j]["area"])
                m = det.labels(0) == big + 1
                ids.append(objs[big]["id"])
                print(f"pair {k}: {len(objs)} objects, the largest: area {objs[big]['area']}, IoU with the square {(m & sq).sum() / (m | sq).sum():.3f}, "
                      f"id {objs[big]['id']} age {objs[big]['age']}, velocity {objs[big]['velocity']}")
            else:
                print(f"pair {k}: no object")
            assert np.array_equal(det.id_map(0), np.concatenate([[0], [r["id"] for r in want[1]]]).astype(np.int32)[want[0]])
        print("the largest object's id persists:", len(ids) == 2 and ids[0] == ids[1])
        names = [n for n, _ in e.stage_times()]
        assert "objects_fit" in names and "objects_label" in names and "objects_assign" in names
        assert "stab_fit" not in names                         # the private stabiliser's launches are the detector's stage
        assert status(lambda: det.labels(1)) == ARG and status(lambda: det.reset(1)) == ARG and status(lambda: det.state(1)) == ARG
        det.reset()
        assert status(lambda: det.objects(0)) == STATE
    finally:
        det.close(); e.close(); ref.close()


def test_context_form_above_one_round_of_chunks():
    """320 x 240 is 75 chunks: the context form (private stabiliser, then the nine launches on the context's stream) where the scan has a
    second round, against the host forms fed with the context's planes"""
    import eppm_amd
    h, w = 240, 320
    noisy = moving_clip(h, w, 3, seed=61)
    e = eppm_amd.EPPM()
    e.init(h, w)
    det = eppm_amd.ObjectDetector(e, min_area=2)
    host = HostDetector(min_area=2)
    try:
        for k in (1, 2):
            if k == 1:
                e.set_data(noisy[0], noisy[1])
            else:
                e.push_frame(noisy[2])
            planes = e.compute_flow_bidirectional()
            det.step()
            want = host.step(*planes)
            host.same(det, 0, want, f"pair {k}")
            roots = [int(np.flatnonzero(want[0] == lab)[0]) for lab in range(1, want[2]["n"] + 1)]
            late = [r for r in roots if r >= 64 * 1024]
            print(f"pair {k}: counts {want[2]}, {len(late)} objects with their root in a chunk >= 64")
            assert late and len(late) < len(roots), "the second round of the scan numbers nothing, or everything"
    finally:
        det.close(); e.close()


def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    noisy = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    det = eppm_amd.ObjectDetector(e, min_area=8)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        assert status(det.step) == STATE                       # before any bidirectional call
        e.compute_flow()
        assert status(det.step) == STATE                       # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(det.step) == STATE                       # a compute_begin is pending
        e.compute_flow_end()
        assert status(det.step) == STATE                       # ... and it was forward-only
        e.compute_flow_bidirectional()
        det.step()
        first = (det.labels(0), plain(det.objects(0)), det.counts(0))
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: det.step(ctx=other)) == ARG     # size mismatch
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: det.step(ctx=bat)) == ARG       # two active pairs, one slot
        with pytest.raises(eppm_amd.EppmError):
            det.step([True, False])
        z = np.zeros(256, np.int32)
        car = np.zeros((h, w), np.uint8)
        assert status(lambda: det.set_state(1, car, z, z, 1)) == ARG
        for bad in (0, -1, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31):
            assert status(lambda: det.set_state(0, car, z, z, bad)) == ARG, bad          # next_id near 2^31
        neg = z.copy(); neg[3] = -1
        assert status(lambda: det.set_state(0, car, z, neg, 1)) == ARG
        with pytest.raises(eppm_amd.EppmError):
            det.set_state(0, car[:, :-1], z, z, 1)
        again = (det.labels(0), plain(det.objects(0)), det.counts(0))
        assert np.array_equal(first[0], again[0]) and first[1:] == again[1:]          # the refused calls changed nothing
        det.set_state(0, car, z, z, 2 ** 30)
        assert det.state(0)[3] == 2 ** 30
    finally:
        det.close(); e.close(); other.close(); bat.close()


# ---- the batch form ----

def test_eight_slots_in_one_launch():
    """eight different clips in one batch context: one step covers the eight slots, each equal to the host forms fed with its pair's
    planes; a step with fewer active pairs leaves the other slots alone"""
    import eppm_amd
    h, w = 96, 128
    clips = [moving_clip(h, w, 3, seed=50 + s, sq_v=(-1 + s % 3, 2 - s % 2), sq=16 + 2 * s) for s in range(8)]
    bat = eppm_amd.EPPMBatch(h, w, 8)
    det = eppm_amd.ObjectDetector(bat, min_area=8)
    hosts = [HostDetector(min_area=8) for _ in range(8)]
    try:
        for t in (1, 2):
            if t == 1:
                bat.set_data([(c[0], c[1]) for c in clips])
            else:
                bat.push_frames([c[2] for c in clips])
            planes = bat.compute_flow_bidirectional()
            cut = [s == 5 for s in range(8)] if t == 1 else None
            det.step(cut)
            for s in range(8):
                want = hosts[s].step(*planes[s], cut=bool(cut and cut[s]))
                hosts[s].same(det, s, want, f"slot {s} step {t}")
        assert len({tuple(det.labels(s).ravel()) for s in range(8)}) > 1
        kept = [read_slot(det, s) for s in range(8)]
        bat.set_data([(clips[0][2], clips[0][1]), (clips[1][2], clips[1][0])])          # two active pairs: slots 2 .. 7 are not covered
        planes = bat.compute_flow_bidirectional()
        det.step()
        for s in range(2):
            want = hosts[s].step(*planes[s])
            hosts[s].same(det, s, want, f"slot {s} step 3")
        for s in range(2, 8):
            now = read_slot(det, s)
            assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(now, kept[s])), f"slot {s} changed"
    finally:
        det.close(); bat.close()


# ---- end to end ----

def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def read_pgm(path):
    data = open(path, "rb").read()
    magic, dims, maxv, rest = data.split(b"\n", 3)
    assert magic == b"P5" and maxv == b"255"
    w, h = [int(x) for x in dims.split()]
    return np.frombuffer(rest, np.uint8).reshape(h, w)


def test_detect_objects_the_batch_helper_and_the_cli(tmp_path):
    import eppm_amd
    h, w = 96, 128
    clip = moving_clip(h, w, 5, seed=81)
    objs, planes = eppm_amd.detect_objects(clip, labels=True, min_area=8)
    assert len(objs) == len(planes) == 4 and all(p.shape == (h, w) and p.dtype == np.uint8 for p in planes)
    for o, p in zip(objs, planes):
        assert sorted(np.unique(p)[1:] if p.any() else []) == list(range(1, len(o) + 1))
        for k, r in enumerate(o):
            assert r["area"] == (p == k + 1).sum() >= 8 and r["centroid"] == (r["sum_x"] / r["area"], r["sum_y"] / r["area"])
    assert sum(len(o) for o in objs) > 0
    with pytest.raises(TypeError):
        eppm_amd.detect_objects(clip, smooth=0.5)
    with pytest.raises(TypeError):
        eppm_amd.detect_objects(clip, lost_permille=3)
    # a forced cut at every pair (lost_permille 0): nothing is carried, so no object is ever older than 0 and ids never repeat
    cut = eppm_amd.detect_objects(clip, auto_cut=True, lost_permille=0, min_area=8)
    assert all(r["age"] == 0 for o in cut for r in o)
    ids = [r["id"] for o in cut for r in o]
    assert ids == list(range(1, len(ids) + 1))
    # many clips through one batch context
    clips = [clip[:3], moving_clip(h, w, 2, seed=82), clip[:4]]
    many, many_planes = eppm_amd.detect_objects_sequences(clips, slots=2, labels=True, min_area=8)
    assert [len(m) for m in many] == [2, 1, 3]
    for k, c in enumerate(clips):
        single, single_planes = eppm_amd.detect_objects(c, labels=True, min_area=8)
        assert single == many[k], f"clip {k}"
        assert all(np.array_equal(a, b) for a, b in zip(single_planes, many_planes[k])), f"clip {k}"
    # the CLI
    names = []
    for j, f in enumerate(clip):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--objects", "--min-area", "8"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = []
    for k, (o, p) in enumerate(zip(objs, planes)):
        assert np.array_equal(read_pgm(f"{prefix}_ob_{k + 1:04d}.pgm"), p), f"CLI labels of pair {k}"
        for r in o:
            vel = "nan nan" if r["velocity"] is None else "%.6f %.6f" % r["velocity"]
            want.append("%d %d %d %d %d %d %d %d %.6f %.6f %s" % (k, r["id"], r["age"], r["area"], r["x0"], r["y0"], r["x1"], r["y1"], *r["centroid"], vel))
    assert open(f"{prefix}_objects.txt").read().splitlines() == want
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--max-objects", "1", "--cut-lost", "0"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    one = eppm_amd.detect_objects(clip, auto_cut=True, lost_permille=0, max_objects=1)
    assert len(open(f"{prefix}_objects.txt").read().splitlines()) == sum(len(o) for o in one)
    assert subprocess.run([exe, "--objects", names[0], names[1]], capture_output=True).returncode == 2          # the detector walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--max-objects", "256"], capture_output=True).returncode == 2
