"""GPU tests of film-defect removal: the kernels against the host form / the numpy restatement byte for byte on
defect_cases(), the launch shapes, the context and batch forms, the hand-over between streams, poisoned allocations, memory, and the
end-to-end helpers on the engine's own flows."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from alloc_fill_child import CLIP_H, CLIP_W, DevMem, across_fills, clip, pair_inputs, put, status_of
from defect_tol_child import bits, device_step, mismatches
from test_defect_cpu import DEFAULTS, LIMIT_SIZES, SIZES, defect_limit_cases, _smooth, blotch_clip, clip_quality, defect_cases, host_step, np_step, psnr
from tfilter_tol_child import rgba, to_device

pytestmark = pytest.mark.gpu

F = np.float32
ARG, STATE = 1, 3

# What the numpy restatement reaches on blotch_clip() with the CPU oracle's bidirectional flows (cold runs) and the default parameters:
# measured on the CPU.  clean_loss: the PSNR a clip without any blotch loses.
ORACLE_FLOW_QUALITY = dict(found=0.9178, false_hit=0.000168, before=23.68, after=33.40, clean_loss=0.45)
# The CPU prototype's figures, a floor for sanity and not the bar: blotch pixels repaired, clean interior pixels hit, PSNR gain.  The
# measurement above misses the first (0.918 < 0.95; 0.945 on true flows: this clip has blotches in three consecutive frames, and a blotch
# whose compensated position in a neighbour frame is damaged too is undecided -- DESIGN.md section 23 says so); the other two hold.
FLOORS = dict(found=0.95, false_hit=0.0002, gain=9.0)


# ---- 1. the kernels equal the host form ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_host_form(size):
    """every case through set_state + eppm_defect_step_frames + the getters, twice: frame, mask, stats and the saved state byte for byte
    the host form's"""
    cases = [c for c in defect_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases, want=host_step)
    assert not bad, bad[:5]
    assert not mismatches(cases[:2])              # and the restatement's, directly


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_host_form_at_the_size_limit(size):
    """thin frames 8192 long: taps and median windows at coordinate 8191, vectors that end on the last column / row and one ulp beyond
    them, the caller's images under a pitch larger than 4 * w"""
    bad = mismatches(defect_limit_cases(size))
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_tolerance_library_at_the_size_limit(size):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "defect_tol_child.py"), "limit", str(size)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "defect_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]
    got = json.loads([l for l in out.stdout.splitlines() if l.startswith("QUALITY ")][0][8:])
    print("tolerance library, engine flows:", got)
    check_quality(got)


# ---- 2. launch shapes ----

def shape_case(kind, w, h, seed):
    """radius 4, grow 4.  "mixed": a planted case; "second": every own vector wrong, so every pixel takes the second chance, whose
    medians are mostly right; "unknown": every own vector wrong and every window holds an unknown vector (all undecided)"""
    rng = np.random.default_rng(seed)
    big = _smooth(rng, h + 8, w + 8)
    noisy = lambda a: np.clip(np.rint(a) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)      # noqa: E731
    prev, cur, nxt = noisy(big[4:4 + h, 3:3 + w]), noisy(big[4:4 + h, 4:4 + w]), noisy(big[4:4 + h, 5:5 + w])   # cur(x) = prev(x + 1) = next(x - 1)
    cur[rng.random((h, w)) < 0.2] = 250
    ys, xs = np.mgrid[0:h, 0:w]
    bu, bv, fu, fv = np.full((h, w), F(1)), np.zeros((h, w), F), np.full((h, w), F(-1)), np.zeros((h, w), F)
    if kind == "plain":
        pass
    elif kind == "mixed":
        wrong = rng.random((h, w)) < 0.3
        bu[wrong] += F(w + 2)
        fu[(xs > w // 2) & (xs < w // 2 + 12)] -= F(w + 2)
    else:
        sign = np.where((xs // 2) % 2 == 0, F(1), F(-1)) * F(w + 2)
        bu = np.where(xs % 2 == 0, bu + sign, bu).astype(F)
        fu = np.where(xs % 2 == 1, fu + sign, fu).astype(F)
        if kind == "unknown":
            fv[(xs % 5 == 0) & (ys % 5 == 0)] = F(np.nan)
    c = dict(name=f"{kind}-{w}x{h}", h=h, w=w, prev=prev, cur=cur, next=nxt, bu=bu, bv=bv, fu=fu, fv=fv, params=dict(DEFAULTS, radius=4, grow=4))
    return c


@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_launch_shapes(w):
    for h in (1, 3, 5, 9):
        cases = [shape_case(kind, w, h, 100 * w + h) for kind in ("mixed", "second", "unknown")]
        bad = mismatches(cases, want=host_step)
        assert not bad, bad[:3]
        n = w * h
        _, _, st = host_step(cases[1])
        assert st["second_chance"] + st["undecided"] == n and st["second_chance"] > n // 2, st          # 100 % took the second chance
        rgb, mask, st = host_step(cases[2])
        assert st == dict(hit=0, grown=0, second_chance=0, undecided=n) and np.array_equal(rgb, cases[2]["cur"])
        _, _, st = host_step(cases[0])
        assert st["hit"] and st["grown"] and st["second_chance"] and st["undecided"], st


def test_both_median_forms_at_their_threshold():
    """a block of 64 x 4 pixels with at most 64 undecided lanes lets a wave select each pixel's medians, one with more lets every lane
    select its own: three blocks with 63, 64 and 65 lanes that want the second chance"""
    from test_defect_cpu import np_chance
    w, h = 192, 4
    c = shape_case("plain", w, h, 3)
    rng = np.random.default_rng(4)
    bu = np.full((h, w), F(1))
    for block, n in enumerate((59, 64, 61)):          # the first and the last column want it anyway: their true vectors leave the frame
        inner = [(y, x) for y in range(h) for x in range(max(64 * block, 1), min(64 * block + 64, w - 1))]
        for j in rng.choice(len(inner), n, replace=False):
            bu[inner[j]] += F(w + 2)
    c = dict(c, name="threshold", bu=bu)
    decided = np_chance(c["prev"], c["cur"], c["next"], c["bu"], c["bv"], c["fu"], c["fv"], 60.0, 30.0)[0]
    assert [int((~decided[:, 64 * b:64 * b + 64]).sum()) for b in range(3)] == [63, 64, 65]
    assert not mismatches([c], want=host_step)
    assert host_step(c)[2]["second_chance"] > 150


def test_an_uncovered_slot_keeps_its_state():
    import eppm_amd
    from eppm_amd._lib import lib
    w, h = 65, 9
    c = shape_case("mixed", w, h, 7)
    kept = shape_case("second", w, h, 8)
    flt = eppm_amd.DefectFilter(None, size=(h, w), slots=3, **c["params"])
    planes = [to_device(rgba(c["cur"])), to_device(rgba(c["next"])), to_device(np.stack([c["fu"], c["fv"]], -1)), to_device(np.zeros((h, w, 2), F))]
    try:
        flt.set_state(2, kept["prev"], np.stack([kept["bu"], kept["bv"]], -1), True)
        want = host_step(c)
        for slot in (1, 0):
            flt.set_state(slot, c["prev"], np.stack([c["bu"], c["bv"]], -1), True)
            flt.step_frames(slot, planes[0].value, planes[1].value, w * 4, planes[2].value, planes[3].value)
            assert np.array_equal(flt.frame(slot), want[0]) and np.array_equal(flt.mask(slot), want[1]) and flt.stats(slot) == want[2]
        assert flt.stats(1) == want[2]                                         # the step of slot 0 left slot 1's counts alone
        frame, bwd, has = flt.state(2)
        assert np.array_equal(frame, kept["prev"]) and np.array_equal(bits(bwd), bits(np.stack([kept["bu"], kept["bv"]], -1))) and has
        assert status_of(lambda: flt.frame(2)) == STATE and status_of(lambda: flt.mask(2)) == STATE and status_of(lambda: flt.stats(2)) == STATE
        assert status_of(lambda: flt.frame(3)) == ARG and status_of(lambda: flt.reset(3)) == ARG
    finally:
        flt.close()
        for p in planes:
            lib().eppm_free_device(p)


# ---- 3. the context and batch forms ----

class HostChain:
    """the slot's state as the header describes it, stepped by the host form"""

    def __init__(self):
        self.prev, self.bwd, self.has_prev = None, None, False

    def step(self, img1, img2, flows, cut=False):
        u, v, bu, bv = flows[:4]
        live = self.has_prev and not cut
        out = io_step(self.prev if live else None, img1, img2 if live else None, self.bwd, (u, v))
        self.prev, self.bwd, self.has_prev = img1, (bu, bv), not cut
        return out

    def reset(self):
        self.has_prev = False


def io_step(prev, cur, nxt, b, f, **params):
    from eppm_amd import io
    b = b if b is not None else (None, None)
    return io.defect_step_host(prev, cur, nxt, b[0], b[1], f[0], f[1], **(params or DEFAULTS))


def same_result(flt, slot, want, what):
    assert np.array_equal(flt.frame(slot), want[0]), what + ": frame"
    assert np.array_equal(flt.mask(slot), want[1]), what + ": mask"
    assert flt.stats(slot) == want[2], what + ": stats"


def test_context_form_equals_the_host_form_on_the_contexts_planes():
    """5 frames of 96x128 through push_frame + compute_flow_bidirectional + step, a cut at pair 2 and a reset before pair 3; a forward
    flow computed with a filter attached is the one computed without"""
    import eppm_amd
    h, w = 96, 128
    dirty, _, _, _ = blotch_clip(seed=11, h=h, w=w)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    flt = eppm_amd.DefectFilter(e)
    e.enable_stage_timing(True)
    chain = HostChain()
    hits = 0
    try:
        for k in range(4):
            for ctx in (e, plain):
                if k == 0:
                    ctx.set_data(dirty[0], dirty[1])
                else:
                    ctx.push_frame(dirty[k + 1])
            res = e.compute_flow_bidirectional()
            if k == 3:
                flt.reset(0); chain.reset()
            flt.step([k == 2])
            want = chain.step(dirty[k], dirty[k + 1], res, cut=k == 2)
            same_result(flt, 0, want, f"pair {k}")
            frame, bwd, has = flt.state(0)
            assert np.array_equal(frame, dirty[k]) and np.array_equal(bits(bwd), bits(np.stack(res[2:4], -1))) and has == (k != 2)
            if k != 1:
                assert not want[1].any() and np.array_equal(want[0], dirty[k])           # the passing steps: the first, the cut, after the reset
            hits += want[2]["hit"]
            for a, b in zip(res, plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a defect filter attached differ"
        assert hits > 50
        names = [n for n, _ in e.stage_times()]
        assert "defect_detect" in names and "defect_apply" in names
    finally:
        flt.close(); e.close(); plain.close()


def test_batch_slots_equal_the_host_form():
    import eppm_amd
    h, w = 96, 128
    clips = [blotch_clip(seed=s, h=h, w=w, n=4)[0] for s in (21, 22, 23)]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    flt = eppm_amd.DefectFilter(bat, radius=2, grow=2)
    chains = [HostChain() for _ in clips]
    try:
        for t in range(3):
            if t == 0:
                bat.set_data([(c[0], c[1]) for c in clips])
            else:
                bat.push_frames([c[t + 1] for c in clips], [False] * 3)
            res = bat.compute_flow_bidirectional()
            cut = [t == 1 and k == 1 for k in range(3)]
            flt.step(cut)
            for k in range(3):
                live = chains[k].has_prev and not cut[k]
                want = io_step(chains[k].prev if live else None, clips[k][t], clips[k][t + 1] if live else None, chains[k].bwd, res[k][:2], detect=60.0,
                               agree=30.0, radius=2, grow=2)
                chains[k].prev, chains[k].bwd, chains[k].has_prev = clips[k][t], res[k][2:4], not cut[k]
                same_result(flt, k, want, f"slot {k} step {t}")
        assert flt.stats(0)["hit"] > 20 and flt.stats(1)["hit"] == 0 and len(flt.frames()) == 3
    finally:
        flt.close(); bat.close()


# ---- 4. hand-over between streams ----

def test_a_defect_filter_stepped_from_two_streams_equals_the_host_chain():
    """context step -> frame_device -> step_frames on the launcher stream -> context step, and the reverse order, with no host
    synchronisation in between; the plane copied behind the first step is the first step's frame"""
    import eppm_amd
    from eppm_amd._lib import check, lib
    h, w = 96, 128
    dirty, _, _, _ = blotch_clip(seed=31, h=h, w=w, n=3)
    rng = np.random.default_rng(5)
    sf = np.stack([np.full((h, w), F(2)), np.full((h, w), F(1))], -1) + (rng.random((h, w, 1)) < 0.05) * F(300)
    sb = np.stack([np.full((h, w), F(-2)), np.full((h, w), F(-1))], -1) + (rng.random((h, w, 1)) < 0.05) * F(300)
    sf, sb = sf.astype(F), sb.astype(F)
    for ctx_first in (True, False):
        e = eppm_amd.EPPM(); e.init(h, w)
        e.set_data(dirty[0], dirty[1])
        flt = eppm_amd.DefectFilter(e)
        d_fwd, d_bwd, d_first = to_device(np.zeros((h, w, 2), F)), to_device(np.zeros((h, w, 2), F)), to_device(np.zeros((h, w, 4), np.uint8))
        planes = [to_device(rgba(dirty[1])), to_device(rgba(dirty[2])), to_device(sf), to_device(sb)]
        try:
            e.compute_flow_bidirectional_device(d_flow=d_fwd.value, d_flow_bwd=d_bwd.value)
            frames = lambda: flt.step_frames(0, planes[0].value, planes[1].value, w * 4, planes[2].value, planes[3].value)  # noqa: E731
            order = [flt.step, frames, flt.step] if ctx_first else [frames, flt.step, frames]
            order[0]()
            flt.frame_device(0, d_first.value, w * 4)
            order[1]()
            order[2]()
            got = (flt.frame(0), flt.mask(0), flt.stats(0))
            fwd, bwd, first = np.empty((h, w, 2), F), np.empty((h, w, 2), F), np.empty((h, w, 4), np.uint8)
            for dst, src in ((fwd, d_fwd), (bwd, d_bwd), (first, d_first)):
                check(lib().eppm_memcpy_d2h(dst.ctypes.data_as(C.c_void_p), src, C.c_size_t(dst.nbytes)), "d2h")
        finally:
            flt.close(); e.close()
            for p in [d_fwd, d_bwd, d_first] + planes:
                lib().eppm_free_device(p)
        split = lambda a: (np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1]))       # noqa: E731
        ctx_pair = (dirty[0], dirty[1], split(fwd) + split(bwd))
        own_pair = (dirty[1], dirty[2], split(sf) + split(sb))
        chain = HostChain()
        seq = [ctx_pair, own_pair, ctx_pair] if ctx_first else [own_pair, ctx_pair, own_pair]
        res = [chain.step(*p) for p in seq]
        assert np.array_equal(first[..., :3], res[0][0]) and (first[..., 3] == 255).all(), "the plane copied behind the first step"
        assert np.array_equal(got[0], res[2][0]) and np.array_equal(got[1], res[2][1]) and got[2] == res[2][2], f"context first: {ctx_first}"
        assert res[1][2]["hit"] + res[1][2]["grown"] > 0 and not np.array_equal(res[2][0], res[0][0])


# ---- 5. poisoned allocations ----

def getters(out, name, flt, slot):
    put(out, f"{name}.frame", flt.frame(slot)); put(out, f"{name}.mask", flt.mask(slot)); put(out, f"{name}.stats", flt.stats(slot))
    frame, bwd, has = flt.state(slot)
    put(out, f"{name}.saved_frame", frame); put(out, f"{name}.saved_bwd", bwd); put(out, f"{name}.has_prev", has)


def attached():
    """the filter on a context over the clip: a step per pair, the last one with a cut flag, and one more after a reset"""
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        flt = None
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            flt = eppm_amd.DefectFilter(e, detect=5.0, agree=60.0, radius=4, grow=2)
            d = DevMem(nbytes=CLIP_H * CLIP_W * 4)
            for k in range(4):              # pair 0 passes (the first), pair 1 detects, pair 2 is cut, and pair 2 once more after a reset
                if k in (1, 2):
                    e.push_frame(f[k + 1])
                if k < 3:
                    e.compute_flow_bidirectional_device()
                else:
                    flt.reset(0)
                flt.step(cut=[k == 2])
                getters(out, f"step{k}", flt, 0)
                flt.frame_device(0, d.addr, CLIP_W * 4)
                put(out, f"step{k}.device", d.get((CLIP_H, CLIP_W, 4), np.uint8))
            d.free()
        finally:
            if flt is not None:
                flt.close()
            e.close()
        return out
    return scenario


def size_only():
    """the filter without a context, three slots: slot 1 is stepped first, then slot 0, slot 2 never; slot 1 goes on with a detecting
    step, a cut step, a reset and another step"""
    import eppm_amd
    P = pair_inputs()
    pitch = CLIP_W * 4

    def scenario():
        out = {}
        flt = eppm_amd.DefectFilter(None, size=(CLIP_H, CLIP_W), slots=3, detect=5.0, agree=60.0, radius=4, grow=2)
        dev = []
        try:
            D = []
            for p in P:
                D.append({k: DevMem(p[k]) for k in ("rgba1", "rgba2", "fwd", "bwd")})
                dev += list(D[-1].values())

            def step(name, slot, k, cut=False):
                flt.step_frames(slot, D[k]["rgba1"].addr, D[k]["rgba2"].addr, pitch, D[k]["fwd"].addr, D[k]["bwd"].addr, cut)
                getters(out, name, flt, slot)

            step("slot1.step1", 1, 0)
            step("slot0.step1", 0, 0)
            getters(out, "slot1.after_slot0", flt, 1)
            step("slot1.step2", 1, 1)
            step("slot1.step3_cut", 1, 2, cut=True)
            flt.reset(1)
            step("slot1.step4_after_reset", 1, 0)
            step("slot0.step2", 0, 1)
            got = [status_of(lambda: flt.frame(2)), status_of(lambda: flt.mask(2)), status_of(lambda: flt.stats(2)), status_of(lambda: flt.state(2))]
            assert got == [STATE] * 4, got
        finally:
            flt.close()
            for d in dev:
                d.free()
        return out
    return scenario


@pytest.mark.parametrize("form", ["attached", "size_only"])
def test_defect_results_do_not_depend_on_what_memory_held(form):
    base = across_fills(attached() if form == "attached" else size_only(), f"defect filter, {form}")
    assert len(base) >= 18
    found = sorted(k for k, v in base.items() if k.endswith(".mask") and v.any())
    assert found == (["step1.mask"] if form == "attached" else ["slot0.step2.mask", "slot1.step2.mask"]), found     # the detecting steps


# ---- 6. memory ----

def free_bytes():
    from eppm_amd._lib import check, lib
    f, t = C.c_size_t(), C.c_size_t()
    check(lib().eppm_device_synchronize(), "sync")
    check(lib().eppm_device_mem_info(C.byref(f), C.byref(t)), "mem_info")
    return f.value


def test_memory_is_the_filters_own():
    import eppm_amd
    from eppm_amd._lib import check, lib
    h, w = 436, 1024
    dirty, _, _, _ = blotch_clip(seed=41, h=h, w=w, n=3)
    e = eppm_amd.EPPM(); e.init(h, w); e.set_data(dirty[0], dirty[1]); e.compute_flow_bidirectional()
    f = eppm_amd.DefectFilter(e); f.step(); f.frame(0); f.close(); e.close()          # code objects, pools
    check(lib().eppm_release_cached_memory(), "release")
    base = free_bytes()
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(dirty[0], dirty[1])
    e.compute_flow_bidirectional()
    m0 = free_bytes()
    e.compute_flow_bidirectional()
    assert free_bytes() == m0                      # a context that creates no defect filter: the use it had before
    plain = base - m0
    flt = eppm_amd.DefectFilter(e)
    doc = ((h * w * 34 + 255) & ~255) + 256        # eppm.h: 34 bytes per pixel and slot, and the stats records
    used = base - free_bytes()
    print("plain", plain, "with a defect filter", used, "documented", doc)
    assert plain + doc <= used <= plain + doc + (4 << 20)          # which the allocator may round up
    m1 = free_bytes()
    flt.step()
    e.push_frame(dirty[2])
    e.compute_flow_bidirectional()
    flt.step()
    flt.frame(0); flt.mask(0); flt.stats(0)
    assert free_bytes() == m1                      # steps allocate nothing, the context did not grow
    flt.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert free_bytes() == m0, "destroy returns the filter's block"
    e.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert free_bytes() == base


# ---- 7. end to end ----

_oracle = {}


def oracle_flows(frames):
    """per frame k of a clip (bu, bv, fu, fv): the CPU oracle's cold bidirectional flows, the backward branch chained as
    tests/test_bidirectional_gpu.py chains it; None where the frame has no such neighbour"""
    from oracle import oracle as O
    from test_bidirectional_gpu import oracle_backward, uv
    pairs = []
    for k in range(len(frames) - 1):
        u, v, st = O.compute_flow(frames[k], frames[k + 1], None, dump=True)
        _, levels = oracle_backward(st, O.default_params())
        pairs.append((np.ascontiguousarray(u, F), np.ascontiguousarray(v, F)) + uv(levels[0]))
    return [(pairs[k - 1][2], pairs[k - 1][3], pairs[k][0], pairs[k][1]) if 0 < k < len(frames) - 1 else None for k in range(len(frames))]


def oracle_run(blotched=(1, 2, 3)):
    """(dirty, clean, masks, repaired, repair masks) of the restatement on the oracle's flows"""
    if blotched not in _oracle:
        dirty, clean, masks, _ = blotch_clip(blotched=blotched)
        flows = oracle_flows(dirty)
        rep, rm = [], []
        for k, f in enumerate(flows):
            r = np_step(dirty[k - 1], dirty[k], dirty[k + 1], *f, **DEFAULTS)[:2] if f else (dirty[k], np.zeros(dirty[k].shape[:2], np.uint8))
            rep.append(r[0]); rm.append(r[1])
        _oracle[blotched] = (dirty, clean, masks, rep, rm)
    return _oracle[blotched]


def oracle_quality():
    dirty, clean, masks, rep, rm = oracle_run()
    q = dict(zip(("found", "false_hit", "before", "after"), clip_quality(dirty, clean, masks, rep, rm)))
    plain, ideal, _, rep0, _ = oracle_run(blotched=())
    q["clean_loss"] = float(np.mean([psnr(plain[k], ideal[k]) - psnr(rep0[k], ideal[k]) for k in (1, 2, 3)]))
    return q


def check_quality(got, floors=False):
    """the bars of ORACLE_FLOW_QUALITY with the margins of the CPU test (0.02 in the shares, 1 dB in PSNR; the blotch-free clip: 0.3 dB);
    floors: and the prototype's floors, where the CPU measurement itself reaches them"""
    q = ORACLE_FLOW_QUALITY
    assert got["found"] >= q["found"] - 0.02, got
    assert got["false_hit"] <= q["false_hit"] + 0.02, got
    assert got["after"] >= q["after"] - 1.0, got
    assert got["clean_loss"] <= q["clean_loss"] + 0.3, got
    if floors:
        assert q["found"] < FLOORS["found"], "the measurement reaches the floor now: assert it"
        assert got["false_hit"] <= FLOORS["false_hit"] and got["after"] - got["before"] >= FLOORS["gain"], got


def test_remove_defects_sequence_on_the_engines_own_flows():
    """128x160, 25 blotches in each of the three inner frames.  The exact library's flows are the oracle's bit for bit (cold runs:
    temporal=False), so its output is the restatement's on the oracle's flows byte for byte; the quality bars are that run's figures."""
    import eppm_amd
    dirty, clean, masks, want, want_masks = oracle_run()
    measured = oracle_quality()
    print("restatement on oracle flows:", measured)
    for k in ("found", "false_hit", "after", "clean_loss"):
        assert abs(measured[k] - ORACLE_FLOW_QUALITY[k]) <= (1.0 if k == "after" else 0.3 if k == "clean_loss" else 0.02), (k, measured)
    rep, rm = eppm_amd.remove_defects_sequence(dirty, masks=True, temporal=False)
    assert len(rep) == 5 and np.array_equal(rep[0], dirty[0]) and np.array_equal(rep[4], dirty[4])
    for k in range(5):
        assert np.array_equal(rm[k], want_masks[k]), f"mask {k}: {int((rm[k] != want_masks[k]).sum())} differ"
        assert np.array_equal(rep[k], want[k]), f"frame {k}"
    plain, ideal, _, want0, _ = oracle_run(blotched=())
    rep0 = eppm_amd.remove_defects_sequence(plain, temporal=False)
    for k in range(5):
        assert np.array_equal(rep0[k], want0[k]), f"blotch-free frame {k}"
    got = dict(zip(("found", "false_hit", "before", "after"), clip_quality(dirty, clean, masks, rep, rm)))
    got["clean_loss"] = float(np.mean([psnr(plain[k], ideal[k]) - psnr(rep0[k], ideal[k]) for k in (1, 2, 3)]))
    print("exact library, engine flows:", got)
    check_quality(got, floors=True)


def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_sequences_and_the_cli_equal_remove_defects_sequence(tmp_path):
    import eppm_amd
    from eppm_amd import io
    h, w = 96, 128
    clips = [blotch_clip(seed=70 + n, h=h, w=w, n=n, blotched=(1,))[0] for n in (2, 3, 4)]
    single = [eppm_amd.remove_defects_sequence(c, masks=True) for c in clips]
    many, many_masks = eppm_amd.remove_defects_sequences(clips, slots=2, masks=True)
    assert [len(m) for m in many] == [2, 3, 4]
    for k, (a, b) in enumerate(zip(single, many)):
        for j, (x, y) in enumerate(zip(a[0], b)):
            assert np.array_equal(x, y), f"clip {k} frame {j}"
        assert all(np.array_equal(x, y) for x, y in zip(a[1], many_masks[k]))
    assert np.array_equal(single[0][0][0], clips[0][0]) and np.array_equal(single[0][0][1], clips[0][1])          # two frames: both are ends
    assert single[2][1][1].any() and not np.array_equal(single[2][0][1], clips[2][1])                              # the blotched frame was repaired
    names = []
    for j, f in enumerate(clips[2]):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--remove-defects"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = open(prefix + "_defects.txt").read().split("\n")[:-1]
    assert len(lines) == 4
    for j, (want, want_mask) in enumerate(zip(*single[2])):
        assert np.array_equal(io.load_ppm(f"{prefix}_df_{j:04d}.ppm"), want), f"CLI frame {j}"
        raw = open(f"{prefix}_dfm_{j:04d}.pgm", "rb").read()
        assert raw.startswith(b"P5\n%d %d\n255\n" % (w, h)) and np.array_equal(np.frombuffer(raw[-h * w:], np.uint8).reshape(h, w), want_mask), f"CLI mask {j}"
        got = [int(x) for x in lines[j].split()]
        assert got[:3] == [j, int((want_mask == 1).sum()), int((want_mask == 2).sum())] and len(got) == 5, lines[j]
    assert subprocess.run([exe, "--remove-defects", names[0], names[1]], capture_output=True).returncode == 2          # the filter walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--defect-radius", "5"], capture_output=True).returncode == 2
