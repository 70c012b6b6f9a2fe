"""GPU tests of flicker removal: the kernels against the numpy restatement bit for bit on deflicker_cases(), the
context and batch forms, slots in the second and third word of the slot masks, the hand-over between streams, error codes, the
tolerance library, and the drivers end to end on the flickering clip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_deflicker_cpu import DEFAULTS, LIMIT_SIZES, SIZES, deflicker_cases, deflicker_limit_cases, flicker_clip, np_case, np_step, psnr, same
from test_tfilter_cpu import moving_clip
from deflicker_tol_child import case_planes, mismatches, read, rgba, to_device

pytestmark = pytest.mark.gpu

F = np.float32
ARG, STATE = 1, 3
# frames 1..5 of flicker_clip(): the input, the restatement on the CPU oracle's cold flows (= the exact library, byte for byte) and the
# tolerance library with its own temporal flows (measured on an MI355X)
ORACLE_FLOW_PSNR = dict(before=[30.54, 30.98, 36.20, 36.00, 37.35], after=[52.18, 46.80, 48.19, 47.04, 46.31],
                        tolerance_after=[52.18, 46.58, 47.79, 46.65, 45.85])


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


def flickering(frames, seed):
    """the frames under a global gain and offset per frame (frame 0 as it is)"""
    rng = np.random.default_rng(seed)
    return [frames[0]] + [np.clip(np.rint(f * rng.uniform(0.95, 1.05) + rng.uniform(-4, 4)), 0, 255).astype(np.uint8) for f in frames[1:]]


def host_step(ref, cur, bu, bv, o2, cut=False, **params):
    from eppm_amd import io
    return io.deflicker_step_host(ref, cur, bu, bv, o2, cut=cut, **params)


# ---- 1. the kernels equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_restatement(size):
    """every case through set_state + eppm_deflicker_step_frames + the getters, stepped twice: bytes, field bits, valid bytes and stats
    are the restatement's (which tests/test_deflicker_cpu.py holds equal to eppm_deflicker_step_host)"""
    cases = [c for c in deflicker_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """thin frames 8192 long at cell 16, 32 and 64: grids 512, 256 and 128 cells long (the field kernel's cells over more than one block),
    taps at coordinate 8191, the caller's images under a pitch larger than 4 * w; two consecutive steps"""
    cases = [c for c in deflicker_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) >= 3
    bad = mismatches(cases)
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_tolerance_library_at_the_size_limit(size):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deflicker_tol_child.py"), "limit", str(size)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_tolerance_library_runs_the_same_arithmetic_and_removes_flicker_on_its_own_flows():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deflicker_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]
    print(out.stdout.splitlines()[-2])


# ---- 2. the context form ----

def test_context_form_equals_the_host_form_and_leaves_the_flows_alone():
    import eppm_amd
    h, w = 192, 256
    clip = flickering(moving_clip(h, w, 3, seed=21)[1], 3)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    dk = eppm_amd.Deflicker(e)
    e.enable_stage_timing(True)
    ref = clip[0]                                   # the empty-slot rule
    try:
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(clip[0], clip[1])
                else:
                    ctx.push_frame(clip[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            dk.step()
            want = host_step(ref, clip[k], bu, bv, o2)
            assert same(read(dk, 0), want), f"step {k}"
            assert want[3]["valid_cells"] > want[3]["cells"] // 2 and not np.array_equal(want[0], clip[k])          # the step corrected something
            assert psnr(want[0], clip[0]) > psnr(clip[k], clip[0])
            ref = want[0]
            assert np.array_equal(dk.state(0)[0], ref) and dk.state(0)[1] is False
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a deflicker object attached differ"
        names = [n for n, _ in e.stage_times()]
        assert "deflicker_fit" in names and "deflicker_apply" in names
    finally:
        dk.close(); e.close(); plain.close()


# ---- 3. batch and slot words ----

def test_an_eight_slot_batch_with_a_clip_change_equals_single_pair_objects():
    import eppm_amd
    h, w = 96, 128
    clips = [flickering(moving_clip(h, w, 4, seed=40 + s)[1], s) for s in range(9)]
    # per slot: the frames it sees and whether the frame starts another clip; slot 5 changes to clip 8 at the third step
    seen = [[(clips[s][k], False) for k in range(4)] for s in range(8)]
    seen[5] = [(clips[5][0], False), (clips[5][1], False), (clips[8][0], True), (clips[8][1], False)]

    def walk(frames):
        e = eppm_amd.EPPM(); e.init(h, w)
        f = eppm_amd.Deflicker(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1][0], frames[k][0])
                e.compute_flow_bidirectional_device()
                f.step([frames[k][1]])
                out.append(read(f, 0))
        finally:
            f.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 8)
    dk = eppm_amd.Deflicker(bat)
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0][0], s[1][0]) for s in seen])
            else:
                bat.push_frames([s[t][0] for s in seen], [s[t][1] for s in seen])
            bat.compute_flow_bidirectional_device()
            dk.step([s[t][1] for s in seen] if t == 2 else None)
            for k in range(8):
                assert same(read(dk, k), want[k][t - 1]), f"slot {k} after step {t}"
        assert np.array_equal(want[5][1][0], clips[8][0]) and want[5][1][3]["used"] == 0          # the cut returned the new clip's frame
        assert len(dk.frames()) == 8
        kept = read(dk, 7)
        bat.set_data([(s[2][0], s[3][0]) for s in seen[:2]])             # two active pairs: the other slots are not covered
        bat.compute_flow_bidirectional_device()
        dk.step()
        assert same(read(dk, 7), kept) and np.array_equal(dk.state(7)[0], kept[0])
    finally:
        dk.close(); bat.close()


def test_slots_of_the_second_and_third_mask_word_equal_one_slot_objects():
    """a 70-slot object stepped on caller planes in slots 0, 31, 32 and 69, each with a case of its own and its own cut / empty bits"""
    import eppm_amd
    from eppm_amd._lib import lib
    cases = [c for c in deflicker_cases() if (c["w"], c["h"]) == (67, 45) and c["params"] == DEFAULTS]
    by = {(c["cut"], c["empty"]): c for c in cases}
    use = {0: by[(False, False)], 31: by[(False, True)], 32: by[(True, False)], 69: by[(True, True)]}
    dk = eppm_amd.Deflicker(None, size=(45, 67), slots=70)
    planes = {}
    try:
        for slot, c in use.items():
            planes[slot] = case_planes(c)
            if not c["empty"]:
                dk.set_state(slot, c["ref"])
        for step in range(2):
            for slot, c in use.items():
                p = planes[slot]
                dk.step_frames(slot, p[0].value, p[1].value, 67 * 4, p[2].value, p[3].value, c["cut"] and step == 0)
        for slot, c in use.items():
            first = np_case(c)
            want = np_step(first[0], c["cur"], c["bu"], c["bv"], c["occ2"], **c["params"])
            assert same(read(dk, slot), want), f"slot {slot}"
            assert want[3]["used"] > 0
        assert status(lambda: dk.frame(1)) == STATE and status(lambda: dk.frame(68)) == STATE and status(lambda: dk.frame(70)) == ARG
    finally:
        dk.close()
        for ps in planes.values():
            for p in ps:
                lib().eppm_free_device(p)


# ---- 4. hand-over between streams ----

def test_an_object_stepped_from_two_streams_equals_the_host_chain():
    """context step -> frame_device -> step_frames on the launcher stream -> context step, and the reverse order, with no host
    synchronisation in between; the plane copied behind the first step is the first step's frame"""
    import eppm_amd
    from eppm_amd._lib import check, lib
    h, w = 96, 128
    _, noisy, flows, masks = moving_clip(h, w, 3, seed=31)
    clip = flickering(noisy, 7)
    rng = np.random.default_rng(5)
    sb = (np.stack(flows[1], -1) + (rng.random((h, w, 1)) < 0.05) * F(300)).astype(F)           # the true vectors of pair (1, 2), some far out
    so = masks[1] | (rng.random((h, w)) < 0.05).astype(np.uint8)
    for ctx_first in (True, False):
        e = eppm_amd.EPPM(); e.init(h, w)
        e.set_data(clip[0], clip[1])
        dk = eppm_amd.Deflicker(e)
        d_bwd, d_occ, d_first = to_device(np.zeros((h, w, 2), F)), to_device(np.zeros((h, w), np.uint8)), to_device(np.zeros((h, w, 4), np.uint8))
        planes = [to_device(rgba(clip[1])), to_device(rgba(clip[2])), to_device(sb), to_device(so)]
        try:
            e.compute_flow_bidirectional_device(d_flow_bwd=d_bwd.value, d_occ2=d_occ.value)
            frames = lambda: dk.step_frames(0, planes[0].value, planes[1].value, w * 4, planes[2].value, planes[3].value)  # noqa: E731
            order = [dk.step, frames, dk.step] if ctx_first else [frames, dk.step, frames]
            order[0]()
            dk.frame_device(0, d_first.value, w * 4)
            order[1]()
            order[2]()
            got = read(dk, 0)
            bwd, occ, first = np.empty((h, w, 2), F), np.empty((h, w), np.uint8), np.empty((h, w, 4), np.uint8)
            for dst, src in ((bwd, d_bwd), (occ, d_occ), (first, d_first)):
                check(lib().eppm_memcpy_d2h(dst.ctypes.data_as(C.c_void_p), src, C.c_size_t(dst.nbytes)), "d2h")
        finally:
            dk.close(); e.close()
            for p in [d_bwd, d_occ, d_first] + planes:
                lib().eppm_free_device(p)
        ctx_pair = (clip[0], clip[1], np.ascontiguousarray(bwd[..., 0]), np.ascontiguousarray(bwd[..., 1]), occ)
        own_pair = (clip[1], clip[2], np.ascontiguousarray(sb[..., 0]), np.ascontiguousarray(sb[..., 1]), so)
        seq = [ctx_pair, own_pair, ctx_pair] if ctx_first else [own_pair, ctx_pair, own_pair]
        res, ref = [], None
        for img1, img2, bu, bv, o2 in seq:
            res.append(host_step(img1 if ref is None else ref, img2, bu, bv, o2))
            ref = res[-1][0]
        assert np.array_equal(first[..., :3], res[0][0]) and (first[..., 3] == 255).all(), "the plane copied behind the first step"
        assert same(got, res[2]), f"context first: {ctx_first}"
        fits = res[1 if ctx_first else 0]               # the caller's pair on the reference that belongs to it
        assert fits[3]["valid_cells"] > fits[3]["cells"] // 2 and not np.array_equal(fits[0], clip[2])          # ... corrected something


# ---- 5. state and arguments ----

def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    clip = flickering(moving_clip(h, w, 2, seed=41)[1], 9)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(clip[0], clip[1])
    dk = eppm_amd.Deflicker(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        for get in (dk.frame, dk.field, dk.stats, dk.state):
            assert status(lambda: get(0)) == STATE              # a slot never stepped
        assert status(dk.step) == STATE                         # before any bidirectional call
        e.compute_flow()
        assert status(dk.step) == STATE                         # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(dk.step) == STATE                         # a compute_begin is pending
        e.compute_flow_end()
        assert status(dk.step) == STATE                         # ... and it was forward-only
        e.compute_flow_bidirectional()
        dk.step()
        first = read(dk, 0)
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: dk.step(ctx=other)) == ARG        # size mismatch
        bat.set_data([(clip[0], clip[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: dk.step(ctx=bat)) == ARG          # two active pairs, one slot
        assert status(lambda: dk.frame(1)) == ARG and status(lambda: dk.reset(1)) == ARG and status(lambda: dk.set_state(1, clip[0])) == ARG
        assert status(lambda: dk.step_frames(0, 0, 0, w * 4, 0, 0)) == ARG and status(lambda: dk.step_frames(1, 8, 8, w * 4, 8, 8)) == ARG
        assert status(lambda: dk.step_frames(0, 8, 8, w * 4 - 1, 8, 8)) == ARG and status(lambda: dk.frame_device(0, 8, w * 4 - 4)) == ARG
        assert same(read(dk, 0), first)                          # the refused calls changed nothing
        dk.reset()
        assert dk.state(0)[1] is True and same(read(dk, 0), first)       # an empty slot keeps what its last step left
        dk.set_state(0, clip[0])
        assert np.array_equal(dk.state(0)[0], clip[0]) and dk.state(0)[1] is False and np.array_equal(dk.frame(0), clip[0])
    finally:
        dk.close(); e.close(); other.close(); bat.close()


# ---- 6. end to end ----

def oracle_planes(frames):
    """per pair (k, k + 1) of a clip (bu, bv, occ2): the CPU oracle's cold backward flow, the backward branch chained as
    tests/test_defect_gpu.py::oracle_flows chains it, and the host criterion's mask"""
    from eppm_amd import io
    from oracle import oracle as O
    from test_bidirectional_gpu import oracle_backward, uv
    out = []
    for k in range(len(frames) - 1):
        u, v, st = O.compute_flow(frames[k], frames[k + 1], None, dump=True)
        _, levels = oracle_backward(st, O.default_params())
        bu, bv = uv(levels[0])
        out.append((bu, bv, io.fb_occlusion(bu, bv, np.ascontiguousarray(u, F), np.ascontiguousarray(v, F))))
    return out


def test_deflicker_sequence_on_the_engines_own_flows(tmp_path):
    """128 x 160, five flickering frames after a clean one.  The exact library's cold flows (temporal=False) are the CPU oracle's bit for
    bit, so its output is the restatement's on the oracle's flows byte for byte; so are deflicker_sequences' and the CLI's."""
    import eppm_amd
    from eppm_amd import io
    flick, plain, _ = flicker_clip()
    planes = oracle_planes(flick)
    want = [flick[0]]
    for k in range(1, 6):
        want.append(np_step(want[-1], flick[k], *planes[k - 1], **DEFAULTS)[0])
    before = [psnr(flick[k], plain[k]) for k in range(1, 6)]
    after = [psnr(want[k], plain[k]) for k in range(1, 6)]
    print("restatement on oracle flows: before", [round(float(x), 2) for x in before], "after", [round(float(x), 2) for x in after])
    assert np.allclose(before, ORACLE_FLOW_PSNR["before"], atol=0.005) and np.allclose(after, ORACLE_FLOW_PSNR["after"], atol=0.005)
    assert all(a > b for a, b in zip(after, before))
    out, fields = eppm_amd.deflicker_sequence(flick, temporal=False, fields=True)
    assert len(out) == 6 and len(fields) == 5 and fields[0][0].shape == (4, 5, 6)
    for k in range(6):
        assert np.array_equal(out[k], want[k]), f"frame {k}: {int((out[k] != want[k]).sum())} bytes differ"
    many = eppm_amd.deflicker_sequences([flick[:3], flick[2:]], slots=2, temporal=False)
    assert all(np.array_equal(a, b) for a, b in zip(many[0], want[:3]))
    assert np.array_equal(many[1][0], flick[2]) and len(many[1]) == 4
    names = []
    for j, f in enumerate(flick[:3]):
        names.append(str(tmp_path / f"f{j}.ppm"))
        with open(names[-1], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (f.shape[1], f.shape[0]) + f.tobytes())
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--deflicker", "--temporal", "0"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j in range(3):
        assert np.array_equal(io.load_ppm(f"{prefix}_fk_{j:04d}.ppm"), want[j]), f"CLI frame {j}"
    assert subprocess.run([exe, "--deflicker", names[0], names[1]], capture_output=True).returncode == 2          # the object walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--flicker-cell", "24"], capture_output=True).returncode == 2
