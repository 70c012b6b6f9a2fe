"""GPU tests of motion-compensated deinterlacing: the kernels against the numpy restatement byte for byte on
deint_cases() and at the size limit, the context and batch forms, slots in the second and third word of the slot masks, the hand-over
between streams, error codes, the tolerance library, and the driver end to end on an interlaced rendering of a moving clip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_deint_cpu import DEFAULTS, LIMIT_SIZES, SIZES, deint_cases, deint_limit_cases, field_clip, np_bob, np_step, psnr, run_case, same
from test_tfilter_cpu import moving_clip
from deflicker_tol_child import rgba, to_device
from deint_tol_child import mismatches, read, step_planes

pytestmark = pytest.mark.gpu

F = np.float32
ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


def host_step(ref, cur, bu, bv, o2, parity, cut=False, **params):
    from eppm_amd import io
    return io.deint_step_host(ref, cur, bu, bv, o2, parity, cut=cut, **params)


def interlaced(h, w, n, seed, first=0):
    """(field frames, progressive frames) of a moving clip read as fields"""
    clean = moving_clip(h, w, n, seed=seed, sigma=0)[0]
    return field_clip(clean, first), clean


# ---- 1. the kernels equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_restatement(size):
    """every case through set_state + eppm_deint_step_frames + the getters, both steps, and k_deint_bob on the case's field: bytes, mask
    and stats are the restatement's (which tests/test_deint_cpu.py holds equal to the host forms)"""
    cases = [c for c in deint_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) >= 2
    bad = mismatches(cases)
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """thin frames 8192 long, taps at coordinate 8191, the caller's images under a pitch larger than 4 * w; two consecutive steps"""
    cases = [c for c in deint_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) == 2 and all(c["pad"] > 0 for c in cases)
    bad = mismatches(cases)
    assert not bad, bad


def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deint_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context form ----

def test_context_form_equals_the_host_form_and_leaves_the_flows_alone():
    import eppm_amd
    h, w = 192, 256
    fields, _ = interlaced(h, w, 3, 21)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    di = eppm_amd.Deinterlacer(e)
    e.enable_stage_timing(True)
    ref = fields[0]                                   # the empty-slot rule
    try:
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(fields[0], fields[1])
                else:
                    ctx.push_frame(fields[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            di.step(parity=k & 1)
            want = host_step(ref, fields[k], bu, bv, o2, k & 1)
            assert same(read(di, 0), want), f"step {k}"
            assert want[2]["temporal"] > 0 and want[2]["spatial"] > 0          # the step took pixels both ways
            ref = want[0]
            assert np.array_equal(di.state(0)[0], ref) and di.state(0)[1] is False
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a deinterlacer attached differ"
        assert "deint_step" in [n for n, _ in e.stage_times()]
    finally:
        di.close(); e.close(); plain.close()


# ---- 3. batch and slot words ----

def test_an_eight_slot_batch_with_a_clip_change_equals_single_pair_objects():
    import eppm_amd
    h, w = 96, 128
    clips = [interlaced(h, w, 4, 40 + s, first=s & 1)[0] for s in range(9)]
    # per slot: the field frames it sees, their parity and whether the frame starts another clip; slot 5 changes to clip 8 at the third step
    seen = [[(clips[s][k], (s & 1) ^ (k & 1), False) for k in range(4)] for s in range(8)]
    seen[5] = [seen[5][0], seen[5][1], (clips[8][0], 0, True), (clips[8][1], 1, False)]

    def walk(frames):
        e = eppm_amd.EPPM(); e.init(h, w)
        f = eppm_amd.Deinterlacer(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1][0], frames[k][0])
                e.compute_flow_bidirectional_device()
                f.step([frames[k][2]], [frames[k][1]])
                out.append(read(f, 0))
        finally:
            f.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 8)
    di = eppm_amd.Deinterlacer(bat)
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0][0], s[1][0]) for s in seen])
            else:
                bat.push_frames([s[t][0] for s in seen], [s[t][2] for s in seen])
            bat.compute_flow_bidirectional_device()
            di.step([s[t][2] for s in seen] if t == 2 else None, [s[t][1] for s in seen])
            for k in range(8):
                assert same(read(di, k), want[k][t - 1]), f"slot {k} after step {t}"
        assert np.array_equal(want[5][1][0], clips[8][0]) and want[5][1][2]["temporal"] == 0          # the cut returned the new clip's bob
        assert {s[3][1] for s in seen} == {0, 1} and len(di.frames()) == 8
        kept = read(di, 7)
        bat.set_data([(s[2][0], s[3][0]) for s in seen[:2]])             # two active pairs: the other slots are not covered
        bat.compute_flow_bidirectional_device()
        di.step(None, [s[3][1] for s in seen[:2]])
        assert same(read(di, 7), kept) and np.array_equal(di.state(7)[0], kept[0])
    finally:
        di.close(); bat.close()


def test_slots_of_the_second_and_third_mask_word_carry_their_own_parity_and_cut_bits():
    """a 70-slot object at 8 x 8 stepped on caller planes in slots 0, 31, 32 and 69, each with its own parity, cut and empty bits"""
    import eppm_amd
    from eppm_amd._lib import lib
    from test_deint_cpu import _case
    use = {0: _case(900, 8, 8, 0), 31: _case(901, 8, 8, 1, empty=True), 32: _case(902, 8, 8, 1, cut=True), 69: _case(903, 8, 8, 0, cut=True, empty=True)}
    di = eppm_amd.Deinterlacer(None, size=(8, 8), slots=70)
    planes = []
    try:
        for slot, c in use.items():
            if not c["empty"]:
                di.set_state(slot, c["ref"])
        for k in range(2):
            for slot, c in use.items():
                s = c["steps"][k]
                p = step_planes(c, s)
                planes += p
                di.step_frames(slot, p[0].value, p[1].value, 8 * 4, p[2].value, p[3].value, c["cut"] and k == 0, s["parity"])
        for slot, c in use.items():
            assert same(read(di, slot), run_case(c, np_step)[1]), f"slot {slot}"
        assert status(lambda: di.frame(1)) == STATE and status(lambda: di.frame(68)) == STATE and status(lambda: di.frame(70)) == ARG
    finally:
        di.close()
        for p in planes:
            lib().eppm_free_device(p)


# ---- 4. hand-over between streams ----

def test_an_object_stepped_from_two_streams_equals_the_host_chain():
    """context step -> frame_device -> step_frames on the launcher stream -> context step, and the reverse order, with no host
    synchronisation in between; the plane copied behind the first step is the first step's frame"""
    import eppm_amd
    from eppm_amd._lib import check, lib
    h, w = 96, 128
    clean, _, flows, masks = moving_clip(h, w, 3, seed=31, sigma=0)
    fields = field_clip(clean)
    rng = np.random.default_rng(5)
    sb = (np.stack(flows[1], -1) + (rng.random((h, w, 1)) < 0.05) * F(300)).astype(F)           # the true vectors of pair (1, 2), some far out
    so = masks[1] | (rng.random((h, w)) < 0.05).astype(np.uint8)
    for ctx_first in (True, False):
        e = eppm_amd.EPPM(); e.init(h, w)
        e.set_data(fields[0], fields[1])
        di = eppm_amd.Deinterlacer(e)
        d_bwd, d_occ, d_first = to_device(np.zeros((h, w, 2), F)), to_device(np.zeros((h, w), np.uint8)), to_device(np.zeros((h, w, 4), np.uint8))
        planes = [to_device(rgba(fields[1])), to_device(rgba(fields[2])), to_device(sb), to_device(so)]
        try:
            e.compute_flow_bidirectional_device(d_flow_bwd=d_bwd.value, d_occ2=d_occ.value)
            own = lambda: di.step_frames(0, planes[0].value, planes[1].value, w * 4, planes[2].value, planes[3].value, False, 0)  # noqa: E731
            ctx = lambda: di.step(parity=1)  # noqa: E731
            order = [ctx, own, ctx] if ctx_first else [own, ctx, own]
            order[0]()
            di.frame_device(0, d_first.value, w * 4)
            order[1]()
            order[2]()
            got = read(di, 0)
            bwd, occ, first = np.empty((h, w, 2), F), np.empty((h, w), np.uint8), np.empty((h, w, 4), np.uint8)
            for dst, src in ((bwd, d_bwd), (occ, d_occ), (first, d_first)):
                check(lib().eppm_memcpy_d2h(dst.ctypes.data_as(C.c_void_p), src, C.c_size_t(dst.nbytes)), "d2h")
        finally:
            di.close(); e.close()
            for p in [d_bwd, d_occ, d_first] + planes:
                lib().eppm_free_device(p)
        ctx_pair = (fields[0], fields[1], np.ascontiguousarray(bwd[..., 0]), np.ascontiguousarray(bwd[..., 1]), occ, 1)
        own_pair = (fields[1], fields[2], np.ascontiguousarray(sb[..., 0]), np.ascontiguousarray(sb[..., 1]), so, 0)
        seq = [ctx_pair, own_pair, ctx_pair] if ctx_first else [own_pair, ctx_pair, own_pair]
        res, ref = [], None
        for img1, img2, bu, bv, o2, parity in seq:
            res.append(host_step(img1 if ref is None else ref, img2, bu, bv, o2, parity))
            ref = res[-1][0]
        assert np.array_equal(first[..., :3], res[0][0]) and (first[..., 3] == 255).all(), "the plane copied behind the first step"
        assert same(got, res[2]), f"context first: {ctx_first}"
        assert all(r[2]["temporal"] > 0 for r in res)


# ---- 5. state and arguments ----

def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    fields, _ = interlaced(h, w, 2, 41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(fields[0], fields[1])
    di = eppm_amd.Deinterlacer(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    step = lambda **kw: di.step(parity=1, **kw)  # noqa: E731
    try:
        for get in (di.frame, di.mask, di.stats, di.state):
            assert status(lambda: get(0)) == STATE              # a slot never stepped
        assert status(step) == STATE                            # before any bidirectional call
        e.compute_flow()
        assert status(step) == STATE                            # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(step) == STATE                            # a compute_begin is pending
        e.compute_flow_end()
        assert status(step) == STATE                            # ... and it was forward-only
        e.compute_flow_bidirectional()
        assert eppm_amd.lib().eppm_deint_step(di._f, e._ctx, None, None) == ARG                    # parity is required
        assert eppm_amd.lib().eppm_deint_step(di._f, e._ctx, None, (C.c_uint8 * 1)(2)) == ARG
        with pytest.raises(eppm_amd.EppmError, match="parity"):
            di.step()
        step()
        first = read(di, 0)
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: step(ctx=other)) == ARG           # size mismatch
        bat.set_data([(fields[0], fields[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: di.step(parity=[1, 1], ctx=bat)) == ARG          # two active pairs, one slot
        assert status(lambda: di.frame(1)) == ARG and status(lambda: di.reset(1)) == ARG and status(lambda: di.set_state(1, fields[0])) == ARG
        assert status(lambda: di.step_frames(0, 0, 0, w * 4, 0, 0)) == ARG and status(lambda: di.step_frames(1, 8, 8, w * 4, 8, 8)) == ARG
        assert status(lambda: di.step_frames(0, 8, 8, w * 4 - 1, 8, 8)) == ARG and status(lambda: di.frame_device(0, 8, w * 4 - 4)) == ARG
        assert status(lambda: di.step_frames(0, 8, 8, w * 4, 8, 8, False, 2)) == ARG
        assert same(read(di, 0), first)                          # the refused calls changed nothing
        di.reset()
        assert di.state(0)[1] is True and same(read(di, 0), first)       # an empty slot keeps what its last step left
        di.set_state(0, fields[0])
        assert np.array_equal(di.state(0)[0], fields[0]) and di.state(0)[1] is False and np.array_equal(di.frame(0), fields[0])
    finally:
        di.close(); e.close(); other.close(); bat.close()


# ---- 6. end to end ----

def test_deinterlace_sequence_equals_the_host_chain_on_the_engines_own_flows():
    """96 x 128, four progressive frames of a moving clip woven into two interlaced frames: the driver's 2n outputs are the host form
    chained over the flows a plain context computes on the same field frames, byte for byte; the PSNRs against the progressive frames are
    printed next to the line average's"""
    import eppm_amd
    h, w = 96, 128
    clean = moving_clip(h, w, 4, sigma=0, bg_v=(2, 0), sq_v=(-1, 2))[0]
    woven = []
    for k in (0, 2):
        f = clean[k].copy()
        f[1::2] = clean[k + 1][1::2]                   # top field first: the even rows are the earlier picture
        woven.append(f)
    fields = field_clip(clean)
    e = eppm_amd.EPPM(); e.init(h, w)
    want, masks = [fields[0]], []
    try:
        for k in range(1, 4):
            e.set_data(fields[k - 1], fields[k])
            _, _, bu, bv, _, o2 = e.compute_flow_bidirectional()
            rgb, m, _ = host_step(want[-1], fields[k], bu, bv, o2, k & 1, **DEFAULTS)
            want.append(rgb); masks.append(m)
    finally:
        e.close()
    out, ms = eppm_amd.deinterlace_sequence(woven, temporal=False, masks=True)
    assert len(out) == 4 and len(ms) == 4
    for k in range(4):
        assert np.array_equal(out[k], want[k]), f"frame {k}: {int((out[k] != want[k]).sum())} bytes differ"
    assert all(np.array_equal(a, b) for a, b in zip(ms[1:], masks)) and set(np.unique(ms[0])) == {0, 2}
    bob = [psnr(fields[k], clean[k]) for k in range(1, 4)]
    got = [psnr(out[k], clean[k]) for k in range(1, 4)]
    print("engine flows: line average", [round(float(x), 2) for x in bob], "deinterlaced", [round(float(x), 2) for x in got])
    single = eppm_amd.deinterlace_sequence(woven, temporal=False, double_rate=False)
    assert len(single) == 2 and np.array_equal(single[0], want[0]) and np.array_equal(single[1], want[2])
    many = eppm_amd.deinterlace_sequences([woven, woven[1:]], slots=2, temporal=False)
    assert all(np.array_equal(a, b) for a, b in zip(many[0], want)) and len(many[1]) == 2 and np.array_equal(many[1][0], fields[2])
    # bottom field first reads the same rows in the other order
    bff = eppm_amd.deinterlace_sequence(woven, tff=False, temporal=False)
    assert np.array_equal(bff[0], np_bob(woven[0][1::2], h, 1)) and np.array_equal(bff[1][0::2], woven[0][0::2])


def test_the_cli_writes_what_deinterlace_sequence_returns(tmp_path):
    """runeppm --sequence ... --deinterlace on PPM frames (--bff, --single-rate, --deint-thresh) and on interlaced y4m clips (the field
    order from the file; --y4m-out at twice the frame rate) against deinterlace_sequence byte for byte; an interlaced y4m clip is
    refused without --deinterlace, and the flags are refused without it"""
    import eppm_amd
    from eppm_amd import io, yuv
    from test_deint_cpu import write_interlaced
    h, w = 96, 128
    clean = moving_clip(h, w, 4, sigma=0, bg_v=(2, 0), sq_v=(-1, 2))[0]
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True, timeout=300)       # noqa: E731

    def weave(first):
        out = []
        for k in (0, 2):
            f = clean[k].copy()
            f[1 - first::2] = clean[k + 1][1 - first::2]
            out.append(f)
        return out
    names = []
    for j, f in enumerate(weave(1)):
        names.append(str(tmp_path / f"f{j}.ppm"))
        with open(names[-1], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h) + f.tobytes())
    prefix = str(tmp_path / "out")
    r = run("--sequence", *names, "--out-prefix", prefix, "--deinterlace", "--bff", "--deint-thresh", "12", "--temporal", "0")
    assert r.returncode == 0, r.stdout + r.stderr
    want = eppm_amd.deinterlace_sequence(weave(1), tff=False, temporal=False, thresh=12)
    assert len(want) == 4 and not os.path.exists(f"{prefix}_di_0004.ppm")
    for j in range(4):
        assert np.array_equal(io.load_ppm(f"{prefix}_di_{j:04d}.ppm"), want[j]), f"CLI frame {j}"
    prefix = str(tmp_path / "single")
    r = run("--sequence", names[0], "--out-prefix", prefix, "--deinterlace", "--single-rate")          # one interlaced frame is a clip
    assert r.returncode == 0, r.stdout + r.stderr
    one = eppm_amd.deinterlace_sequence(weave(1)[:1], double_rate=False)
    assert len(one) == 1 and np.array_equal(io.load_ppm(f"{prefix}_di_0000.ppm"), one[0]) and not os.path.exists(f"{prefix}_di_0001.ppm")
    # y4m clips: the field order is the file's, whatever --bff says
    fmt = yuv.YuvFormat(layout=yuv.I420, matrix=yuv.BT601)
    for tag, first in (("It", 0), ("Ib", 1)):
        clip = str(tmp_path / f"{tag}.y4m")
        write_interlaced(clip, [yuv.from_rgb(f, fmt) for f in weave(first)], tag, fps=(30000, 1001))
        prefix = str(tmp_path / tag)
        r = run("--sequence", clip, "--out-prefix", prefix, "--deinterlace", "--y4m-out", *(["--bff"] if first == 0 else []))
        assert r.returncode == 0, r.stdout + r.stderr
        reader = yuv.read_y4m(clip, interlaced=True)
        assert reader.interlace == first + 1
        want = eppm_amd.deinterlace_sequence(list(reader), tff=first == 0)
        got = yuv.read_y4m(f"{prefix}_di.y4m", native=True)
        assert (got.h, got.w, got.fps) == (h, w, (60000, 1001))
        frames = list(got)
        assert len(frames) == 4
        for j, f in enumerate(frames):
            back = yuv.from_rgb(want[j], f.fmt)
            assert all(np.array_equal(a, b) for a, b in zip(f.planes, back.planes)), f"{tag} frame {j}"
        r = run("--sequence", clip, "--out-prefix", prefix, "--denoise")
        assert r.returncode == 1 and f"interlaced material ({tag}) is not supported" in r.stderr
    r = run("--sequence", str(tmp_path / "It.y4m"), "--out-prefix", prefix, "--deinterlace", "--single-rate", "--y4m-out")
    assert r.returncode == 0 and yuv.read_y4m(f"{prefix}_di.y4m").fps == (30000, 1001) and len(list(yuv.read_y4m(f"{prefix}_di.y4m"))) == 2
    for bad in (["--bff"], ["--single-rate"], ["--deinterlace", "--denoise"], ["--deinterlace", "--auto-cut"], ["--deint-thresh", "766"]):
        assert run("--sequence", *names, "--out-prefix", prefix, *bad).returncode == 2, bad
    assert run("--deinterlace", names[0], names[1]).returncode == 2
