"""GPU tests of global camera-motion estimation and video stabilisation: the kernels against the numpy restatement
bit for bit on stab_cases() in both libraries, the context and batch forms, call order and arguments, and the end-to-end helpers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from stabilize_tol_child import mismatches
from test_stabilize_cpu import LIMIT_SIZES, OFFSETS, SIZES, stab_limit_cases, band_limited, host_step, moving_clip, same_bits, same_model, stab_cases

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


# ---- 1. the kernels equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_restatement(size):
    """every case through reset / set_path + eppm_stab_step_frames + the getters, twice: model, path, mask and frame bit for bit the
    restatement's (which tests/test_stabilize_cpu.py holds equal to the host forms)"""
    cases = [c for c in stab_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """thin frames 8192 long: gm_X / gm_Y up to +-4095.5, 256 and 512 slabs under the solve kernel's 64 lanes, the warp's taps at
    coordinate 8191, the caller's image under a pitch larger than 4 * w"""
    cases = [c for c in stab_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) >= 3
    bad = mismatches(cases)
    assert not bad, bad


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stabilize_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stabilize_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context form ----

def host_walk(img2, u, v, o1, path, tau=1.0, iters=3, smooth=0.9, cut=False):
    """one step of the host forms from `path` (None: an empty slot) on engine planes: dict(model, mask, C, S, rgb)"""
    c = dict(u=u, v=v, occ=o1, tau=tau, iters=iters, smooth=smooth, cut=cut, path=path, img2=img2)
    return host_step(c)


def test_context_form_equals_the_host_forms_and_leaves_the_flows_alone():
    import eppm_amd
    h, w = 192, 256
    noisy = moving_clip(h, w, 3, seed=21)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    stab = eppm_amd.Stabilizer(e)
    e.enable_stage_timing(True)
    path = None
    try:
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            stab.step()
            want = host_walk(noisy[k], u, v, o1, path)
            path = (want["C"], want["S"])
            cc, ss = stab.path(0)
            assert same_model(stab.model(0), want["model"]) and want["model"]["valid"], f"model after step {k}"
            assert same_bits(cc, want["C"]) and same_bits(ss, want["S"]), f"path after step {k}"
            assert np.array_equal(stab.mask(0), want["mask"]), f"mask after step {k}"
            assert np.array_equal(stab.frame(0), want["rgb"]), f"frame after step {k}"
            assert (want["mask"] == 0).mean() > 0.5              # the background moves with the camera
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a stabiliser attached differ"
        names = [n for n, _ in e.stage_times()]
        assert "stab_fit" in names and "stab_warp" in names
    finally:
        stab.close(); e.close(); plain.close()


# ---- 3. batch ----

def test_batch_slots_equal_single_pair_stabilizers():
    import eppm_amd
    h, w = 157, 211
    A, B, Cc, D = [moving_clip(h, w, 5, seed=s) for s in (31, 32, 33, 34)]
    # per slot: the frames it sees and whether the frame starts another clip
    seen = [[(A[k], False) for k in range(5)],
            [(B[0], False), (B[1], False), (B[2], False), (Cc[0], True), (Cc[1], False)],
            [(D[k], False) for k in range(4)]]

    def snapshot(s, slot):
        return dict(model=s.model(slot), path=s.path(slot, counts=True), mask=s.mask(slot), rgb=s.frame(slot))

    def same(a, b):
        return (same_model(a["model"], b["model"]) and same_bits(a["path"][0], b["path"][0]) and same_bits(a["path"][1], b["path"][1])
                and a["path"][2] == b["path"][2] and np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["rgb"], b["rgb"]))

    def walk(frames):
        """a single-pair context's stabiliser over the slot's frames: a snapshot after every step"""
        e = eppm_amd.EPPM(); e.init(h, w)
        s = eppm_amd.Stabilizer(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1][0], frames[k][0])
                e.compute_flow_bidirectional_device()
                s.step([frames[k][1]])
                out.append(snapshot(s, 0))
        finally:
            s.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    stab = eppm_amd.Stabilizer(bat)
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0][0], s[1][0]) for s in seen])
            else:
                bat.push_frames([s[t][0] for s in seen], [s[t][1] for s in seen])
            bat.compute_flow_bidirectional_device()
            stab.step([s[t][1] for s in seen] if t == 3 else None)
            for k in range(3):
                assert same(snapshot(stab, k), want[k][t - 1]), f"slot {k} after step {t}"
        cut = snapshot(stab, 1)
        assert same_bits(cut["path"][0], (1, 0, 0, 1, 0, 0)) and cut["path"][2] == (0, 0) and np.array_equal(cut["rgb"], Cc[0])   # the cut left the new clip's frame
        assert snapshot(stab, 0)["path"][2][0] == 3 and len(stab.frames()) == 3
        kept = snapshot(stab, 2)
        # one step with two active pairs: slot 2 is not covered
        bat.set_data([(seen[0][3][0], seen[0][4][0]), (seen[1][3][0], seen[1][4][0])])
        bat.compute_flow_bidirectional_device()
        stab.step()
        for k in range(2):
            assert same(snapshot(stab, k), want[k][3]), f"slot {k} after the two-pair step"
        assert same(snapshot(stab, 2), kept) and same(kept, want[2][2])
    finally:
        stab.close(); bat.close()


# ---- 4. call order and arguments ----

def test_call_order_and_arguments():
    import eppm_amd
    from eppm_amd._lib import check, lib
    h, w = 96, 128
    noisy = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    stab = eppm_amd.Stabilizer(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        for get in (stab.frame, stab.mask, stab.model):
            assert status(lambda: get(0)) == STATE             # an empty slot
        assert same_bits(stab.path(0)[0], (1, 0, 0, 1, 0, 0))  # ... whose path is the identity
        assert status(stab.step) == STATE                      # before any bidirectional call
        e.compute_flow()
        assert status(stab.step) == STATE                      # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(stab.step) == STATE                      # a compute_begin is pending
        e.compute_flow_end()
        assert status(stab.step) == STATE                      # ... and it was forward-only
        e.compute_flow_bidirectional()
        stab.step()
        first = stab.path(0, counts=True)
        frame = stab.frame(0)
        # the device getter: RGBA words (alpha 255) into a pitched caller plane, behind the step on its stream
        pitch = w * 4 + 64
        plane = C.c_void_p()
        check(lib().eppm_malloc_device(C.byref(plane), C.c_size_t(pitch * h)), "malloc")
        try:
            check(lib().eppm_memset_device(plane, 0x11, C.c_size_t(pitch * h)), "memset")
            e.compute_flow_bidirectional_device()
            stab.reset(0)
            stab.step()                                        # asynchronous; the copy below is ordered behind it
            stab.frame_device(0, plane.value, pitch)
            got = np.empty((h, pitch), np.uint8)
            check(lib().eppm_device_synchronize(), "sync")
            check(lib().eppm_memcpy_d2h(got.ctypes.data_as(C.c_void_p), plane, C.c_size_t(pitch * h)), "d2h")
            words = got[:, :w * 4].reshape(h, w, 4)
            assert np.array_equal(words[..., :3], frame) and (words[..., 3] == 255).all() and (got[:, w * 4:] == 0x11).all()
            assert np.array_equal(stab.frame(0), frame)
            assert status(lambda: stab.frame_device(0, plane.value, w * 4 - 4)) == ARG and status(lambda: stab.frame_device(0, plane.value, w * 4 + 2)) == ARG
            assert status(lambda: stab.frame_device(1, plane.value, pitch)) == ARG
        finally:
            lib().eppm_free_device(plane)
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: stab.step(ctx=other)) == ARG     # size mismatch
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: stab.step(ctx=bat)) == ARG       # two active pairs, one slot
        assert status(lambda: stab.frame(1)) == ARG and status(lambda: stab.reset(1)) == ARG and status(lambda: stab.path(1)) == ARG
        assert status(lambda: stab.set_path(-1, first[0], first[1])) == ARG
        again = stab.path(0, counts=True)
        assert same_bits(again[0], first[0]) and same_bits(again[1], first[1]) and again[2] == first[2] == (1, 0)
        assert np.array_equal(stab.frame(0), frame)            # the refused calls changed nothing
        stab.reset()
        assert status(lambda: stab.frame(0)) == STATE
        stab.set_path(0, first[0], first[1])
        assert same_bits(stab.path(0)[1], first[1]) and status(lambda: stab.frame(0)) == STATE      # a path, but no step yet
        for bad in [dict(tau=0.0), dict(tau=float("nan")), dict(iters=0), dict(iters=9), dict(smooth=-0.5), dict(smooth=1.5)]:
            assert status(lambda: eppm_amd.Stabilizer(e, **bad)) == ARG, bad
        for size in [(0, 4), (4, 8193), (8193, 8192)]:
            assert status(lambda: eppm_amd.Stabilizer(None, size=size)) == ARG, size
        assert status(lambda: eppm_amd.Stabilizer(None, size=(4, 4), slots=0)) == ARG
        with pytest.raises(eppm_amd.EppmError):
            eppm_amd.Stabilizer(None)                          # no context and no size
    finally:
        stab.close(); e.close(); other.close(); bat.close()


# ---- 5. end to end ----

def smooth_jitter_clip(h, w, offsets, seed=61):
    """a static band-limited scene seen through a window that moves by integer offsets"""
    rng = np.random.default_rng(seed)
    pad = 16
    scene = np.rint(band_limited(rng, h + 2 * pad, w + 2 * pad, 2.0, 40, 215)).astype(np.uint8)
    return [scene[pad + oy:pad + oy + h, pad + ox:pad + ox + w].copy() for ox, oy in offsets]


def motion(frames, border=16):
    """mean absolute difference between consecutive frames, the border left out"""
    inner = [f[border:-border, border:-border].astype(np.float64) for f in frames]
    return float(np.mean([np.abs(a - b).mean() for a, b in zip(inner, inner[1:])]))


def test_sequences_agree_and_pass_through():
    import eppm_amd
    h, w = 96, 128
    clips = [moving_clip(h, w, n, seed=70 + n) for n in (2, 3, 4)]
    single = [eppm_amd.stabilize_sequence(c, masks=True) for c in clips]
    many = eppm_amd.stabilize_sequences(clips, slots=2, masks=True)
    assert [len(m[0]) for m in many] == [2, 3, 4] and [len(m[1]) for m in many] == [1, 2, 3]
    for k, (a, b) in enumerate(zip(single, many)):
        for j, (x, y) in enumerate(zip(a[0], b[0])):
            assert np.array_equal(x, y), f"clip {k} frame {j}"
        for j, (x, y) in enumerate(zip(a[1], b[1])):
            assert np.array_equal(x, y), f"clip {k} mask {j}"
        for j, (x, y) in enumerate(zip(a[2], b[2])):
            assert same_model(x, y), f"clip {k} model {j}"
    assert np.array_equal(single[2][0][0], clips[2][0])
    through = eppm_amd.stabilize_sequence(clips[2], smooth=0.0)
    assert len(through) == 4
    for j, (x, y) in enumerate(zip(through, clips[2])):
        assert np.array_equal(x, y), f"smooth = 0, frame {j}"


def test_stabilize_sequence_steadies_a_jittering_clip():
    """5 frames of 256x192, a static scene under integer camera jitter, smooth = 1.  Only asserted: the mean absolute difference between
    consecutive output frames (interior) is below the input clip's.  The host forms on the true flows give 0 (tripod lock is exact)."""
    import eppm_amd
    frames = smooth_jitter_clip(192, 256, OFFSETS)
    out, masks, models = eppm_amd.stabilize_sequence(frames, smooth=1.0, masks=True)
    assert len(out) == 5 and np.array_equal(out[0], frames[0])
    before, after = motion(frames), motion(out)
    print(f"input {before:.4f}, stabilised {after:.4f}, ratio {after / before:.4f}; models", [np.round(m["p"], 4).tolist() for m in models])
    assert after < before


def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_the_cli_equals_stabilize_sequence(tmp_path):
    import eppm_amd
    from eppm_amd import io
    clip = moving_clip(96, 128, 4, seed=74)
    want = eppm_amd.stabilize_sequence(clip, smooth=0.5)
    names = []
    for j, f in enumerate(clip):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--smooth", "0.5"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j, w in enumerate(want):
        assert np.array_equal(io.load_ppm(f"{prefix}_st_{j:04d}.ppm"), w), f"CLI frame {j}"
    assert subprocess.run([exe, "--stabilize", names[0], names[1]], capture_output=True).returncode == 2          # the stabiliser walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--smooth", "2"], capture_output=True).returncode == 2
