"""GPU tests of scene-cut detection: the kernels against the numpy restatement in every integer on cutdet_cases() in
both libraries, the context and batch forms, call order and arguments, and auto_cut end to end -- a clip of three shots comes out as the
three shots processed one by one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from cutdet_tol_child import mismatches
from test_cutdet_cpu import FIELDS, LIMIT_SIZES, SIZES, cutdet_cases, cutdet_limit_cases, differences
from test_stabilize_cpu import band_limited, moving_clip

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


def record(stats):
    return {k: stats[k] for k in FIELDS}


# ---- 1. the kernels equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_restatement(size):
    """every case through eppm_cutdet_step_frames + eppm_cutdet_get / eppm_cutdet_cuts, twice: every integer of the record is the
    restatement's (which tests/test_cutdet_cpu.py holds equal to the host form)"""
    cases = [c for c in cutdet_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """thin frames 8192 long: 256 and 512 slabs under the finish kernel's 64 lanes, taps at coordinate 8191, 32 KiB image rows under a
    pitch of (w + 8) words"""
    cases = [c for c in cutdet_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) >= 3
    bad = mismatches(cases)
    assert not bad, bad


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cutdet_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cutdet_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context form ----

def test_context_form_equals_the_host_form_and_leaves_the_flows_alone():
    import eppm_amd
    from eppm_amd import io
    h, w = 96, 128
    noisy = moving_clip(h, w, 3, seed=21)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    det = eppm_amd.CutDetector(e, residual_max=6.0)
    e.enable_stage_timing(True)
    try:
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            det.step()
            want = io.cutdet_host(noisy[k - 1], noisy[k], bu, bv, o1, o2, residual_max=6.0)
            got = det.stats(0)
            assert not differences(want, got), f"record after step {k}"
            assert got["n"] == h * w and sum(got["c1"]) == h * w and sum(got["c2"]) == h * w and got["cut"] == 0 and det.cuts() == [False]
            assert got["n_tracked"] > h * w // 2                   # consecutive frames of one shot
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a detector attached differ"
        assert "cutdet" in [n for n, _ in e.stage_times()]
    finally:
        det.close(); e.close(); plain.close()


# ---- 3. batch ----

def test_batch_slots_equal_single_pair_detectors():
    import eppm_amd
    h, w = 157, 211
    A, B, Cc, D = [moving_clip(h, w, 5, seed=s) for s in (31, 32, 33, 34)]
    # per slot the frames it sees: slot 1 crosses a cut at step 3
    seen = [[A[k] for k in range(5)], [B[0], B[1], B[2], Cc[0], Cc[1]], [D[k] for k in range(4)]]

    def walk(frames):
        """a single-pair context's detector over the slot's frames: the record after every step"""
        e = eppm_amd.EPPM(); e.init(h, w)
        d = eppm_amd.CutDetector(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1], frames[k])
                e.compute_flow_bidirectional_device()
                d.step()
                out.append(record(d.stats(0)))
        finally:
            d.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    det = eppm_amd.CutDetector(bat)
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0], s[1]) for s in seen])
            else:
                bat.push_frames([s[t] for s in seen])
            bat.compute_flow_bidirectional_device()
            det.step()
            for k in range(3):
                assert record(det.stats(k)) == want[k][t - 1], f"slot {k} after step {t}"
            assert det.cuts() == [False, t == 3, False], f"verdicts after step {t}"
        kept = record(det.stats(2))
        # one step with two active pairs: slot 2 is not covered
        bat.set_data([(seen[0][3], seen[0][4]), (seen[1][3], seen[1][4])])
        bat.compute_flow_bidirectional_device()
        det.step()
        for k in range(2):
            assert record(det.stats(k)) == want[k][3], f"slot {k} after the two-pair step"
        assert record(det.stats(2)) == kept == want[2][2]
        assert det.cuts() == [False, False] and det.cuts(3) == [False, False, False]
    finally:
        det.close(); bat.close()


# ---- 4. call order and arguments ----

def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    noisy = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    det = eppm_amd.CutDetector(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        assert status(lambda: det.stats(0)) == STATE           # a slot without a step ...
        assert det.cuts() == [False]                           # ... reports no cut
        assert status(det.step) == STATE                       # before any bidirectional call
        e.compute_flow()
        assert status(det.step) == STATE                       # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(det.step) == STATE                       # a compute_begin is pending
        e.compute_flow_end()
        assert status(det.step) == STATE                       # ... and it was forward-only
        assert status(lambda: det.stats(0)) == STATE           # the refused steps left no record
        e.compute_flow_bidirectional()
        det.step()
        first = det.stats(0)
        assert first["stepped"] == 1 and first["n"] == h * w
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: det.step(ctx=other)) == ARG      # size mismatch
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: det.step(ctx=bat)) == ARG        # two active pairs, one slot
        assert status(lambda: det.stats(1)) == ARG and status(lambda: det.stats(-1)) == ARG
        assert status(lambda: det.cuts(2)) == ARG and status(lambda: det.cuts(0)) == ARG
        assert status(lambda: det.step_frames(1, 1, 1, w * 4, 1, 1, 1)) == ARG             # slot out of range: nothing is launched
        assert status(lambda: det.step_frames(0, 1, 1, w * 4 - 4, 1, 1, 1)) == ARG         # bad pitch
        assert status(lambda: det.step_frames(0, 1, 1, w * 4, 0, 1, 1)) == ARG             # a NULL plane
        assert det.stats(0) == first and det.cuts() == [bool(first["cut"])]               # the refused calls changed nothing
        for bad in [dict(lost_permille=-1), dict(lost_permille=1001), dict(residual_max=float("nan")), dict(residual_max=256.0),
                    dict(residual_max=float("inf"))]:
            assert status(lambda: eppm_amd.CutDetector(e, **bad)) == ARG, bad
        for size in [(0, 4), (4, 8193), (8193, 8192)]:
            assert status(lambda: eppm_amd.CutDetector(None, size=size)) == ARG, size
        assert status(lambda: eppm_amd.CutDetector(None, size=(4, 4), slots=0)) == ARG
        with pytest.raises(eppm_amd.EppmError):
            eppm_amd.CutDetector(None)                         # no context and no size
    finally:
        det.close(); e.close(); other.close(); bat.close()


# ---- 5. end to end ----

H, W = 96, 128


def bright_clip(h, w, nframes, seed):
    """moving_clip with a brighter palette: the background is band_limited(..., 90, 255)"""
    rng = np.random.default_rng(seed)
    bg_v, sq_v, sq, sigma = (2, 1), (-1, 2), 24, 5.0
    pad = nframes * 2
    canvas = band_limited(rng, h + 2 * pad, w + 2 * pad, 2.0, 90, 255)
    tex = band_limited(rng, sq, sq, 1.2, 30, 225)
    frames = []
    for k in range(nframes):
        f = canvas[pad - k * bg_v[1]: pad - k * bg_v[1] + h, pad - k * bg_v[0]: pad - k * bg_v[0] + w].copy()
        sx, sy = w // 2 + k * sq_v[0], h // 4 + k * sq_v[1]
        f[sy:sy + sq, sx:sx + sq] = tex
        frames.append(np.clip(np.rint(np.rint(f) + rng.normal(0, sigma, f.shape)), 0, 255).astype(np.uint8))
    return frames


@functools.lru_cache(maxsize=None)
def shots():
    """A (4 frames), B (3), D (3, brighter): three shots; read-only"""
    out = (moving_clip(H, W, 4, seed=31), moving_clip(H, W, 3, seed=32), bright_clip(H, W, 3, 34))
    for s in out:
        for f in s:
            f.setflags(write=False)
    return out


def film():
    a, b, d = shots()
    return a + b + d


CUTS = [k in (3, 6) for k in range(9)]          # pairs 3 (A3 -> B0) and 6 (B2 -> D0) cross a cut


def test_detect_cuts_finds_the_two_cuts():
    import eppm_amd
    cuts, stats = eppm_amd.detect_cuts(film())
    for k, s in enumerate(stats):
        print(f"pair {k}: lost share of image 1 {1 - s['c1'][0] / s['n']:.4f}, of image 2 {1 - s['n_tracked'] / s['n']:.4f}, "
              f"mean residual {s['sad'] / max(s['n_tracked'], 1):.3f}, cut {s['cut']}")
    assert cuts == CUTS and [bool(s["cut"]) for s in stats] == CUTS


def test_denoise_sequence_with_auto_cut_is_the_shots_one_by_one():
    import eppm_amd
    got = eppm_amd.denoise_sequence(film(), auto_cut=True)
    want = [f for s in shots() for f in eppm_amd.denoise_sequence(s)]
    assert len(got) == len(want) == 10
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"frame {k}"


def test_stabilize_sequence_with_auto_cut_is_the_shots_one_by_one():
    import eppm_amd
    got = eppm_amd.stabilize_sequence(film(), auto_cut=True)
    want = [f for s in shots() for f in eppm_amd.stabilize_sequence(s)]
    assert len(got) == len(want) == 10
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"frame {k}"
    # what the feature is for: without it the first cut's model stays in the camera path
    blind = eppm_amd.stabilize_sequence(film())
    assert all(np.array_equal(a, b) for a, b in zip(blind[:4], want[:4]))
    assert not any(np.array_equal(a, b) for a, b in zip(blind[4:], want[4:]))


def test_flow_sequence_with_auto_cut_keeps_the_shots_flows():
    import eppm_amd
    flows, cuts = eppm_amd.flow_sequence(film(), auto_cut=True)
    assert cuts == CUTS and len(flows) == 9
    kept = [f for f, c in zip(flows, cuts) if not c]
    want = [f for s in shots() for f in eppm_amd.flow_sequence(s)]
    assert len(kept) == len(want) == 7
    for k, (a, b) in enumerate(zip(kept, want)):
        assert len(a) == 2 and np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8)) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)), k


def test_batch_sequences_with_auto_cut_agree_with_the_single_forms():
    import eppm_amd
    a, b, d = shots()
    clips = [a + b, d + a, b + d]
    flows, cuts = eppm_amd.flow_sequences(clips, slots=2, auto_cut=True)
    frames = eppm_amd.denoise_sequences(clips, slots=2, auto_cut=True)
    for k, clip in enumerate(clips):
        f1, c1 = eppm_amd.flow_sequence(clip, auto_cut=True)
        assert cuts[k] == c1 and sum(c1) == 1, f"clip {k}: {cuts[k]} / {c1}"
        for j, (x, y) in enumerate(zip(flows[k], f1)):
            if not c1[j]:
                assert np.array_equal(x[0].view(np.uint8), y[0].view(np.uint8)) and np.array_equal(x[1].view(np.uint8), y[1].view(np.uint8)), (k, j)
        one = eppm_amd.denoise_sequence(clip, auto_cut=True)
        assert len(frames[k]) == len(one) == len(clip)
        for j, (x, y) in enumerate(zip(frames[k], one)):
            assert np.array_equal(x, y), f"clip {k} frame {j}"


# ---- 6. the CLI ----

def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_the_cli_equals_denoise_sequence_with_auto_cut(tmp_path):
    import eppm_amd
    from eppm_amd import io
    a, b, _ = shots()
    clip = a[1:] + b
    want = eppm_amd.denoise_sequence(clip, auto_cut=True)
    cuts, stats = eppm_amd.detect_cuts(clip)
    assert cuts == [False, False, True, False, False]
    names = []
    for j, f in enumerate(clip):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--denoise", "--auto-cut"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j, w in enumerate(want):
        assert np.array_equal(io.load_ppm(f"{prefix}_dn_{j:04d}.ppm"), w), f"CLI frame {j}"
    lines = [[int(x) for x in ln.split()] for ln in open(f"{prefix}_cuts.txt").read().splitlines()]
    assert [ln[0] for ln in lines] == list(range(5)) and [bool(ln[1]) for ln in lines] == cuts
    for ln, s in zip(lines, stats):
        assert ln[2:] == [s["n"], *s["c1"], *s["c2"], s["n_tracked"], s["sad"]]
    # alone, with another threshold: nothing is a cut at 1000
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--cut-lost", "1000"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert [ln.split()[1] for ln in open(f"{prefix}_cuts.txt").read().splitlines()] == ["0"] * 5
    assert subprocess.run([exe, "--auto-cut", names[0], names[1]], capture_output=True).returncode == 2          # the detector walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--cut-lost", "1001"], capture_output=True).returncode == 2
