"""GPU tests of the motion-compensated temporal filter: the kernel against the host form / the numpy restatement
bit for bit on tfilter_cases(), the context and batch forms, call order and memory, the tolerance library, and the end-to-end helpers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_tfilter_cpu import LIMIT_SIZES, SIZES, tfilter_limit_cases, host_filter, moving_clip, psnr, same_bits, tfilter_cases
from tfilter_tol_child import mismatches

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


# ---- 1. the kernel equals the host form ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernel_equals_the_host_form(size):
    """every case through set_state + eppm_tfilter_step_frames + get_state / get, twice: state and bytes bit for bit the restatement's
    (which tests/test_tfilter_cpu.py holds equal to eppm_tfilter_step_host)"""
    from eppm_amd import io
    cases = [c for c in tfilter_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad
    c = cases[1]                                  # and against the host form directly
    got, rgb = io.tfilter_step_host(c["acc"], c["img2"], c["bu"], c["bv"], c["occ"], c["thresh"], c["n_max"], c["cut"])
    assert same_bits(got, c["want_acc"]) and np.array_equal(rgb, c["want_rgb"])


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernel_equals_the_host_form_at_the_size_limit(size):
    """thin frames 8192 long: taps at coordinate 8191, vectors that leave the frame by less than a pixel at both ends, image planes under
    a pitch larger than 4 * w"""
    cases = [c for c in tfilter_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) >= 3
    bad = mismatches(cases)
    assert not bad, bad


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tfilter_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 2. the context form ----

def test_context_form_equals_the_host_form_and_leaves_the_flows_alone():
    import eppm_amd
    from eppm_amd import io
    h, w = 192, 256
    _, noisy, _, _ = moving_clip(h, w, 3, seed=21)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    flt = eppm_amd.TemporalFilter(e)
    e.enable_stage_timing(True)
    acc = None
    try:
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            flt.step()
            if acc is None:
                acc = io.tfilter_seed_host(noisy[0])          # the empty-slot rule
            acc, rgb = io.tfilter_step_host(acc, noisy[k], bu, bv, o2)
            assert same_bits(flt.state(0), acc), f"state after step {k}"
            assert np.array_equal(flt.frame(0), rgb), f"frame after step {k}"
            assert (acc[..., 3] >= 2).mean() > 0.1             # the step blended: not resets alone
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the flows with a filter attached differ"
        assert "tfilter_step" in [n for n, _ in e.stage_times()]
    finally:
        flt.close(); e.close(); plain.close()


# ---- 3. batch ----

def test_batch_slots_equal_single_pair_filters():
    import eppm_amd
    h, w = 157, 211
    A, B, Cc, D = [moving_clip(h, w, 5, seed=s)[1] for s in (31, 32, 33, 34)]
    # per slot: the frames it sees and whether the frame starts another clip
    seen = [[(A[k], False) for k in range(5)],
            [(B[0], False), (B[1], False), (B[2], False), (Cc[0], True), (Cc[1], False)],
            [(D[k], False) for k in range(4)]]

    def walk(frames):
        """a single-pair context's filter over the slot's frames: [(state, frame)] after every step"""
        e = eppm_amd.EPPM(); e.init(h, w)
        f = eppm_amd.TemporalFilter(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1][0], frames[k][0])
                e.compute_flow_bidirectional_device()
                f.step([frames[k][1]])
                out.append((f.state(0), f.frame(0)))
        finally:
            f.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    flt = eppm_amd.TemporalFilter(bat)
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0][0], s[1][0]) for s in seen])
            else:
                bat.push_frames([s[t][0] for s in seen], [s[t][1] for s in seen])
            bat.compute_flow_bidirectional_device()
            flt.step([s[t][1] for s in seen] if t == 3 else None)
            for k in range(3):
                assert same_bits(flt.state(k), want[k][t - 1][0]), f"slot {k} state after step {t}"
                assert np.array_equal(flt.frame(k), want[k][t - 1][1]), f"slot {k} frame after step {t}"
        assert (flt.state(1)[..., 3] == 1).all() and np.array_equal(flt.frame(1), Cc[0])          # the cut left the new clip's seed
        assert len(flt.frames()) == 3
        kept = flt.state(2).copy()
        # one step with two active pairs: slot 2 is not covered
        bat.set_data([(seen[0][3][0], seen[0][4][0]), (seen[1][3][0], seen[1][4][0])])
        bat.compute_flow_bidirectional_device()
        flt.step()
        for k in range(2):
            assert same_bits(flt.state(k), want[k][3][0]), f"slot {k} state after the two-pair step"
            assert np.array_equal(flt.frame(k), want[k][3][1])
        assert same_bits(flt.state(2), kept) and same_bits(kept, want[2][2][0]) and np.array_equal(flt.frame(2), want[2][2][1])
    finally:
        flt.close(); bat.close()


# ---- 4. state and memory ----

def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    _, noisy, _, _ = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    flt = eppm_amd.TemporalFilter(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        assert status(lambda: flt.frame(0)) == STATE and status(lambda: flt.state(0)) == STATE          # an empty slot
        assert status(flt.step) == STATE                       # before any bidirectional call
        e.compute_flow()
        assert status(flt.step) == STATE                       # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(flt.step) == STATE                       # a compute_begin is pending
        e.compute_flow_end()
        assert status(flt.step) == STATE                       # ... and it was forward-only
        e.compute_flow_bidirectional()
        flt.step()
        first = flt.state(0)
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: flt.step(ctx=other)) == ARG     # size mismatch
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: flt.step(ctx=bat)) == ARG       # two active pairs, one slot
        assert status(lambda: flt.frame(1)) == ARG and status(lambda: flt.reset(1)) == ARG
        assert same_bits(flt.state(0), first)                   # the refused calls changed nothing
        flt.reset()
        assert status(lambda: flt.frame(0)) == STATE
        flt.set_state(0, first)
        assert same_bits(flt.state(0), first)                   # ... and set_state fills the slot again
    finally:
        flt.close(); e.close(); other.close(); bat.close()


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
    _, noisy, _, _ = moving_clip(h, w, 3, seed=51)
    e = eppm_amd.EPPM(); e.init(h, w); e.set_data(noisy[0], noisy[1]); e.compute_flow_bidirectional()
    f = eppm_amd.TemporalFilter(e); f.step(); f.frame(0); f.close(); e.close()          # code objects, pools
    check(lib().eppm_release_cached_memory(), "release")
    base = free_bytes()
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    e.compute_flow_bidirectional()
    m0 = free_bytes()
    e.compute_flow_bidirectional()
    assert free_bytes() == m0                      # a context without a filter: a compute allocates nothing
    plain = base - m0
    flt = eppm_amd.TemporalFilter(e)
    doc = (h * w * 36 + 255) & ~255                # eppm.h: 36 bytes per pixel and slot
    used = base - free_bytes()
    print("plain", plain, "with a filter", used, "documented", doc)
    assert plain + doc <= used <= plain + doc + (4 << 20)          # which the allocator may round up
    m1 = free_bytes()
    flt.step()
    e.push_frame(noisy[2])
    e.compute_flow_bidirectional()
    flt.step()
    flt.frame(0)
    assert free_bytes() == m1                      # steps allocate nothing, the context did not grow
    flt.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert free_bytes() == m0, "destroy returns the filter's block"
    e.close()
    check(lib().eppm_release_cached_memory(), "release")
    assert free_bytes() == base


# ---- 5. the tolerance library ----

def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tfilter_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 6. end to end ----

def test_denoise_sequence_gains_on_a_noisy_clip():
    """5 frames of 256x192, sigma 5.  Only asserted: the engine-flow output is closer to the clean frame than the noisy frame is.  The
    yardstick printed beside it is the host form on the true flows.  Measured on an MI355X: noisy 34.17 dB, engine flows 38.47 dB
    (+4.30), true flows 40.99 dB (+6.82); 93.2 % of the interior has n >= 2."""
    import eppm_amd
    h, w = 192, 256
    clean, noisy, flows, masks = moving_clip(h, w, 5, seed=61)
    out = eppm_amd.denoise_sequence(noisy)
    assert len(out) == 5 and np.array_equal(out[0], noisy[0])
    ref, _ = host_filter(noisy, flows, masks)
    before, engine, true = psnr(noisy[-1], clean[-1]), psnr(out[-1], clean[-1]), psnr(ref[-1], clean[-1])
    print(f"noisy {before:.2f} dB, engine flows {engine:.2f} dB (+{engine - before:.2f}), true flows {true:.2f} dB (+{true - before:.2f})")
    assert engine > before


# ---- 7. equivalences ----

def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_sequences_and_the_cli_equal_denoise_sequence(tmp_path):
    import eppm_amd
    from eppm_amd import io
    h, w = 96, 128
    clips = [moving_clip(h, w, n, seed=70 + n)[1] for n in (2, 3, 4)]
    single = [eppm_amd.denoise_sequence(c) for c in clips]
    many = eppm_amd.denoise_sequences(clips, slots=2)
    assert [len(m) for m in many] == [2, 3, 4]
    for k, (a, b) in enumerate(zip(single, many)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), f"clip {k} frame {j}"
    names = []
    for j, f in enumerate(clips[2]):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--denoise"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j, want in enumerate(single[2]):
        assert np.array_equal(io.load_ppm(f"{prefix}_dn_{j:04d}.ppm"), want), f"CLI frame {j}"
    assert subprocess.run([exe, "--denoise", names[0], names[1]], capture_output=True).returncode == 2          # the filter walks a clip
