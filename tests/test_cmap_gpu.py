"""GPU tests of the dense correspondence map: the kernels against the host forms / the numpy restatement bit for
bit on cmap_cases(), the context and batch forms, the layer and its render on the device, the tolerance library, and the end-to-end
helpers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_cmap_cpu import LIMIT_SIZES, SIZES, cmap_cases, cmap_limit_cases, host_step, np_known, np_seed
from test_tfilter_cpu import moving_clip, same_bits
from cmap_tol_child import mismatches, to_device

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


def paint_layer(h, w, seed):
    rng = np.random.default_rng(seed)
    lay = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    lay[: h // 3, :, 3] = 255
    lay[-(h // 3):, :, 3] = 0
    return lay


# ---- 5. the kernels equal the host forms ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_host_forms(size):
    """every case through set_state + eppm_cmap_step_frames + get_state + set_layer + render, twice: map and bytes bit for bit the
    restatement's (which tests/test_cmap_cpu.py holds equal to the host forms)"""
    cases = [c for c in cmap_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, bad
    c = cases[1]                                  # and against the host forms directly
    got, rgb = host_step(c)
    assert same_bits(got, c["want_map"]) and np.array_equal(rgb, c["want_rgb"])


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=[f"{w}x{h}" for w, h in LIMIT_SIZES])
def test_kernels_equal_the_host_forms_at_the_size_limit(size):
    """thin frames 8192 long: map values and taps at coordinate 8191, vectors that end on the last column / row and one ulp beyond them,
    the caller's images under a pitch larger than 4 * w"""
    cases = [c for c in cmap_limit_cases() if (c["w"], c["h"]) == LIMIT_SIZES[size]]
    assert len(cases) >= 3
    bad = mismatches(cases)
    assert not bad, bad


def test_tolerance_library_at_the_size_limit():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cmap_tol_child.py"), "limit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 6. the context form ----

def test_context_form_equals_the_host_form_and_leaves_the_flows_alone():
    import eppm_amd
    from eppm_amd import io
    h, w = 192, 256
    _, noisy, _, _ = moving_clip(h, w, 3, seed=21)
    e, plain = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); plain.init(h, w)
    cm = eppm_amd.CorrespondenceMap(e)
    e.enable_stage_timing(True)
    M = None
    try:
        assert status(lambda: cm.render(0)) == STATE and status(lambda: cm.map(0)) == STATE          # never stepped
        with pytest.raises(eppm_amd.EppmError):
            cm.age(0)
        assert status(cm.step) == STATE                        # before any bidirectional call
        for k in (1, 2):
            for ctx in (e, plain):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[2])
            u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
            cm.step()
            M = io.cmap_step_host(M, noisy[0], noisy[k], bu, bv, o2)          # M None: the empty-slot rule (the seed, image 1 the anchor)
            assert same_bits(cm.map(0), M), f"map after step {k}"
            assert np.array_equal(cm.render(0), io.cmap_render_host(M, noisy[k], None, noisy[0])), f"render after step {k}"
            assert cm.age(0) == k
            known = np_known(M[..., 0], M[..., 1])
            assert np.array_equal(cm.known(0), known)
            print(f"step {k}: {100 * known.mean():.1f} % known")
            assert known.mean() >= 0.10                        # not all lost
            for a, b in zip((u, v, bu, bv, o1, o2), plain.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the planes with a map attached differ"
        names = [n for n, _ in e.stage_times()]
        assert "cmap_step" in names and "cmap_render" in names
        assert status(lambda: cm.map(1)) == ARG and status(lambda: cm.reset(1)) == ARG and status(lambda: cm.set_layer(None, 1)) == ARG
        cm.reset()
        assert status(lambda: cm.render(0)) == STATE
    finally:
        cm.close(); e.close(); plain.close()


def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    _, noisy, _, _ = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    cm = eppm_amd.CorrespondenceMap(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        assert status(cm.step) == STATE                        # before any bidirectional call
        e.compute_flow()
        assert status(cm.step) == STATE                        # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(cm.step) == STATE                        # a compute_begin is pending
        e.compute_flow_end()
        assert status(cm.step) == STATE                        # ... and it was forward-only
        cm.set_layer(paint_layer(h, w, 3), 0)                  # allowed on an empty slot, which stays empty
        assert status(lambda: cm.render(0)) == STATE
        e.compute_flow_bidirectional()
        cm.step()
        first, shown = cm.map(0), cm.render(0)
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: cm.step(ctx=other)) == ARG      # size mismatch
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: cm.step(ctx=bat)) == ARG        # two active pairs, one slot
        assert status(lambda: cm.set_layer(np.zeros((h, w, 4), np.uint8), 1)) == ARG
        with pytest.raises(eppm_amd.EppmError):
            cm.set_layer(np.zeros((h, w, 3), np.uint8))
        with pytest.raises(eppm_amd.EppmError):
            cm.step([True, False])
        assert same_bits(cm.map(0), first) and np.array_equal(cm.render(0), shown) and cm.age(0) == 1          # the refused calls changed nothing
        cm.reset()
        assert status(lambda: cm.map(0)) == STATE
        cm.set_state(0, first, noisy[0])
        assert same_bits(cm.map(0), first) and cm.age(0) == 0          # ... and set_state fills the slot again
    finally:
        cm.close(); e.close(); other.close(); bat.close()


# ---- 7. batch ----

def test_batch_slots_equal_single_pair_maps():
    import eppm_amd
    h, w = 157, 211
    A, B, Cc, D = [moving_clip(h, w, 5, seed=s)[1] for s in (31, 32, 33, 34)]
    # per slot: the frames it sees and whether the frame starts another clip
    seen = [[(A[k], False) for k in range(5)],
            [(B[0], False), (B[1], False), (B[2], False), (Cc[0], True), (Cc[1], False)],
            [(D[k], False) for k in range(4)]]

    def walk(frames):
        """a single-pair context's map over the slot's frames: [(map, render, age)] after every step"""
        e = eppm_amd.EPPM(); e.init(h, w)
        f = eppm_amd.CorrespondenceMap(e)
        out = []
        try:
            for k in range(1, len(frames)):
                e.set_data(frames[k - 1][0], frames[k][0])
                e.compute_flow_bidirectional_device()
                f.step([frames[k][1]])
                out.append((f.map(0), f.render(0), f.age(0)))
        finally:
            f.close(); e.close()
        return out
    want = [walk(s) for s in seen]
    bat = eppm_amd.EPPMBatch(h, w, 3)
    cm = eppm_amd.CorrespondenceMap(bat)

    def same(k, t):
        assert same_bits(cm.map(k), want[k][t][0]), f"slot {k} map after step {t + 1}"
        assert np.array_equal(cm.render(k), want[k][t][1]), f"slot {k} render after step {t + 1}"
        assert cm.age(k) == want[k][t][2]
    try:
        for t in (1, 2, 3):
            if t == 1:
                bat.set_data([(s[0][0], s[1][0]) for s in seen])
            else:
                bat.push_frames([s[t][0] for s in seen], [s[t][1] for s in seen])
            bat.compute_flow_bidirectional_device()
            cm.step([s[t][1] for s in seen] if t == 3 else None)
            for k in range(3):
                same(k, t - 1)
        assert same_bits(cm.map(1), np_seed(h, w)) and cm.age(1) == 0 and np.array_equal(cm.render(1), Cc[0])          # the cut re-anchored slot 1
        assert cm.age(0) == 3 and cm.age(2) == 3
        kept = cm.map(2).copy()
        # one step with two active pairs: slot 2 is not covered
        bat.set_data([(seen[0][3][0], seen[0][4][0]), (seen[1][3][0], seen[1][4][0])])
        bat.compute_flow_bidirectional_device()
        cm.step()
        for k in range(2):
            same(k, 3)
        assert cm.age(1) == 1
        assert same_bits(cm.map(2), kept) and same_bits(kept, want[2][2][0]) and np.array_equal(cm.render(2), want[2][2][1]) and cm.age(2) == 3
    finally:
        cm.close(); bat.close()


# ---- 8. the layer and the device render ----

def test_render_device_equals_render_and_layers_stay_in_their_slots():
    import eppm_amd
    from eppm_amd import io
    from eppm_amd._lib import check, lib
    h, w = 45, 67
    cases = [c for c in cmap_cases() if (c["w"], c["h"]) == (w, h)]
    a, b = cases[1], cases[2]
    cm = eppm_amd.CorrespondenceMap(None, size=(h, w), slots=2)
    pitch = w * 4 + 64
    d_out = to_device(np.zeros((h, pitch), np.uint8))
    try:
        cm.set_state(0, a["want_map"], a["anchor"])
        cm.set_state(1, b["want_map"], b["anchor"])
        assert cm.age(0) == 0
        base = [io.cmap_render_host(c["want_map"], c["anchor"], None, c["anchor"]) for c in (a, b)]
        assert np.array_equal(cm.render(0), base[0]) and np.array_equal(cm.render(1), base[1])
        lay = paint_layer(h, w, 5)
        cm.set_layer(lay, 1)
        painted = io.cmap_render_host(b["want_map"], b["anchor"], lay)
        assert (painted != base[1]).any()
        assert np.array_equal(cm.render(1), painted)
        assert np.array_equal(cm.render(0), base[0]), "slot 1's layer shows in slot 0"
        for slot, want in ((0, base[0]), (1, painted)):
            cm.render_device(slot, d_out.value, pitch)
            check(lib().eppm_device_synchronize(), "sync")
            got = np.empty((h, pitch), np.uint8)
            check(lib().eppm_memcpy_d2h(got.ctypes.data_as(C.c_void_p), d_out, C.c_size_t(got.nbytes)), "d2h")
            words = got[:, : w * 4].reshape(h, w, 4)
            assert np.array_equal(words[..., :3], want) and (words[..., 3] == 255).all(), f"render_device, slot {slot}"
        cm.set_layer(None, 1)
        assert np.array_equal(cm.render(1), base[1])          # the default layer again
        assert status(lambda: cm.render_device(0, d_out.value, w * 4 - 4)) == ARG
    finally:
        cm.close()
        lib().eppm_free_device(d_out)


# ---- 9. the tolerance library ----

def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cmap_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- 10. end to end ----

def write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def test_propagate_layer_and_the_cli(tmp_path):
    import eppm_amd
    from eppm_amd import io
    h, w = 96, 128
    clip = moving_clip(h, w, 5, seed=81)[1]
    lay = paint_layer(h, w, 7)
    out, maps = eppm_amd.propagate_layer(clip, lay, maps=True)
    assert len(out) == len(clip) == len(maps)
    assert np.array_equal(out[0], io.cmap_render_host(np_seed(h, w), clip[0], lay)) and same_bits(maps[0], np_seed(h, w))
    assert (out[0] != clip[0]).any()
    for k in range(1, 5):                                    # every frame is the host render of its own map
        assert np.array_equal(out[k], io.cmap_render_host(maps[k], clip[k], lay)), f"frame {k}"
        assert np_known(maps[k][..., 0], maps[k][..., 1]).mean() >= 0.10
        assert (out[k] != clip[k]).any()
    # a forced cut (lost_permille 0: any lost pixel makes the first pair a cut): the frames after it are the input frames
    cut = eppm_amd.propagate_layer(clip, lay, auto_cut=True, lost_permille=0)
    assert len(cut) == len(clip) and np.array_equal(cut[0], out[0])
    for k in range(1, 5):
        assert np.array_equal(cut[k], clip[k]), f"frame {k} after the cut"
    # without a cut found, auto_cut changes nothing
    calm = eppm_amd.propagate_layer(clip, lay, auto_cut=True)
    assert all(np.array_equal(x, y) for x, y in zip(calm, out))
    with pytest.raises(TypeError):
        eppm_amd.propagate_layer(clip, lay, n_max=3)
    # many clips through one batch context
    clips = [clip[:3], moving_clip(h, w, 2, seed=82)[1], clip[:4]]
    layers = [lay, paint_layer(h, w, 8), lay]
    many = eppm_amd.propagate_layers(clips, layers, slots=2)
    assert [len(m) for m in many] == [3, 2, 4]
    for k, (c, l) in enumerate(zip(clips, layers)):
        single = eppm_amd.propagate_layer(c, l)
        for j, (x, y) in enumerate(zip(single, many[k])):
            assert np.array_equal(x, y), f"clip {k} frame {j}"
    # the CLI
    names = []
    for j, f in enumerate(clip):
        names.append(str(tmp_path / f"f{j}.ppm"))
        write_ppm(names[-1], f)
    write_ppm(str(tmp_path / "layer.ppm"), lay[..., :3])
    write_ppm(str(tmp_path / "alpha.ppm"), np.repeat(lay[..., 3:], 3, axis=2))
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    tail = ["--propagate", str(tmp_path / "layer.ppm"), str(tmp_path / "alpha.ppm")]
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, *tail], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j, want in enumerate(out):
        assert np.array_equal(io.load_ppm(f"{prefix}_pl_{j:04d}.ppm"), want), f"CLI frame {j}"
    run = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, *tail, "--cut-lost", "0"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    for j, want in enumerate(cut):
        assert np.array_equal(io.load_ppm(f"{prefix}_pl_{j:04d}.ppm"), want), f"CLI frame {j} with a cut"
    assert subprocess.run([exe, *tail, names[0], names[1]], capture_output=True).returncode == 2          # the map walks a clip
    assert subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--propagate", names[0]], capture_output=True).returncode == 2
