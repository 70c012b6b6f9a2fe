"""GPU tests of background plates: the kernels against the numpy restatement (which tests/test_plate_cpu.py holds
equal to the host forms) in every bit on plate_cases(), slot independence, the context and batch forms against the host forms fed with
the context's own planes, errors, a context without a plate, the tolerance library, and the end-to-end helpers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_plate_cpu import F, IDENT, LIMIT_IDS, LIMIT_SIZES, SIZES, plate_limit_cases, differences, host_case, np_advance, np_coverage, np_word, plate_cases, same_bits
from test_stabilize_cpu import band_limited, moving_clip
from plate_tol_child import case_params, case_planes, device_case, device_differences, free_planes, from_device, mismatches, to_device

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 3


def status(call):
    """the status of a failing call of the Python layer (EppmError: '<what>: status N: ...')"""
    import eppm_amd
    with pytest.raises(eppm_amd.EppmError) as e:
        call()
    return int(str(e.value).split("status ")[1].split(":")[0])


# ---- the kernels equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_kernels_equal_the_restatement(size):
    """every case through reset / set_state + eppm_plate_step_frames + get_state + get_path + eppm_plate_render_frames + get, twice in a
    row on one plate: the second step runs the non-empty branch and the in-place update"""
    cases = [c for c in plate_cases() if (c["w"], c["h"]) == SIZES[size]]
    bad = mismatches(cases)
    assert not bad, (len(bad), bad[:3])
    c = cases[len(cases) // 2]                    # and the host forms directly
    assert not differences(c, *host_case(c))


def test_slots_are_independent():
    """eight slots of one plate hold eight different cases; a slot keeps what it has while the others are stepped, loaded and reset"""
    import eppm_amd
    w, h = 65, 17
    common = dict(mx=3, my=2, grow=1, accept=False, thresh=40.0, n_max=64, min_count=2)
    pool = [c for c in plate_cases() if (c["w"], c["h"], c["mx"], c["my"]) == (w, h, 3, 2) and c["pname"] in ("identity", "int", "sub", "sub2", "rotzoom")]
    picked = []
    for c in pool:
        d = {k: v for k, v in c.items() if k != "want"}
        d.update(common, name=c["name"] + "_common")
        picked.append(d)
    assert len(picked) >= 10
    first, second = picked[:8], picked[2:10]
    pl = eppm_amd.BackgroundPlate(None, size=(h, w), slots=8, **case_params(picked[0]))
    planes = {id(c): case_planes(c) for c in picked}
    try:
        res = [device_case(c, pl, slot, planes[id(c)]) for slot, c in enumerate(first)]
        for slot, c in enumerate(first):
            assert not device_differences(c, res[slot]), (slot, c["name"])
        held = [(pl.state(s), pl.path(s)) for s in range(8)]
        for slot in (1, 3, 6):                     # three slots take other cases, one is reset: the rest keep theirs
            assert not device_differences(second[slot], device_case(second[slot], pl, slot, planes[id(second[slot])])), slot
        pl.reset(4)
        assert status(lambda: pl.state(4)) == STATE and status(lambda: pl.plate(4)) == STATE
        assert pl.path(4).tolist() == list(IDENT)
        for slot in (0, 2, 5, 7):
            st, path = pl.state(slot), pl.path(slot)
            assert same_bits(st, held[slot][0]) and same_bits(path, held[slot][1]), slot
            assert same_bits(st, res[slot][1][0])
    finally:
        pl.close()
        for p in planes.values():
            free_planes(p)


@pytest.mark.parametrize("size", range(len(LIMIT_SIZES)), ids=LIMIT_IDS)
def test_kernels_equal_the_restatement_at_the_size_limit(size):
    """frames and canvases 8192 long, with no margin along the long side, with a margin across it, and with margins (3, 2) around a frame
    that leaves them room: canvas taps at coordinate 8191, images and render output under a pitch larger than 4 * w"""
    bad = mismatches(plate_limit_cases(size))
    assert not bad, bad


@pytest.mark.parametrize("half", [0, 3], ids=["wide", "tall"])
def test_tolerance_library_at_the_size_limit(half):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plate_tol_child.py"), "limit", str(half)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_tolerance_library_runs_the_same_kernels():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plate_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


# ---- the context form ----

class HostPlate:
    """the host forms along a clip, fed with a context's planes: what a slot of a BackgroundPlate must hold"""

    def __init__(self, h, w, **params):
        self.p = dict(tau=1.0, iters=3, margin_x=0, margin_y=0, grow=2, accept_invalid=0, thresh=40.0, n_max=64, min_count=2)
        self.p.update(params)
        self.h, self.w = h, w
        self.path = np.array(IDENT)
        self.st = np.zeros((h + 2 * self.p["margin_y"], w + 2 * self.p["margin_x"], 4), F)

    def step(self, img1, u, v, o1, cut=False):
        from eppm_amd import io
        p = self.p
        m = (p["margin_x"], p["margin_y"])
        model, self.mask = io.gmotion_fit_host(u, v, o1, p["tau"], p["iters"])
        self.used = self.path.copy()
        fwd, inv, ok = io.plate_forms_host(self.path)
        self.blocked = io.plate_block_host(self.mask, p["grow"], p["accept_invalid"])
        if ok:
            self.st = io.plate_accumulate_host(self.st, fwd, img1, self.blocked, margins=m, thresh=p["thresh"], n_max=p["n_max"])
        self.render = io.plate_render_host(self.st, inv, ok, img1, self.blocked, margins=m, min_count=p["min_count"])
        self.path = np.array(IDENT) if cut else np_advance(self.path, model["p"], model["valid"])
        self.model = model

    def same(self, pl, slot, what, ctx=None):
        assert same_bits(pl.state(slot), self.st), f"{what}: state"
        assert same_bits(pl.plate(slot), np_word(self.st[..., :3])), f"{what}: plate"
        assert same_bits(pl.coverage(slot), np_coverage(self.st)), f"{what}: coverage"
        assert same_bits(pl.mask(slot), self.mask), f"{what}: mask"
        assert same_bits(pl.path(slot), self.path), f"{what}: path"
        out, fill = pl.render(slot, ctx)
        assert same_bits(out, self.render[0]) and same_bits(fill, self.render[1]), f"{what}: render"


def clean_background(h, w, nframes, seed=11, bg_v=(2, 1)):
    """moving_clip's noise-free background and its pad: frame k shows canvas[pad - k * dy + y, pad - k * dx + x]"""
    rng = np.random.default_rng(seed)
    pad = nframes * max(abs(bg_v[0]), abs(bg_v[1]), 1)
    return np.rint(band_limited(rng, h + 2 * pad, w + 2 * pad, 2.0, 40, 215)), pad


def test_context_form_equals_the_host_forms_and_leaves_the_flows_alone():
    import eppm_amd
    h, w, n = 192, 256, 4
    params = dict(margin_x=8, margin_y=6)
    noisy = moving_clip(h, w, n)
    e, ref = eppm_amd.EPPM(), eppm_amd.EPPM()
    e.init(h, w); ref.init(h, w)
    pl = eppm_amd.BackgroundPlate(e, **params)
    host = HostPlate(h, w, **params)
    e.enable_stage_timing(True); ref.enable_stage_timing(True)
    try:
        assert (pl.ch, pl.cw) == (h + 12, w + 16)
        assert status(lambda: pl.plate(0)) == STATE and status(lambda: pl.state(0)) == STATE and status(lambda: pl.mask(0)) == STATE          # empty
        assert status(lambda: pl.render(0)) == STATE and pl.path(0).tolist() == list(IDENT)
        assert status(pl.step) == STATE                        # before any bidirectional call: outside the window
        share = []
        for k in range(1, n):
            for ctx in (e, ref):
                if k == 1:
                    ctx.set_data(noisy[0], noisy[1])
                else:
                    ctx.push_frame(noisy[k])
            u, v, bu, bv, o1, o2 = planes = e.compute_flow_bidirectional()
            pl.step()
            host.step(noisy[k - 1], u, v, o1)
            host.same(pl, 0, f"pair {k}")
            for a, b in zip(planes, ref.compute_flow_bidirectional()):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the planes with a plate attached differ"
            sx, sy = w // 2 - (k - 1), h // 4 + 2 * (k - 1)          # measured, not asserted: the square's footprint
            fill = host.render[1][sy:sy + 24, sx:sx + 24]
            share.append(float((fill == 1).mean()))
        bg, pad = clean_background(h, w, n)
        cov = pl.coverage(0) >= 1
        truth = bg[pad - 6:pad - 6 + pl.ch, pad - 8:pad - 8 + pl.cw]
        err = (pl.plate(0).astype(np.float64) - truth)[cov]
        print(f"plate vs the noise-free background over {cov.mean():.3f} of the canvas: PSNR {10 * np.log10(255 ** 2 / (err ** 2).mean()):.2f} dB "
              f"(one noisy frame: {10 * np.log10(255 ** 2 / 25.0):.2f} dB); share of the square's footprint filled per pair {share}")
        names = [nm for nm, _ in e.stage_times()]
        assert "plate_fit" in names and "plate_block" in names and "plate_accumulate" in names and "plate_render" in names
        assert "stab_fit" not in names                         # the private stabiliser's launches are the plate's stage
        # a context that creates no plate: the same stage names without the plate's, the same flow bytes (above)
        assert [nm for nm in names if not nm.startswith("plate_")] == [nm for nm, _ in ref.stage_times()]
        assert status(lambda: pl.plate(1)) == ARG and status(lambda: pl.reset(1)) == ARG and status(lambda: pl.path(1)) == ARG
        pl.reset()
        assert status(lambda: pl.plate(0)) == STATE and pl.path(0).tolist() == list(IDENT)
    finally:
        pl.close(); e.close(); ref.close()


def test_batch_form_and_a_cut():
    """three slots run clips of different seeds; a cut flag on slot 1 in the middle makes its path the identity, keeps its canvas and
    leaves the other slots alone: every slot equals its own host run after every step"""
    import eppm_amd
    h, w, n = 96, 128, 4
    clips = [moving_clip(h, w, n, seed=s) for s in (11, 12, 13)]
    e = eppm_amd.EPPMBatch(h, w, 3)
    pl = eppm_amd.BackgroundPlate(e, margin_x=4)
    hosts = [HostPlate(h, w, margin_x=4) for _ in clips]
    try:
        assert pl.nslots == 3
        for k in range(1, n):
            if k == 1:
                e.set_data([(c[0], c[1]) for c in clips])
            else:
                e.push_frames([c[k] for c in clips])
            planes = e.compute_flow_bidirectional()
            cut = [False, k == 2, False]
            before = pl.state(1) if k == 3 else None
            pl.step(cut)
            for s, (u, v, bu, bv, o1, o2) in enumerate(planes):
                hosts[s].step(clips[s][k - 1], u, v, o1, cut[s])
                hosts[s].same(pl, s, f"slot {s} pair {k}", e)
            if k == 2:
                assert pl.path(1).tolist() == list(IDENT) and pl.path(0).tolist() != list(IDENT)
                assert (pl.coverage(1) >= 1).any()             # the canvas is kept
            if k == 3:
                assert same_bits(hosts[1].used, np.array(IDENT)) and not same_bits(before, pl.state(1))
    finally:
        pl.close(); e.close()


def test_call_order_and_arguments():
    import eppm_amd
    h, w = 96, 128
    noisy = moving_clip(h, w, 2, seed=41)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    pl = eppm_amd.BackgroundPlate(e)
    other = eppm_amd.EPPM(); other.init(h, w + 4)
    bat = eppm_amd.EPPMBatch(h, w, 2)
    try:
        assert status(pl.step) == STATE                        # before any bidirectional call
        e.compute_flow()
        assert status(pl.step) == STATE                        # after a forward-only compute
        e.compute_flow_bidirectional()
        e.compute_flow_begin()
        assert status(pl.step) == STATE                        # a compute_begin is pending
        e.compute_flow_end()
        assert status(pl.step) == STATE                        # ... and it was forward-only
        e.compute_flow_bidirectional()
        pl.step()
        first = (pl.state(0), pl.render(0))
        other.set_data(np.zeros((h, w + 4, 3), np.uint8), np.zeros((h, w + 4, 3), np.uint8))
        other.compute_flow_bidirectional()
        assert status(lambda: pl.step(ctx=other)) == ARG      # other dimensions
        assert status(lambda: pl.render(0, ctx=other)) == ARG
        bat.set_data([(noisy[0], noisy[1])] * 2)
        bat.compute_flow_bidirectional()
        assert status(lambda: pl.step(ctx=bat)) == ARG        # two active pairs, one slot
        with pytest.raises(eppm_amd.EppmError):
            pl.step(cut=[False, True])
        e.compute_flow()
        assert status(lambda: pl.render(0)) == STATE           # outside the window
        assert same_bits(pl.state(0), first[0])                # the failed calls changed nothing
        e.compute_flow_bidirectional()
        again = pl.render(0)
        assert same_bits(again[0], first[1][0]) and same_bits(again[1], first[1][1])
        assert status(lambda: pl.step_frames(1, 1, w * 4, 1)) == ARG and status(lambda: pl.step_frames(0, 1, w * 4 - 1, 1)) == ARG
        assert status(lambda: pl.render_frames(0, 1, w * 4, 1, None, 1, w * 4 - 4, 1)) == ARG
        assert status(lambda: pl.set_path(3, IDENT)) == ARG and status(lambda: pl.get_device(0, 1, w * 4 - 4)) == ARG
        d = to_device(nbytes=(h + 1) * (w + 8) * 4)              # eppm_plate_get_device: the canvas words at a pitch of the caller's
        try:
            pl.get_device(0, d.value, (w + 8) * 4)
            words = from_device(d, (h + 1, w + 8, 4), np.uint8)[:h, :w]
            assert same_bits(np.ascontiguousarray(words[..., :3]), pl.plate(0)) and (words[..., 3] == 255).all()
        finally:
            free_planes([d])
        with pytest.raises(eppm_amd.EppmError):
            pl.set_state(0, np.zeros((h, w, 3), F))
        with pytest.raises(eppm_amd.EppmError):
            eppm_amd.BackgroundPlate(None)
    finally:
        pl.close(); e.close(); other.close(); bat.close()


# ---- the helpers ----

def test_helpers_agree_with_the_class_used_by_hand():
    import eppm_amd
    h, w, n = 96, 128, 4
    clips = [moving_clip(h, w, n, seed=11), moving_clip(h, w, 3, seed=12), moving_clip(h, w, n, seed=13)]
    params = dict(margin_x=6, margin_y=4)
    by_hand, removed = [], None
    for c in clips:
        e = eppm_amd.EPPM(); e.init(h, w); e.set_temporal(True)
        pl = eppm_amd.BackgroundPlate(e, **params)
        try:
            kept = []
            for k in range(len(c) - 1):
                if k == 0:
                    e.set_data(c[0], c[1])
                else:
                    e.push_frame(c[k + 1])
                e.compute_flow_bidirectional_device()
                path = pl.path(0)
                pl.step()
                kept.append((pl.mask(0), path))
            by_hand.append((pl.plate(0), pl.coverage(0)))
            if removed is None:
                removed = [pl.render_frame(0, c[k], m, p) for k, (m, p) in enumerate(kept)]
        finally:
            pl.close(); e.close()
    plate, cov = eppm_amd.background_plate(clips[0], **params)
    assert same_bits(plate, by_hand[0][0]) and same_bits(cov, by_hand[0][1])
    assert plate.shape == (h + 8, w + 12, 3) and (cov >= 1).mean() > 0.2
    frames, fills = eppm_amd.remove_objects_sequence(clips[0], **params)
    assert len(frames) == len(fills) == n
    for k, (o, f) in enumerate(removed):
        assert same_bits(frames[k], o) and same_bits(fills[k], f), k
    assert same_bits(frames[-1], clips[0][-1]) and not fills[-1].any()          # the last frame has no pair of its own
    assert any((f == 1).any() for f in fills[:-1])
    share = [float((fills[k][h // 4 + 2 * k:h // 4 + 2 * k + 24, w // 2 - k:w // 2 - k + 24] == 1).mean()) for k in range(n - 1)]
    print(f"two passes at {w}x{h}: canvas covered {(cov >= 1).mean():.3f}, share of the square's footprint filled per frame {share}")          # measured
    many = eppm_amd.background_plates(clips, slots=2, **params)
    assert len(many) == 3
    for k, (p, c) in enumerate(many):
        assert same_bits(p, by_hand[k][0]) and same_bits(c, by_hand[k][1]), k
    with pytest.raises(TypeError):
        eppm_amd.background_plate(clips[0], smooth=0.5)
    with pytest.raises(TypeError):
        eppm_amd.background_plate(clips[0], lost_permille=500)
    with pytest.raises(eppm_amd.EppmError):
        eppm_amd.background_plate(clips[0][:1])


def test_cli_writes_the_plate_and_the_frames_without_objects(tmp_path):
    """runeppm --sequence ... --plate --plate-margin MX MY --remove-objects: the files are what the helpers return"""
    import eppm_amd
    from conftest import read_ppm
    h, w, n = 96, 128, 4
    clip = moving_clip(h, w, n, seed=13)
    names = []
    for k, f in enumerate(clip):
        names.append(str(tmp_path / f"f{k}.ppm"))
        with open(names[-1], "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h) + f.tobytes())
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")
    prefix = str(tmp_path / "out")
    out = subprocess.run([exe, "--sequence", *names, "--out-prefix", prefix, "--remove-objects", "--plate-margin", "6", "4"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-1000:]
    plate, cov = eppm_amd.background_plate(clip, margin_x=6, margin_y=4)
    frames, fills = eppm_amd.remove_objects_sequence(clip, margin_x=6, margin_y=4)
    assert same_bits(read_ppm(prefix + "_plate.ppm"), plate)
    raw = open(prefix + "_plate_cov.pgm", "rb").read()
    head = b"P5\n%d %d\n255\n" % (w + 12, h + 8)
    assert raw.startswith(head) and same_bits(np.frombuffer(raw[len(head):], np.uint8).reshape(cov.shape), cov)
    for k in range(n):
        assert same_bits(read_ppm(prefix + f"_ro_{k:04d}.ppm"), frames[k]), k
    assert f"{sum(int((f == 1).sum()) for f in fills)} pixels filled" in out.stdout
    for bad in (["--plate"], ["--sequence", *names, "--out-prefix", prefix, "--plate-margin", "-1", "0"], [names[0], names[1], "--remove-objects"]):
        r = subprocess.run([exe, *bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "usage: runeppm" in r.stderr, bad
