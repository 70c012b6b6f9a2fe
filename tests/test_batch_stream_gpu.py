"""GPU tests of batch streaming: many clips through one batch context, a temporal prior per slot.  The exact
library is bit for bit, and the expectation is always what the single-pair paths produce (tests/test_temporal_gpu.py checks those against
the CPU oracle): the advection kernels over several slots against the host form per slot, a batch push against a batch set_data of the same
pairs, every slot's stream against a single-pair context walking the same clip, cuts against cold single-pair runs, flow_sequences against
flow_sequence per clip; then the state rules, the memory of the mode, and the tolerance library inside its envelope."""
import ctypes as C
import functools
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_bidirectional_gpu import eq
from test_temporal_cpu import PRIOR_CASES, UNKNOWN, make_clip, random_field
from test_temporal_gpu import PLANES, free_bytes, rgba_dev

pytestmark = pytest.mark.gpu

TEST_SECONDS = 300
SEEDED = ("prior1", "prior2", "nnf_init1", "nnf_init2", "cost_init1", "cost_init2")
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(autouse=True)
def time_limit():
    def on_alarm(signum, frame):
        raise TimeoutError(f"test exceeded {TEST_SECONDS} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@functools.lru_cache(maxsize=None)
def clip(h, w, seed, n, max_flow):
    return make_clip(h, w, seed, n=n, max_flow=max_flow)[0]


def mk_params(params):
    import eppm_amd
    return eppm_amd.Params(**dict(params)) if params else None


@functools.lru_cache(maxsize=None)
def single_stream(h, w, seed, n, max_flow, bidirectional=False, params=()):
    """The reference of every stream test, computed once per clip: a single-pair context in temporal mode walks the clip.  Per pair:
    (the flows, the six seeded-start planes or None for a cold pair).  Nothing may write into what this returns."""
    import eppm_amd
    frames = clip(h, w, seed, n, max_flow)
    e = eppm_amd.EPPM(params=mk_params(params))
    e.init(h, w)
    e.set_temporal(True)
    L = len(e.level_dims()) - 1
    out = []
    for t in range(n - 1):
        if t == 0:
            e.set_data(frames[0], frames[1])
        else:
            e.push_frame(frames[t + 1])
            assert e.temporal_valid()
        res = e.compute_flow_bidirectional() if bidirectional else e.compute_flow()
        out.append((res, {p: e.plane(p, L) for p in SEEDED} if t else None))
    e.close()
    return out


def cold(a, b, params=()):
    import eppm_amd
    e = eppm_amd.EPPM(params=mk_params(params))
    e.init(a, b, a.shape[0], a.shape[1])
    r = e.compute_flow()
    e.close()
    return r


def eq_flows(got, want, what):
    assert len(got) == len(want)
    for j, (x, y) in enumerate(zip(got, want)):
        eq(x, y, f"{what}: output {j}")


def batch_planes(b, k, nl=3):
    return {(n, l): b.plane(k, n, l) for l in range(nl) for n in PLANES}


# ---- 1. the advection kernels over several slots ----

@pytest.mark.parametrize("h,w,spread,unknown", PRIOR_CASES)
@pytest.mark.parametrize("backward", [False, True])
def test_prior_batch_kernels_equal_host_form_per_slot(h, w, spread, unknown, backward):
    from eppm_amd import io, stages
    rng = np.random.default_rng(h * 91 + w + int(backward))
    prevs = np.stack([random_field(rng, h, w, spread, unknown) for _ in range(3)])
    first, second = stages.temporal_prior_batch(prevs, backward, armed=[1, 0, 1], calls=2)
    for k in (0, 2):
        eq(first[k], io.temporal_prior(prevs[k], backward), f"slot {k} == eppm_temporal_prior_host")
    assert (first[1]["x"] == UNKNOWN).all() and (first[1]["y"] == UNKNOWN).all(), "an unarmed slot has no prior anywhere"
    eq(second, first, "a second call on the same planes")
    every = stages.temporal_prior_batch(prevs, backward)                  # armed = NULL: all slots
    for k in range(3):
        eq(every[k], io.temporal_prior(prevs[k], backward), f"armed NULL, slot {k}")


# ---- 2. push equals set_images ----

@pytest.mark.parametrize("h,w", [(157, 211), (192, 256)])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_batch_push_equals_set_images(h, w, device_form):
    import eppm_amd
    clips = [clip(h, w, 40 + k, 3, 8.0) for k in range(3)]
    ref = eppm_amd.EPPMBatch(h, w, 3)
    ref.set_data([(c[1], c[2]) for c in clips])
    want_planes = [batch_planes(ref, k) for k in range(3)]
    want = ref.compute_flow()
    b = eppm_amd.EPPMBatch(h, w, 3)
    b.set_data([(c[0], c[1]) for c in clips])
    b.compute_flow()                       # the slabs' scratch planes have been used, as in a stream
    if device_form:
        d = [rgba_dev(c[2]) for c in clips]
        b.push_frames_device([x.ptr.value for x in d], d[0].pitch)
        b.synchronize()
    else:
        b.push_frames([c[2] for c in clips])
    for k in range(3):
        got = batch_planes(b, k)
        for key in want_planes[k]:
            eq(got[key], want_planes[k][key], f"slot {k}: plane {key} after push")
    got = b.compute_flow()
    for k in range(3):
        eq_flows(got[k], want[k], f"slot {k} after push")
        for l in range(3):
            eq(b.plane(k, "flow", l), ref.plane(k, "flow", l), f"slot {k}: flow level {l}")
    b.close(); ref.close()


# ---- 3. streams equal single-pair streams ----

def check_streams(h, w, seeds, n, max_flow, bidirectional=False, **params):
    import eppm_amd
    params = tuple(sorted(params.items()))
    clips = [clip(h, w, s, n, max_flow) for s in seeds]
    refs = [single_stream(h, w, s, n, max_flow, bidirectional, params) for s in seeds]
    b = eppm_amd.EPPMBatch(h, w, len(seeds), params=mk_params(params))
    b.set_temporal(True)
    b.enable_stage_timing(True)
    for t in range(n - 1):
        if t == 0:
            b.set_data([(c[0], c[1]) for c in clips])
        else:
            b.push_frames([c[t + 1] for c in clips])
        b.stage_times()
        res = b.compute_flow_bidirectional() if bidirectional else b.compute_flow()
        names = [nm for nm, _ in b.stage_times()]
        # once per step, whatever the number of slots
        assert names.count("temporal_advect") == names.count("temporal_select") == int(t > 0) and names.count("patchmatch") == 1, names
        for k in range(len(seeds)):
            flows, planes = refs[k][t]
            eq_flows(res[k], flows, f"slot {k}, pair {t}")
            for p in SEEDED:
                if planes is None:
                    with pytest.raises(eppm_amd.EppmError):
                        b.plane(k, p, 2)
                else:
                    eq(b.plane(k, p, 2), planes[p], f"slot {k}, pair {t}: {p}")
    b.close()


def test_streams_three_slots_211x157():
    """level 2 is 53x40: a multiple neither of 16 nor of 256; radius 9: k_pm_cost_select_tile<9, 2>"""
    check_streams(157, 211, (11, 12, 13), 4, 8.0)


@pytest.mark.parametrize("patch_r", [17, 5])
def test_streams_two_slots_256x192_radius(patch_r):
    """k_pm_cost_select_tile<17> and the any-radius k_pm_cost_select"""
    check_streams(192, 256, (77, 78), 4, 10.0, patch_r=patch_r)


def test_streams_two_slots_256x192_six_iterations():
    check_streams(192, 256, (77, 78), 4, 10.0, num_iter=6)


def test_streams_two_slots_256x192_bidirectional():
    check_streams(192, 256, (77, 78), 4, 10.0, bidirectional=True)


def test_streams_eight_slots_1024x436():
    """eight slots take other sweep and search forms than a single pair does"""
    check_streams(436, 1024, tuple(range(1234, 1242)), 3, 20.0)


# ---- 4. cuts ----

def test_cuts_and_reset():
    import eppm_amd
    h, w = 192, 256
    X, Y, Z = clip(h, w, 21, 6, 8.0), clip(h, w, 22, 2, 8.0), clip(h, w, 23, 4, 8.0)
    sx, sz = single_stream(h, w, 21, 6, 8.0), single_stream(h, w, 23, 4, 8.0)
    b = eppm_amd.EPPMBatch(h, w, 2)
    b.set_temporal(True)

    def valid():
        return [b.temporal_valid(0), b.temporal_valid(1)]

    def seeded():
        out = []
        for k in range(2):
            try:
                b.plane(k, "prior1", 2)
                out.append(True)
            except eppm_amd.EppmError:
                out.append(False)
        return out

    assert valid() == [False, False]
    b.set_data([(X[0], X[1]), (Y[0], Y[1])])
    assert valid() == [False, False]
    r = b.compute_flow()                                                   # step 1
    assert valid() == [False, False] and seeded() == [False, False]
    eq_flows(r[0], sx[0][0], "step 1, slot 0: X's stream"); eq_flows(r[1], cold(Y[0], Y[1]), "step 1, slot 1: cold (Y0, Y1)")
    b.push_frames([X[2], Z[0]], new_clip=[0, 1])
    assert valid() == [True, False]
    r = b.compute_flow()                                                   # step 2: the pair across the cut
    assert valid() == [False, False] and seeded() == [True, False]
    eq_flows(r[0], sx[1][0], "step 2, slot 0: X's stream"); eq_flows(r[1], cold(Y[1], Z[0]), "step 2, slot 1: cold (Y1, Z0)")
    b.push_frames([X[3], Z[1]])
    assert valid() == [True, False], "the pair across a cut leaves no prior"
    r = b.compute_flow()                                                   # step 3: the new clip's first pair
    assert seeded() == [True, False]
    eq_flows(r[0], sx[2][0], "step 3, slot 0: X's stream"); eq_flows(r[1], cold(Z[0], Z[1]), "step 3, slot 1: cold (Z0, Z1)")
    eq_flows(r[1], sz[0][0], "step 3, slot 1: the first pair of Z's stream")
    b.push_frames([X[4], Z[2]], new_clip=[0, 0])
    assert valid() == [True, True]
    r = b.compute_flow()                                                   # step 4: the new clip's second pair is seeded
    assert valid() == [False, False] and seeded() == [True, True]
    eq_flows(r[0], sx[3][0], "step 4, slot 0: X's stream"); eq_flows(r[1], sz[1][0], "step 4, slot 1: seeded (Z1, Z2)")
    for p in SEEDED:
        eq(b.plane(1, p, 2), sz[1][1][p], f"step 4, slot 1: {p}")
    b.push_frames([X[5], Z[3]])
    assert valid() == [True, True]
    b.temporal_reset(0)
    assert valid() == [False, True]
    r = b.compute_flow()                                                   # step 5: slot 0 reset, slot 1 goes on
    assert seeded() == [False, True]
    eq_flows(r[0], cold(X[4], X[5]), "step 5, slot 0: cold after the reset"); eq_flows(r[1], sz[2][0], "step 5, slot 1: seeded (Z2, Z3)")
    # two pushes in a row, a reset of every slot, and set_data drop the fields
    b.push_frames([X[0], Z[0]])
    assert valid() == [True, True]
    b.push_frames([X[1], Z[1]])
    assert valid() == [False, False]
    b.compute_flow()
    b.push_frames([X[2], Z[2]])
    assert valid() == [True, True]
    b.temporal_reset()
    assert valid() == [False, False]
    b.compute_flow()
    b.push_frames([X[3], Z[3]])
    assert valid() == [True, True]
    b.set_data([(X[0], X[1]), (Y[0], Y[1])])
    assert valid() == [False, False]
    b.compute_flow()
    b.push_frames([X[2], Y[0]])
    assert valid() == [True, True]
    b.set_temporal(False)
    assert valid() == [False, False]
    b.close()


# ---- 5. flow_sequences ----

def test_flow_sequences_equal_flow_sequence_per_clip():
    import eppm_amd
    h, w = 96, 128
    clips = [clip(h, w, 60 + i, n, 5.0) for i, n in enumerate((5, 2, 3, 2, 4))]
    got = eppm_amd.flow_sequences(clips, slots=2)
    assert [len(g) for g in got] == [4, 1, 2, 1, 3]
    for i, c in enumerate(clips):
        want = eppm_amd.flow_sequence(c)
        for k, (g, x) in enumerate(zip(got[i], want)):
            eq_flows(g, x, f"clip {i}, pair {k}")
    one = eppm_amd.flow_sequences(clips[2:3], slots=8, bidirectional=True)      # more slots than clips
    want = eppm_amd.flow_sequence(clips[2], bidirectional=True)
    for k in range(2):
        eq_flows(one[0][k], want[k], f"one clip, bidirectional, pair {k}")


# ---- 6. state, and off means off ----

def test_state_errors_and_begin_end():
    import eppm_amd
    L = eppm_amd.lib()
    h, w = 96, 128
    seeds = (5, 6)
    clips = [clip(h, w, s, 4, 4.0) for s in seeds]
    refs = [single_stream(h, w, s, 4, 4.0) for s in seeds]
    b = eppm_amd.EPPMBatch(h, w, 3)
    imgs = [np.ascontiguousarray(c[2]) for c in clips]
    dev = [rgba_dev(i) for i in imgs]
    host2, dev2 = b._ptrs(imgs), b._ptrs([d.ptr.value for d in dev])
    stride, pitch = C.c_size_t(w * 3), C.c_size_t(dev[0].pitch)
    assert L.eppm_batch_push_images(b._ctx, 2, host2, stride, None) == ERR_STATE              # no pair yet
    assert L.eppm_batch_push_images_device(b._ctx, 2, dev2, pitch, None) == ERR_STATE
    assert not b.temporal_valid(0) and not b.temporal_valid(2) and not b.temporal_valid(3) and not b.temporal_valid(-1)
    assert L.eppm_batch_temporal_reset(b._ctx, 3) == ERR_ARG and L.eppm_batch_temporal_reset(b._ctx, 2) == 0
    b.set_temporal(True)
    b.set_data([(c[0], c[1]) for c in clips])                                               # two of the three pairs are active
    for n in (1, 3):
        assert L.eppm_batch_push_images(b._ctx, n, b._ptrs(imgs + imgs), stride, None) == ERR_ARG
        assert L.eppm_batch_push_images_device(b._ctx, n, b._ptrs([d.ptr.value for d in dev + dev]), pitch, None) == ERR_ARG
    assert L.eppm_batch_push_images(b._ctx, 2, host2, C.c_size_t(w * 3 - 1), None) == ERR_ARG   # row_stride < 3 w
    assert L.eppm_batch_push_images_device(b._ctx, 2, dev2, C.c_size_t(w * 4 - 4), None) == ERR_ARG
    assert L.eppm_batch_push_images(b._ctx, 2, b._ptrs([imgs[0], 0]), stride, None) == ERR_ARG  # a NULL image
    # the stream through begin_into / end, and a push refused while a begin is pending
    out = [(np.empty((h, w), np.float32), np.empty((h, w), np.float32)) for _ in range(2)]
    for t in range(3):
        if t:
            b.push_frames([c[t + 1] for c in clips])
        b.compute_flow_begin(out)
        assert L.eppm_batch_push_images(b._ctx, 2, host2, stride, None) == ERR_STATE
        assert L.eppm_batch_push_images_device(b._ctx, 2, dev2, pitch, None) == ERR_STATE
        res = b.compute_flow_end(out)
        for k in range(2):
            eq_flows(res[k], refs[k][t][0], f"begin / end, slot {k}, pair {t}")
    b.close()
    # a context of one pair made by eppm_create_batch takes the batch calls; the single-pair calls keep refusing a batch (test_temporal_gpu)
    one = eppm_amd.EPPMBatch(h, w, 1)
    one.set_temporal(True)
    one.set_data([(clips[0][0], clips[0][1])])
    eq_flows(one.compute_flow()[0], refs[0][0][0], "npairs = 1, pair 0")
    one.push_frames([clips[0][2]])
    assert one.temporal_valid(0)
    eq_flows(one.compute_flow()[0], refs[0][1][0], "npairs = 1, pair 1")
    one.close()


def test_batch_off_means_off_and_memory():
    import eppm_amd
    h, w, n = 436, 1024, 8
    frames = clip(h, w, 1234, 3, 20.0)
    pairs = [(frames[0], frames[1])] * n
    eppm_amd.lib().eppm_release_cached_memory()
    base = free_bytes()
    b = eppm_amd.EPPMBatch(h, w, n)
    b.set_data(pairs)
    want = b.compute_flow()
    m0 = free_bytes()
    got = b.compute_flow()                         # never enabled: a compute allocates nothing
    assert free_bytes() == m0
    plain = base - m0
    b.set_temporal(True)
    b.set_temporal(False)
    b.compute_flow()
    assert free_bytes() == m0, "a context that never computed in temporal mode holds what a plain one holds"
    b.set_temporal(True)
    got = b.compute_flow()                         # cold: the same flows
    for k in range(n):
        eq_flows(got[k], want[k], f"mode on, first pair, slot {k}")
    lh, lw = (h + 3) // 4, (w + 3) // 4
    r256 = lambda x: (x + 255) & ~255
    doc = n * (8 * r256(lh * lw * 4) + r256(lh * lw * 8))          # eppm.h: 40 bytes per level-L pixel and slot, planes rounded up to 256
    used = base - free_bytes()
    print("plain", plain, "with the mode on", used, "documented", doc)
    # which the allocator may round up or carve out of a block it holds already (the method of test_off_means_off)
    assert plain <= used <= plain + doc + (4 << 20)
    m1 = free_bytes()
    b.push_frames([frames[2]] * n)
    b.compute_flow()                               # a steady-state step allocates nothing
    assert free_bytes() == m1
    b.close()
    eppm_amd.lib().eppm_release_cached_memory()
    assert free_bytes() == base, "close() returns the temporal planes"


# ---- 7. the tolerance library ----

TOL_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %r)
import conftest                                   # (selects the test library: overridden below, before anything is loaded)
import eppm_amd
eppm_amd.select_library(sys.argv[1])
from test_temporal_cpu import make_clip
out = {"version": eppm_amd.lib().eppm_version().decode()}
same = lambda a, b: bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
for name, (h, w, seeds, n, mf) in {"clip1024": (436, 1024, range(1234, 1242), 3, 20.0), "clip256": (192, 256, (77, 78), 4, 10.0)}.items():
    clips = [make_clip(h, w, s, n=n, max_flow=mf)[0] for s in seeds]
    flows = eppm_amd.flow_sequences(clips, slots=len(clips), bidirectional=True)
    np.savez(os.path.join(sys.argv[2], name + ".npz"),
             **{"s%%d_f%%d_%%d" %% (s, k, j): flows[s][k][j] for s in range(len(clips)) for k in range(n - 1) for j in range(4)})
    # the library's own single-pair stream of every slot's clip
    out[name] = [[all(same(flows[s][k][j], x[j]) for j in range(6)) for k, x in enumerate(eppm_amd.flow_sequence(c, bidirectional=True))]
                 for s, c in enumerate(clips)]
    # the cold batch against the cold single pair in this library
    b = eppm_amd.EPPMBatch(h, w, len(clips)); b.set_data([(c[0], c[1]) for c in clips]); r = b.compute_flow(); b.close()
    cold = []
    for s, c in enumerate(clips):
        e = eppm_amd.EPPM(); e.init(c[0], c[1], h, w); u, v = e.compute_flow(); e.close()
        cold.append(same(r[s][0], u) and same(r[s][1], v))
    out[name + "_cold"] = cold
print(json.dumps(out))
""" % os.path.join(ROOT, "tests")

TOL_SLOTS = {"clip1024": (8, 3), "clip256": (2, 4)}


def test_tolerance_library_batch_streams_inside_the_envelope(tmp_path):
    """The streams of test 3 at 256x192 and 1024x436 in the tolerance library, each slot against the exact library's flows of the same
    slot with the two bounds of test_temporal_gpu.py::test_tolerance_library_stream_inside_the_envelope (section 9.4's synthetic-pair
    envelope: mean EPE <= 3e-2 px, <= 1e-3 of the pixels off by more than 1 px).  In both libraries every slot's flows, masks included,
    equal the library's own single-pair stream of the slot's clip bit for bit (a batch is the same arithmetic per pair)."""
    res = {}
    for variant in ("", "tol"):
        d = tmp_path / (variant or "exact")
        d.mkdir()
        p = subprocess.run([sys.executable, "-c", TOL_CHILD, variant, str(d)], capture_output=True, text=True, timeout=280, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        res[variant] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in res["tol"]["version"] and "tolerance" not in res[""]["version"]
    for name, (slots, n) in TOL_SLOTS.items():
        print(name, "slots equal the library's own single-pair stream: exact", res[""][name], "tolerance", res["tol"][name],
              "cold batch == cold single pair: exact", res[""][name + "_cold"], "tolerance", res["tol"][name + "_cold"])
        x, t = np.load(tmp_path / "exact" / (name + ".npz")), np.load(tmp_path / "tol" / (name + ".npz"))
        for s in range(slots):
            for k in range(n - 1):
                for j in (0, 2):
                    d = np.sqrt((x[f"s{s}_f{k}_{j}"] - t[f"s{s}_f{k}_{j}"]) ** 2 + (x[f"s{s}_f{k}_{j + 1}"] - t[f"s{s}_f{k}_{j + 1}"]) ** 2)
                    epe, off = float(d.mean()), float((d > 1.0).mean())
                    print(name, "slot", s, "pair", k, "backward" if j else "forward", "EPE", epe, "off by > 1 px", off)
                    assert epe <= 3e-2 and off <= 1e-3, (name, s, k, j, epe, off)
        for variant in ("", "tol"):
            assert all(all(row) for row in res[variant][name]), (variant, name, res[variant][name])
            assert all(res[variant][name + "_cold"]), (variant, name, res[variant][name + "_cold"])
