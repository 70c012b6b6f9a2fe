"""GPU tests of the Y'CbCr 4:2:0 frames (include/eppm_yuv.h): the two kernels against the host forms byte for byte
over every format, and the context contract: after a YUV call a context holds, bit for bit, what it holds after the RGB call on
yuv.to_rgb of the same frames -- single and batch, host and device forms, across pushes with the temporal mode on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_yuv_cpu import fmt_id, formats
from yuv_tol_child import kernel_mismatches

pytestmark = pytest.mark.gpu

PLANES = ("img1", "img2", "census1", "census2")


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("f", list(formats()), ids=fmt_id)
def test_kernels_equal_the_host_forms(f):
    """both directions, every size of yuv_tol_child.KERNEL_SIZES, pitched planes whose padding must stay poison, both store variants of
    k_yuv_to_rgba (a 16-byte aligned destination; pitch 4w + 4, also 4 bytes off) and of k_rgba_to_yuv (word stores; sample stores)"""
    bad = kernel_mismatches([f])
    assert not bad, bad


def test_tolerance_library_runs_the_same_arithmetic():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "yuv_tol_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-2000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]


def test_device_call_argument_errors():
    """a legal call, then an RGBA pitch that is no multiple of 4, an RGBA base that is none, and a pitch below the row"""
    import ctypes as C
    import eppm_amd
    from eppm_amd import yuv
    L = eppm_amd.lib()
    f = yuv.YuvFormat()
    y, uv = yuv.from_rgb(np.zeros((4, 4, 3), np.uint8)).to_device()
    ptrs, pitches = yuv._dev_args([y, uv])
    out = C.c_void_p()
    assert L.eppm_malloc_device(C.byref(out), 4 * 32) == 0
    try:
        assert L.eppm_yuv_to_rgba(C.byref(f), ptrs, pitches, out, 32, 4, 4, None) == 0
        assert L.eppm_yuv_to_rgba(C.byref(f), ptrs, pitches, out, 18, 4, 4, None) == 1 and b"pitch" in L.eppm_last_error()
        assert L.eppm_yuv_to_rgba(C.byref(f), ptrs, pitches, out.value + 2, 32, 4, 4, None) == 1
        assert L.eppm_yuv_from_rgba(C.byref(f), out, 12, ptrs, pitches, 4, 4, None) == 1
        assert L.eppm_device_synchronize() == 0
    finally:
        L.eppm_free_device(out)


# ---- 2. the context contract ----
def yuv_clip(fmt, h, w, n, seed):
    """n frames of a moving synthetic scene as YuvFrames of fmt"""
    from eppm_amd import synth, yuv
    a, b, _, _ = synth.make_pair(h, w, seed=seed, max_flow=3.0)
    c, d, _, _ = synth.make_pair(h, w, seed=seed + 1, max_flow=3.0)
    return [yuv.from_rgb(x, fmt) for x in (a, b, c, d)[:n]]


def context_state(e, flow=True):
    """every image and census plane of every level, and the flow"""
    out = {}
    for level in range(len(e.level_dims())):
        for name in PLANES:
            out[name, level] = e.plane(name, level)
    if flow:
        u, v = e.compute_flow()
        out["u"], out["v"] = u.copy(), v.copy()
        out["flow", 0] = e.plane("flow", 0)
    return out


def same_state(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]


NV12_8 = dict(layout=0, depth=8)
P010 = dict(layout=0, depth=10, msb_aligned=1)


@pytest.mark.parametrize("fmt_kw", [NV12_8, P010], ids=["nv12", "p010"])
@pytest.mark.parametrize("h,w", [(96, 128), (45, 67)])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_context_holds_what_the_rgb_call_leaves(fmt_kw, h, w, device_form):
    import eppm_amd
    from eppm_amd import yuv
    fmt = yuv.YuvFormat(**fmt_kw)
    A, B, Cc, D = yuv_clip(fmt, h, w, 4, seed=11)
    ref, e = eppm_amd.EPPM(), eppm_amd.EPPM()
    ref.init(h, w)
    e.init(h, w)
    keep = []

    def set_pair(x, y):
        if device_form:
            dx, dy = x.to_device(pitched=True), y.to_device(pitched=True)
            keep.extend([dx, dy])
            e.set_data_yuv_device(fmt, dx, dy)
        else:
            e.set_data_yuv(x, y)

    def push(x):
        if device_form:
            dx = x.to_device(pitched=True)
            keep.append(dx)
            e.push_frame_yuv_device(fmt, dx)
        else:
            e.push_frame_yuv(x)
    try:
        ref.set_data(yuv.to_rgb(A), yuv.to_rgb(B))
        set_pair(A, B)
        assert same_state(context_state(e), context_state(ref)) == []
        # two pushes with the temporal mode on: the arming and the seeded computes agree too
        for ctx in (ref, e):
            ctx.set_temporal(True)
        ref.set_data(yuv.to_rgb(A), yuv.to_rgb(B))
        set_pair(A, B)
        assert not e.temporal_valid() and not ref.temporal_valid()
        assert same_state(context_state(e), context_state(ref)) == []
        for nxt in (Cc, D):
            ref.push_frame(yuv.to_rgb(nxt))
            push(nxt)
            assert e.temporal_valid() == ref.temporal_valid() is True
            assert same_state(context_state(e), context_state(ref)) == []
    finally:
        e.close()
        ref.close()


def test_context_call_errors_are_the_rgb_calls():
    import eppm_amd
    from eppm_amd import yuv
    h, w = 16, 16
    A, B = yuv_clip(yuv.YuvFormat(), h, w, 2, seed=3)
    e = eppm_amd.EPPM()
    e.init(h, w)
    try:
        with pytest.raises(eppm_amd.EppmError, match="status 3"):           # EPPM_ERR_STATE: no pair set yet
            e.push_frame_yuv(A)
        with pytest.raises(eppm_amd.EppmError, match="frames must be"):
            e.set_data_yuv(*yuv_clip(yuv.YuvFormat(), 20, 16, 2, seed=3))
        with pytest.raises(eppm_amd.EppmError, match="one format"):
            e.set_data_yuv(A, yuv.from_rgb(yuv.to_rgb(B), depth=10))
        e.set_data_yuv(A, B)
        small = yuv_clip(yuv.YuvFormat(), 12, 16, 1, seed=3)[0].to_device()          # device planes of another size: refused like host frames
        with pytest.raises(eppm_amd.EppmError, match="frames must be"):
            e.push_frame_yuv_device(A.fmt, small)
        A.fmt.depth = 9
        with pytest.raises(eppm_amd.EppmError, match="status 1.*depth"):
            e.push_frame_yuv(A)
    finally:
        e.close()


# ---- 3. batch ----
def batch_planes(bat, k):
    return {(name, level): bat.plane(k, name, level) for level in range(len(bat.level_dims())) for name in PLANES}


@pytest.mark.parametrize("fmt_kw", [NV12_8, dict(layout=1, depth=10, msb_aligned=0)], ids=["nv12", "i420p10"])
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_batch_three_slots_with_a_new_clip(fmt_kw, device_form):
    """3 slots at 45 x 67, set, compute, push with new_clip on slot 1, compute: planes, flows and arming of every slot equal those of the
    RGB batch calls on to_rgb of the same frames (whose slots the existing suite holds to single contexts)"""
    import eppm_amd
    from eppm_amd import yuv
    h, w, n = 45, 67, 3
    fmt = yuv.YuvFormat(**fmt_kw)
    clips = [yuv_clip(fmt, h, w, 3, seed=20 + 2 * k) for k in range(n)]
    ref, bat = eppm_amd.EPPMBatch(h, w, n), eppm_amd.EPPMBatch(h, w, n)
    keep = []

    def dev(frames):
        d = [f.to_device() for f in frames]
        keep.extend(d)
        return d
    try:
        for b in (ref, bat):
            b.set_temporal(True)
        ref.set_data([(yuv.to_rgb(c[0]), yuv.to_rgb(c[1])) for c in clips])
        if device_form:
            bat.set_data_yuv_device(fmt, dev([c[0] for c in clips]), dev([c[1] for c in clips]))
        else:
            bat.set_data_yuv([(c[0], c[1]) for c in clips])
        f0, r0 = bat.compute_flow(), ref.compute_flow()
        cuts = [False, True, False]
        ref.push_frames([yuv.to_rgb(c[2]) for c in clips], cuts)
        if device_form:
            bat.push_frames_yuv_device(fmt, dev([c[2] for c in clips]), cuts)
        else:
            bat.push_frames_yuv([c[2] for c in clips], cuts)
        assert [bat.temporal_valid(k) for k in range(n)] == [ref.temporal_valid(k) for k in range(n)] == [True, False, True]
        f1, r1 = bat.compute_flow(), ref.compute_flow()
        for k in range(n):
            assert same_state(batch_planes(bat, k), batch_planes(ref, k)) == [], k
            for got, want in ((f0[k], r0[k]), (f1[k], r1[k])):
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), k
        single = eppm_amd.EPPM()
        single.init(h, w)
        try:
            single.set_data(yuv.to_rgb(clips[1][1]), yuv.to_rgb(clips[1][2]))      # slot 1 against a single context, at its new pair
            want = context_state(single, flow=False)
            got = batch_planes(bat, 1)
            assert [k for k in got if got[k].tobytes() != want[k].tobytes()] == []
        finally:
            single.close()
        with pytest.raises(eppm_amd.EppmError, match="status 1"):               # n must equal the active pairs
            bat.push_frames_yuv([clips[0][0]] * 2)
    finally:
        bat.close()
        ref.close()


def slot_frames(fmt, h, w, distinct, seed):
    from eppm_amd import yuv
    rng = np.random.default_rng(seed)
    return [yuv.from_rgb(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), fmt) for _ in range(distinct)]


@pytest.mark.parametrize("n,h,w", [(17, 16, 16), (4096, 4, 4)], ids=["one-more-than-a-chunk", "4096-slots"])
def test_batch_pointer_table_chunks(n, h, w):
    """one slot more than one pointer-table chunk holds, and the largest batch at the smallest legal frame, through the device form (the
    caller's pointers travel in the kernel arguments) and the host form: every slot holds the planes a context holds after the RGB call on
    its own frame.  8 distinct frames, dealt so that neighbouring slots and neighbouring chunks differ."""
    import eppm_amd
    from eppm_amd import yuv
    fmt = yuv.YuvFormat()
    frames = slot_frames(fmt, h, w, 8, seed=n)
    pick = [(5 * k + k // 16) % 8 for k in range(n)]
    ref = eppm_amd.EPPMBatch(h, w, 8)
    bat = eppm_amd.EPPMBatch(h, w, n)
    try:
        ref.set_data([(yuv.to_rgb(f), yuv.to_rgb(frames[(i + 1) % 8])) for i, f in enumerate(frames)])
        want = [batch_planes(ref, i) for i in range(8)]
        dev = [f.to_device() for f in frames]
        for form in ("device", "host"):
            if form == "device":
                bat.set_data_yuv_device(fmt, [dev[i] for i in pick], [dev[(i + 1) % 8] for i in pick])
            else:
                bat.set_data_yuv([(frames[(i + 3) % 8], frames[(i + 4) % 8]) for i in pick])
            shift = 0 if form == "device" else 3
            step = 1 if n <= 64 else 61          # every slot of the small batch; of the large one every 61st, and each chunk's edges
            slots = sorted(set(range(0, n, step)) | {k for k in range(n) if k % 16 in (0, 15) and k // 16 in (0, 1, n // 16 - 1)})
            for k in slots:
                got = batch_planes(bat, k)
                w_ = want[(pick[k] + shift) % 8]
                assert [key for key in got if got[key].tobytes() != w_[key].tobytes()] == [], (form, k)
            for k in range(n):                   # and the two level-0 images of every slot
                w_ = want[(pick[k] + shift) % 8]
                assert all(bat.plane(k, name, 0).tobytes() == w_[name, 0].tobytes() for name in ("img1", "img2")), (form, k)
    finally:
        bat.close()
        ref.close()


# ---- 5. the CLI ----
def test_cli_y4m_clip_equals_the_ppm_clip(tmp_path):
    """runeppm --sequence clip.y4m against --sequence on the PPMs of yuv.to_rgb of the same frames: the same flows byte for byte, the
    denoised frames of --y4m-out = from_rgb of the PPM run's frames in the input's format and rate, --yuv-matrix changes what goes in"""
    import eppm_amd
    from eppm_amd import yuv
    h, w = 96, 128
    fmt = yuv.YuvFormat(layout=1, depth=10, siting=1, matrix=0)         # as a reader finds it: 96 rows -> BT.601
    clip = yuv_clip(fmt, h, w, 3, seed=31)
    yuv.write_y4m(tmp_path / "clip.y4m", clip, fps=(24, 1))
    for k, f in enumerate(clip):
        (tmp_path / f"f{k}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + yuv.to_rgb(f).tobytes())
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path("")), "runeppm")

    def run(*args):
        out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-1000:]
    run("--sequence", "clip.y4m", "--out-prefix", "y", "--denoise", "--y4m-out")
    run("--sequence", "f0.ppm", "f1.ppm", "f2.ppm", "--out-prefix", "p", "--denoise")
    for k in (1, 2):
        assert (tmp_path / f"y_{k:04d}.flo").read_bytes() == (tmp_path / f"p_{k:04d}.flo").read_bytes()
    r = yuv.read_y4m(tmp_path / "y_dn.y4m")
    got = list(r)
    assert r.fps == (24, 1) and r.fmt.as_dict() == fmt.as_dict() and len(got) == 3
    for k, f in enumerate(got):
        raw = (tmp_path / f"p_dn_{k:04d}.ppm").read_bytes()
        want = yuv.from_rgb(np.frombuffer(raw[-h * w * 3:], np.uint8).reshape(h, w, 3), fmt)
        assert all(np.array_equal(a, b) for a, b in zip(f.planes, want.planes)), k
    assert not list(tmp_path.glob("y_dn_*.ppm"))
    run("--sequence", "clip.y4m", "--out-prefix", "m", "--yuv-matrix", "2020")
    assert (tmp_path / "m_0001.flo").read_bytes() != (tmp_path / "y_0001.flo").read_bytes()
    bad = subprocess.run([exe, "--sequence", "clip.y4m", "--out-prefix", "b", "--yuv-matrix", "500"], capture_output=True, text=True, cwd=tmp_path)
    assert bad.returncode == 2 and "usage" in bad.stderr
