"""Child process of tests/test_alloc_fill_gpu.py, and the home of what both share: the scenarios that run the library's public calls in
memory poisoned by the test option "alloc_fill" (include/eppm_test.h; DESIGN.md, "Write-before-read of every allocation").

A scenario is a function without arguments that builds its objects, returns every output as an ordered {name: bytes} dict and has closed
everything when it returns.  across_fills() runs it once per fill -- eppm_release_cached_memory(), the option, the scenario, the option
back to -1, eppm_release_cached_memory() again -- and compares the bytes of every output with the unfilled run's: np.array_equal, no
tolerance.  As a program it selects the tolerance library's test build (the pytest process holds the exact one), runs every scenario and
expects the same; it prints the library's version first and "PART OK" last."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))

# -1: the unfilled baseline; 0xFF: NaN floats, -1 integers, 255 bytes; 0x01: denormal floats, small positive int16, "set" mask and label
# bytes; 0x7F: huge finite floats, 0x7f7f... keys
FILLS = (-1, 0xFF, 0x01, 0x7F)
CLIP_H, CLIP_W = 96, 128
SUB = (slice(20, 95), slice(30, 127))          # the 97x75 sub-crop of the 160x120 crop: no dimension a multiple of 16, odd pyramid halves
SECOND_RADIUS = 17                             # tests/test_variants_gpu.py: RADII
VARIANTS = (("sweep_spec", 0, -1), ("sweep_spec", 1, -1), ("sweep_spec", 2, -1), ("sweep_spec", 3, -1), ("c2f_force_split", 1, 0),
            ("c2f_no_split", 1, 0), ("search_pre_from", 0, -1), ("rand_table", 0, 1))
STATE = 3                                      # EPPM_ERR_STATE


def L():
    from eppm_amd._lib import lib
    return lib()


def set_option(name, value):
    from eppm_amd._lib import check
    check(L().eppm_test_set_option(name.encode(), int(value)), f"eppm_test_set_option {name}")


# ---- outputs as bytes ----
def put(out, name, x):
    """x, flattened into out under `name`: arrays as their bytes, containers entry by entry, anything else as its repr"""
    if isinstance(x, np.ndarray):
        assert name not in out, name
        out[name] = np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
    elif isinstance(x, dict):
        for k in sorted(x):
            put(out, f"{name}.{k}", x[k])
    elif isinstance(x, (list, tuple)):
        put(out, f"{name}.len", repr(len(x)))
        for k, v in enumerate(x):
            put(out, f"{name}[{k}]", v)
    else:
        assert name not in out, name
        out[name] = np.frombuffer(repr(x).encode(), np.uint8)


def status_of(call):
    """the status of a call that is expected to fail (-1: an EppmError that names none), 0 if it does not fail"""
    from eppm_amd import EppmError
    try:
        call()
    except EppmError as e:
        return int(str(e).split("status ")[1].split(":")[0]) if "status " in str(e) else -1
    return 0


def run_filled(scenario, fill):
    L().eppm_release_cached_memory()
    try:
        set_option("alloc_fill", fill)
        return scenario()
    finally:
        L().eppm_test_set_option(b"alloc_fill", -1)
        L().eppm_release_cached_memory()


def first_difference(base, got):
    if list(base) != list(got):
        return "the outputs themselves: " + repr(sorted(set(base) ^ set(got))[:4])
    for k in base:
        if not np.array_equal(base[k], got[k]):
            n = int((base[k] != got[k]).sum()) if base[k].shape == got[k].shape else -1
            return f"output '{k}' ({n} of {base[k].size} bytes)"
    return None


def across_fills(scenario, what, also=None):
    """the scenario under every fill, in order; stops at the first fill whose bytes differ from the unfilled run's and names the output.
    also(outputs, fill): a further check of every run (the oracle, where the suite has one)"""
    base = run_filled(scenario, FILLS[0])
    if also:
        also(base, FILLS[0])
    for fill in FILLS[1:]:
        got = run_filled(scenario, fill)
        bad = first_difference(base, got)
        assert bad is None, f"{what}: under fill 0x{fill:02X} {bad} differs from the unfilled run: something read memory nothing had written"
        if also:
            also(got, fill)
    return base


# ---- inputs ----
_cache = {}


def stills():
    """{"crop": the 160x120 crop fixture, "sub": its 97x75 sub-crop}"""
    if "stills" not in _cache:
        from conftest import GOLDEN, read_ppm
        a, b = (read_ppm(os.path.join(GOLDEN, n)) for n in ("frame10.ppm", "frame11.ppm"))
        a, b = a[180:300, 240:400].copy(), b[180:300, 240:400].copy()
        _cache["stills"] = {"crop": (a, b), "sub": (a[SUB].copy(), b[SUB].copy())}
    return _cache["stills"]


def clip():
    if "clip" not in _cache:
        from test_stabilize_cpu import moving_clip
        _cache["clip"] = moving_clip(CLIP_H, CLIP_W, 4)
    return _cache["clip"]


def rgba_of(rgb):
    """(h, w, 3) uint8 -> (h, w, 4) with alpha 0, as set_data makes it"""
    return np.ascontiguousarray(np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,), np.uint8)], axis=2))


class DevMem:
    """caller device memory (eppm_malloc_device: not one of the library's own blocks, never filled)"""

    def __init__(self, arr=None, nbytes=None):
        from eppm_amd._lib import check
        self.p = C.c_void_p()
        self.n = int(arr.nbytes if arr is not None else nbytes)
        check(L().eppm_malloc_device(C.byref(self.p), C.c_size_t(max(self.n, 1))), "malloc")
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            check(L().eppm_memcpy_h2d(self.p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)), "h2d")
        else:
            check(L().eppm_memset_device(self.p, 0xA5, C.c_size_t(self.n)), "memset")         # the caller's own pattern, the same in every run

    @property
    def addr(self):
        return self.p.value

    def get(self, shape, dtype):
        from eppm_amd._lib import check
        out = np.empty(shape, dtype)
        assert out.nbytes == self.n
        check(L().eppm_device_synchronize(), "sync")
        check(L().eppm_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(self.n)), "d2h")
        return out

    def free(self):
        if self.p:
            L().eppm_free_device(self.p)
            self.p = C.c_void_p()


def pair_inputs():
    """What the size-only forms of the attachments step on, per pair of the clip: the RGBA frames, both flows (float2), both masks and the
    stabiliser's motion mask -- computed once, without a fill, and the same arrays under every fill."""
    if "pairs" not in _cache:
        import eppm_amd
        f = clip()
        e = eppm_amd.EPPM()
        out = []
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            st = eppm_amd.Stabilizer(e)
            for k in range(len(f) - 1):
                if k:
                    e.push_frame(f[k + 1])
                u, v, bu, bv, o1, o2 = e.compute_flow_bidirectional()
                st.step()
                out.append(dict(rgba1=rgba_of(f[k]), rgba2=rgba_of(f[k + 1]), fwd=np.ascontiguousarray(np.stack([u, v], -1)),
                                bwd=np.ascontiguousarray(np.stack([bu, bv], -1)), occ1=o1, occ2=o2, mask=st.mask()))
            st.close()
        finally:
            e.close()
        _cache["pairs"] = out
    return _cache["pairs"]


# ---- scenario A: the core path ----
def planes_of(out, name, e, top_only=("nnf1", "nnf2", "cost1", "cost2"), every=("flow", "img1", "img2", "census1", "census2")):
    nl = len(e.level_dims())
    for p in every:
        for l in range(nl):
            put(out, f"{name}.{p}_L{l}", e.plane(p, l))
    for p in top_only:
        put(out, f"{name}.{p}_L{nl - 1}", e.plane(p, nl - 1))


def core_forms(size):
    """set_data + compute_flow with every plane, the begin / end form, the device form, the colour-coded flow"""
    import eppm_amd
    a, b = stills()[size]
    h, w, _ = a.shape

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        bufs = []
        try:
            e.init(h, w)
            e.set_data(a, b)
            u, v = e.compute_flow()
            put(out, "compute.u", u); put(out, "compute.v", v)
            planes_of(out, "compute", e)
            put(out, "color", e.compute_flow_color())
            e.compute_flow_begin()
            put(out, "begin_end", e.compute_flow_end())
            bufs = [DevMem(rgba_of(a)), DevMem(rgba_of(b)), DevMem(nbytes=h * w * 8)]
            e.set_data_device(bufs[0].addr, bufs[1].addr, w * 4)
            e.compute_flow_device(bufs[2].addr)
            e.synchronize()
            put(out, "device.flow", bufs[2].get((h, w, 2), np.float32))
            planes_of(out, "device", e)
        finally:
            e.close()
            for d in bufs:
                d.free()
        return out
    return scenario


def core_variant(option, value, default, size="crop", patch_r=None):
    """the plain compute under a variant switch that changes which planes are used (option None: none), or at another patch radius"""
    import eppm_amd
    a, b = stills()[size]
    h, w, _ = a.shape

    def scenario():
        out = {}
        e = None
        try:
            if option:
                set_option(option, value)
            e = eppm_amd.EPPM(params=eppm_amd.Params(patch_r=patch_r) if patch_r else None)
            e.init(a, b, h, w)
            u, v = e.compute_flow()
            put(out, "compute.u", u); put(out, "compute.v", v)
            planes_of(out, "compute", e, every=("flow",))
            u, v = e.compute_flow()          # and again in the planes the first run left
            put(out, "again.u", u); put(out, "again.v", v)
        finally:
            if e is not None:
                e.close()
            if option:
                set_option(option, default)
        return out
    return scenario


def core_recycled(size="crop"):
    """the cache's other path: a context works on another pair (bidirectional, so that the backward branch has used the slab's planes too)
    and is destroyed; the next context of its size takes its slab and pinned buffers from the cache -- the other pair's leftovers in the
    unfilled run, the fill otherwise -- and must compute what a context in fresh memory computes"""
    import eppm_amd
    a, b = stills()[size]
    h, w, _ = a.shape

    def scenario():
        out = {}
        first, e = eppm_amd.EPPM(), eppm_amd.EPPM()
        try:
            first.init(np.ascontiguousarray(b[::-1]), np.ascontiguousarray(a[:, ::-1]), h, w)
            put(out, "other_pair", first.compute_flow_bidirectional())
            first.close()
            e.init(a, b, h, w)
            u, v = e.compute_flow()
            put(out, "compute.u", u); put(out, "compute.v", v)
            planes_of(out, "compute", e)
            put(out, "bidir", e.compute_flow_bidirectional())
        finally:
            first.close()
            e.close()
        return out
    return scenario


def ref_abi_path(force_split=False):
    """the reference's stage launchers in the order its class calls them, on the crop: their planes live in the launchers' scratch;
    force_split: the candidate refine's launchers bring the split path's cost scratch ("c2f_force_split", which contexts do not read)"""
    import eppm_amd
    from eppm_amd import stages as S
    from eppm_amd.api import uchar4
    a, b = stills()["crop"]
    h, w, _ = a.shape

    def raw(rgb):
        r = np.zeros((h, w), uchar4)
        r["x"], r["y"], r["z"] = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        return r

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        e.init(h, w)
        dims = e.level_dims()
        e.close()
        S.set_params(None)
        i1, i2, c1, c2 = S.prepare(raw(a), raw(b), dims)
        top = len(dims) - 1
        n1, k1 = S.patchmatch(S.PlaneSet(i1[top], i2[top], c1[top], c2[top]))
        n2, k2 = S.patchmatch(S.PlaneSet(i2[top], i1[top], c2[top], c1[top]))
        put(out, "patchmatch", (n1, k1, n2, k2))
        n1, k1, n2, k2 = S.left_right_check(n1, k1, n2, k2)
        n1, k1 = S.outlier_removal(n1, k1)
        n1 = S.weighted_median(n1, i1[top], 20, True)
        n1 = S.fill_holes(n1, i1[top])
        flow = S.nnf2flow(n1)
        put(out, f"flow_L{top}", flow)
        try:
            if force_split:
                set_option("c2f_force_split", 1)
            for l in range(top - 1, -1, -1):
                flow = S.blf_c2f(flow, S.PlaneSet(i1[l], i2[l], c1[l], c2[l]), dims[l + 1])
                flow = S.flow_smoothing(flow, i1[l])
                put(out, f"flow_L{l}", flow)
        finally:
            if force_split:
                set_option("c2f_force_split", 0)
        put(out, "flow", S.flow_smoothing(flow, i1[0]))
        return out
    return scenario


def oracle_flow_check(crop_stages):
    """also= of across_fills for a scenario on the crop: compute.u / compute.v equal the oracle's flow under every fill"""
    def also(out, fill):
        for k in ("u", "v"):
            want = np.frombuffer(np.ascontiguousarray(crop_stages[k]).tobytes(), np.uint8)
            assert np.array_equal(out[f"compute.{k}"], want), f"fill {fill}: {k} of the crop differs from the oracle"
    return also


# ---- scenario B: the lazily made blocks ----
LAZY_OPS = ("bidir", "bidir_device", "interpolate", "mblur0", "mblur1")


def lazy_block(size, op, after_forward):
    """op as the first call of a new context, or (after_forward) as the second call after a forward-only compute"""
    import eppm_amd
    a, b = stills()[size]
    h, w, _ = a.shape

    def bwd_planes(out, e):
        for l in range(len(e.level_dims())):
            put(out, f"flow_bwd_L{l}", e.plane("flow_bwd", l))
        put(out, "occ1_L0", e.plane("occ1", 0)); put(out, "occ2_L0", e.plane("occ2", 0))

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        bufs = []
        try:
            e.init(a, b, h, w)
            if after_forward:
                put(out, "forward", e.compute_flow())
            if op == "bidir":
                put(out, "bidir", e.compute_flow_bidirectional())
                bwd_planes(out, e)
            elif op == "bidir_device":
                bufs = [DevMem(nbytes=h * w * 8), DevMem(nbytes=h * w * 8), DevMem(nbytes=h * w), DevMem(nbytes=h * w)]
                e.compute_flow_bidirectional_device(*[d.addr for d in bufs])
                e.synchronize()
                put(out, "bidir_device", [bufs[0].get((h, w, 2), np.float32), bufs[1].get((h, w, 2), np.float32),
                                          bufs[2].get((h, w), np.uint8), bufs[3].get((h, w), np.uint8)])
                bwd_planes(out, e)
            elif op == "interpolate":
                e.compute_flow_bidirectional()
                put(out, "interpolate", e.interpolate([0.25, 0.5, 1.0]))
                put(out, "interpolate_again", e.interpolate([0.0, 0.75]))
            elif op == "mblur0":
                if not after_forward:
                    e.compute_flow()
                put(out, "mblur0", e.motion_blur(frame=0))
            else:
                e.compute_flow_bidirectional()
                put(out, "mblur1", e.motion_blur(frame=1))
                put(out, "mblur0", e.motion_blur(frame=0, shutter=1.0, max_radius=31, taps=3))
        finally:
            e.close()
            for d in bufs:
                d.free()
        return out
    return scenario


# ---- scenario C: streaming and draft ----
TEMPORAL_PLANES = ("prior1", "prior2", "nnf_init1", "nnf_init2", "cost_init1", "cost_init2")


def streaming(stop_level):
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_temporal(True)
            if stop_level:
                e.set_stop_level(stop_level)
            e.set_data(f[0], f[1])
            put(out, "pair0", e.compute_flow())
            top = len(e.level_dims()) - 1
            for k in (2, 3):
                e.push_frame(f[k])
                assert e.temporal_valid()
                put(out, f"pair{k - 1}", e.compute_flow())
                for p in TEMPORAL_PLANES:
                    put(out, f"pair{k - 1}.{p}", e.plane(p, top))
            e.temporal_reset()
            put(out, "after_reset", e.compute_flow())
            e.push_frame(f[0])
            put(out, "bidir_seeded", e.compute_flow_bidirectional())
        finally:
            e.close()
        return out
    return scenario


# ---- scenario D: batch contexts ----
def batch(case):
    """"shrink": three active pairs, then two, then three again; "partial": two active pairs of three from the start -- slot 2 holds
    nothing but what the allocation held -- streaming with one new_clip flag, then the bidirectional form"""
    import eppm_amd
    a, b = stills()["sub"]
    h, w, _ = a.shape
    c, d = np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1])
    pairs = [(a, b), (b, a), (c, d)]

    def scenario():
        out = {}
        e = eppm_amd.EPPMBatch(h, w, 3)
        try:
            if case == "shrink":
                for k, n in enumerate((3, 2, 3)):
                    e.set_data(pairs[:n])
                    put(out, f"compute{k}_{n}pairs", e.compute_flow())
                put(out, "bidir3", e.compute_flow_bidirectional())
                e.set_data(pairs[1:])
                put(out, "bidir2", e.compute_flow_bidirectional())
                put(out, "interpolate2", e.interpolate([0.5]))
                put(out, "mblur2", e.motion_blur(frame=1))
            else:
                e.set_temporal(True)
                e.set_data(pairs[:2])
                put(out, "pair0", e.compute_flow())
                e.push_frames([c, d], new_clip=[False, True])
                put(out, "valid", [e.temporal_valid(k) for k in range(3)])
                put(out, "pair1", e.compute_flow())
                put(out, "prior1.slot0", e.plane(0, "prior1", len(_levels(e)) - 1))
                e.push_frames([a, c])
                put(out, "pair2", e.compute_flow_bidirectional())
                for k in range(2):
                    for l in range(len(_levels(e))):
                        put(out, f"flow_bwd.slot{k}_L{l}", e.plane(k, "flow_bwd", l))
                put(out, "interpolate", e.interpolate([0.25, 1.0]))
                put(out, "mblur", e.motion_blur(frame=0))
        finally:
            e.close()
        return out
    return scenario


def _levels(e):
    n = L().eppm_num_levels(e._ctx)
    return list(range(n))


# ---- scenario E: the attachments ----
ATTACHMENTS = ("tracker", "tfilter", "stab", "cutdet", "cmap", "objects")


def make_attachment(kind, ctx, slots=1):
    import eppm_amd
    cls = {"tfilter": eppm_amd.TemporalFilter, "stab": eppm_amd.Stabilizer, "cutdet": eppm_amd.CutDetector, "cmap": eppm_amd.CorrespondenceMap,
           "objects": eppm_amd.ObjectDetector}
    if kind == "tracker":
        return eppm_amd.Tracker(ctx)
    return cls[kind](ctx) if ctx is not None else cls[kind](None, size=(CLIP_H, CLIP_W), slots=slots)


def layer_rgba():
    rng = np.random.default_rng(5)
    return rng.integers(0, 256, (CLIP_H, CLIP_W, 4), dtype=np.uint8)


def getters(out, name, kind, att, slot):
    """every getter of the attachment on one slot"""
    if kind == "tracker":
        put(out, f"{name}.counts", att.counts()); put(out, f"{name}.tracks", att.tracks()); put(out, f"{name}.ended", att.ended())
    elif kind == "tfilter":
        put(out, f"{name}.frame", att.frame(slot)); put(out, f"{name}.state", att.state(slot))
    elif kind == "stab":
        put(out, f"{name}.frame", att.frame(slot)); put(out, f"{name}.mask", att.mask(slot))
        put(out, f"{name}.model", att.model(slot)); put(out, f"{name}.path", att.path(slot, counts=True))
    elif kind == "cutdet":
        put(out, f"{name}.stats", att.stats(slot)); put(out, f"{name}.cuts", att.cuts(att.nslots))
    elif kind == "cmap":
        put(out, f"{name}.map", att.map(slot)); put(out, f"{name}.render", att.render(slot)); put(out, f"{name}.age", att.age(slot))
        att.set_layer(layer_rgba(), slot)
        put(out, f"{name}.render_layer", att.render(slot))
        att.set_layer(None, slot)
        put(out, f"{name}.render_default", att.render(slot))
    else:
        put(out, f"{name}.objects", att.objects(slot)); put(out, f"{name}.counts", att.counts(slot))
        put(out, f"{name}.labels", att.labels(slot)); put(out, f"{name}.state", att.state(slot))


def unstepped_statuses(kind, att, slot):
    """what every getter answers on a slot that was never stepped: {getter: status or value}, and what it answers today"""
    if kind == "tfilter":
        got = {"frame": status_of(lambda: att.frame(slot)), "state": status_of(lambda: att.state(slot))}
        want = {"frame": STATE, "state": STATE}
    elif kind == "stab":
        c, s, counts = att.path(slot, counts=True)
        got = {"frame": status_of(lambda: att.frame(slot)), "mask": status_of(lambda: att.mask(slot)), "model": status_of(lambda: att.model(slot)),
               "path": (c.tolist(), s.tolist(), counts)}
        want = {"frame": STATE, "mask": STATE, "model": STATE, "path": ([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], (0, 0))}
    elif kind == "cutdet":
        got = {"stats": status_of(lambda: att.stats(slot)), "cut": att.cuts(att.nslots)[slot]}
        want = {"stats": STATE, "cut": False}
    elif kind == "cmap":
        got = {"map": status_of(lambda: att.map(slot)), "render": status_of(lambda: att.render(slot)), "age": status_of(lambda: att.age(slot))}
        want = {"map": STATE, "render": STATE, "age": -1}         # (eppm_cmap_age returns -1, which age() raises without a status)
    else:
        car, pid, page, nxt = att.state(slot)
        got = {"objects": status_of(lambda: att.objects(slot)), "labels": status_of(lambda: att.labels(slot)),
               "state": (int(car.any()), int(pid.any()), int(page.any()), nxt)}
        want = {"objects": STATE, "labels": STATE, "state": (0, 0, 0, 1)}
    assert got == want, f"{kind}: a never-stepped slot answers {got}, not {want}"
    return got


def attached(kind):
    """the attachment on a context over the four-frame clip: a step per pair, the middle one with a cut flag, a reset before the last"""
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        att = None
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            att = make_attachment(kind, e)
            for k in range(3):
                if k:
                    e.push_frame(f[k + 1])
                e.compute_flow_bidirectional_device()
                if k == 2 and hasattr(att, "reset"):
                    att.reset(0)
                if kind in ("tracker", "cutdet"):
                    att.step()
                else:
                    att.step(cut=[k == 1])
                getters(out, f"pair{k}", kind, att, 0)
        finally:
            if att is not None:
                att.close()
            e.close()
        return out
    return scenario


def size_only(kind):
    """the attachment without a context, three slots: slot 1 is stepped first, then slot 0, slot 2 never; slot 1 goes on with a cut step,
    a reset and another step; every getter after every step"""
    P = pair_inputs()
    pitch = CLIP_W * 4

    def scenario():
        out = {}
        att = make_attachment(kind, None, slots=3)
        dev = []
        try:
            D = []
            for p in P:
                D.append({k: DevMem(v) for k, v in p.items()})
                dev += list(D[-1].values())

            def step(slot, k, cut=False):
                d = {n: m.addr for n, m in D[k].items()}
                if kind == "tfilter":
                    att.step_frames(slot, d["rgba1"], d["rgba2"], pitch, d["bwd"], d["occ2"], cut)
                elif kind == "stab":
                    att.step_frames(slot, d["rgba2"], pitch, d["fwd"], d["occ1"], cut)
                elif kind == "cutdet":
                    att.step_frames(slot, d["rgba1"], d["rgba2"], pitch, d["bwd"], d["occ1"], d["occ2"])
                elif kind == "cmap":
                    att.step_frames(slot, d["rgba1"], d["rgba2"], pitch, d["bwd"], d["occ2"], cut)
                else:
                    att.step_frames(slot, d["mask"], d["fwd"], d["bwd"], d["occ2"], cut)

            step(1, 0)
            getters(out, "slot1.step1", kind, att, 1)
            step(0, 0)
            getters(out, "slot0.step1", kind, att, 0)
            getters(out, "slot1.after_slot0", kind, att, 1)
            step(1, 1, cut=True)
            getters(out, "slot1.step2_cut", kind, att, 1)
            if hasattr(att, "reset"):
                att.reset(1)
            step(1, 2)
            getters(out, "slot1.step3_after_reset", kind, att, 1)
            step(0, 1)
            getters(out, "slot0.step2", kind, att, 0)
            put(out, "slot2.unstepped", unstepped_statuses(kind, att, 2))
        finally:
            att.close()
            for d in dev:
                d.free()
        return out
    return scenario


def tracker_frames():
    """the tracker has one state and no constructor without a context: its caller-plane form on the clip's pairs"""
    import eppm_amd
    P = pair_inputs()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        att = None
        dev = []
        try:
            e.init(CLIP_H, CLIP_W)
            att = eppm_amd.Tracker(e)
            for k, p in enumerate(P):
                d = {n: DevMem(p[n]) for n in ("rgba1", "rgba2", "fwd", "bwd")}
                dev += list(d.values())
                att.step_frames(d["rgba1"].addr, d["rgba2"].addr, CLIP_W * 4, d["fwd"].addr, d["bwd"].addr)
                getters(out, f"pair{k}", "tracker", att, 0)
        finally:
            if att is not None:
                att.close()
            e.close()
            for d in dev:
                d.free()
        return out
    return scenario


# ---- the list of everything, for the child; the pytest module parametrises over the same constructors ----
def all_scenarios():
    S = []
    for size in ("crop", "sub"):
        S.append((f"core forms {size}", core_forms(size)))
        S.append((f"core recycled {size}", core_recycled(size)))
    S.append(("core plain crop", core_variant(None, 0, 0)))
    for o, v, d in VARIANTS:
        S.append((f"core {o}={v}", core_variant(o, v, d)))
    S.append((f"core patch_r={SECOND_RADIUS}", core_variant(None, 0, 0, patch_r=SECOND_RADIUS)))
    S.append(("reference-ABI launchers", ref_abi_path()))
    S.append(("reference-ABI launchers, split refine", ref_abi_path(force_split=True)))
    for op in LAZY_OPS:
        for after in (False, True):
            S.append((f"lazy {op} {'after a forward compute' if after else 'first call'}", lazy_block("sub", op, after)))
    S.append(("lazy bidir crop", lazy_block("crop", "bidir", False)))
    for stop in (0, 1, 2):
        S.append((f"streaming stop_level={stop}", streaming(stop)))
    for case in ("shrink", "partial"):
        S.append((f"batch {case}", batch(case)))
    for kind in ATTACHMENTS:
        S.append((f"attached {kind}", attached(kind)))
        S.append((f"size-only {kind}", tracker_frames() if kind == "tracker" else size_only(kind)))
    return S


def control():
    """the switch reaches the memory: a new 97x75 context's img1 plane, read before any set_data, is the fill byte everywhere"""
    import eppm_amd
    out = {}

    def scenario():
        e = eppm_amd.EPPM()
        try:
            e.init(75, 97)
            out["img1"] = e.plane("img1", 0)
        finally:
            e.close()
        return {}
    run_filled(scenario, 0x7F)
    got = out["img1"].view(np.uint8)
    assert got.size == 75 * 97 * 4 and (got == 0x7F).all(), f"{int((got != 0x7F).sum())} of {got.size} bytes of a fresh plane are not the fill"


def main():
    import conftest  # noqa: F401  (selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol_test")
    print(eppm_amd.lib().eppm_version().decode())
    control()
    n = 0
    for what, scenario in all_scenarios():
        across_fills(scenario, what)
        n += 1
    print(f"{n} scenarios are the same bytes under the fills {[hex(f & 0xFF) for f in FILLS[1:]]}")
    print("PART OK")


if __name__ == "__main__":
    main()
