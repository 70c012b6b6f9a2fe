"""Host-side mirror of ``class bao_flow_patchmatch_multiscale_cuda`` over the C ABI."""
import ctypes as C

import numpy as np

from .io import object_record
from ._lib import CDefectParams, CDefectStats, CDeintParams, CDeintStats, CDeflickerParams, CDeflickerStats, CObject, CObjectsCounts, CObjectsParams, CPlateParams, CRSParams, CCMapParams, CCutParams, CCutStats, CGMotionModel, CMBlurParams, CParams, CStabParams, CTFilterParams, CTrackCounts, CTrackParams, EppmError, check, lib

uchar4 = np.dtype([("x", "u1"), ("y", "u1"), ("z", "u1"), ("w", "u1")])
short2 = np.dtype([("x", "i2"), ("y", "i2")])
float2 = np.dtype([("x", "f4"), ("y", "f4")])

_PLANE_DTYPES = {"img1": uchar4, "img2": uchar4, "census1": np.uint8, "census2": np.uint8, "nnf1": short2,
                 "nnf2": short2, "cost1": np.float32, "cost2": np.float32, "flow": float2,
                 "flow_bwd": float2, "occ1": np.uint8, "occ2": np.uint8,
                 "prior1": short2, "prior2": short2, "nnf_init1": short2, "nnf_init2": short2, "cost_init1": np.float32, "cost_init2": np.float32}


def _params(struct, default_fn, noun, start=None, /, **kw):
    """A parameter struct with the library's defaults (or a copy of `start`) and the overrides kw; an unknown key is a TypeError."""
    p = struct()
    if start is not None:
        C.memmove(C.byref(p), C.byref(start), C.sizeof(p))
    else:
        check(getattr(lib(), default_fn)(C.byref(p)), default_fn)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown {noun} {k}")
        setattr(p, k, v)
    return p


def Params(**kw):
    """Tunables with the defaults of defs.h:31-76 (patch_r, num_iter, search_range, num_guess, seg_len, wmf_iters, seed, propagation: 0 segmented sweeps / 1 jump flood / 2 4-neighbour, levels: pyramid depth)."""
    return _params(CParams, "eppm_default_params", "parameter", **kw)


def host_register(arr):
    """Pin a numpy array's memory for DMA (eppm_host_register): set_data reads registered images, and compute_flow(out=...)
    writes registered planes, over PCIe directly -- no staging copy.  Keep the array alive until host_unregister."""
    check(lib().eppm_host_register(arr.ctypes.data, arr.nbytes), "eppm_host_register")
    return arr


def host_unregister(arr):
    check(lib().eppm_host_unregister(arr.ctypes.data), "eppm_host_unregister")


def pinned_empty(shape, dtype=np.uint8):
    """A numpy array in pinned host memory from eppm_host_alloc (counts as registered); freed with the array."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = C.c_void_p()
    check(lib().eppm_host_alloc(C.byref(p), max(n, 1)), "eppm_host_alloc")
    addr = p.value

    class _Owner:
        def __del__(self):
            try:
                lib().eppm_host_free(addr)
            except Exception:
                pass
    buf = (C.c_char * max(n, 1)).from_address(addr)
    buf._owner = _Owner()
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def _times(times):
    ts = [float(t) for t in times]
    if not ts:
        raise EppmError("interpolate: at least one time")
    return (C.c_float * len(ts))(*ts)


def MBlurParams(**kw):
    """eppm_mblur_params with the defaults of DESIGN.md section 18 (shutter 0.5, max_radius 16, taps 8)."""
    return _params(CMBlurParams, "eppm_mblur_default_params", "motion-blur parameter", **kw)


def RSParams(**kw):
    """eppm_rs_params with the defaults of DESIGN.md section 27 (readout 0.5, anchor 0.5, iters 3, axis 0)."""
    return _params(CRSParams, "eppm_rs_default_params", "rolling-shutter parameter", **kw)


def TrackParams(params=None, **kw):
    """eppm_track_params with the defaults of DESIGN.md section 12 (spacing 8, min_eig 2500, fb_alpha 0.01, fb_beta 0.5, mb_alpha 0.01,
    mb_beta 0.002, capacity 0: 4 x the number of cells); params: a CTrackParams to start from instead."""
    return _params(CTrackParams, "eppm_track_default_params", "track parameter", params, **kw)


class _Handle:
    """An object that owns one C handle: the attribute named by _handle, destroyed by eppm_<_prefix>_destroy (no prefix: eppm_destroy)."""
    _prefix, _handle = None, "_f"

    def close(self):
        if getattr(self, self._handle, None):
            getattr(lib(), f"eppm_{self._prefix}_destroy" if self._prefix else "eppm_destroy")(getattr(self, self._handle))
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SlotObject(_Handle):
    """What the per-clip objects with one slot per pair of a context share.  A class names its C prefix
    (eppm_<_prefix>_*) and sets self.params, an instance of its parameter struct, before _open."""

    def _open(self, ctx, size, slots, device):
        """eppm_<prefix>_create on a context, or (ctx None) eppm_<prefix>_create_size: size = (h, w), `slots` slots on `device`."""
        self._f = C.c_void_p()
        self.ctx = ctx
        name = f"eppm_{self._prefix}_create"
        if ctx is None:
            if size is None or len(size) != 2:
                raise EppmError(f"{type(self).__name__}: without a context, size=(h, w) is required")
            self.h, self.w, self.nslots = int(size[0]), int(size[1]), int(slots)
            check(getattr(lib(), name + "_size")(self.h, self.w, self.nslots, int(device), C.byref(self.params), C.byref(self._f)), name + "_size")
            return
        check(getattr(lib(), name)(ctx._ctx, C.byref(self.params), C.byref(self._f)), name)
        self.h, self.w = ctx.h, ctx.w
        self.nslots = int(lib().eppm_batch_size(ctx._ctx))

    def _call(self, fn, *args):
        name = f"eppm_{self._prefix}_{fn}"
        check(getattr(lib(), name)(self._f, *args), name)

    def _rgb(self, fn, slot):
        """(h, w, 3) uint8 from eppm_<prefix>_<fn>(slot, rgb, row_stride)"""
        rgb = np.empty((self.h, self.w, 3), np.uint8)
        self._call(fn, int(slot), rgb.ctypes.data, self.w * 3)
        return rgb


class _ClipObject(_SlotObject):
    """A slot object whose slots carry a state from pair to pair (every one but the cut detector): a cut restarts it, reset empties it."""

    def step(self, cut=None, ctx=None):
        """One step of every active pair's slot; cut: None, or one flag per active pair (true: the pair's image 2 is the first frame of
        another clip; what that means for the slot: the class's description).  Asynchronous on the context's stream."""
        c = self.ctx if ctx is None else ctx
        flags = None if cut is None else (C.c_uint8 * len(cut))(*[int(bool(x)) for x in cut])
        if flags is not None and len(cut) != getattr(c, "n", 1):
            raise EppmError(f"{type(self).__name__}.step: one cut flag per active pair")
        self._call("step", c._ctx, flags)

    def reset(self, slot=None):
        """The slot is empty again (slot=None: every slot); what its next step starts from: the class's description."""
        self._call("reset", -1 if slot is None else int(slot))


class _FrameObject(_ClipObject):
    """A clip object whose step leaves one output frame per slot (eppm_<prefix>_get, eppm_<prefix>_get_device); what frame(slot) shows:
    the class's frame."""

    def frames(self):
        """frame(k) of the context's active pairs' slots."""
        return [self.frame(k) for k in range(getattr(self.ctx, "n", 1))]

    def frame_device(self, slot, d_rgba, pitch):
        self._call("get_device", int(slot), d_rgba, pitch)


class Tracker(_Handle):
    """Dense point trajectories over the pairs of a context (eppm_tracker_*).  ctx: an EPPM or EPPMBatch; every
    step() advances the tracks by pair `pair` of the context's last compute_flow_bidirectional.  The tracker is its own allocation on the
    context's device; close() frees it."""
    _prefix, _handle = "tracker", "_t"

    def __init__(self, ctx, pair=0, params=None, **track_params):
        self._t = C.c_void_p()
        self.ctx, self.pair = ctx, int(pair)
        self.params = TrackParams(params, **track_params)
        check(lib().eppm_tracker_create(ctx._ctx, C.byref(self.params), C.byref(self._t)), "eppm_tracker_create")
        self.capacity = lib().eppm_track_capacity(C.byref(self.params), ctx.h, ctx.w)

    def step(self, pair=None, ctx=None):
        """One step on pair `pair` (default: the tracker's) of ctx (default: the tracker's); asynchronous on the context's stream."""
        c = self.ctx if ctx is None else ctx
        check(lib().eppm_track_step(self._t, c._ctx, self.pair if pair is None else int(pair)), "eppm_track_step")

    def step_frames(self, d_rgba1, d_rgba2, pitch, d_flow, d_flow_bwd):
        """eppm_track_step_frames: one step on caller device planes (addresses), synchronous."""
        check(lib().eppm_track_step_frames(self._t, d_rgba1, d_rgba2, pitch, d_flow, d_flow_bwd, self.ctx.h, self.ctx.w), "eppm_track_step_frames")

    def counts(self):
        c = CTrackCounts()
        check(lib().eppm_tracker_get(self._t, 0, None, None, None, C.byref(c)), "eppm_tracker_get")
        return c.as_dict()

    def tracks(self):
        """(ids int32 (n,), starts int32 (n,), xy float32 (n, 2)): the live tracks, positions in the current frame."""
        n = self.counts()["live"]
        ids, starts, xy = np.empty(n, np.int32), np.empty(n, np.int32), np.empty((n, 2), np.float32)
        c = CTrackCounts()
        check(lib().eppm_tracker_get(self._t, n, ids.ctypes.data, starts.ctypes.data, xy.ctypes.data, C.byref(c)), "eppm_tracker_get")
        return ids, starts, xy

    def ended(self):
        """(ids, starts, xy (last positions, in the frame before the last step), reasons 1..4, counts dict) of the last step."""
        n = self.counts()["ended"]
        ids, starts, why = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        xy = np.empty((n, 2), np.float32)
        c = CTrackCounts()
        check(lib().eppm_tracker_get_ended(self._t, n, ids.ctypes.data, starts.ctypes.data,
                                           xy.ctypes.data, why.ctypes.data, C.byref(c)), "eppm_tracker_get_ended")
        return ids, starts, xy, why, c.as_dict()

    def set(self, ids, starts, xy, next_id, frame):
        """Load a state (eppm_tracker_set): tracks at positions inside the frame, the next id and the current frame."""
        ids = np.ascontiguousarray(ids, np.int32)
        starts = np.ascontiguousarray(starts, np.int32)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        if not (len(ids) == len(starts) == len(xy)):
            raise EppmError("Tracker.set: ids, starts and xy of one length")
        check(lib().eppm_tracker_set(self._t, len(ids), ids.ctypes.data, starts.ctypes.data, xy.ctypes.data, int(next_id), int(frame)), "eppm_tracker_set")


class TemporalFilter(_FrameObject):
    """Motion-compensated temporal denoising over the pairs of a context (eppm_tfilter_*).  ctx: an EPPM or an
    EPPMBatch; one slot per pair of it.  Every step() moves the active pairs' slots from image 1 to image 2 of the context's last
    compute_flow_bidirectional*; an empty slot (new, or after reset()) starts from its pair's image 1.  The filter is its own allocation on
    the context's device; close() frees it."""
    _prefix = "tfilter"

    def __init__(self, ctx, thresh=40.0, n_max=8, size=None, slots=1, device=0):
        """ctx None: a filter without a context, for step_frames on caller planes (eppm_tfilter_create_size): size = (h, w), `slots` slots."""
        self.params = CTFilterParams(float(thresh), int(n_max))
        self._open(ctx, size, slots, device)

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, cut=False):
        """eppm_tfilter_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, int(bool(cut)))

    def frame(self, slot=0):
        """(h, w, 3) uint8: the slot's filtered frame."""
        return self._rgb("get", slot)

    def state(self, slot=0):
        """(h, w, 4) float32 {R, G, B, n}: the slot's state."""
        acc = np.empty((self.h, self.w, 4), np.float32)
        self._call("get_state", int(slot), acc.ctypes.data)
        return acc

    def set_state(self, slot, acc):
        acc = np.ascontiguousarray(acc, np.float32)
        if acc.shape != (self.h, self.w, 4):
            raise EppmError(f"TemporalFilter.set_state: the state must be ({self.h},{self.w},4) float32")
        self._call("set_state", int(slot), acc.ctypes.data)


class DefectFilter(_FrameObject):
    """Film-defect removal over the pairs of a context (eppm_defect_*): single-frame blotches (dust, dirt, dropouts)
    are concealed from both motion-compensated neighbours.  ctx: an EPPM or an EPPMBatch; one slot per pair of it.  Every step() repairs
    IMAGE 1 of the active pairs of the context's last compute_flow_bidirectional*, from image 2 and from the frame and backward flow the
    step before saved; the first step of a slot (new, after reset() or after a cut) and a step whose pair is cut pass image 1 through, so
    the first and the last frame of a clip are never repaired.  The filter is its own allocation on the context's device; close() frees it."""
    _prefix = "defect"

    def __init__(self, ctx, detect=60.0, agree=30.0, radius=3, grow=1, size=None, slots=1, device=0):
        """ctx None: a filter without a context, for step_frames on caller planes (eppm_defect_create_size): size = (h, w), `slots` slots."""
        self.params = CDefectParams(float(detect), float(agree), int(radius), int(grow))
        self._open(ctx, size, slots, device)

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow, d_flow_bwd, cut=False):
        """eppm_defect_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow, d_flow_bwd, int(bool(cut)))

    def frame(self, slot=0):
        """(h, w, 3) uint8: the slot's repaired image 1 of the last step."""
        return self._rgb("get", slot)

    def mask(self, slot=0):
        """(h, w) uint8: 0 untouched, 1 hit, 2 grown."""
        m = np.empty((self.h, self.w), np.uint8)
        self._call("get_mask", int(slot), m.ctypes.data)
        return m

    def stats(self, slot=0):
        """dict(hit, grown, second_chance, undecided): the pixel counts of the slot's last step."""
        st = CDefectStats()
        self._call("get_stats", int(slot), C.byref(st))
        return st.as_dict()

    def state(self, slot=0):
        """(frame (h, w, 3) uint8, backward flow (h, w, 2) float32, has_prev): what the slot's last step saved."""
        rgb, bwd, has = np.empty((self.h, self.w, 3), np.uint8), np.empty((self.h, self.w, 2), np.float32), C.c_int()
        self._call("get_state", int(slot), rgb.ctypes.data, bwd.ctypes.data, C.byref(has))
        return rgb, bwd, bool(has.value)

    def set_state(self, slot, frame, bwd, has_prev=True):
        rgb, bwd = np.ascontiguousarray(frame, np.uint8), np.ascontiguousarray(bwd, np.float32)
        if rgb.shape != (self.h, self.w, 3) or bwd.shape != (self.h, self.w, 2):
            raise EppmError(f"DefectFilter.set_state: a ({self.h},{self.w},3) uint8 frame and a ({self.h},{self.w},2) float32 flow")
        self._call("set_state", int(slot), rgb.ctypes.data, bwd.ctypes.data, int(bool(has_prev)))


class Deflicker(_FrameObject):
    """Flicker removal over the pairs of a context (eppm_deflicker_*): a gain and an offset per colour on a grid of
    cell x cell pixels, fitted to the motion-compensated reference and applied to IMAGE 2 of the active pairs of the context's last
    compute_flow_bidirectional*.  ctx: an EPPM or an EPPMBatch; one slot per pair of it.  The reference of a slot is its previous output;
    an empty slot (new, or after reset()) starts from its pair's image 1, and a step whose pair is cut returns image 2 itself.  The object
    is its own allocation on the context's device; close() frees it."""
    _prefix = "deflicker"

    def __init__(self, ctx, cell=32, iters=2, reject=60.0, tau=12.0, keep=1.0, n_min=32, size=None, slots=1, device=0):
        """ctx None: an object without a context, for step_frames on caller planes (eppm_deflicker_create_size): size = (h, w), `slots` slots."""
        self.params = CDeflickerParams(int(cell), int(iters), float(reject), float(tau), float(keep), int(n_min))
        self._open(ctx, size, slots, device)
        self.cells_y, self.cells_x = -(-self.h // int(cell)), -(-self.w // int(cell))

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, cut=False):
        """eppm_deflicker_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, int(bool(cut)))

    def frame(self, slot=0):
        """(h, w, 3) uint8: the slot's corrected image 2 of the last step."""
        return self._rgb("get", slot)

    def field(self, slot=0):
        """(field (cells_y, cells_x, 6) float32 {aR, aG, aB, bR, bG, bB}, valid (cells_y, cells_x) uint8) of the slot's last step."""
        f, v = np.empty((self.cells_y, self.cells_x, 6), np.float32), np.empty((self.cells_y, self.cells_x), np.uint8)
        self._call("get_field", int(slot), f.ctypes.data, v.ctypes.data)
        return f, v

    def stats(self, slot=0):
        """dict(used, valid_cells, cells): the members of the slot's last pass, the cells with n_min of them, the cells of the grid."""
        st = CDeflickerStats()
        self._call("get_stats", int(slot), C.byref(st))
        return st.as_dict()

    def state(self, slot=0):
        """(frame (h, w, 3) uint8, empty): the slot's reference and whether the slot counts as empty."""
        rgb, empty = np.empty((self.h, self.w, 3), np.uint8), C.c_int()
        self._call("get_state", int(slot), rgb.ctypes.data, C.byref(empty))
        return rgb, bool(empty.value)

    def set_state(self, slot, frame, empty=False):
        rgb = np.ascontiguousarray(frame, np.uint8)
        if rgb.shape != (self.h, self.w, 3):
            raise EppmError(f"Deflicker.set_state: a ({self.h},{self.w},3) uint8 frame")
        self._call("set_state", int(slot), rgb.ctypes.data, int(bool(empty)))


def DeintParams(params=None, **kw):
    """eppm_deint_params with the defaults of DESIGN.md section 26 (thresh 24, use_occ 1); params: a CDeintParams to start from instead."""
    return _params(CDeintParams, "eppm_deint_default_params", "deinterlacer parameter", params, **kw)


class Deinterlacer(_FrameObject):
    """Motion-compensated deinterlacing over the pairs of a context (eppm_deint_*).  The context's frames are FIELD
    FRAMES: a field's rows in place, the other rows filled by the line average (io.deint_bob_host).  Every step() makes the progressive
    frame at the time of IMAGE 2 of the active pairs of the context's last compute_flow_bidirectional*: its real rows (parity) are image
    2's, a pixel of a missing row is the slot's previous output gathered along the backward flow where the gate accepts it, the line
    average elsewhere.  ctx: an EPPM or an EPPMBatch; one slot per pair of it.  An empty slot (new, or after reset()) starts from its
    pair's image 1; a cut step takes nothing from the reference.  The object is its own allocation on the context's device; close() frees it."""
    _prefix = "deint"

    def __init__(self, ctx, thresh=24, use_occ=1, size=None, slots=1, device=0):
        """ctx None: an object without a context, for step_frames on caller planes (eppm_deint_create_size): size = (h, w), `slots` slots."""
        self.params = CDeintParams(int(thresh), int(use_occ))
        self._open(ctx, size, slots, device)

    def step(self, cut=None, parity=None, ctx=None):
        """One step of every active pair's slot.  parity: 0 or 1 per active pair (one number for a single pair): the rows of that pair's
        image 2 that are real.  cut: None, or one flag per active pair.  Asynchronous on the context's stream."""
        c = self.ctx if ctx is None else ctx
        n = getattr(c, "n", 1)
        if parity is None:
            raise EppmError("Deinterlacer.step: parity is required")
        par = [parity] if np.isscalar(parity) else list(parity)
        if len(par) != n or any(p not in (0, 1) for p in par):
            raise EppmError("Deinterlacer.step: one parity, 0 or 1, per active pair")
        if cut is not None and len(cut) != n:
            raise EppmError("Deinterlacer.step: one cut flag per active pair")
        flags = None if cut is None else (C.c_uint8 * n)(*[int(bool(x)) for x in cut])
        self._call("step", c._ctx, flags, (C.c_uint8 * n)(*[int(p) for p in par]))

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, cut=False, parity=0):
        """eppm_deint_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, int(bool(cut)), int(parity))

    def frame(self, slot=0):
        """(h, w, 3) uint8: the slot's progressive frame of the last step."""
        return self._rgb("get", slot)

    def mask(self, slot=0):
        """(h, w) uint8: 0 real row, 1 temporal, 2 spatial."""
        m = np.empty((self.h, self.w), np.uint8)
        self._call("get_mask", int(slot), m.ctypes.data)
        return m

    def stats(self, slot=0):
        """dict(temporal, spatial): the missing pixels of the slot's last step by mask value."""
        st = CDeintStats()
        self._call("get_stats", int(slot), C.byref(st))
        return st.as_dict()

    def state(self, slot=0):
        """(frame (h, w, 3) uint8, empty): the slot's reference and whether the slot counts as empty."""
        rgb, empty = np.empty((self.h, self.w, 3), np.uint8), C.c_int()
        self._call("get_state", int(slot), rgb.ctypes.data, C.byref(empty))
        return rgb, bool(empty.value)

    def set_state(self, slot, frame, empty=False):
        rgb = np.ascontiguousarray(frame, np.uint8)
        if rgb.shape != (self.h, self.w, 3):
            raise EppmError(f"Deinterlacer.set_state: a ({self.h},{self.w},3) uint8 frame")
        self._call("set_state", int(slot), rgb.ctypes.data, int(bool(empty)))


class Stabilizer(_FrameObject):
    """Global camera motion and video stabilisation over the pairs of a context (eppm_stab_*).  ctx: an EPPM or an
    EPPMBatch; one slot per pair of it.  Every step() fits the camera motion of the active pairs of the context's last
    compute_flow_bidirectional*, moves the slots' paths and renders image 2 from the smoothed camera; an empty slot (new, or after reset())
    starts from the identity.  The stabiliser is its own allocation on the context's device; close() frees it."""
    _prefix = "stab"

    def __init__(self, ctx, tau=1.0, iters=3, smooth=0.9, size=None, slots=1, device=0):
        """ctx None: a stabiliser without a context, for step_frames on caller planes (eppm_stab_create_size): size = (h, w), `slots` slots."""
        self.params = CStabParams(float(tau), int(iters), float(smooth))
        self._open(ctx, size, slots, device)

    def step_frames(self, slot, d_rgba2, pitch, d_flow, d_occ1, cut=False):
        """eppm_stab_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba2, pitch, d_flow, d_occ1, int(bool(cut)))

    def frame(self, slot=0):
        """(h, w, 3) uint8: the slot's stabilised frame."""
        return self._rgb("get", slot)

    def mask(self, slot=0):
        """(h, w) uint8: 0 the pixel of image 1 moves with the camera, 1 it moves on its own, 2 it has no valid vector."""
        m = np.empty((self.h, self.w), np.uint8)
        self._call("get_mask", int(slot), m.ctypes.data)
        return m

    def model(self, slot=0):
        """The camera motion of the slot's last pair: dict(p (6 float64, displacement form), n_valid, n_inliers, valid, passes)."""
        m = CGMotionModel()
        self._call("get_model", int(slot), C.byref(m))
        return m.as_dict()

    def path(self, slot=0, counts=False):
        """(C, S): the camera path and the smoothed path, six float64 {a00, a01, a10, a11, tx, ty} each; counts=True adds (frames,
        invalid_steps)."""
        p = np.empty(12, np.float64)
        n, bad = C.c_int64(), C.c_int64()
        self._call("get_path", int(slot), p.ctypes.data, C.byref(n), C.byref(bad))
        return (p[:6].copy(), p[6:].copy(), (n.value, bad.value)) if counts else (p[:6].copy(), p[6:].copy())

    def set_path(self, slot, c, s):
        p = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).ravel(), np.asarray(s, np.float64).ravel()]))
        if p.shape != (12,):
            raise EppmError("Stabilizer.set_path: C and S are six numbers each")
        self._call("set_path", int(slot), p.ctypes.data)


class CutDetector(_SlotObject):
    """Scene-cut detection from the bidirectional flow over the pairs of a context (eppm_cutdet_*).  ctx: an EPPM or
    an EPPMBatch; one slot per pair of it.  Every step() counts, for the active pairs of the context's last compute_flow_bidirectional*,
    the pixels that found no consistent partner in the other frame and decides whether the pair crosses a cut.  The detector is its own
    allocation on the context's device; close() frees it."""
    _prefix = "cutdet"

    def __init__(self, ctx, lost_permille=530, residual_max=-1.0, size=None, slots=1, device=0):
        """ctx None: a detector without a context, for step_frames on caller planes (eppm_cutdet_create_size): size = (h, w), `slots` slots."""
        self.params = CCutParams(int(lost_permille), float(residual_max))
        self._open(ctx, size, slots, device)

    def step(self, ctx=None):
        """One step of every active pair's slot.  Asynchronous on the context's stream."""
        c = self.ctx if ctx is None else ctx
        self._call("step", c._ctx)

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ1, d_occ2):
        """eppm_cutdet_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ1, d_occ2)

    def stats(self, slot=0):
        """The record of the slot's last step: dict(n, c1 (4 counts), c2, n_tracked, sad, cut, stepped)."""
        st = CCutStats()
        self._call("get", int(slot), C.byref(st))
        return st.as_dict()

    def cuts(self, n=None):
        """The verdicts of slots 0 .. n - 1 (default: the context's active pairs) as a list of bools: one small copy, synchronous."""
        n = int(getattr(self.ctx, "n", 1) if n is None else n)
        out = (C.c_uint8 * max(n, 1))()
        self._call("cuts", n, out)
        return [bool(x) for x in out[:n]]


def CMapParams(**kw):
    """eppm_cmap_params with the defaults of DESIGN.md section 19 (thresh 90, tear 2, use_occ 1)."""
    return _params(CCMapParams, "eppm_cmap_default_params", "correspondence-map parameter", **kw)


class CorrespondenceMap(_ClipObject):
    """Dense correspondence maps to an anchor frame over the pairs of a context (eppm_cmap_*).  ctx: an EPPM or an
    EPPMBatch; one slot per pair of it.  Every step() moves the active pairs' slots from image 1 to image 2 of the context's last
    compute_flow_bidirectional*: map(slot)[y, x] is then the position in the slot's anchor frame that pixel (x, y) of image 2 shows, and
    render(slot) the slot's layer composited over image 2 through that map.  A step renders too; an empty slot (new, or after reset())
    anchors on its pair's image 1, a slot whose pair is flagged as a cut on that pair's image 2.  The object is its own allocation on the
    context's device; close() frees it.  params: CMapParams' thresh, tear and use_occ."""
    _prefix = "cmap"

    def __init__(self, ctx, size=None, slots=1, device=0, **params):
        """ctx None: a map without a context, for step_frames on caller planes (eppm_cmap_create_size): size = (h, w), `slots` slots."""
        self.params = CMapParams(**params)
        self._open(ctx, size, slots, device)

    def step_frames(self, slot, d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, cut=False):
        """eppm_cmap_step_frames: one step of one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_rgba1, d_rgba2, pitch, d_flow_bwd, d_occ2, int(bool(cut)))

    def map(self, slot=0):
        """(h, w, 2) float32 (sx, sy): the slot's map; a lost pixel holds (1e10, 1e10)."""
        xy = np.empty((self.h, self.w, 2), np.float32)
        self._call("get_state", int(slot), xy.ctypes.data)
        return xy

    state = map

    def known(self, slot=0):
        """(h, w) bool: the pixels of the current frame whose position in the anchor frame is known."""
        m = self.map(slot)
        with np.errstate(invalid="ignore"):
            return (np.abs(m[..., 0]) <= np.float32(1e9)) & (np.abs(m[..., 1]) <= np.float32(1e9))

    def set_state(self, slot, xy, anchor):
        """Load a map and its (h, w, 3) uint8 anchor frame, which also becomes the slot's current frame (eppm_cmap_set_state)."""
        xy = np.ascontiguousarray(xy, np.float32)
        a = np.ascontiguousarray(anchor, np.uint8)
        if xy.shape != (self.h, self.w, 2) or a.shape != (self.h, self.w, 3):
            raise EppmError(f"CorrespondenceMap.set_state: a ({self.h},{self.w},2) float32 map and a ({self.h},{self.w},3) uint8 anchor")
        self._call("set_state", int(slot), xy.ctypes.data, a.ctypes.data, self.w * 3)

    def set_layer(self, rgba, slot=0):
        """The slot's layer: (h, w, 4) uint8 RGBA with straight alpha, in the anchor frame's geometry; None: the default layer (the anchor
        frame with alpha 255)."""
        if rgba is None:
            self._call("set_layer", int(slot), None, 0)
            return
        a = np.ascontiguousarray(rgba, np.uint8)
        if a.shape != (self.h, self.w, 4):
            raise EppmError(f"CorrespondenceMap.set_layer: the layer must be ({self.h},{self.w},4) uint8")
        self._call("set_layer", int(slot), a.ctypes.data, self.w * 4)

    def render(self, slot=0):
        """(h, w, 3) uint8: the slot's layer composited over its current frame through its map."""
        return self._rgb("render", slot)

    def render_device(self, slot, d_rgba, pitch):
        self._call("render_device", int(slot), d_rgba, pitch)

    def age(self, slot=0):
        """Steps since the slot's anchor frame."""
        a = int(lib().eppm_cmap_age(self._f, int(slot)))
        if a < 0:
            raise EppmError(f"eppm_cmap_age: {lib().eppm_last_error().decode()}")
        return a


def ObjectsParams(**kw):
    """eppm_objects_params with the defaults of DESIGN.md section 20 (tau 1, iters 3, connectivity 8, min_area 16, max_objects 64,
    min_overlap 4)."""
    return _params(CObjectsParams, "eppm_objects_default_params", "object-detector parameter", **kw)


class ObjectDetector(_ClipObject):
    """Moving objects over the pairs of a context (eppm_objects_*): the connected components of the motion mask of
    image 1 (what moves against the camera), with a box, an area, a velocity and an id that survives from one pair to the next.  ctx: an
    EPPM or an EPPMBatch; one slot per pair of it.  Every step() works on the active pairs of the context's last
    compute_flow_bidirectional*; nothing is carried into an empty slot (new, or after reset(): the next id is 1) or across a pair flagged
    as a cut.  The detector is its own allocation on the context's device; close() frees it.  params: ObjectsParams' tau, iters,
    connectivity, min_area, max_objects and min_overlap."""
    _prefix = "objects"

    def __init__(self, ctx, size=None, slots=1, device=0, **params):
        """ctx None: a detector without a context, for step_frames on caller planes (eppm_objects_create_size): size = (h, w), `slots`
        slots."""
        self.params = ObjectsParams(**params)
        self._open(ctx, size, slots, device)

    def step_frames(self, slot, d_mask, d_flow, d_flow_bwd=None, d_occ2=None, cut=False):
        """eppm_objects_step_frames: the kernels alone for one slot on caller device planes (addresses), synchronous."""
        self._call("step_frames", int(slot), d_mask, d_flow, d_flow_bwd, d_occ2, int(bool(cut)))

    def _get(self, slot):
        n = int(self.params.max_objects)
        rec = (CObject * n)()
        cnt = CObjectsCounts()
        self._call("get", int(slot), n, rec, C.byref(cnt))
        return rec, cnt

    def objects(self, slot=0):
        """The slot's objects in label order: dicts of id, age, area, x0, y0, x1, y1, n_flow, sum_x, sum_y, sum_qu, sum_qv, and derived
        in float64 centroid (x, y) and velocity (u, v) in pixels per frame (None without a valid vector)."""
        rec, cnt = self._get(slot)
        return [object_record(rec[k]) for k in range(cnt.n)]

    def counts(self, slot=0):
        """dict n, n_found, n_components, next_id."""
        return self._get(slot)[1].as_dict()

    def labels(self, slot=0):
        """(h, w) uint8: per pixel of image 1 the index (1 .. n) of its object in objects(slot), 0 for none."""
        lab = np.empty((self.h, self.w), np.uint8)
        self._call("get_labels", int(slot), lab.ctypes.data)
        return lab

    def id_map(self, slot=0):
        """(h, w) int32: per pixel the id of its object, 0 for none."""
        rec, cnt = self._get(slot)
        lut = np.zeros(256, np.int32)
        for k in range(cnt.n):
            lut[k + 1] = rec[k].id
        return lut[self.labels(slot)]

    def state(self, slot=0):
        """(carried (h, w) uint8, prev_id, prev_age (256 int32 each), next_id): what the slot's next step starts from."""
        car = np.empty((self.h, self.w), np.uint8)
        pid, page = np.empty(256, np.int32), np.empty(256, np.int32)
        nxt = C.c_int32()
        self._call("get_state", int(slot), *[x.ctypes.data for x in (car, pid, page)], C.byref(nxt))
        return car, pid, page, int(nxt.value)

    def set_state(self, slot, carried, prev_id, prev_age, next_id):
        car = np.ascontiguousarray(carried, np.uint8)
        pid, page = np.ascontiguousarray(prev_id, np.int32), np.ascontiguousarray(prev_age, np.int32)
        if car.shape != (self.h, self.w) or pid.shape != (256,) or page.shape != (256,):
            raise EppmError(f"ObjectDetector.set_state: a ({self.h},{self.w}) uint8 plane and two tables of 256 int32")
        if not -2 ** 31 <= int(next_id) < 2 ** 31:
            raise EppmError("ObjectDetector.set_state: status 1: next_id is not an int32")
        self._call("set_state", int(slot), *[x.ctypes.data for x in (car, pid, page)], int(next_id))


def PlateParams(**kw):
    """eppm_plate_params with the defaults of DESIGN.md section 22 (tau 1, iters 3, margin_x 0, margin_y 0, grow 2, accept_invalid 0,
    thresh 40, n_max 64, min_count 2)."""
    return _params(CPlateParams, "eppm_plate_default_params", "background-plate parameter", **kw)


class BackgroundPlate(_ClipObject):
    """The scene behind the moving objects over the pairs of a context (eppm_plate_*): per slot a canvas in the
    coordinates of the clip's first frame that accumulates, pair by pair, what image 1 shows outside the grown motion mask, along the
    camera path the fits compose; and image 1 with its moving objects painted out from that canvas.  ctx: an EPPM or an EPPMBatch; one
    slot per pair of it.  Every step() works on the active pairs of the context's last compute_flow_bidirectional*: image 1 of the pair is
    accumulated, then the path advances to image 2 (a pair flagged as a cut: the path becomes the identity, the canvas is kept).  An empty
    slot (new, or after reset()) has no canvas and the identity as its path.  The plate is its own allocation on the context's device;
    close() frees it.  params: PlateParams' tau, iters, margin_x, margin_y, grow, accept_invalid, thresh, n_max and min_count."""
    _prefix = "plate"

    def __init__(self, ctx, size=None, slots=1, device=0, **params):
        """ctx None: a plate without a context, for step_frames / render_frames on caller planes (eppm_plate_create_size): size = (h, w),
        `slots` slots."""
        self.params = PlateParams(**params)
        self._open(ctx, size, slots, device)
        self.ch, self.cw = self.h + 2 * int(self.params.margin_y), self.w + 2 * int(self.params.margin_x)

    @staticmethod
    def _path(path):
        if path is None:
            return None, None
        p = np.ascontiguousarray(path, np.float64)
        if p.shape != (6,):
            raise EppmError("BackgroundPlate: a path is six numbers {a00, a01, a10, a11, tx, ty}")
        return p, p.ctypes.data

    def step_frames(self, slot, d_rgba, pitch, d_mask, path=None, cut=False):
        """eppm_plate_step_frames: the kernels alone for one slot on caller device planes (addresses), synchronous.  path: six float64 that
        become the slot's path for this step, None: the slot's own."""
        keep, ptr = self._path(path)
        self._call("step_frames", int(slot), d_rgba, int(pitch), d_mask, ptr, int(bool(cut)))

    def render(self, slot=0, ctx=None):
        """(image 1 of the slot's last stepped pair with its blocked pixels filled from the canvas: (h, w, 3) uint8; the fill bytes: (h, w)
        uint8, 0 free, 1 filled, 2 blocked and not filled)."""
        c = self.ctx if ctx is None else ctx
        out, fill = np.empty((self.h, self.w, 3), np.uint8), np.empty((self.h, self.w), np.uint8)
        self._call("render", c._ctx, int(slot), out.ctypes.data, self.w * 3, fill.ctypes.data)
        return out, fill

    def render_frames(self, slot, d_rgba, pitch, d_mask, path, d_rgba_out, out_pitch, d_fill):
        """eppm_plate_render_frames: the render alone on caller device planes (addresses) against the slot's canvas, synchronous."""
        keep, ptr = self._path(path)
        self._call("render_frames", int(slot), d_rgba, int(pitch), d_mask, ptr, d_rgba_out, int(out_pitch), d_fill)

    def render_frame(self, slot, frame, mask, path=None):
        """render_frames for host planes: an (h, w, 3) uint8 frame, its (h, w) uint8 mask and its path, uploaded, rendered and read back.
        Returns (frame with the blocked pixels filled, fill bytes)."""
        from .stages import Dev
        f = np.ascontiguousarray(frame, np.uint8)
        m = np.ascontiguousarray(mask, np.uint8)
        if f.shape != (self.h, self.w, 3) or m.shape != (self.h, self.w):
            raise EppmError(f"BackgroundPlate.render_frame: a ({self.h},{self.w},3) frame and a ({self.h},{self.w}) mask")
        rgba = np.zeros((self.h, self.w, 4), np.uint8)
        rgba[..., :3] = f
        bufs = [Dev(rgba.view(np.uint32)[..., 0]), Dev(m), Dev(shape=(self.h, self.w), dtype=np.uint32), Dev(shape=(self.h, self.w), dtype=np.uint8)]
        try:
            self.render_frames(slot, bufs[0].ptr, bufs[0].pitch, bufs[1].ptr, path, bufs[2].ptr, bufs[2].pitch, bufs[3].ptr)
            out = np.ascontiguousarray(bufs[2].get()).view(np.uint8).reshape(self.h, self.w, 4)[..., :3].copy()
            return out, bufs[3].get()
        finally:
            for b in bufs:
                b.free()

    def _get(self, slot, want_cov):
        rgb = np.empty((self.ch, self.cw, 3), np.uint8)
        cov = np.empty((self.ch, self.cw), np.uint8) if want_cov else None
        self._call("get", int(slot), rgb.ctypes.data, self.cw * 3, None if cov is None else cov.ctypes.data)
        return rgb, cov

    def plate(self, slot=0):
        """The canvas as an (h + 2*margin_y, w + 2*margin_x, 3) uint8 image; the clip's first frame sits at (margin_x, margin_y)."""
        return self._get(slot, False)[0]

    def coverage(self, slot=0):
        """Per canvas pixel min(n, 255): how often its value has been confirmed; 0: nothing seen there."""
        return self._get(slot, True)[1]

    def get_device(self, slot, d_rgba, pitch):
        self._call("get_device", int(slot), d_rgba, int(pitch))

    def mask(self, slot=0):
        """(h, w) uint8: the fit's mask of the slot's last step (0 moves with the camera, 1 moves on its own, 2 not valid)."""
        m = np.empty((self.h, self.w), np.uint8)
        self._call("get_mask", int(slot), m.ctypes.data)
        return m

    def path(self, slot=0):
        """The slot's camera path, frame 0 -> image 1 of the next pair: six float64 {a00, a01, a10, a11, tx, ty}."""
        p = np.empty(6, np.float64)
        self._call("get_path", int(slot), p.ctypes.data)
        return p

    def set_path(self, slot, path):
        keep, ptr = self._path(np.asarray(path))
        self._call("set_path", int(slot), ptr)

    def state(self, slot=0):
        """(ch, cw, 4) float32: per canvas pixel the running mean {R, G, B} and its count n."""
        st = np.empty((self.ch, self.cw, 4), np.float32)
        self._call("get_state", int(slot), st.ctypes.data)
        return st

    def set_state(self, slot, state):
        st = np.ascontiguousarray(state, np.float32)
        if st.shape != (self.ch, self.cw, 4):
            raise EppmError(f"BackgroundPlate.set_state: a ({self.ch},{self.cw},4) float32 array")
        self._call("set_state", int(slot), st.ctypes.data)


def _level(level):
    """a stop level as a plain int; anything that is not an integer is refused before the library is touched"""
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, np.integer)):
        raise EppmError(f"stop level must be an integer, not {level!r}")
    return int(level)


class _Context(_Handle):
    """What EPPM and EPPMBatch share word for word: the calls of the ABI that take a context of either kind."""
    _handle = "_ctx"

    def _need(self):
        """a context exists (EPPM: init has been called; a batch has one from its construction)"""

    # -- Y'CbCr 4:2:0 frames (eppm_amd.yuv): what the _yuv methods of both contexts share
    def _yuv_frames(self, frames, what):
        """(format, plane pointers, strides, the frames kept alive) of host YuvFrames of one format and of the context's size"""
        from . import yuv
        fmt, ptrs, strides, keep = yuv.frames_args(frames, what)
        if (keep[0].h, keep[0].w) != (self.h, self.w):
            raise EppmError(f"{what}: frames must be {self.w} x {self.h}")
        return fmt, ptrs, strides, keep

    def _yuv_devices(self, frames, what):
        """(plane pointers, pitches) of frames given as lists of stages.Dev planes of one pitch set and of the context's size"""
        from . import yuv
        for planes in frames:
            if (planes[0].h, planes[0].w) != (self.h, self.w):
                raise EppmError(f"{what}: frames must be {self.w} x {self.h}")
        return yuv.device_args(frames, what)

    def set_stop_level(self, level):
        """Draft mode (eppm_set_stop_level): the pyramid levels below `level` are upsampled edge-aware from the level
        above (one launch each) instead of being refined and smoothed; 0 (default): the full path.  Takes effect at the next compute; a
        batch: for every slot."""
        level = _level(level)
        self._need()
        check(lib().eppm_set_stop_level(self._ctx, level), "eppm_set_stop_level")

    def stop_level(self):
        self._need()
        return int(lib().eppm_stop_level(self._ctx))

    def set_occlusion_params(self, alpha=0.01, beta=0.5):
        """alpha, beta of the occlusion masks' forward-backward criterion (eppm_set_occlusion_params)."""
        self._need()
        check(lib().eppm_set_occlusion_params(self._ctx, alpha, beta), "eppm_set_occlusion_params")
        self._occ_params = (float(alpha), float(beta))

    def synchronize(self):
        self._need()
        check(lib().eppm_synchronize(self._ctx), "eppm_synchronize")

    def level_dims(self):
        self._need()
        out = []
        for l in range(lib().eppm_num_levels(self._ctx)):
            h, w = C.c_int(), C.c_int()
            check(lib().eppm_level_dims(self._ctx, l, C.byref(h), C.byref(w)), "eppm_level_dims")
            out.append((h.value, w.value))
        return out

    def enable_stage_timing(self, on=True):
        self._need()
        check(lib().eppm_enable_stage_timing(self._ctx, int(on)), "eppm_enable_stage_timing")

    def stage_times(self, clear=True):
        """[(stage name, ms)] for every set_data / compute_flow since the last clear (timing enabled)."""
        self._need()
        cap = 1 << 16
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = lib().eppm_stage_times(self._ctx, names, ms, cap)
        out = [(names[i].decode(), float(ms[i])) for i in range(n)]
        if clear:
            check(lib().eppm_clear_stage_times(self._ctx), "eppm_clear_stage_times")
        return out


class EPPM(_Context):
    """``init`` / ``set_data`` / ``compute_flow`` as in bao_flow_patchmatch_multiscale_cuda.h:36-44.

    Images are (h, w, 3) uint8 arrays in R,G,B order (the reference's ``unsigned char***``);
    flows are (h, w) float32 arrays (``float**``).
    """

    def __init__(self, device=0, params=None):
        self._ctx = C.c_void_p()
        self._device = device
        self._params = params
        self._pending_out = None
        self.h = self.w = 0

    # -- reference interface ---------------------------------------------------------------
    def init(self, *args):
        """init(h, w)  or  init(img1, img2, h, w)   (driver .cpp:106-157)"""
        if len(args) == 4:
            img1, img2, h, w = args
            self.init(h, w)
            self.set_data(img1, img2)
            return
        h, w = args
        self.close()
        ctx = C.c_void_p()
        check(lib().eppm_create(C.byref(ctx), int(h), int(w), int(self._device), C.byref(self._params) if self._params is not None else None), "eppm_create")
        self._ctx, self.h, self.w = ctx, int(h), int(w)
        self._occ_params = (0.01, 0.5)          # the new context's defaults

    def set_data(self, img1, img2):
        """RGB->RGBA, H2D, prefilter, pyramid, census (driver .cpp:159-168).  Returns True like the reference."""
        self._need()
        a = np.ascontiguousarray(img1, np.uint8)
        b = np.ascontiguousarray(img2, np.uint8)
        if a.shape != (self.h, self.w, 3) or b.shape != (self.h, self.w, 3):
            raise EppmError(f"set_data: images must be ({self.h},{self.w},3) uint8")
        check(lib().eppm_set_images(self._ctx, a.ctypes.data, b.ctypes.data, self.w * 3), "eppm_set_images")
        return True

    # -- streaming -------------------------------------------------------
    def push_frame(self, img):
        """Image 2 becomes image 1, img becomes image 2 (eppm_push_image): only img is uploaded and prepared."""
        self._need()
        a = np.ascontiguousarray(img, np.uint8)
        if a.shape != (self.h, self.w, 3):
            raise EppmError(f"push_frame: the image must be ({self.h},{self.w},3) uint8")
        check(lib().eppm_push_image(self._ctx, a.ctypes.data, self.w * 3), "eppm_push_image")

    # -- Y'CbCr 4:2:0 frames (eppm_amd.yuv): the context then holds what it holds after the RGB call on yuv.to_rgb ---
    def set_data_yuv(self, frame1, frame2):
        """set_data on two YuvFrames (eppm_yuv_set_images): the planes are uploaded as they are and converted on the device."""
        self._need()
        fmt, ptrs, strides, _keep = self._yuv_frames([frame1, frame2], "set_data_yuv")
        check(lib().eppm_yuv_set_images(self._ctx, C.byref(fmt), C.byref(ptrs, 0), C.byref(ptrs, 3 * C.sizeof(C.c_void_p)), strides), "eppm_yuv_set_images")
        return True

    def push_frame_yuv(self, frame):
        """push_frame on a YuvFrame (eppm_yuv_push_image)"""
        self._need()
        fmt, ptrs, strides, _keep = self._yuv_frames([frame], "push_frame_yuv")
        check(lib().eppm_yuv_push_image(self._ctx, C.byref(fmt), ptrs, strides), "eppm_yuv_push_image")

    def set_data_yuv_device(self, fmt, planes1, planes2):
        """planes1, planes2: the format's planes as stages.Dev buffers (eppm_yuv_set_images_device): read in stream order, no RGBA copy."""
        self._need()
        ptrs, pitches = self._yuv_devices([planes1, planes2], "set_data_yuv_device")
        check(lib().eppm_yuv_set_images_device(self._ctx, C.byref(fmt), C.byref(ptrs, 0), C.byref(ptrs, 3 * C.sizeof(C.c_void_p)), pitches),
              "eppm_yuv_set_images_device")

    def push_frame_yuv_device(self, fmt, planes):
        self._need()
        ptrs, pitches = self._yuv_devices([planes], "push_frame_yuv_device")
        check(lib().eppm_yuv_push_image_device(self._ctx, C.byref(fmt), ptrs, pitches), "eppm_yuv_push_image_device")

    def push_frame_device(self, d_rgba, pitch):
        self._need()
        check(lib().eppm_push_image_device(self._ctx, d_rgba, pitch), "eppm_push_image_device")

    def set_temporal(self, on=True):
        """Temporal mode (eppm_set_temporal): a compute after push_frame starts PatchMatch from the previous pair's result moved along its
        own motion; set_data starts a new clip."""
        self._need()
        check(lib().eppm_set_temporal(self._ctx, int(bool(on))), "eppm_set_temporal")

    def temporal_reset(self):
        """Drop the previous pair's fields: the next compute is a cold run (eppm_temporal_reset)."""
        self._need()
        check(lib().eppm_temporal_reset(self._ctx), "eppm_temporal_reset")

    def temporal_valid(self):
        self._need()
        return bool(lib().eppm_temporal_valid(self._ctx))

    def _out(self, out):
        if out is None:
            return np.empty((self.h, self.w), np.float32), np.empty((self.h, self.w), np.float32)
        u, v = out
        for a in (u, v):
            if a.shape != (self.h, self.w) or a.dtype != np.float32 or not a.flags.c_contiguous:
                raise EppmError(f"out planes must be C-contiguous ({self.h},{self.w}) float32")
        return u, v

    def compute_flow(self, out=None):
        """Returns (disp1_x, disp1_y) (driver .cpp:217-306); out=(u, v): write into these planes (registered planes are written
        by DMA directly, see host_register)."""
        self._need()
        u, v = self._out(out)
        check(lib().eppm_compute(self._ctx, u.ctypes.data, v.ctypes.data), "eppm_compute")
        return u, v

    def compute_flow_bidirectional(self, alpha=None, beta=None):
        """(u, v, bu, bv, occ1, occ2): the forward flow (== compute_flow), the backward flow (image 2 -> image 1) and the uint8
        occlusion masks of image 1's / image 2's pixels (0 consistent, 1 inconsistent, 2 leaves the frame, 3 unknown vector).
        alpha / beta given: set the criterion's parameters first (eppm_set_occlusion_params; the other keeps its value)."""
        self._need()
        if alpha is not None or beta is not None:
            a0, b0 = getattr(self, "_occ_params", (0.01, 0.5))
            self._occ_params = (a0 if alpha is None else float(alpha), b0 if beta is None else float(beta))
            self.set_occlusion_params(*self._occ_params)
        f = [np.empty((self.h, self.w), np.float32) for _ in range(4)]
        o = [np.empty((self.h, self.w), np.uint8) for _ in range(2)]
        check(lib().eppm_compute_bidirectional(self._ctx, *[a.ctypes.data for a in f + o]), "eppm_compute_bidirectional")
        return (*f, *o)

    def compute_flow_bidirectional_device(self, d_flow=None, d_flow_bwd=None, d_occ1=None, d_occ2=None):
        """eppm_compute_bidirectional_device: asynchronous, device addresses (or None) of the two float2 flows and the two masks."""
        self._need()
        check(lib().eppm_compute_bidirectional_device(self._ctx, d_flow, d_flow_bwd, d_occ1, d_occ2), "eppm_compute_bidirectional_device")

    def interpolate(self, times):
        """Frames at the given times between image 1 (t = 0) and image 2 (t = 1) from the last compute_flow_bidirectional
        (eppm_interpolate): a list of (h, w, 3) uint8 R,G,B arrays."""
        self._need()
        ts = _times(times)
        out = [np.empty((self.h, self.w, 3), np.uint8) for _ in range(len(ts))]
        ptrs = (C.c_void_p * len(out))(*[a.ctypes.data for a in out])
        check(lib().eppm_interpolate(self._ctx, len(ts), ts, ptrs, self.w * 3), "eppm_interpolate")
        return out

    def interpolate_device(self, times, d_ptrs, pitch):
        """eppm_interpolate_device: asynchronous on the context's stream; d_ptrs: one device RGBA plane (pitch bytes per row) per time."""
        self._need()
        ts = _times(times)
        if len(d_ptrs) != len(ts):
            raise EppmError("interpolate_device: one device plane per time")
        ptrs = (C.c_void_p * len(ts))(*d_ptrs)
        check(lib().eppm_interpolate_device(self._ctx, len(ts), ts, ptrs, pitch), "eppm_interpolate_device")

    def motion_blur(self, shutter=0.5, max_radius=16, taps=8, frame=0):
        """The frame as a camera with an open shutter would have recorded it (eppm_motion_blur): an (h, w, 3) uint8
        R,G,B array.  frame=0: image 1 along the forward flow, after any compute of the current images; frame=1: image 2 along the backward
        flow, after compute_flow_bidirectional.  shutter: the open fraction of the frame interval; max_radius: the longest half-vector
        in pixels; taps: taps to each side of a pixel."""
        self._need()
        p = MBlurParams(shutter=shutter, max_radius=max_radius, taps=taps)
        out = np.empty((self.h, self.w, 3), np.uint8)
        check(lib().eppm_motion_blur(self._ctx, C.byref(p), int(frame), out.ctypes.data, self.w * 3), "eppm_motion_blur")
        return out

    def motion_blur_device(self, d_rgba, pitch, shutter=0.5, max_radius=16, taps=8, frame=0):
        """eppm_motion_blur_device: asynchronous on the context's stream; d_rgba: a device RGBA plane of pitch bytes per row."""
        self._need()
        p = MBlurParams(shutter=shutter, max_radius=max_radius, taps=taps)
        check(lib().eppm_motion_blur_device(self._ctx, C.byref(p), int(frame), d_rgba, pitch), "eppm_motion_blur_device")

    def rolling_shutter(self, readout=0.5, anchor=0.5, iters=3, axis=0, frame=0):
        """The frame as a global shutter would have recorded it (eppm_rolling_shutter): an (h, w, 3) uint8 R,G,B
        array.  frame=0: image 1 along the forward flow, after any compute of the current images; frame=1: image 2 along the backward
        flow, after compute_flow_bidirectional.  readout: the share of the frame interval the sensor takes to read a frame (negative: last
        line first); anchor: the position along the axis whose sampling time is the frame's; iters: fixed-point steps; axis: 0 rows are
        read one after another, 1 columns."""
        self._need()
        p = RSParams(readout=readout, anchor=anchor, iters=iters, axis=axis)
        out = np.empty((self.h, self.w, 3), np.uint8)
        check(lib().eppm_rolling_shutter(self._ctx, C.byref(p), int(frame), out.ctypes.data, self.w * 3), "eppm_rolling_shutter")
        return out

    def rolling_shutter_device(self, d_rgba, pitch, readout=0.5, anchor=0.5, iters=3, axis=0, frame=0):
        """eppm_rolling_shutter_device: asynchronous on the context's stream; d_rgba: a device RGBA plane of pitch bytes per row."""
        self._need()
        p = RSParams(readout=readout, anchor=anchor, iters=iters, axis=axis)
        check(lib().eppm_rolling_shutter_device(self._ctx, C.byref(p), int(frame), d_rgba, pitch), "eppm_rolling_shutter_device")

    def compute_flow_color(self, max_disp=(20.0, 20.0)):
        """The optional color_flow output of compute_flow (driver .cpp:308-314): (h, w, 3) uint8 R,G,B of the last flow."""
        self._need()
        rgb = np.empty((self.h, self.w, 3), np.uint8)
        check(lib().eppm_compute_color(self._ctx, rgb.ctypes.data, self.w * 3, max_disp[0], max_disp[1]), "eppm_compute_color")
        return rgb

    def compute_flow_begin(self, out=None):
        """Enqueue compute_flow and its device-to-host copy, return at once (eppm_compute_begin; with out=(u, v):
        eppm_compute_begin_into, which lets registered planes receive the copy directly)."""
        self._need()
        if out is None:
            check(lib().eppm_compute_begin(self._ctx), "eppm_compute_begin")
        else:
            u, v = self._out(out)
            self._pending_out = (u, v)      # the copy engine writes these planes until compute_flow_end: keep them alive
            check(lib().eppm_compute_begin_into(self._ctx, u.ctypes.data, v.ctypes.data), "eppm_compute_begin_into")

    def compute_flow_end(self, out=None):
        """Wait for compute_flow_begin; returns (disp1_x, disp1_y)."""
        self._need()
        u, v = self._out(out)
        check(lib().eppm_compute_end(self._ctx, u.ctypes.data, v.ctypes.data), "eppm_compute_end")
        self._pending_out = None
        return u, v

    # -- device-resident variants (no PCIe in the timed region) ----------------------------
    def set_data_device(self, d_rgba1, d_rgba2, pitch):
        self._need()
        check(lib().eppm_set_images_device(self._ctx, d_rgba1, d_rgba2, pitch), "eppm_set_images_device")

    def compute_flow_device(self, d_flow=None):
        self._need()
        check(lib().eppm_compute_device(self._ctx, d_flow), "eppm_compute_device")

    def set_stream(self, hip_stream):
        self._need()
        check(lib().eppm_set_stream(self._ctx, hip_stream), "eppm_set_stream")

    # -- introspection ---------------------------------------------------------------------
    def plane(self, name, level):
        self._need()
        dims = self.level_dims()
        if name not in _PLANE_DTYPES or not 0 <= level < len(dims):
            raise EppmError(f"plane({name!r}, {level}): unknown plane or level")
        h, w = dims[level]
        a = np.empty((h, w), _PLANE_DTYPES[name])
        check(lib().eppm_get_plane(self._ctx, name.encode(), level, a.ctypes.data, a.nbytes), "eppm_get_plane")
        return a

    def _need(self):
        if not self._ctx:
            raise EppmError("EPPM: init(h, w) has not been called")


class EPPMBatch(_Context):
    """A batch of independent pairs of one size on one GPU (eppm_create_batch): every kernel launch of the path covers all
    active pairs.  ``set_data(pairs)`` / ``compute_flow()`` mirror the single-pair class; each pair's flow is bit-identical
    to the single-pair result."""

    def __init__(self, h, w, npairs, device=0, params=None):
        self._ctx = C.c_void_p()
        check(lib().eppm_create_batch(C.byref(self._ctx), int(h), int(w), int(device),
                                      C.byref(params) if params is not None else None, int(npairs)), "eppm_create_batch")
        self.h, self.w, self.npairs, self.n = int(h), int(w), int(npairs), 0
        self._pending_out = None

    @staticmethod
    def _ptrs(arrs):
        return (C.c_void_p * len(arrs))(*[a.ctypes.data if hasattr(a, "ctypes") else a for a in arrs])

    def set_data(self, pairs):
        """pairs: up to npairs (img1, img2) tuples of (h, w, 3) uint8 arrays."""
        a = [np.ascontiguousarray(p[0], np.uint8) for p in pairs]
        b = [np.ascontiguousarray(p[1], np.uint8) for p in pairs]
        for x in a + b:
            if x.shape != (self.h, self.w, 3):
                raise EppmError(f"set_data: images must be ({self.h},{self.w},3) uint8")
        check(lib().eppm_batch_set_images(self._ctx, len(pairs), self._ptrs(a), self._ptrs(b), self.w * 3), "eppm_batch_set_images")
        self.n = len(pairs)

    def set_data_device(self, d1, d2, pitch):
        """d1, d2: lists of device addresses of RGBA planes."""
        check(lib().eppm_batch_set_images_device(self._ctx, len(d1), self._ptrs(list(d1)), self._ptrs(list(d2)), pitch), "eppm_batch_set_images_device")
        self.n = len(d1)

    # -- batch streaming: one clip per slot ----------------------------------
    @staticmethod
    def _cuts(new_clip, n):
        if new_clip is None:
            return None
        if len(new_clip) != n:
            raise EppmError("new_clip: one flag per frame")
        return (C.c_uint8 * n)(*[int(bool(x)) for x in new_clip])

    def push_frames(self, frames, new_clip=None):
        """Slot k's image 2 becomes its image 1 and frames[k] its image 2 (eppm_batch_push_images): only the new frames are uploaded and
        prepared.  One frame per active pair; new_clip[k] true: frames[k] is the first frame of another clip (the pair across the cut and
        the clip's first pair are cold runs)."""
        a = [np.ascontiguousarray(f, np.uint8) for f in frames]
        for x in a:
            if x.shape != (self.h, self.w, 3):
                raise EppmError(f"push_frames: images must be ({self.h},{self.w},3) uint8")
        check(lib().eppm_batch_push_images(self._ctx, len(a), self._ptrs(a), self.w * 3, self._cuts(new_clip, len(a))), "eppm_batch_push_images")

    # -- Y'CbCr 4:2:0 frames (eppm_amd.yuv) ---------------------------------------
    def set_data_yuv(self, pairs):
        """pairs: up to npairs (frame1, frame2) tuples of YuvFrames of one format (eppm_yuv_batch_set_images)."""
        n = len(pairs)
        fmt, ptrs, strides, _keep = self._yuv_frames([p[0] for p in pairs] + [p[1] for p in pairs], "set_data_yuv")
        check(lib().eppm_yuv_batch_set_images(self._ctx, C.byref(fmt), n, C.byref(ptrs, 0), C.byref(ptrs, 3 * n * C.sizeof(C.c_void_p)), strides),
              "eppm_yuv_batch_set_images")
        self.n = n

    def push_frames_yuv(self, frames, new_clip=None):
        """push_frames on one YuvFrame per active pair (eppm_yuv_batch_push_images)"""
        fmt, ptrs, strides, _keep = self._yuv_frames(list(frames), "push_frames_yuv")
        check(lib().eppm_yuv_batch_push_images(self._ctx, C.byref(fmt), len(frames), ptrs, strides, self._cuts(new_clip, len(frames))),
              "eppm_yuv_batch_push_images")

    def set_data_yuv_device(self, fmt, planes1, planes2):
        """planes1, planes2: per pair, the format's planes as stages.Dev buffers (eppm_yuv_batch_set_images_device)."""
        n = len(planes1)
        ptrs, pitches = self._yuv_devices(list(planes1) + list(planes2), "set_data_yuv_device")
        check(lib().eppm_yuv_batch_set_images_device(self._ctx, C.byref(fmt), n, C.byref(ptrs, 0), C.byref(ptrs, 3 * n * C.sizeof(C.c_void_p)), pitches),
              "eppm_yuv_batch_set_images_device")
        self.n = n

    def push_frames_yuv_device(self, fmt, planes, new_clip=None):
        ptrs, pitches = self._yuv_devices(list(planes), "push_frames_yuv_device")
        check(lib().eppm_yuv_batch_push_images_device(self._ctx, C.byref(fmt), len(planes), ptrs, pitches, self._cuts(new_clip, len(planes))),
              "eppm_yuv_batch_push_images_device")

    def push_frames_device(self, ptrs, pitch, new_clip=None):
        """ptrs: one device address of an RGBA plane per active pair (eppm_batch_push_images_device)."""
        ptrs = list(ptrs)
        check(lib().eppm_batch_push_images_device(self._ctx, len(ptrs), self._ptrs(ptrs), pitch, self._cuts(new_clip, len(ptrs))),
              "eppm_batch_push_images_device")

    def set_temporal(self, on=True):
        """Temporal mode per slot (eppm_batch_set_temporal): after push_frames a slot's compute starts PatchMatch from the slot's previous
        pair moved along its own motion; set_data starts a new clip in every slot."""
        check(lib().eppm_batch_set_temporal(self._ctx, int(bool(on))), "eppm_batch_set_temporal")

    def temporal_valid(self, pair):
        return bool(lib().eppm_batch_temporal_valid(self._ctx, int(pair)))

    def temporal_reset(self, pair=None):
        """The slot's next compute is a cold run; pair=None: every slot's (eppm_batch_temporal_reset)."""
        check(lib().eppm_batch_temporal_reset(self._ctx, -1 if pair is None else int(pair)), "eppm_batch_temporal_reset")

    def _outs(self, out=None):
        if out is not None:
            u, v = [o[0] for o in out], [o[1] for o in out]
            for a in u + v:
                if a.shape != (self.h, self.w) or a.dtype != np.float32 or not a.flags.c_contiguous:
                    raise EppmError(f"out planes must be C-contiguous ({self.h},{self.w}) float32")
            if len(u) < self.n:
                raise EppmError("out: one (u, v) per active pair")
            return u[:self.n], v[:self.n]
        u = [np.empty((self.h, self.w), np.float32) for _ in range(self.n)]
        v = [np.empty((self.h, self.w), np.float32) for _ in range(self.n)]
        return u, v

    def compute_flow(self, out=None):
        """[(u, v)] for the active pairs; out: list of (u, v) planes to write into (registered planes receive the DMA directly)."""
        u, v = self._outs(out)
        check(lib().eppm_batch_compute(self._ctx, self._ptrs(u), self._ptrs(v)), "eppm_batch_compute")
        return list(zip(u, v))

    def compute_flow_bidirectional(self):
        """[(u, v, bu, bv, occ1, occ2)] for the active pairs (eppm_batch_compute_bidirectional); see EPPM.compute_flow_bidirectional."""
        f = [[np.empty((self.h, self.w), np.float32) for _ in range(self.n)] for _ in range(4)]
        o = [[np.empty((self.h, self.w), np.uint8) for _ in range(self.n)] for _ in range(2)]
        check(lib().eppm_batch_compute_bidirectional(self._ctx, *[self._ptrs(t) for t in f + o]), "eppm_batch_compute_bidirectional")
        return list(zip(*f, *o))

    def compute_flow_bidirectional_device(self):
        """eppm_compute_bidirectional_device on every active pair: asynchronous, the results stay in the context (plane(), interpolate(),
        Tracker, TemporalFilter)."""
        check(lib().eppm_compute_bidirectional_device(self._ctx, None, None, None, None), "eppm_compute_bidirectional_device")

    def interpolate(self, times):
        """[[frame at times[k] for k] for each active pair] after compute_flow_bidirectional (eppm_batch_interpolate)."""
        ts = _times(times)
        out = [[np.empty((self.h, self.w, 3), np.uint8) for _ in range(len(ts))] for _ in range(self.n)]
        flat = [a for row in out for a in row]
        check(lib().eppm_batch_interpolate(self._ctx, len(ts), ts, self._ptrs(flat), self.w * 3), "eppm_batch_interpolate")
        return out

    def motion_blur(self, shutter=0.5, max_radius=16, taps=8, frame=0):
        """[blurred frame for each active pair] (eppm_batch_motion_blur); see EPPM.motion_blur."""
        p = MBlurParams(shutter=shutter, max_radius=max_radius, taps=taps)
        out = [np.empty((self.h, self.w, 3), np.uint8) for _ in range(self.n)]
        check(lib().eppm_batch_motion_blur(self._ctx, C.byref(p), int(frame), self._ptrs(out), self.w * 3), "eppm_batch_motion_blur")
        return out

    def rolling_shutter(self, readout=0.5, anchor=0.5, iters=3, axis=0, frame=0):
        """[corrected frame for each active pair] (eppm_batch_rolling_shutter); see EPPM.rolling_shutter."""
        p = RSParams(readout=readout, anchor=anchor, iters=iters, axis=axis)
        out = [np.empty((self.h, self.w, 3), np.uint8) for _ in range(self.n)]
        check(lib().eppm_batch_rolling_shutter(self._ctx, C.byref(p), int(frame), self._ptrs(out), self.w * 3), "eppm_batch_rolling_shutter")
        return out

    def compute_flow_device(self, d_flows=None):
        check(lib().eppm_batch_compute_device(self._ctx, self._ptrs(list(d_flows)) if d_flows is not None else None), "eppm_batch_compute_device")

    def compute_flow_begin(self, out=None):
        if out is None:
            check(lib().eppm_compute_begin(self._ctx), "eppm_compute_begin")
        else:
            u, v = self._outs(out)
            self._pending_out = (u, v)      # the copy engine writes these planes until compute_flow_end: keep them alive
            check(lib().eppm_batch_compute_begin_into(self._ctx, self._ptrs(u), self._ptrs(v)), "eppm_batch_compute_begin_into")

    def compute_flow_end(self, out=None):
        u, v = self._outs(out)
        check(lib().eppm_batch_compute_end(self._ctx, self._ptrs(u), self._ptrs(v)), "eppm_batch_compute_end")
        self._pending_out = None
        return list(zip(u, v))

    def plane(self, pair, name, level):
        hh, ww = self.level_dims()[level]
        a = np.empty((hh, ww), _PLANE_DTYPES[name])
        check(lib().eppm_batch_get_plane(self._ctx, int(pair), name.encode(), level, a.ctypes.data, a.nbytes), "eppm_batch_get_plane")
        return a


def __getattr__(name):
    """The clip drivers and their helpers lived in this module before sequences.py: eppm_amd.api.<name> still finds what is defined there."""
    from . import sequences
    obj = getattr(sequences, name, None)
    if getattr(obj, "__module__", None) != sequences.__name__:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    return obj
