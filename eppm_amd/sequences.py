"""The clip drivers: whole clips, one or many, through a streaming context and a per-clip stage object.

_Run is the streaming loop; every driver below it supplies a stage factory, its compute call and what it reads per slot."""
import numpy as np

from . import io, yuv
from ._lib import EppmError
from .api import (EPPM, BackgroundPlate, CorrespondenceMap, CutDetector, DefectFilter, Deflicker, Deinterlacer, EPPMBatch, ObjectDetector, Stabilizer, TemporalFilter,
                  Tracker, _level)


def _sequence_plan(lengths, slots):
    """The schedule of flow_sequences, a pure function: clips of the given lengths (frames, >= 2 each) through min(slots, len(lengths))
    slots.  Yields one list per step with one (clip, frame, new_clip, keep) per slot: frame `frame` of clip `clip` becomes the slot's image
    2 at that step.  Step 0 is the set_data step (image 1 is the clip's frame 0, frame = 1); every later step is a push.  keep: the pair
    the slot then holds is (frame - 1, frame) of `clip` and its flow is wanted.  A slot whose clip has ended takes the next clip of the
    queue (frame 0 with new_clip set; the pair across the cut is not kept); a slot with nothing left is fed its last frame again."""
    lengths = [int(n) for n in lengths]
    if not lengths or min(lengths) < 2:
        raise EppmError("flow_sequences: every clip needs at least two frames")
    n = min(int(slots), len(lengths))
    if n < 1:
        raise EppmError("flow_sequences: at least one slot")
    cur = [[k, 1] for k in range(n)]            # per slot: its clip and the frame that is its image 2
    queue = list(range(n, len(lengths)))
    yield [(k, 1, False, True) for k in range(n)]
    while queue or any(f + 1 < lengths[c] for c, f in cur):
        step = []
        for slot in cur:
            c, f = slot
            if f + 1 < lengths[c]:
                slot[1] = f + 1
                step.append((c, f + 1, False, True))
            elif queue:
                slot[0], slot[1] = queue.pop(0), 0
                step.append((slot[0], 0, True, False))
            else:
                step.append((c, f, False, False))
        yield step


def _bidirectional_device(run):
    run.e.compute_flow_bidirectional_device()


class _RgbView:
    """The frames of a clip of YuvFrames as a driver reads them outside the context: yuv.to_rgb(frame), the bytes the context holds
    (DESIGN.md section 25), made when asked for"""

    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [yuv.to_rgb(f) for f in self.frames[k]]
        return yuv.to_rgb(self.frames[k])

    def __iter__(self):
        return (yuv.to_rgb(f) for f in self.frames)


def _clip_lists(who, clips):
    """(the clips as lists, whether their frames are YuvFrames).  Every clip is read ONCE, here: a clip may be a generator (yuv.read_y4m
    is one).  A run with a YuvFrame in it must be YuvFrames throughout, of one format and one size."""
    clips = [list(clip) for clip in clips]
    if not any(isinstance(f, yuv.YuvFrame) for clip in clips for f in clip):
        return clips, False
    first = next(f for clip in clips for f in clip)
    for clip in clips:
        for f in clip:
            if not isinstance(f, yuv.YuvFrame) or f.fmt.as_dict() != first.fmt.as_dict() or (f.h, f.w) != (first.h, first.w):
                raise EppmError(f"{who}: all frames of a run must be YuvFrames of one format and size")
    return clips, True


class _Run:
    """One streaming run of clips through a context, a stage object and a cut detector: the protocol every clip driver shares.

        with _Run(who, clips, slots, ...) as run:        # checks, then opens the context, the stage and the detector
            ...                                          # the driver's first entries; run.e, run.stage, run.det, run.clips, run.h, run.w
            for slot, c, f, new_clip, keep in run:       # per step: feed, compute, auto-cut, stage.step; then one item per slot
                ...                                      # what the driver reads of the slot; run.res[slot], run.found[slot], run.last
                                                         # leaving the block, by an exception too, closes detector, stage and context

    clips: a list of clips of (h, w, 3) uint8 frames.  slots None: the ONE clip of the list through an EPPM (set_data / push_frame), the
    schedule being _sequence_plan's for one clip in one slot: its n - 1 pairs, every one kept.  slots a number: an EPPMBatch of
    min(slots, len(clips)) slots (set_data / push_frames) on _sequence_plan's schedule.  An item says that frame f of clip c has become
    the slot's image 2; new_clip: the slot has taken clip c from the queue and f is 0 (the pair across the change is not kept, and the
    slot's cut flag was set for the step); keep: the slot holds the pair (f - 1, f) of clip c.

    stop_level None: set_stop_level is not called.  stage: a factory, stage(context), of the object that is stepped once per step with
    the cut flags: None for one clip without auto_cut, else one flag per slot, the schedule's new_clip ORed with the detector's verdict.
    A driver that opens run.stage itself (the tracker, which needs a computed pair) steps it itself; it is closed here.  auto_cut: a
    CutDetector(context, **cut_params) is stepped after every compute, its verdicts are run.found (None without auto_cut), and every
    detected slot's next compute is a cold run (temporal_reset), so the pair across the cut leaves no prior.  compute(run): the step's
    compute call; run.res is its result per slot.  hand_over: the stage outlives the run: after a run without an exception it stays open
    and is the caller's to close; after an exception it is closed here, before the detector.  step_args: None, or step_args(step), the
    keyword arguments stage.step gets besides the cut flags, from the step's list of (clip, frame, new_clip, keep)."""

    def __init__(self, who, clips, slots, params, temporal, stop_level, stage=None, auto_cut=False, cut_params=None, compute=_bidirectional_device,
                 hand_over=False, step_args=None):
        clips, is_yuv = _clip_lists(who, clips)
        self.yuv = clips if is_yuv else None       # clips of YuvFrames go through the context's _yuv methods; run.clips: their RGB form
        if is_yuv:
            self.clips = [_RgbView(clip) for clip in clips]
        else:
            self.clips = [[np.ascontiguousarray(f, np.uint8) for f in clip] for clip in clips]
        self.single = slots is None
        if self.single and len(self.clips[0]) < 2:
            raise EppmError(f"{who}: at least two frames")
        if self.yuv is not None:
            self.h, self.w = self.yuv[0][0].h, self.yuv[0][0].w
        else:
            self.h, self.w, _ = self.clips[0][0].shape
        self.steps = list(_sequence_plan([len(c) for c in self.clips], 1 if self.single else slots))
        self.level = None if stop_level is None else _level(stop_level)
        self.params, self.temporal, self.make_stage, self.compute, self.hand_over = params, temporal, stage, compute, hand_over
        self.step_args = step_args
        self.cut_params = dict(cut_params or {}) if auto_cut else None
        self.e = self.stage = self.det = self.res = self.found = None
        self.last = False

    def __enter__(self):
        try:
            if self.single:
                self.e = EPPM(params=self.params)
                self.e.init(self.h, self.w)
            else:
                self.e = EPPMBatch(self.h, self.w, len(self.steps[0]), params=self.params)
            self.e.set_temporal(self.temporal)
            if self.level is not None:
                self.e.set_stop_level(self.level)
            if self.make_stage is not None:
                self.stage = self.make_stage(self.e)
            if self.cut_params is not None:
                self.det = CutDetector(self.e, **self.cut_params)
        except BaseException:
            self._close(True)
            raise
        return self

    def __iter__(self):
        e, clips = self.e, self.clips
        for t, step in enumerate(self.steps):
            self.last = t == len(self.steps) - 1
            if self.yuv is not None and t == 0:
                pairs = [(self.yuv[c][0], self.yuv[c][1]) for c, _, _, _ in step]
                e.set_data_yuv(*pairs[0]) if self.single else e.set_data_yuv(pairs)
            elif self.yuv is not None:
                frames = [self.yuv[c][f] for c, f, _, _ in step]
                e.push_frame_yuv(frames[0]) if self.single else e.push_frames_yuv(frames, [new_clip for _, _, new_clip, _ in step])
            elif t == 0:
                pairs = [(clips[c][0], clips[c][1]) for c, _, _, _ in step]
                e.set_data(*pairs[0]) if self.single else e.set_data(pairs)
            else:
                frames = [clips[c][f] for c, f, _, _ in step]
                e.push_frame(frames[0]) if self.single else e.push_frames(frames, [new_clip for _, _, new_clip, _ in step])
            res = self.compute(self)
            self.res = [res] if self.single else res
            flags = None if self.single else [new_clip for _, _, new_clip, _ in step]
            if self.det is not None:
                self.det.step()
                self.found = self.det.cuts()
                for slot, cut in enumerate(self.found):
                    if cut:
                        e.temporal_reset() if self.single else e.temporal_reset(slot)
                flags = self.found if flags is None else [a or b for a, b in zip(flags, self.found)]
            if self.make_stage is not None and self.step_args is not None:
                self.stage.step(flags, **self.step_args(step))
            elif self.make_stage is not None:
                self.stage.step(flags)
            for slot, (c, f, new_clip, keep) in enumerate(step):
                yield slot, c, f, new_clip, keep

    def __exit__(self, exc_type, exc, tb):
        self._close(exc_type is not None)

    def _close(self, failed):
        order = [self.det, self.stage, self.e]
        if self.hand_over:
            order = [self.stage, self.det, self.e] if failed else [self.det, self.e]
        for x in order:
            if x is not None:
                x.close()


_CUT_KEYS = ("lost_permille", "residual_max")
_DEFECT_KEYS = ("detect", "agree", "radius", "grow")
_DEFLICKER_KEYS = ("cell", "iters", "reject", "tau", "keep", "n_min")
_DEINT_KEYS = ("thresh", "use_occ")
_CMAP_KEYS = ("thresh", "tear", "use_occ")
_OBJECTS_KEYS = ("tau", "iters", "connectivity", "min_area", "max_objects", "min_overlap")
_PLATE_KEYS = ("tau", "iters", "margin_x", "margin_y", "grow", "accept_invalid", "thresh", "n_max", "min_count")


def _split(kw, keys, who, auto_cut=True):
    """the keyword arguments of a driver: those in `keys` go to its stage object, CutDetector's to the detector; without auto_cut the
    detector's are refused in the name of `who`"""
    kw = dict(kw)
    own = {k: kw.pop(k) for k in keys if k in kw}
    cut = {k: kw.pop(k) for k in _CUT_KEYS if k in kw}
    if kw:
        raise TypeError(f"unknown parameter {sorted(kw)[0]}")
    if cut and not auto_cut:
        raise TypeError(f"{who}: lost_permille and residual_max need auto_cut=True")
    return own, cut


def detect_cuts(frames, params=None, stop_level=0, **cut_params):
    """Scene cuts of a clip ((h, w, 3) uint8 frames): one streaming context, one bidirectional call on the device and one CutDetector step
    per consecutive pair.  Returns (cuts, stats): one bool and one record (CutDetector.stats) per pair; cuts[k] true: frame k + 1 starts
    another shot.  After a detected cut the next pair is a cold run.  cut_params: CutDetector's lost_permille and residual_max."""
    cuts, stats = [], []
    with _Run("detect_cuts", [frames], None, params, True, _level(stop_level), auto_cut=True, cut_params=cut_params) as run:
        for _ in run:
            cuts.append(run.found[0])
            stats.append(run.det.stats(0))
    return cuts, stats


def _flows(who, clips, slots, params, temporal, bidirectional, stop_level, auto_cut, cut_params):
    """flow_sequence(s): (flows, cuts), one list per clip each"""
    def compute(run):
        return run.e.compute_flow_bidirectional() if bidirectional or auto_cut else run.e.compute_flow()
    with _Run(who, clips, slots, params, temporal, stop_level, None, auto_cut, cut_params, compute) as run:
        out, cuts = [[] for _ in run.clips], [[] for _ in run.clips]
        for slot, c, _, _, keep in run:
            if keep:
                out[c].append(run.res[slot] if bidirectional else run.res[slot][:2])
                if auto_cut:
                    cuts[c].append(run.found[slot])
    return out, cuts


def flow_sequence(frames, params=None, temporal=True, bidirectional=False, stop_level=0, auto_cut=False, **cut_params):
    """The flows of the consecutive pairs of a clip ((h, w, 3) uint8 frames) through ONE context: the first pair by set_data, every later
    frame by push_frame (only the new frame is uploaded and prepared), with temporal mode (each pair's PatchMatch starts from the previous
    pair's result moved along its motion) unless temporal=False.  Returns a list of (u, v), or of (u, v, bu, bv, occ1, occ2) with
    bidirectional=True.  Memory does not grow with the clip.  stop_level: draft mode (EPPM.set_stop_level).  auto_cut=True: every pair is
    computed bidirectionally (its forward flow is compute_flow's) and a CutDetector (cut_params: its lost_permille / residual_max) decides
    whether it crosses a scene cut; the pair after a cut is a cold run.  Returns (flows, cuts) then: one bool per pair, and the flow of a
    cut pair is of no use."""
    out, cuts = _flows("flow_sequence", [frames], None, params, temporal, bidirectional, _level(stop_level), auto_cut, cut_params)
    return (out[0], cuts[0]) if auto_cut else out[0]


def flow_sequences(clips, slots=8, params=None, temporal=True, bidirectional=False, stop_level=0, auto_cut=False, **cut_params):
    """flow_sequence for many clips at once: any number of clips of one frame size and of any lengths (two frames at least) through ONE
    batch context of min(slots, len(clips)) slots, every slot advanced by one frame per step (push_frames; temporal mode per slot unless
    temporal=False).  A slot whose clip ends takes the next clip in the queue.  Returns one list of flows per clip, in the order given, each
    what flow_sequence(clip) returns.  stop_level: draft mode (EPPMBatch.set_stop_level).  auto_cut=True: flow_sequence's, per slot; returns
    (flows, cuts), one list per clip each."""
    out, cuts = _flows("flow_sequences", clips, slots, params, temporal, bidirectional, _level(stop_level), auto_cut, cut_params)
    return (out, cuts) if auto_cut else out


def motion_blur_sequence(frames, params=None, shutter=0.5, max_radius=16, taps=8, temporal=True, stop_level=0):
    """A clip ((h, w, 3) uint8 frames) with a synthetic shutter (EPPM.motion_blur): one streaming context --
    set_data, then push_frame --, a forward-only compute per pair and its image 1 blurred along the forward flow; the last pair is computed
    bidirectionally and gives the clip's last frame too, blurred along the backward flow.  Returns len(frames) frames.  Memory does not grow
    with the clip.  params: the flow's eppm Params; temporal / stop_level: the flow's temporal and draft modes."""
    blur = dict(shutter=shutter, max_radius=max_radius, taps=taps)
    out = []

    def compute(run):
        return run.e.compute_flow_bidirectional_device() if run.last else run.e.compute_flow()
    with _Run("motion_blur_sequence", [frames], None, params, temporal, _level(stop_level), compute=compute) as run:
        for _ in run:
            out.append(run.e.motion_blur(frame=0, **blur))
            if run.last:
                out.append(run.e.motion_blur(frame=1, **blur))
    return out


def _rolling_shutter(who, clips, slots, rs, params, temporal, stop_level, auto_cut, cut_params):
    """rolling_shutter_sequence(s): one list of frames per clip.  Per clip, with c the pair's cut flag:

        fallback = frames[0]
        for each pair (k-1, k):
            out[k-1] = fallback      if c else rolling_shutter(frame=0)
            fallback = frames[k]     if c else rolling_shutter(frame=1)
        out[n-1] = fallback

    so no frame is warped along a flow across a cut.  One clip without auto_cut has no cut and needs frame=1 for its last pair only."""
    _, cut_params = _split(cut_params, (), who, auto_cut)
    both = auto_cut or slots is not None

    def compute(run):
        return run.e.compute_flow_bidirectional_device() if both or run.last else run.e.compute_flow()
    with _Run(who, clips, slots, params, temporal, stop_level, None, auto_cut, cut_params, compute) as run:
        out = [[c[0].copy()] for c in run.clips]
        for slot, c, f, _, keep in run:
            if slot == 0:               # once per step, every active pair
                r0 = run.e.rolling_shutter(frame=0, **rs)
                r1 = run.e.rolling_shutter(frame=1, **rs) if both or run.last else None
                if run.single:
                    r0, r1 = [r0], [r1]
            if not keep:
                continue
            cut = auto_cut and bool(run.found[slot])
            if not cut:
                out[c][f - 1] = r0[slot]
            out[c].append(run.clips[c][f].copy() if cut or r1 is None else r1[slot])
    return out


def rolling_shutter_sequence(frames, readout=0.5, anchor=0.5, iters=3, axis=0, params=None, temporal=True, stop_level=0, auto_cut=False, **cut_params):
    """A clip ((h, w, 3) uint8 frames, or yuv.YuvFrames) with its rolling-shutter distortion removed (EPPM.rolling_shutter, DESIGN.md
    section 27): one streaming context -- set_data, then push_frame --, a forward-only compute per pair and its image 1 corrected along the
    forward flow; the last pair is computed bidirectionally and gives the clip's last frame too, corrected along the backward flow.
    Returns len(frames) frames.  Memory does not grow with the clip.  readout / anchor / iters / axis: EPPM.rolling_shutter's; params: the
    flow's eppm Params; temporal / stop_level: the flow's temporal and draft modes.  auto_cut=True: every pair is computed bidirectionally
    and a CutDetector (cut_params: its lost_permille / residual_max) looks at it; the frames either side of a cut are corrected along the
    flows of their own shots (the last frame of a shot along its backward flow), and a one-frame shot comes back unchanged."""
    rs = dict(readout=readout, anchor=anchor, iters=iters, axis=axis)
    return _rolling_shutter("rolling_shutter_sequence", [frames], None, rs, params, temporal, _level(stop_level), auto_cut, cut_params)[0]


def rolling_shutter_sequences(clips, slots=8, readout=0.5, anchor=0.5, iters=3, axis=0, params=None, temporal=True, stop_level=0, auto_cut=False,
                              **cut_params):
    """rolling_shutter_sequence for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch
    context of min(slots, len(clips)) slots, on flow_sequences' schedule, every pair computed bidirectionally.  A slot that takes the next
    clip of the queue holds a pair across two clips for that step: nothing is read of it.  Returns one list of frames per clip, each what
    rolling_shutter_sequence(clip) returns."""
    rs = dict(readout=readout, anchor=anchor, iters=iters, axis=axis)
    return _rolling_shutter("rolling_shutter_sequences", clips, slots, rs, params, temporal, _level(stop_level), auto_cut, cut_params)


def _denoise(who, clips, slots, params, thresh, n_max, temporal, stop_level, auto_cut, cut_params):
    with _Run(who, clips, slots, params, temporal, stop_level, lambda e: TemporalFilter(e, thresh, n_max), auto_cut, cut_params) as run:
        out = [[c[0].copy()] for c in run.clips]
        for slot, c, _, _, keep in run:
            if keep:
                out[c].append(run.stage.frame(slot))
    return out


def denoise_sequence(frames, params=None, thresh=40.0, n_max=8, temporal=True, stop_level=0, auto_cut=False, **cut_params):
    """A clip ((h, w, 3) uint8 frames) denoised by the motion-compensated temporal filter (TemporalFilter): one
    streaming context -- set_data, then push_frame --, one bidirectional call on the device and one filter step per pair.  Returns
    len(frames) frames; the first is the input itself.  Memory does not grow with the clip.  params: the flow's eppm Params; temporal /
    stop_level: the flow's temporal and draft modes.  auto_cut=True: a CutDetector (cut_params: its lost_permille / residual_max) looks at
    every pair before the filter does; a frame that starts another shot restarts the filter and the flow's temporal prior, so the result
    is what denoise_sequence returns for every shot on its own (one host read of the verdict per step)."""
    return _denoise("denoise_sequence", [frames], None, params, thresh, n_max, temporal, _level(stop_level), auto_cut, cut_params)[0]


def denoise_sequences(clips, slots=8, params=None, thresh=40.0, n_max=8, temporal=True, stop_level=0, auto_cut=False, **cut_params):
    """denoise_sequence for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch context
    of min(slots, len(clips)) slots and one TemporalFilter, on flow_sequences' schedule.  A slot that takes the next clip of the queue
    passes `cut` for that step: its output is that clip's frame 0.  Returns one list of frames per clip, each what denoise_sequence(clip)
    returns.  auto_cut=True: denoise_sequence's, per slot; the detector's verdicts are ORed into the schedule's cut flags."""
    return _denoise("denoise_sequences", clips, slots, params, thresh, n_max, temporal, _level(stop_level), auto_cut, cut_params)


def _remove_defects(who, clips, slots, auto_cut, stop_level, masks, params, temporal, kw):
    """remove_defects_sequence(s): (frames, masks), one list per clip each"""
    df, cut_params = _split(kw, _DEFECT_KEYS, who)
    stop_level = _level(0 if stop_level is None else stop_level)
    with _Run(who, clips, slots, params, temporal, stop_level, lambda e: DefectFilter(e, **df), auto_cut, cut_params) as run:
        out, ms = [[] for _ in run.clips], [[] for _ in run.clips]
        for slot, c, _, _, keep in run:
            if keep:            # the slot's pair is (frame - 1, frame) of clip c: the step's output is frame - 1
                out[c].append(run.stage.frame(slot))
                if masks:
                    ms[c].append(run.stage.mask(slot))
    for c, clip in enumerate(run.clips):
        out[c].append(clip[-1].copy())
        ms[c].append(np.zeros((run.h, run.w), np.uint8))
    return out, ms


def remove_defects_sequence(frames, auto_cut=False, stop_level=None, masks=False, params=None, temporal=True, **kw):
    """A clip ((h, w, 3) uint8 frames) with its single-frame defects concealed (DefectFilter): one streaming context
    -- set_data, then push_frame --, one bidirectional call on the device and one filter step per pair; the step of pair (k, k + 1)
    gives frame k.  Returns len(frames) frames: the first, the last and (auto_cut=True: a CutDetector looks at every pair first) the
    frames next to a cut are the input itself.  masks=True: (frames, masks), one (h, w) uint8 mask per frame (0 untouched, 1 hit, 2
    grown).  kw: DefectFilter's detect / agree / radius / grow and CutDetector's lost_permille / residual_max.  params: the flow's eppm
    Params; temporal / stop_level: the flow's temporal and draft modes.  Memory does not grow with the clip."""
    out, ms = _remove_defects("remove_defects_sequence", [frames], None, auto_cut, stop_level, masks, params, temporal, kw)
    return (out[0], ms[0]) if masks else out[0]


def remove_defects_sequences(clips, slots=8, auto_cut=False, stop_level=None, masks=False, params=None, temporal=True, **kw):
    """remove_defects_sequence for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch
    context of min(slots, len(clips)) slots and one DefectFilter, on flow_sequences' schedule.  A slot that takes the next clip of the queue
    passes `cut` for that step.  Returns one list of frames per clip (masks=True: (frames, masks)), each what remove_defects_sequence(clip)
    returns.  auto_cut=True: per slot; the detector's verdicts are ORed into the schedule's cut flags."""
    out, ms = _remove_defects("remove_defects_sequences", clips, slots, auto_cut, stop_level, masks, params, temporal, kw)
    return (out, ms) if masks else out


def _deflicker(who, clips, slots, params, temporal, stop_level, auto_cut, fields, kw):
    """deflicker_sequence(s): (frames, fields), one list per clip each"""
    dk, cut_params = _split(kw, _DEFLICKER_KEYS, who, auto_cut)
    with _Run(who, clips, slots, params, temporal, _level(stop_level), lambda e: Deflicker(e, **dk), auto_cut, cut_params) as run:
        out, fl = [[c[0].copy()] for c in run.clips], [[] for _ in run.clips]
        for slot, c, _, _, keep in run:
            if keep:
                out[c].append(run.stage.frame(slot))
                if fields:
                    fl[c].append(run.stage.field(slot))
    return out, fl


def deflicker_sequence(frames, params=None, temporal=True, stop_level=0, auto_cut=False, fields=False, **kw):
    """A clip ((h, w, 3) uint8 frames) with its flicker removed (Deflicker): one streaming context -- set_data, then
    push_frame --, one bidirectional call on the device and one deflicker step per pair; every frame is corrected towards the corrected
    frame before it.  Returns len(frames) frames; the first is the input itself.  fields=True: (frames, fields), one (field, valid) per
    pair (Deflicker.field).  kw: Deflicker's cell / iters / reject / tau / keep / n_min, and with auto_cut=True CutDetector's
    lost_permille / residual_max: a detector looks at every pair first, and a frame that starts another shot is returned as it is and
    becomes the reference.  params: the flow's eppm Params; temporal / stop_level: the flow's temporal and draft modes.  Memory does not
    grow with the clip."""
    out, fl = _deflicker("deflicker_sequence", [frames], None, params, temporal, stop_level, auto_cut, fields, kw)
    return (out[0], fl[0]) if fields else out[0]


def deflicker_sequences(clips, slots=8, params=None, temporal=True, stop_level=0, auto_cut=False, fields=False, **kw):
    """deflicker_sequence for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch
    context of min(slots, len(clips)) slots and one Deflicker, on flow_sequences' schedule.  A slot that takes the next clip of the queue
    passes `cut` for that step: its output is that clip's frame 0.  Returns one list of frames per clip (fields=True: (frames, fields)),
    each what deflicker_sequence(clip) returns.  auto_cut=True: per slot; the detector's verdicts are ORed into the schedule's cut flags."""
    out, fl = _deflicker("deflicker_sequences", clips, slots, params, temporal, stop_level, auto_cut, fields, kw)
    return (out, fl) if fields else out


def _field_frames(who, clip, first):
    """the 2n field frames of a clip of n interlaced frames, bobbed on the host: field frame k has parity first ^ (k & 1)"""
    out = []
    for frame in clip:
        if isinstance(frame, yuv.YuvFrame):
            fields = [yuv.to_rgb(f) for f in yuv.split_fields(frame)]
            h = frame.h
        else:
            frame = np.ascontiguousarray(frame, np.uint8)
            if frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 2:
                raise EppmError(f"{who}: frames of (h, w, 3) uint8 with h >= 2")
            fields, h = [frame[0::2], frame[1::2]], frame.shape[0]
        out += [io.deint_bob_host(fields[p], h, p) for p in (first, first ^ 1)]
    return out


def _deinterlace(who, clips, slots, tff, double_rate, masks, params, temporal, stop_level, auto_cut, kw):
    """deinterlace_sequence(s): (frames, masks), one list per clip each"""
    di, cut_params = _split(kw, _DEINT_KEYS, who, auto_cut)
    stop_level = _level(stop_level)             # refused before any field is bobbed
    first = 0 if tff else 1
    clips = [list(clip) for clip in clips]
    if not clips or any(len(clip) < 1 for clip in clips):
        raise EppmError(f"{who}: at least one frame per clip")
    clips = [_field_frames(who, clip, first) for clip in clips]

    def parities(step):
        return dict(parity=[first ^ (f & 1) for _, f, _, _ in step])
    with _Run(who, clips, slots, params, temporal, stop_level, lambda e: Deinterlacer(e, **di), auto_cut, cut_params,
              step_args=parities) as run:
        bob_mask = np.where((np.arange(run.h) & 1) == first, 0, 2).astype(np.uint8)[:, None].repeat(run.w, 1)
        out, ms = [[c[0].copy()] for c in run.clips], [[bob_mask.copy()] for _ in run.clips]
        for slot, c, _, _, keep in run:
            if keep:
                out[c].append(run.stage.frame(slot))
                if masks:
                    ms[c].append(run.stage.mask(slot))
    if not double_rate:
        out, ms = [o[0::2] for o in out], [m[0::2] for m in ms]
    return out, ms


def deinterlace_sequence(frames, tff=True, double_rate=True, masks=False, params=None, temporal=True, stop_level=0, auto_cut=False, **kw):
    """A clip of n interlaced frames ((h, w, 3) uint8 arrays, or YuvFrames of h % 4 == 0) as 2n progressive frames at field rate
    (Deinterlacer).  tff: the top field (the even rows) is the first in time; False: the bottom field.  Every frame
    is split into its two fields -- arrays by row slicing, YuvFrames by yuv.split_fields and yuv.to_rgb -- and every field is bobbed to
    full height ON THE HOST (io.deint_bob_host; the device kernel eppm_deint_bob is for callers that hold their frames on the device).
    The 2n field frames go through one streaming context -- set_data, then push_frame --, one bidirectional call on the device and one
    deinterlacer step per pair; field frame f has parity first ^ (f & 1).  Returns 2n frames, the first being field frame 0 itself (the
    bob); double_rate=False: n frames, one per first field.  masks=True: (frames, masks), one (h, w) uint8 mask per frame (0 real row, 1
    temporal, 2 spatial).  kw: Deinterlacer's thresh / use_occ, and with auto_cut=True CutDetector's lost_permille / residual_max: a
    detector looks at every pair first, and a field that starts another shot takes nothing from the reference.  params: the flow's eppm
    Params; temporal / stop_level: the flow's temporal and draft modes.  Memory on the device does not grow with the clip."""
    out, ms = _deinterlace("deinterlace_sequence", [frames], None, tff, double_rate, masks, params, temporal, stop_level, auto_cut, kw)
    return (out[0], ms[0]) if masks else out[0]


def deinterlace_sequences(clips, slots=8, tff=True, double_rate=True, masks=False, params=None, temporal=True, stop_level=0, auto_cut=False, **kw):
    """deinterlace_sequence for many clips at once: clips of one frame size and of any lengths through ONE batch context of
    min(slots, len(clips)) slots and one Deinterlacer, on flow_sequences' schedule over the clips' field frames.  A slot that takes the
    next clip of the queue passes `cut` for that step: its output is that clip's field frame 0, bobbed.  Returns one list of frames per
    clip (masks=True: (frames, masks)), each what deinterlace_sequence(clip) returns.  auto_cut=True: per slot; the detector's verdicts are
    ORed into the schedule's cut flags."""
    out, ms = _deinterlace("deinterlace_sequences", clips, slots, tff, double_rate, masks, params, temporal, stop_level, auto_cut, kw)
    return (out, ms) if masks else out


def _propagate(who, clips, layers, slots, auto_cut, stop_level, maps, params):
    """propagate_layer(s): (frames, maps), one list per clip each"""
    cm_params, cut_params = _split(params, _CMAP_KEYS, who, auto_cut)
    clips, layers = list(clips), list(layers)
    if len(layers) != len(clips):
        raise EppmError("propagate_layers: one layer per clip")
    with _Run(who, clips, slots, None, True, stop_level, lambda e: CorrespondenceMap(e, **cm_params), auto_cut, cut_params) as run:
        cm = run.stage
        out, mp = [[] for _ in clips], [[] for _ in clips]
        drawn = {}

        def draw(slot, c):          # the slot's map is anchored on frame 0 of clip c: its layer from here on
            cm.set_layer(layers[c], slot)
            drawn[slot] = True
            out[c].append(cm.render(slot))
        for slot, (c, _, _, _) in enumerate(run.steps[0]):
            cm.set_state(slot, io.cmap_seed(run.h, run.w), run.clips[c][0])
            draw(slot, c)
            if maps:
                mp[c].append(cm.map(slot))
        for slot, c, f, new_clip, keep in run:
            if new_clip:
                draw(slot, c)
            elif keep:
                if auto_cut and run.found[slot]:        # the layer belongs to the shot before the cut
                    drawn[slot] = False
                out[c].append(cm.render(slot) if drawn[slot] else run.clips[c][f].copy())
                if maps:
                    mp[c].append(cm.map(slot))
    return out, mp


def propagate_layer(frames, layer_rgba, auto_cut=False, stop_level=None, maps=False, **params):
    """A layer painted on a clip's first frame follows the surface through the clip (CorrespondenceMap): frames are
    (h, w, 3) uint8, layer_rgba is (h, w, 4) uint8 with straight alpha in frame 0's geometry.  One streaming context -- set_data, then
    push_frame --, one bidirectional call on the device and one map step per pair; every output frame samples the layer ONCE, at the
    composed map.  Returns len(frames) frames; frame 0 is the layer composited through the seed map.  Memory does not grow with the clip.
    params: CMapParams' thresh, tear and use_occ, and with auto_cut=True CutDetector's lost_permille and residual_max: a detector looks at
    every pair before the map does, a frame that starts another shot re-anchors the map on itself, and from then on the layer is not drawn
    (it belongs to the first shot): those frames are the input frames.  stop_level: the flow's draft mode (None: full quality).
    maps=True: returns (frames, maps), one (h, w, 2) float32 map per frame."""
    out, mp = _propagate("propagate_layer", [frames], [layer_rgba], None, auto_cut, stop_level, maps, params)
    return (out[0], mp[0]) if maps else out[0]


def propagate_layers(clips, layers, slots=8, auto_cut=False, stop_level=None, **params):
    """propagate_layer for many clips at once: clips of one frame size and of any lengths (two frames at least), one layer per clip, through
    ONE batch context of min(slots, len(clips)) slots and one CorrespondenceMap, on flow_sequences' schedule.  A slot that takes the next
    clip of the queue passes `cut` for that step and takes that clip's layer: its output is the layer over that clip's frame 0.  Returns one
    list of frames per clip, each what propagate_layer(clip, layer) returns."""
    return _propagate("propagate_layers", clips, layers, slots, auto_cut, stop_level, False, params)[0]


def _objects(who, clips, slots, auto_cut, stop_level, labels, params):
    """detect_objects(_sequences): (objects, label planes), one list per clip each"""
    ob_params, cut_params = _split(params, _OBJECTS_KEYS, who, auto_cut)
    with _Run(who, clips, slots, None, True, stop_level, lambda e: ObjectDetector(e, **ob_params), auto_cut, cut_params) as run:
        out, planes = [[] for _ in run.clips], [[] for _ in run.clips]
        for slot, c, _, new_clip, keep in run:
            if new_clip:
                run.stage.reset(slot)
            elif keep:
                out[c].append(run.stage.objects(slot))
                if labels:
                    planes[c].append(run.stage.labels(slot))
    return out, planes


def detect_objects(frames, auto_cut=False, stop_level=None, labels=False, **params):
    """The moving objects of every consecutive pair of a clip ((h, w, 3) uint8 frames; ObjectDetector): one
    streaming context -- set_data, then push_frame --, one bidirectional call on the device and one detector step per pair.  Returns one
    list of object dicts (ObjectDetector.objects) per pair: the objects of the pair's first frame; an id persists while the object is
    followed.  Memory does not grow with the clip.  params: ObjectsParams', and with auto_cut=True CutDetector's lost_permille and
    residual_max: a pair that the cut detector calls a cut carries nothing over, so the objects of the next pair are all new.
    stop_level: the flow's draft mode (None: full quality).  labels=True: returns (objects, labels), one (h, w) uint8 plane per pair."""
    out, planes = _objects("detect_objects", [frames], None, auto_cut, stop_level, labels, params)
    return (out[0], planes[0]) if labels else out[0]


def detect_objects_sequences(clips, slots=8, auto_cut=False, stop_level=None, labels=False, **params):
    """detect_objects for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch context
    of min(slots, len(clips)) slots and one ObjectDetector, on flow_sequences' schedule.  A slot that takes the next clip of the queue is
    reset after that step, so the clip's ids start at 1.  Returns one list per clip, each what detect_objects(clip) returns."""
    out, planes = _objects("detect_objects_sequences", clips, slots, auto_cut, stop_level, labels, params)
    return (out, planes) if labels else out


def _plate_clip(frames, auto_cut, stop_level, params, per_pair=None):
    """one streaming context and one BackgroundPlate over a clip; per_pair(plate, k, path): called after pair k's step with the path that
    step used.  Returns (the frames, the plate): the plate is still open, the caller closes it; the context is closed."""
    pl_params, cut_params = _split(params, _PLATE_KEYS, "background plate", auto_cut)
    paths = []

    def compute(run):
        run.e.compute_flow_bidirectional_device()
        if per_pair is not None:
            paths.append(run.stage.path(0))
    with _Run("background plate", [frames], None, None, True, stop_level, lambda e: BackgroundPlate(e, **pl_params), auto_cut, cut_params,
              compute, hand_over=True) as run:
        for _, _, f, _, _ in run:
            if per_pair is not None:
                per_pair(run.stage, f - 1, paths[-1])
    return run.clips[0], run.stage


def background_plate(frames, auto_cut=False, stop_level=None, **params):
    """The background plate of a clip ((h, w, 3) uint8 frames; BackgroundPlate): one streaming context -- set_data,
    then push_frame --, one bidirectional call on the device and one plate step per pair.  Returns (plate, coverage): the canvas as an
    (h + 2*margin_y, w + 2*margin_x, 3) uint8 image in the coordinates of the first frame, and per pixel how often its value was
    confirmed (0: never seen).  The last frame of the clip has no pair of its own and is not accumulated.  params: PlateParams', and with
    auto_cut=True CutDetector's lost_permille and residual_max: after a pair the cut detector calls a cut the path starts again at the
    identity and the canvas is kept.  stop_level: the flow's draft mode (None: full quality)."""
    _, pl = _plate_clip(frames, auto_cut, stop_level, params)
    try:
        return pl.plate(0), pl.coverage(0)
    finally:
        pl.close()


def remove_objects_sequence(frames, auto_cut=False, stop_level=None, **params):
    """The frames of a clip with their moving objects painted out from the clip's background plate, in two passes over one plate.  Pass 1
    steps the clip as background_plate does and keeps each pair's mask and path on the host; pass 2 renders every frame against the
    FINISHED plate (BackgroundPlate.render_frame), so a frame is also filled from what only later frames reveal.  Returns (frames, fills):
    one (h, w, 3) uint8 image and one (h, w) uint8 fill plane (0 free, 1 filled, 2 blocked and not filled) per input frame.  The last
    frame of a clip has no pair of its own -- no mask, no path --, so it is returned unchanged with fill 0."""
    kept = []
    frames, pl = _plate_clip(frames, auto_cut, stop_level, params, per_pair=lambda p, k, path: kept.append((p.mask(0), path)))
    try:
        out, fills = [], []
        for k, (mask, path) in enumerate(kept):
            o, f = pl.render_frame(0, frames[k], mask, path)
            out.append(o)
            fills.append(f)
        out.append(frames[-1].copy())
        fills.append(np.zeros(frames[-1].shape[:2], np.uint8))
        return out, fills
    finally:
        pl.close()


def background_plates(clips, slots=8, auto_cut=False, stop_level=None, **params):
    """background_plate for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch context
    of min(slots, len(clips)) slots and one BackgroundPlate, on flow_sequences' schedule.  A clip's plate is read after the step of its
    last pair; a slot that takes the next clip of the queue is reset after that step.  Returns one (plate, coverage) per clip, each what
    background_plate(clip) returns."""
    pl_params, cut_params = _split(params, _PLATE_KEYS, "background_plates", auto_cut)
    with _Run("background_plates", clips, slots, None, True, stop_level, lambda e: BackgroundPlate(e, **pl_params), auto_cut, cut_params) as run:
        out = [None for _ in run.clips]
        for slot, c, f, new_clip, keep in run:
            if new_clip:
                run.stage.reset(slot)
            elif keep and f == len(run.clips[c]) - 1:
                out[c] = (run.stage.plate(slot), run.stage.coverage(slot))
    return out


def _stabilize(who, clips, slots, params, tau, iters, smooth, temporal, stop_level, masks, auto_cut, cut_params):
    """stabilize_sequence(s): (frames, masks, models), one list per clip each"""
    with _Run(who, clips, slots, params, temporal, stop_level, lambda e: Stabilizer(e, tau, iters, smooth), auto_cut, cut_params) as run:
        out, mk, md = [[c[0].copy()] for c in run.clips], [[] for _ in run.clips], [[] for _ in run.clips]
        for slot, c, _, _, keep in run:
            if keep:
                out[c].append(run.stage.frame(slot))
                if masks:
                    mk[c].append(run.stage.mask(slot))
                    md[c].append(run.stage.model(slot))
    return out, mk, md


def stabilize_sequence(frames, params=None, tau=1.0, iters=3, smooth=0.9, temporal=True, stop_level=0, masks=False, auto_cut=False, **cut_params):
    """A clip ((h, w, 3) uint8 frames) re-rendered from a smoothed camera path (Stabilizer): one streaming context --
    set_data, then push_frame --, one bidirectional call on the device and one stabiliser step per pair.  Returns len(frames) frames; the
    first is the input itself.  masks=True: (frames, masks, models) with one motion mask of image 1 and one model per pair.  params: the
    flow's eppm Params; temporal / stop_level: the flow's temporal and draft modes.  auto_cut=True: a CutDetector (cut_params: its
    lost_permille / residual_max) looks at every pair before the stabiliser does; a frame that starts another shot restarts the camera
    path and the flow's temporal prior, so the frames are what stabilize_sequence returns for every shot on its own."""
    out, mk, md = _stabilize("stabilize_sequence", [frames], None, params, tau, iters, smooth, temporal, _level(stop_level), masks, auto_cut, cut_params)
    return (out[0], mk[0], md[0]) if masks else out[0]


def stabilize_sequences(clips, slots=8, params=None, tau=1.0, iters=3, smooth=0.9, temporal=True, stop_level=0, masks=False, auto_cut=False,
                        **cut_params):
    """stabilize_sequence for many clips at once: clips of one frame size and of any lengths (two frames at least) through ONE batch context
    of min(slots, len(clips)) slots and one Stabilizer, on flow_sequences' schedule.  A slot that takes the next clip of the queue passes
    `cut` for that step: its output is that clip's frame 0.  Returns one result per clip, each what stabilize_sequence(clip) returns.
    auto_cut=True: stabilize_sequence's, per slot; the detector's verdicts are ORed into the schedule's cut flags."""
    out, mk, md = _stabilize("stabilize_sequences", clips, slots, params, tau, iters, smooth, temporal, _level(stop_level), masks, auto_cut, cut_params)
    return list(zip(out, mk, md)) if masks else out


def _track_start(frame, trk):
    """track_sequence's dictionary with the seeds of a clip's first frame"""
    seeds = io.track_seeds(frame, trk.params)[:trk.capacity]
    return {k: {"start": 0, "positions": [xy], "reason": None} for k, xy in enumerate(seeds)}


def _track_collect(out, trk):
    """one step's ended and live tracks into track_sequence's dictionary"""
    e_ids, _, _, why, _ = trk.ended()
    for i, r in zip(e_ids.tolist(), why.tolist()):
        out[i]["reason"] = int(r)
    ids, starts, xy = trk.tracks()
    for i, s0, p in zip(ids.tolist(), starts.tolist(), xy):
        if i in out:
            out[i]["positions"].append(p)
        else:
            out[i] = {"start": int(s0), "positions": [p], "reason": None}


def track_sequence(frames, params=None, streaming=False, stop_level=0, **track_params):
    """Dense point trajectories through a list of (h, w, 3) uint8 frames: one bidirectional call on a batch of the consecutive pairs, then
    one tracker step per pair.  Returns {track id: {"start": first frame, "positions": (n, 2) float32 positions in frames start ..
    start + n - 1, "reason": the end reason 1..4, or None while alive}}.  params: the flow's eppm Params; track_params: TrackParams'.
    streaming=True: one single-pair context instead of the batch -- push_frame and temporal mode, one bidirectional call and one tracker
    step per pair --, so that memory does not grow with the clip; the flows from the second pair on start from a temporal prior and are
    not bit for bit the batch's.  stop_level: draft mode (EPPM.set_stop_level): the tracker runs on the draft flows."""
    stop_level = _level(stop_level)
    (frames,), is_yuv = _clip_lists("track_sequence", [frames])
    as_yuv = frames if is_yuv else None
    if not is_yuv:
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    if len(frames) < 2:
        raise EppmError("track_sequence: at least two frames")
    first = (lambda: yuv.to_rgb(frames[0])) if as_yuv is not None else (lambda: frames[0])      # the frame the seeds are read from
    if streaming:
        with _Run("track_sequence", [frames], None, params, True, stop_level) as run:
            for _ in run:
                if run.stage is None:           # the tracker needs a computed pair
                    run.stage = Tracker(run.e, 0, **track_params)
                    out = _track_start(first(), run.stage)
                run.stage.step()
                _track_collect(out, run.stage)
    else:               # every pair at once: no frame loop to share
        h, w = (frames[0].h, frames[0].w) if as_yuv is not None else frames[0].shape[:2]
        bat = EPPMBatch(h, w, len(frames) - 1, params=params)
        trk = None
        try:
            bat.set_stop_level(stop_level)
            if as_yuv is not None:
                bat.set_data_yuv(list(zip(frames[:-1], frames[1:])))
            else:
                bat.set_data(list(zip(frames[:-1], frames[1:])))
            bat.compute_flow_bidirectional()
            trk = Tracker(bat, 0, **track_params)
            out = _track_start(first(), trk)
            for k in range(len(frames) - 1):
                trk.step(k)
                _track_collect(out, trk)
        finally:
            if trk is not None:
                trk.close()
            bat.close()
    for t in out.values():
        t["positions"] = np.asarray(t["positions"], np.float32).reshape(-1, 2)
    return out
