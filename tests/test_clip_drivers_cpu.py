"""CPU test of the clip drivers: every call a driver makes on the context, the stage object, the cut detector and
the tracker, with its arguments and in its order, and everything it returns or raises, against a recording.

The drivers reach the library only through EPPM, EPPMBatch, the seven stage classes, CutDetector and Tracker.  Those names are replaced,
in the module that holds the drivers, by fakes that write every call into one trace and return tagged placeholders; no library is loaded.
Arguments are bound to the real method's signature first, so a positional and a keyword form of one call read alike and a call the real
class would refuse is refused here too.  An array is written as dtype, shape and first byte: the frames of clip c are filled with
10 * c + frame, so that byte names clip and frame.  The cut detector's verdicts and the failing compute come from a script in the case.

tests/golden/clip_driver_traces.json was recorded with `python tests/test_clip_drivers_cpu.py --record` before the drivers were moved
onto one streaming loop; it is recorded again only when a driver is meant to make other calls."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import eppm_amd
from eppm_amd import api

PATH = os.path.join(GOLDEN, "clip_driver_traces.json")
FAKED = ("EPPM", "EPPMBatch", "TemporalFilter", "DefectFilter", "Stabilizer", "CutDetector", "CorrespondenceMap", "ObjectDetector",
         "BackgroundPlate", "Tracker")
H, W = 4, 6

TRACE = []
SCRIPT = {}
COUNT = {}


def show(x):
    """one argument or result as a short string"""
    if isinstance(x, Fake):
        return x.name
    if isinstance(x, np.ndarray):
        s = f"{x.dtype}{list(x.shape)}:{x.ravel().view(np.uint8)[0] if x.size else '-'}"
        return s + (f"={x.tolist()}" if x.dtype != np.uint8 and x.size <= 16 else "")
    if isinstance(x, (list, tuple)):
        inner = ", ".join(show(v) for v in x)
        return f"[{inner}]" if isinstance(x, list) else f"({inner})"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}: {show(v)}" for k, v in sorted(x.items())) + "}"
    if isinstance(x, (bool, np.bool_)):
        return repr(bool(x))
    if isinstance(x, np.integer):
        return repr(int(x))
    return repr(x)


def nest(x):
    """a returned structure for the recording: lists stay lists, a tuple becomes ["tuple", ...], a dict [["dict"], [key, value], ...]"""
    if isinstance(x, tuple):
        return ["tuple"] + [nest(v) for v in x]
    if isinstance(x, list):
        return [nest(v) for v in x]
    if isinstance(x, dict):
        return [["dict"]] + [[show(k), nest(v)] for k, v in x.items()]
    return show(x)


class Fake:
    """A stand-in for one handle class: every call is bound to the real signature and written into TRACE."""
    real = None

    def __init__(self, *a, **kw):
        k = COUNT[self.real.__name__] = COUNT.get(self.real.__name__, 0) + 1
        self.name = f"{self.real.__name__}{k}"
        self.calls = {}
        bound = self._record("__init__", a, kw)
        self.n = 1                                                  # active pairs: EPPMBatch.set_data sets it
        self.ctx = bound.get("ctx")
        self.params, self.capacity = "track-params", 2              # what track_sequence reads of a Tracker

    def _record(self, method, a, kw):
        b = inspect.signature(getattr(self.real, method)).bind(self, *a, **kw)
        b.apply_defaults()
        args = dict(list(b.arguments.items())[1:])
        TRACE.append(f"{self.name}.{method}({', '.join(show(v) for v in args.values())})")
        return args

    def __getattr__(self, method):
        if method.startswith("__") or not callable(getattr(self.real, method, None)):
            raise AttributeError(method)

        def call(*a, **kw):
            args = self._record(method, a, kw)
            j = self.calls[method] = self.calls.get(method, 0) + 1
            return self._result(method, args, j - 1, f"{self.name}.{method}#{len(TRACE) - 1}")
        return call

    def _result(self, method, args, j, tag):
        """what call number j (from 0) of `method` returns; tag: a placeholder that names the call"""
        pairs = self.n if self.real.__name__ == "EPPMBatch" else None
        if method == "set_data" and pairs is not None:
            self.n = len(args["pairs"])
            return None
        if method.startswith("compute_flow"):
            k = COUNT["compute"] = COUNT.get("compute", 0) + 1
            if k == SCRIPT.get("fail_at"):
                raise RuntimeError("scripted failure in compute")
            if method == "compute_flow_bidirectional_device":
                return None
            names = ("u", "v", "bu", "bv", "occ1", "occ2")[:2 if method == "compute_flow" else 6]
            if pairs is None:
                return tuple(f"{tag}.{s}" for s in names)
            return [tuple(f"{tag}[{p}].{s}" for s in names) for p in range(pairs)]
        if method == "cuts":                                        # the detector's verdicts: SCRIPT["cuts"] = {step: [slots]}
            return [p in SCRIPT.get("cuts", {}).get(j, ()) for p in range(self.ctx.n)]
        if self.real.__name__ == "Tracker" and method == "ended":   # track 0 ends at the second step, for reason 3
            ids = np.array([0] if j == 1 else [], np.int32)
            return ids, None, None, np.full(len(ids), 3, np.int32), None
        if self.real.__name__ == "Tracker" and method == "tracks":  # a track that is no seed starts at the second step
            ids = np.array([0, 1] if j == 0 else [1, 2], np.int32)
            return ids, np.array([0, 0] if j == 0 else [0, 2], np.int32), np.full((2, 2), j + 0.5, np.float32)
        if method == "render_frame":
            return f"{tag}.out", f"{tag}.fill"
        if method in ("set_temporal", "set_stop_level", "init", "push_frame", "push_frames", "temporal_reset", "step", "reset", "close",
                      "set_state", "set_layer", "set_data"):
            return None
        return tag


def fakes(monkeypatch):
    """the fakes in place of the handle classes, where the drivers look them up"""
    mod = sys.modules[eppm_amd.flow_sequence.__module__]
    for name in FAKED:
        monkeypatch.setattr(mod, name, type(name, (Fake,), {"real": getattr(api, name)}))
    monkeypatch.setattr(eppm_amd.io, "track_seeds", lambda img, params=None, **kw: np.array([[1, 1], [4, 2]], np.float32))


def clip(c, n):
    return [np.full((H, W, 3), 10 * c + k, np.uint8) for k in range(n)]


def clips(lengths=(2, 4, 3)):
    return [clip(c, n) for c, n in enumerate(lengths)]


def layer(c=0):
    return np.full((H, W, 4), 200 + c, np.uint8)


SINGLE = ("detect_cuts", "flow_sequence", "motion_blur_sequence", "denoise_sequence", "remove_defects_sequence", "propagate_layer",
          "detect_objects", "background_plate", "remove_objects_sequence", "stabilize_sequence", "track_sequence")
BATCH = ("flow_sequences", "denoise_sequences", "remove_defects_sequences", "propagate_layers", "detect_objects_sequences",
         "background_plates", "stabilize_sequences")
REFUSED = set()                 # the cases that must raise before anything is opened


def cases():
    """{id: (driver, args, kwargs, script)}"""
    out = {}

    def add(name, fn, args, kw=None, refused=False, **script):
        assert name not in out, name
        out[name] = (fn, args, kw or {}, script)
        if refused:
            REFUSED.add(name)

    ac = dict(auto_cut=True)
    cut1 = {1: [0]}
    # -- every single-clip driver, its flags in every position, auto_cut off and on (a verdict at pair 1) -----------------------------
    add("detect_cuts", "detect_cuts", (clip(0, 4),))
    add("detect_cuts-cut", "detect_cuts", (clip(0, 4),), dict(lost_permille=500, params="P"), cuts=cut1)
    for bi in (False, True):
        add(f"flow_sequence-bi{bi:d}", "flow_sequence", (clip(0, 4),), dict(bidirectional=bi, params="P"))
        add(f"flow_sequence-bi{bi:d}-auto", "flow_sequence", (clip(0, 4),), dict(bidirectional=bi, residual_max=3.0, **ac), cuts=cut1)
    add("flow_sequence-cold", "flow_sequence", (clip(0, 3),), dict(temporal=False))
    add("motion_blur_sequence", "motion_blur_sequence", (clip(0, 4),), dict(shutter=0.25, params="P"))
    add("motion_blur_sequence-2", "motion_blur_sequence", (clip(0, 2),), dict(temporal=False, taps=4))
    add("denoise_sequence", "denoise_sequence", (clip(0, 4),), dict(thresh=30.0, params="P"))
    add("denoise_sequence-auto", "denoise_sequence", (clip(0, 4),), dict(n_max=4, lost_permille=400, **ac), cuts=cut1)
    for m in (False, True):
        add(f"remove_defects_sequence-m{m:d}", "remove_defects_sequence", (clip(0, 4),), dict(masks=m, detect=50.0, params="P"))
        add(f"remove_defects_sequence-m{m:d}-auto", "remove_defects_sequence", (clip(0, 4),), dict(masks=m, lost_permille=400, **ac), cuts=cut1)
        add(f"propagate_layer-m{m:d}", "propagate_layer", (clip(0, 4), layer()), dict(maps=m, tear=3))
        add(f"propagate_layer-m{m:d}-auto", "propagate_layer", (clip(0, 4), layer()), dict(maps=m, residual_max=2.0, **ac), cuts=cut1)
        add(f"detect_objects-l{m:d}", "detect_objects", (clip(0, 4),), dict(labels=m, min_area=4))
        add(f"detect_objects-l{m:d}-auto", "detect_objects", (clip(0, 4),), dict(labels=m, lost_permille=400, **ac), cuts=cut1)
        add(f"stabilize_sequence-m{m:d}", "stabilize_sequence", (clip(0, 4),), dict(masks=m, smooth=0.5, params="P"))
        add(f"stabilize_sequence-m{m:d}-auto", "stabilize_sequence", (clip(0, 4),), dict(masks=m, temporal=False, **ac), cuts=cut1)
        add(f"track_sequence-s{m:d}", "track_sequence", (clip(0, 4),), dict(streaming=m, spacing=4, params="P"))
    for fn in ("background_plate", "remove_objects_sequence"):
        add(fn, fn, (clip(0, 4),), dict(margin_x=2))
        add(f"{fn}-auto", fn, (clip(0, 4),), dict(grow=1, lost_permille=400, **ac), cuts=cut1)
    # -- every many-clip driver: a slot that takes the next clip and an idle slot (2), one slot (1), more slots than clips (8);
    #    auto_cut on: one verdict on an ordinary step and one on the step where that slot takes a new clip (8 slots: on an idle slot)
    many = (("flow_sequences", (), dict(params="P")), ("flow_sequences", (), dict(bidirectional=True)),
            ("denoise_sequences", (), dict(thresh=30.0, params="P")), ("remove_defects_sequences", (), dict(params="P")),
            ("remove_defects_sequences", (), dict(masks=True, radius=2)), ("propagate_layers", ([layer(c) for c in range(3)],), dict(thresh=80.0)),
            ("detect_objects_sequences", (), {}), ("detect_objects_sequences", (), dict(labels=True, tau=2.0)),
            ("background_plates", (), dict(margin_y=1)), ("stabilize_sequences", (), dict(params="P")),
            ("stabilize_sequences", (), dict(masks=True, tau=2.0, temporal=False)))
    for fn, extra, kw in many:
        for slots, cuts in ((2, {1: [0], 2: [1]}), (1, {1: [0], 3: [0]}), (8, {1: [0, 1]})):
            flag = "".join(f"-{k}" for k in ("bidirectional", "masks", "labels") if kw.get(k))
            add(f"{fn}{flag}-slots{slots}", fn, (clips(), *extra), dict(slots=slots, **kw))
            add(f"{fn}{flag}-slots{slots}-auto", fn, (clips(), *extra), dict(slots=slots, lost_permille=400, **ac, **kw), cuts=cuts)
    # -- stop_level on one driver of each default convention (0; None that means 0; None that leaves the context alone) ---------------
    for level in (None, 0, 1):
        for fn in ("flow_sequence", "remove_defects_sequence", "detect_objects"):
            add(f"{fn}-level{level}", fn, (clip(0, 3),), dict(stop_level=level))
            add(f"{fn}s-level{level}", fn.replace("detect_objects", "detect_objects_sequence") + "s", (clips((2, 3)),), dict(stop_level=level, slots=2))
    # -- refusals: nothing is opened -----------------------------------------------------------------------------------------------------
    for bad in (True, 1.5):
        for fn in ("detect_cuts", "flow_sequence", "motion_blur_sequence", "denoise_sequence", "remove_defects_sequence", "stabilize_sequence"):
            add(f"{fn}-level{bad}", fn, (clip(0, 3),), dict(stop_level=bad), refused=True)
        for s in (False, True):
            add(f"track_sequence-s{s:d}-level{bad}", "track_sequence", (clip(0, 3),), dict(stop_level=bad, streaming=s), refused=True)
        for fn in ("flow_sequences", "denoise_sequences", "remove_defects_sequences", "stabilize_sequences"):
            add(f"{fn}-level{bad}", fn, (clips(),), dict(stop_level=bad), refused=True)
    for fn in SINGLE:
        extra = (layer(),) if fn == "propagate_layer" else ()
        add(f"{fn}-one-frame", fn, (clip(0, 1), *extra), refused=True)
        add(f"{fn}-no-frame", fn, ([], *extra), refused=True)
    add("track_sequence-streaming-one-frame", "track_sequence", (clip(0, 1),), dict(streaming=True), refused=True)
    for fn in BATCH:
        extra = ([layer(c) for c in range(3)],) if fn == "propagate_layers" else ()
        add(f"{fn}-short-clip", fn, (clips((2, 1, 3)), *extra), refused=True)
        add(f"{fn}-slots0", fn, (clips(), *extra), dict(slots=0), refused=True)
    add("propagate_layers-two-layers", "propagate_layers", (clips(), [layer(0), layer(1)]), refused=True)
    for fn in ("remove_defects_sequence", "propagate_layer", "detect_objects", "background_plate", "remove_objects_sequence",
               "remove_defects_sequences", "propagate_layers", "detect_objects_sequences", "background_plates"):
        first = clips() if fn in BATCH else clip(0, 3)
        extra = {"propagate_layer": (layer(),), "propagate_layers": ([layer(c) for c in range(3)],)}.get(fn, ())
        add(f"{fn}-unknown-keyword", fn, (first, *extra), dict(bogus=1, also=2), refused=True)
        add(f"{fn}-unknown-keyword-auto", fn, (first, *extra), dict(bogus=1, **ac), refused=True)
        add(f"{fn}-cut-params-alone", fn, (first, *extra), dict(residual_max=2.0), refused="defects" not in fn)      # the two defect drivers take them
    # -- keywords that today's drivers with **cut_params take without auto_cut, and what the detector makes of them with it -----------
    for fn in ("detect_cuts", "flow_sequence", "denoise_sequence", "stabilize_sequence", "flow_sequences", "denoise_sequences", "stabilize_sequences"):
        first = clips() if fn in BATCH else clip(0, 3)
        add(f"{fn}-unknown-keyword", fn, (first,), dict(bogus=1))
        if fn != "detect_cuts":
            add(f"{fn}-unknown-keyword-auto", fn, (first,), dict(bogus=1, **ac))
    # -- failure in flight: the third compute raises -------------------------------------------------------------------------------------
    for fn in ("denoise_sequence", "remove_objects_sequence", "background_plate", "propagate_layer", "flow_sequence", "detect_cuts"):
        extra = (layer(),) if fn == "propagate_layer" else ()
        add(f"{fn}-fails", fn, (clip(0, 5), *extra), fail_at=3)
        if fn != "detect_cuts":
            add(f"{fn}-fails-auto", fn, (clip(0, 5), *extra), ac, fail_at=3, cuts=cut1)
    add("track_sequence-streaming-fails", "track_sequence", (clip(0, 5),), dict(streaming=True), fail_at=3)
    add("track_sequence-streaming-fails-first", "track_sequence", (clip(0, 5),), dict(streaming=True), fail_at=1)
    for fn in ("denoise_sequences", "background_plates", "propagate_layers", "flow_sequences"):
        extra = ([layer(c) for c in range(3)],) if fn == "propagate_layers" else ()
        add(f"{fn}-fails", fn, (clips(), *extra), dict(slots=2), fail_at=3)
        add(f"{fn}-fails-auto", fn, (clips(), *extra), dict(slots=2, **ac), fail_at=3, cuts=cut1)
    return out


CASES = cases()


def run(case):
    """{"trace": [...], and "returns": structure or "raises": [type, message]} of one case under the fakes"""
    fn, args, kw, script = CASES[case]
    TRACE.clear()
    COUNT.clear()
    SCRIPT.clear()
    SCRIPT.update(script)
    try:
        end = {"returns": nest(getattr(eppm_amd, fn)(*args, **kw))}
    except Exception as ex:
        end = {"raises": [type(ex).__name__, str(ex)]}
    return {"trace": list(TRACE), **end}


@pytest.fixture(scope="module")
def recorded():
    with open(PATH) as f:
        return json.load(f)


def test_the_recording_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_reproduces_its_recorded_calls_and_result(case, recorded, monkeypatch):
    fakes(monkeypatch)
    got, want = run(case), recorded[case]
    assert got["trace"] == want["trace"]
    assert got == want


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_a_refusal_opens_nothing(case, monkeypatch):
    fakes(monkeypatch)
    got = run(case)
    assert "raises" in got and got["trace"] == [], got


@pytest.mark.parametrize("bad", [True, 1.5], ids=repr)
@pytest.mark.parametrize("fn", ["propagate_layer", "detect_objects", "background_plate", "remove_objects_sequence", "propagate_layers",
                                "detect_objects_sequences", "background_plates"])
def test_a_bad_stop_level_opens_nothing_where_none_leaves_the_context_alone(fn, bad, monkeypatch):
    """The drivers whose stop_level=None skips set_stop_level: the level is checked before the context is opened (it was checked after)."""
    fakes(monkeypatch)
    first = clips() if fn in BATCH else clip(0, 3)
    extra = {"propagate_layer": (layer(),), "propagate_layers": ([layer(c) for c in range(3)],)}.get(fn, ())
    TRACE.clear()
    COUNT.clear()
    SCRIPT.clear()
    with pytest.raises(eppm_amd.EppmError, match=f"stop level must be an integer, not {bad!r}"):
        getattr(eppm_amd, fn)(first, *extra, stop_level=bad)
    assert TRACE == []


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_clip_drivers_cpu.py --record")
    mp = pytest.MonkeyPatch()
    fakes(mp)
    rec = {case: run(case) for case in sorted(CASES)}
    mp.undo()
    with open(PATH, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases, {os.path.getsize(PATH)} bytes -> {PATH}")
