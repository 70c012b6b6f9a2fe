"""CPU test of the clip drivers on clips of YuvFrames, with the fakes of tests/test_clip_drivers_cpu.py: a driver
fed with YuvFrames makes the context's _yuv calls where it makes the RGB ones for a clip of arrays -- same order, same frames, same flags
-- and every other call as before; frames it reads itself are yuv.to_rgb of the clip's.  A run of mixed formats or sizes opens nothing."""
import re
import sys

import numpy as np
import pytest

import eppm_amd
from eppm_amd import api, yuv
import test_clip_drivers_cpu as D


class YuvFake(D.Fake):
    def _result(self, method, args, j, tag):
        if method.endswith("_yuv"):                 # what the RGB call of that name returns, and EPPMBatch.set_data's count of pairs
            method = method[:-4]
        return super()._result(method, args, j, tag)


def show(x, _show=D.show):
    if isinstance(x, yuv.YuvFrame):
        return f"F:{int(x.planes[0][0, 0])}"       # the frame's first luma sample names clip and frame, as an array's first byte does
    if isinstance(x, (list, tuple)) and any(isinstance(v, (yuv.YuvFrame, list, tuple)) for v in x):
        inner = ", ".join(show(v) for v in x)
        return f"[{inner}]" if isinstance(x, list) else f"({inner})"
    return _show(x)


def fakes(monkeypatch):
    mod = sys.modules[eppm_amd.flow_sequence.__module__]
    for name in D.FAKED:
        monkeypatch.setattr(mod, name, type(name, (YuvFake,), {"real": getattr(api, name)}))
    monkeypatch.setattr(eppm_amd.io, "track_seeds", lambda img, params=None, **kw: np.array([[1, 1], [4, 2]], np.float32))
    monkeypatch.setattr(D, "show", show)


def yuv_clip(c, n, **fmt):
    return [yuv.YuvFrame.nv12(np.full((D.H, D.W), 10 * c + k, np.uint8), np.full((D.H // 2, D.W), 128, np.uint8), **fmt) for k in range(n)]


def trace(fn, args, kw, script=None):
    D.TRACE.clear()
    D.COUNT.clear()
    D.SCRIPT.clear()
    D.SCRIPT.update(script or {})
    result = getattr(eppm_amd, fn)(*args, **kw)
    return list(D.TRACE), result


FEED = re.compile(r"\.(set_data|push_frame|push_frames)(_yuv)?\(")


def normal(lines):
    """a trace with the feeding calls under their RGB names and their frames as F:<first byte>; other arrays without their first byte (a
    frame a driver read itself is to_rgb of the YuvFrame: another byte)"""
    out = []
    for ln in lines:
        if FEED.search(ln):
            ln = FEED.sub(lambda m: f".{m.group(1)}(", ln)
            ln = re.sub(r"uint8\[4, 6, 3\]:(\d+)", r"F:\1", ln)
        else:
            ln = re.sub(r"(uint8\[4, 6, 3\]):\d+", r"\1", ln)
        out.append(ln)
    return out


LAYERS = {"propagate_layer": lambda: (D.layer(),), "propagate_layers": lambda: ([D.layer(c) for c in range(3)],)}
RUNS = [(fn, {}, None) for fn in D.SINGLE] + [("track_sequence", dict(streaming=True), None), ("flow_sequence", dict(auto_cut=True), {"cuts": {1: [0]}})]
RUNS += [(fn, dict(slots=s), None) for fn in D.BATCH for s in (2, 8)] + [("denoise_sequences", dict(slots=2, auto_cut=True), {"cuts": {1: [0], 2: [1]}})]


@pytest.mark.parametrize("fn,kw,script", RUNS, ids=[f"{fn}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for fn, kw, _ in RUNS])
def test_yuv_clip_makes_the_yuv_calls_in_the_rgb_order(fn, kw, script, monkeypatch):
    fakes(monkeypatch)
    extra = LAYERS.get(fn, lambda: ())()
    many = fn in D.BATCH
    rgb = D.clips() if many else D.clip(0, 4)
    src = [yuv_clip(c, n) for c, n in enumerate((2, 4, 3))] if many else yuv_clip(0, 4)
    want, _ = trace(fn, (rgb, *extra), kw, script)
    got, _ = trace(fn, (src, *extra), kw, script)
    feeds = [ln for ln in got if FEED.search(ln)]
    assert feeds and all("_yuv(" in ln for ln in feeds)                 # every frame went in through a _yuv method ...
    assert not any("_yuv(" in ln for ln in want)                        # ... and an RGB clip makes none of those calls
    assert normal(got) == normal(want)


def test_frames_a_driver_reads_itself_are_to_rgb_of_the_clip(monkeypatch):
    fakes(monkeypatch)
    rng = np.random.default_rng(0)
    src = [yuv.from_rgb(rng.integers(0, 256, (D.H, D.W, 3), dtype=np.uint8)) for _ in range(3)]
    _, out = trace("stabilize_sequence", (src,), {})
    assert isinstance(out[0], np.ndarray) and np.array_equal(out[0], yuv.to_rgb(src[0]))      # the first output frame is the input itself
    _, (frames, fills) = trace("remove_objects_sequence", (src,), {})
    assert np.array_equal(frames[-1], yuv.to_rgb(src[-1])) and fills[-1].shape == (D.H, D.W)


@pytest.mark.parametrize("fn", ["flow_sequence", "denoise_sequences", "track_sequence"])
def test_mixed_runs_are_refused_before_anything_is_opened(fn, monkeypatch):
    fakes(monkeypatch)
    many = fn in D.BATCH
    for other in (yuv_clip(0, 1, depth=8, matrix=0)[0], yuv.from_rgb(np.zeros((6, 6, 3), np.uint8)), np.zeros((D.H, D.W, 3), np.uint8)):
        a = yuv_clip(0, 3)
        a[2] = other
        D.TRACE.clear()
        with pytest.raises(eppm_amd.EppmError, match="one format and size"):
            getattr(eppm_amd, fn)([yuv_clip(1, 2), a] if many else a)
        assert D.TRACE == []


@pytest.mark.parametrize("fn", ["denoise_sequence", "track_sequence", "flow_sequences"])
def test_clips_may_be_generators(fn, monkeypatch, tmp_path):
    """a clip is read once: a generator of RGB arrays makes the calls the list makes (as before YuvFrames were known here), and
    yuv.read_y4m handed over as it is -- a one-shot iterator -- is the clip of all its frames, not one short"""
    fakes(monkeypatch)
    many = fn in D.BATCH
    as_list = D.clips() if many else D.clip(0, 4)
    as_gen = (iter(c) for c in D.clips()) if many else iter(D.clip(0, 4))
    want, _ = trace(fn, (as_list,), {})
    got, _ = trace(fn, (as_gen,), {})
    assert got == want and got
    src = [yuv.from_rgb(np.full((D.H, D.W, 3), 10 * k, np.uint8), layout=1, matrix=0) for k in range(4)]
    yuv.write_y4m(tmp_path / "c.y4m", src)
    lists = [list(yuv.read_y4m(tmp_path / "c.y4m")) for _ in range(2)]
    want, _ = trace(fn, (lists if many else lists[0],), {})
    readers = [yuv.read_y4m(tmp_path / "c.y4m") for _ in range(2)]
    got, _ = trace(fn, (iter(readers) if many else readers[0],), {})
    assert got == want
    feeds = [ln for ln in got if FEED.search(ln)]
    assert feeds and all("_yuv(" in ln for ln in feeds)
    if fn == "denoise_sequence":                   # set_data on frames 0, 1, then pushes of 2 and 3: every frame of the file went in
        assert [re.findall(r"F:(\d+)", ln) for ln in feeds] == [[str(int(f.planes[0][0, 0])) for f in lists[0][:2]]] + [[str(int(f.planes[0][0, 0]))] for f in lists[0][2:]]
