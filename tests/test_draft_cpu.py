"""Draft mode without a GPU: the ABI and the wrappers exist, the CLI refuses a bad --stop-level, the replicate
helper that the GPU tests share does what the definition says at the sizes where the clamp matters, and the draft result means
something on the oracle alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # (not from conftest: tests/draft_tol_child.py imports this module)

NEW_SYMBOLS = ("eppm_set_stop_level", "eppm_stop_level", "eppm_flow_upsample")
UNKNOWN_THRESH = np.float32(1e9)


def replicate2x_clamped(F, h, w):
    """The (h, w) plane whose pixel (y, x) is F[min(y >> 1, hc - 1), min(x >> 1, wc - 1)] (any dtype, structured ones included)."""
    hc, wc = F.shape
    ys = np.minimum(np.arange(h) >> 1, hc - 1)
    xs = np.minimum(np.arange(w) >> 1, wc - 1)
    return np.ascontiguousarray(F[np.ix_(ys, xs)])


def oracle_jbu(F, img):
    """The specification of the upsampling: the oracle's flow smoothing, guided by img, of the doubled and replicated coarse flow F."""
    from oracle import oracle as O
    h, w = img.shape
    rep = replicate2x_clamped(np.ascontiguousarray(F, O.float2), h, w)
    d = np.zeros((h, w), O.float2)
    d["x"] = np.float32(2.0) * rep["x"]
    d["y"] = np.float32(2.0) * rep["y"]
    return O.flow_smoothing(d, img)


def test_product_libraries_export_the_draft_abi():
    import eppm_amd
    for variant in ("", "tol"):
        L = C.CDLL(eppm_amd.lib_path(variant))
        for s in NEW_SYMBOLS:
            getattr(L, s)                    # AttributeError: not exported
    assert set(NEW_SYMBOLS) <= set(eppm_amd._lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr


def test_python_wrappers_refuse_a_non_integer_level_before_the_library():
    import eppm_amd
    from eppm_amd import api
    for cls in (api.EPPM, api.EPPMBatch):
        assert callable(getattr(cls, "set_stop_level")) and callable(getattr(cls, "stop_level"))
    e = api.EPPM()                           # no context: an integer level would fail with "init(h, w) has not been called"
    for bad in (1.0, "1", None, True, np.float32(1)):
        with pytest.raises(eppm_amd.EppmError, match="must be an integer"):
            e.set_stop_level(bad)
    with pytest.raises(eppm_amd.EppmError, match="init"):
        e.set_stop_level(np.int64(1))
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    for fn, args in ((api.flow_sequence, (frames,)), (api.flow_sequences, ([frames],)), (api.track_sequence, (frames,))):
        with pytest.raises(eppm_amd.EppmError, match="must be an integer"):
            fn(*args, stop_level=0.5)


@pytest.mark.parametrize("args", [["--stop-level"], ["--stop-level", "-1"], ["--stop-level", "x"], ["--stop-level", "1.5"]], ids=" ".join)
def test_cli_refuses_a_bad_stop_level(args):
    import eppm_amd
    exe = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "usage: runeppm" in p.stderr and "--stop-level" in p.stderr, (p.returncode, p.stderr)


@pytest.mark.parametrize("fine,coarse", [((157, 211), (78, 105)), ((78, 105), (39, 52))], ids=["211x157", "105x78"])
def test_replicate_helper_where_the_clamp_matters(fine, coarse):
    h, w = fine
    hc, wc = coarse
    assert (hc, wc) == (int(h * 0.5), int(w * 0.5))
    F = np.arange(hc * wc, dtype=np.float32).reshape(hc, wc)
    R = replicate2x_clamped(F, h, w)
    assert R.shape == (h, w)
    for y in range(h):
        for x in (0, 1, 2, w - 3, w - 2, w - 1):
            assert R[y, x] == F[min(y // 2, hc - 1), min(x // 2, wc - 1)]
    # the last fine column / row lies past the coarse plane and repeats its last one
    assert (w - 1) >> 1 == wc and np.array_equal(R[:, w - 1], R[:, w - 2])
    if (h - 1) >> 1 == hc:
        assert np.array_equal(R[h - 1], R[h - 2])
    S = replicate2x_clamped(np.zeros((hc, wc), np.dtype([("x", "f4"), ("y", "f4")])), h, w)
    assert S.shape == (h, w) and S.dtype.names == ("x", "y")


def test_draft_meaning_on_the_oracle(capsys):
    """The oracle chain ending in flow_smoothing(2 * rep(flow[1]), img1[0]) against the full oracle chain on synth.make_pair(192, 256): both
    end-point errors against the ground truth (16-px border excluded) are printed (and recorded in DESIGN.md section 14); asserted: the
    draft error is finite and the draft has no more unknown vectors than the full result."""
    from eppm_amd import synth
    from oracle import oracle as O
    h, w = 192, 256
    a, b, gu, gv = synth.make_pair(h, w)
    u, v, st = O.compute_flow(a, b, dump=True)
    d = oracle_jbu(st["flow_L1"], st["img1_L0"])
    du, dv = d["x"], d["y"]
    inner = (slice(16, h - 16), slice(16, w - 16))

    def epe(fu, fv):
        known = ~((fu > UNKNOWN_THRESH) | (fv > UNKNOWN_THRESH))
        e = np.sqrt((fu.astype(np.float64) - gu) ** 2 + (fv.astype(np.float64) - gv) ** 2)
        return float(e[inner][known[inner]].mean()), int((~known).sum())

    full, full_unknown = epe(u, v)
    draft, draft_unknown = epe(du, dv)
    with capsys.disabled():
        print(f"\ndraft meaning {w}x{h}: EPE full {full:.4f} px ({full_unknown} unknown), draft s=1 {draft:.4f} px ({draft_unknown} unknown)")
    assert np.isfinite(draft)
    assert draft_unknown <= full_unknown
