"""Rolling-shutter correction in poisoned memory ("Write-before-read of every allocation"; section 27): the context forms as
the first and as a later call of a context, the batch form with fewer active pairs than slots, and the caller-plane form, each under the
fills 0xFF, 0x01 and 0x7F of the test option "alloc_fill".  Every result must be the bytes of the unfilled run: the velocity plane is
written whole before the gather reads it, and the packed output before it is copied."""
import numpy as np
import pytest

from alloc_fill_child import DevMem, across_fills, put, rgba_of, stills

pytestmark = pytest.mark.gpu


def context_forms(after_forward):
    import eppm_amd
    a, b = stills()["sub"]
    h, w, _ = a.shape

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        bufs = []
        try:
            e.init(a, b, h, w)
            if after_forward:
                put(out, "forward", e.compute_flow())
                put(out, "rs0_first", e.rolling_shutter(readout=1.0))
            put(out, "bidir", e.compute_flow_bidirectional())
            put(out, "rs1", e.rolling_shutter(readout=1.0, frame=1))
            put(out, "rs0", e.rolling_shutter(readout=-0.75, anchor=0.0, iters=8, axis=1))
            bufs = [DevMem(nbytes=h * w * 4)]
            e.rolling_shutter_device(bufs[0].addr, w * 4, readout=1.0, frame=1)
            e.synchronize()
            put(out, "rs1_device", bufs[0].get((h, w, 4), np.uint8))
            put(out, "bidir_again", e.compute_flow_bidirectional())
        finally:
            e.close()
            for d in bufs:
                d.free()
        return out
    return scenario


def batch_form():
    """two active pairs of three: slot 2's part of the block holds nothing but what the allocation held"""
    import eppm_amd
    a, b = stills()["sub"]
    h, w, _ = a.shape

    def scenario():
        out = {}
        e = eppm_amd.EPPMBatch(h, w, 3)
        try:
            e.set_data([(a, b), (b, a)])
            put(out, "bidir", e.compute_flow_bidirectional())
            put(out, "rs0", e.rolling_shutter(readout=1.0))
            put(out, "rs1", e.rolling_shutter(readout=1.0, frame=1))
            e.set_data([(a, b), (b, a), (np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1]))])
            put(out, "forward3", e.compute_flow())
            put(out, "rs0_3", e.rolling_shutter(readout=0.75, axis=1))
        finally:
            e.close()
        return out
    return scenario


def caller_planes():
    """eppm_rolling_shutter_frames: the velocity plane lives in the launchers' scratch"""
    import ctypes as C
    import eppm_amd
    from eppm_amd._lib import check, lib
    a, b = stills()["sub"]
    h, w, _ = a.shape
    ys, xs = np.mgrid[0:h, 0:w]
    flow = np.ascontiguousarray(np.stack([6 * np.sin(xs / 9.0), 5 * np.cos(ys / 7.0)], -1).astype(np.float32))

    def scenario():
        out = {}
        bufs = [DevMem(rgba_of(a)), DevMem(flow), DevMem(nbytes=h * w * 4)]
        try:
            for frame, axis in ((0, 0), (1, 1)):
                p = eppm_amd.RSParams(readout=1.0, axis=axis)
                check(lib().eppm_rolling_shutter_frames(bufs[2].addr, w * 4, bufs[0].addr, w * 4, bufs[1].addr, h, w, frame, C.byref(p)),
                      "eppm_rolling_shutter_frames")
                put(out, f"frames{frame}", bufs[2].get((h, w, 4), np.uint8))
        finally:
            for d in bufs:
                d.free()
        return out
    return scenario


@pytest.mark.parametrize("form", ["first_call", "after_forward", "batch", "caller_planes"])
def test_rolling_shutter_results_do_not_depend_on_what_memory_held(form):
    make = {"first_call": lambda: context_forms(False), "after_forward": lambda: context_forms(True), "batch": batch_form, "caller_planes": caller_planes}
    base = across_fills(make[form](), f"rolling-shutter correction, {form}")
    rs = {k: v for k, v in base.items() if (k.startswith("rs") or k.startswith("frames")) and v.size > 1000}
    assert len(rs) >= 2 and len({v.tobytes() for v in rs.values()}) == len(rs)          # results, and no two the same
