"""The hand-over of a per-clip stage object between streams: a step on another stream than the last waits for the
object's event, an asynchronous getter runs behind the last step and the next step on any stream behind the getter."""
import ctypes as C

import numpy as np
import pytest

from test_tfilter_cpu import _vectors, moving_clip, same_bits
from tfilter_tol_child import rgba, to_device

pytestmark = pytest.mark.gpu


def test_a_filter_stepped_from_two_streams_equals_the_host_chain():
    """context step -> frame_device -> step_frames on the launcher stream -> context step, with no host synchronisation in between: the
    state and the frame equal seed_host + 3 x step_host bit for bit, and the plane copied after the first step is the first step's frame.
    96x128: the kernel is not under test (tests/test_tfilter_gpu.py), the order of its launches and copies on two streams is."""
    import eppm_amd
    from eppm_amd import io
    from eppm_amd._lib import check, lib
    h, w = 96, 128
    _, noisy, _, _ = moving_clip(h, w, 3, seed=41)
    rng = np.random.default_rng(12)
    su, sv = _vectors(rng, h, w, 0.4)                   # the synthetic backward flow and mask of the step on caller planes
    socc = np.where(rng.random((h, w)) < 0.7, 0, rng.integers(0, 4, (h, w))).astype(np.uint8)
    e = eppm_amd.EPPM(); e.init(h, w)
    e.set_data(noisy[0], noisy[1])
    flt = eppm_amd.TemporalFilter(e)
    d_bwd, d_occ2 = to_device(np.zeros((h, w, 2), np.float32)), to_device(np.zeros((h, w), np.uint8))          # the context's results, read at the end
    d_first = to_device(np.zeros((h, w, 4), np.uint8))
    planes = [to_device(rgba(noisy[1])), to_device(rgba(noisy[2])), to_device(np.stack([su, sv], -1).astype(np.float32)), to_device(socc)]
    try:
        e.compute_flow_bidirectional_device(d_flow_bwd=d_bwd.value, d_occ2=d_occ2.value)
        flt.step()                                                                                     # the context's stream
        flt.frame_device(0, d_first.value, w * 4)                                                      # a copy behind it
        flt.step_frames(0, planes[0].value, planes[1].value, w * 4, planes[2].value, planes[3].value)  # the launcher stream
        flt.step()                                                                                     # the context's stream again
        state, frame = flt.state(0), flt.frame(0)
        bwd, occ2, first = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8), np.empty((h, w, 4), np.uint8)
        for dst, src in ((bwd, d_bwd), (occ2, d_occ2), (first, d_first)):
            check(lib().eppm_memcpy_d2h(dst.ctypes.data_as(C.c_void_p), src, C.c_size_t(dst.nbytes)), "d2h")
    finally:
        flt.close(); e.close()
        for p in [d_bwd, d_occ2, d_first] + planes:
            lib().eppm_free_device(p)
    bu, bv = np.ascontiguousarray(bwd[..., 0]), np.ascontiguousarray(bwd[..., 1])
    acc1, rgb1 = io.tfilter_step_host(io.tfilter_seed_host(noisy[0]), noisy[1], bu, bv, occ2)
    acc2, _ = io.tfilter_step_host(acc1, noisy[2], su, sv, socc)
    acc3, rgb3 = io.tfilter_step_host(acc2, noisy[1], bu, bv, occ2)
    assert (acc1[..., 3] >= 2).mean() > 0.1 and not same_bits(acc3, acc1) and not same_bits(acc3, acc2)          # the steps blended and differ
    assert np.array_equal(first[..., :3], rgb1), "the plane copied behind the first step"
    assert same_bits(state, acc3), "state after the three steps"
    assert np.array_equal(frame, rgb3), "frame after the three steps"
