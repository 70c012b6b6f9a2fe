"""Y'CbCr frames in poisoned memory ("Write-before-read of every allocation"; section 25): the context's host and device
forms, single and batch, under the fills 0xFF, 0x01 and 0x7F of the test option "alloc_fill".  Every plane and flow must be the bytes of
the unfilled run: the staging of a host frame -- its half of d_rgb and of the pinned h_rgb at depth 8; d_yuv and h_yuv, made by the
first call with 16-bit words -- is written, every row of every plane, before k_yuv_to_rgba reads exactly those bytes, and the kernel
writes every word of the raw planes' rows that the prepare kernels read.  Odd frame sizes: the chroma planes' last row and column."""
import pytest

from alloc_fill_child import across_fills, put

pytestmark = pytest.mark.gpu

H, W = 45, 67
PLANES = ("img1", "img2", "census1", "census2")


def frames(fmt_kw, n):
    import numpy as np
    from eppm_amd import yuv
    rng = np.random.default_rng(5)
    return [yuv.from_rgb(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), **fmt_kw) for _ in range(n)]


def single(fmt_kw, device_form):
    import eppm_amd
    f = frames(fmt_kw, 3)

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        keep = []
        try:
            e.init(H, W)
            for step in range(2):
                if device_form:
                    d = [x.to_device() for x in (f[:2] if step == 0 else f[2:])]
                    keep.extend(d)
                    e.set_data_yuv_device(f[0].fmt, *d) if step == 0 else e.push_frame_yuv_device(f[0].fmt, d[0])
                else:
                    e.set_data_yuv(f[0], f[1]) if step == 0 else e.push_frame_yuv(f[2])
                for level in range(len(e.level_dims())):
                    for name in PLANES:
                        put(out, f"step{step}.{name}.{level}", e.plane(name, level))
                put(out, f"step{step}.flow", list(e.compute_flow()))
        finally:
            e.close()
        return out
    return scenario


def batch(fmt_kw):
    """three slots of a four-slot context (the fourth slot's staging and planes stay as allocated), a push with a new clip in slot 1"""
    import eppm_amd
    f = frames(fmt_kw, 9)

    def scenario():
        out = {}
        b = eppm_amd.EPPMBatch(H, W, 4)
        try:
            b.set_data_yuv([(f[2 * k], f[2 * k + 1]) for k in range(3)])
            put(out, "flow0", [list(p) for p in b.compute_flow()])
            b.push_frames_yuv(f[6:9], [False, True, False])
            for k in range(3):
                for name in PLANES:
                    put(out, f"slot{k}.{name}", b.plane(k, name, 0))
            put(out, "flow1", [list(p) for p in b.compute_flow()])
        finally:
            b.close()
        return out
    return scenario


FORMATS = [dict(layout=0, depth=8), dict(layout=0, depth=10, msb_aligned=1), dict(layout=1, depth=16)]
IDS = ["nv12", "p010", "i420p16"]


@pytest.mark.parametrize("fmt_kw", FORMATS, ids=IDS)
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
def test_single_context(fmt_kw, device_form):
    across_fills(single(fmt_kw, device_form), f"yuv single {fmt_kw} device={device_form}")


@pytest.mark.parametrize("fmt_kw", FORMATS[:2], ids=IDS[:2])
def test_batch_context(fmt_kw):
    across_fills(batch(fmt_kw), f"yuv batch {fmt_kw}")
