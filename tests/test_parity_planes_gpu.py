"""The exact library's column-parity planes: the PatchMatch random search and cost field at patch radius 9 read a
target row as 3 buffer loads of 4-byte texels and unpack each word on the device.  The unpack must give the float4 texel bit for bit,
and the planes must exist (and be read) exactly where the library says."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _unpack(words):
    from eppm_amd._lib import check, lib
    w = np.ascontiguousarray(words, np.uint32)
    y = np.empty((w.size, 2, 4), np.float32)
    check(lib().eppm_probe_unpack_texel(w.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), w.size), "probe_unpack_texel")
    return y[:, 0], y[:, 1]


def test_unpack_texel_every_byte_and_census():
    """Every byte value in each of R, G, B, against a spread of census bytes: unpack_texel(w) == make_texel(w, w >> 24), and both equal
    the texture model's c / 255.0f with the census byte in all four bytes of the fourth word."""
    b = np.arange(256, dtype=np.uint32)
    census = np.array([0, 1, 2, 0x55, 0x7f, 0x80, 0xaa, 0xfe, 0xff], np.uint32)
    words = [b | (((b * 7 + 3) & 0xff) << 8) | (((255 - b) & 0xff) << 16) | (c << 24) for c in census]
    words += [(b << 8) | (c << 24) for c in census] + [(b << 16) | ((b ^ 0x3c) << 24)]
    rng = np.random.default_rng(5)
    words.append(rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32))
    w = np.concatenate(words)
    got, ref = _unpack(w)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    for k in range(3):
        assert np.array_equal(got[:, k], ((w >> (8 * k)) & 0xff).astype(np.float32) / np.float32(255))
    assert np.array_equal(got[:, 3].view(np.uint32), (w >> 24) * np.uint32(0x01010101))
    # the reason for the exact division: one multiply by fl(1/255) differs for 126 of the 256 bytes
    assert int((b.astype(np.float32) * np.float32(1 / 255) != b.astype(np.float32) / np.float32(255)).sum()) == 126


def _parity(ctx):
    from eppm_amd._lib import check, lib
    pitch, pad, kernels = C.c_int(), C.c_int(), C.c_int()
    check(lib().eppm_probe_pm_parity(ctx, C.byref(pitch), C.byref(pad), C.byref(kernels)), "probe_pm_parity")
    return pitch.value, pad.value, kernels.value


def _same(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("patch_r", [9, 17])
def test_exact_library_builds_and_reads_parity_planes_at_radius_9(patch_r):
    """Radius 9: a context has the planes, in the tolerance library's layout (pad = R + 1 rounded up to even), and the random search and
    the cost field read them; phase A of the sweeps keeps its gathers (slower on the planes).  Radius 17: no planes, nothing reads them.
    Either way the flow is the CPU oracle's, bit for bit, in a one-pair and in a two-pair batch context."""
    import eppm_amd
    from eppm_amd import synth
    from oracle import oracle as O
    h, w = 96, 128
    a, b, _, _ = synth.make_pair(h, w, seed=11, max_flow=6.0)
    e = eppm_amd.EPPM(device=0, params=eppm_amd.Params(patch_r=patch_r))
    e.init(a, b, h, w)
    pitch, pad, kernels = _parity(e._ctx)
    u, v = e.compute_flow()
    e.close()
    if patch_r == 9:
        wl = O.pyr_init_dim(h, w)[1][-1]          # width of the PatchMatch level
        assert (pad, kernels) == (10, 1 | 4) and pitch == (wl + 2 * pad + 1) // 2 + 1, (pitch, pad, kernels)
    else:
        assert (pitch, pad, kernels) == (0, 0, 0)
    op = O.default_params(patch_r=patch_r)
    ou, ov = O.compute_flow(a, b, params=op)
    assert _same(u, ou) and _same(v, ov)
    bat = eppm_amd.EPPMBatch(h, w, 2, device=0, params=eppm_amd.Params(patch_r=patch_r))
    assert _parity(bat._ctx) == (pitch, pad, kernels)
    bat.set_data([(a, b), (b, a)])
    (u0, v0), (u1, v1) = bat.compute_flow()
    bat.close()
    ru, rv = O.compute_flow(b, a, params=op)
    assert _same(u0, ou) and _same(v0, ov) and _same(u1, ru) and _same(v1, rv)
