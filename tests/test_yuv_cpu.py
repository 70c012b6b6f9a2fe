"""CPU tests of the Y'CbCr 4:2:0 conversion (include/eppm_yuv.h): the host forms against a numpy restatement written
here from the specification (it reads none of eppm_amd/csrc/yuv.h), the fixed point against float64, the round trip of every colour, the
anchors, the binding table against the header, and the argument errors.  tests/test_yuv_gpu.py holds the kernels to the host forms."""
import ctypes as C
import itertools
import math
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import _lib, yuv
from test_abi_cpu import _declared, _exported, _prototypes

# ---- the restatement ----
KRB = {0: (0.299, 0.114), 1: (0.2126, 0.0722), 2: (0.2627, 0.0593)}
DEPTH_FORMS = [(8, 0), (10, 1), (10, 0), (12, 0), (16, 0)]          # (depth, msb_aligned)
SIZES = [(4, 4), (5, 7), (7, 5), (45, 67)]


def formats(layouts=(0, 1), forms=DEPTH_FORMS, matrices=(0, 1, 2), ranges=(0, 1), sitings=(0, 1)):
    for lay, (d, msb), m, fr, s in itertools.product(layouts, forms, matrices, ranges, sitings):
        yield yuv.YuvFormat(layout=lay, depth=d, msb_aligned=msb, matrix=m, full_range=fr, siting=s)


def fmt_id(f):
    return "{layout}-{depth}{msb_aligned}-m{matrix}-r{full_range}-s{siting}".format(**f.as_dict())


def rnd(x):
    return math.floor(x + 0.5)


def coeffs(f):
    Kr, Kb = KRB[f.matrix]
    Kg = 1.0 - Kr - Kb
    d = f.depth
    peak = (1 << d) - 1
    yr = float(peak) if f.full_range else float(219 << (d - 8))
    cr = float(peak) if f.full_range else float(224 << (d - 8))
    k = dict(peak=peak, yr=yr, cr=cr, yoff=0 if f.full_range else 16 << (d - 8), coff=1 << (d - 1), Kr=Kr, Kb=Kb, Kg=Kg)
    s = float(1 << 20)
    k["cy"] = rnd(s * 255.0 / yr)
    k["crv"] = rnd(s * 255.0 * 2.0 * (1.0 - Kr) / cr)
    k["cbu"] = rnd(s * 255.0 * 2.0 * (1.0 - Kb) / cr)
    k["cgu"] = rnd(s * 255.0 * 2.0 * (1.0 - Kb) * Kb / Kg / cr)
    k["cgv"] = rnd(s * 255.0 * 2.0 * (1.0 - Kr) * Kr / Kg / cr)
    S = 24 - d
    t = float(1 << S)
    K = (Kr, Kg, Kb)
    k["S"] = S
    k["fy"] = [rnd(t * (yr / 255.0 * K[c])) for c in range(3)]
    k["fu"] = [rnd(t * (cr / 255.0 * ((1.0 if c == 2 else 0.0) - K[c]) / (2.0 * (1.0 - Kb)))) for c in range(3)]
    k["fv"] = [rnd(t * (cr / 255.0 * ((1.0 if c == 0 else 0.0) - K[c]) / (2.0 * (1.0 - Kr)))) for c in range(3)]
    return k


def decode(words, f):
    w = words.astype(np.int64)
    if f.depth == 8:
        return w
    return w >> (16 - f.depth) if f.msb_aligned else w & ((1 << f.depth) - 1)


def encode(values, f):
    if f.depth == 8:
        return values.astype(np.uint8)
    return (values << (16 - f.depth) if f.msb_aligned else values).astype(np.uint16)


def taps_center(n_luma, n):
    x = np.arange(n_luma)
    i = x >> 1
    even = (x & 1) == 0
    a = np.where(even, i - 1, i)
    b = np.where(even, i, i + 1)
    return np.clip(a, 0, n - 1), np.clip(b, 0, n - 1), np.where(even, 1, 3), np.where(even, 3, 1)


def taps_left(n_luma, n):
    x = np.arange(n_luma)
    j = x >> 1
    even = (x & 1) == 0
    return j, np.clip(np.where(even, j, j + 1), 0, n - 1), np.where(even, 4, 2), np.where(even, 0, 2)


def upsample(c, h, w, siting):
    ch, cw = c.shape
    r0, r1, v0, v1 = taps_center(h, ch)
    c0, c1, h0, h1 = taps_center(w, cw) if siting == 1 else taps_left(w, cw)
    total = np.zeros((h, w), np.int64)
    for rr, wv in ((r0, v0), (r1, v1)):
        for cc, wh in ((c0, h0), (c1, h1)):
            total += wv[:, None] * wh[None, :] * c[rr][:, cc]
    return (total + 8) >> 4


def matrix_to_rgb(Y, Cb, Cr, k):
    y, u, v = Y - k["yoff"], Cb - k["coff"], Cr - k["coff"]
    half = 1 << 19
    R = np.clip((k["cy"] * y + k["crv"] * v + half) >> 20, 0, 255)
    G = np.clip((k["cy"] * y - k["cgu"] * u - k["cgv"] * v + half) >> 20, 0, 255)
    B = np.clip((k["cy"] * y + k["cbu"] * u + half) >> 20, 0, 255)
    return R, G, B


def chroma_planes(planes, f):
    if f.layout == 0:
        return decode(planes[1][:, 0::2], f), decode(planes[1][:, 1::2], f)
    return decode(planes[1], f), decode(planes[2], f)


def r_to_rgb(planes, f):
    """planes: arrays of words (views of their first columns if padded) -> (h, w, 3) uint8"""
    k = coeffs(f)
    Y = decode(planes[0], f)
    h, w = Y.shape
    cb, cr = chroma_planes(planes, f)
    R, G, B = matrix_to_rgb(Y, upsample(cb, h, w, f.siting), upsample(cr, h, w, f.siting), k)
    return np.stack([R, G, B], -1).astype(np.uint8)


def block_sums(rgb, siting):
    """(ch, cw, 3) sums over every block's support and the shift of their weight"""
    h, w, _ = rgb.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    p = rgb.astype(np.int64)
    i, j = np.arange(ch), np.arange(cw)
    rows = [np.clip(2 * i, 0, h - 1), np.clip(2 * i + 1, 0, h - 1)]
    if siting == 1:
        cols, shift = [(np.clip(2 * j, 0, w - 1), 1), (np.clip(2 * j + 1, 0, w - 1), 1)], 2
    else:
        cols, shift = [(np.clip(2 * j - 1, 0, w - 1), 1), (np.clip(2 * j, 0, w - 1), 2), (np.clip(2 * j + 1, 0, w - 1), 1)], 3
    s = np.zeros((ch, cw, 3), np.int64)
    for r in rows:
        for c, wt in cols:
            s += wt * p[r][:, c]
    return s, shift


def r_from_rgb(rgb, f):
    """-> the format's planes as arrays of words"""
    k = coeffs(f)
    S = k["S"]
    p = rgb.astype(np.int64)
    Y = np.clip(((k["fy"][0] * p[..., 0] + k["fy"][1] * p[..., 1] + k["fy"][2] * p[..., 2] + (1 << (S - 1))) >> S) + k["yoff"], 0, k["peak"])
    s, shift = block_sums(rgb, f.siting)
    sh = S + shift
    out = []
    for m in (k["fu"], k["fv"]):
        out.append(np.clip(((m[0] * s[..., 0] + m[1] * s[..., 1] + m[2] * s[..., 2] + (1 << (sh - 1))) >> sh) + k["coff"], 0, k["peak"]))
    if f.layout == 0:
        return [encode(Y, f), encode(np.stack(out, -1).reshape(out[0].shape[0], -1), f)]
    return [encode(Y, f), encode(out[0], f), encode(out[1], f)]


# ---- frames for the tests (shared with tests/test_yuv_gpu.py) ----
def plane_shapes(f, h, w):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return [(h, w), (ch, 2 * cw)] if f.layout == 0 else [(h, w), (ch, cw), (ch, cw)]


def random_frame(f, h, w, rng, pad=5):
    """A YuvFrame of random words over the whole word range (junk in the ignored bits of 10- and 12-bit words included) whose rows are
    `pad` samples further apart than they are long"""
    dt = np.uint16 if f.depth > 8 else np.uint8
    planes = []
    for r, c in plane_shapes(f, h, w):
        full = rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), (r, c + pad), dtype=np.int64).astype(dt)
        planes.append(full[:, :c])
    return yuv.YuvFrame(planes, f)


def padded_like(f, h, w, fill, pad=5):
    dt = np.uint16 if f.depth > 8 else np.uint8
    fulls = [np.full((r, c + pad), fill, dt) for r, c in plane_shapes(f, h, w)]
    return fulls, yuv.YuvFrame([a[:, :a.shape[1] - pad] for a in fulls], f)


def host_to_rgb_strided(frame, pad=4, fill=0xA5):
    full = np.full((frame.h, frame.w * 3 + pad), fill, np.uint8)
    planes, strides = frame._args()
    rc = eppm_amd.lib().eppm_yuv_to_rgb_host(C.byref(frame.fmt), planes, strides, full.ctypes.data, full.strides[0], frame.h, frame.w)
    assert rc == 0, eppm_amd.lib().eppm_last_error()
    return full


def host_from_rgb_strided(rgb, f, fill=0xA5):
    h, w, _ = rgb.shape
    fulls, frame = padded_like(f, h, w, fill)
    full_rgb = np.zeros((h, w * 3 + 7), np.uint8)
    full_rgb[:, :w * 3] = rgb.reshape(h, -1)
    planes, strides = frame._args()
    rc = eppm_amd.lib().eppm_yuv_from_rgb_host(C.byref(f), full_rgb.ctypes.data, full_rgb.strides[0], planes, strides, h, w)
    assert rc == 0, eppm_amd.lib().eppm_last_error()
    return fulls, frame


# ---- 1. host forms against the restatement ----
@pytest.mark.parametrize("f", list(formats()), ids=fmt_id)
def test_host_forms_equal_the_restatement(f):
    rng = np.random.default_rng(zlib.crc32(fmt_id(f).encode()))
    for h, w in SIZES:
        frame = random_frame(f, h, w, rng)
        full = host_to_rgb_strided(frame)
        want = r_to_rgb(frame.planes, f)
        assert np.array_equal(full[:, :w * 3].reshape(h, w, 3), want), (h, w)
        assert (full[:, w * 3:] == 0xA5).all()                      # bytes outside the rows stay untouched
        assert np.array_equal(yuv.to_rgb(frame), want)
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rgb[0, 0], rgb[-1, -1] = 0, 255
        fulls, got = host_from_rgb_strided(rgb, f)
        for a, b, whole in zip(got.planes, r_from_rgb(rgb, f), fulls):
            assert np.array_equal(a, b), (h, w)
            assert (whole[:, a.shape[1]:] == 0xA5).all()
        for a, b in zip(yuv.from_rgb(rgb, f).planes, got.planes):
            assert np.array_equal(a, b)


def test_the_clamps_are_reached():
    """random words over the whole range leave the nominal range: both ends of the RGB clamp occur at every depth form"""
    for d, msb in DEPTH_FORMS:
        rgb = yuv.to_rgb(random_frame(yuv.YuvFormat(depth=d, msb_aligned=msb), 45, 67, np.random.default_rng(1)))
        assert (rgb == 0).any() and (rgb == 255).any()


# ---- 2. fixed point against float64 ----
def float_to_rgb(Y, Cb, Cr, k):
    y = (Y - k["yoff"]) / k["yr"]
    u, v = (Cb - k["coff"]) / k["cr"], (Cr - k["coff"]) / k["cr"]
    R = y + 2.0 * (1.0 - k["Kr"]) * v
    B = y + 2.0 * (1.0 - k["Kb"]) * u
    G = y - 2.0 * (1.0 - k["Kb"]) * k["Kb"] / k["Kg"] * u - 2.0 * (1.0 - k["Kr"]) * k["Kr"] / k["Kg"] * v
    return [np.clip(np.floor(255.0 * c + 0.5), 0, 255) for c in (R, G, B)]


def float_from_rgb(mean_rgb, k):
    R, G, B = [mean_rgb[..., c] for c in range(3)]
    Yp = k["Kr"] * R + k["Kg"] * G + k["Kb"] * B
    Y = k["yr"] / 255.0 * Yp
    Cb = k["cr"] / 255.0 * (B - Yp) / (2.0 * (1.0 - k["Kb"]))
    Cr = k["cr"] / 255.0 * (R - Yp) / (2.0 * (1.0 - k["Kr"]))
    return [np.clip(np.floor(c + off + 0.5), 0, k["peak"]) for c, off in ((Y, k["yoff"]), (Cb, k["coff"]), (Cr, k["coff"]))]


@pytest.mark.parametrize("f", list(formats(layouts=(1,))), ids=fmt_id)
def test_fixed_point_is_within_one_of_float64(f):
    """both directions of the host forms against floor(float64 formula + 0.5): the matrix on the upsampled chroma (whose integer blend test
    1 holds to the specification), and the forward matrix on the mean of every block's support"""
    rng = np.random.default_rng(7)
    k = coeffs(f)
    h, w = 45, 67
    frame = random_frame(f, h, w, rng, pad=0)
    got = yuv.to_rgb(frame).astype(np.int64)
    cb, cr = chroma_planes(frame.planes, f)
    want = float_to_rgb(decode(frame.planes[0], f).astype(np.float64), upsample(cb, h, w, f.siting).astype(np.float64),
                        upsample(cr, h, w, f.siting).astype(np.float64), k)
    assert max(np.abs(got[..., c] - want[c]).max() for c in range(3)) <= 1
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = yuv.from_rgb(rgb, f)
    s, shift = block_sums(rgb, f.siting)
    wy = float_from_rgb(rgb.astype(np.float64), k)[0]
    _, wcb, wcr = float_from_rgb(s / float(1 << shift), k)
    for a, b in zip(out.planes, (wy, wcb, wcr)):
        assert np.abs(decode(a, f) - b).max() <= 1


# ---- 3. round trip of every colour ----
ROUND_TRIP_BOUND = {(8, 0): 2, (8, 1): 1}         # (depth, full_range) -> levels; depth 10 and above: 0


def pointwise_round_trip(rgb, f):
    """flat frames pass the chroma filters exactly (4c and 8c over weight 4 and 8; 16c over 16), so a flat frame's round trip is the two
    matrices on its colour: rgb (n, 3) -> (n, 3)"""
    k = coeffs(f)
    S = k["S"]
    p = rgb.astype(np.int64)
    out = []
    for m, off in ((k["fy"], k["yoff"]), (k["fu"], k["coff"]), (k["fv"], k["coff"])):
        out.append(np.clip(((m[0] * p[:, 0] + m[1] * p[:, 1] + m[2] * p[:, 2] + (1 << (S - 1))) >> S) + off, 0, k["peak"]))
    return np.stack(matrix_to_rgb(out[0], out[1], out[2], k), -1)


@pytest.mark.parametrize("depth,full_range", [(8, 0), (8, 1), (10, 0), (10, 1), (12, 0), (16, 0)])
@pytest.mark.parametrize("matrix", [0, 1, 2])
def test_round_trip_of_all_colours(depth, full_range, matrix):
    """all 2^24 colours (one 4096 x 4096 image's worth, each as a flat frame) through the restatement, and the host forms on flat
    frames of the worst colours found: at most 2 levels at 8-bit limited range, 1 at 8-bit full range, 0 from depth 10"""
    f = yuv.YuvFormat(layout=1, depth=depth, matrix=matrix, full_range=full_range)
    bound = ROUND_TRIP_BOUND.get((depth, full_range), 0)
    worst, worst_rgb = 0, None
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r0 in range(0, 256, 16):
        rgb = np.stack([np.repeat(np.arange(r0, r0 + 16), 65536), np.tile(g.ravel(), 16), np.tile(b.ravel(), 16)], -1)
        err = np.abs(pointwise_round_trip(rgb, f) - rgb).max(axis=1)
        if worst_rgb is None or err.max() > worst:
            worst, worst_rgb = int(err.max()), rgb[int(err.argmax())]
    print(f"depth {depth} full_range {full_range} matrix {matrix}: worst round-trip error {worst} at {worst_rgb.tolist()}")
    assert worst <= bound
    for colour in (worst_rgb, np.array([255, 0, 0]), np.array([0, 255, 0]), np.array([0, 0, 255]), np.array([255, 255, 255]), np.array([0, 0, 0])):
        for siting, lay in ((0, 0), (1, 1)):
            ff = yuv.YuvFormat(f, siting=siting, layout=lay)
            flat = np.broadcast_to(colour.astype(np.uint8), (5, 7, 3))
            back = yuv.to_rgb(yuv.from_rgb(flat, ff))
            assert np.array_equal(back, np.broadcast_to(pointwise_round_trip(colour[None], f)[0].astype(np.uint8), (5, 7, 3)))


@pytest.mark.parametrize("depth,full_range,matrix", [(8, 0, 1), (8, 1, 0), (10, 0, 2), (12, 0, 1), (16, 1, 0)])
def test_host_forms_round_trip_a_million_colours(depth, full_range, matrix):
    """the C host forms themselves against the bound: every (G, B) with 16 values of R, each colour a 4 x 4 block of a 1024 x 1024 image at
    CENTER siting.  A block's 2 x 2 chroma samples are sums over its own colour, and its four inner pixels blend those samples only, so
    they carry the flat round trip of the colour: within the class's bound, and equal to the restatement's pointwise result"""
    f = yuv.YuvFormat(layout=1, depth=depth, matrix=matrix, full_range=full_range, siting=1)
    bound = ROUND_TRIP_BOUND.get((depth, full_range), 0)
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for r in range(3, 256, 16):
        colours = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)                   # (256, 256, 3)
        img = np.repeat(np.repeat(colours, 4, axis=0), 4, axis=1)
        back = yuv.to_rgb(yuv.from_rgb(img, f))
        inner = back[1::4, 1::4]
        assert all(np.array_equal(back[dy::4, dx::4], inner) for dy in (1, 2) for dx in (1, 2))
        assert np.abs(inner.astype(np.int64) - colours).max() <= bound
        assert np.array_equal(inner, pointwise_round_trip(colours.reshape(-1, 3), f).reshape(256, 256, 3))


# ---- 4. anchors ----
@pytest.mark.parametrize("f", list(formats(layouts=(1,), ranges=(0,))), ids=fmt_id)
def test_limited_range_black_and_white(f):
    s = f.depth - 8
    for (y, c), want in (((16, 128), 0), ((235, 128), 255)):
        planes = [encode(np.full(shp, v << s, np.int64), f) for shp, v in zip(plane_shapes(f, 4, 6), (y, c, c))]
        assert (yuv.to_rgb(yuv.YuvFrame(planes, f)) == want).all()
    assert [int(p[0, 0]) for p in r_from_rgb(np.zeros((2, 2, 3), np.uint8), f)] == [int(encode(np.int64(v << s), f)) for v in (16, 128, 128)]


@pytest.mark.parametrize("f", list(formats(layouts=(0,), ranges=(1,), forms=[(8, 0)])), ids=fmt_id)
def test_full_range_grey_is_grey(f):
    for g in range(256):
        planes = [np.full(shp, v, np.uint8) for shp, v in zip(plane_shapes(f, 2, 2), (g, 128))]
        assert (yuv.to_rgb(yuv.YuvFrame(planes, f)) == g).all()
        assert (yuv.from_rgb(np.full((2, 2, 3), g, np.uint8), f).planes[0] == g).all()


# ---- 6. the ABI ----
def test_binding_table_equals_the_header():
    protos = _prototypes("eppm_yuv.h")
    assert list(protos) == list(_lib._YUV_ABI) and len(protos) == 19
    wrong = {n: (_lib._YUV_ABI[n], want) for n, want in protos.items() if _lib._YUV_ABI[n] != want}
    assert not wrong, wrong
    assert set(protos) == _declared("eppm_yuv.h")
    assert not set(protos) & (set(_lib.SYMBOLS) | set(_lib.TEST_SYMBOLS)) and not set(protos) & set(_lib.SIGNATURES)
    assert not [n for n in protos if n.startswith("eppm_test") or n.startswith("eppm_probe")]
    for variant in ("", "test", "tol", "tol_test"):
        assert set(protos) <= _exported(eppm_amd.lib_path(variant)), variant
    L = eppm_amd.lib()
    for n, (res, args) in _lib._YUV_ABI.items():
        fn = getattr(L, n)
        assert fn.restype == res and list(fn.argtypes) == args, n


def test_default_format():
    want = _lib.CYuvFormat()
    assert eppm_amd.lib().eppm_yuv_default_format(C.byref(want)) == 0
    assert yuv.YuvFormat().as_dict() == want.as_dict() == dict(layout=0, depth=8, msb_aligned=0, matrix=1, full_range=0, siting=0)
    assert eppm_amd.YuvFormat(depth=10).depth == 10
    with pytest.raises(TypeError, match="^unknown yuv format field nonsense$"):
        yuv.YuvFormat(nonsense=1)


def test_plane_dims():
    assert yuv.plane_dims(yuv.YuvFormat(), 5, 7) == [(5, 7), (3, 8)]
    assert yuv.plane_dims(yuv.YuvFormat(layout=1, depth=10), 5, 7) == [(5, 14), (3, 8), (3, 8)]
    rows, row = C.c_int(9), C.c_int(9)
    f = yuv.YuvFormat()
    assert eppm_amd.lib().eppm_yuv_plane_dims(C.byref(f), 5, 7, 2, C.byref(rows), C.byref(row)) == 0 and (rows.value, row.value) == (0, 0)
    assert eppm_amd.lib().eppm_yuv_plane_dims(C.byref(f), 5, 7, 3, C.byref(rows), C.byref(row)) == 1


@pytest.mark.parametrize("change,message", [
    (dict(layout=2), "unknown layout"), (dict(depth=9), "depth is not 8, 10, 12 or 16"), (dict(msb_aligned=1), "msb_aligned with depth 8"),
    (dict(matrix=3), "unknown matrix"), (dict(matrix=-1), "unknown matrix"), (dict(full_range=2), "full_range"), (dict(siting=2), "unknown siting"),
    (dict(depth=10, msb_aligned=2), "msb_aligned is not 0 or 1")])
def test_format_errors(change, message):
    L = eppm_amd.lib()
    f = yuv.YuvFormat(**change)
    y, uv, rgb = np.zeros((4, 8), np.uint16), np.zeros((2, 8), np.uint16), np.zeros((4, 4, 3), np.uint8)
    planes, strides = (C.c_void_p * 3)(y.ctypes.data, uv.ctypes.data, uv.ctypes.data), (C.c_size_t * 3)(16, 16, 16)
    for rc in (L.eppm_yuv_to_rgb_host(C.byref(f), planes, strides, rgb.ctypes.data, 12, 4, 4),
               L.eppm_yuv_from_rgb_host(C.byref(f), rgb.ctypes.data, 12, planes, strides, 4, 4),
               L.eppm_yuv_to_rgba(C.byref(f), planes, strides, rgb.ctypes.data, 16, 4, 4, None),           # refused before any GPU call
               L.eppm_yuv_from_rgba(C.byref(f), rgb.ctypes.data, 16, planes, strides, 4, 4, None)):
        assert rc == 1 and message in L.eppm_last_error().decode()


def test_plane_errors():
    L = eppm_amd.lib()
    y, uv, rgb = np.zeros((4, 8), np.uint16), np.zeros((2, 8), np.uint16), np.zeros((4, 4, 3), np.uint8)

    def call(f, ptrs, strides, stride_rgb=12):
        return L.eppm_yuv_to_rgb_host(C.byref(f), (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*strides), rgb.ctypes.data, stride_rgb, 4, 4)
    ok = [y.ctypes.data, uv.ctypes.data, uv.ctypes.data]
    f8, f10, i420 = yuv.YuvFormat(), yuv.YuvFormat(depth=10), yuv.YuvFormat(layout=1)
    assert call(f8, ok, [4, 4, 0]) == 0 and call(f10, ok, [8, 8, 0]) == 0 and call(i420, ok, [4, 2, 2]) == 0
    assert call(f8, ok, [3, 4, 0]) == 1 and "pitch 3 of plane 0 is below the row's 4 bytes" in L.eppm_last_error().decode()
    assert call(f8, ok, [4, 3, 0]) == 1 and "plane 1" in L.eppm_last_error().decode()
    assert call(i420, ok, [4, 2, 1]) == 1 and "plane 2" in L.eppm_last_error().decode()
    assert call(f10, ok, [9, 8, 0]) == 1 and "odd pitch 9 of plane 0 for 16-bit words" in L.eppm_last_error().decode()
    assert call(f8, [ok[0], None, None], [4, 4, 0]) == 1 and "NULL plane 1" in L.eppm_last_error().decode()
    assert call(i420, [ok[0], ok[1], None], [4, 2, 2]) == 1 and "NULL plane 2" in L.eppm_last_error().decode()
    assert call(f8, [ok[0], ok[1], None], [4, 4, 0]) == 0                      # the third pointer is ignored for NV12
    assert call(f8, ok, [4, 4, 0], stride_rgb=11) == 1
    assert L.eppm_yuv_to_rgb_host(None, None, None, None, 0, 4, 4) == 1
    with pytest.raises(eppm_amd.EppmError, match="plane shapes"):
        yuv.YuvFrame.nv12(np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8))
    with pytest.raises(eppm_amd.EppmError, match="uint16"):
        yuv.YuvFrame.nv12(np.zeros((4, 4), np.uint8), np.zeros((2, 4), np.uint8), depth=10)


def test_context_calls_refuse_bad_arguments_without_a_gpu():
    L = eppm_amd.lib()
    f = yuv.YuvFormat()
    three = (C.c_void_p * 3)()
    strides = (C.c_size_t * 3)(4, 4, 0)
    assert L.eppm_yuv_set_images(None, C.byref(f), three, three, strides) == 1
    assert L.eppm_yuv_push_image(None, C.byref(f), three, strides) == 1
    assert L.eppm_yuv_batch_set_images_device(None, C.byref(f), 1, three, three, strides) == 1
    assert L.eppm_yuv_batch_push_images(None, C.byref(f), 1, three, strides, None) == 1
    e = eppm_amd.EPPM()
    with pytest.raises(eppm_amd.EppmError):
        e.push_frame_yuv(yuv.from_rgb(np.zeros((4, 4, 3), np.uint8)))
