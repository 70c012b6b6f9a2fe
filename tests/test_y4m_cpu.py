"""CPU tests of the y4m files (include/eppm_yuv.h: eppm_y4m_*; eppm_amd.yuv.read_y4m / write_y4m): round trips between the library's
reader and writer and the Python restatement of both, every accepted header tag as a byte literal, every refusal by its message, and
truncated files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import eppm_amd
from eppm_amd import yuv
from test_yuv_cpu import formats, fmt_id


def clip(fmt, h, w, n, seed=0):
    rng = np.random.default_rng(seed)
    return [yuv.from_rgb(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), fmt) for _ in range(n)]


def same_frames(a, b):
    return len(a) == len(b) and all(x.fmt.as_dict() == y.fmt.as_dict() and all(np.array_equal(p, q) for p, q in zip(x.planes, y.planes))
                                    for x, y in zip(a, b))


Y4M_FORMATS = [f for f in formats(layouts=(1,), forms=[(8, 0), (10, 0), (12, 0), (16, 0)], matrices=(0,))]


@pytest.mark.parametrize("f", Y4M_FORMATS, ids=fmt_id)
@pytest.mark.parametrize("writer_native", [False, True], ids=["python-writer", "c-writer"])
def test_round_trip_between_the_two_implementations(tmp_path, f, writer_native):
    """Python writer -> C reader and C writer -> Python reader (and each with itself): the frames, the format and the rate come back; odd
    sizes; the matrix follows the size and the caller's override"""
    h, w = 5, 7
    frames = clip(f, h, w, 3)
    path = tmp_path / "a.y4m"
    assert yuv.write_y4m(path, frames, fps=(30000, 1001), native=writer_native) == 3
    for reader_native in (not writer_native, writer_native):
        r = yuv.read_y4m(path, native=reader_native)
        assert (r.h, r.w, r.fps) == (h, w, (30000, 1001)) and r.fmt.as_dict() == f.as_dict()       # 5 rows: BT.601, as written
        assert same_frames(list(r), frames)
        r = yuv.read_y4m(path, matrix=yuv.BT2020, native=reader_native)
        assert r.fmt.matrix == yuv.BT2020 and next(r).fmt.matrix == yuv.BT2020
        r.close()
    both = [tmp_path / "p.y4m", tmp_path / "c.y4m"]
    yuv.write_y4m(both[0], frames, native=False)
    yuv.write_y4m(both[1], frames, native=True)
    assert both[0].read_bytes() == both[1].read_bytes()                  # the two writers emit the same bytes
    assert both[0].read_bytes().startswith(b"YUV4MPEG2 W7 H5 F25:1 Ip A1:1 C420")


def test_matrix_follows_the_size(tmp_path):
    for h, want in ((719, yuv.BT601), (720, yuv.BT709)):
        path = tmp_path / f"{h}.y4m"
        path.write_bytes(b"YUV4MPEG2 W2 H%d F25:1\n" % h)
        for native in (False, True):
            assert yuv.read_y4m(path, native=native).fmt.matrix == want


HEADERS = [
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420jpeg\n", dict(depth=8, siting=yuv.CENTER, full_range=0)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420mpeg2\n", dict(depth=8, siting=yuv.LEFT, full_range=0)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420\n", dict(depth=8, siting=yuv.LEFT, full_range=0)),
    (b"YUV4MPEG2 W6 H4 F25:1\n", dict(depth=8, siting=yuv.LEFT, full_range=0)),
    (b"YUV4MPEG2 H4 W6 F24000:1001 I? A0:0 C420p10 XYSCSS=420P10\n", dict(depth=10, siting=yuv.LEFT, full_range=0)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420p12 XCOLORRANGE=LIMITED\n", dict(depth=12, siting=yuv.LEFT, full_range=0)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420p16 XCOLORRANGE=FULL\n", dict(depth=16, siting=yuv.LEFT, full_range=1)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420jpeg XCOLORRANGE=FULL\n", dict(depth=8, siting=yuv.CENTER, full_range=1)),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420p10 XEPPM_SITING=CENTER\n", dict(depth=10, siting=yuv.CENTER, full_range=0)),
]


@pytest.mark.parametrize("header,want", HEADERS, ids=[h[10:-1].decode().replace(" ", "_") for h, _ in HEADERS])
@pytest.mark.parametrize("native", [False, True], ids=["python", "c"])
def test_accepted_headers(tmp_path, header, want, native):
    f = yuv.YuvFormat(layout=yuv.I420, matrix=yuv.BT601, msb_aligned=0, **want)
    frame = clip(f, 4, 6, 1)[0]
    path = tmp_path / "h.y4m"
    path.write_bytes(header + b"FRAME\n" + b"".join(p.tobytes() for p in frame.planes) + b"FRAME Ip\n" + b"".join(p.tobytes() for p in frame.planes))
    r = yuv.read_y4m(path, native=native)
    assert r.fmt.as_dict() == f.as_dict() and (r.h, r.w) == (4, 6)
    assert same_frames(list(r), [frame, frame])


REFUSED = [
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420paldv\n", "C420paldv"), (b"YUV4MPEG2 W6 H4 F25:1 Ip C422\n", "C422"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C422p10\n", "C422p10"), (b"YUV4MPEG2 W6 H4 F25:1 Ip C444\n", "C444"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C444alpha\n", "C444alpha"), (b"YUV4MPEG2 W6 H4 F25:1 Ip Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip Cmono16\n", "Cmono16"), (b"YUV4MPEG2 W6 H4 F25:1 It C420\n", r"interlaced material \(It\)"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ib\n", r"interlaced material \(Ib\)"), (b"YUV4MPEG2 W6 H4 F25:1 Im\n", r"interlaced material \(Im\)"),
    (b"YUV4MPEG2 H4 F25:1 Ip\n", "malformed: missing W or H"), (b"YUV4MPEG2 W6 F25:1 Ip\n", "malformed: missing W or H"),
    (b"YUV4MPEG W6 H4\n", "malformed: no YUV4MPEG2 header line"), (b"YUV4MPEG2 W6 H4", "malformed: no YUV4MPEG2 header line"),
    (b"", "malformed: no YUV4MPEG2 header line"),
]


@pytest.mark.parametrize("header,message", REFUSED, ids=[m.replace(" ", "_") + str(i) for i, (_, m) in enumerate(REFUSED)])
@pytest.mark.parametrize("native", [False, True], ids=["python", "c"])
def test_refused_headers(tmp_path, header, message, native):
    path = tmp_path / "r.y4m"
    path.write_bytes(header + (b"FRAME\n" + bytes(36) if header.endswith(b"\n") else b""))
    with pytest.raises(eppm_amd.EppmError, match=message):
        yuv.read_y4m(path, native=native)


@pytest.mark.parametrize("native", [False, True], ids=["python", "c"])
def test_malformed_frames(tmp_path, native):
    head = b"YUV4MPEG2 W6 H4 F25:1 Ip C420\n"
    body = bytes(range(36))
    good = head + b"FRAME\n" + body
    for tail, message in ((b"FRAME\n" + body[:35], "truncated frame"), (b"FRAME\n" + body[:24], "truncated frame"), (b"FRAME\n", "truncated frame"),
                          (b"FRAM", "missing FRAME line"), (b"frame\n" + body, "missing FRAME line"), (body, "missing FRAME line"),
                          (b"FRAMEX\n" + body, "missing FRAME line")):
        path = tmp_path / "m.y4m"
        path.write_bytes(good + tail)
        r = yuv.read_y4m(path, native=native)
        first = next(r)                                         # the whole frame before the damage is delivered
        assert first.planes[0].tobytes() == body[:24] and first.planes[2].tobytes() == body[30:]
        with pytest.raises(eppm_amd.EppmError, match="malformed: " + message):
            next(r)
        r.close()
    path.write_bytes(head)                                      # no frame at all is a clean, empty clip
    assert list(yuv.read_y4m(path, native=native)) == []


def test_writer_refuses_what_a_y4m_file_cannot_hold(tmp_path):
    L = eppm_amd.lib()
    y = C.c_void_p()
    path = str(tmp_path / "w.y4m").encode()
    for f, message in ((yuv.YuvFormat(), "I420 planes"), (yuv.YuvFormat(layout=1, depth=10, msb_aligned=1), "low-aligned"), (yuv.YuvFormat(layout=1, depth=9), "depth")):
        assert L.eppm_y4m_open_write(C.byref(y), path, 4, 6, C.byref(f), 25, 1) == 1 and message in L.eppm_last_error().decode() and not y.value
    ok = yuv.YuvFormat(layout=1)
    assert L.eppm_y4m_open_write(C.byref(y), path, 4, 6, C.byref(ok), 0, 1) == 1 and L.eppm_y4m_open_write(C.byref(y), path, 0, 6, C.byref(ok), 25, 1) == 1
    assert L.eppm_y4m_open_write(C.byref(y), str(tmp_path / "no" / "dir.y4m").encode(), 4, 6, C.byref(ok), 25, 1) == 1
    with pytest.raises(eppm_amd.EppmError, match="I420"):
        yuv.write_y4m(tmp_path / "n.y4m", clip(yuv.YuvFormat(), 4, 6, 1))
    with pytest.raises(eppm_amd.EppmError, match="one format and size"):
        yuv.write_y4m(tmp_path / "n.y4m", clip(ok, 4, 6, 1) + clip(ok, 6, 6, 1))
    with pytest.raises(eppm_amd.EppmError, match="no frame"):
        yuv.write_y4m(tmp_path / "n.y4m", [])
    # a reader is no writer, and the other way round (EPPM_ERR_STATE)
    assert L.eppm_y4m_open_write(C.byref(y), path, 4, 6, C.byref(ok), 25, 1) == 0
    three, strides, got = (C.c_void_p * 3)(), (C.c_size_t * 3)(), C.c_int()
    assert L.eppm_y4m_read_frame(y, three, strides, C.byref(got)) == 3
    assert L.eppm_y4m_write_frame(y, three, strides) == 1                 # NULL planes
    assert L.eppm_y4m_close(y) == 0 and L.eppm_y4m_close(None) == 0
    with pytest.raises(eppm_amd.EppmError, match="cannot open"):
        yuv.read_y4m(tmp_path / "absent.y4m", native=True)


def test_y4m_code_under_sanitizers(tmp_path):
    """eppm_io.cpp's reader and writer (no GPU code) under ASan + UBSan in a program of their own: round trips at every depth into planes
    that end with their last row, every prefix of a good file, headers and FRAME lines without end, absurd and negative sizes
    (tests/csrc/y4m_sanitize_driver.cpp)."""
    exe = str(tmp_path / "y4m_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "y4m_sanitize_driver.cpp"), os.path.join(ROOT, "eppm_amd", "csrc", "eppm_io.cpp"), "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("native", [False, True], ids=["python", "c"])
def test_header_edge_cases_read_alike(tmp_path, native):
    """both readers: a later C tag replaces an earlier one whole; W, H and F are their leading digits only -- a sign or a blank is no
    number --; a rate beyond int, without a colon or with a tail is unknown (0:0), not an error"""
    path = tmp_path / "e.y4m"

    def header(line):
        path.write_bytes(line + b"\n")
        r = yuv.read_y4m(path, native=native)
        return r.h, r.w, r.fps, r.fmt.depth, r.fmt.siting
    assert header(b"YUV4MPEG2 W6 H4 F25:1 C420p10 C420jpeg") == (4, 6, (25, 1), 8, yuv.CENTER)
    assert header(b"YUV4MPEG2 W6 H4 F25:1 C420jpeg C420p12") == (4, 6, (25, 1), 12, yuv.LEFT)
    assert header(b"YUV4MPEG2 W6x H4 F9999999999999:0") == (4, 6, (2147483647, 0), 8, yuv.LEFT)
    for rate in (b"F25", b"F25:", b"F:1", b"F25:1x", b"F-25:1", b"F+25:1"):
        assert header(b"YUV4MPEG2 W6 H4 " + rate)[2] == (0, 0), rate
    for bad in (b"YUV4MPEG2 W+6 H4", b"YUV4MPEG2 W6 H-4", b"YUV4MPEG2 W6 H"):
        path.write_bytes(bad + b"\n")
        with pytest.raises(eppm_amd.EppmError, match="missing W or H"):
            yuv.read_y4m(path, native=native)
