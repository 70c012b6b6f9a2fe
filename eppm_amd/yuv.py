"""Y'CbCr 4:2:0 frames (include/eppm_yuv.h): NV12 / I420 planes of 8-bit samples or 16-bit words to and from RGB, on
the host and on the device, and y4m files.  The arithmetic is integer only: host forms and kernels agree byte for byte, and a context fed
with a YuvFrame holds exactly the planes it holds after the RGB call on to_rgb(frame)."""
import ctypes as C
import re

import numpy as np

from ._lib import CYuvFormat, EppmError, check, lib
from .api import _params

NV12, I420 = 0, 1
BT601, BT709, BT2020 = 0, 1, 2
LEFT, CENTER = 0, 1


def YuvFormat(fmt=None, **kw):
    """eppm_yuv_format with the library's defaults (NV12, 8 bit, BT.709, limited range, LEFT siting) or a copy of fmt, and the overrides kw
    (layout, depth, msb_aligned, matrix, full_range, siting)."""
    return _params(CYuvFormat, "eppm_yuv_default_format", "yuv format field", fmt, **kw)


def _same_format(a, b):
    return a.as_dict() == b.as_dict()


def plane_dims(fmt, h, w):
    """[(rows, bytes per row)] of the format's planes for an h x w frame"""
    out = []
    for p in range(2 if fmt.layout == NV12 else 3):
        rows, row = C.c_int(), C.c_int()
        check(lib().eppm_yuv_plane_dims(C.byref(fmt), h, w, p, C.byref(rows), C.byref(row)), "eppm_yuv_plane_dims")
        out.append((rows.value, row.value))
    return out


class YuvFrame:
    """The planes of one frame and their format.  planes: 2-D arrays of uint8 (depth 8) or uint16 whose rows may be further apart than
    their length (a view a[:, :n]); an NV12 chroma plane has 2 * ceil(w / 2) samples per row, Cb first."""

    def __init__(self, planes, fmt):
        self.fmt = YuvFormat(fmt)
        dt = np.uint16 if self.fmt.depth > 8 else np.uint8
        self.planes = []
        for p in planes:
            p = np.asarray(p)
            if p.ndim == 3:
                p = p.reshape(p.shape[0], -1)
            if p.ndim != 2 or p.dtype != dt:
                raise EppmError(f"YuvFrame: planes must be 2-D {np.dtype(dt).name} arrays at depth {self.fmt.depth}")
            if p.strides[1] != p.itemsize or p.strides[0] < p.shape[1] * p.itemsize:
                p = np.ascontiguousarray(p)
            self.planes.append(p)
        self.h, self.w = self.planes[0].shape
        want = [(r, b // self.planes[0].itemsize) for r, b in plane_dims(self.fmt, self.h, self.w)]
        if [p.shape for p in self.planes] != want:
            raise EppmError(f"YuvFrame: plane shapes {[p.shape for p in self.planes]}, the format needs {want}")

    @classmethod
    def nv12(cls, y, uv, fmt=None, **kw):
        return cls([y, uv], YuvFormat(fmt, **dict(kw, layout=NV12)))

    @classmethod
    def i420(cls, y, u, v, fmt=None, **kw):
        return cls([y, u, v], YuvFormat(fmt, **dict(kw, layout=I420)))

    def packed(self):
        """the same frame with every plane contiguous (what the context calls take: one set of strides for all frames of a call)"""
        if all(p.flags.c_contiguous for p in self.planes):
            return self
        return YuvFrame([np.ascontiguousarray(p) for p in self.planes], self.fmt)

    def _args(self):
        ptrs = [p.ctypes.data for p in self.planes] + [None] * (3 - len(self.planes))
        strides = [p.strides[0] for p in self.planes] + [0] * (3 - len(self.planes))
        return (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*strides)

    def to_device(self, pitched=False):
        """the planes as stages.Dev buffers"""
        from .stages import Dev
        return [Dev(np.ascontiguousarray(p), pitched=pitched) for p in self.planes]


def empty_frame(fmt, h, w):
    dt = np.uint16 if fmt.depth > 8 else np.uint8
    return YuvFrame([np.zeros((r, b // np.dtype(dt).itemsize), dt) for r, b in plane_dims(fmt, h, w)], fmt)


def to_rgb(frame):
    """(h, w, 3) uint8 of a YuvFrame (eppm_yuv_to_rgb_host): the bytes a context holds after the frame's set_data_yuv / push_frame_yuv"""
    rgb = np.empty((frame.h, frame.w, 3), np.uint8)
    planes, strides = frame._args()
    check(lib().eppm_yuv_to_rgb_host(C.byref(frame.fmt), planes, strides, rgb.ctypes.data, frame.w * 3, frame.h, frame.w), "eppm_yuv_to_rgb_host")
    return rgb


def from_rgb(rgb, fmt=None, **kw):
    """A YuvFrame of format fmt (default: the library's) from an (h, w, 3) uint8 image (eppm_yuv_from_rgb_host)"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise EppmError("from_rgb: the image must be (h, w, 3) uint8")
    h, w = rgb.shape[:2]
    out = empty_frame(YuvFormat(fmt, **kw), h, w)
    planes, strides = out._args()
    check(lib().eppm_yuv_from_rgb_host(C.byref(out.fmt), rgb.ctypes.data, w * 3, planes, strides, h, w), "eppm_yuv_from_rgb_host")
    return out


def _dev_args(planes):
    ptrs = [p.ptr for p in planes] + [None] * (3 - len(planes))
    pitches = [p.pitch for p in planes] + [0] * (3 - len(planes))
    return (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*pitches)


def to_rgba_device(fmt, planes, out=None, stream=None):
    """k_yuv_to_rgba alone (eppm_yuv_to_rgba): planes: the format's stages.Dev planes; out: a Dev of uchar4 words (made here if None)."""
    from .api import uchar4
    from .stages import Dev
    h, w = planes[0].h, planes[0].w
    out = Dev(shape=(h, w), dtype=uchar4, pitched=True) if out is None else out
    ptrs, pitches = _dev_args(planes)
    check(lib().eppm_yuv_to_rgba(C.byref(fmt), ptrs, pitches, out.ptr, out.pitch, h, w, stream), "eppm_yuv_to_rgba")
    return out


def from_rgba_device(fmt, rgba, planes=None, stream=None):
    """k_rgba_to_yuv alone (eppm_yuv_from_rgba): rgba: a Dev of uchar4 words; planes: the destination Devs (made here if None)."""
    from .stages import Dev
    h, w = rgba.h, rgba.w
    if planes is None:
        dt = np.uint16 if fmt.depth > 8 else np.uint8
        planes = [Dev(shape=(r, b // np.dtype(dt).itemsize), dtype=dt) for r, b in plane_dims(fmt, h, w)]
    ptrs, pitches = _dev_args(planes)
    check(lib().eppm_yuv_from_rgba(C.byref(fmt), rgba.ptr, rgba.pitch, ptrs, pitches, h, w, stream), "eppm_yuv_from_rgba")
    return planes


def frames_args(frames, what):
    """(format, 3n plane pointers, strides) of host frames for one context call: one format, one size, packed planes"""
    frames = [f.packed() for f in frames]
    f0 = frames[0]
    for f in frames[1:]:
        if not _same_format(f.fmt, f0.fmt) or (f.h, f.w) != (f0.h, f0.w):
            raise EppmError(f"{what}: all frames of a call must share one format and size")
    ptrs = []
    for f in frames:
        ptrs += list(f._args()[0])
    return f0.fmt, (C.c_void_p * len(ptrs))(*ptrs), f0._args()[1], frames


def device_args(frames, what):
    """the same for frames given as lists of stages.Dev planes"""
    p0 = [p.pitch for p in frames[0]]
    ptrs = []
    for planes in frames:
        if [p.pitch for p in planes] != p0:
            raise EppmError(f"{what}: all frames of a call must share their pitches")
        ptrs += list(_dev_args(planes)[0])
    return (C.c_void_p * len(ptrs))(*ptrs), _dev_args(frames[0])[1]


# ---- y4m files, restated in Python (the library's own reader and writer: native=True) ----
_C_TAGS = {"420jpeg": (8, CENTER), "420mpeg2": (8, LEFT), "420": (8, LEFT), "420p10": (10, LEFT), "420p12": (12, LEFT), "420p16": (16, LEFT)}


def _y4m_header(line, path, interlaced=False):
    if not re.fullmatch(rb"YUV4MPEG2( .*)?", line):
        raise EppmError(f"read_y4m: {path}: malformed: no YUV4MPEG2 header line")
    h = w = 0
    fps = (0, 0)
    fmt = YuvFormat(layout=I420)
    center = False
    mode = 0
    for tok in line.decode("ascii", "replace").split(" ")[1:]:
        if not tok:
            continue
        k, v = tok[0], tok[1:]
        if k in "WH":
            n = int(re.match(r"\d*", v).group() or 0)       # the leading digits, as the library reads them
            w, h = (n, h) if k == "W" else (w, n)
        elif k == "F":
            m = re.fullmatch(r"(\d+):(\d+)", v)
            fps = (min(int(m.group(1)), 2 ** 31 - 1), min(int(m.group(2)), 2 ** 31 - 1)) if m else (0, 0)       # as the library: an int each
        elif k == "I":
            if v[:1] == "m" or (not interlaced and v[:1] in ("t", "b")):
                raise EppmError(f"read_y4m: {path}: interlaced material ({tok}) is not supported")
            mode = {"t": 1, "b": 2}.get(v[:1], 0)
        elif k == "C":
            if v not in _C_TAGS:
                raise EppmError(f"read_y4m: {path}: colour space {tok} is not supported (4:2:0 {'only' if interlaced else 'progressive only'})")
            fmt.depth, fmt.siting = _C_TAGS[v]
        elif tok == "XCOLORRANGE=FULL":
            fmt.full_range = 1
        elif tok == "XCOLORRANGE=LIMITED":
            fmt.full_range = 0
        elif tok == "XEPPM_SITING=CENTER":
            center = True
    if h < 1 or w < 1:
        raise EppmError(f"read_y4m: {path}: malformed: missing W or H")
    if h > 65535 or w > 65535:
        raise EppmError(f"read_y4m: {path}: malformed: W or H beyond 65535")
    if mode and h % 4:
        raise EppmError(f"read_y4m: {path}: an interlaced 4:2:0 file needs H a multiple of 4 (H{h}): each field is a 4:2:0 picture")
    if center:
        fmt.siting = CENTER
    fmt.matrix = BT601 if h < 720 else BT709
    return h, w, fmt, fps, mode


class read_y4m:
    """Iterates over the frames of a y4m file as YuvFrames (I420); .h, .w, .fmt, .fps = (num, den).  matrix: BT601 / BT709 / BT2020 instead
    of the default by size (601 below 720 rows); native: through the library's reader (eppm_y4m_*) instead of this module's.
    interlaced=True: It / Ib files are accepted too (eppm_deint_y4m_open_read) and .interlace says what the file
    is: 0 progressive, 1 top field first, 2 bottom field first; the frames are whole, both fields woven (split_fields)."""

    def __init__(self, path, matrix=None, native=False, interlaced=False):
        self.path, self._y, self._f = str(path), None, None
        self.interlace = 0
        if native and interlaced:
            y, h, w, num, den, mode = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
            self.fmt = CYuvFormat()
            check(lib().eppm_deint_y4m_open_read(C.byref(y), self.path.encode(), C.byref(h), C.byref(w), C.byref(self.fmt), C.byref(num),
                                                 C.byref(den), C.byref(mode)), "eppm_deint_y4m_open_read")
            self._y, self.h, self.w, self.fps, self.interlace = y, h.value, w.value, (num.value, den.value), mode.value
        elif native:
            y, h, w, num, den = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
            self.fmt = CYuvFormat()
            check(lib().eppm_y4m_open_read(C.byref(y), self.path.encode(), C.byref(h), C.byref(w), C.byref(self.fmt), C.byref(num), C.byref(den)),
                  "eppm_y4m_open_read")
            self._y, self.h, self.w, self.fps = y, h.value, w.value, (num.value, den.value)
        else:
            self._f = open(self.path, "rb")
            line = self._f.readline(4096)
            if not line.endswith(b"\n"):
                self.close()
                raise EppmError(f"read_y4m: {self.path}: malformed: no YUV4MPEG2 header line")
            try:
                self.h, self.w, self.fmt, self.fps, self.interlace = _y4m_header(line[:-1], self.path, interlaced)
            except EppmError:
                self.close()
                raise
        if matrix is not None:
            self.fmt.matrix = matrix

    def __iter__(self):
        return self

    def __next__(self):
        if self._y is None and self._f is None:
            raise StopIteration
        frame = empty_frame(self.fmt, self.h, self.w)
        if self._y is not None:
            got = C.c_int()
            planes, strides = frame._args()
            check(lib().eppm_y4m_read_frame(self._y, planes, strides, C.byref(got)), "eppm_y4m_read_frame")
            if not got.value:
                self.close()
                raise StopIteration
            return frame
        line = self._f.readline(256)
        if not line:
            self.close()
            raise StopIteration
        if not re.fullmatch(rb"FRAME( .*)?\n", line):
            self.close()
            raise EppmError(f"read_y4m: {self.path}: malformed: missing FRAME line")
        for p in frame.planes:
            raw = self._f.read(p.nbytes)
            if len(raw) != p.nbytes:
                self.close()
                raise EppmError(f"read_y4m: {self.path}: malformed: truncated frame")
            p[...] = np.frombuffer(raw, p.dtype).reshape(p.shape)
        return frame

    def close(self):
        if self._y is not None:
            lib().eppm_y4m_close(self._y)
            self._y = None
        if self._f is not None:
            self._f.close()
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_fields(frame):
    """The two fields (top, bottom) of an interlaced 4:2:0 frame as YuvFrames of the frame's format: field p is the luma rows p::2 and the
    chroma rows p::2.  The frame needs h % 4 == 0, so that each field is itself a 4:2:0 picture.  A field's chroma sits a quarter line
    off the siting the format names; that is not corrected."""
    if frame.h % 4:
        raise EppmError(f"split_fields: an interlaced 4:2:0 frame needs h a multiple of 4, not {frame.h}")
    return tuple(YuvFrame([np.ascontiguousarray(p[par::2]) for p in frame.planes], frame.fmt) for par in (0, 1))


def _y4m_tags(fmt):
    if fmt.layout != I420 or fmt.msb_aligned:
        raise EppmError("write_y4m: a y4m file holds I420 planes of low-aligned words")
    if fmt.depth == 8:
        tag = "C420jpeg" if fmt.siting == CENTER else "C420mpeg2"
    else:
        tag = f"C420p{fmt.depth}" + (" XEPPM_SITING=CENTER" if fmt.siting == CENTER else "")
    return tag + " XCOLORRANGE=" + ("FULL" if fmt.full_range else "LIMITED")


def write_y4m(path, frames, fps=(25, 1), native=False):
    """Write YuvFrames (I420, one format and size) as a y4m file at fps = (num, den); returns the number of frames written.  The matrix is
    not stored: a reader assumes it from the size."""
    num, den = int(fps[0]), int(fps[1])
    n, first, y, f = 0, None, None, None
    try:
        for fr in frames:
            if first is None:
                first = fr
                if native:
                    y = C.c_void_p()
                    check(lib().eppm_y4m_open_write(C.byref(y), str(path).encode(), fr.h, fr.w, C.byref(fr.fmt), num, den), "eppm_y4m_open_write")
                else:
                    tags = _y4m_tags(fr.fmt)
                    if num < 1 or den < 1:
                        raise EppmError(f"write_y4m: bad rate {num}:{den}")
                    f = open(str(path), "wb")
                    f.write(f"YUV4MPEG2 W{fr.w} H{fr.h} F{num}:{den} Ip A1:1 {tags}\n".encode())
            elif not _same_format(fr.fmt, first.fmt) or (fr.h, fr.w) != (first.h, first.w):
                raise EppmError("write_y4m: all frames must share one format and size")
            if native:
                planes, strides = fr._args()
                check(lib().eppm_y4m_write_frame(y, planes, strides), "eppm_y4m_write_frame")
            else:
                f.write(b"FRAME\n")
                for p in fr.planes:
                    f.write(np.ascontiguousarray(p).tobytes())
            n += 1
    finally:
        if y is not None:
            check(lib().eppm_y4m_close(y), "eppm_y4m_close")
        if f is not None:
            f.close()
    if first is None:
        raise EppmError("write_y4m: no frame")
    return n
