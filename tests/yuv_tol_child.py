"""Child process of tests/test_yuv_gpu.py, and the home of what both share: kernel_mismatches() runs k_yuv_to_rgba and k_rgba_to_yuv alone on
caller planes (eppm_yuv_to_rgba / eppm_yuv_from_rgba) and compares every byte of every destination, padding included, with the host forms.
As a program it selects the tolerance library (the pytest process holds the exact test library) and runs a spread of formats at every
size: the conversion has no EPPM_TOL branch, so the result is the same.  Prints the library's version first and "PART OK" last."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))

# 4k, 4k + 1, 4k + 2, 4k + 3 wide; odd heights; more than one block each way (a block covers 256 x 4 pixels to RGBA, 512 x 8 from it)
KERNEL_SIZES = [(4, 4), (5, 7), (45, 67), (96, 128), (6, 13), (6, 14), (6, 15), (9, 517)]
POISON = 0xA5


class Arena:
    """one device allocation, handed out in 256-byte aligned pieces and reused by every case"""

    def __init__(self, nbytes=8 << 20):
        from eppm_amd._lib import check, lib
        self.base, self.size, self.used = C.c_void_p(), nbytes, 0
        check(lib().eppm_malloc_device(C.byref(self.base), C.c_size_t(nbytes)), "malloc")

    def reset(self):
        self.used = 0

    def take(self, nbytes):
        at = (self.used + 255) & ~255
        assert at + nbytes <= self.size
        self.used = at + nbytes
        return self.base.value + at

    def free(self):
        from eppm_amd._lib import lib
        lib().eppm_free_device(self.base)


class Plane:
    """a 2-D host array, padding columns included, and its device copy `offset` bytes past a 256-byte boundary; cols: the columns in use"""

    def __init__(self, arena, full, cols, offset=0):
        from eppm_amd._lib import check, lib
        self.full, self.cols = np.ascontiguousarray(full), cols
        self.ptr = arena.take(self.full.nbytes + offset) + offset
        self.pitch = self.full.strides[0]
        check(lib().eppm_memcpy_h2d(self.ptr, self.full.ctypes.data, self.full.nbytes), "h2d")

    def get(self):
        from eppm_amd._lib import check, lib
        out = np.empty_like(self.full)
        check(lib().eppm_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "d2h")
        return out


def _args(planes):
    ptrs = [p.ptr for p in planes] + [None] * (3 - len(planes))
    return (C.c_void_p * 3)(*ptrs), (C.c_size_t * 3)(*([p.pitch for p in planes] + [0] * (3 - len(planes))))


def rgba_words(rgb):
    p = rgb.astype(np.uint32)
    return p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)


def to_rgba_case(arena, f, h, w, rng):
    """-> [what differs] over three destinations: 16-byte aligned base and pitch, pitch 4w + 4, and pitch 4w + 4 at a base 4 bytes off"""
    from eppm_amd import yuv
    from eppm_amd._lib import check, lib
    from test_yuv_cpu import plane_shapes
    dt = np.uint16 if f.depth > 8 else np.uint8
    arena.reset()
    src = [Plane(arena, rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), (r, c + 5), dtype=np.int64).astype(dt), c) for r, c in plane_shapes(f, h, w)]
    want = rgba_words(yuv.to_rgb(yuv.YuvFrame([p.full[:, :p.cols] for p in src], f)))
    bad = []
    for name, words, offset in (("aligned", (w + 3) // 4 * 4 + 4, 0), ("pitch 4w+4", w + 1, 0), ("pitch 4w+4, base+4", w + 1, 4)):
        dst = Plane(arena, np.full((h, words), 0xDEADBEEF, np.uint32), w, offset)
        ptrs, pitches = _args(src)
        check(lib().eppm_yuv_to_rgba(C.byref(f), ptrs, pitches, dst.ptr, dst.pitch, h, w, None), "eppm_yuv_to_rgba")
        check(lib().eppm_device_synchronize(), "sync")
        expect = dst.full.copy()
        expect[:, :w] = want
        got = dst.get()
        if not np.array_equal(got, expect):
            bad.append((f.as_dict(), h, w, "to_rgba " + name, int((got != expect).sum())))
    return bad


def from_rgba_case(arena, f, h, w, rng):
    """-> [what differs] over two sets of destination planes: bases and pitches multiples of 4 (the word stores), and neither"""
    from eppm_amd import yuv
    from eppm_amd._lib import check, lib
    from test_yuv_cpu import plane_shapes
    dt = np.dtype(np.uint16 if f.depth > 8 else np.uint8)
    arena.reset()
    src = Plane(arena, rng.integers(0, 1 << 32, (h, w + 3), dtype=np.int64).astype(np.uint32), w)       # alpha and padding: junk
    rgb = np.stack([(src.full[:, :w] >> s) & 255 for s in (0, 8, 16)], -1).astype(np.uint8)
    want = yuv.from_rgb(rgb, f).planes
    bad = []
    for name, aligned in (("aligned", True), ("unaligned", False)):
        dst = []
        for r, c in plane_shapes(f, h, w):
            cols = c + 4
            while (cols * dt.itemsize % 4 == 0) != aligned:
                cols += 1
            dst.append(Plane(arena, np.full((r, cols), POISON, dt), c, 0 if aligned else dt.itemsize))
        ptrs, pitches = _args(dst)
        check(lib().eppm_yuv_from_rgba(C.byref(f), src.ptr, src.pitch, ptrs, pitches, h, w, None), "eppm_yuv_from_rgba")
        check(lib().eppm_device_synchronize(), "sync")
        for k, (p, wnt) in enumerate(zip(dst, want)):
            expect = p.full.copy()
            expect[:, :p.cols] = wnt
            got = p.get()
            if not np.array_equal(got, expect):
                bad.append((f.as_dict(), h, w, f"from_rgba {name} plane {k}", int((got != expect).sum())))
    return bad


def kernel_mismatches(fmts, sizes=KERNEL_SIZES, seed=0):
    arena = Arena()
    rng = np.random.default_rng(seed)
    bad = []
    try:
        for f in fmts:
            for h, w in sizes:
                bad += to_rgba_case(arena, f, h, w, rng)
                bad += from_rgba_case(arena, f, h, w, rng)
    finally:
        arena.free()
    return bad


def main():
    import conftest  # noqa: F401             (selects the test library: overridden below, before anything is loaded)
    import eppm_amd
    eppm_amd.select_library("tol")
    from test_yuv_cpu import formats          # (its parametrised tests make formats, which loads the library, when it is imported)
    print(eppm_amd.lib().eppm_version().decode())
    fmts = list(formats(matrices=(1,), ranges=(0,)))         # every layout, depth form and siting: the kernels' template arguments
    bad = kernel_mismatches(fmts)
    print(f"{len(fmts)} formats x {len(KERNEL_SIZES)} sizes, {len(bad)} destinations differ from the host forms: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
