#!/usr/bin/env python3
"""Recorded outputs of the reference's own host code (oracle/_ref/libeppm_refio.so: its .flo / PPM I/O, flow tools and Middlebury colour
coding) on the inputs of the CPU tests that compare this library with it (tests/test_abi_cpu.py, tests/test_oracle_cpu.py), so that those
tests run where the reference sources are absent.  Where oracle/_ref was built the tests check the live code too.  Run once where it
was built (a second of CPU):

    python tests/golden/make_golden_refio.py

Writes tests/golden/refio_recorded.npz.  The inputs below must stay exactly those of the tests.
"""
import ctypes as C
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(HERE, "refio_recorded.npz")

# the cases of the tests (tests/test_abi_cpu.py, tests/test_oracle_cpu.py)
BORDERS = (0, 1, 5, 18, 30)
THRESHOLDS = (0, 1, 3, 10)
CUTOFFS = ((4, False), (4, True), (-7, False), (0, True), (1000, False))
COLOUR_CASES = ((1, 6.0), (2, 0.01), (3, 300.0))
PYR_SIZES = ((436, 1024), (480, 640), (1080, 1920), (2160, 3840), (437, 1023), (101, 77))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def flo_fields():
    rng = np.random.default_rng(1)
    u = (rng.standard_normal((20, 31)) * 30).astype(np.float32); v = (rng.standard_normal((20, 31)) * 30).astype(np.float32)
    u[3, 4] = v[3, 4] = 1e10
    return u, v


def epe_fields():
    rng = np.random.default_rng(2)
    shp = (24, 40)
    u, v, gu, gv = [(rng.standard_normal(shp) * 5).astype(np.float32) for _ in range(4)]
    gu[0, :5] = 0; gv[0, :5] = 0
    gu[1, 1] = 1e10
    return u, v, gu, gv


def flow_fields(seed, shp=(37, 53)):
    rng = np.random.default_rng(seed)
    u, v, gu, gv = [(rng.standard_normal(shp) * 6).astype(np.float32) for _ in range(4)]
    gu[0, :5] = 0; gv[0, :5] = 0
    gu[3, 7] = 1e10; gv[5, 9] = -1e10
    gu[8, 8] = 1e10; gv[8, 8] = 1e10
    u[10, 10] = 1e10; v[11, 11] = 2e9
    return u, v, gu, gv


def colour_fields(seed, scale):
    rng = np.random.default_rng(seed)
    h, w = 61, 83
    u = (rng.standard_normal((h, w)) * scale).astype(np.float32)
    v = (rng.standard_normal((h, w)) * scale).astype(np.float32)
    u[0, :] = 0; v[0, :] = np.linspace(-scale, scale, w, dtype=np.float32)
    v[1, :] = 0; u[1, :] = np.linspace(-scale, scale, w, dtype=np.float32)
    u[2, 2] = v[2, 2] = 0
    u[5, 5] = 1e10; v[6, 6] = -3e9
    return u, v


def compute_color_fields():
    """The normalised vectors test_flow_color_close_to_middlebury_cpu_routine hands computeColor."""
    rng = np.random.default_rng(3)
    n = 20000
    fx = (rng.standard_normal(n) * 0.7).astype(np.float32)
    fy = (rng.standard_normal(n) * 0.7).astype(np.float32)
    mr = np.float32(np.sqrt(np.float32(800.0)))
    return ((fx * mr) / mr).astype(np.float32), ((fy * mr) / mr).astype(np.float32)


def main():
    R = O.refio()
    if R is None:
        sys.exit("oracle/_ref/libeppm_refio.so is not built (it needs the reference sources)")
    rec = {}
    u, v = flo_fields()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "r.flo")
        R.refio_save_flo(path.encode(), _p(u), _p(v), 20, 31)
        rec["flo_writer_bytes"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    img = np.zeros((480, 640, 3), np.uint8)
    assert R.refio_load_ppm(os.path.join(HERE, "frame10.ppm").encode(), _p(img), 480, 640) == 3
    rec["ppm_frame10_sha256"] = np.array(hashlib.sha256(img.tobytes()).hexdigest())
    epe, aae = C.c_float(), C.c_float()
    R.refio_flow_error(*[_p(a) for a in epe_fields()], 24, 40, C.byref(epe), C.byref(aae))
    rec["flow_error"] = np.array([epe.value, aae.value], np.float32)
    u, v, gu, gv = flow_fields(11)
    for b in BORDERS:
        epe, aae = C.c_float(0), C.c_float(0)
        R.refio_flow_error_border(_p(u), _p(v), _p(gu), _p(gv), 37, 53, b, C.byref(epe), C.byref(aae))
        rec[f"flow_error_border_{b}"] = np.array([epe.value, aae.value], np.float32)
    R.refio_flow_error_percentage.restype = C.c_float
    u, v, gu, gv = flow_fields(12)
    for t in THRESHOLDS:
        m = np.full((37, 53), 7, np.uint8)
        rec[f"flow_error_percentage_{t}"] = np.array(R.refio_flow_error_percentage(_p(u), _p(v), _p(gu), _p(gv), 37, 53, t, _p(m)), np.float32)
        rec[f"flow_error_percentage_map_{t}"] = m
    u, v, _, _ = flow_fields(13)
    for cut, inval in CUTOFFS:
        wu, wv = np.empty_like(u), np.empty_like(v)
        R.refio_flow_cutoff(_p(wu), _p(wv), _p(u), _p(v), 37, 53, cut, int(inval))
        rec[f"flow_cutoff_{cut}_{int(inval)}"] = np.stack([wu, wv])
    for seed, scale in COLOUR_CASES:
        u, v = colour_fields(seed, scale)
        rgb = np.empty((61, 83, 3), np.uint8)
        R.refio_flow_to_color(_p(rgb), _p(u), _p(v), 61, 83)
        rec[f"flow_to_color_{seed}"] = rgb
    nx, ny = compute_color_fields()
    pix = (C.c_ubyte * 3)()
    bgr = np.zeros((len(nx), 3), np.uint8)
    for i in range(len(nx)):
        R.refio_compute_color(C.c_float(float(nx[i])), C.c_float(float(ny[i])), pix)
        bgr[i] = (pix[0], pix[1], pix[2])
    rec["compute_color_bgr"] = bgr
    dims = []
    for h, w in PYR_SIZES:
        ah, aw = (C.c_int * 8)(), (C.c_int * 8)()
        n = R.refio_pyr_init_dim(ah, aw, h, w, 3, C.c_float(0.5))
        dims.append([n] + [ah[i] for i in range(8)] + [aw[i] for i in range(8)])
    rec["pyr_init_dim"] = np.array(dims, np.int32)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(rec)} arrays)")


if __name__ == "__main__":
    main()
