"""CPU tests of the oracle: committed golden vectors, hand-checkable known-answer tests,
and the pieces of the reference that DO compile here (oracle/_ref: its host-side helpers)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O


def eq(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert a.tobytes() == b.tobytes(), f"{what}: planes differ"


# ---------------------------------------------------------------- golden vectors
def test_golden_whole_path_crop(crop_stages):
    g = np.load(os.path.join(GOLDEN, "crop160_stages.npz"))
    for k in g.files:
        eq(crop_stages[k], g[k], k)


def test_golden_patchmatch_iterations(crop_stages):
    st = crop_stages
    g = np.load(os.path.join(GOLDEN, "pm_iters.npz"))
    for it in (0, 1):
        nnf, cost = O.patchmatch(st["img1_L2"], st["img2_L2"], st["cen1_L2"], st["cen2_L2"], iters_done=it)
        eq(nnf, g[f"nnf_it{it}"], f"nnf after {it} iterations")
        eq(cost, g[f"cost_it{it}"], f"cost after {it} iterations")
    eq(st["nnf1_pm"], g["nnf_it10"], "nnf after 10 iterations")


def test_golden_xorwow():
    g = json.load(open(os.path.join(GOLDEN, "xorwow.json")))
    for sub, vals in g.items():
        assert [int(x) for x in O.xorwow_stream(1234, int(sub), 8)] == vals


def test_fixture_frames_are_the_bundled_pair(frames):
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    import hashlib
    for n in ("frame10.ppm", "frame11.ppm"):
        assert hashlib.sha256(open(os.path.join(GOLDEN, n), "rb").read()).hexdigest() == man[n]
    assert frames[0].shape == (480, 640, 3)        # 640x480, not 584x388


# ---------------------------------------------------------------- arithmetic
def test_fast_exp_accuracy_and_anchors():
    x = -np.linspace(0, 86, 50001).astype(np.float32)
    y = O.fast_exp(x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    # CUDA documents __expf's error as 2 + floor(|1.16 x|) ulp (the x*log2e product is rounded to float)
    bound = (2 + np.floor(1.16 * np.abs(x.astype(np.float64)))) * 2.0 ** -23
    assert (np.abs(y / ref - 1) <= bound).all()
    assert np.max(np.abs(y / ref - 1)[x > -1]) < 4e-7
    assert O.fast_exp([0.0])[0] == 1.0
    # no flush (the reference is built without -ftz): gradual underflow, correctly rounded scaling
    sub = -np.linspace(87.5, 103.5, 4001).astype(np.float32)
    ys = O.fast_exp(sub).astype(np.float64)
    assert (ys > 0).all() and (ys < 2.0 ** -126).all()
    assert (np.abs(ys - np.exp(sub.astype(np.float64)) * (ys / ys)) <= 2.0 ** -149 * 0.5 + np.exp(sub.astype(np.float64)) * 1.3e-5).all()
    assert O.fast_exp([-100.0])[0] == np.float32(2.0 ** -149 * 27)      # exp(-100) = 26.5 * 2^-149 -> 27 subnormal steps
    assert O.fast_exp([-104.5])[0] == 0.0 and O.fast_exp([-4000.0])[0] == 0.0


def test_luts_follow_the_reference_formulas():
    gs, cn = O.pm_luts(9)
    f = np.float32
    assert np.allclose(gs, [np.exp(-(i * i) / 20.25) for i in range(10)], rtol=2e-7)
    assert np.allclose(cn, [1 - np.exp(-(k * k) / 5.76) for k in range(9)], rtol=0, atol=2e-7)
    assert gs[0] == f(1) and cn[0] == f(0)
    assert np.allclose(O.wmf_lut(), [np.exp(-(i * i) / 16.0) for i in range(5)], rtol=2e-7)
    assert np.allclose(O.blf_lut(), [np.exp(-(i * i) / 25.0) for i in range(11)], rtol=2e-7)


def test_divconst_exhaustive_c_program(tmp_path):
    exe = str(tmp_path / "verify_divconst")
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "csrc", "verify_divconst.c"),
                           "-o", exe, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


# ---------------------------------------------------------------- hand-checkable KATs
def _const_img(h, w, val):
    a = np.zeros((h, w), O.uchar4)
    a["x"] = a["y"] = a["z"] = val
    return a


def test_patch_cost_of_identical_constant_images_is_zero():
    img = _const_img(40, 40, 77)
    cen = np.zeros((40, 40), np.uint8)
    for planefit in (False, True):
        assert O.patch_dist(img, img, cen, cen, 20, 20, 22, 19, planefit=planefit) == 0.0


def test_patch_cost_black_vs_white():
    a, b = _const_img(40, 40, 0), _const_img(40, 40, 255)
    cen = np.zeros((40, 40), np.uint8)
    # d = 1 -> 1 - exp(-100) = 1 (flushed); census equal -> +0; all weights equal -> exactly 1
    assert O.patch_dist(a, b, cen, cen, 20, 20, 20, 20) == 1.0
    # census all-ones vs zero: Hamming 8 -> + cn[8]
    cen8 = np.full((40, 40), 255, np.uint8)
    gs, cn = O.pm_luts(9)
    assert O.patch_dist(a, a, cen, cen8, 20, 20, 20, 20) == cn[8]


def test_patch_cost_clamps_out_of_range_targets():
    rng = np.random.default_rng(0)
    a = np.zeros((30, 30), O.uchar4); b = np.zeros((30, 30), O.uchar4)
    for ch in "xyz":
        a[ch] = rng.integers(0, 256, (30, 30)); b[ch] = rng.integers(0, 256, (30, 30))
    c1 = rng.integers(0, 256, (30, 30)).astype(np.uint8); c2 = rng.integers(0, 256, (30, 30)).astype(np.uint8)
    # target (30,30) is one past the image (random init draws x in [0,w], y in [0,h]); clamp addressing makes
    # it differ from (29,29) only through the patch offsets, never crash
    v = O.patch_dist(a, b, c1, c2, 0, 0, 30, 30)
    assert np.isfinite(v) and 0 <= v <= 2


def test_census_of_a_ramp():
    img = np.zeros((3, 3), O.uchar4)
    ramp = np.arange(9).reshape(3, 3) * 10
    img["x"] = img["y"] = img["z"] = ramp
    c = O.census(img)
    # centre pixel (1,1)=40: neighbours larger are (2,1)=50 bit4, (0,2)=60 bit5, (1,2)=70 bit6, (2,2)=80 bit7
    assert c[1, 1] == (1 << 4) | (1 << 5) | (1 << 6) | (1 << 7)
    # corner (0,0)=0 with clamp addressing: bits 2 (x+1,y-1 -> (1,0)=10), 4 (1,0), 5 (x-1,y+1 -> (0,1)=30), 6, 7
    assert c[0, 0] == (1 << 2) | (1 << 4) | (1 << 5) | (1 << 6) | (1 << 7)
    assert c[2, 2] == 0


def test_pyramid_dims_and_decimation_maps():
    assert O.pyr_init_dim(436, 1024) == ([436, 218, 109], [1024, 512, 256])
    assert O.pyr_init_dim(480, 640) == ([480, 240, 120], [640, 320, 160])
    assert O.pyr_init_dim(437, 1023) == ([437, 218, 109], [1023, 511, 255])
    img = np.zeros((16, 24), O.uchar4)
    img["x"] = np.arange(24)[None, :]; img["y"] = np.arange(16)[:, None]
    half = O.resize_rgba(img, 8, 12, 0.5)
    assert (half["x"] == (2 * np.arange(12) + 1)[None, :]).all() and (half["y"] == (2 * np.arange(8) + 1)[:, None]).all()
    quarter = O.resize_rgba(img, 4, 6, 0.25)
    assert (quarter["x"] == (4 * np.arange(6) + 3)[None, :]).all() and (quarter["y"] == (4 * np.arange(4) + 3)[:, None]).all()


def test_pyramid_level2_is_built_from_level1():
    """.cuh:649 `int n=log(0.25)/log(ratio)` evaluates to 1 in C++ (float log overload), so level 2 is
    decimate(blur_1(level 1)), not decimate_4(blur_2(level 0))."""
    rng = np.random.default_rng(3)
    raw = np.zeros((48, 64), O.uchar4)
    for ch in "xyz":
        raw[ch] = rng.integers(0, 256, (48, 64))
    imgs, _ = O.prepare(raw)
    l0 = O.gauss_filter_rgba(raw, 0.5, 2)
    l1 = O.resize_rgba(O.gauss_filter_rgba(l0, 1.0, 3), 24, 32, 0.5)
    l2 = O.resize_rgba(O.gauss_filter_rgba(l1, 1.0, 3), 12, 16, 0.5)
    eq(imgs[0], l0, "L0"); eq(imgs[1], l1, "L1"); eq(imgs[2], l2, "L2")


def test_flow_upsample_and_unknown_handling():
    f = np.zeros((2, 2), O.float2)
    f["x"] = [[1, 3], [5, 7]]
    up = O.resize_flow(f, 4, 4, 2.0)
    # fx = (x+1)/2 - 1 -> -0.5, 0, 0.5, 1: pixel 0, pixel 0, mean, pixel 1
    assert list(up["x"][0]) == [1, 1, 2, 3]
    assert list(up["x"][:, 0]) == [1, 1, 3, 5]
    nnf = np.zeros((1, 3), O.short2)
    nnf["x"] = [5, -10000, -9990]; nnf["y"] = [0, -10000, 0]
    fl = O.nnf2flow(nnf)
    assert fl["x"][0, 0] == 5 and fl["x"][0, 1] == np.float32(1e10) and fl["x"][0, 2] == -9992


def test_left_right_check_and_outlier_rules():
    w = h = 8
    yy, xx = np.mgrid[0:h, 0:w]
    n1 = np.zeros((h, w), O.short2); n2 = np.zeros((h, w), O.short2)
    n1["x"], n1["y"] = xx, yy              # identity both ways: everything consistent
    n2["x"], n2["y"] = xx, yy
    n1["x"][0, 0] = 8                      # target outside [0,w) -> invalid
    n1["x"][3, 3], n1["y"][3, 3] = 4, 3    # points at (4,3) whose backward match is (4,3) != (3,3) -> invalid
    c = np.ones((h, w), np.float32)
    a, ca, b, cb = O.left_right_check(n1, c, n2, c)
    bad = (a["x"] == -10000)
    assert bad[0, 0] and bad[3, 3] and bad.sum() == 2
    assert ca[0, 0] == np.finfo(np.float32).max
    # second launch sees the marks: nnf2[0,0] -> nnf1[0,0] is invalid now
    assert b["x"][0, 0] == -10000 and b["x"][3, 3] == -10000
    # outlier: 8x8 image, every pixel has < 84 neighbours in its clipped 13x13 window except none -> all invalid
    o, _ = O.outlier_removal(a, ca)
    assert (o["x"] == -10000).all()


# ---------------------------------------------------------------- XORWOW
def test_xorwow_skip_matrix_equals_stepping():
    full = O.xorwow_stream(1234, 5, 700)
    for k in (1, 48, 510, 643):
        assert (O.xorwow_stream(1234, 5, 700 - k, skip=k) == full[k:]).all()


def test_xorwow_marsaglia_recurrence():
    """The state update is Marsaglia's xorwow (JSS 8(14), p.5): checked against an independent numpy restatement."""
    st = O.xorwow_state(1234, 3)
    v = [int(x) for x in st[:5]]; d = int(st[5])
    out = []
    M = 0xFFFFFFFF
    for _ in range(16):
        t = v[0] ^ (v[0] >> 2)
        v = v[1:] + [((v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))) & M]
        d = (d + 362437) & M
        out.append((v[4] + d) & M)
    assert [int(x) for x in O.xorwow_stream(1234, 3, 16)] == out


# ---------------------------------------------------------------- the reference's own host code (oracle/_ref)
# what it returns, recorded where oracle/_ref was built (tests/golden/make_golden_refio.py); checked live too where it exists
def _refio_recorded():
    return np.load(os.path.join(GOLDEN, "refio_recorded.npz"))


def test_pyr_dims_match_reference_code():
    R = O.refio()
    rec = _refio_recorded()["pyr_init_dim"]
    for k, (h, w) in enumerate([(436, 1024), (480, 640), (1080, 1920), (2160, 3840), (437, 1023), (101, 77)]):
        n = int(rec[k][0])
        assert (rec[k][1:1 + n].tolist(), rec[k][9:9 + n].tolist()) == O.pyr_init_dim(h, w)
        if R is not None:
            ah, aw = (C.c_int * 8)(), (C.c_int * 8)()
            n = R.refio_pyr_init_dim(ah, aw, h, w, 3, C.c_float(0.5))
            assert (list(ah)[:n], list(aw)[:n]) == O.pyr_init_dim(h, w)


def test_oracle_under_address_and_ub_sanitizers(tmp_path):
    """Whole oracle path (all three propagation modes) under ASan + UBSan on the CPU."""
    exe = str(tmp_path / "orc_san")
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                           "-mavx2", "-mfma", "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "csrc", "oracle_sanitize_driver.c"),
                           os.path.join(ROOT, "oracle", "eppm_oracle.c"), "-o", exe, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok")


def test_parallel_propagate_rule():
    """d_neighbor_propagate (kernel.cu:720-787): the four neighbours' matches are tried unshifted in the order
    upper, lower, left, right with strict <; outside the image the neighbour is the clamped border pixel; Jacobi."""
    rng = np.random.default_rng(5)
    h, w = 12, 14
    rgb1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb2 = np.roll(rgb1, 1, axis=1)
    i1, i2 = O.rgb2rgba(rgb1), O.rgb2rgba(rgb2)
    c1, c2 = O.census(i1), O.census(i2)
    nnf = np.zeros((h, w, 2), np.int16)
    nnf[..., 0] = rng.integers(0, w + 1, (h, w)); nnf[..., 1] = rng.integers(0, h + 1, (h, w))
    cost = O.cost_field(nnf, i1, i2, c1, c2)
    oc, on = O.parallel_propagate(cost, nnf, i1, i2, c1, c2)
    for y in range(h):
        for x in range(w):
            best, bc = nnf[y, x].copy(), cost[y, x]
            for ny, nx in ((max(y - 1, 0), x), (min(y + 1, h - 1), x), (y, max(x - 1, 0)), (y, min(x + 1, w - 1))):
                d = nnf[ny, nx]
                cv = O.patch_dist(i1, i2, c1, c2, x, y, int(d[0]), int(d[1]))
                if cv < bc:
                    best, bc = d.copy(), cv
            assert (on[y, x] == best).all() and oc[y, x] == bc, (x, y)
    assert (oc <= cost).all()


def test_planefit_offsets():
    """The affine passes of the plane-fitting cost (kernel.cu:334-513) sample image 2 at
    floor(((x+j + uu) + j*A) + i*B) in float.  x+j+uu is an integer M; the HIP refine kernel (c2f_device.cuh, c2f_pass)
    relies on floor(...) == M + floor(fl(fl(j*A) + fl(i*B))) for every M an image can produce, and on the y offset
    taking at most two consecutive values along a sample row.  Exhaustive over M for both instantiated radii."""
    f = np.float32
    kc = [(0.177, -0.011, -0.003, 0.301), (0.125, -0.357, 0.009, 0.308), (0.205, 0.370, 0.011, 0.296)]
    for R in (9, 17):
        M = np.arange(-R, 32764, dtype=np.float32)      # the launcher requires w + R < 32764, h + R < 32764
        for (A, B, C, D) in kc:
            for a, b in ((A, B), (C, D)):
                for i in range(-R, R + 1, 2):
                    row = []
                    for j in range(-R, R + 1, 2):
                        ja, ib = f(j) * f(a), f(i) * f(b)
                        t = ((M + ja).astype(np.float32) + ib).astype(np.float32)
                        off = int(np.floor(f(ja + ib)))
                        assert np.array_equal(np.floor(t), M + f(off)), (R, a, b, i, j)
                        row.append(off)
                    if (a, b) == (C, D):
                        assert max(row) - min(row) <= 1, (R, i, row)


# ---------------------------------------------------------------- XORWOW pins
def test_xorwow_transition_and_2pow67_jump_equal_rocrand_matrices(tmp_path):
    """The oracle's GF(2) transition and subsequence jump against an independent implementation shipped in the ROCm image."""
    hdr = "/opt/rocm/include/rocrand/rocrand_xorwow_precomputed.h"
    if not os.path.exists(hdr):
        pytest.skip("rocRAND headers not installed")
    O.lib()
    so = os.path.join(ROOT, "oracle", "_build", "libeppm_oracle.so")
    exe = str(tmp_path / "xpin")
    subprocess.check_call(["g++", "-O2", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "csrc", "xorwow_rocrand_pin.cpp"), so,
                           f"-Wl,-rpath,{os.path.dirname(so)}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout


def test_xorwow_curand_seeding_kat():
    """curand_init's seed scrambling, from the constants file (restated from curand_kernel.h; see its _about)."""
    import json
    k = json.load(open(os.path.join(GOLDEN, "xorwow_curand_kat.json")))
    M = 0xFFFFFFFF
    for seed in (1234, 0, 0x0123456789abcdef):
        s0 = (seed & M) ^ int(k["seed_xor_lo"], 16)
        s1 = (seed >> 32) ^ int(k["seed_xor_hi"], 16)
        t0, t1 = (k["mul_lo"] * s0) & M, (k["mul_hi"] * s1) & M
        v = k["v_init"]
        want = [(v[0] + t0) & M, v[1] ^ t0, (v[2] + t1) & M, v[3] ^ t1, (v[4] + t0) & M, (k["d_init"] + t1 + t0) & M]
        assert [int(x) for x in O.xorwow_state(seed, 0)] == want


# ---------------------------------------------------------------- flow colour coding (next: n4)
def _flow2(u, v):
    f = np.zeros(np.shape(u), O.float2)
    f["x"], f["y"] = u, v
    return f


def test_flow_color_kats():
    """basic/bao_basic_cuda.cuh:776-845: zero flow is white, an unknown / huge vector is black, a vector of the maximum
    radius pointing right is the first wheel colour (pure red), beyond the radius colours are darkened by .75."""
    mr = np.sqrt(np.float32(800.0))                    # sqrt(20^2 + 20^2), the driver's call (:311)
    u = np.array([[0, 1e10, 999999, -999999, mr, 2 * mr, 999998.0]], np.float32)
    v = np.zeros_like(u)
    c = O.flow_to_color(_flow2(u, v), 20, 20)
    rgb = np.stack([c["x"], c["y"], c["z"]], -1)[0]
    assert (rgb[0] == 255).all()                       # rad 0: col = 1 - 0*(1-col) = 1
    assert (rgb[1] == 0).all() and (rgb[2] == 0).all() and (rgb[3] == 0).all()     # |f| >= 999999 is not drawn (:825)
    assert tuple(rgb[4]) == (255, 0, 0)                # rad 1, angle -pi: wheel[0] = (255,0,0)
    assert tuple(rgb[5]) == (191, 0, 0)                # rad 2 > 1: (int)(255.0 * (1 * .75)) = 191
    assert rgb[6][0] == 191                            # 999998 < 999999 is drawn
    assert (c["w"] == 0).all()


def test_flow_color_close_to_middlebury_cpu_routine():
    """The device routine is a port of Middlebury's computeColor (colorcode.cpp:61-85), differing in pi (3.14159f vs M_PI):
    on random vectors the oracle's restatement equals it except for rare one-level differences."""
    R = O.refio()
    import ctypes as C
    rng = np.random.default_rng(3)
    n = 20000
    fx = (rng.standard_normal(n) * 0.7).astype(np.float32)
    fy = (rng.standard_normal(n) * 0.7).astype(np.float32)
    mr = float(np.sqrt(np.float32(800.0)))
    c = O.flow_to_color(_flow2((fx * np.float32(mr)).reshape(1, n), (fy * np.float32(mr)).reshape(1, n)), 20, 20)
    ours = np.stack([c["x"], c["y"], c["z"]], -1)[0].astype(int)
    bgr = _refio_recorded()["compute_color_bgr"]
    ref = bgr[:, ::-1].astype(int)                     # Middlebury writes B,G,R
    if R is not None:
        live = np.zeros((n, 3), int)
        pix = (C.c_ubyte * 3)()
        nx = ((fx * np.float32(mr)) / np.float32(mr)).astype(np.float32)      # what the kernel divides back to
        ny = ((fy * np.float32(mr)) / np.float32(mr)).astype(np.float32)
        for i in range(n):
            R.refio_compute_color(C.c_float(float(nx[i])), C.c_float(float(ny[i])), pix)
            live[i] = (pix[2], pix[1], pix[0])
        assert np.array_equal(live, ref)
    d = np.abs(ours - ref)
    assert d.max() <= 1, d.max()
    assert (d.max(axis=1) == 0).mean() > 0.995


# ---------------------------------------------------------------- second, independent restatement of the patch costs
def _np_patch_cost(img1, img2, c1, c2, x1, y1, x2, y2, R, coef):
    """numpy/float32 restatement of _d_compute_patch_dist (coef None, bao_pmflow_kernel.cu:255-301) and of ONE pass of
    _d_compute_patch_dist_planefitting (:353-391 with coef = (A, B, C, D) of :319-332), written from the .cu text, not from the
    C oracle: IEEE float32 elementwise operations, the terms added one by one in the source's loop order.  Only __expf comes
    from the shared formula (orc_fast_exp), as everywhere."""
    f32 = np.float32
    h, w = img1.shape
    gs, cn = O.pm_luts(R)
    fexp = O.lib().orc_fast_exp

    def tex(img, x, y):                       # point sampling, clamp addressing, unorm8 -> float
        p = img[min(max(int(y), 0), h - 1), min(max(int(x), 0), w - 1)]
        return f32(p["x"]) / f32(255.0), f32(p["y"]) / f32(255.0), f32(p["z"]) / f32(255.0)

    def cen(c, x, y):
        return int(c[min(max(int(y), 0), h - 1), min(max(int(x), 0), w - 1)])

    def maxdiff(a, b):
        return max(max(abs(f32(a[0] - b[0])), abs(f32(a[1] - b[1]))), abs(f32(a[2] - b[2])))

    cp1, cp2 = tex(img1, x1, y1), tex(img2, x2, y2)
    uu, vv = f32(x2 - x1), f32(y2 - y1)
    cost_sum, weight_sum = f32(0), f32(0)
    lam2, sig2 = f32(f32(0.1) * f32(0.1)), f32(f32(0.1) * f32(0.1))
    for i in range(-R, R + 1, 2):
        for j in range(-R, R + 1, 2):
            if coef is None:
                sx1, sy1, sx2, sy2 = x1 + j, y1 + i, x2 + j, y2 + i
            else:
                cx1, cy1 = f32(x1 + j), f32(y1 + i)
                cx2 = f32(f32(f32(cx1 + uu) + f32(f32(j) * f32(coef[0]))) + f32(f32(i) * f32(coef[1])))
                cy2 = f32(f32(f32(cy1 + vv) + f32(f32(j) * f32(coef[2]))) + f32(f32(i) * f32(coef[3])))
                sx1, sy1, sx2, sy2 = np.floor(cx1), np.floor(cy1), np.floor(cx2), np.floor(cy2)
            p1, p2 = tex(img1, sx1, sy1), tex(img2, sx2, sy2)
            k = bin(cen(c1, sx1, sy1) ^ cen(c2, sx2, sy2)).count("1")
            cost = maxdiff(p1, p2)
            cost = f32(f32(1) - f32(fexp(float(f32(-f32(cost * cost)) / lam2))))
            cost = f32(cost + cn[k])
            wgt = maxdiff(cp1, p1)
            wgt = f32(wgt * wgt)
            tmp = maxdiff(cp2, p2)
            tmp = f32(tmp * tmp)
            wgt = f32(fexp(float(f32(-f32(wgt + tmp)) / sig2)))
            wgt = f32(wgt * f32(gs[abs(j)] * gs[abs(i)]))
            cost = f32(cost * wgt)
            cost_sum = f32(cost_sum + cost)
            weight_sum = f32(weight_sum + wgt)
    return f32(cost_sum / weight_sum)


def test_patch_costs_against_a_second_restatement(crop_stages):
    """The C oracle's orc_patch_dist / orc_patch_dist_planefit equal, bit for bit, a second restatement written in numpy from
    the reference source (pins the oracle's reading of the sampling grid, the affine coordinate arithmetic, floor + clamp,
    the term order and the nested __min against an independently written one)."""
    st = crop_stages
    i1, i2, c1, c2 = st["img1_L1"], st["img2_L1"], st["cen1_L1"], st["cen2_L1"]
    h, w = i1.shape
    rng = np.random.default_rng(17)
    coefs = [(0.177, -0.011, -0.003, 0.301), (0.125, -0.357, 0.009, 0.308), (0.205, 0.370, 0.011, 0.296)]
    pts = [(0, 0, w, h), (w - 1, h - 1, -3, -2), (5, 7, 5, 7)] + [tuple(int(v) for v in (rng.integers(0, w), rng.integers(0, h), rng.integers(-4, w + 4), rng.integers(-4, h + 4))) for _ in range(12)]
    for (x1, y1, x2, y2) in pts:
        for R in (9, 5):
            want = _np_patch_cost(i1, i2, c1, c2, x1, y1, x2, y2, R, None)
            got = np.float32(O.patch_dist(i1, i2, c1, c2, x1, y1, x2, y2, patch_r=R))
            assert got.view(np.uint32) == want.view(np.uint32), ("plain", x1, y1, x2, y2, R, got, want)
        c = [_np_patch_cost(i1, i2, c1, c2, x1, y1, x2, y2, 9, None)] + [_np_patch_cost(i1, i2, c1, c2, x1, y1, x2, y2, 9, k) for k in coefs]
        m34 = c[2] if c[2] < c[3] else c[3]                       # __min(cost1,__min(cost2,__min(cost3,cost4))), :512
        m234 = c[1] if c[1] < m34 else m34
        want = c[0] if c[0] < m234 else m234
        got = np.float32(O.patch_dist(i1, i2, c1, c2, x1, y1, x2, y2, patch_r=9, planefit=True))
        assert got.view(np.uint32) == np.float32(want).view(np.uint32), ("planefit", x1, y1, x2, y2, got, want)


# ---------------------------------------------------------------- second restatements of the remaining stages (numpy, from the .cu text)
def _f32(x):
    return np.float32(x)


def _unorm(p):
    return _f32(p["x"]) / _f32(255.0), _f32(p["y"]) / _f32(255.0), _f32(p["z"]) / _f32(255.0)


def _maxdiff(a, b):
    return max(max(abs(_f32(b[0] - a[0])), abs(_f32(b[1] - a[1]))), abs(_f32(b[2] - a[2])))


def _fexp(x):
    return _f32(O.lib().orc_fast_exp(float(_f32(x))))


def test_second_restatement_prepare_stages(crop_stages):
    """census (bao_pmflow_census_kernel.cu:39-90), dense Gaussian (.cuh:437-467), uchar4 and float2 bilinear resize
    (.cuh:565-601, :511-537) restated in numpy on a sub-plane: byte / bit identical to the C oracle."""
    st = crop_stages
    img = st["img1_L1"][10:34, 20:52].copy()
    h, w = img.shape
    # census: bit k = lum(neighbour k) > lum(centre), clamp addressing, .3R + .6G + .1B evaluated left to right
    def lum(p):
        r, g, b = _unorm(p)
        return _f32(_f32(_f32(_f32(0.3) * r) + _f32(_f32(0.6) * g)) + _f32(_f32(0.1) * b))
    cen = np.zeros((h, w), np.uint8)
    offs = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
    for y in range(h):
        for x in range(w):
            c = lum(img[y, x])
            v = 0
            for k, (dx, dy) in enumerate(offs):
                if lum(img[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]) > c:
                    v += 1 << k
            cen[y, x] = v
    assert np.array_equal(cen, O.census(img))
    # Gaussian, sigma .5 radius 2 and sigma 1 radius 3: weight = __expf(-(dy^2+dx^2)/(2 sigma^2)), float sums in tap order, truncation
    for sigma, radius in ((0.5, 2), (1.0, 3)):
        s2 = _f32(_f32(_f32(sigma) * _f32(sigma)) * _f32(2))
        out = np.zeros((h, w), O.uchar4)
        for y in range(h):
            for x in range(w):
                val = [_f32(0)] * 4
                tot = _f32(0)
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        p = img[max(0, min(h - 1, y + dy)), max(0, min(w - 1, x + dx))]
                        wgt = _fexp(_f32(-_f32(dy * dy + dx * dx)) / s2)
                        for k, ch in enumerate("xyzw"):
                            val[k] = _f32(val[k] + _f32(_f32(p[ch]) * wgt))
                        tot = _f32(tot + wgt)
                for k, ch in enumerate("xyzw"):
                    out[ch][y, x] = int(_f32(val[k] / tot))
        assert np.array_equal(out.view(np.uint8), O.gauss_filter_rgba(img, sigma, radius).view(np.uint8)), (sigma, radius)
    # bilinear resizes: fx = (x+1)/ratio - 1, truncation, weights |1-m-dx| |1-n-dy|, m outer n inner
    def resize(get, put, oh, ow, ih, iw, ratio, nch):
        div = _f32(_f32(1.0) / _f32(ratio))
        for y in range(oh):
            for x in range(ow):
                fx = _f32(_f32(_f32(x + 1) * div) - _f32(1))
                fy = _f32(_f32(_f32(y + 1) * div) - _f32(1))
                xx, yy = int(fx), int(fy)
                dx = max(min(_f32(fx - _f32(xx)), _f32(1)), _f32(0))
                dy = max(min(_f32(fy - _f32(yy)), _f32(1)), _f32(0))
                res = [_f32(0)] * nch
                for m in (0, 1):
                    for n in (0, 1):
                        u, v = max(0, min(iw - 1, xx + m)), max(0, min(ih - 1, yy + n))
                        s = _f32(abs(_f32(_f32(1 - m) - dx)) * abs(_f32(_f32(1 - n) - dy)))
                        src = get(v, u)
                        for k in range(nch):
                            res[k] = _f32(res[k] + _f32(_f32(src[k]) * s))
                put(y, x, res)
    for (oh, ow, ratio) in ((h // 2, w // 2, 0.5), (7, 11, 0.37)):
        out = np.zeros((oh, ow), O.uchar4)
        resize(lambda v, u: [img[v, u][c] for c in "xyzw"],
               lambda y, x, r: [out[c].__setitem__((y, x), int(r[k])) for k, c in enumerate("xyzw")], oh, ow, h, w, ratio, 4)
        assert np.array_equal(out.view(np.uint8), O.resize_rgba(img, oh, ow, ratio).view(np.uint8)), ratio
    fl = st["flow_L2"][5:17, 8:26].copy()
    fl["x"][3, 4] = 1e10                      # unknown vectors are averaged in like any number
    fh, fw = fl.shape
    out = np.zeros((2 * fh, 2 * fw), O.float2)
    resize(lambda v, u: [fl["x"][v, u], fl["y"][v, u]],
           lambda y, x, r: (out["x"].__setitem__((y, x), r[0]), out["y"].__setitem__((y, x), r[1])), 2 * fh, 2 * fw, fh, fw, 2.0, 2)
    assert np.array_equal(out.view(np.uint32), O.resize_flow(fl, 2 * fh, 2 * fw, 2.0).view(np.uint32))


def test_second_restatement_level2_post_and_smoothing(crop_stages):
    """Left-right check, outlier vote, one weighted-median launch, hole filling, NNF->flow (bao_pmflow_refine_kernel.cu:53-76,
    :149-182, :198-259, :297-371, :636-655) and the joint-bilateral flow smoothing (:756-799), restated in numpy with the
    oracle's Jacobi order (read the input plane, write the output plane): identical to the C oracle on a sub-plane."""
    st = crop_stages
    ys, xs = slice(0, 30), slice(0, 40)
    img = st["img1_L2"][ys, xs].copy()
    h, w = img.shape
    INV = -10000
    rng = np.random.default_rng(4)
    # --- left-right check on synthetic NNFs (absolute coordinates inside / outside the sub-plane)
    n1 = np.zeros((h, w), O.short2)
    n2 = np.zeros((h, w), O.short2)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    n1["x"], n1["y"] = gx + 2, gy + 1                      # a consistent field: 1->2 shifts by (+2,+1), 2->1 by (-2,-1) ...
    n2["x"], n2["y"] = gx - 2, gy - 1
    pert = rng.random((h, w)) < 0.08                       # ... with some inconsistent matches and some targets outside the plane
    n1["x"][pert] += rng.integers(-3, 4, int(pert.sum())).astype(np.int16)
    n1["y"][pert] += rng.integers(-3, 4, int(pert.sum())).astype(np.int16)
    c1 = rng.random((h, w)).astype(np.float32)
    c2 = rng.random((h, w)).astype(np.float32)
    want, wc = n1.copy(), c1.copy()
    for y in range(h):
        for x in range(w):
            dx, dy = int(n1["x"][y, x]), int(n1["y"][y, x])
            bad = dy < 0 or dy >= h or dx < 0 or dx >= w
            if not bad:
                bad = abs(int(n2["x"][dy, dx]) - x) > 0 or abs(int(n2["y"][dy, dx]) - y) > 0
            if bad:
                want["x"][y, x] = want["y"][y, x] = INV
                wc[y, x] = np.finfo(np.float32).max
    got = O.left_right_check(n1, c1, n2, c2)
    assert np.array_equal(got[0].view(np.int16), want.view(np.int16)) and np.array_equal(got[1], wc)
    assert 0.05 < (want["x"] < 0).mean() < 0.5             # the check rejected some matches and kept most
    lr = got[0]
    # --- outlier vote: 13x13, |dflow| <= 2 in both components, self included, < 84 -> invalid
    want, wc = lr.copy(), got[1].copy()
    for y in range(h):
        for x in range(w):
            cx, cy = int(lr["x"][y, x]), int(lr["y"][y, x])
            if cx < 0 and cy < 0:
                continue
            fx, fy = np.int16(cx - x), np.int16(cy - y)
            cnt = 0
            for dy in range(-6, 7):
                for dx in range(-6, 7):
                    yy, xx = y + dy, x + dx
                    if xx < 0 or yy < 0 or xx >= w or yy >= h:
                        continue
                    nx, ny = np.int16(int(lr["x"][yy, xx]) - xx), np.int16(int(lr["y"][yy, xx]) - yy)
                    if abs(int(nx) - int(fx)) <= 2 and abs(int(ny) - int(fy)) <= 2:
                        cnt += 1
            if cnt < 84:
                want["x"][y, x] = want["y"][y, x] = INV
                wc[y, x] = np.finfo(np.float32).max
    got = O.outlier_removal(lr, wc * 0 + c1)      # (the cost plane's marks are not compared here)
    assert np.array_equal(got[0].view(np.int16), want.view(np.int16))
    assert ((want["x"] < 0) & (lr["x"] >= 0)).sum() > 10 and (want["x"] >= 0).mean() > 0.3      # some votes failed (borders), most of the interior stands
    holes = got[0].copy()
    holes["x"][12:17, 14:22] = INV
    holes["y"][12:17, 14:22] = INV
    # --- one weighted-median launch, occlusion only
    g = O.wmf_lut()
    sig2 = _f32(_f32(0.02) * _f32(0.02))
    want = holes.copy()
    for y in range(h):
        for x in range(w):
            if holes["x"][y, x] >= 0 and holes["y"][y, x] >= 0:
                continue
            centre = _unorm(img[y, x])
            best, ox, oy = np.finfo(np.float32).max, int(holes["x"][y, x]), int(holes["y"][y, x])
            taps = []
            for dy2 in range(-4, 5):
                for dx2 in range(-4, 5):
                    yy, xx = y + dy2, x + dx2
                    if xx < 0 or yy < 0 or xx >= w or yy >= h:
                        continue
                    dx_, dy_ = int(holes["x"][yy, xx]), int(holes["y"][yy, xx])
                    if dx_ < 0 or dy_ < 0:
                        continue
                    d = _maxdiff(centre, _unorm(img[yy, xx]))
                    wgt = _f32(_fexp(_f32(-_f32(d * d)) / sig2) * _f32(g[abs(dx2)] * g[abs(dy2)]))
                    taps.append((np.int16(dx_ - xx), np.int16(dy_ - yy), wgt))
            for (cfx, cfy, _) in taps:                # candidates = the same valid taps, row-major
                cs, ws = _f32(0), _f32(0)
                for (tfx, tfy, wgt) in taps:
                    cs = _f32(cs + _f32(wgt * _f32(max(abs(int(cfx) - int(tfx)), abs(int(cfy) - int(tfy))))))
                    ws = _f32(ws + wgt)
                if ws > 0 and cs < best:
                    best, ox, oy = cs, int(np.int16(int(cfx) + x)), int(np.int16(int(cfy) + y))
            if not (ox < 0 or oy < 0):
                want["x"][y, x], want["y"][y, x] = ox, oy
    assert np.array_equal(O.weighted_median(holes, img, 1, True).view(np.int16), want.view(np.int16))
    assert ((want["x"] >= 0) & (holes["x"] < 0)).sum() > 20                                       # the launch did fill pixels
    # --- hole filling: nearest valid left, right, up, down; closest colour, strict <
    want = holes.copy()
    for y in range(h):
        for x in range(w):
            cx, cy = int(holes["x"][y, x]), int(holes["y"][y, x])
            if cx >= 0 and cy >= 0:
                continue
            nd = [(cx, cy)] * 4
            npos = [(x, y)] * 4
            for k, rngk in enumerate((range(x - 1, -1, -1), range(x + 1, w), range(y - 1, -1, -1), range(y + 1, h))):
                for c in rngk:
                    yy, xx = (y, c) if k < 2 else (c, x)
                    nd[k] = (int(holes["x"][yy, xx]), int(holes["y"][yy, xx]))
                    if nd[k][0] >= 0 and nd[k][1] >= 0:
                        npos[k] = (xx, yy)
                        break
            cur = _unorm(img[y, x])
            bestd, fx, fy = np.finfo(np.float32).max, cx, cy
            for k in range(4):
                d = _maxdiff(cur, _unorm(img[npos[k][1], npos[k][0]]))
                if d < bestd and nd[k][0] >= 0 and nd[k][1] >= 0:
                    bestd, fx, fy = d, int(np.int16(nd[k][0] - npos[k][0])), int(np.int16(nd[k][1] - npos[k][1]))
            want["x"][y, x], want["y"][y, x] = np.int16(fx + x), np.int16(fy + y)
    filled = O.fill_holes(holes, img)
    assert np.array_equal(filled.view(np.int16), want.view(np.int16))
    assert ((want["x"] >= 0) & (holes["x"] < 0)).sum() > 20
    # --- NNF -> flow
    fl = O.nnf2flow(holes)
    for y in range(h):
        for x in range(w):
            dx, dy = int(holes["x"][y, x]), int(holes["y"][y, x])
            e = (1e10, 1e10) if (dx <= INV or dy <= INV) else (float(dx - x), float(dy - y))
            assert (fl["x"][y, x], fl["y"][y, x]) == (np.float32(e[0]), np.float32(e[1]))
    # --- joint-bilateral smoothing of the flow (21x21, unknown vectors skipped, written only when the weight sum is non-zero)
    b = O.blf_lut()
    hh, ww = 14, 18
    sub = img[:hh, :ww].copy()
    f = fl[:hh, :ww].copy()
    want = f.copy()
    for y in range(hh):
        for x in range(ww):
            centre = _unorm(sub[y, x])
            nx, ny, wsum = _f32(0), _f32(0), _f32(0)
            for dy in range(-10, 11):
                for dx in range(-10, 11):
                    yy, xx = y + dy, x + dx
                    if xx < 0 or yy < 0 or xx >= ww or yy >= hh:
                        continue
                    if f["x"][yy, xx] > 1e9 or f["y"][yy, xx] > 1e9:
                        continue
                    d = _maxdiff(centre, _unorm(sub[yy, xx]))
                    wgt = _f32(_fexp(_f32(-_f32(d * d)) / sig2) * _f32(b[abs(dx)] * b[abs(dy)]))
                    nx = _f32(nx + _f32(wgt * f["x"][yy, xx]))
                    ny = _f32(ny + _f32(wgt * f["y"][yy, xx]))
                    wsum = _f32(wsum + wgt)
            if wsum != 0:
                want["x"][y, x], want["y"][y, x] = _f32(nx / wsum), _f32(ny / wsum)
    assert np.array_equal(O.flow_smoothing(f, sub).view(np.uint32), want.view(np.uint32))


def test_second_restatement_patchmatch_steps(crop_stages):
    """Random initial NNF, the four segmented sweeps and the random search restated in numpy from bao_pmflow_kernel.cu
    (:73-109, :1049-1165, :1519-1586) with the order DESIGN.md 3.2 defines (all segments advance in lockstep, seeds read before
    step 0, the doubly visited forward pixel 10 seen by segment 1 first): NNF, cost and generator positions equal the C
    oracle's.  Patch costs come from orc_patch_dist, which test_patch_costs_against_a_second_restatement pins."""
    st = crop_stages
    i1, i2, c1, c2 = (st[k][:30, :40].copy() for k in ("img1_L2", "img2_L2", "cen1_L2", "cen2_L2"))
    h, w = i1.shape
    L = 10
    seed = 1234
    gx, gy = (w + 15) // 16, (h + 15) // 16

    def pd(x1, y1, x2, y2):
        return np.float32(O.patch_dist(i1, i2, c1, c2, int(x1), int(y1), int(x2), int(y2)))

    # ---- random field: thread (0,0) of each block draws r1, r2 per pixel, row-major over the FULL 16x16 block (:90-101)
    nnf = np.zeros((h, w), O.short2)
    for by in range(gy):
        for bx in range(gx):
            r = O.xorwow_stream(seed, by * gx + bx, 512)
            for i in range(16):
                for j in range(16):
                    x, y = bx * 16 + j, by * 16 + i
                    if x < w and y < h:
                        nnf["x"][y, x] = np.int16(int(r[2 * (16 * i + j)]) % (w + 1))
                        nnf["y"][y, x] = np.int16(int(r[2 * (16 * i + j) + 1]) % (h + 1))
    onnf, states = O.gen_rand_field(w, h, seed)
    assert np.array_equal(nnf.view(np.int16), onnf.view(np.int16))
    cost = O.cost_field(nnf, i1, i2, c1, c2)
    assert cost[3, 5].view(np.uint32) == pd(5, 3, nnf["x"][3, 5], nnf["y"][3, 5]).view(np.uint32)

    # ---- one sweep in lockstep
    def sweep(cost, nnf, direction):
        cost, nnf = cost.copy(), nnf.copy()
        is_row, rev = direction in (0, 2), direction in (2, 3)
        length, lines = (w, h) if is_row else (h, w)
        nseg = (length + L - 1) // L
        P = lambda line, i: (line, i) if is_row else (i, line)          # (y, x) index of position i on a line
        for line in range(lines):
            segs = []
            for k in range(nseg):
                if not rev:
                    start = 0 if k == 0 else k * L - 1
                    end = min(length - 1, start + L)
                    walk = list(range(start + 1, end + 1))
                else:
                    start = min((k + 1) * L, length - 1)
                    walk = list(range(start - 1, k * L - 1, -1))
                y, x = P(line, start)
                segs.append({"prev": [int(nnf["x"][y, x]), int(nnf["y"][y, x])], "walk": walk})     # seeds: before step 0
            for s in range(max(len(g["walk"]) for g in segs)):
                # forward: segment 1's first step precedes segment 0's last one on the shared pixel -- different steps, so the
                # order of the segments inside one step is immaterial (each step touches distinct pixels)
                for g in segs:
                    if s >= len(g["walk"]):
                        continue
                    i = g["walk"][s]
                    y, x = P(line, i)
                    px, py = g["prev"]
                    if is_row:
                        px = max(px - 1, 0) if rev else min(px + 1, w - 1)
                    else:
                        py = max(py - 1, 0) if rev else min(py + 1, h - 1)
                    cv = pd(x, y, px, py)
                    if cv < cost[y, x]:
                        nnf["x"][y, x], nnf["y"][y, x], cost[y, x] = px, py, cv
                        g["prev"] = [px, py]
                    else:
                        g["prev"] = [int(nnf["x"][y, x]), int(nnf["y"][y, x])]
        return cost, nnf

    cc, nn = cost, nnf
    for direction in range(4):
        wc, wn = sweep(cc, nn, direction)
        oc, on = O.seg_propagate_dir(cc, nn, i1, i2, c1, c2, direction)
        assert np.array_equal(wn.view(np.int16), on.view(np.int16)) and np.array_equal(wc.view(np.uint32), oc.view(np.uint32)), direction
        assert (wn.view(np.int16) != nn.view(np.int16)).any()            # the sweep changed something
        cc, nn = wc, wn

    # ---- random search: six guesses from the pre-search best, radii 30,15,7,3,1,1; block stream continues after the 512 init draws
    wc, wn = cc.copy(), nn.copy()
    for by in range(gy):
        for bx in range(gx):
            r = O.xorwow_stream(seed, by * gx + bx, 6 * 512, skip=512)
            for ty in range(16):
                for tx in range(16):
                    x, y = bx * 16 + tx, by * 16 + ty
                    if x >= w or y >= h:
                        continue
                    bxy = (int(nn["x"][y, x]), int(nn["y"][y, x]))
                    mag, guesses = 30, []
                    for k in range(6):
                        r1 = int(np.int16(np.uint16(int(r[512 * k + 2 * (16 * ty + tx)]) & 0xffff))) & 0xffffffff      # short(rdn) -> unsigned int
                        r2 = int(np.int16(np.uint16(int(r[512 * k + 2 * (16 * ty + tx) + 1]) & 0xffff))) & 0xffffffff
                        xmin, xmax = max(bxy[0] - mag, 0), min(bxy[0] + mag + 1, w + 1)
                        ymin, ymax = max(bxy[1] - mag, 0), min(bxy[1] + mag + 1, h + 1)
                        gxv = int(np.int16(np.uint16((xmin + r1 % (xmax - xmin)) & 0xffff)))
                        gyv = int(np.int16(np.uint16((ymin + r2 % (ymax - ymin)) & 0xffff)))
                        guesses.append((gxv, gyv))
                        if mag // 2 >= 1:
                            mag //= 2
                    best, bc = bxy, wc[y, x]
                    for g in guesses:
                        cv = pd(x, y, g[0], g[1])
                        if cv < bc:
                            best, bc = g, cv
                    wn["x"][y, x], wn["y"][y, x], wc[y, x] = best[0], best[1], bc
    os_, oc, on = O.random_search(states, cc, nn, i1, i2, c1, c2)
    assert np.array_equal(wn.view(np.int16), on.view(np.int16)) and np.array_equal(wc.view(np.uint32), oc.view(np.uint32))
    assert (wn.view(np.int16) != nn.view(np.int16)).any()
    for b in range(gx * gy):                                             # generator positions: 512 + 6*512 draws in
        assert np.array_equal(os_[b], O.xorwow_state(seed, b, skip=512 + 6 * 512))


def test_second_restatement_candidate_refine(crop_stages):
    """d_bilateral_refine_flow_planefitting (bao_pmflow_kernel.cu:2005-2041) in numpy: truncation of the up-sampled flow toward
    zero, 3x3 candidates with the x offset as the outer loop, out-of-image candidates skipped, strict <, unknown flow -> (0,0)."""
    st = crop_stages
    i1, i2, c1, c2 = (st[k][:22, :28].copy() for k in ("img1_L1", "img2_L1", "cen1_L1", "cen2_L1"))
    h, w = i1.shape
    rng = np.random.default_rng(8)
    f = np.zeros((h, w), O.float2)
    f["x"] = rng.normal(0, 2.5, (h, w)).astype(np.float32)
    f["y"] = rng.normal(0, 2.5, (h, w)).astype(np.float32)
    f["x"][3, 4] = f["y"][3, 4] = 1e10
    f["x"][0, 0], f["y"][0, 0] = -3.7, -2.2          # candidates outside the image
    want = f.copy()
    for y in range(h):
        for x in range(w):
            fx, fy = f["x"][y, x], f["y"][y, x]
            if fx > 1e9 or fy > 1e9:
                want["x"][y, x] = want["y"][y, x] = 0
                continue
            cx1, cy1 = int(fx) + x, int(fy) + y       # short(flow) truncates toward zero
            best, bc = (cx1, cy1), np.float32(999999)
            for m in (-1, 0, 1):
                for n in (-1, 0, 1):
                    cx, cy = cx1 + m, cy1 + n
                    if cx < 0 or cy < 0 or cx >= w or cy >= h:
                        continue
                    cv = np.float32(O.patch_dist(i1, i2, c1, c2, x, y, cx, cy, planefit=True))
                    if cv < bc:
                        best, bc = (cx, cy), cv
            want["x"][y, x], want["y"][y, x] = best[0] - x, best[1] - y
    assert np.array_equal(O.c2f_refine(f, i1, i2, c1, c2).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- the restated path computes optical flow (sign, axis and scale conventions)
def test_oracle_flow_explains_the_image_motion(crop, crop_stages):
    """Semantic sanity of the whole restated path, independent of any bit pattern: warping frame 2 back by the flow
    (I2(x + u, y + v), reference convention disp = target - source, u along x) must explain frame 1 far better than no motion,
    and on a synthetic pair with known motion the flow must be closer to the truth than the zero field and of the same sign."""
    from oracle import oracle as O
    from eppm_amd import synth
    a, b = crop
    u, v = crop_stages["u"], crop_stages["v"]
    h, w = u.shape
    yy, xx = np.mgrid[0:h, 0:w]
    warp = b[np.clip(np.rint(yy + v).astype(int), 0, h - 1), np.clip(np.rint(xx + u).astype(int), 0, w - 1)].astype(np.float64)
    err_flow = np.abs(a.astype(np.float64) - warp).mean()
    err_none = np.abs(a.astype(np.float64) - b.astype(np.float64)).mean()
    swapped = b[np.clip(np.rint(yy + u).astype(int), 0, h - 1), np.clip(np.rint(xx + v).astype(int), 0, w - 1)].astype(np.float64)
    negated = b[np.clip(np.rint(yy - v).astype(int), 0, h - 1), np.clip(np.rint(xx - u).astype(int), 0, w - 1)].astype(np.float64)
    assert err_flow < 0.5 * err_none, (err_flow, err_none)
    assert err_flow < np.abs(a - swapped).mean() and err_flow < np.abs(a - negated).mean()       # u is x, v is y, target - source
    sa, sb, gu, gv = synth.make_pair(144, 192, seed=5, max_flow=8.0)
    su, sv = O.compute_flow(sa, sb)
    m = np.s_[16:-16, 16:-16]
    epe = np.sqrt((su - gu) ** 2 + (sv - gv) ** 2)[m]
    zero = np.sqrt(gu ** 2 + gv ** 2)[m]
    assert epe.mean() < 0.6 * zero.mean() and np.median(epe) < 1.0, (epe.mean(), zero.mean(), np.median(epe))
    big = zero > 2.0                                                                          # where there is motion, the signs agree
    assert ((su[m] * gu[m] + sv[m] * gv[m])[big] > 0).mean() > 0.8


# ---------------------------------------------------------------- the error bar of "parity unpinned"
def test_parity_envelope_of_the_legal_alternative_readings(crop, crop_stages):
    """tools/parity_envelope.py on the 160x120 crop: how far the OTHER legal readings of the racy / unspecified parts of the
    reference move the flow away from the lockstep oracle.  Pins the finding DESIGN.md section 3.6 states: a different order of
    the racing sweeps or in-place post-processing, or another random stream, each moves the flow by 0.05 - 0.6 px mean EPE
    (hundreds of times north_star's 1e-3 px), while the arithmetic alternative (libm expf for the 2-ulp __expf) stays below
    1e-3 px -- so 1e-3 px against ONE run of the CUDA binary is not attainable by any implementation, including a second run
    of the CUDA binary on other hardware, and bit-exactness against a defined order is the only checkable statement."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import parity_envelope as PE
    a, b = crop
    env = PE.envelope(a, b, O)
    u, v = O.compute_flow(a, b)                        # the variant switch is back at the lockstep reading
    eq(u, crop_stages["u"], "u after the variants")
    eq(v, crop_stages["v"], "v after the variants")
    pinned = {"sweep_serial": 0.18276572594806909, "sweep_pixelL": 0.07964160849575345, "wmf_inplace": 0.51999, "smoothing_inplace": 0.15001,
              "other_stream": 0.16444956765237942}
    for name, want in pinned.items():
        got = env[name]["mean_epe_px"]
        assert abs(got - want) <= 2e-5 * max(1.0, want), (name, got, want)     # integer-order variants on the shared exp: deterministic
        assert got > 50 * 1e-3
    assert 0 < env["libm_expf"]["mean_epe_px"] < 1e-3 and env["libm_expf"]["frac_over_1px"] == 0      # depends on the host's libm in the last digits
    assert env["fill_inplace"]["mean_epe_px"] == 0.0                                                       # holes are far apart after 20 median launches
    assert env["outlier_inplace"]["mean_epe_px"] > 1000      # raster-order vote: every invalidated pixel stops supporting its neighbours, the field cascades
    assert env["all_but_outlier"]["mean_epe_px"] > 0.3


def test_config3_manifest_covers_all_64_pairs():
    """tests/golden/MANIFEST_config3.json (bench.py --verify-config3): 64 pairs, seeds 1234..1297, and its first eight agree with
    MANIFEST_large.json; pair 0's inputs regenerate on this host."""
    import hashlib
    from eppm_amd import shard, synth
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST_config3.json")))
    large = json.load(open(os.path.join(GOLDEN, "MANIFEST_large.json")))
    assert man["n_pairs"] == 64 and sorted(int(k) for k in man["pairs"]) == list(range(64))
    for i in range(64):
        assert man["pairs"][str(i)]["seed"] == 1234 + i
    for i in range(8):
        assert man["pairs"][str(i)]["flow_sha256"] == large[f"sintel_{1234 + i}"]["flow_sha256"]
    assert sorted(sum((shard.pairs_for_rank(64, r, 8) for r in range(8)), [])) == list(range(64))
    a, b, _, _ = synth.make_pair(man["h"], man["w"], seed=1234)
    assert hashlib.sha256(a.tobytes()).hexdigest() == man["pairs"]["0"]["img1_sha256"]


# ---------------------------------------------------------------- the speculative sweeps and their evaluation cache, restated
def test_speculative_sweep_form_and_evaluation_cache_equal_the_lockstep_sweeps(crop_stages):
    """DESIGN.md 3.2 / 4, on the CPU: the two-launch form of a sweep -- phase A evaluates, for every visited pixel, the candidate
    its chain tries when the previous pixel rejected (shift of that pixel's stored match), with no regard to the chains; phase B
    walks the chains in lockstep order, takes phase A's cost on every step that follows a rejection (or starts a segment) and
    evaluates only after an accepted candidate -- and the per-direction evaluation cache (a candidate evaluated for a pixel in an
    earlier sweep of the same direction is not evaluated again) restated in Python on the oracle's patch cost: NNF and cost equal
    orc_seg_propagate_dir's after every one of 12 sweeps (3 iterations x 4 directions, random searches in between), and the
    evaluation counts show what each device kernel saves."""
    st = crop_stages
    i1, i2, c1, c2 = (st[k][:30, :40].copy() for k in ("img1_L2", "img2_L2", "cen1_L2", "cen2_L2"))
    h, w = i1.shape
    L = 10
    evals = {"A": 0, "A_cached": 0, "B_fresh": 0}

    def pd(x1, y1, x2, y2):
        return np.float32(O.patch_dist(i1, i2, c1, c2, int(x1), int(y1), int(x2), int(y2)))

    def shift(c, direction):
        x, y = c
        if direction == 0: return (min(x + 1, w - 1), y)
        if direction == 1: return (x, min(y + 1, h - 1))
        if direction == 2: return (max(x - 1, 0), y)
        return (x, max(y - 1, 0))

    cache = [dict() for _ in range(4)]           # per direction: pixel (y, x) -> (candidate, cost)

    def sweep(cost, nnf, d):
        nin = nnf.copy()                         # phase A and the seeds read the input plane, every visited pixel is written to nout
        nout, cost = nnf.copy(), cost.copy()
        is_row, rev = d in (0, 2), d >= 2
        length, lines = (w, h) if is_row else (h, w)
        step = -1 if rev else 1
        at = (lambda line, i: (line, i)) if is_row else (lambda line, i: (i, line))      # (y, x) of position i on a line
        get = lambda plane, p: (int(plane["x"][p]), int(plane["y"][p]))
        # ---- phase A: the rejection-path candidate of every visited pixel (the first pixel of a line against the sweep is never visited)
        spec = {}
        for line in range(lines):
            for i in range(length):
                q = i - step
                if q < 0 or q >= length:
                    continue
                p = at(line, i)
                cand = shift(get(nin, at(line, q)), d)
                if cand == get(nin, p):
                    continue                     # equal to the pixel's own match: rejected unevaluated (skip rule)
                hit = cache[d].get(p)
                if hit is not None and hit[0] == cand:
                    evals["A_cached"] += 1       # evaluated by an earlier sweep of this direction: the cost stands
                else:
                    evals["A"] += 1
                    cache[d][p] = (cand, pd(p[1], p[0], cand[0], cand[1]))
                spec[p] = cache[d][p][1]
        # ---- phase B: the chains in lockstep order (segment 1 reaches forward pixel L before segment 0 does)
        nseg = (length + L - 1) // L
        for line in range(lines):
            chains = []
            for k in range(nseg):
                if not rev:
                    start = 0 if k == 0 else k * L - 1
                    count = min(length - 1, start + L) - start
                else:
                    start = min((k + 1) * L, length - 1)
                    count = start - k * L
                chains.append(dict(start=start, count=count, carry=get(nin, at(line, start)), from_nin=True))
            for s in range(L):
                order = range(nseg - 1, -1, -1) if not rev else range(nseg)          # the order that matters only for pixel L
                for k in order:
                    ch = chains[k]
                    if s >= ch["count"]:
                        continue
                    i = ch["start"] + step * (s + 1)
                    p = at(line, i)
                    cand = shift(ch["carry"], d)
                    own = get(nout, p) if (not rev and k == 0 and s == L - 1 and nseg > 1) else get(nin, p)
                    cur = cost[p]
                    if cand == own:
                        cv = cur
                    elif ch["from_nin"]:
                        cv = spec[p]             # phase A evaluated exactly this candidate
                    else:
                        evals["B_fresh"] += 1
                        cv = pd(p[1], p[0], cand[0], cand[1])
                    if cv < cur:
                        nout["x"][p], nout["y"][p] = cand
                        cost[p] = cv
                        ch["carry"], ch["from_nin"] = cand, False
                    else:
                        ch["carry"], ch["from_nin"] = own, True
        return cost, nout

    nnf, states = O.gen_rand_field(w, h)
    cost = O.cost_field(nnf, i1, i2, c1, c2)
    ocost, onnf = cost, nnf
    for it in range(3):
        for d in range(4):
            cost, nnf = sweep(cost, nnf, d)
            ocost, onnf = O.seg_propagate_dir(ocost, onnf, i1, i2, c1, c2, d)
            assert np.array_equal(nnf.view(np.int16), onnf.view(np.int16)), (it, d)
            assert np.array_equal(cost.view(np.uint32), ocost.view(np.uint32)), (it, d)
        states, ocost, onnf = O.random_search(states, ocost, onnf, i1, i2, c1, c2)
        cost, nnf = ocost, onnf
    visited = 12 * (h * w - min(h, w))          # roughly: every pixel but one per line, per sweep
    assert evals["A_cached"] > 0 and evals["B_fresh"] > 0
    assert evals["A"] + evals["B_fresh"] < visited      # fewer evaluations than the reference's one per visited pixel


# ---------------------------------------------------------------- the tolerance library's arithmetic, on the CPU
def test_tolerance_arithmetic_moves_no_match_on_the_bundled_pair(frames):
    """tools/tolerance_envelope.py's finding, which libeppm_hip_tol.so is built on, on the full bundled pair: the
    integer-domain table form of the patch term -- with fused accumulation (PatchMatch in its chunked canonical order, the refine in sample order) and the refine's
    weight as one exp2 of a summed argument, i.e. what the tolerance kernels compute -- changes most bits of the PatchMatch cost plane and NOT ONE match; the final flow
    stays three orders of magnitude inside north_star's 1e-3 px.  The same substitution in the smoothing alone moves ~88 % of the pixels
    (mean ~5e-4 px): the smoothed mean of equal integer flows sits on the next level's truncation boundary, which is why the tolerance
    library keeps the smoothing exact.  The oracle variants are test infrastructure; the parity oracle is the run with all of them off."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tolerance_envelope as TE
    a, b = frames
    u0, v0, st0 = O.compute_flow(a, b, dump=True)
    O.set_tol_variant(23, 3)                           # tables | fma | PatchMatch's chunked order | exp2 weights in the refine: what the kernels compute
    try:
        u1, v1, st1 = O.compute_flow(a, b, dump=True)
    finally:
        O.set_tol_variant()
    c0, c1 = st0["cost1_pm"], st1["cost1_pm"]
    assert (c0 != c1).mean() > 0.5                                     # a different arithmetic: most cost bits differ ...
    assert np.abs(c1 - c0).max() <= 1e-5 * np.abs(c0).max()
    assert np.array_equal(st0["nnf1_pm"], st1["nnf1_pm"]) and np.array_equal(st0["nnf2_pm"], st1["nnf2_pm"])      # ... and no decision does
    e = TE.epe_stats(u1, v1, u0, v0)
    assert e["mean_epe_px"] <= 1e-4 and e["frac_over_1px"] == 0.0, e
    O.set_tol_variant(1, 4)                            # the same tables in the smoothing only
    try:
        u2, v2 = O.compute_flow(a, b)
    finally:
        O.set_tol_variant()
    s = TE.epe_stats(u2, v2, u0, v0)
    assert s["frac_differing"] > 0.5 and 1e-4 < s["mean_epe_px"] < 1e-3, s
    u3, v3 = O.compute_flow(a, b)                      # the switch is back at the lockstep reading
    eq(u3, u0, "u after the variants")
    eq(v3, v0, "v after the variants")
