"""CPU tests of the streaming mode: the host form of the temporal prior against an independent numpy restatement
of the rule, the convergence of a seeded PatchMatch against a cold one with the CPU oracle, and the ABI's defaults and state errors that
need no GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

UNKNOWN = -10000


def make_clip(h, w, seed, n=4, max_flow=20.0):
    """synth.make_pair's pair, then frames 3.. by warping the last frame with the same flow (steady motion): (frames, u, v)."""
    from eppm_amd import synth
    a, b, u, v = synth.make_pair_cached(h, w, seed=seed, max_flow=max_flow)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = [a, b]
    while len(frames) < n:
        nxt = synth._bilinear(frames[-1].astype(np.float64), xx - u, yy - v)
        frames.append(np.clip(nxt, 0, 255).astype(np.uint8))
    return frames, u, v


def numpy_prior(prev, backward):
    """The rule of section 13, restated with array operations (no loop over pixels, no shared code with the library): every source with a
    known displacement lands on p + s*d; per landing pixel the smallest source index wins; the prior is landing pixel + d if inside."""
    from eppm_amd.api import short2
    h, w = prev.shape
    dx, dy = prev["x"].astype(np.int64).ravel(), prev["y"].astype(np.int64).ravel()
    idx = np.arange(h * w)
    x, y = idx % w, idx // w
    s = -1 if backward else 1
    qx, qy = x + s * dx, y + s * dy
    ok = (dx > UNKNOWN) & (dy > UNKNOWN) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    winner = np.full(h * w, np.iinfo(np.int64).max)
    np.minimum.at(winner, (qy * w + qx)[ok], idx[ok])
    has = winner < h * w
    wi = np.where(has, winner, 0)
    tx, ty = x + dx[wi], y + dy[wi]
    has &= (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    out = np.empty(h * w, short2)
    out["x"] = np.where(has, tx, UNKNOWN)
    out["y"] = np.where(has, ty, UNKNOWN)
    return out.reshape(h, w)


def random_field(rng, h, w, spread, unknown_fraction):
    from eppm_amd.api import short2
    f = np.empty((h, w), short2)
    f["x"] = rng.integers(-spread, spread + 1, (h, w))
    f["y"] = rng.integers(-spread, spread + 1, (h, w))
    m = rng.random((h, w)) < unknown_fraction
    f["x"][m] = UNKNOWN
    f["y"][m & (rng.random((h, w)) < 0.5)] = UNKNOWN - 7      # either component marks the vector, anything at or below the mark does
    return f


PRIOR_CASES = [(16, 16, 3, 0.0), (37, 53, 5, 0.2), (109, 256, 12, 0.1), (23, 9, 30, 0.3), (1, 40, 4, 0.0), (50, 1, 4, 0.1)]


@pytest.mark.parametrize("h,w,spread,unknown", PRIOR_CASES)
@pytest.mark.parametrize("backward", [False, True])
def test_prior_host_equals_numpy_rule(h, w, spread, unknown, backward):
    from eppm_amd import io
    rng = np.random.default_rng(h * 1000 + w + int(backward))
    for _ in range(3):
        prev = random_field(rng, h, w, spread, unknown)
        got, want = io.temporal_prior(prev, backward), numpy_prior(prev, backward)
        assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"])


def test_prior_host_named_cases():
    """Collision (two sources, one landing pixel: the smallest index wins), a target that leaves the frame, an unknown source."""
    from eppm_amd import io
    from eppm_amd.api import short2
    prev = np.zeros((4, 6), short2)
    prev["x"][:] = UNKNOWN
    prev["y"][:] = UNKNOWN
    prev[0, 0] = (2, 1)      # lands on (2, 1), index 0
    prev[1, 1] = (1, 0)      # lands on (2, 1) too, index 7: loses
    prev[2, 3] = (2, 0)      # lands on (5, 2); target (7, 2) leaves the frame: no prior
    prev[3, 0] = (-1, 0)     # lands outside: dropped
    p = io.temporal_prior(prev, False)
    assert tuple(p[1, 2]) == (4, 2)
    assert tuple(p[2, 5]) == (UNKNOWN, UNKNOWN)
    assert int((p["x"] > UNKNOWN).sum()) == 1
    b = io.temporal_prior(prev, True)      # q = p - d, target q + d = p
    assert tuple(b[1, 0]) == (1, 1) and tuple(b[2, 1]) == (3, 2) and tuple(b[3, 1]) == (0, 3)
    assert int((b["x"] > UNKNOWN).sum()) == 3          # (0, 0) - (2, 1) lies outside


def displacement(nnf):
    from eppm_amd.api import short2
    h, w = nnf.shape
    yy, xx = np.mgrid[0:h, 0:w]
    known = (nnf["x"] > UNKNOWN) & (nnf["y"] > UNKNOWN)
    d = np.empty((h, w), short2)
    d["x"] = np.where(known, nnf["x"] - xx, UNKNOWN)
    d["y"] = np.where(known, nnf["y"] - yy, UNKNOWN)
    return d


def select(rand, cost_rand, prior, cost_prior):
    """Section 13's select: the prior where it exists and is strictly cheaper, else the random match."""
    take = (prior["x"] > UNKNOWN) & (prior["y"] > UNKNOWN) & (cost_prior < cost_rand)
    nnf = rand.copy()
    nnf[take] = prior[take]
    return nnf, np.where(take, cost_prior, cost_rand).astype(np.float32)


def prior_or(prior, rand):
    """a field the cost function can take everywhere: the prior, the random match where there is none"""
    has = (prior["x"] > UNKNOWN) & (prior["y"] > UNKNOWN)
    f = rand.copy()
    f[has] = prior[has]
    return f


def test_oracle_seeded_convergence_1024x436():
    """Cold against seeded PatchMatch on pair (B, C) of the steady-motion clip at 1024x436, seed 1234, level 2, with the CPU oracle's stage
    functions.  Asserted: the seeded initial cost <= the cold one at every pixel; mean cost seeded(k) <= cold(k) for k = 0..3;
    seeded(1) <= cold(2); seeded(2) <= cold(3).  Reported, not asserted: k = 4, 5, 10 (both runs sit within 1 % of the converged cost)."""
    from eppm_amd import io
    from oracle import oracle as O
    O.set_num_threads(min(16, os.cpu_count() or 1))
    frames, _, _ = make_clip(436, 1024, 1234, n=3)
    prm = O.default_params()
    lv = [O.prepare(O.rgb2rgba(f)) for f in frames]
    L = 2
    (ia, ca), (ib, cb), (ic, cc) = [(im[L], ce[L]) for im, ce in lv]
    # the previous pair's forward field as nnf2flow converts it
    n1, c1 = O.patchmatch(ia, ib, ca, cb, prm)
    n2, c2 = O.patchmatch(ib, ia, cb, ca, prm)
    n1, c1, _, _ = O.left_right_check(n1, c1, n2, c2)
    n1, c1 = O.outlier_removal(n1, c1)
    n1 = O.weighted_median(n1, ia, prm.wmf_iters, True)
    n1 = O.fill_holes(n1, ia)
    prior = io.temporal_prior(displacement(n1), False)
    h, w = prior.shape
    have = float(((prior["x"] > UNKNOWN) & (prior["y"] > UNKNOWN)).mean())
    rand, states = O.gen_rand_field(w, h, prm.seed)
    cost_rand = O.cost_field(rand, ib, ic, cb, cc, prm)
    cost_prior = O.cost_field(prior_or(prior, rand), ib, ic, cb, cc, prm)
    seeded, cost_seeded = select(rand, cost_rand, prior, cost_prior)
    assert (cost_seeded <= cost_rand).all()

    def run(nnf, cost, iters=10):
        st = states.copy()
        means = [float(cost.mean())]
        for _ in range(iters):
            for d in range(4):
                cost, nnf = O.seg_propagate_dir(cost, nnf, ib, ic, cb, cc, d, prm)
            st, cost, nnf = O.random_search(st, cost, nnf, ib, ic, cb, cc, prm)
            means.append(float(cost.mean()))
        return means

    cold, warm = run(rand, cost_rand), run(seeded, cost_seeded)
    print(f"\npixels with a prior: {have:.3f}")
    print("k      " + " ".join(f"{k:7d}" for k in (0, 1, 2, 3, 4, 5, 10)))
    print("cold   " + " ".join(f"{cold[k]:7.4f}" for k in (0, 1, 2, 3, 4, 5, 10)))
    print("seeded " + " ".join(f"{warm[k]:7.4f}" for k in (0, 1, 2, 3, 4, 5, 10)))
    for k in range(4):
        assert warm[k] <= cold[k], (k, warm[k], cold[k])
    assert warm[1] <= cold[2], (warm[1], cold[2])
    assert warm[2] <= cold[3], (warm[2], cold[3])


def test_abi_defaults_and_errors_without_gpu():
    """The entry points exist in every library, argument errors need no device, and the header still compiles as C."""
    import eppm_amd
    L = eppm_amd.lib()
    for name in ("eppm_push_image", "eppm_push_image_device", "eppm_set_temporal", "eppm_temporal_reset", "eppm_temporal_valid",
                 "eppm_temporal_prior_host", "eppm_temporal_prior"):
        assert hasattr(L, name), name
    assert L.eppm_push_image(None, None, 0) == 1 and L.eppm_push_image_device(None, None, 0) == 1
    assert L.eppm_set_temporal(None, 1) == 1 and L.eppm_temporal_reset(None) == 1
    assert L.eppm_temporal_valid(None) == 0
    buf = (C.c_int16 * 8)()
    assert L.eppm_temporal_prior_host(None, buf, 2, 2, 0) == 1 and L.eppm_temporal_prior_host(buf, buf, 0, 2, 0) == 1
    src = "#include \"eppm.h\"\nint main(void) { return eppm_temporal_valid(0) + eppm_set_temporal(0, 0) + eppm_push_image(0, 0, 0); }\n"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_product_libraries_export_the_streaming_abi():
    import eppm_amd
    for variant in ("", "tol"):
        out = subprocess.run(["nm", "-D", "--defined-only", eppm_amd.lib_path(variant)], capture_output=True, text=True, check=True).stdout
        for name in ("eppm_push_image", "eppm_set_temporal", "eppm_temporal_prior_host", "eppm_temporal_prior"):
            assert f" T {name}\n" in out, (variant, name)
        assert "eppm_probe_ctx_rng_states" not in out
