"""The two-phase random search on the GPU (csrc/k_pm_search.hip, PRE): one launch against the oracle's random search
bit for bit -- match field, costs, generator position -- on fields where nearly every guess survives the pre-test, where a handful do
and where none does; the rest-weight plane against its numpy statement; and whole contexts against the same build with the two-phase
form switched off, and against the committed flows of the 1024x436 pairs."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import search_pretest_model as M  # noqa: E402

from test_parity_gpu import O, S, eq  # noqa: F401  (S, O: fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(48, 20), (80, 36)]          # partial blocks on both edges; 3 x 2 and 5 x 3 blocks
LAUNCHES = [(1, 1), (2, 1), (2, 2)]    # (directions, pairs): one problem, forward + backward, a 2-pair batch
FIELDS = ["random", "converged", "all_rejected"]


@functools.lru_cache(None)
def pair(w, h, k):
    """level planes of pair k: (img1, img2, census1, census2)"""
    from oracle import oracle
    from eppm_amd import synth
    a, b, _, _ = synth.make_pair(h, w, seed=21 + k, max_flow=3.0)
    i1, i2 = oracle.rgb2rgba(a), oracle.rgb2rgba(b)
    return i1, i2, oracle.census(i1), oracle.census(i2)


def problem(w, h, k, d):
    i1, i2, c1, c2 = pair(w, h, k)
    return (i1, i2, c1, c2) if d == 0 else (i2, i1, c2, c1)


@functools.lru_cache(None)
def case(w, h, k, d, field):
    """(cost, nnf) the launch starts from and (states, cost, nnf) the oracle's search leaves, for direction d of pair k"""
    from oracle import oracle
    P = problem(w, h, k, d)
    nnf0, states = oracle.gen_rand_field(w, h)
    if field == "random":
        nnf, cost = nnf0, oracle.cost_field(nnf0, *P)
    else:
        nnf, cost = oracle.patchmatch(*P)
        if field == "all_rejected":
            cost = np.zeros_like(cost)
    return cost, nnf, oracle.random_search(states, cost, nnf, *P)


def launch(S, w, h, ndir, npairs, field, pretest=True, sums=False):
    rng = S.PmRng(w, h)
    S.pm_gen_rand_field(rng)          # the generator at the first search's position, as oracle.gen_rand_field leaves it
    probs = [(k, d) for k in range(npairs) for d in range(ndir)]
    costs = [case(w, h, k, d, field)[0] for k, d in probs]
    nnfs = [case(w, h, k, d, field)[1] for k, d in probs]
    out = S.pm_search_launch(rng, costs, nnfs, [pair(w, h, k)[:2] for k in range(npairs)], ndir, pretest, sums)
    return probs, out, rng.block_states()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("ndir,npairs", LAUNCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_two_phase_launch_equals_the_oracle(S, O, shape, ndir, npairs, field):
    w, h = shape
    probs, (costs, nnfs, _), states = launch(S, w, h, ndir, npairs, field)
    for i, (k, d) in enumerate(probs):
        ostates, ocost, onnf = case(w, h, k, d, field)[2]
        eq(nnfs[i], onnf, f"nnf pair {k} direction {d}")
        eq(costs[i], ocost, f"cost pair {k} direction {d}")
        eq(states, ostates, "generator position")
    if field == "all_rejected":          # and nothing was accepted: the fields stand
        for i, (k, d) in enumerate(probs):
            eq(nnfs[i], case(w, h, k, d, field)[1], "field untouched")
            assert not costs[i].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_rest_weight_plane_equals_numpy(S, shape):
    """to the last bit, edge pixels (whose source samples clamp) included; both directions of two pairs"""
    w, h = shape
    _, row0, rows, _, _, _ = S.probe_search_pretest(0, w, h)
    probs, (_, _, restw), _ = launch(S, w, h, 2, 2, "converged")
    for i, (k, d) in enumerate(probs):
        eq(restw[i], M.rest_weight(problem(w, h, k, d)[0], M.centre_rows(row0, rows)), f"rest weight pair {k} direction {d}")


@pytest.mark.parametrize("field", ["random", "converged"])
@pytest.mark.parametrize("shape", SHAPES)
def test_centre_row_sums_equal_numpy(S, shape, field):
    """N and D_A as the search's own helper forms them on its own tile, every pixel with its stored match as the guess (a random field: guesses
    all over the target, its clamped edges w and h included; a converged one: near matches), against the numpy statement that the CPU
    soundness tests run -- to the last bit, both directions of two pairs."""
    w, h = shape
    _, row0, rows, _, _, _ = S.probe_search_pretest(0, w, h)
    probs, out, _ = launch(S, w, h, 2, 2, field, sums=True)
    ys, xs = np.mgrid[0:h, 0:w]
    for i, (k, d) in enumerate(probs):
        nnf = case(w, h, k, d, field)[1]
        N, D = M.centre_sums(*problem(w, h, k, d), xs.reshape(-1), ys.reshape(-1), nnf["x"].reshape(-1), nnf["y"].reshape(-1), M.centre_rows(row0, rows))
        eq(out[3][i], N.reshape(h, w), f"N pair {k} direction {d}")
        eq(out[4][i], D.reshape(h, w), f"D_A pair {k} direction {d}")


def test_one_phase_launch_of_the_same_entry_equals_the_oracle(S, O):
    """the entry's pretest = 0 is today's kernel: the comparison above is not an artefact of the entry"""
    w, h = SHAPES[0]
    probs, (costs, nnfs, restw), states = launch(S, w, h, 2, 2, "random", pretest=False)
    assert restw is None
    for i, (k, d) in enumerate(probs):
        ostates, ocost, onnf = case(w, h, k, d, "random")[2]
        eq(nnfs[i], onnf, "nnf"); eq(costs[i], ocost, "cost"); eq(states, ostates, "generator position")


# ---- whole contexts --------------------------------------------------------------------------------------------------------------
def _with_pre_from(value, fn):
    import eppm_amd
    L = eppm_amd.lib()
    assert L.eppm_test_set_option(b"search_pre_from", value) == 0
    try:
        return fn()
    finally:
        assert L.eppm_test_set_option(b"search_pre_from", -1) == 0


def _clips(n, h, w):
    from eppm_amd import synth
    out = []
    for k in range(n):
        a, b, _, _ = synth.make_pair(h, w, seed=400 + (k % 4), max_flow=3.0)
        out.append((a, b, np.roll(b, (1, 2), (0, 1))))
    return out


def _single(seeded):
    from eppm_amd import api
    a, b, c = _clips(1, 48, 64)[0]
    e = api.EPPM()
    e.init(48, 64)
    try:
        e.set_temporal(seeded)
        e.set_data(a, b)
        f = [e.compute_flow()]
        if seeded:
            e.push_frame(c)
            f.append(e.compute_flow())
        return f
    finally:
        e.close()


def _batch(n, seeded):
    from eppm_amd import api
    clips = _clips(n, 48, 64)
    e = api.EPPMBatch(48, 64, n)
    try:
        e.set_temporal(seeded)
        e.set_data([(a, b) for a, b, _ in clips])
        f = [e.compute_flow()]
        if seeded:
            e.push_frames([c for _, _, c in clips])
            f.append(e.compute_flow())
        return f
    finally:
        e.close()


def _same(f, g):
    for x, y in zip(f, g):
        for p, q in zip(x, y) if isinstance(x, list) else [(x, y)]:
            eq(p[0], q[0], "u"); eq(p[1], q[1], "v")


@pytest.mark.parametrize("seeded", [False, True])
def test_context_flow_is_the_one_phase_flow(S, seeded):
    """64x48, three levels, plain and seeded start: the flow with the two-phase search from the first iteration on equals the flow with
    it switched off (a threshold beyond the last iteration).  One pair of that size searches in eighth-block workgroups, which have no
    two-phase form; a batch of as many pairs as make the library take quarter blocks does run it."""
    _same(_with_pre_from(0, lambda: _single(seeded)), _with_pre_from(1000, lambda: _single(seeded)))
    n = next(n for n in (32, 64, 128, 256) if S.probe_search_pretest(0, 16, 12, 9, 2, n)[5])
    _same(_with_pre_from(0, lambda: _batch(n, seeded)), _with_pre_from(1000, lambda: _batch(n, seeded)))


def test_batch_context_matches_the_committed_flows(S):
    """the first four pairs of the 1024x436 configuration through one batch context (quarter blocks: the library's own two-phase
    searches, and the two-phase form from the first iteration on) against their committed hashes"""
    from eppm_amd import api, synth
    assert S.probe_search_pretest(9, 256, 109, 9, 2, 4)[5]
    man = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "MANIFEST_config3.json")))
    pairs = [synth.make_pair_cached(man["h"], man["w"], seed=man["seed0"] + k)[:2] for k in range(4)]

    def run():
        e = api.EPPMBatch(man["h"], man["w"], 4)
        try:
            e.set_data(pairs)
            return e.compute_flow()
        finally:
            e.close()

    for flows in (run(), _with_pre_from(0, run)):
        for k, (u, v) in enumerate(flows):
            assert hashlib.sha256(u.tobytes() + v.tobytes()).hexdigest() == man["pairs"][str(k)]["flow_sha256"], k
