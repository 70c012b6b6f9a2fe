"""The batch sizes of tests/test_batch_forms_gpu.py and their ledger.

Every launcher that chooses between kernels decides by the size of the LAUNCH: pixels x problems x pairs.  The
single-pair ledger (tests/test_variants_cpu.py) reaches each "large launch" kernel at the smallest single-pair shape that takes it --
several hundred pixels a side.  A batch of many small pairs takes the same kernels on tiny ragged levels, with the pair index at values
no single-pair launch has.  This file builds the batch sizes n at which one 83x61 pair shape changes form, by asking the launchers' own
decision functions (eppm_probe_dispatch, include/eppm_test.h) for every n up to the capacity of the test's context: no threshold is
written down here, and the refine's split factor, which is not monotone in n, is scanned, not bisected.  The ledger asserts that over the
listed sizes every answer a decision can give for this shape is given, on both sides of every change: retuning a threshold moves the
batch sizes, or fails here, but never silently drops a kernel from the GPU suite.

The tables are functions (cached), not module constants: the child process of the tolerance test imports this module before it selects its
library, and builds the tables from THAT library's answers."""
import functools

import pytest

from test_variants_cpu import DIRS, RADII, probe

W, H = 83, 61            # every level is ragged against 16, 32 and 64
CAPACITY = 512           # pairs of the GPU test's context
PROBLEMS = 2             # a context's PatchMatch launch holds both directions of every pair


def params(R):
    import eppm_amd
    return eppm_amd.Params(patch_r=R)


@functools.lru_cache(None)
def level_dims():
    """[(w, h)] per level, from the library's own pyramid arithmetic (what eppm_level_dims answers for a context of this size; the GPU test
    asserts that it does)"""
    levels = params(9).levels
    nl = probe("levels", W, H, levels, 0, nout=3)[0]
    return tuple(probe("levels", W, H, levels, l, nout=3)[1:] for l in range(nl))


def decide(R, name, n):
    """the answer of decision `name` for a launch of n pairs at this shape and radius"""
    from eppm_amd import stages
    p = params(R)
    kind, _, level = name.rpartition("_L")
    w, h = level_dims()[int(level)]
    if kind == "smoothing":
        return probe("smoothing", w, h, n)
    if kind == "refine":
        return probe("refine", w, h, R, n, 0)
    if kind == "search_rows":
        return probe("search", w, h, R, PROBLEMS, n, 1)
    if kind == "search_two_phase":                # (has the form at all, the iterations that take it)
        return (stages.probe_search_pretest(0, w, h, R, PROBLEMS, n)[5],
                tuple(stages.probe_search_pretest(it, w, h, R, PROBLEMS, n)[0] for it in range(p.num_iter)))
    if kind.startswith("sweep_dir"):
        return probe("sweep", w, h, R, p.seg_len, int(kind[-1]), PROBLEMS, n, nout=3)
    if kind == "speculative":
        return tuple(probe("patchmatch", w, h, it, PROBLEMS, n, nout=2)[0] for it in range(p.num_iter))
    if kind == "merged":
        return tuple(probe("patchmatch", w, h, it, PROBLEMS, n, nout=2)[1] for it in range(p.num_iter))
    raise KeyError(name)


@functools.lru_cache(None)
def decisions():
    """every decision that depends on the pairs of a launch, at every level it applies to: the refine levels are smoothed and refined,
    the last level runs PatchMatch"""
    L = len(level_dims()) - 1
    out = [f"smoothing_L{l}" for l in range(L)] + [f"refine_L{l}" for l in range(L)]
    out += [f"search_rows_L{L}", f"search_two_phase_L{L}"] + [f"sweep_dir{d}_L{L}" for d in DIRS] + [f"speculative_L{L}", f"merged_L{L}"]
    return tuple(out)


@functools.lru_cache(None)
def scan(R):
    """{decision: [answer for n = 0 (None), 1, .., CAPACITY]}"""
    return {name: [None] + [decide(R, name, n) for n in range(1, CAPACITY + 1)] for name in decisions()}


@functools.lru_cache(None)
def change_points(R):
    """{decision: [n at which the answer differs from the one at n - 1]}"""
    return {name: [n for n in range(2, CAPACITY + 1) if a[n] != a[n - 1]] for name, a in scan(R).items()}


def mixed_sweeps(R):
    """the n at which the row sweeps (directions 0, 2) and the column sweeps (1, 3) of one iteration take different forms"""
    s = scan(R)
    L = len(level_dims()) - 1
    return [n for n in range(1, CAPACITY + 1) if {s[f"sweep_dir{d}_L{L}"][n] for d in (0, 2)} != {s[f"sweep_dir{d}_L{L}"][n] for d in (1, 3)}]


@functools.lru_cache(None)
def batch_sizes(R):
    """every change point n and n - 1; at radius 9 also one n > 1 of either split factor and one n inside the mixed-sweep interval.
    At radius 17 only the decisions that change at all contribute (the others have no change points)."""
    out = set()
    for name, cps in change_points(R).items():
        for n in cps:
            out |= {n, n - 1}
    if R == 9:
        s = scan(R)
        for factor in (3, 4):
            out.add(min(n for n in range(2, CAPACITY + 1) if s["refine_L0"][n] == factor))
        mixed = mixed_sweeps(R)
        out.add(mixed[len(mixed) // 2])
    return tuple(sorted(out))


@functools.lru_cache(None)
def change_sizes(R):
    """the sizes that are a change point (the upper side of a change): these also run the bidirectional call"""
    return tuple(sorted({n for cps in change_points(R).values() for n in cps}))


def forms(R, n):
    """{decision: answer} of a batch of n pairs: what a GPU case asserts it reaches"""
    return {name: scan(R)[name][n] for name in decisions()}


def case_id(R, n):
    """R9_n103_sweep_dir1_L2+sweep_dir3_L2: the decisions that change at n or at n + 1"""
    cps = change_points(R)
    at = [name for name in decisions() if n in cps[name]]
    below = [name for name in decisions() if n + 1 in cps[name]]
    tag = "+".join(at) if at else ("below_" + "+".join(below) if below else "inside")
    return f"R{R}_n{n}_{tag}"


# ---- what the launchers must then be seen to do (eppm_probe_launch_log) ---------------------------------------------------------------------

def expected_patchmatch_launches(R, n):
    """the sweep and search entries of one PatchMatch run of n pairs, in launch order, as (stage, form, extra)"""
    f = forms(R, n)
    L = len(level_dims()) - 1
    out = []
    for it in range(params(R).num_iter):
        if f[f"merged_L{L}"][it]:
            out.append(("sweeps_merged", 1, it))
        else:
            for d in DIRS:
                lpc, pre, tile = f[f"sweep_dir{d}_L{L}"]
                out.append(("sweep", -1 if f[f"speculative_L{L}"][it] else lpc * 4 + pre * 2 + tile, d))
        two_phase = int(f[f"search_two_phase_L{L}"][1][it])
        out.append(("search", 4 if two_phase else f[f"search_rows_L{L}"], two_phase))
    return out


def check_reached(entries, R, n, draft=False):
    """The launches of ONE compute of n pairs took the forms the probe answers for (level, n): every refine and smoothing launch of a
    level, and the PatchMatch level's sweeps and searches in their order.  draft: stop level 1 -- level 0 is upsampled, not refined."""
    f = forms(R, n)
    dims = level_dims()
    L = len(dims) - 1
    for stage, w, h, pairs, form, extra in entries:
        assert pairs == n, f"a {stage} launch of {pairs} pairs in a compute of {n}"
    for l in range(L):
        kinds = (("jbu", "smoothing"),) if draft and l == 0 else (("refine", "refine"), ("smoothing", "smoothing"))
        for stage, decision in kinds:
            got = [e[4] for e in entries if e[0] == stage and (e[1], e[2]) == dims[l]]
            assert got and set(got) == {f[f"{decision}_L{l}"]}, (f"level {l}, n = {n}: the {stage} launches took {got}, "
                                                                 f"the probe answers {f[f'{decision}_L{l}']}")
    if draft:
        assert not [e for e in entries if e[0] == "refine" and (e[1], e[2]) == dims[0]]
    pm = [(e[0], e[4], e[5]) for e in entries if e[0] in ("sweep", "sweeps_merged", "search")]
    assert all((e[1], e[2]) == dims[L] for e in entries if e[0] in ("sweep", "sweeps_merged", "search"))
    assert pm == expected_patchmatch_launches(R, n), f"level {L}, n = {n}: PatchMatch launched {pm}"


# ---- the ledger ------------------------------------------------------------------------------------------------------------------------

def test_probe_answers_for_the_new_stages():
    import eppm_amd
    from eppm_amd._lib import probe_dispatch
    assert level_dims()[0] == (W, H) and len(level_dims()) == params(9).levels
    for (w0, h0), (w1, h1) in zip(level_dims(), level_dims()[1:]):
        assert w1 < w0 and h1 < h0
    with pytest.raises(eppm_amd.EppmError, match="level"):
        probe_dispatch("levels", W, H, 3, 3, nout=3)
    with pytest.raises(eppm_amd.EppmError, match="takes 5 arguments"):
        probe_dispatch("patchmatch", W, H, 0, nout=2)
    # the merged form is a speculative form; neither is taken before the other's first iteration, and both are monotone in the iteration
    for n in (1, CAPACITY):
        w, h = level_dims()[-1]
        got = [probe("patchmatch", w, h, it, PROBLEMS, n, nout=2) for it in range(params(9).num_iter)]
        assert all(s >= m for s, m in got) and got == sorted(got), got
    # one 1920x1080 pair: speculative from some iteration on, merged later (the sizes DESIGN.md section 4.1 names)
    big = [probe("patchmatch", 480, 270, it, 2, 1, nout=2) for it in range(10)]
    assert big[0] == (0, 0) and big[-1] == (1, 1) and (1, 0) in big, big


@pytest.mark.parametrize("R", RADII)
def test_ledger_every_answer_of_every_decision_has_a_batch_size(R):
    sizes, s, cps = batch_sizes(R), scan(R), change_points(R)
    assert sizes and min(sizes) >= 1 and max(sizes) <= CAPACITY
    for name in decisions():
        can = set(s[name][1:])
        got = {s[name][n] for n in sizes}
        if len(can) > 1:
            assert got == can, (R, name, can - got)
        for n in cps[name]:                      # both sides of every change
            assert n in sizes and n - 1 in sizes, (R, name, n)
            assert s[name][n] != s[name][n - 1]
        if not cps[name]:
            assert len(can) == 1, (R, name)
    assert set(change_sizes(R)) <= set(sizes)
    ids = [case_id(R, n) for n in sizes]
    assert len(ids) == len(set(ids))


def test_ledger_radius_9_reaches_the_large_launch_forms():
    R, s = 9, scan(9)
    sizes = batch_sizes(R)
    L = len(level_dims()) - 1
    # every decision changes somewhere below the capacity at this shape: otherwise the GPU half runs one of its forms only
    for name in decisions():
        assert change_points(R)[name], f"{name} never changes for 1 <= n <= {CAPACITY}: the batch test no longer reaches its other form"
    # either split factor at n > 1, and the window kernel (no split) at both refine levels
    assert {s["refine_L0"][n] for n in sizes if n > 1} >= {0, 3, 4} and {s["refine_L1"][n] for n in sizes if n > 1} >= {0, 3, 4}
    # the four sweeps of one iteration in different forms: excluded by construction from the single-pair ledger
    mixed = [n for n in sizes if n in set(mixed_sweeps(R))]
    assert mixed, "no listed n has directions 0 / 2 and 1 / 3 in different sweep forms"
    assert any(n not in change_sizes(R) and n + 1 not in change_sizes(R) for n in mixed), "one n INSIDE the mixed interval"
    # quarter-block search with its two-phase form, the speculative and the merged sweeps, on the 20x15 level
    top = max(sizes)
    assert s[f"search_rows_L{L}"][top] == 4 and s[f"search_rows_L{L}"][1] == 2
    assert s[f"search_two_phase_L{L}"][top][0] and any(s[f"search_two_phase_L{L}"][top][1]) and not s[f"search_two_phase_L{L}"][1][0]
    assert any(s[f"speculative_L{L}"][top]) and any(s[f"merged_L{L}"][top]) and not any(s[f"speculative_L{L}"][1])
    # two pixels per lane at both refine levels; the largest n takes them at level 1
    assert s["smoothing_L0"][top] == 2 and s["smoothing_L1"][top] == 2 and s["smoothing_L1"][1] == 1
    assert min(n for n in sizes if s["smoothing_L0"][n] == 2) < min(n for n in sizes if s["smoothing_L1"][n] == 2)


def test_ledger_radius_17_is_cut_down_to_what_depends_on_the_pairs():
    R = 17
    changing = {name for name, cps in change_points(R).items() if cps}
    assert changing, "nothing depends on the pairs at radius 17"
    assert any(n.startswith("refine") for n in changing) and any(n.startswith("smoothing") for n in changing)
    want = set()
    for name in changing:
        for n in change_points(R)[name]:
            want |= {n, n - 1}
    assert set(batch_sizes(R)) == want
