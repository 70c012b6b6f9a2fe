"""Stage parity of the tolerance library's kernels (libeppm_hip_tol_test.so: the tolerance library's own objects plus the test hooks).

(a) every PatchMatch stage against the oracle variant (7, 1) -- tables, fma, the canonical chunked order --, every bit of every plane;
(b) a stored cost is the bits of the cost field of the stored match, whichever kernel wrote it (DESIGN.md section 9.2's tie invariant), in
    the tolerance library and, in this process, in the exact one;
(c) the candidate refine against the oracle variant (23, 2) at decision level: equal flows except at near ties of the variant's own cost;
(d) the PatchMatch planes and generator states of whole contexts, cold and seeded, against the oracle chain under (7, 1).

The pytest process holds the exact test library, so every tolerance test runs tests/tol_stage_child.py in a fresh child process that
selects "tol_test"; the oracle side runs there too.  Each child has a time limit of its own and its exit status is checked; children run
one after another, and nothing is started after a child that ended by a signal or its time limit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "tol_stage_child.py")
_stopped = []                  # why no further child is started


def run_child(part, *args, seconds=420):
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    cmd = [sys.executable, CHILD, "tol_test", part, *[str(a) for a in args]]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds, cwd=ROOT)
    except subprocess.TimeoutExpired as ex:
        _stopped.append(f"the child of {part} {args} exceeded its {seconds} s")
        pytest.fail(_stopped[0] + "\n" + str(ex.stdout or "")[-2000:])
    print(p.stdout[-6000:])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _stopped.append(f"the child of {part} {args} ended with status {p.returncode}")
        pytest.fail(_stopped[0] + "\n" + p.stdout[-2000:] + p.stderr[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert lines and lines[-1] == "PART OK" and "tolerance arithmetic" in lines[0], p.stdout[-2000:]
    return p.stdout


def test_tolerance_test_library_probes():
    """the switches and probes of include/eppm_test.h in the test build of the tolerance library: its own window,
    unpack_texel, the parity planes, fast_exp / div_const with the exact library's bits; the delta-table probe of the patch term answers
    EPPM_ERR_ARG with a message"""
    run_child("probes")


# ---- (a) ----

@pytest.mark.parametrize("image,patch_r,seg_len", [
    ("crop_L1", 9, 10), ("crop_L1", 9, 24), ("crop_L1", 9, 25), ("crop_L1", 9, 2),      # both sides of the LDS-tile limit, and two steps per chain
    ("crop_L1", 17, 10), ("crop_L1", 17, 25),
    ("crop_L1", 5, 10), ("crop_L1", 4, 7),                                              # generic radii: tol_chunk's (R + 2) / 2 branch
    ("ragged", 9, 10), ("ragged", 17, 3), ("ragged", 4, 24),                            # 101 x 77: no dimension a multiple of 16
    ("strip", 9, 10), ("strip", 17, 10),                                                # 6 x 1000: the patch is taller than the image
    ("flat11", 9, 10), ("flat12", 9, 5), ("flat13", 17, 10), ("flat14", 5, 7),          # costs tie by construction, weights underflow
])
def test_patchmatch_substages_equal_the_oracle_variant(image, patch_r, seg_len):
    """random field, cost field, four sweep directions in the classic form and under sweep_spec 1, 2 and 3, and the search drawing while
    it searches: NNF, cost and generator states == the oracle under (7, 1), bit for bit (NaNs compare equal, as in eq).  The stand-alone
    eppm_pm_random_search always streams; the search reading numbers drawn ahead exists in contexts only and is checked there (d)"""
    run_child("substages", image, patch_r, seg_len)


def test_patchmatch_evaluation_kernels_with_arbitrary_nnf_equal_the_oracle_variant():
    run_child("arbitrary_nnf")


def test_patchmatch_launcher_and_optional_propagations_equal_the_oracle_variant():
    """baoCudaPatchMatch under every sweep_spec (the merged form included), jump flood, 4-neighbour propagation"""
    run_child("launcher", seconds=600)


@pytest.mark.parametrize("stage,patch_r,group", [
    ("search", 9, "above"), ("search", 9, "below"), ("search", 17, "above"), ("search", 17, "below"),
    ("sweep", 9, "small"), ("sweep", 9, "large"), ("sweep", 9, "thin"), ("sweep", 9, "tall"),
    ("sweep", 17, "small"), ("sweep", 17, "large"), ("sweep", 17, "thin"), ("sweep", 17, "tall"),
])
def test_size_dependent_variants_equal_the_oracle_variant(stage, patch_r, group):
    """parts c and d of tests/test_variants_gpu.py on the tolerance library, whose search and sweep kernels are its own code: one search
    launch on each side of the eighth-block boundary (numbers drawn ahead and drawn while searching, the random and the arbitrary
    start field), and the classic sweep's four directions on small and large launches, strips, and both sides of the LDS tile's limit;
    shapes from this library's own dispatch probe"""
    out = run_child("variants", stage, patch_r, group, seconds=120)
    assert out.count("case ") >= 1


# ---- (b) ----

def test_one_cost_one_bit_pattern_tolerance_library():
    run_child("tie_invariant")


def test_one_cost_one_bit_pattern_exact_library():
    """the same code in this process: the exact test library"""
    import eppm_amd
    import tol_stage_child
    assert b"tolerance" not in eppm_amd.lib().eppm_version()
    tol_stage_child.part_tie_invariant()


# ---- (c) ----

@pytest.mark.parametrize("group", ["r9", "r17"])
def test_refine_decisions_equal_the_oracle_variant_up_to_near_ties(group):
    run_child("refine", group, seconds=600)


def test_refine_launcher_equals_the_oracle_variant_up_to_near_ties():
    run_child("refine_launcher")


# ---- (d) ----

@pytest.mark.parametrize("which", ["crop", "odd"])
def test_context_patchmatch_planes_equal_the_oracle_chain(which):
    """eppm_compute on the crop (160 x 120) and the odd crop (157 x 123), with and without the numbers drawn ahead, the library's own choice
    of the sweeps' form and the merged form: nnf1 / cost1 / nnf2 / cost2 bit for bit; the generator states after PatchMatch equal the
    oracle's where the context draws while it searches, and repeat from run to run where it reads numbers drawn ahead (those search
    kernels carry no state)"""
    run_child("context", which)


def test_seeded_context_equals_the_oracle_chain():
    """the part test_temporal_gpu.py could not run for the tolerance library: nnf_init* / cost_init* == select() over the variant's two cost
    fields, then the seeded PatchMatch's planes; the generator states of the seeded run equal the cold run's, and the oracle's where the
    context draws while it searches; with and without the numbers drawn ahead"""
    run_child("context_seeded", seconds=600)
