"""GPU tests of the sentence every allocation of the library leans on (mem_cache.cpp): "nothing depends on a block's contents: every plane
is written before it is read".  The test option "alloc_fill" (include/eppm_test.h) fills every device and pinned block the library
allocates -- fresh, recycled or from the retry -- with a chosen byte before it is handed out; every public result must then be the same
bytes as in the unfilled run, under 0xFF (NaN floats, -1 integers), 0x01 (denormal floats, small positive shorts, "set" mask and label
bytes) and 0x7F (huge finite floats), and equal to the oracle where the suite has one.  The scenarios live in tests/alloc_fill_child.py,
which also runs all of them on the tolerance library in a child process.  DESIGN.md, "Write-before-read of every allocation", has the
audit these tests hold the code to."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
import alloc_fill_child as A

pytestmark = pytest.mark.gpu


def test_the_fill_reaches_the_memory():
    """fill 0x7F: a new 97x75 context's img1 plane, read before any set_data (eppm_get_plane has no state check for it), is 0x7F in every
    byte; nothing is claimed about an unfilled block"""
    A.control()


# ---- A: the core path ----
@pytest.mark.parametrize("size", ["crop", "sub"])
def test_core_forms(size, crop_stages):
    """set_data + compute_flow, begin / end, the device form and the colour-coded flow at both still sizes, with flow, img1/2 and census1/2
    of every level and nnf1/2, cost1/2 of the top level; on the crop u, v also equal the oracle under every fill"""
    A.across_fills(A.core_forms(size), f"core forms {size}", A.oracle_flow_check(crop_stages) if size == "crop" else None)


@pytest.mark.parametrize("size", ["crop", "sub"])
def test_core_in_a_recycled_slab(size, crop_stages):
    """cache_alloc's other path: the context takes the slab and the pinned buffers a destroyed context of its size left in the cache --
    that context's leftovers in the unfilled run, the fill otherwise"""
    A.across_fills(A.core_recycled(size), f"core recycled {size}", A.oracle_flow_check(crop_stages) if size == "crop" else None)


@pytest.mark.parametrize("option,value,default", [(None, 0, 0)] + list(A.VARIANTS), ids=lambda v: str(v))
def test_core_under_the_variant_switches(option, value, default, crop_stages):
    """the plain compute on the crop, twice per context, under every switch that changes which planes are used: every variant computes the
    oracle's bits, under every fill"""
    A.across_fills(A.core_variant(option, value, default), f"core {option}={value}", A.oracle_flow_check(crop_stages))


def test_core_at_the_second_patch_radius():
    A.across_fills(A.core_variant(None, 0, 0, patch_r=A.SECOND_RADIUS), f"core patch_r={A.SECOND_RADIUS}")


@pytest.mark.parametrize("force_split", [False, True], ids=["plain", "split_refine"])
def test_reference_abi_launchers(force_split):
    """the reference-signature stage launchers in the class's order on the crop: their work planes are the launchers' scratch, which the
    option fills at every hand-out"""
    A.across_fills(A.ref_abi_path(force_split), "reference-ABI launchers")


# ---- B: the lazily made blocks ----
@pytest.mark.parametrize("after_forward", [False, True], ids=["first_call", "after_forward"])
@pytest.mark.parametrize("op", A.LAZY_OPS)
def test_lazy_blocks(op, after_forward):
    A.across_fills(A.lazy_block("sub", op, after_forward), f"lazy {op} after_forward={after_forward}")


def test_lazy_bidirectional_on_the_crop():
    A.across_fills(A.lazy_block("crop", "bidir", False), "lazy bidir crop")


# ---- C: streaming and draft ----
@pytest.mark.parametrize("stop_level", [0, 1, 2])
def test_streaming_and_draft(stop_level):
    A.across_fills(A.streaming(stop_level), f"streaming stop_level={stop_level}")


# ---- D: batch contexts ----
@pytest.mark.parametrize("case", ["shrink", "partial"])
def test_batch(case):
    A.across_fills(A.batch(case), f"batch {case}")


# ---- E: the attachments ----
@pytest.mark.parametrize("kind", A.ATTACHMENTS)
def test_attachment_on_a_context(kind):
    A.across_fills(A.attached(kind), f"attached {kind}")


@pytest.mark.parametrize("kind", A.ATTACHMENTS)
def test_attachment_without_a_context(kind):
    """three slots, slot 1 stepped first, then slot 0, slot 2 never: its getters answer what they answer today.  (The tracker has one state
    and no constructor without a context: its caller-plane form.)"""
    A.across_fills(A.tracker_frames() if kind == "tracker" else A.size_only(kind), f"size-only {kind}")


def test_tolerance_library_under_the_fills():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "alloc_fill_child.py")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("PART OK"), out.stdout[-2000:] + out.stderr[-3000:]
    assert "tolerance arithmetic" in out.stdout.splitlines()[0]
