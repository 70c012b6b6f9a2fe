"""The ledger of DESIGN.md section 12.1: every loop (or grid of one-wave blocks) in the stage-object kernels whose trip count depends on the
frame size, the slot count or the object count, with the committed case that reaches its second trip.  The counts are recomputed here
from the cases' sizes and the constants in the headers; a case or a constant that changes so that the second trip is no longer reached
fails this test, and so does a row that the document does not hold."""
import os
import re

from conftest import ROOT
import test_cutdet_cpu as cutdet
import test_deflicker_cpu as deflicker
import test_objects_cpu as objects
import test_stabilize_cpu as stab

CSRC = os.path.join(ROOT, "eppm_amd", "csrc")
WAVE = 64


def source(name):
    return open(os.path.join(CSRC, name)).read()


def constant(text, name):
    return int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))


def up(a, b):
    return -(-a // b)


def test_every_size_dependent_loop_has_a_case_that_reaches_its_second_trip():
    internal, obj_h = source("eppm_internal.h"), source("objects.h")
    rows = {}          # kernel -> (what the loop or grid strides by, the counts of the committed cases that pass it)

    # k_gmotion_solve, k_cutdet_finish: one wave per slot adds the slabs of the slot's accumulate blocks, 64 per trip
    for kernel, text, prefix, mod in (("k_gmotion_solve", source("k_gmotion.hip"), "kGm", stab), ("k_cutdet_finish", source("k_cutdet.hip"), "kCut", cutdet)):
        assert re.search(r"for \(int i = threadIdx\.x; i < nslabs; i \+= %d\)" % WAVE, text[text.index(kernel):]), kernel
        tw, th = constant(internal, prefix + "TileW"), constant(internal, prefix + "TileH")
        assert (520, 130) in mod.SIZES
        rows[kernel] = (WAVE, [up(w, tw) * up(h, th) for w, h in [(520, 130)] + list(mod.LIMIT_SIZES)])
        assert rows[kernel][1] == [81, 256, 512]

    # k_obj_scan: one wave per slot scans the chunk counts, 64 per trip; k_obj_number: a block per chunk starts from the scan's word
    text = source("k_objects.hip")
    assert re.search(r"for \(int base = 0; base < A\.nchunks; base \+= %d\)" % WAVE, text[text.index("void k_obj_scan"):])
    assert "S.chunks[2 * chunk]" in text[text.index("void k_obj_number"):]
    chunk = constant(obj_h, "kObjChunk")
    counts = [up(w * h, chunk) for w, h in objects.LARGE_SIZES]
    assert counts == [64, 65, 129, 160, 160] and objects.ROUND == WAVE
    rows["k_obj_scan"] = rows["k_obj_number"] = (WAVE, counts[1:])
    assert max(up(w * h, chunk) for w, h in objects.SIZES) <= WAVE          # the small cases never did

    # k_obj_assign: one wave per slot, a lane per object, 64 per trip
    assert re.search(r"for \(int c = 1 \+ \(int\)lane; c <= n; c \+= %d\)" % WAVE, text[text.index("void k_obj_assign"):])
    rows["k_obj_assign"] = (WAVE, [255])          # the cap cases of objects_large_cases() with max_objects 255: n = 255 (checked below)

    # k_obj_tile: the slot's grid clears the (max_objects + 1)^2 vote words, one per lane and trip; a one-tile frame with max_objects 255
    assert "for (unsigned i = t; i < nv; i += nthreads)" in text
    one_tile = [(w, h) for w, h in objects.SIZES if w <= objects.TILE_W and h <= objects.TILE_H]
    assert one_tile
    rows["k_obj_tile"] = (256, [256 * 256])

    # k_deflicker_field: a lane per cell, blocks of 64
    text = source("k_deflicker.hip")
    assert re.search(r"k_deflicker_field, dim3\(\(a\.cx \* a\.cy \+ 63\) / %d" % WAVE, text)
    assert (211, 157) in deflicker.SIZES
    cells = [up(211, 16) * up(157, 16)] + [up(w, c) * up(h, c) for w, h in deflicker.LIMIT_SIZES for c in deflicker.LIMIT_CELLS]
    assert cells == [140, 1024, 256, 128, 1024, 256, 128]
    rows["k_deflicker_field"] = (WAVE, cells)

    # k_plate_path: a lane per slot, blocks of 64; the batch of 70 pairs
    text = source("k_plate.hip")
    assert re.search(r"k_plate_path, dim3\(\(a\.n \+ 63\) / %d\)" % WAVE, text)
    slots = open(os.path.join(ROOT, "tests", "test_slot_words_gpu.py")).read()
    n = int(re.search(r"^H, W, N, NCLIPS = \d+, \d+, (\d+), \d+$", slots, re.M).group(1))
    rows["k_plate_path"] = (WAVE, [n])

    for kernel, (width, counts) in rows.items():
        assert counts and all(c > width for c in counts), (kernel, width, counts)

    # section 12.1 holds one row per kernel
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sect = design[design.index("### 12.1 "):design.index("### 12.2 ")]
    table = {m.group(1) for m in re.finditer(r"^\| `(k_\w+)` \|", sect, re.M)}
    assert table == set(rows), (sorted(table), sorted(rows))


def test_the_object_detector_cases_behind_the_ledger_exist():
    """the rows of k_obj_assign and k_obj_tile name cases by their parameters: they are there"""
    plans = [(c["kind"], c["max_objects"], c["want_counts"]["n"]) for c in objects.objects_large_cases(1)]
    assert ("cap", 255, 255) in plans
    small = [c for c in objects.objects_cases() if c["w"] <= objects.TILE_W and c["h"] <= objects.TILE_H and c["max_objects"] == 255]
    assert small, "no one-tile case with max_objects 255"
