"""CPU tests of batch streaming: the new entry points exist in every library, their argument errors need no
device, the header still compiles as C, and the schedule of flow_sequences keeps every pair of every clip exactly once."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

NAMES = ("eppm_batch_set_temporal", "eppm_batch_push_images", "eppm_batch_push_images_device", "eppm_batch_temporal_valid",
         "eppm_batch_temporal_reset", "eppm_temporal_prior_batch")


def test_all_four_libraries_export_the_batch_streaming_abi():
    import eppm_amd
    for variant in ("", "test", "tol", "tol_test"):
        out = subprocess.run(["nm", "-D", "--defined-only", eppm_amd.lib_path(variant)], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert f" T {name}\n" in out, (variant, name)
    for name in NAMES:
        assert name in eppm_amd._lib.SYMBOLS


def test_argument_errors_without_gpu():
    import eppm_amd
    L = eppm_amd.lib()
    one = (C.c_void_p * 1)()
    assert L.eppm_batch_set_temporal(None, 1) == 1
    assert L.eppm_batch_push_images(None, 1, one, C.c_size_t(12), None) == 1
    assert L.eppm_batch_push_images_device(None, 1, one, C.c_size_t(16), None) == 1
    assert L.eppm_batch_temporal_reset(None, 0) == 1 and L.eppm_batch_temporal_reset(None, -1) == 1
    assert L.eppm_batch_temporal_valid(None, 0) == 0
    buf = (C.c_int16 * 8)()
    for args in ((None, buf, 2, 2, 0, 1), (buf, None, 2, 2, 0, 1), (buf, buf, 0, 2, 0, 1), (buf, buf, 2, 0, 0, 1), (buf, buf, 2, 2, 0, 0),
                 (buf, buf, 2, 2, 0, 4097), (buf, buf, 32768, 2, 0, 1), (buf, buf, 32767, 32767, 0, 2)):
        assert L.eppm_temporal_prior_batch(*args, None) == 1, args[2:]


def test_header_compiles_as_c():
    src = ("#include \"eppm.h\"\nint main(void) { return eppm_batch_set_temporal(0, 0) + eppm_batch_push_images(0, 0, 0, 0, 0) + "
           "eppm_batch_push_images_device(0, 0, 0, 0, 0) + eppm_batch_temporal_valid(0, 0) + eppm_batch_temporal_reset(0, -1) + "
           "eppm_temporal_prior_batch(0, 0, 1, 1, 0, 1, 0); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


@pytest.mark.parametrize("lengths,slots", [([5, 2, 3, 2, 4], 2), ([3], 8), ([2, 2, 2], 3), ([2, 7, 2, 2, 3, 2, 2], 3), ([4, 4], 1)])
def test_sequence_plan(lengths, slots):
    from eppm_amd.api import _sequence_plan
    plan = list(_sequence_plan(lengths, slots))
    n = min(slots, len(lengths))
    assert all(len(step) == n for step in plan)
    kept = {c: [] for c in range(len(lengths))}
    held = [None] * n                                   # per slot: (clip, frame) of its image 2
    started = set()
    for t, step in enumerate(plan):
        for k, (c, f, cut, keep) in enumerate(step):
            if t == 0:
                assert (f, cut, keep) == (1, False, True) and c == k
                started.add(c)
                held[k] = (c, 0)                        # set_data: image 1 is frame 0
            # every first frame of a queued clip carries new_clip, and nothing else does
            assert cut == (f == 0), (t, k)
            if cut:
                assert c not in started and held[k][0] != c
                started.add(c)
            if keep:                                    # no kept pair spans two clips: image 1 is the frame before, of the same clip
                assert held[k] == (c, f - 1), (t, k, held[k], c, f)
                kept[c].append((f - 1, f))
            else:                                       # a cut, or an idle slot fed its last frame again
                assert cut or held[k] == (c, f)
            held[k] = (c, f)
    # every consecutive pair of every clip exactly once and in order
    for c, m in enumerate(lengths):
        assert kept[c] == [(i, i + 1) for i in range(m - 1)], (c, kept[c])
    # no step is wasted: the last one keeps something
    assert any(keep for _, _, _, keep in plan[-1])


def test_sequence_plan_refuses_short_clips():
    import eppm_amd
    from eppm_amd.api import _sequence_plan
    for lengths, slots in (([3, 1], 2), ([], 2), ([3], 0)):
        with pytest.raises(eppm_amd.EppmError):
            list(_sequence_plan(lengths, slots))
