"""The case table of tests/test_variants_gpu.py and its ledger.

Several launchers choose between kernels by the size of the launch.  Each of those choices is one host function,
which the test libraries answer through eppm_probe_dispatch (include/eppm_test.h) without a GPU.  The case table below is built from
those answers: for every decision, the smallest ragged shape on each side of the boundary, found by asking the probe -- no threshold is
written down here.  The ledger walks the table and asserts that the variants the cases reach are ALL the variants a decision function
can return, and that a case named "above" or "below" sits on that side: retuning a threshold moves the shapes, or fails here, but
never silently drops a kernel from the GPU suite.

The tables are functions (cached), not module constants: the child processes of the tolerance tests import this module before they
select their library, and build the tables from THAT library's answers."""
import functools

import pytest

RADII = (9, 17)
DIRS = (0, 1, 2, 3)


def probe(stage, *args, nout=1):
    from eppm_amd._lib import probe_dispatch
    r = probe_dispatch(stage, *args, nout=nout)
    return r[0] if nout == 1 else r


class option:
    """with option(name, value, default): a switch of include/eppm_test.h, back at its default afterwards"""

    def __init__(self, name, value, default):
        self.name, self.value, self.default = name.encode(), value, default

    def __enter__(self):
        import eppm_amd
        assert eppm_amd.lib().eppm_test_set_option(self.name, self.value) == 0

    def __exit__(self, *exc):
        import eppm_amd
        eppm_amd.lib().eppm_test_set_option(self.name, self.default)
        return False


def first_true(lo, hi, pred):
    """smallest v in [lo, hi] with pred(v), for a monotone pred; None when pred(hi) is false"""
    if not pred(hi):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


# ---- a. smoothing: pixels per lane ---------------------------------------------------------------------------------------------------
SMOOTH_H = 33        # odd, three tile rows of 16, the last of which holds a single image row


@functools.lru_cache(None)
def smoothing_cases():
    """(name, w, h, pixels per lane).  The width is the smallest at which a 33-row launch takes two pixels per lane -- one column into a
    new tile, so never a multiple of 32 --, one column less for the other kernel, and an even-height neighbour of the first so that
    k_flow_blf<2> also runs with the lower pixel present on its last row."""
    w2 = first_true(1, 1 << 16, lambda w: probe("smoothing", w, SMOOTH_H, 1) == 2)
    assert w2 is not None and w2 > 1
    return (("two_per_lane_odd_h", w2, SMOOTH_H, 2), ("one_per_lane", w2 - 1, SMOOTH_H, 1), ("two_per_lane_even_h", w2, SMOOTH_H + 1, 2))


# ---- b. refine: split factor -----------------------------------------------------------------------------------------------------------
# sub-crops (w, h) of the 160x120 level-0 planes of the crop, largest first: whole tiles, and ragged in both dimensions
REFINE_ALIGNED = [(w, h) for h in (112, 96, 80, 64, 48) for w in (160, 144, 128, 112, 96, 80, 64)]
REFINE_RAGGED = [(w - 3, h - 5) for (w, h) in REFINE_ALIGNED] + [(157, 119)]


@functools.lru_cache(None)
def refine_cases():
    """(name, w, h, patch_r, split factor): per radius one aligned and one ragged sub-crop for each factor the decision returns"""
    out = []
    for R in RADII:
        for factor in (3, 4):
            for kind, shapes in (("aligned", REFINE_ALIGNED), ("ragged", sorted(REFINE_RAGGED, key=lambda s: -s[0] * s[1]))):
                hit = [s for s in shapes if probe("refine", s[0], s[1], R, 1, 0) == factor]
                if hit:
                    out.append((f"R{R}_factor{factor}_{kind}", hit[0][0], hit[0][1], R, factor))
    return tuple(out)


# ---- c. search: rows per workgroup -----------------------------------------------------------------------------------------------------
SEARCH_W = 241       # 16 tile columns, the last one column wide


@functools.lru_cache(None)
def search_shapes():
    """{"above": (w, h), "below": (w, h)}: the smallest ragged height at which a one-problem search with numbers drawn ahead takes the
    quarter-block workgroups at radius 9, and a ragged height one tile row below it"""
    h4 = first_true(1, 1 << 14, lambda h: probe("search", SEARCH_W, h, 9, 1, 1, 1) == 4)
    assert h4 is not None and h4 > 16, h4
    if h4 % 16 == 0:
        h4 += 1
    assert probe("search", SEARCH_W, h4, 9, 1, 1, 1) == 4
    return {"above": (SEARCH_W, h4), "below": (SEARCH_W, (h4 - 1) // 16 * 16 - 1)}


NNFS = ("random", "arbitrary")


@functools.lru_cache(None)
def search_cases():
    """(name, side, w, h, patch_r, table, nnf, extra parameters, rows per workgroup)"""
    out = []
    for side, (w, h) in search_shapes().items():
        for R in RADII:
            for table in (1, 0):
                for nnf in NNFS:
                    out.append((f"{side}_R{R}_{'table' if table else 'drawing'}_{nnf}", side, w, h, R, table, nnf, (),
                                probe("search", w, h, R, 1, 1, table)))
        out.append((f"{side}_R9_table_random_8_guesses_range_1", side, w, h, 9, 1, "random", (("num_guess", 8), ("search_range", 1)),
                    probe("search", w, h, 9, 1, 1, 1)))
    return tuple(out)


# ---- d. classic sweep: lanes per chain, up-front fetch, tile or gather --------------------------------------------------------------------
SMALL = (80, 60)     # the level-1 planes of the crop


def sweep_form(w, h, R, seg_len):
    """the form of all four directions, which must agree for a case to stand for one variant"""
    forms = {probe("sweep", w, h, R, seg_len, d, 1, 1, nout=3) for d in DIRS}
    return forms.pop() if len(forms) == 1 else None


def sweep_extremes(R, seg_len):
    """the forms of a launch that cannot fill the chip and of one that can, at this radius and segment length"""
    return sweep_form(16, 16, R, seg_len), sweep_form(4000, 4000, R, seg_len)


def large_shape(R, seg_len):
    """the smallest ragged (s + 14) x s at which every direction takes the form of a launch that fills the chip; the small side when both
    forms are the same"""
    small, large = sweep_extremes(R, seg_len)
    if small == large:                        # one form at this radius: the shape radius 9 needs, so that the launch is as large
        return large_shape(9, seg_len) if R != 9 else SMALL
    for s in range(61, 1500, 2):
        if sweep_form(s + 14, s, R, seg_len) == large:
            return (s + 14, s)
    raise AssertionError(f"no shape up to 1500 takes {large} at R={R} seg_len={seg_len}")


def tile_limit(w, h, R):
    """the smallest segment length at which this launch's source tile no longer fits LDS"""
    s = first_true(1, 4096, lambda v: sweep_form(w, h, R, v) is not None and sweep_form(w, h, R, v)[2] == 0)
    assert s is not None and s > 1
    return s


@functools.lru_cache(None)
def sweep_cases():
    """(name, side, w, h, patch_r, seg_len, nnf, (lanes per chain, up-front fetch, tile))"""
    out = []

    def add(tag, side, w, h, R, seg_len, nnfs=NNFS):
        form = sweep_form(w, h, R, seg_len)
        assert form is not None, f"{tag}: the four directions of {w}x{h} R={R} seg_len={seg_len} take different forms"
        for nnf in nnfs:
            out.append((f"{tag}_R{R}_seg{seg_len}_{nnf}", side, w, h, R, seg_len, nnf, form))

    for R in RADII:
        add("small", "below", *SMALL, R, 10)
        add("large", "above", *large_shape(R, 10), R, 10)
        add("thin_strip", None, 24, 4000, R, 10, ("random",))
        add("tall_strip", None, 4000, 24, R, 10, ("random",))
        # the segment length at which the source tile stops fitting LDS, and one below it, for either lane width
        s = tile_limit(*SMALL, R)
        add("small_tile", None, *SMALL, R, s - 1, ("random",))
        add("small_gather", None, *SMALL, R, s, ("random",))
        if sweep_extremes(R, 10)[0] != sweep_extremes(R, 10)[1]:
            big = large_shape(R, 64)
            s = tile_limit(*big, R)
            big = large_shape(R, s)
            assert sweep_form(*big, R, s - 1) == sweep_form(*big, R, s)[:2] + (1,), "one shape on both sides of the tile limit"
            add("large_tile", "above", *big, R, s - 1, ("random",))
            add("large_gather", "above", *big, R, s, ("random",))
    return tuple(out)


# ---- e. speculative sweeps on a converged field: chosen by the data, listed for completeness ----------------------------------------------
CONVERGED_MODES = (0, 1, 2)          # sweep_spec of the stage launcher; 3 (the merged form) runs in a context


# ---- f. the ledger -------------------------------------------------------------------------------------------------------------------------

def test_probe_rejects_what_it_does_not_know():
    import eppm_amd
    from eppm_amd._lib import probe_dispatch
    with pytest.raises(eppm_amd.EppmError, match="unknown stage"):
        probe_dispatch("no_such_stage", 16, 16)
    with pytest.raises(eppm_amd.EppmError, match="takes 3 arguments"):
        probe_dispatch("smoothing", 16, 16)
    with pytest.raises(eppm_amd.EppmError, match="seg_len"):
        probe_dispatch("sweep", 80, 60, 9, 0, 0, 1, 1, nout=3)


def test_decisions_agree_with_the_pipeline_sizes_the_design_names():
    """the sizes whose measurements justify each threshold (comments at the thresholds) still fall where those comments say"""
    assert probe("smoothing", 1920, 1080, 1) == 2 and probe("smoothing", 1024, 436, 1) == 1
    assert probe("refine", 512, 218, 9, 1, 0) == 0                   # level 1 of one 1024x436 pair: 448 tiles, the window kernel
    assert probe("refine", 256, 109, 9, 1, 0) in (3, 4) and probe("refine", 256, 109, 9, 1, 1) == 0
    assert probe("refine", 64, 64, 5, 1, 0) == 0
    assert probe("search", 256, 109, 9, 2, 1, 1) == 2 and probe("search", 480, 270, 9, 2, 1, 1) == 4
    assert probe("search", 256, 109, 9, 2, 1, 0) == 4 and probe("search", 256, 109, 17, 2, 1, 1) == 4
    small, large = probe("sweep", 256, 109, 9, 10, 0, 2, 1, nout=3), probe("sweep", 256, 109, 9, 10, 0, 2, 8, nout=3)
    assert small[0] >= large[0] and small[1] == 1 and large[1] == 0 and small[2] == large[2] == 1
    assert probe("sweep", 256, 109, 5, 10, 0, 2, 1, nout=3) == (0, 0, 0)


def test_ledger_every_variant_of_every_decision_has_a_case():
    # a. smoothing
    assert {c[3] for c in smoothing_cases()} == {1, 2}
    for name, w, h, ppl in smoothing_cases():
        assert probe("smoothing", w, h, 1) == ppl, name
    name, w, h, _ = smoothing_cases()[0]
    assert h % 2 == 1 and w % 32 != 0 and h % 16 == 1, "the two-pixel kernel's shape: odd height, ragged width, one row in the last tile row"
    assert smoothing_cases()[2][2] % 2 == 0
    # b. refine: 3 and 4 per radius, aligned and ragged; no split at another radius
    for R in RADII:
        got = {(c[4], c[0].split("_")[-1]) for c in refine_cases() if c[3] == R}
        assert got == {(3, "aligned"), (3, "ragged"), (4, "aligned"), (4, "ragged")}, (R, got)
    for name, w, h, R, factor in refine_cases():
        assert probe("refine", w, h, R, 1, 0) == factor and probe("refine", w, h, R, 1, 1) == 0, name
        assert probe("refine", w, h, 5, 1, 0) == 0, name
        if name.endswith("ragged"):
            assert w % 16 and h % 16, name
    # c. search: the eighth-block form exists at radius 9 with the table only
    can = {(R, table): {probe("search", w, h, R, 1, 1, table) for (w, h) in ((16, 16), (4000, 4000))} for R in RADII for table in (0, 1)}
    assert can[(9, 1)] == {2, 4} and can[(9, 0)] == can[(17, 0)] == can[(17, 1)] == {4}, can
    for key, rows in can.items():
        assert {c[8] for c in search_cases() if (c[4], c[5]) == key} == rows, key
    for name, side, w, h, R, table, nnf, extra, rows in search_cases():
        assert probe("search", w, h, R, 1, 1, table) == rows, name
        assert (w % 16 and h % 16), name
        assert probe("search", w, h, 9, 1, 1, 1) == (4 if side == "above" else 2), name
    # d. classic sweep: every (lanes per chain, up-front fetch, tile) the decision returns over small and large launches and every
    # segment length, per radius
    for R in RADII:
        can = {sweep_form(w, h, R, s) for (w, h) in ((16, 16), (4000, 4000)) for s in range(1, 257)}
        got = {c[7] for c in sweep_cases() if c[4] == R}
        assert got == can, (R, got ^ can)
        small, large = sweep_extremes(R, 10)
        for name, side, w, h, RR, seg_len, nnf, form in sweep_cases():
            if RR != R:
                continue
            assert sweep_form(w, h, R, seg_len) == form, name
            if side == "above":                  # lanes per chain and up-front fetch of a launch that fills the chip / that cannot
                assert form[:2] == sweep_extremes(R, seg_len)[1][:2], name
            if side == "below":
                assert form[:2] == sweep_extremes(R, seg_len)[0][:2], name
        names = [c[0] for c in sweep_cases()]
        assert len(names) == len(set(names))
    # the gather cases sit exactly at the limit: one segment step shorter fits the tile
    for name, side, w, h, R, seg_len, nnf, form in sweep_cases():
        if "gather" in name:
            assert form[2] == 0 and sweep_form(w, h, R, seg_len - 1)[2] == 1, name
