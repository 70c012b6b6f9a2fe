"""Flicker removal in poisoned memory ("Write-before-read of every allocation"; section 24): the context form over the
four-frame clip and the caller-plane form on its pairs, each under the fills 0xFF, 0x01 and 0x7F of the test option "alloc_fill".  Every
public result must be the bytes of the unfilled run: an empty slot's reference planes are never read, every launch of a step writes all
it leaves -- the sums, the field and the valid byte of every cell, members or not --, and a slot that was never stepped answers
EPPM_ERR_STATE whatever its block holds."""
import numpy as np
import pytest

from alloc_fill_child import CLIP_H, CLIP_W, DevMem, across_fills, clip, pair_inputs, put, status_of

pytestmark = pytest.mark.gpu

STATE = 3
# 8 x 6 cells of 256 pixels; the clip's noise leaves about a quarter of a cell's pixels within tau: cells on both sides of n_min
PARAMS = dict(cell=16, n_min=64)


def getters(out, name, dk, slot):
    put(out, f"{name}.frame", dk.frame(slot)); put(out, f"{name}.field", dk.field(slot))
    put(out, f"{name}.stats", dk.stats(slot)); put(out, f"{name}.state", dk.state(slot))


def never_stepped(dk, slot):
    got = {k: status_of(lambda k=k: getattr(dk, k)(slot)) for k in ("frame", "field", "stats", "state")}
    assert got == dict(frame=STATE, field=STATE, stats=STATE, state=STATE), got


def attached():
    """the object on a context over the clip: a step per pair, the middle one with a cut flag, a reset before the last; every getter
    after every step"""
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        dk = None
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            dk = eppm_amd.Deflicker(e, **PARAMS)
            never_stepped(dk, 0)
            for k in range(3):
                if k:
                    e.push_frame(f[k + 1])
                e.compute_flow_bidirectional_device()
                if k == 2:
                    dk.reset(0)
                dk.step(cut=[k == 1])
                getters(out, f"pair{k}", dk, 0)
        finally:
            if dk is not None:
                dk.close()
            e.close()
        return out
    return scenario


def size_only():
    """the object without a context, three slots: slot 1 is stepped first, then slot 0, slot 2 never; slot 1 goes on with a cut step, a
    reset and another step; every getter after every step.  One pair's mask is set over the frame's left half: the field of cells outside
    any pass"""
    import eppm_amd
    P = [dict(p) for p in pair_inputs()]
    P[2]["occ2"] = P[2]["occ2"].copy()
    P[2]["occ2"][:, :CLIP_W // 2] = 1
    pitch = CLIP_W * 4

    def scenario():
        out = {}
        dk = eppm_amd.Deflicker(None, size=(CLIP_H, CLIP_W), slots=3, **PARAMS)
        dev = []
        try:
            D = []
            for p in P:
                D.append({k: DevMem(p[k]) for k in ("rgba1", "rgba2", "bwd", "occ2")})
                dev += list(D[-1].values())

            def step(name, slot, k, cut=False):
                d = {n: m.addr for n, m in D[k].items()}
                dk.step_frames(slot, d["rgba1"], d["rgba2"], pitch, d["bwd"], d["occ2"], cut)
                getters(out, name, dk, slot)

            step("slot1.step1", 1, 0)
            step("slot0.step1", 0, 0)
            getters(out, "slot1.after_slot0", dk, 1)
            step("slot1.step2_cut", 1, 1, cut=True)
            dk.reset(1)
            step("slot1.step3_after_reset", 1, 2)
            step("slot0.step2", 0, 1)
            never_stepped(dk, 2)
            dk.set_state(2, P[0]["rgba1"][..., :3])
            put(out, "slot2.loaded", dk.state(2))
            assert status_of(lambda: dk.frame(2)) == STATE
        finally:
            dk.close()
            for d in dev:
                d.free()
        return out
    return scenario


@pytest.mark.parametrize("form", ["attached", "size_only"])
def test_deflicker_results_do_not_depend_on_what_memory_held(form):
    base = across_fills(attached() if form == "attached" else size_only(), f"flicker removal, {form}")
    assert len(base) >= 15
    valid = {k: v for k, v in base.items() if ".field[1]" in k}
    assert any(v.any() and not v.all() for v in valid.values())          # some step left valid and invalid cells side by side
    if form == "size_only":
        v = valid["slot1.step3_after_reset.field[1]"].reshape(CLIP_H // 16, CLIP_W // 16)
        assert not v[:, :CLIP_W // 32].any()                               # the masked half: cells outside any pass
        ident = np.tile(np.array([1, 1, 1, 0, 0, 0], np.float32), (CLIP_H // 16, 1, 1)).view(np.uint8).ravel()
        f = base["slot1.step3_after_reset.field[0]"].reshape(CLIP_H // 16, CLIP_W // 16, 24)
        assert np.array_equal(f[:, 0].ravel(), ident)                      # ... and away from every valid cell the field is the identity
