"""Deinterlacing in poisoned memory ("Write-before-read of every allocation"; section 26): the context form over the four-frame
clip and the caller-plane form on its pairs, each under the fills 0xFF, 0x01 and 0x7F of the test option "alloc_fill".  Every public
result must be the bytes of the unfilled run: an empty slot's reference planes are never read, a step writes every word of the other
reference plane and every byte of the mask plane, and a slot that was never stepped answers EPPM_ERR_STATE whatever its block holds."""
import pytest

from alloc_fill_child import CLIP_H, CLIP_W, DevMem, across_fills, clip, pair_inputs, put, status_of

pytestmark = pytest.mark.gpu

STATE = 3


def getters(out, name, di, slot):
    put(out, f"{name}.frame", di.frame(slot)); put(out, f"{name}.mask", di.mask(slot))
    put(out, f"{name}.stats", di.stats(slot)); put(out, f"{name}.state", di.state(slot))


def never_stepped(di, slot):
    got = {k: status_of(lambda k=k: getattr(di, k)(slot)) for k in ("frame", "mask", "stats", "state")}
    assert got == dict(frame=STATE, mask=STATE, stats=STATE, state=STATE), got


def attached():
    """the object on a context over the clip: a step per pair with alternating parity, the middle one with a cut flag, a reset before the
    last; every getter after every step"""
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        di = None
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            di = eppm_amd.Deinterlacer(e)
            never_stepped(di, 0)
            for k in range(3):
                if k:
                    e.push_frame(f[k + 1])
                e.compute_flow_bidirectional_device()
                if k == 2:
                    di.reset(0)
                di.step(cut=[k == 1], parity=[(k + 1) & 1])
                getters(out, f"pair{k}", di, 0)
        finally:
            if di is not None:
                di.close()
            e.close()
        return out
    return scenario


def size_only():
    """the object without a context, three slots: slot 1 is stepped first, then slot 0, slot 2 never; slot 1 goes on with a cut step, a
    reset and another step; every getter after every step"""
    import eppm_amd
    P = pair_inputs()
    pitch = CLIP_W * 4

    def scenario():
        out = {}
        di = eppm_amd.Deinterlacer(None, size=(CLIP_H, CLIP_W), slots=3)
        dev = []
        try:
            D = []
            for p in P:
                D.append({k: DevMem(p[k]) for k in ("rgba1", "rgba2", "bwd", "occ2")})
                dev += list(D[-1].values())

            def step(name, slot, k, parity, cut=False):
                d = {n: m.addr for n, m in D[k].items()}
                di.step_frames(slot, d["rgba1"], d["rgba2"], pitch, d["bwd"], d["occ2"], cut, parity)
                getters(out, name, di, slot)

            step("slot1.step1", 1, 0, 1)
            step("slot0.step1", 0, 0, 0)
            getters(out, "slot1.after_slot0", di, 1)
            step("slot1.step2_cut", 1, 1, 0, cut=True)
            di.reset(1)
            step("slot1.step3_after_reset", 1, 2, 1)
            step("slot0.step2", 0, 1, 1)
            never_stepped(di, 2)
            di.set_state(2, P[0]["rgba1"][..., :3])
            put(out, "slot2.loaded", di.state(2))
            assert status_of(lambda: di.frame(2)) == STATE
        finally:
            di.close()
            for d in dev:
                d.free()
        return out
    return scenario


@pytest.mark.parametrize("form", ["attached", "size_only"])
def test_deint_results_do_not_depend_on_what_memory_held(form):
    base = across_fills(attached() if form == "attached" else size_only(), f"deinterlacing, {form}")
    assert len(base) >= 15
    masks = {k: v for k, v in base.items() if k.endswith(".mask")}
    assert any((v == 1).any() and (v == 2).any() for v in masks.values())          # some step took pixels both ways
    cut = base["pair1.mask" if form == "attached" else "slot1.step2_cut.mask"]
    assert not (cut == 1).any() and (cut == 2).any()
