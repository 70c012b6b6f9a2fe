"""Background plates in poisoned memory ("Write-before-read of every allocation"; section 22): the context form over the
four-frame clip and the caller-plane form on its pairs, each under the fills 0xFF, 0x01 and 0x7F of the test option "alloc_fill".  Every
public result must be the bytes of the unfilled run: an empty slot's canvas is never read, a step defines every state it leaves, and the
scratch of the synchronous calls is written before it is copied."""
import numpy as np
import pytest

from alloc_fill_child import CLIP_H, CLIP_W, DevMem, across_fills, clip, pair_inputs, put, status_of

pytestmark = pytest.mark.gpu

STATE = 3
PARAMS = dict(margin_x=5, margin_y=3)


def getters(out, name, pl, slot, mask=True):
    put(out, f"{name}.plate", pl.plate(slot)); put(out, f"{name}.coverage", pl.coverage(slot))
    put(out, f"{name}.state", pl.state(slot)); put(out, f"{name}.path", pl.path(slot))
    if mask:
        put(out, f"{name}.mask", pl.mask(slot))


def attached():
    """the plate on a context over the clip: a step per pair, the middle one with a cut flag, a reset before the last; every getter and
    the render after every step"""
    import eppm_amd
    f = clip()

    def scenario():
        out = {}
        e = eppm_amd.EPPM()
        pl = None
        try:
            e.init(CLIP_H, CLIP_W)
            e.set_data(f[0], f[1])
            pl = eppm_amd.BackgroundPlate(e, **PARAMS)
            for k in range(3):
                if k:
                    e.push_frame(f[k + 1])
                e.compute_flow_bidirectional_device()
                if k == 2:
                    pl.reset(0)
                pl.step(cut=[k == 1])
                getters(out, f"pair{k}", pl, 0)
                put(out, f"pair{k}.render", pl.render(0))
        finally:
            if pl is not None:
                pl.close()
            e.close()
        return out
    return scenario


def size_only():
    """the plate without a context, three slots: slot 1 is stepped first, then slot 0, slot 2 never; slot 1 goes on with a cut step, a
    reset and another step; every getter and a render on caller planes after every step"""
    import eppm_amd
    P = pair_inputs()
    pitch = CLIP_W * 4
    paths = [(1, 0, 0, 1, 0, 0), (1.001, 0.002, -0.002, 0.999, 2.25, 1.5), (1, 0, 0, 1, 4.0, 2.0)]

    def scenario():
        out = {}
        pl = eppm_amd.BackgroundPlate(None, size=(CLIP_H, CLIP_W), slots=3, **PARAMS)
        dev = []
        try:
            D = []
            for p in P:
                D.append({k: DevMem(p[k]) for k in ("rgba1", "mask")})
                dev += list(D[-1].values())
            o, fl = DevMem(nbytes=CLIP_H * pitch), DevMem(nbytes=CLIP_H * CLIP_W)
            dev += [o, fl]

            def step(name, slot, k, cut=False, path=True):
                pl.step_frames(slot, D[k]["rgba1"].addr, pitch, D[k]["mask"].addr, paths[k] if path else None, cut)
                getters(out, name, pl, slot, mask=False)
                pl.render_frames(slot, D[k]["rgba1"].addr, pitch, D[k]["mask"].addr, None, o.addr, pitch, fl.addr)
                put(out, f"{name}.render", o.get((CLIP_H, CLIP_W, 4), np.uint8)); put(out, f"{name}.fill", fl.get((CLIP_H, CLIP_W), np.uint8))

            step("slot1.step1", 1, 0)
            step("slot0.step1", 0, 0)
            getters(out, "slot1.after_slot0", pl, 1, mask=False)
            step("slot1.step2_cut", 1, 1, cut=True)
            pl.reset(1)
            step("slot1.step3_after_reset", 1, 2, path=False)
            step("slot0.step2", 0, 1)
            got = {"plate": status_of(lambda: pl.plate(2)), "state": status_of(lambda: pl.state(2)), "mask": status_of(lambda: pl.mask(2)),
                   "path": pl.path(2).tolist()}
            assert got == {"plate": STATE, "state": STATE, "mask": STATE, "path": [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]}, got
            assert status_of(lambda: pl.mask(0)) == STATE          # a step without a fit leaves no mask
        finally:
            pl.close()
            for d in dev:
                d.free()
        return out
    return scenario


@pytest.mark.parametrize("form", ["attached", "size_only"])
def test_plate_results_do_not_depend_on_what_memory_held(form):
    base = across_fills(attached() if form == "attached" else size_only(), f"background plate, {form}")
    assert any(".render" in k for k in base) and len(base) >= 15
    cov = [v for k, v in base.items() if k.endswith(".coverage")]
    assert all(c.any() for c in cov)          # every step accumulated something
