"""Child process of tests/test_defect_gpu.py, and the home of what both share: device_step() runs one case of defect_cases() through
set_state + eppm_defect_step_frames + the getters on a context-less defect filter.  As a program it selects the tolerance library (the
pytest process holds the exact test library), runs every case twice and expects the kernels to equal the numpy restatement byte for byte
-- the filter has no EPPM_TOL branch --, then runs the end-to-end clip and prints its quality.  Prints the library's version first and
"PART OK" last."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))

from tfilter_tol_child import rgba, to_device  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_step(c, runs=2, slots=1, slot=0):
    """[(frame, mask, stats, saved frame, saved backward plane, has_prev)] of `runs` independent runs of case c on the device; the
    backward plane of the step's own pair is the case's forward plane negated (any plane will do: the step only saves it)"""
    import eppm_amd
    from eppm_amd._lib import lib
    h, w = c["h"], c["w"]
    nxt = c["cur"] if c["next"] is None else c["next"]
    own_bwd = np.stack([-c["fu"], -c["fv"]], -1).astype(np.float32)
    pad = c.get("pad", 0)
    planes = [to_device(rgba(c["cur"], pad=pad)), to_device(rgba(nxt, pad=pad)), to_device(np.stack([c["fu"], c["fv"]], -1).astype(np.float32)), to_device(own_bwd)]
    flt = eppm_amd.DefectFilter(None, size=(h, w), slots=slots, **c["params"])
    out = []
    try:
        for _ in range(runs):
            if c["prev"] is None:
                flt.reset(slot)
            else:
                flt.set_state(slot, c["prev"], np.stack([c["bu"], c["bv"]], -1), True)
            flt.step_frames(slot, planes[0].value, planes[1].value, (w + pad) * 4, planes[2].value, planes[3].value, c["next"] is None)
            out.append((flt.frame(slot), flt.mask(slot), flt.stats(slot)) + flt.state(slot))
    finally:
        flt.close()
        for p in planes:
            lib().eppm_free_device(p)
    for r in out:
        assert np.array_equal(r[3], c["cur"]) and np.array_equal(bits(r[4]), bits(own_bwd)) and r[5] == (c["next"] is not None), c["name"]
    return out


def mismatches(cases, want=None):
    """want(c): (rgb, mask, stats) to compare with; default: the case's restatement results"""
    bad = []
    for c in cases:
        rgb, mask, stats = want(c) if want else (c["want_rgb"], c["want_mask"], c["want_stats"])
        for k, r in enumerate(device_step(c)):
            if not np.array_equal(r[0], rgb) or not np.array_equal(r[1], mask) or r[2] != stats:
                bad.append((c["name"], k, int((r[0] != rgb).any(axis=-1).sum()), int((r[1] != mask).sum()), r[2], stats))
    return bad


def main():
    from test_defect_cpu import blotch_clip, clip_quality, defect_cases, defect_limit_cases, psnr    # (imports conftest, which selects the test library: overridden below)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    limit = sys.argv[1:2] == ["limit"]
    cases = defect_limit_cases(int(sys.argv[2])) if limit else defect_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    if limit:
        print("PART OK")
        return
    dirty, clean, masks, _ = blotch_clip()
    rep, rm = eppm_amd.remove_defects_sequence(dirty, masks=True, temporal=False)
    plain, ideal, _, _ = blotch_clip(blotched=())
    rep0 = eppm_amd.remove_defects_sequence(plain, temporal=False)
    loss = float(np.mean([psnr(plain[k], ideal[k]) - psnr(rep0[k], ideal[k]) for k in (1, 2, 3)]))
    print("QUALITY " + json.dumps(dict(zip(("found", "false_hit", "before", "after"), clip_quality(dirty, clean, masks, rep, rm)), clean_loss=loss)))
    print("PART OK")


if __name__ == "__main__":
    main()
