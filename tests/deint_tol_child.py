"""Child process of tests/test_deint_gpu.py, and the home of what both share: device_steps() runs one case of deint_cases() through
set_state + eppm_deint_step_frames + the getters on a context-less object, both of its steps; device_bob() runs k_deint_bob on caller
planes.  As a program it selects the tolerance library (the pytest process holds the exact test library) and expects the kernels to equal
the numpy restatement byte for byte on every case -- deinterlacing has no EPPM_TOL branch.  Prints the library's version first and
"PART OK" last."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))

from deflicker_tol_child import rgba, to_device      # noqa: E402


def step_planes(c, s):
    """the caller planes of one step of a case on the device: image 1, image 2, the backward flow, occ2"""
    pad = c.get("pad", 0)
    return [to_device(rgba(c["img1"], pad=pad)), to_device(rgba(s["cur"], pad=pad)), to_device(np.stack([s["bu"], s["bv"]], -1).astype(np.float32)),
            to_device(s["occ2"])]


def read(di, slot):
    return di.frame(slot), di.mask(slot), di.stats(slot)


def device_steps(c, slot=0, slots=1):
    """[(rgb, mask, stats)] after each of the case's two steps on the device: the first from the case's reference (or from an empty
    slot), the second from the first one's output"""
    import eppm_amd
    from eppm_amd._lib import lib
    di = eppm_amd.Deinterlacer(None, size=(c["h"], c["w"]), slots=slots, **c["params"])
    out, planes = [], []
    try:
        if not c["empty"]:
            di.set_state(slot, c["ref"])
        for k, s in enumerate(c["steps"]):
            p = step_planes(c, s)
            planes += p
            di.step_frames(slot, p[0].value, p[1].value, (c["w"] + c.get("pad", 0)) * 4, p[2].value, p[3].value, c["cut"] and k == 0, s["parity"])
            out.append(read(di, slot))
    finally:
        di.close()
        for p in planes:
            lib().eppm_free_device(p)
    return out


def device_bob(field, h, parity, pad=0, stream_form=False):
    """k_deint_bob on caller planes: (the (h, w, 3) frame, its alpha bytes, the bytes beyond the rows).  The output plane starts as 0xEE."""
    from eppm_amd._lib import check, lib
    fh, w, _ = field.shape
    d_field = to_device(rgba(field, pad=pad))
    out = np.full((h, w + pad, 4), 0xEE, np.uint8)
    d_out = to_device(out)
    try:
        pitch = (w + pad) * 4
        if stream_form:
            check(lib().eppm_deint_bob_stream(d_out, pitch, d_field, pitch, h, w, parity, None), "eppm_deint_bob_stream")
        else:
            check(lib().eppm_deint_bob(d_out, pitch, d_field, pitch, h, w, parity), "eppm_deint_bob")
        check(lib().eppm_device_synchronize(), "eppm_device_synchronize")
        check(lib().eppm_memcpy_d2h(out.ctypes.data_as(C.c_void_p), d_out, C.c_size_t(out.nbytes)), "d2h")
    finally:
        lib().eppm_free_device(d_field)
        lib().eppm_free_device(d_out)
    return out[:, :w, :3], out[:, :w, 3], out[:, w:]


def mismatches(cases):
    from test_deint_cpu import np_bob, np_step, run_case, same
    bad = []
    for c in cases:
        want = run_case(c, np_step)
        for k, got in enumerate(device_steps(c)):
            if not same(got, want[k]):
                bad.append((c["name"], k, int((got[0] != want[k][0]).sum()), int((got[1] != want[k][1]).sum()), got[2], want[k][2]))
        s = c["steps"][0]
        field = s["cur"][s["parity"]::2]
        rgb, alpha, beyond = device_bob(field, c["h"], s["parity"], pad=c.get("pad", 0), stream_form=bool(s["parity"]))
        if not (np.array_equal(rgb, np_bob(field, c["h"], s["parity"])) and (alpha == 0).all() and (beyond == 0xEE).all()):
            bad.append((c["name"], "bob"))
    return bad


def main():
    from test_deint_cpu import deint_cases, deint_limit_cases        # (imports conftest, which selects the test library: overridden below)
    import eppm_amd
    eppm_amd.select_library("tol")
    print(eppm_amd.lib().eppm_version().decode())
    cases = deint_cases() + deint_limit_cases()
    bad = mismatches(cases)
    print(f"{len(cases)} cases, {len(bad)} differ from the restatement: {bad[:5]}")
    assert not bad
    print("PART OK")


if __name__ == "__main__":
    main()
