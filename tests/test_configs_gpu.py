"""GPU parity at the sizes of BASELINE.json's configurations, without running the oracle on the GPU box: the oracle's flows
were computed once in the build container (tests/golden/make_golden_large.py) and MANIFEST_large.json keeps their sha256,
per-band hashes, means and a 64x64 crop.  Plus: a fixed-seed fuzz sweep against the live oracle (small sizes), the flow
colour coding, the reference's own main.cpp on the drop-in boundary, and bench.py's self-spawned ranks."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _manifest():
    return json.load(open(os.path.join(GOLDEN, "MANIFEST_large.json")))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _check_flow(name, u, v, rec, crops):
    """HIP flow against the committed oracle record: crop first (readable failure), then band hashes, then the full hash."""
    cy, cx = rec["crop_origin_yx"]
    cu, cv = crops[name + "_u"], crops[name + "_v"]
    du = np.abs(u[cy:cy + 64, cx:cx + 64] - cu).max()
    dv = np.abs(v[cy:cy + 64, cx:cx + 64] - cv).max()
    assert du == 0 and dv == 0, f"{name}: centre crop differs from the oracle's (max |du| {du}, |dv| {dv})"
    bands = [hashlib.sha256(u[y:y + 16].tobytes() + v[y:y + 16].tobytes()).hexdigest()[:16] for y in range(0, u.shape[0], 16)]
    badb = [i for i, (a, b) in enumerate(zip(bands, rec["band_sha256"])) if a != b]
    assert not badb, f"{name}: {len(badb)} of {len(bands)} 16-row bands differ from the oracle's, first at rows {badb[0] * 16}.."
    assert hashlib.sha256(u.tobytes() + v.tobytes()).hexdigest() == rec["flow_sha256"], name


def _pair(rec):
    from eppm_amd import synth
    a, b, _, _ = synth.make_pair(rec["h"], rec["w"], seed=rec["seed"], max_flow=rec["max_flow"])
    assert _sha(a) == rec["img1_sha256"] and _sha(b) == rec["img2_sha256"], \
        "the synthetic pair generated on this host differs from the one the golden flow was computed on (numpy/libm difference)"
    return a, b


def _run_case(name):
    import eppm_amd
    rec = _manifest()[name]
    crops = np.load(os.path.join(GOLDEN, "large_crops.npz"))
    a, b = _pair(rec)
    e = eppm_amd.EPPM(params=eppm_amd.Params(patch_r=rec["patch_r"]))
    e.init(a, b, rec["h"], rec["w"])
    u, v = e.compute_flow()
    e.close()
    _check_flow(name, u, v, rec, crops)


def test_config2_sintel_shape_pair_bit_exact():
    """BASELINE configs[1]: one 1024x436 pair (seed 1234), full pyramid: HIP flow == oracle flow, bit for bit."""
    _run_case("sintel_1234")


def test_config3_eight_pairs_per_gpu_pipelined():
    """BASELINE configs[2]: the 8 pairs one GPU of the 64-pair / 8-GPU batch processes (seeds 1234..1241), through three
    contexts kept in flight (eppm_amd.shard.run_pairs_pipelined, the sharded runner's per-GPU loop): every flow == oracle's."""
    import eppm_amd
    from eppm_amd import shard
    man = _manifest()
    crops = np.load(os.path.join(GOLDEN, "large_crops.npz"))
    names = [f"sintel_{s}" for s in range(1234, 1242)]
    pairs = [_pair(man[n]) for n in names]
    engs = []
    for _ in range(3):
        e = eppm_amd.EPPM()
        e.init(436, 1024)
        engs.append(e)
    mine = shard.pairs_for_rank(8, 0, 1)
    out = shard.run_pairs_pipelined(engs, pairs, mine)
    assert sorted(out) == list(range(8))
    for i, n in enumerate(names):
        _check_flow(n, out[i][0], out[i][1], man[n], crops)


def test_config3_eight_pairs_in_one_batch_context():
    """BASELINE configs[2] through the batch context (eppm_create_batch): the same 8 pairs share EVERY kernel launch
    (blockIdx.z / .y = pair); each flow == the oracle's, i.e. == what a single-pair context computes.  Then a partial batch
    (3 active pairs of 8) and the single-pair entry points on the same batch context."""
    import eppm_amd
    man = _manifest()
    crops = np.load(os.path.join(GOLDEN, "large_crops.npz"))
    names = [f"sintel_{s}" for s in range(1234, 1242)]
    pairs = [_pair(man[n]) for n in names]
    B = eppm_amd.EPPMBatch(436, 1024, 8)
    B.set_data(pairs)
    out = B.compute_flow()
    assert len(out) == 8
    for n, (u, v) in zip(names, out):
        _check_flow(n, u, v, man[n], crops)
    from eppm_amd import shard
    again = shard.run_pairs_batched(B, pairs, [6, 1])     # the sharded runner's batched form
    for i in (6, 1):
        _check_flow(names[i], again[i][0], again[i][1], man[names[i]], crops)
    B.set_data(pairs)
    B.compute_flow()
    nnf3 = B.plane(3, "nnf1", 2)
    B.set_data([pairs[5], pairs[0], pairs[3]])          # partial batch, other order
    out = B.compute_flow()
    assert len(out) == 3
    for n, (u, v) in zip([names[5], names[0], names[3]], out):
        _check_flow(n, u, v, man[n], crops)
    assert np.array_equal(B.plane(2, "nnf1", 2).view(np.uint8), nnf3.view(np.uint8))      # pair 3's NNF, now in slot 2
    B.close()


def test_batch_context_small_sizes_against_oracle(crop, crop_stages):
    """Batch contexts at small sizes and other parameters (split level-1 refine at n = 1 but not at n = 5, R = 17, jump flood,
    odd sizes): every pair of the batch == the live oracle."""
    import eppm_amd
    from oracle import oracle as O
    a, b = crop
    st = crop_stages
    B = eppm_amd.EPPMBatch(120, 160, 5)
    B.set_data([(a, b), (b, a), (a, a), (a, b), (b, a)])
    out = B.compute_flow()
    want = {0: (st["u"], st["v"]), 3: (st["u"], st["v"])}
    want[1] = want[4] = O.compute_flow(b, a)
    want[2] = O.compute_flow(a, a)
    for k, (u, v) in enumerate(out):
        assert np.array_equal(u.view(np.uint32), want[k][0].view(np.uint32)) and np.array_equal(v.view(np.uint32), want[k][1].view(np.uint32)), k
    B.close()
    for params, (h, w) in ((dict(patch_r=17), (96, 128)), (dict(propagation=1, num_iter=3), (77, 101)), (dict(patch_r=5, levels=2, propagation=2, num_iter=2), (64, 90))):
        pa, pb = a[:h, :w].copy(), b[:h, :w].copy()
        B = eppm_amd.EPPMBatch(h, w, 3, params=eppm_amd.Params(**params))
        B.set_data([(pa, pb), (pb, pa), (pa, pb)])
        out = B.compute_flow()
        w0 = O.compute_flow(pa, pb, O.default_params(**params))
        w1 = O.compute_flow(pb, pa, O.default_params(**params))
        for k, wk in enumerate((w0, w1, w0)):
            assert np.array_equal(out[k][0].view(np.uint32), wk[0].view(np.uint32)) and np.array_equal(out[k][1].view(np.uint32), wk[1].view(np.uint32)), (params, k)
        B.close()


def test_batch_device_entry_points_and_begin_end(crop, crop_stages):
    """eppm_batch_set_images_device / eppm_batch_compute_device (device-resident RGBA in, float2 flows left in HBM) and the
    two-halves form eppm_compute_begin / eppm_batch_compute_end on a batch context: same flows as the host-pointer calls."""
    import eppm_amd
    from eppm_amd import stages as S
    from oracle import oracle as O
    a, b = crop
    st = crop_stages
    h, w = 120, 160
    ra, rb = O.rgb2rgba(a), O.rgb2rgba(b)
    d = [S.Dev(ra, pitched=True), S.Dev(rb, pitched=True)]
    outs = [S.Dev(shape=(h, w), dtype=eppm_amd.api.float2) for _ in range(3)]
    B = eppm_amd.EPPMBatch(h, w, 3)
    B.set_data_device([d[0].ptr.value, d[1].ptr.value, d[0].ptr.value], [d[1].ptr.value, d[0].ptr.value, d[1].ptr.value], d[0].pitch)
    B.compute_flow_device([o.ptr.value for o in outs])
    B.synchronize()
    rev = O.compute_flow(b, a)
    for k, want in enumerate(((st["u"], st["v"]), rev, (st["u"], st["v"]))):
        f = outs[k].get()
        assert np.array_equal(f["x"].copy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(f["y"].copy().view(np.uint32), want[1].view(np.uint32)), k
    B.set_data([(b, a), (a, b)])
    B.compute_flow_begin()
    got = B.compute_flow_end()
    assert len(got) == 2
    for (u, v), want in zip(got, (rev, (st["u"], st["v"]))):
        assert np.array_equal(u.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(v.view(np.uint32), want[1].view(np.uint32))
    with pytest.raises(eppm_amd.EppmError):
        B.compute_flow_end()                                # end without begin
    B.close()


def test_host_boundary_registered_buffers_and_begin_into(crop, crop_stages):
    """a2 / a19 without staging copies: images in memory registered with eppm_host_register (or from eppm_host_alloc) are read
    by DMA where they lie, flow planes in registered memory are written directly (eppm_compute, eppm_compute_begin_into,
    eppm_batch_compute_begin_into); mixed registered / unregistered arguments, strided rows and a destination that changes
    between begin and end all give the flows of the plain staged calls, bit for bit."""
    import eppm_amd
    from oracle import oracle as O
    a, b = crop
    st = crop_stages
    h, w = 120, 160
    want = (st["u"], st["v"])
    rev = O.compute_flow(b, a)

    def same(got, ref):
        return np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
    L = eppm_amd.lib()
    pa, pb = eppm_amd.pinned_empty((h, w, 3)), eppm_amd.pinned_empty((h, w, 3))          # eppm_host_alloc
    pa[:], pb[:] = a, b
    ra = eppm_amd.host_register(a.copy())                                                 # eppm_host_register on malloc'ed memory
    u, v = eppm_amd.host_register(np.full((h, w), -7, np.float32)), eppm_amd.host_register(np.full((h, w), -7, np.float32))
    import ctypes as C

    def is_reg(x):
        return L.eppm_host_is_registered(C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes))
    assert is_reg(pa) == 1 and is_reg(ra) == 1 and is_reg(u) == 1 and is_reg(b) == 0
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_data(pa, pb)
    assert same(e.compute_flow(out=(u, v)), want), "registered in, registered out"
    e.set_data(ra, b)                                   # one registered, one staged
    assert same(e.compute_flow(), want), "mixed in, staged out"
    pa[:] = 0                                            # set_data has consumed the images when it returns
    e.set_data(pb, ra)
    ra[:] = 0
    uu = np.empty((h, w), np.float32)
    assert same(e.compute_flow(out=(uu, v)), rev), "registered in (reused right after the call), one registered plane out"
    pa[:], ra[:] = a, a
    # strided rows inside a registered block
    wide = eppm_amd.pinned_empty((h, w + 13, 3))
    wide2 = eppm_amd.pinned_empty((h, w + 13, 3))
    wide[:, :w], wide2[:, :w] = a, b
    from eppm_amd._lib import check
    check(L.eppm_set_images(e._ctx, C.c_void_p(wide.ctypes.data), C.c_void_p(wide2.ctypes.data), C.c_size_t((w + 13) * 3)), "strided")
    assert same(e.compute_flow(), want), "strided registered rows"
    # begin_into + end: same pointers (only waits), other pointers (copied from the direct destination), begin without destination
    e.set_data(pa, pb)
    e.compute_flow_begin(out=(u, v))
    got = e.compute_flow_end(out=(u, v))
    assert got[0] is u and same(got, want)
    e.set_data(pb, pa)
    e.compute_flow_begin(out=(u, v))
    other = e.compute_flow_end()                          # fresh unregistered planes
    assert same(other, rev) and same((u, v), rev)
    e.set_data(pa, pb)
    e.compute_flow_begin()
    assert same(e.compute_flow_end(out=(u, v)), want)
    e.close()
    # batch context: registered and unregistered destinations in one call
    B = eppm_amd.EPPMBatch(h, w, 3)
    B.set_data([(pa, pb), (b, a), (ra, pb)])
    outs = [(u, v), (np.empty((h, w), np.float32), np.empty((h, w), np.float32)),
            (eppm_amd.pinned_empty((h, w), np.float32), eppm_amd.pinned_empty((h, w), np.float32))]
    B.compute_flow_begin(out=outs)
    got = B.compute_flow_end(out=outs)
    for k, ref in enumerate((want, rev, want)):
        assert same(got[k], ref), k
    got = B.compute_flow(out=outs[::-1])
    for k, ref in enumerate((want, rev, want)):
        assert same(got[k], ref), k
    B.close()
    for x in (ra, u, v):
        eppm_amd.host_unregister(x)
    with pytest.raises(eppm_amd.EppmError):
        eppm_amd.host_unregister(u)                       # twice


def test_class_pinned_caller_buffers_cli(tmp_path):
    """The drop-in class with set_option("pin_caller_buffers", 1) (runeppm --pin): bao_alloc-shaped blocks registered for DMA,
    no host copies; the .flo equals the default class's byte for byte, and the steady-state loop reproduces it (the CLI
    compares every repetition with the first flow)."""
    exe = os.path.join(ROOT, "eppm_amd", "lib", "runeppm")
    outs = []
    for extra in ([], ["--pin"]):
        o = str(tmp_path / ("flow%d.flo" % len(outs)))
        r = subprocess.run([exe, "--size", "320x200", "--pairs", "5", "--out", o] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(o, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) == 12 + 320 * 200 * 8


@pytest.mark.parametrize("mode", ["", "--pin", "--trust"])
def test_class_reads_through_rewritten_pointer_tables(tmp_path, mode):
    """The reference indexes its images through the row-pointer tables on every call (basic/bao_basic_cuda.h:258-267).  The class reads a
    bao_alloc-shaped table as one block only after checking EVERY pixel pointer, on every call (for a table seen before: while the
    device already works, redoing the call through the pointers when the walk fails).  tests/csrc/class_tables.cpp rewrites the interior
    pointers of a table between two calls, row ends untouched: the flow must be that of the image the pointers describe -- with plain
    and with pinned caller buffers; the opt-in trust cache ("trust_verified_tables") is the documented exception."""
    exe = str(tmp_path / "class_tables")
    libdir = os.path.join(ROOT, "eppm_amd", "lib")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "class_tables.cpp"), "-o", exe,
                           "-L", libdir, "-leppm_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe] + ([mode] if mode else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("OK"), r.stdout + r.stderr


def test_class_pinned_blocks_shared_by_two_workers(tmp_path):
    """runeppm --gpus 2 --pin on one GPU: two objects on two host threads register the SAME image blocks (registrations are counted:
    the worker that finishes first must not unpin the pages under the other's DMA reads) and their own flow planes; every
    repetition of every worker reproduces the first flow, and it equals the unpinned single-worker flow byte for byte."""
    exe = os.path.join(ROOT, "eppm_amd", "lib", "runeppm")
    outs = []
    for extra in ([], ["--pin", "--gpus", "2"], ["--pin", "--gpus", "3", "--pairs", "31"]):
        o = str(tmp_path / ("flow%d.flo" % len(outs)))
        r = subprocess.run([exe, "--size", "320x200", "--pairs", "24", "--out", o] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(open(o, "rb").read())
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == 12 + 320 * 200 * 8


def test_unregister_under_a_pending_transfer_fails_instead_of_unpinning():
    """eppm_compute_begin_into has the copy engine write registered planes until eppm_compute_end: unregistering them in between must
    not unpin the pages under the transfer -- the call waits (bounded) and fails with EPPM_ERR_STATE, the registration stands, and after
    eppm_compute_end it succeeds."""
    import ctypes as C
    import eppm_amd
    from eppm_amd import synth
    L = eppm_amd.lib()
    h, w = 96, 128
    a, b, _, _ = synth.make_pair(h, w, seed=4, max_flow=5.0)
    uv = np.zeros((2, h, w), np.float32)
    p = C.c_void_p(uv.ctypes.data)
    assert L.eppm_host_register(p, C.c_size_t(uv.nbytes)) == 0
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    want = e.compute_flow()
    e.compute_flow_begin(out=(uv[0], uv[1]))
    assert L.eppm_host_unregister(p) == 3 and b"in flight" in L.eppm_last_error()          # EPPM_ERR_STATE
    assert L.eppm_host_is_registered(p, C.c_size_t(uv.nbytes)) == 1
    u, v = e.compute_flow_end(out=(uv[0], uv[1]))
    assert L.eppm_host_unregister(p) == 0 and L.eppm_host_is_registered(p, C.c_size_t(uv.nbytes)) == 0
    e.close()
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1])


def test_last_owner_leaving_meets_a_new_owner_arriving():
    """The window inside eppm_host_unregister: the LAST owner waits (lock dropped) for a transfer in flight on the block, and meanwhile
    another thread registers the same block.  The new owner must keep the pinning: the waiter, once the transfer is over, returns OK
    WITHOUT unpinning, the block stays registered, transfers into it stay direct, and the new owner's own unregister succeeds and unpins.
    (Before round 5 the waiter erased the block and unpinned it under the new owner, whose unregister then failed: ADVICE r4.)"""
    import ctypes as C
    import threading
    import time
    import eppm_amd
    from eppm_amd import synth
    L = eppm_amd.lib()
    h, w = 96, 128
    a, b, _, _ = synth.make_pair(h, w, seed=4, max_flow=5.0)
    uv = np.zeros((2, h, w), np.float32)
    p, n = C.c_void_p(uv.ctypes.data), C.c_size_t(uv.nbytes)
    assert L.eppm_host_register(p, n) == 0                                   # owner A
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    want = e.compute_flow()
    e.compute_flow_begin(out=(uv[0], uv[1]))                                  # a transfer in flight on the block
    res = {}
    t = threading.Thread(target=lambda: res.update(rc=L.eppm_host_unregister(p)))   # A leaves: last owner, waits for the transfer
    t.start()
    time.sleep(0.3)
    assert t.is_alive()                                                      # (waiting: bounded at 5 s)
    assert L.eppm_host_is_registered(p, n) == 0                              # closing: no NEW transfer starts on it ...
    assert L.eppm_host_register(p, n) == 0                                   # ... until owner B arrives and keeps it
    assert L.eppm_host_is_registered(p, n) == 1
    u, v = e.compute_flow_end(out=(uv[0], uv[1]))                             # the transfer ends; the waiter wakes up
    t.join(timeout=10)
    assert not t.is_alive() and res["rc"] == 0, res
    assert L.eppm_host_is_registered(p, n) == 1                              # B's registration stands
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1])
    uv[:] = 0
    e.compute_flow_begin(out=(uv[0], uv[1]))                                  # still written in place by the copy engine
    u2, v2 = e.compute_flow_end(out=(uv[0], uv[1]))
    assert np.array_equal(uv[0], want[0]) and np.array_equal(uv[1], want[1]) and u2 is not None and v2 is not None
    assert L.eppm_host_unregister(p) == 0 and L.eppm_host_is_registered(p, n) == 0     # B leaves: unpinned now
    assert L.eppm_host_unregister(p) != 0
    e.close()


def test_unregister_through_an_inner_pointer_can_be_retried_after_a_timeout():
    """A range registered INSIDE a registered block is an owner of that block, found through an alias entry.  When it is the last owner
    and its unregister times out under a pending transfer (EPPM_ERR_STATE), the SAME pointer must still name the block afterwards:
    the retry after eppm_compute_end succeeds.  (Before round 5 the alias entry was erased before the wait: 'not a block'.)"""
    import ctypes as C
    import eppm_amd
    from eppm_amd import synth
    L = eppm_amd.lib()
    h, w = 96, 128
    a, b, _, _ = synth.make_pair(h, w, seed=4, max_flow=5.0)
    uv = np.zeros((2, h, w), np.float32)
    p, n = C.c_void_p(uv.ctypes.data), C.c_size_t(uv.nbytes)
    inner, ni = C.c_void_p(uv[1].ctypes.data), C.c_size_t(uv[1].nbytes)
    assert L.eppm_host_register(p, n) == 0 and L.eppm_host_register(inner, ni) == 0      # two owners; the second through an alias
    assert L.eppm_host_unregister(p) == 0 and L.eppm_host_is_registered(p, n) == 1       # the alias owner is the last one now
    e = eppm_amd.EPPM()
    e.init(a, b, h, w)
    e.compute_flow_begin(out=(uv[0], uv[1]))
    assert L.eppm_host_unregister(inner) == 3 and b"in flight" in L.eppm_last_error()    # EPPM_ERR_STATE after the bounded wait
    assert L.eppm_host_is_registered(p, n) == 1
    e.compute_flow_end(out=(uv[0], uv[1]))
    assert L.eppm_host_unregister(inner) == 0 and L.eppm_host_is_registered(p, n) == 0  # the retry, same pointer
    e.close()


def test_host_registration_is_counted():
    """eppm_host_register twice on one block (and once on a range inside it) = three owners: the block stays registered until the
    third eppm_host_unregister; a context computing into it in between is unaffected."""
    import ctypes as C
    import eppm_amd
    from eppm_amd import synth
    L = eppm_amd.lib()
    h, w = 96, 128
    a, b, _, _ = synth.make_pair(h, w, seed=3, max_flow=5.0)
    blk = np.zeros((2, h, w, 3), np.uint8)
    blk[0], blk[1] = a, b
    p = C.c_void_p(blk.ctypes.data)
    inner = C.c_void_p(blk[1].ctypes.data)
    assert L.eppm_host_register(p, C.c_size_t(blk.nbytes)) == 0
    assert L.eppm_host_register(p, C.c_size_t(blk.nbytes)) == 0
    assert L.eppm_host_register(inner, C.c_size_t(blk[1].nbytes)) == 0
    e = eppm_amd.EPPM()
    e.init(h, w)
    e.set_data(blk[0], blk[1])
    u0, v0 = e.compute_flow()
    assert L.eppm_host_unregister(p) == 0 and L.eppm_host_is_registered(p, C.c_size_t(blk.nbytes)) == 1
    assert L.eppm_host_unregister(inner) == 0 and L.eppm_host_is_registered(inner, C.c_size_t(blk[1].nbytes)) == 1
    e.set_data(blk[0], blk[1])
    u1, v1 = e.compute_flow()
    assert L.eppm_host_unregister(p) == 0 and L.eppm_host_is_registered(p, C.c_size_t(blk.nbytes)) == 0
    assert L.eppm_host_unregister(p) != 0                       # no owner left
    q = eppm_amd.pinned_empty((64,), np.uint8)                  # eppm_host_alloc memory counts as registered; a registration on top is one more owner
    qp = C.c_void_p(q.ctypes.data)
    assert L.eppm_host_register(qp, C.c_size_t(64)) == 0 and L.eppm_host_unregister(qp) == 0
    assert L.eppm_host_unregister(qp) != 0 and L.eppm_host_is_registered(qp, C.c_size_t(64)) == 1      # the allocation itself goes with eppm_host_free
    e.set_data(blk[0], blk[1])                                  # through the staging buffers now
    u2, v2 = e.compute_flow()
    e.close()
    assert np.array_equal(u0, u1) and np.array_equal(v0, v1) and np.array_equal(u0, u2) and np.array_equal(v0, v2)


def test_config1_single_scale_full_size(frames):
    """BASELINE configs[0] reads "single scale": levels = 1 (PYR_MAX_DEPTH 1: PatchMatch, post-processing and the final
    smoothing all at full resolution, no coarse-to-fine step) on the whole 640x480 bundled pair with default parameters,
    against the live oracle (about 40 s on 16 threads)."""
    import eppm_amd
    from oracle import oracle as O
    a, b = frames
    e = eppm_amd.EPPM(params=eppm_amd.Params(levels=1))
    e.init(a, b, 480, 640)
    u, v = e.compute_flow()
    e.close()
    ou, ov = O.compute_flow(a, b, O.default_params(levels=1))
    assert np.array_equal(u.view(np.uint32), ou.view(np.uint32)) and np.array_equal(v.view(np.uint32), ov.view(np.uint32))


def test_config4_hd_pair_bit_exact():
    """BASELINE configs[3]: 1920x1080, full pyramid + bilateral refine (the non-split tiled refine with many tiles, XCD tile
    order, two-pixel-per-lane smoothing)."""
    _run_case("hd_1234")


def test_config5_uhd_patch_radius_17_bit_exact():
    """BASELINE configs[4]: 3840x2160, PATCH_R 17, 10 PatchMatch iterations (64-lane sweeps, R=17 search and refine, 32-bit texel offsets)."""
    _run_case("uhd_r17_1234")


# ---------------------------------------------------------------------------------------------------
# fixed-seed fuzz sweep: random sizes, parameters and image statistics; HIP == live oracle (small sizes: seconds)
# ---------------------------------------------------------------------------------------------------
def _fuzz_case(seed, t):
    from eppm_amd import synth
    rng = np.random.default_rng([seed, t])
    h, w = int(rng.integers(16, 200)), int(rng.integers(16, 260))
    kind = t % 4
    if kind == 0:
        a, b, _, _ = synth.make_pair(h, w, seed=int(rng.integers(1 << 30)), max_flow=float(rng.uniform(1, 30)))
    elif kind == 1:   # pure noise, unrelated images
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == 2:   # flat regions + saturated blocks
        a = np.zeros((h, w, 3), np.uint8)
        a[h // 3:, w // 4:] = 255
        a[: h // 2, : w // 2, 1] = 128
        b = np.roll(a, (int(rng.integers(-9, 9)), int(rng.integers(-9, 9))), axis=(0, 1))
    else:             # low contrast
        base = rng.integers(100, 110, (h, w, 3)).astype(np.uint8)
        a, b = base, np.roll(base, 3, axis=1)
    params = dict(patch_r=int(rng.choice([9, 9, 9, 17, 5, 4])), num_iter=int(rng.integers(1, 5)), num_guess=int(rng.integers(1, 9)),
                  seg_len=int(rng.integers(2, 14)), wmf_iters=int(rng.integers(0, 6)), search_range=int(rng.integers(1, 40)),
                  seed=int(rng.integers(1, 1 << 40)), propagation=int(rng.integers(0, 3)), levels=int(rng.integers(1, 5)))
    return a, b, params


FUZZ_SEEDS = [11, 12, 13, 14, 15, 16, 17, 18]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_parity_fixed_seeds(seed):
    import eppm_amd
    from oracle import oracle as O
    for t in range(8):
        a, b, params = _fuzz_case(seed, t)
        h, w, _ = a.shape
        e = eppm_amd.EPPM(params=eppm_amd.Params(**params))
        e.init(a, b, h, w)
        u, v = e.compute_flow()
        e.close()
        ou, ov = O.compute_flow(a, b, O.default_params(**params))
        same = np.array_equal(u.view(np.uint32), ou.view(np.uint32)) and np.array_equal(v.view(np.uint32), ov.view(np.uint32))
        assert same, f"fuzz seed {seed} case {t}: {w}x{h} {params}"


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_parity_window_kernels_at_small_sizes(seed):
    """The fuzz sweep again with the test switch "c2f_no_split" (eppm_test_set_option): the candidate refine of small images then
    runs the LDS-window kernels (k_c2f_refine_win / _win4) instead of the split gather kernel they normally get, at ragged
    sizes, radii 9 and 17, every propagation mode and pyramid depth."""
    import eppm_amd
    assert eppm_amd.lib().eppm_test_set_option(b"c2f_no_split", 1) == 0
    try:
        test_fuzz_parity_fixed_seeds(seed)
    finally:
        eppm_amd.lib().eppm_test_set_option(b"c2f_no_split", 0)


# ---------------------------------------------------------------------------------------------------
# live oracle at BASELINE's full sizes (the oracle takes 2.5 s at 1024x436 and ~13 s at 1920x1080 on 16 threads): pairs that
# are in no committed fixture, other image statistics than the fixtures', single-pair and batch contexts
# ---------------------------------------------------------------------------------------------------
def _same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _full_size_pairs():
    from eppm_amd import synth
    h, w = 436, 1024
    rng = np.random.default_rng(20260)
    pairs = {}
    pairs["synth_4321_flow40"] = synth.make_pair(h, w, seed=4321, max_flow=40.0)[:2]           # flows beyond the search range
    pairs["synth_4322_flow3"] = synth.make_pair(h, w, seed=4322, max_flow=3.0)[:2]              # near-static
    n1, n2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pairs["noise_unrelated"] = (n1, n2)                                                           # incoherent matches everywhere: refine fallback path
    flat = np.full((h, w, 3), 117, np.uint8)
    flat[100:300, 200:700] = (250, 3, 90)
    pairs["flat_with_block"] = (flat, np.roll(flat, (7, -11), axis=(0, 1)))                       # zero weights' complement: constant patches
    return pairs


@pytest.mark.parametrize("name", ["synth_4321_flow40", "synth_4322_flow3", "noise_unrelated", "flat_with_block"])
def test_config2_full_size_against_live_oracle(name):
    """1024x436 (BASELINE configs[1]) against the oracle run live on the same inputs: large and tiny flows, unrelated noise images,
    flat images -- none of them in the committed fixtures."""
    import eppm_amd
    from oracle import oracle as O
    a, b = _full_size_pairs()[name]
    e = eppm_amd.EPPM()
    e.init(a, b, 436, 1024)
    got = e.compute_flow()
    e.close()
    assert _same(got, O.compute_flow(a, b)), name


def test_config3_batch_of_mixed_pairs_against_live_oracle():
    """The four pairs above in ONE batch context (every launch covers all four: coherent and incoherent tiles, flat and textured
    images side by side) == four live oracle runs."""
    import eppm_amd
    from oracle import oracle as O
    pairs = list(_full_size_pairs().values())
    B = eppm_amd.EPPMBatch(436, 1024, 4)
    B.set_data(pairs)
    out = B.compute_flow()
    B.close()
    for k, (a, b) in enumerate(pairs):
        assert _same(out[k], O.compute_flow(a, b)), k


def test_config4_hd_against_live_oracle():
    """1920x1080 (BASELINE configs[3]) on a pair that is in no fixture, against the live oracle."""
    import eppm_amd
    from eppm_amd import synth
    from oracle import oracle as O
    a, b = synth.make_pair(1080, 1920, seed=777, max_flow=25.0)[:2]
    e = eppm_amd.EPPM()
    e.init(a, b, 1080, 1920)
    got = e.compute_flow()
    e.close()
    assert _same(got, O.compute_flow(a, b))


def test_bundled_pair_both_directions_and_odd_crops(frames):
    """The reference's bundled Middlebury pair: backward direction at full size, and crops at odd offsets / ragged sizes."""
    import eppm_amd
    from oracle import oracle as O
    a, b = frames
    for (y0, x0, h, w) in ((0, 0, 480, 640), (3, 5, 431, 577), (100, 37, 255, 333)):
        pa, pb = b[y0:y0 + h, x0:x0 + w].copy(), a[y0:y0 + h, x0:x0 + w].copy()       # frame11 -> frame10
        e = eppm_amd.EPPM()
        e.init(pa, pb, h, w)
        got = e.compute_flow()
        e.close()
        assert _same(got, O.compute_flow(pa, pb)), (y0, x0, h, w)


def test_soak_contexts_in_flight_are_deterministic():
    """Race hunt: three single-pair contexts and one 4-pair batch context kept in flight together (begin/end, each on its own
    stream, kernels of all four interleaving on the GPU) for 40 rounds at 1024x436 -- every flow of every round must hash like the
    first one of its pair, which is compared with the live oracle."""
    import hashlib
    import eppm_amd
    from eppm_amd import synth
    from oracle import oracle as O
    h, w = 436, 1024
    pairs = [synth.make_pair(h, w, seed=9000 + i)[:2] for i in range(4)]
    engs = []
    for i in range(3):
        e = eppm_amd.EPPM()
        e.init(h, w)
        engs.append(e)
    B = eppm_amd.EPPMBatch(h, w, 4)
    digest = lambda uv: hashlib.sha256(uv[0].tobytes() + uv[1].tobytes()).hexdigest()
    first = {}
    for rnd in range(40):
        for k, e in enumerate(engs):
            e.set_data(*pairs[(rnd + k) % 4])
            e.compute_flow_begin()
        B.set_data([pairs[(rnd + j) % 4] for j in range(4)])
        B.compute_flow_begin()
        got = [((rnd + k) % 4, e.compute_flow_end()) for k, e in enumerate(engs)]
        got += [((rnd + j) % 4, uv) for j, uv in enumerate(B.compute_flow_end())]
        for i, uv in got:
            d = digest(uv)
            if i not in first:
                first[i] = d
                assert _same(uv, O.compute_flow(*pairs[i])), i
            assert d == first[i], (rnd, i)
    for e in engs:
        e.close()
    B.close()


# ---------------------------------------------------------------------------------------------------
# n4: flow colour coding on the device
# ---------------------------------------------------------------------------------------------------
def test_flow_color_kernel_bytes(crop, crop_stages):
    """k_flow_to_color == orc_flow_to_color byte for byte: random vectors (inside and beyond the radius), the validity
    threshold, signed zeros and axis-aligned vectors (the atan2 quadrant edges), and the flow of the bundled crop."""
    from eppm_amd import stages as S
    from oracle import oracle as O
    rng = np.random.default_rng(9)
    h, w = 96, 160
    f = np.zeros((h, w), O.float2)
    f["x"] = (rng.standard_normal((h, w)) * 25).astype(np.float32)
    f["y"] = (rng.standard_normal((h, w)) * 25).astype(np.float32)
    edge = np.array([0.0, -0.0, 1e10, -1e10, 999999.0, -999999.0, 999998.94, 28.284271, -28.284271, 20.0, -20.0, 1e-30, -1e-30, 5.0], np.float32)
    k = 0
    for ex in edge:
        for ey in edge:
            f["x"].flat[k], f["y"].flat[k] = ex, ey
            k += 1
    for md in ((20.0, 20.0), (100.0, 100.0), (3.0, 50.0)):
        got, want = S.flow_to_color(f, *md), O.flow_to_color(f, *md)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    # the class path: eppm_compute_color on the context's own flow (driver .cpp:308-314)
    import eppm_amd
    e = eppm_amd.EPPM()
    e.init(crop[0], crop[1], 120, 160)
    u, v = e.compute_flow()
    rgb = e.compute_flow_color()
    ff = np.zeros((120, 160), O.float2)
    ff["x"], ff["y"] = u, v
    want = O.flow_to_color(ff, 20, 20)
    assert np.array_equal(rgb, np.stack([want["x"], want["y"], want["z"]], -1))
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 8          # a real colour image, not a constant


# ---------------------------------------------------------------------------------------------------
# boundary: the reference's own main.cpp, unmodified, on include/ + libeppm_hip.so
# ---------------------------------------------------------------------------------------------------
def test_reference_main_cpp_unmodified_writes_the_same_flo(tmp_path):
    """oracle/_ref/runeppm_ref (reference main.cpp compiled unmodified, oracle/Makefile) run where frame10/11.ppm lie:
    its flow.flo equals, byte for byte, the one tools/runeppm writes through the same drop-in class."""
    import shutil
    import eppm_amd
    from oracle import oracle as O
    exe = O.runeppm_ref()
    assert exe is not None, "oracle/_ref/runeppm_ref was not built (it travels with the snapshot; build() makes it when /root/reference is present)"
    for n in ("frame10.ppm", "frame11.ppm"):
        shutil.copy(os.path.join(GOLDEN, n), tmp_path / n)
    txt = subprocess.check_output([exe], cwd=tmp_path, text=True, timeout=300)
    assert "Running time (GPU)" in txt and "Saving flo file" in txt, txt          # bao_timer_gpu_cpu::time_display, main.cpp:66-68
    ours = os.path.join(os.path.dirname(eppm_amd.lib_path()), "runeppm")
    subprocess.check_call([ours, os.path.join(GOLDEN, "frame10.ppm"), os.path.join(GOLDEN, "frame11.ppm"), str(tmp_path / "ours.flo")])
    assert open(tmp_path / "flow.flo", "rb").read() == open(tmp_path / "ours.flo", "rb").read()
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    fu, fv = eppm_amd.io.load_flo(str(tmp_path / "flow.flo"))
    assert hashlib.sha256(fu.tobytes() + fv.tobytes()).hexdigest() == man["oracle_flow_640x480_sha256"]


# ---------------------------------------------------------------------------------------------------
# bench.py --gpus N without a launcher (two ranks share the one GPU of the test box; gloo for the barrier)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_bench_two_ranks_share_one_gpu(backend):
    """backend nccl: RCCL refuses two ranks on one device, at the first collective -- the probe all-reduce on the RCCL group
    must catch that, the ranks must AGREE on it over the gloo group that always exists, and the barrier and the MAX then go over
    gloo on every rank (the data path has no collective).  The line carries its correctness bits: every flow of the timed region
    and (default at N > 1) every rank's share of the 64 config-3 pairs against the committed oracle hashes."""
    env = dict(os.environ, EPPM_BENCH_SHARE_GPU="1")
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "6", "--warmup", "3", "--dist-backend", backend,
                          "--no-extras", "--no-cpu-baseline"] + (["--no-verify-config3"] if backend == "nccl" else []),
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, out.stdout
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["roofline"]["frac"] > 0 and d["roofline"]["avg_launch_ms"] > 0
    assert ("barrier and MAX go over gloo" in out.stderr) == (backend == "nccl")
    tv = d["timed_region_verified"]                 # 6 steps per rank -> 6 flows per rank, pairs 0..5 and 24..29 of the 64
    assert tv["of"] == 12 and tv["ok"] == 12 and tv["inputs_differ_on_this_host"] == 0 and tv["all_ok"], tv
    if backend == "gloo":
        # BASELINE configs[2] with its correctness bit: the two ranks' shares (pairs 0,2,4,.. and 1,3,5,..) of the 64 pairs, every flow
        # equal to the committed oracle hash (tests/golden/MANIFEST_config3.json); on by default at N > 1
        v = d["config3_verified"]
        assert v["pairs"] == 64 and v["verified_pairs"] == 64 and v["all_ok"] and v["state"] == "verified", v
    else:
        assert "config3_verified" not in d


def test_bench_eight_ranks_share_one_gpu():
    """The rehearsal of the run the driver makes on an 8-GPU node, `python bench.py --gpus 8`, on the one GPU of the test box: eight rank
    processes (spawned by the parent before anything touches the GPU), each with its three 8-pair batch contexts, its own 24 of the 64
    pairs in flight (ranks 3..7 wrap around the 64: (rank * 24 + j) mod 64), its share of the 64 config-3 pairs through the host
    boundary, every rank's synth workers running side by side -- barrier and MAX over gloo.  One JSON line, exit code 0, every flow
    verified, well inside two minutes.  Not exercised here, and not exercisable on one GPU: RCCL between eight devices (the barrier
    falls back to gloo by agreement when it is unusable) and eight PCIe / NUMA paths."""
    import time
    env = dict(os.environ, EPPM_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--steps", "16", "--dist-backend", "gloo", "--no-extras",
                          "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    wall = time.time() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(line) == 1 and line[0].startswith("{"), out.stdout[:2000]          # ONE line on stdout and nothing else
    d = json.loads(line[0])
    assert d["n_gpus"] == 8 and d["steps"] == 16 and d["value"] > 0 and d["scaling"] == "weak"
    tv = d["timed_region_verified"]                 # 16 steps per rank -> 16 flows per rank
    assert tv["of"] == 128 and tv["ok"] == 128 and tv["inputs_differ_on_this_host"] == 0 and tv["all_ok"], tv
    v = d["config3_verified"]
    assert v["pairs"] == 64 and v["verified_pairs"] == 64 and v["all_ok"] and v["state"] == "verified", v
    hb = d["config"]["host_binding"]["ranks"]
    assert len(hb) == 8 and all(r["pci"] == hb[0]["pci"] for r in hb), hb              # eight ranks seen, all on the one device
    assert wall < 120, wall


def test_bench_default_line_is_self_verifying():
    """The whole line of `python bench.py --full` at N = 1: every flow of the timed region hashed against the committed oracle
    flows, the single-pair latency beside ms_per_step, BASELINE configs[3] and [4] as `other_configs` (each checked against its oracle
    hash), roofline + cpu_baseline.  Fewer steps than the default keep the test short; everything else is the default --full path."""
    env = dict(os.environ)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "5", "--repeats", "2"], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    tv = d["timed_region_verified"]
    assert tv["of"] == 20 and tv["ok"] == 20 and tv["all_ok"], tv
    assert 0 < d["ms_per_step"] < d["latency_ms_per_pair"] < 20
    oc = d["other_configs"]
    for key, ctxs in (("bundled", 3), ("natural_1024x436", 3), ("hd", 3), ("uhd_r17", 2)):
        assert "error" not in oc[key], oc[key]
        assert oc[key]["verified"] == dict(oc[key]["verified"], ok=ctxs, of=ctxs, state="verified"), oc[key]
        assert oc[key]["value"] > 0 and oc[key]["ms_per_step"] > 0
    for key in ("bundled", "natural_1024x436"):         # BASELINE configs[0] and a natural pair of the headline shape: the reference's own window too
        assert 0 < oc[key]["ms_per_step"] < oc[key]["latency_ms_per_pair"] < oc[key]["cold_ms"] < 50, oc[key]
        assert oc[key]["cpu_oracle"]["ms_per_pair"] > 100 * oc[key]["latency_ms_per_pair"] and "patchmatch" in oc[key]["stage_ms"]
    assert oc["bundled"]["levels_1_ms_per_pair"] > 0
    # the tolerance library beside the exact one, never instead of it: `value` above is the exact library's, every flow verified
    assert d["library"].startswith("exact")
    tm = d["tolerance_mode"]
    assert "error" not in tm and tm["value"] > 1.2 * d["value"] and tm["ms_per_step"] < d["ms_per_step"], (tm.get("error"), tm.get("value"), d["value"])
    assert 0 < tm["latency_ms_per_pair"] < d["latency_ms_per_pair"] and tm["roofline"]["frac"] > 0
    ep = tm["epe_vs_oracle_px"]["cases"]
    assert ep["bundled_640x480"]["mean"] <= 1e-3 and ep["bundled_640x480_backwards"]["mean"] <= 1e-3, ep
    assert all(c["mean"] <= 3e-2 for c in ep.values()) and {"config2_1024x436", "config4_1920x1080", "config5_3840x2160_r17"} <= set(ep), ep
    assert all("error" not in tm["other_configs"][k] and tm["other_configs"][k]["value"] > 0 for k in ("bundled", "natural_1024x436", "hd", "uhd_r17")), tm["other_configs"]
    assert d["roofline"]["frac"] > 0 and d["roofline"]["hbm"]["frac"] > 0 if d["roofline"].get("hbm") else d["roofline"]["frac"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    wh = cb["whole_host"]           # the box's own rate: one 16-thread oracle process per 16 hardware threads, distinct pairs
    assert "error" not in wh and wh["processes"] == max(1, wh["usable_cpus"] // 16) and wh["cores"] == wh["processes"] * wh["threads_per_process"]
    assert wh["usable_cpus"] == min(wh["physical_cores"], int(wh["cgroup_cpu_quota"] or wh["physical_cores"]))       # what the job's cgroup lets it use
    assert sum(wh["round_s"]) < 60, wh              # bounded: the default bench line finishes within minutes
    assert cb["value"] == wh["value"] and cb["single_pair_16_threads"]["value"] > 0
    assert d["config"]["host_binding"]["ranks"][0]["pci"]
    assert d["vs_baseline"] is None
    hb = d["host_boundary"]
    assert "error" not in hb and hb["pipelined"] > 0 and hb["sync"] > 0


def test_bench_plain_run_times_its_steps_and_dumps_the_last_flow(tmp_path):
    """`python bench.py --gpus 1 --steps N --warmup W` without --full: exactly N timed steps in one window, the contract fields and nothing
    of the --full legs; --dump-outputs writes the flow of the last step (step N-1 -> timed pair N-1 of the 64 config-3 pairs) and it is
    the CPU oracle's flow of that pair, bit for bit (tests/golden/MANIFEST_config3.json)."""
    env = dict(os.environ)
    env.pop("RANK", None)
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(d)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(line) == 1, out.stdout[:2000]
    r = json.loads(line[0])
    assert r["steps"] == 5 and r["repeats"] == 1 and len(r["ms_per_step_by_repeat"]) == 1 and r["ms_per_step"] > 0
    assert r["metric"] == "Mflow-vectors/sec" and r["unit"] == "Mflow-vectors/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert abs(r["value"] - 1024 * 436 / (r["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * r["value"]
    assert not {"timed_region_verified", "roofline", "other_configs", "tolerance_mode", "cpu_baseline", "host_boundary"} & set(r), sorted(r)
    assert sorted(os.listdir(d)) == ["flow.npy"]
    f = np.load(d / "flow.npy")
    assert f.dtype == np.float32 and f.shape == (436, 1024, 2)
    man = json.load(open(os.path.join(GOLDEN, "MANIFEST_config3.json")))
    assert hashlib.sha256(np.ascontiguousarray(f[..., 0]).tobytes() + np.ascontiguousarray(f[..., 1]).tobytes()).hexdigest() == man["pairs"]["4"]["flow_sha256"]

# ---------------------------------------------------------------------------------------------------
# the tolerance library (libeppm_hip_tol.so: integer-domain tables / one hardware exp2 instead of the two software exp of the patch
# term, fused sums).  Default-on: north_star's floating-point bar is "within 1e-3 px EPE on the bundled
# Middlebury pair"; these tests hold the library to it against the exact library, which the rest of this suite pins to the oracle bit
# for bit -- so the numbers are end-point errors against the CPU oracle at sizes it cannot be re-run at on the GPU box.
# ---------------------------------------------------------------------------------------------------
TOL_BUNDLED_PX = 1e-3          # north_star: frame10/frame11, full size, both directions
TOL_ENVELOPE_PX = 3e-2         # every other configuration: mean EPE inside the envelope of DESIGN.md section 3.6 (measured: <= 1e-5)


@pytest.fixture(scope="module")
def tolerance_report():
    """tools/tolerance_epe.py in child processes (this process holds the parity tests' library): one for the tolerance library, the
    parent for the exact one; configs[4] (3840x2160, radius 17) included."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tolerance_epe.py"), "--all"], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in d["library"] and "tolerance" not in d["against"].split("(")[0], d
    return d


def test_tolerance_library_within_1e3_px_on_the_bundled_pair(tolerance_report):
    """frame10/frame11 640x480, the default three levels, forwards and backwards: mean EPE against the oracle <= 1e-3 px."""
    for name in ("bundled_640x480", "bundled_640x480_backwards"):
        c = tolerance_report["cases"][name]
        assert c["pixels"] == 640 * 480
        assert c["epe_mean_px"] <= TOL_BUNDLED_PX, (name, c)
        assert c["frac_over_1px"] <= 1e-4, (name, c)


def test_tolerance_library_inside_the_parity_envelope_on_every_configuration(tolerance_report):
    """configs[1] 1024x436, configs[3] 1920x1080, configs[4] 3840x2160 radius 17 and the 64 fuzz cases of the parity suite (8 seeds x 8 kinds: odd
    sizes, radii, levels, propagation modes; unrelated noise, saturated blocks whose costs tie and whose weights underflow, low contrast):
    mean EPE and the fraction of pixels off by more than 1 px are reported per case and must stay inside DESIGN.md section 3.6's
    envelope (what ANOTHER legal order of the reference's own races does is 0.04 - 0.9 px)."""
    cases = tolerance_report["cases"]
    assert {"config2_1024x436", "config4_1920x1080", "config5_3840x2160_r17"} <= set(cases) and sum(k.startswith("fuzz_") for k in cases) == 64
    for name, c in cases.items():
        assert c["epe_mean_px"] <= TOL_ENVELOPE_PX and c["frac_over_1px"] <= 1e-3, (name, c)
    print(json.dumps({k: (c["epe_mean_px"], c["frac_over_1px"]) for k, c in cases.items()}))


def test_tolerance_library_integer_stages_stay_bit_exact(frames):
    """The stages that do not depend on a float comparison of patch costs are the exact library's code and stay bit-identical in the
    tolerance library: prepare (prefilter, pyramid), census, and the final flow's smoothing given the same input.  Checked through the
    C ABI of the tolerance library in a child process: image pyramid + census planes of the bundled pair against the oracle's."""
    code = r"""
import os, sys, json, hashlib
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
from conftest import read_ppm, GOLDEN
import eppm_amd
eppm_amd.select_library("tol")
from oracle import oracle as O
a, b = read_ppm(os.path.join(GOLDEN, "frame10.ppm")), read_ppm(os.path.join(GOLDEN, "frame11.ppm"))
e = eppm_amd.EPPM(); e.init(a, b, 480, 640); e.compute_flow()
_, _, st = O.compute_flow(a, b, dump=True)
ok = {}
for l in range(3):
    for name, key in (("img1", "img1"), ("img2", "img2"), ("census1", "cen1"), ("census2", "cen2")):
        got, want = e.plane(name, l), st[f"{key}_L{l}"]
        ok[f"{name}_L{l}"] = bool(np.array_equal(np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)))
nn = np.ascontiguousarray(e.plane("nnf1", 2)); ok["nnf1_after_fill_equal_frac"] = float((nn.view(np.int16).reshape(-1) == np.ascontiguousarray(st["nnf1_fill"]).view(np.int16).reshape(-1)).mean())
print(json.dumps({"version": eppm_amd.lib().eppm_version().decode(), "ok": ok}))
""" % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert "tolerance arithmetic" in d["version"]
    for k, v in d["ok"].items():
        if k.endswith("_frac"):
            assert v >= 0.9999, d            # the NNF after hole filling: integer decisions on tolerance costs (measured: identical)
        else:
            assert v is True, d
