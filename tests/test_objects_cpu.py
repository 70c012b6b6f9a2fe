"""CPU tests of moving-object detection: a numpy / pure-Python restatement of the labelling (breadth-first flood
fill in raster order), the carry and the identity rule, which shares nothing with the C code; the host forms against it on
objects_cases(); the exact meaning on an analytic clip; the ABI's argument checks; objects.h under sanitizers.  tests/test_objects_gpu.py
runs the same cases through the kernels."""
import ctypes as C
import functools
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest

import eppm_amd
from eppm_amd import _lib, io
from conftest import ROOT
from test_tfilter_cpu import moving_clip

F = np.float32
ARG, STATE = 1, 3
SIZES = [(1, 1), (7, 1), (1, 7), (64, 4), (65, 17), (67, 45), (211, 157)]          # (w, h)
TILE_W, TILE_H = 64, 16
FIELDS = ("area", "x0", "y0", "x1", "y1", "n_flow", "sum_x", "sum_y", "sum_qu", "sum_qv")


# ---- the restatement ----

def np_components(fg, conn):
    """(h, w) int32: the raw component number of every foreground pixel, 1, 2, ... in the order a raster scan meets the components (the
    first pixel met is the component's smallest linear index, its root), 0 for background; breadth-first flood fill"""
    h, w = fg.shape
    flat = fg.ravel().tolist()
    comp = [0] * (h * w)
    steps = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (-1, 1), (1, -1), (-1, -1)] if conn == 8 else [])
    n = 0
    for i in range(h * w):
        if not flat[i] or comp[i]:
            continue
        n += 1
        comp[i] = n
        q = deque([i])
        while q:
            j = q.popleft()
            y, x = divmod(j, w)
            for dx, dy in steps:
                nx, ny = x + dx, y + dy
                if 0 <= nx < w and 0 <= ny < h:
                    k = ny * w + nx
                    if flat[k] and not comp[k]:
                        comp[k] = n
                        q.append(k)
    return np.array(comp, np.int32).reshape(h, w)


def np_flow_ok(u, v):
    with np.errstate(invalid="ignore"):
        return (np.abs(u) <= F(8192)) & (np.abs(v) <= F(8192))


def np_label(mask, u, v, conn, min_area, max_objects):
    """(labels, records, counts, raw components)"""
    comp = np_components(mask == 1, conn)
    areas = np.bincount(comp.ravel())[1:]
    found = areas >= min_area
    number = np.cumsum(found) * found                       # 1, 2, ... in raw (root) order
    number[number > max_objects] = 0
    labels = np.concatenate([[0], number])[comp].astype(np.uint8)
    n = int(min(found.sum(), max_objects))
    ok = np_flow_ok(u, v)
    with np.errstate(invalid="ignore", over="ignore"):
        qu, qv = np.rint(u * F(256)), np.rint(v * F(256))
    recs = []
    for k in range(1, n + 1):
        ys, xs = np.nonzero(labels == k)
        sel = ok[ys, xs]
        recs.append(dict(area=len(xs), x0=int(xs.min()), y0=int(ys.min()), x1=int(xs.max()), y1=int(ys.max()), n_flow=int(sel.sum()),
                         sum_x=int(xs.sum()), sum_y=int(ys.sum()), sum_qu=int(qu[ys, xs][sel].astype(np.int64).sum()),
                         sum_qv=int(qv[ys, xs][sel].astype(np.int64).sum())))
    return labels, recs, dict(n=n, n_found=int(found.sum()), n_components=len(areas)), comp


def np_carry(labels, bu, bv, occ2):
    h, w = labels.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        known = (np.abs(bu) <= F(1e9)) & (np.abs(bv) <= F(1e9))
        qx, qy = xs.astype(F) + bu, ys.astype(F) + bv
        inside = (qx >= 0) & (qx <= F(w - 1)) & (qy >= 0) & (qy <= F(h - 1))
        ok = (occ2 == 0) & known & inside
        nx = np.where(ok, np.floor(qx + F(0.5)), 0).astype(np.int64)
        ny = np.where(ok, np.floor(qy + F(0.5)), 0).astype(np.int64)
    assert nx.min() >= 0 and nx.max() < w and ny.min() >= 0 and ny.max() < h
    return np.where(ok, labels[ny, nx], 0).astype(np.uint8)


def np_assign(labels, carried, n, prev_id, prev_age, next_id, max_objects, min_overlap):
    """(ids, ages, prev_id, prev_age, next_id, outcomes): the identity rule, and which way each object went"""
    S = max_objects + 1
    V = np.zeros((S, S), np.int64)
    if carried is not None:
        p = np.where(carried.astype(np.int64) <= max_objects, carried, 0).astype(np.int64)
        sel = (labels >= 1) & (labels <= n) & (p >= 1)
        np.add.at(V, (labels[sel].astype(np.int64), p[sel]), 1)
    best = [0] * S
    for c in range(1, n + 1):
        if V[c, 1:].max(initial=0) > 0:
            best[c] = 1 + int(np.argmax(V[c, 1:]))           # the first largest: ties to the lower p
    winner = [0] * S
    for p in range(1, S):
        cl = [c for c in range(1, n + 1) if best[c] == p]
        if cl:
            winner[p] = max(cl, key=lambda c: (V[c, p], -c))  # ties to the lower c
    ids, ages, how = [], [], []
    nid, nage = np.zeros(256, np.int32), np.zeros(256, np.int32)
    nxt = int(next_id)
    for c in range(1, n + 1):
        p = best[c]
        if p and winner[p] == c and V[c, p] >= min_overlap:
            ids.append(int(prev_id[p])); ages.append(int(prev_age[p]) + 1); how.append("inherited")
        else:
            ids.append(nxt); ages.append(0)
            nxt += 1
            how.append("no vote" if not p else "lost" if winner[p] != c else "below")
        nid[c], nage[c] = ids[-1], ages[-1]
    return ids, ages, nid, nage, (1 if nxt > 2 ** 30 else nxt), how


# ---- the cases ----

def spiral(h, w):
    """a one-pixel-wide spiral through the whole frame, one background pixel between its turns"""
    m = np.zeros((h, w), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    inside = lambda a, b: 0 <= a < w and 0 <= b < h          # noqa: E731
    while True:
        for _ in range(2):
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and not m[ny, nx] and not (inside(fx, fy) and m[fy, fx]):
                x, y = nx, ny
                m[y, x] = 1
                break
            dx, dy = -dy, dx
        else:
            return m


def blocks(h, w):
    """4 x 3 rectangles, 8 pixels apart, on rows of tiles: labelled 1, 2, ... in raster order at either connectivity"""
    m = np.zeros((h, w), np.uint8)
    for y in range(0, h - 2, 5):
        for x in range(0, w - 3, 8):
            m[y:y + 3, x:x + 4] = 1
    return m


def make_mask(kind, h, w, rng):
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    if kind == "empty":
        pass
    elif kind == "full":
        m[:] = 1
    elif kind == "bytes":
        m = rng.integers(0, 4, (h, w)).astype(np.uint8)
        m[rng.random((h, w)) < 0.05] = 255
    elif kind.startswith("rand"):
        m = (rng.random((h, w)) < int(kind[4:]) / 100).astype(np.uint8)
    elif kind == "checker":
        m = ((xs + ys) % 2 == 0).astype(np.uint8)
    elif kind == "spiral":
        m = spiral(h, w)
    elif kind == "comb":
        m[:, ::2] = 1
        m[-1, :] = 1                                         # vertical teeth joined only by the bottom row
    elif kind == "diag":
        m = ((xs + ys) % 4 == 0).astype(np.uint8)
    elif kind == "stripes_in":                               # the last column / row of a tile
        m[:, TILE_W - 1::TILE_W] = 1
        m[TILE_H - 1::TILE_H, :] = 1
    elif kind == "stripes_out":                              # the first column / row of the next tile
        m[:, TILE_W::TILE_W] = 1
        m[TILE_H::TILE_H, :] = 1
    elif kind == "stripes_dashed":                           # dashes on both sides of every border: they touch by their corners only
        m[:, TILE_W - 1::TILE_W] = (ys % 4 < 2)[:, TILE_W - 1::TILE_W]
        m[:, TILE_W::TILE_W] = (ys % 4 >= 2)[:, TILE_W::TILE_W]
        m[TILE_H - 1::TILE_H, :] |= (xs % 4 < 2)[TILE_H - 1::TILE_H, :]
        m[TILE_H::TILE_H, :] |= (xs % 4 >= 2)[TILE_H::TILE_H, :]
    elif kind == "ushapes":                                  # two nested U shapes joined by one bridge in the bottom right tile
        for d in (1, 4):
            m[d:h - d, d] = 1
            m[d:h - d, w - 1 - d] = 1
            m[h - 1 - d, d:w - d] = 1
        m[h - 5:h - 1, w - 8] = 1
    elif kind == "blocks":
        m = blocks(h, w)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(m, np.uint8)


SPECIAL = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, -0.0, 8192.0, np.nextafter(F(8192), F(0)), np.nextafter(F(8192), F(1e9)),
                    -8192.0, -np.nextafter(F(8192), F(1e9)), 1e9, 3e38, 0.5, -0.5, 1.5, 2.5, 1 / 512, 3 / 512], F)


def make_flow(kind, h, w, rng):
    if kind == "integer":
        u, v = rng.integers(-3, 4, (h, w)).astype(F), rng.integers(-3, 4, (h, w)).astype(F)
    else:
        u, v = (rng.standard_normal((h, w)) * 3).astype(F), (rng.standard_normal((h, w)) * 3).astype(F)
    if kind == "special":
        for a in (u, v):
            sel = rng.random((h, w)) < 0.3
            a[sel] = SPECIAL[rng.integers(0, len(SPECIAL), int(sel.sum()))]
    return u, v


MASKS = ["empty", "full", "bytes", "rand30", "rand45", "rand60", "checker", "spiral", "comb", "diag", "stripes_in", "stripes_out",
         "stripes_dashed", "ushapes", "blocks"]
BOTH = {"full", "checker", "spiral", "comb", "diag", "stripes_dashed", "ushapes", "rand45"}


def finish_case(c, labelled=None):
    """the restatement's results of a case (labelled: np_label's result on the case, if the caller has it already)"""
    h, w, M = c["h"], c["w"], c["max_objects"]
    labels, recs, counts, comp = labelled or np_label(c["mask"], c["u"], c["v"], c["conn"], c["min_area"], M)
    empty = c["prev"] == "empty"
    pid, page, nxt = (np.zeros(256, np.int32), np.zeros(256, np.int32), 1) if empty else (c["prev_id"], c["prev_age"], c["next_id"])
    ids, ages, nid, nage, nxt, how = np_assign(labels, None if empty else c["carried"], counts["n"], pid, page, nxt, M, c["min_overlap"])
    for r, i, a in zip(recs, ids, ages):
        r["id"], r["age"] = i, a
    carry = c["bu"] is not None and not c["cut"]
    c.update(want_labels=labels, want_recs=recs, want_counts=dict(counts, next_id=nxt), want_prev_id=nid, want_prev_age=nage, how=how, comp=comp,
             want_carried=np_carry(labels, c["bu"], c["bv"], c["occ2"]) if carry else np.zeros((h, w), np.uint8))
    return c


def previous_state(kind, mask, conn, min_area, M, rng, labels=None):
    """a carried plane and tables for a case: (carried, prev_id, prev_age, next_id); labels: the case's labels, if the caller has them"""
    h, w = mask.shape
    pid = np.zeros(256, np.int32)
    page = np.zeros(256, np.int32)
    pid[1:] = rng.permutation(255) + 100
    page[1:] = rng.integers(0, 50, 255)
    nxt = int(rng.integers(400, 500))
    if labels is None:
        labels = np_label(mask, np.zeros((h, w), F), np.zeros((h, w), F), conn, min_area, M)[0]
    if kind == "zero":
        car = np.zeros((h, w), np.uint8)
    elif kind == "full":                                     # previous object 1 everywhere: every vote of a wave lands on one address
        car = np.ones((h, w), np.uint8)
    elif kind == "shifted":                                  # the labels themselves, renumbered and moved by (2, 1)
        perm = np.concatenate([[0], rng.permutation(M) + 1]).astype(np.uint8)
        car = np.zeros((h, w), np.uint8)
        car[1:, 2:] = perm[labels][:h - 1, :w - 2] if h > 1 and w > 2 else 0
    elif kind == "split":                                    # one previous object over every pair of current ones
        car = ((labels.astype(np.int64) + 1) // 2).astype(np.uint8)
    elif kind == "merge":                                    # two previous objects in every current one: the left part is the smaller
        xs = np.mgrid[0:h, 0:w][1]
        car = np.where(labels > 0, np.minimum(2 * labels.astype(np.int64) - (xs % 8 < 1), 255), 0).astype(np.uint8)
    elif kind == "random":                                   # any byte, those above max_objects too
        car = rng.integers(0, 256, (h, w)).astype(np.uint8)
        car[rng.random((h, w)) < 0.5] = 0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(car), pid, page, nxt


def identity_case(h, w, rng):
    """blocks of 12 pixels and a carried plane that sends the rule through every outcome, min_overlap 4: object 1 votes 2 and 3 equally
    (inherits 2's id: the lower p), 2 and 3 both vote 5 with 6 pixels each (2 wins: the lower c; 3 is lost), 4 has exactly 4 pixels of 7
    (inherits), 5 has 3 pixels of 8 (below), 6 has none, 7 votes 9 with 5 pixels against 8's 7 (lost to the larger claimant)"""
    mask = blocks(h, w)
    car = np.zeros((h, w), np.uint8)
    x = lambda k: 8 * (k - 1)                                # noqa: E731
    car[0, x(1):x(1) + 4], car[1, x(1):x(1) + 4] = 3, 2
    car[0:2, x(2):x(2) + 3] = 5
    car[0:2, x(3):x(3) + 3] = 5
    car[0, x(4):x(4) + 4] = 7
    car[0, x(5):x(5) + 3] = 8
    car[0:2, x(7):x(7) + 4] = 9
    car[0:2, x(7) + 1:x(7) + 2] = 0
    car[1, x(7) + 3] = 0
    car[0:2, x(8):x(8) + 4] = 9
    car[0, x(8)] = 0
    return mask, car


@functools.lru_cache(maxsize=None)
def objects_cases():
    rng = np.random.default_rng(2026)
    cases = []
    prevs = ["empty", "zero", "shifted", "split", "merge", "random"]
    flows = ["integer", "fraction", "special"]
    k = 0
    for w, h in SIZES:
        for kind in MASKS:
            if kind == "ushapes" and (h < 12 or w < 16):
                continue
            if kind == "blocks" and (h < 3 or w < 12):
                continue
            mask = make_mask(kind, h, w, rng)
            for conn in ((4, 8) if kind in BOTH else ((4, 8)[k % 2],)):
                k += 1
                M = (1, 64, 255, 64)[k % 4]
                min_area = (1, 16, 1, h * w + 1, 4)[k % 5]
                if kind in ("spiral", "ushapes", "comb"):
                    min_area = (1, 16)[k % 2]
                if kind == "rand30" and w * h >= 256:
                    min_area, M = 1, 64                      # n_found > max_objects
                if kind == "rand45" and w * h >= 256:
                    min_area, M = 16, 255                    # drops some, keeps some
                prev = prevs[k % len(prevs)]
                c = dict(name=f"{w}x{h}-{kind}-c{conn}-a{min_area}-m{M}-{prev}", h=h, w=w, kind=kind, mask=mask, conn=conn, min_area=min_area,
                         max_objects=M, min_overlap=(4, 1, 9)[k % 3], prev=prev, cut=k % 7 == 3)
                c["u"], c["v"] = make_flow(flows[k % 3], h, w, rng)
                c["bu"], c["bv"] = make_flow(flows[(k + 1) % 3], h, w, rng)
                if k % 11 == 5:
                    c["bu"] = c["bv"] = None                 # no carry
                c["occ2"] = (rng.integers(0, 4, (h, w)) * (rng.random((h, w)) < 0.2)).astype(np.uint8)
                if prev != "empty":
                    c["carried"], c["prev_id"], c["prev_age"], c["next_id"] = previous_state(prev, mask, conn, min_area, M, rng)
                cases.append(finish_case(c))
        if w >= 64:                                          # the identity rule's outcomes, ties and thresholds
            mask, car = identity_case(h, w, rng)
            c = dict(name=f"{w}x{h}-identity", h=h, w=w, kind="identity", mask=mask, conn=8, min_area=12, max_objects=64, min_overlap=4,
                     prev="designed", cut=False, carried=car, prev_id=(np.arange(256) * 3 + 7).astype(np.int32),
                     prev_age=(np.arange(256) % 9).astype(np.int32), next_id=2 ** 30 - 2 if w == 65 else 1000)
            c["u"], c["v"] = make_flow("integer", h, w, rng)
            c["bu"], c["bv"] = make_flow("integer", h, w, rng)
            c["occ2"] = np.zeros((h, w), np.uint8)
            cases.append(finish_case(c))
    # what the generator holds of its own cases, so that none is vacuous
    big = [c for c in cases if c["w"] >= 64]
    assert any(c["want_counts"]["n_found"] > c["max_objects"] for c in big)
    assert any(0 < c["want_counts"]["n_found"] < c["want_counts"]["n_components"] for c in big)
    assert any(spans_tiles(c, 3) for c in big)
    for c in cases:
        if c["kind"] == "spiral" and c["w"] * c["h"] > 1:
            assert np.bincount(c["comp"].ravel())[1:].max() * 3 >= c["w"] * c["h"], c["name"]
            assert c["want_counts"]["n_components"] == 1
        if c["kind"] == "ushapes":
            assert c["want_counts"]["n_components"] == 1, c["name"]
        if c["kind"] == "identity":
            assert c["how"][:7] == ["inherited", "inherited", "lost", "inherited", "below", "no vote", "lost"], c["how"][:8]
            assert c["how"][7] == "inherited" and c["want_recs"][0]["id"] == 2 * 3 + 7 and c["want_recs"][1]["id"] == 5 * 3 + 7
    for kind in ("diag", "checker"):
        a = {(c["w"], c["h"], c["conn"]): c["want_counts"]["n_components"] for c in big if c["kind"] == kind}
        assert all(a[(w, h, 4)] > a[(w, h, 8)] for (w, h, conn) in a if conn == 4), kind
    seen = {o for c in cases for o in c["how"]}
    assert seen == {"inherited", "lost", "below", "no vote"}, seen
    assert any(c["want_counts"]["next_id"] == 1 and c["prev"] == "designed" for c in cases)          # next_id passed 2^30 and started again
    return cases


def spans_tiles(c, n):
    comp = c["comp"]
    for k in np.argsort(np.bincount(comp.ravel())[1:])[::-1][:3] + 1:
        ys, xs = np.nonzero(comp == k)
        if len(np.unique(xs // TILE_W)) >= n and len(np.unique(ys // TILE_H)) >= n:
            return True
    return False


# ---- the large cases: launch shapes only large or thin frames reach ----

LARGE_SIZES = [(256, 256), (257, 256), (513, 257), (8192, 20), (20, 8192)]          # (w, h): 64, 65, 129, 160 and 160 chunks
ROUND = 64                                                   # chunks per trip of k_obj_scan's loop: one per lane of its wave
LARGE_MIN_AREA = 6


def obj_chunk():
    src = open(os.path.join(ROOT, "eppm_amd", "csrc", "objects.h")).read()
    return int(re.search(r"constexpr int kObjChunk = (\d+);", src).group(1))


def _extent(shape, y, x, w):
    """inclusive (y0, y1, x0, x1) of a shape: a speck is one pixel, a run 6 pixels of one row, a blob 2 x 6 pixels and one more that
    touches them by a corner only (an object of 13 pixels at connectivity 8; one of 12 and a speck at 4)"""
    return (y, y, x, x) if shape == "speck" else (y, y, x, x + 5) if shape == "run" else (y, y + 2, x, min(x + 6, w - 1))


def _free(m, y0, y1, x0, x1):
    return not m[max(y0 - 1, 0):y1 + 2, max(x0 - 1, 0):x1 + 2].any()


def _stamp(m, shape, y, x):
    if shape == "speck":
        m[y, x] = 1
    elif shape == "run":
        m[y, x:x + 6] = 1
    else:
        m[y:y + 2, x:x + 6] = 1
        if x + 6 < m.shape[1]:
            m[y + 2, x + 6] = 1


def _thin(seq, n):
    """n of seq, evenly, the first and the last among them"""
    if len(seq) <= n:
        return list(seq)
    return [seq[i] for i in np.linspace(0, len(seq) - 1, n).round().astype(int)]


def large_mask(kind, h, w, M, boundary):
    """Isolated shapes on a frame: a speck (below LARGE_MIN_AREA) in every chunk, and objects whose roots (their first pixels) are chosen
    by kind.  late: only in chunks >= boundary.  spread: about 90 over the whole frame, the last in the last chunk.  cap: M - 2 in the
    chunks below boundary, then 20 in a row from it, so that number M + 1 falls inside a chunk >= boundary."""
    chunk, npx = obj_chunk(), h * w
    m = np.zeros((h, w), np.uint8)
    for k in range(-(-npx // chunk)):
        n = min(chunk, npx - k * chunk)
        for t in range(n):
            y, x = divmod(k * chunk + (389 * k + 211 + 7 * t) % n, w)
            if _free(m, y, y, x, x):
                m[y, x] = 1
                break
        else:
            raise AssertionError(f"no room for a speck in chunk {k}")
    cand = [("blob", y, x) for y in range(0, h - 4, 4) for x in range(0, w - 5, 8)] + [("run", h - 1, x) for x in range(0, w - 5, 8)]
    cand = [c for c in cand if _free(m, *_extent(*c, w))]           # in the order of their roots; no two touch
    late = [c for c in cand if c[1] * w + c[2] >= boundary * chunk]
    if kind == "late":
        pick = _thin(late, 40)
    elif kind == "spread":
        pick = _thin(cand, 90)
    elif kind == "cap":
        pick = _thin(cand[:len(cand) - len(late)], M - 2) + late[:20]
    else:
        raise ValueError(kind)
    for c in pick:
        _stamp(m, *c)
    return m


def stripe(h, w):
    """two lines along the frame's long side, 17 pixels apart and joined at the far end: one component from index 0 through every tile"""
    m = np.zeros((h, w), np.uint8)
    if w >= h:
        m[0, :] = m[17, :] = 1
        m[0:18, w - 1] = 1
    else:
        m[:, 0] = m[:, 17] = 1
        m[h - 1, 0:18] = 1
    return m


def stripe_sums(h, w):
    """(area, sum_x, sum_y) of stripe(h, w) in closed form: two lines of `long` pixels and the 16 pixels between their ends"""
    long = max(h, w)
    along, across = long * (long - 1) + 16 * (long - 1), 17 * long + 16 * 17 // 2
    return (2 * long + 16,) + ((along, across) if w >= h else (across, along))


@functools.lru_cache(maxsize=None)
def objects_large_cases(size=None):
    """the cases of LARGE_SIZES[size], or of every size; built on the first call, never at import"""
    if size is None:
        return [c for k in range(len(LARGE_SIZES)) for c in objects_large_cases(k)]
    w, h = LARGE_SIZES[size]
    rng = np.random.default_rng(3000 + size)
    nchunks = -(-h * w // obj_chunk())
    second = ROUND if nchunks > ROUND else nchunks - 1      # 256 x 256 is one full round: its "late" chunk is the round's last
    third = 2 * ROUND if nchunks > 2 * ROUND else second
    plan = [("late", 4, 255, second, "zero"), ("late", 8, 64, second, "empty"), ("spread", 4, 128, second, "empty"),
            ("spread", 8, 255, second, "random"), ("cap", 8, 3, second, "random"), ("cap", 4, 255, third, "zero"),
            ("carried", 4, 128, second, "shifted"), ("carried", 8, 255, second, "shifted")]
    if max(w, h) == 8192:
        plan += [("stripe", 4, 1, second, "empty"), ("stripe", 8, 64, second, "full")]
    if (w, h) == (513, 257):
        plan += [(kind, conn, M, second, prev) for kind in ("spiral", "comb") for conn, M, prev in ((4, 1, "full"), (8, 64, "empty"))]
    flows = ["integer", "fraction", "special"]
    cases = []
    for k, (kind, conn, M, boundary, prev) in enumerate(plan):
        if kind == "stripe":
            mask, min_area = stripe(h, w), 16
        elif kind in ("spiral", "comb"):
            mask, min_area = make_mask(kind, h, w, rng), 16
        else:
            mask, min_area = large_mask("spread" if kind == "carried" else kind, h, w, M, boundary), LARGE_MIN_AREA
        c = dict(name=f"{w}x{h}-{kind}-c{conn}-m{M}-{prev}", h=h, w=w, kind=kind, mask=mask, conn=conn, min_area=min_area, max_objects=M,
                 min_overlap=(4, 5, 1)[k % 3], prev=prev, cut=False, boundary=boundary)
        c["u"], c["v"] = make_flow(flows[k % 3], h, w, rng)
        c["bu"], c["bv"] = make_flow(flows[(k + 1) % 3], h, w, rng)
        if k % 5 == 4:                                       # vectors that end on the frame's last column and row, and just beyond them
            ys, xs = np.mgrid[0:h, 0:w]
            c["bu"], c["bv"] = (F(w - 1) - xs).astype(F), (F(h - 1) - ys).astype(F)
            c["bu"][::2, ::3] = np.nextafter(c["bu"][::2, ::3], F(1e9))
            c["bv"][1::2, 1::3] = np.nextafter(c["bv"][1::2, 1::3], F(1e9))
        c["occ2"] = (rng.integers(0, 4, (h, w)) * (rng.random((h, w)) < 0.2)).astype(np.uint8)
        labelled = np_label(mask, c["u"], c["v"], conn, min_area, M)
        if kind in ("stripe", "spiral", "comb") and prev == "full":
            c["min_overlap"] = int(mask.sum())               # inherits only if every pixel's vote is counted
        if kind == "carried":                                # a blob moved by (2, 1) keeps 4 votes, 5 with its corner pixel at connectivity 8:
            c["min_overlap"] = 4 if conn == 4 else 6         # exactly enough, and one too few
        if prev != "empty":
            c["carried"], c["prev_id"], c["prev_age"], c["next_id"] = previous_state(prev, mask, conn, min_area, M, rng, labels=labelled[0])
        cases.append(finish_case(c, labelled))
    return cases


def large_ledger(c):
    """what a large case makes the scan and the numbering do, from the restatement's raw components alone: per chunk the roots and the
    found roots (a root is a component's first pixel in raster order), by rounds of ROUND chunks"""
    chunk, npx = obj_chunk(), c["h"] * c["w"]
    nchunks = -(-npx // chunk)
    ids, roots = np.unique(c["comp"].ravel(), return_index=True)
    roots = roots[ids > 0]
    areas = np.bincount(c["comp"].ravel())[1:]
    assert len(roots) == len(areas) and np.all(np.diff(roots) > 0)
    found = roots[areas >= c["min_area"]]
    per_chunk = lambda r: np.bincount(r // chunk, minlength=nchunks)          # noqa: E731
    rounds = -(-nchunks // ROUND)
    by_round = lambda a: [int(a[k * ROUND:(k + 1) * ROUND].sum()) for k in range(rounds)]          # noqa: E731
    tiles_x, tiles_y = -(-c["w"] // TILE_W), -(-c["h"] // TILE_H)
    ys, xs = np.nonzero(c["comp"] == 1)
    return dict(nchunks=nchunks, rounds=rounds, found=by_round(per_chunk(found)), components=by_round(per_chunk(roots)),
                specks=per_chunk(roots[areas < c["min_area"]]), found_roots=found, chunk=chunk, tiles=(tiles_x, tiles_y),
                tiles_of_first=len(set(zip((ys // TILE_H).tolist(), (xs // TILE_W).tolist()))))


def host_case(c):
    """the host forms on a case: (labels, records with id and age, counts with next_id, carried, prev_id, prev_age)"""
    M = c["max_objects"]
    labels, recs, counts = io.objects_label_host(c["mask"], c["u"], c["v"], c["conn"], c["min_area"], M)
    empty = c["prev"] == "empty"
    pid, page, nxt = io.objects_state() if empty else (c["prev_id"], c["prev_age"], c["next_id"])
    ids, ages, pid, page, nxt = io.objects_assign_host(labels, counts["n"], None if empty else c["carried"], pid, page, nxt, M, c["min_overlap"])
    for r, i, a in zip(recs, ids, ages):
        r["id"], r["age"] = i, a
    carry = c["bu"] is not None and not c["cut"]
    car = io.objects_carry_host(labels, c["bu"], c["bv"], c["occ2"]) if carry else np.zeros_like(labels)
    return labels, recs, dict(counts, next_id=nxt), car, pid, page


def differences(c, labels, recs, counts, carried, pid, page):
    """what differs from the restatement's results of case c"""
    bad = []
    if not np.array_equal(labels, c["want_labels"]):
        bad.append(("labels", int((labels != c["want_labels"]).sum())))
    if counts != c["want_counts"]:
        bad.append(("counts", counts, c["want_counts"]))
    got = [{k: r[k] for k in FIELDS + ("id", "age")} for r in recs]
    if got != c["want_recs"]:
        bad.append(("records", [(g, w) for g, w in zip(got, c["want_recs"]) if g != w][:2], len(got), len(c["want_recs"])))
    if not np.array_equal(carried, c["want_carried"]):
        bad.append(("carried", int((carried != c["want_carried"]).sum())))
    if not np.array_equal(pid, c["want_prev_id"]) or not np.array_equal(page, c["want_prev_age"]):
        bad.append(("tables",))
    return bad


# ---- 1. the host forms equal the restatement ----

@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_forms_equal_the_restatement(size):
    cases = [c for c in objects_cases() if (c["w"], c["h"]) == SIZES[size]]
    assert len(cases) >= 10
    for c in cases:
        bad = differences(c, *host_case(c))
        assert not bad, (c["name"], bad)
    c = cases[-1]                                            # the derived fields
    for r in io.objects_label_host(c["mask"], c["u"], c["v"], c["conn"], c["min_area"], c["max_objects"])[1]:
        assert r["centroid"] == (r["sum_x"] / r["area"], r["sum_y"] / r["area"])
        assert r["velocity"] is None if not r["n_flow"] else r["velocity"] == (r["sum_qu"] / (256.0 * r["n_flow"]), r["sum_qv"] / (256.0 * r["n_flow"]))


LARGE_IDS = [f"{w}x{h}" for w, h in LARGE_SIZES]


@pytest.mark.parametrize("size", range(len(LARGE_SIZES)), ids=LARGE_IDS)
def test_host_forms_equal_the_restatement_on_large_frames(size):
    cases = objects_large_cases(size)
    assert len(cases) >= 8
    for c in cases:
        bad = differences(c, *host_case(c))
        assert not bad, (c["name"], bad)


@pytest.mark.parametrize("size", range(len(LARGE_SIZES)), ids=LARGE_IDS)
def test_large_cases_reach_what_they_advertise(size):
    """The ledger of objects_large_cases(): every case makes k_obj_scan and k_obj_number do what its kind says, computed from the
    restatement's components alone.  A case that stops meeting its condition fails here; none is skipped."""
    w, h = LARGE_SIZES[size]
    cases = objects_large_cases(size)
    kinds = [c["kind"] for c in cases]
    assert all(kinds.count(k) == 2 for k in ("late", "spread", "cap", "carried"))
    assert kinds.count("stripe") == (2 if max(w, h) == 8192 else 0) and kinds.count("spiral") == kinds.count("comb") == (2 if (w, h) == (513, 257) else 0)
    assert {c["conn"] for c in cases if c["kind"] in ("late", "spread", "carried")} == {4, 8}
    assert {c["max_objects"] for c in cases if c["kind"] == "cap"} == {3, 255}
    assert any(c["prev"] == "empty" for c in cases) and any(c["prev"] != "empty" for c in cases)
    want_chunks = {(256, 256): 64, (257, 256): 65, (513, 257): 129, (8192, 20): 160, (20, 8192): 160}[(w, h)]
    for c in cases:
        L, n, M = large_ledger(c), c["want_counts"], c["max_objects"]
        name = c["name"]
        assert L["nchunks"] == want_chunks and L["rounds"] == -(-want_chunks // ROUND), name
        assert L["tiles"] == (-(-w // 64), -(-h // 16)), name
        assert sum(L["found"]) == n["n_found"] and sum(L["components"]) == n["n_components"], name
        later = L["rounds"] > 1                              # 256 x 256 is exactly one round: its conditions are on the round's last chunk
        b = c["boundary"]
        assert (b % ROUND == 0 and ROUND <= b < L["nchunks"]) if later else b == L["nchunks"] - 1, name          # a later round's first chunk
        first_late = L["found_roots"][L["found_roots"] >= b * L["chunk"]]
        if c["kind"] in ("late", "spread", "cap", "carried"):
            assert L["specks"].min() >= 1, name               # below min_area in every chunk
            assert len(first_late) > 0, name                  # found roots in round >= 2
            if later:                                         # found roots in every later round; a cap case stops 20 objects after its boundary
                assert (any if c["kind"] == "cap" else all)(f > 0 for f in L["found"][1:]), name
        if c["kind"] == "late":
            assert (L["found"][0] == 0) if later else (L["found_roots"].min() >= b * L["chunk"]), name          # the prefix entering round 2
            assert L["components"][0] >= ROUND - 1 and n["n_found"] <= M, name
            y, x = divmod(int(first_late[0]), w)
            assert c["want_labels"][y, x] == 1, name          # the first found root of round 2 is object 1
        if c["kind"] in ("spread", "carried"):
            assert L["found"][0] > 0 and n["n_found"] <= M and n["n"] == n["n_found"], name
            y, x = divmod(int(L["found_roots"][-1]), w)
            assert L["found_roots"][-1] // L["chunk"] == L["nchunks"] - 1 and c["want_labels"][y, x] == n["n"], name
        if c["kind"] == "carried":
            how = set(c["how"])
            assert ("inherited" in how and "below" not in how) if c["conn"] == 4 else ("below" in how and "inherited" not in how), (name, how)
        if c["kind"] == "cap":
            assert n["n_found"] > M and n["n"] == M, name
            last_in, first_out = int(L["found_roots"][M - 1]), int(L["found_roots"][M])
            assert last_in // L["chunk"] == first_out // L["chunk"] >= b and (b >= ROUND) == later, name          # crossed inside a chunk
            for root, lab in ((last_in, M), (first_out, 0), (int(L["found_roots"][-1]), 0)):
                assert c["want_labels"][root // w, root % w] == lab, name
        if c["kind"] in ("stripe", "spiral", "comb"):
            ys, xs = np.nonzero(c["mask"])
            r = c["want_recs"][0]
            assert n == dict(n=1, n_found=1, n_components=1, next_id=n["next_id"]) and c["comp"][0, 0] == 1, name
            assert L["tiles_of_first"] == L["tiles"][0] * L["tiles"][1], name
            assert (r["area"], r["sum_x"], r["sum_y"]) == (len(xs), int(xs.sum()), int(ys.sum())), name
            if c["kind"] == "stripe":
                assert (r["area"], r["sum_x"], r["sum_y"]) == stripe_sums(h, w), name
                assert (r["x1"], r["y1"]) == (w - 1, 17) if w > h else (r["x1"], r["y1"]) == (17, h - 1), name
            if c["prev"] == "full":
                assert c["how"] == ["inherited"] and c["min_overlap"] == r["area"], name
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)


def test_raw_components_equal_scipy():
    try:
        from scipy import ndimage
    except ImportError:
        return                                               # the cross-check is a bonus: the restatement stands without it
    n = 0
    for c in objects_cases():
        if c["w"] * c["h"] > 67 * 45 and c["kind"] not in ("spiral", "rand45", "ushapes"):
            continue
        want, _ = ndimage.label(c["mask"] == 1, structure=np.ones((3, 3), int) if c["conn"] == 8 else None)
        assert np.array_equal(want, c["comp"]), c["name"]
        n += 1
    assert n >= 50


def test_special_vectors():
    """one ulp either side of 8192, -0.0, NaN, inf and 1e10 in the forward flow: which pixels count, and what they add"""
    hi, lo = np.nextafter(F(8192), F(1e9)), np.nextafter(F(8192), F(0))
    u = np.array([[8192.0, hi, lo, -8192.0, -hi, -0.0, np.nan, np.inf, 1e10, 0.5 / 256, 1.5 / 256, 2.5 / 256]], F)
    v = np.zeros_like(u)
    _, recs, _ = io.objects_label_host(np.ones_like(u, np.uint8), u, v, min_area=1)
    assert len(recs) == 1 and recs[0]["n_flow"] == 7                                   # hi, -hi, NaN, inf and 1e10 do not count
    assert recs[0]["sum_qu"] == 8192 * 256 + 2 ** 21 - 8192 * 256 + 0 + 0 + 2 + 2          # lo * 256 = 2^21 - 1/8; rintf: half to even
    _, recs, _ = io.objects_label_host(np.ones_like(u, np.uint8), v, u, min_area=1)
    assert recs[0]["n_flow"] == 7 and recs[0]["sum_qu"] == 0 and recs[0]["sum_qv"] == 2 ** 21 + 4
    # the carry: an end half a pixel short of the next pixel rounds up to it; the frame test is closed; NaN and unknown give 0
    lab = np.arange(1, 8, dtype=np.uint8)[None, :]
    bu = np.array([[0.5, 0.49, -1.0, 3.0 + 1e-6, np.nan, 1e10, -0.0]], F)
    assert io.objects_carry_host(lab, bu, np.zeros_like(bu), np.zeros_like(lab)).tolist() == [[2, 2, 2, 0, 0, 0, 7]]
    assert io.objects_carry_host(lab, bu, np.zeros_like(bu), np.full_like(lab, 2)).tolist() == [[0] * 7]


# ---- 2. meaning, exact ----

def analytic_clip(h, w, nframes, bg_v=(2, 1), sq_v=(-1, 2), sq=24):
    """test_stabilize_cpu.moving_clip's geometry: per pair (u, v, occ1, bu, bv, occ2, inside): the analytic flows of a background moving by
    bg_v and a sq x sq square moving by sq_v over it, the masks (1: covered by the square in the other frame, 2: the vector leaves the
    frame) and the square's pixels in image 1"""
    _, _, bwd, occ2 = moving_clip(h, w, nframes, bg_v=bg_v, sq_v=sq_v, sq=sq)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = []
    for k in range(nframes):
        m = np.zeros((h, w), bool)
        sx, sy = w // 2 + k * sq_v[0], h // 4 + k * sq_v[1]
        m[sy:sy + sq, sx:sx + sq] = True
        inside.append(m)
    out = []
    for k in range(nframes - 1):
        u = np.where(inside[k], sq_v[0], bg_v[0]).astype(F)
        v = np.where(inside[k], sq_v[1], bg_v[1]).astype(F)
        tx, ty = xs + u.astype(int), ys + v.astype(int)
        leaves = (tx < 0) | (tx >= w) | (ty < 0) | (ty >= h)
        covered = ~inside[k] & inside[k + 1][np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
        occ1 = np.where(leaves, 2, np.where(covered, 1, 0)).astype(np.uint8)
        out.append((u, v, occ1, bwd[k][0], bwd[k][1], occ2[k], inside[k]))
    return out


def test_moving_square_is_one_object_with_one_id():
    h, w = 96, 128
    car = None
    pid, page, nxt = io.objects_state()
    for k, (u, v, occ1, bu, bv, occ2, inside) in enumerate(analytic_clip(h, w, 8)):
        model, mask = io.gmotion_fit_host(u, v, occ1)
        assert model["valid"]
        labels, recs, counts = io.objects_label_host(mask, u, v)
        assert counts == dict(n=1, n_found=1, n_components=1), (k, counts)
        ids, ages, pid, page, nxt = io.objects_assign_host(labels, 1, car, pid, page, nxt)
        ys, xs = np.nonzero(inside & (occ1 == 0))
        r = recs[0]
        assert (r["x0"], r["y0"], r["x1"], r["y1"]) == (xs.min(), ys.min(), xs.max(), ys.max()) and r["area"] == len(xs) == 24 * 24
        assert r["n_flow"] == r["area"] and r["sum_qu"] == -256 * r["n_flow"] and r["sum_qv"] == 512 * r["n_flow"]
        assert r["velocity"] == (-1.0, 2.0) and r["centroid"] == (xs.mean(), ys.mean())
        assert np.array_equal(labels == 1, inside)
        assert (ids, ages, nxt) == ([1], [k], 2), (k, ids, ages, nxt)
        car = io.objects_carry_host(labels, bu, bv, occ2)
    assert k == 6


# ---- 3. ABI: arguments and states ----

NAMES = ["eppm_objects_default_params", "eppm_objects_create", "eppm_objects_create_size", "eppm_objects_destroy", "eppm_objects_reset",
         "eppm_objects_step", "eppm_objects_step_frames", "eppm_objects_get", "eppm_objects_get_labels", "eppm_objects_get_state",
         "eppm_objects_set_state", "eppm_objects_label_host", "eppm_objects_carry_host", "eppm_objects_assign_host"]


def test_header_declares_the_detector_and_arguments_are_checked():
    hdr = open(os.path.join(ROOT, "include", "eppm.h")).read()
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS
    for s in ("ObjectsParams", "ObjectDetector", "detect_objects", "detect_objects_sequences"):
        assert hasattr(eppm_amd, s), s
    L = eppm_amd.lib()
    p = _lib.CObjectsParams()
    assert L.eppm_objects_default_params(C.byref(p)) == 0
    assert (p.tau, p.iters, p.connectivity, p.min_area, p.max_objects, p.min_overlap) == (1.0, 3, 8, 16, 64, 4)
    assert L.eppm_objects_default_params(None) == ARG
    q = eppm_amd.ObjectsParams(min_area=5)
    assert (q.connectivity, q.min_area) == (8, 5)
    with pytest.raises(TypeError):
        eppm_amd.ObjectsParams(smooth=0.5)
    out = C.c_void_p()
    assert L.eppm_objects_create(None, None, C.byref(out)) == ARG
    assert L.eppm_objects_create_size(4, 4, 1, 0, None, None) == ARG
    # section 16's frame bounds, before the device is touched
    for h, w, n in ((0, 4, 1), (4, -1, 1), (4, 4, 0), (4, 4, 4097), (65536, 65536, 1), (8193, 4, 1), (4, 8193, 1), (8192, 8200, 1)):
        assert L.eppm_objects_create_size(h, w, n, 0, None, C.byref(out)) == ARG and not out.value
    assert L.eppm_objects_destroy(None) == 0
    assert L.eppm_objects_reset(None, 0) == ARG
    assert L.eppm_objects_step(None, None, None) == ARG
    assert L.eppm_objects_step_frames(None, 0, None, None, None, None, 0) == ARG
    assert L.eppm_objects_get(None, 0, 0, None, None) == ARG and L.eppm_objects_get_labels(None, 0, None) == ARG
    assert L.eppm_objects_get_state(None, 0, None, None, None, None) == ARG
    assert L.eppm_objects_set_state(None, 0, None, None, None, 1) == ARG
    # the parameter limits, through the host form and through create
    h, w = 4, 5
    mask, z, lab = np.ones((h, w), np.uint8), np.zeros((h, w), F), np.zeros((h, w), np.uint8)
    rec, cnt = (_lib.CObject * 255)(), _lib.CObjectsCounts()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)              # noqa: E731
    inf, nan = float("inf"), float("nan")
    for vals, ok in (((1.0, 3, 8, 16, 64, 4), True), ((1.0, 1, 4, 1, 1, 1), True), ((3e38, 8, 8, 2 ** 31 - 1, 255, 2 ** 31 - 1), True),
                     ((1.0, 3, 6, 16, 64, 4), False), ((1.0, 3, 0, 16, 64, 4), False), ((1.0, 3, 8, 0, 64, 4), False),
                     ((1.0, 3, 8, -3, 64, 4), False), ((1.0, 3, 8, 16, 0, 4), False), ((1.0, 3, 8, 16, 256, 4), False),
                     ((1.0, 3, 8, 16, 64, 0), False), ((0.0, 3, 8, 16, 64, 4), False), ((-1.0, 3, 8, 16, 64, 4), False),
                     ((inf, 3, 8, 16, 64, 4), False), ((nan, 3, 8, 16, 64, 4), False), ((1.0, 0, 8, 16, 64, 4), False),
                     ((1.0, 9, 8, 16, 64, 4), False)):
        pp = _lib.CObjectsParams(*vals)
        assert (L.eppm_objects_label_host(C.byref(pp), ptr(mask), ptr(z), ptr(z), h, w, ptr(lab), rec, C.byref(cnt)) == 0) == ok, vals
        if not ok:
            assert L.eppm_objects_create_size(h, w, 1, 0, C.byref(pp), C.byref(out)) == ARG and not out.value, vals
    good = [C.byref(p), ptr(mask), ptr(z), ptr(z)]
    tail = [ptr(lab), rec, C.byref(cnt)]
    for k in range(7):
        a = good + tail
        a[k] = None
        assert L.eppm_objects_label_host(*a[:4], h, w, *a[4:]) == ARG, k
    assert L.eppm_objects_label_host(*good, 0, w, *tail) == ARG and L.eppm_objects_label_host(*good, 8193, 4, *tail) == ARG
    car = np.zeros((h, w), np.uint8)
    cg = [ptr(lab), ptr(z), ptr(z), ptr(car)]
    assert L.eppm_objects_carry_host(*cg, h, w, ptr(mask)) == 0
    for k in range(4):
        a = list(cg)
        a[k] = None
        assert L.eppm_objects_carry_host(*a, h, w, ptr(mask)) == ARG, k
    assert L.eppm_objects_carry_host(*cg, h, w, None) == ARG and L.eppm_objects_carry_host(*cg, h, w, ptr(lab)) == ARG          # gathers: not in place
    assert L.eppm_objects_carry_host(*cg, h, 0, ptr(mask)) == ARG
    pid, page, nxt = np.zeros(256, np.int32), np.zeros(256, np.int32), C.c_int32(1)
    ag = [C.byref(p), ptr(lab), ptr(car)]
    at = [ptr(pid), ptr(page), C.byref(nxt), rec]
    assert L.eppm_objects_assign_host(*ag, h, w, 0, *at) == 0
    assert L.eppm_objects_assign_host(ag[0], ag[1], None, h, w, 0, *at) == 0                  # carried NULL: all zero
    assert L.eppm_objects_assign_host(*ag, h, w, 0, at[0], at[1], at[2], None) == 0           # no objects, no records
    assert L.eppm_objects_assign_host(*ag, h, w, 1, at[0], at[1], at[2], None) == ARG
    assert L.eppm_objects_assign_host(None, ag[1], ag[2], h, w, 0, *at) == ARG and L.eppm_objects_assign_host(ag[0], None, ag[2], h, w, 0, *at) == ARG
    for k in range(3):
        a = list(at)
        a[k] = None
        assert L.eppm_objects_assign_host(*ag, h, w, 0, *a) == ARG, k
    assert L.eppm_objects_assign_host(*ag, h, w, -1, *at) == ARG and L.eppm_objects_assign_host(*ag, h, w, 65, *at) == ARG
    for bad in (0, -5, 2 ** 30 + 1, 2 ** 31 - 1):
        nxt.value = bad
        assert L.eppm_objects_assign_host(*ag, h, w, 0, *at) == ARG, bad
    nxt.value = 2 ** 30
    assert L.eppm_objects_assign_host(*ag, h, w, 0, *at) == 0
    page[7] = -1
    assert L.eppm_objects_assign_host(*ag, h, w, 0, *at) == ARG
    with pytest.raises(eppm_amd.EppmError):
        io.objects_label_host(mask, z, z, connectivity=5)
    with pytest.raises(ValueError):
        io.objects_label_host(mask, z[:2], z)


def test_no_input_reads_outside_a_plane():
    """labels, vectors and carried bytes of every value on planes of their exact size: the host forms return what the restatement says"""
    rng = np.random.default_rng(5)
    for k in range(30):
        h, w = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        lab = rng.integers(0, 256, (h, w)).astype(np.uint8)
        bu = SPECIAL[rng.integers(0, len(SPECIAL), (h, w))] * F(rng.choice([1, -1, 0.001]))
        bv = SPECIAL[rng.integers(0, len(SPECIAL), (h, w))]
        occ = (rng.integers(0, 256, (h, w)) * (rng.random((h, w)) < 0.3)).astype(np.uint8)
        assert np.array_equal(io.objects_carry_host(lab, bu, bv, occ), np_carry(lab, bu, bv, occ))
        M = int(rng.choice([1, 3, 255]))
        n = int(rng.integers(0, M + 1))
        cur = rng.integers(0, n + 1, (h, w)).astype(np.uint8)
        pid, page = rng.integers(-2 ** 31, 2 ** 31, 256).astype(np.int32), rng.integers(0, 2 ** 30, 256).astype(np.int32)
        want = np_assign(cur, lab, n, pid, page, 17, M, 1)
        got = io.objects_assign_host(cur, n, lab, pid, page, 17, M, 1)
        assert (got[0], got[1], got[4]) == (want[0], want[1], want[4])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])


def test_semantics_under_sanitizers(tmp_path):
    """objects.h -- the per-pixel functions and the three host forms -- under ASan + UBSan + float-cast checks on exactly sized planes
    (tests/csrc/objects_sanitize_driver.cpp, a program of its own, built without HIP)"""
    exe = str(tmp_path / "objects_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "objects_sanitize_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
