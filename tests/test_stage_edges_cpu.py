"""Input builders and ledger of tests/test_stage_edges_gpu.py: adversarial stage parity for the prepare kernels (k_prepare.hip) and the
level-2 post kernels (k_post.hip).

The stage tests of test_parity_gpu.py give these kernels one natural input, the 160x120 crop whose level-2 plane is 40x30: under one
64-wide tile, a multiple of every tile height, with out-of-range targets only at x == w / y == h and never a pixel with exactly one
negative component.  Here every input is BUILT: a pure function of the shape and a fixed seed that plants the situations in which these
kernels can go wrong.  This file runs without a GPU.  For every shape it asserts, from the inputs and the CPU oracle's outputs alone,
that each planted situation does occur (the ledger): a GPU test then cannot pass by missing its branch.  A situation that a shape
cannot produce is named in EXEMPT; only the three degenerate shapes may have exemptions."""
import functools

import numpy as np
import pytest

KINV = -10000                      # kInvalid / INVALID_LOCATION
VOTE_R, VOTE_THRESH, SIM_THRESH = 6, 84, 2
WMF_R = 4

# (w, h).  75x21: two 64-wide and three 32-wide tiles (the last ragged by 11), three 8-tall tiles (ragged by 5), six 4-tall tiles (ragged
# by 1): halos cross interior tile borders in both directions.  5x3: smaller than every halo (blur radius 6, 13x13 vote, 9x9 median).
# 1x37 and 70x1: one-pixel column / row, every clamp active.
FULL = (75, 21)
SHAPES = (FULL, (5, 3), (1, 37), (70, 1))
PREPARE_SHAPES = SHAPES + ((160, 120),)
sid = lambda s: "%dx%d" % s  # noqa: E731


def _O():
    from oracle import oracle
    return oracle


def short2(x, y):
    O = _O()
    x, y = np.asarray(x), np.asarray(y)
    a = np.zeros(x.shape, O.short2)
    a["x"], a["y"] = x.astype(np.int16), y.astype(np.int16)
    return a


def low_contrast(w, h, seed):
    """a guide image whose range weights stay non-zero"""
    rng = np.random.default_rng([w, h, seed])
    return _O().rgb2rgba(rng.integers(96, 104, (h, w, 3), dtype=np.uint8))


def grid(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs, ys


# a situation a shape cannot produce, by stage: {shape: {situation: why}}
EXEMPT = {
    "outlier": {s: {k: "a 13x13 window holds at most %d pixels of this plane: no vote reaches 83" % (min(13, s[0]) * min(13, s[1]))
                    for k in ("vote83_full", "vote84_full", "vote85_full", "vote83_cut", "vote84_cut", "vote85_cut", "kept_by_diff2", "dropped_by_diff3",
                              "kept_by_wrap", "kept_one_negative")} for s in SHAPES[1:]},
    "wmf": {(5, 3): {"taps_over_64": "15 pixels", "progressive": "every pixel lies within the window of the valid columns: one launch fills all"},
            (1, 37): {"taps_over_64": "a window holds at most 9 pixels"},
            (70, 1): {"taps_over_64": "a window holds at most 9 pixels"}},
    "fill": {(5, 3): {"far_over_64": "no run of 64 pixels"},
             (1, 37): {"far_over_64": "no run of 64 pixels", "missing_1": "left and right are always missing"},
             (70, 1): {"missing_1": "up and down are always missing"}},
    "nnf2flow": {(5, 3): {"both": "15 pixels hold the 14 one-component cases; the cases with both components set need 7 more"}},
}


def check_ledger(stage, shape, counts):
    """every situation of `counts` occurs unless the shape is exempt from it; an exemption is never granted on the full shape, and an
    exempt situation must indeed be absent (else the table is stale)"""
    ex = EXEMPT.get(stage, {}).get(shape, {})
    assert shape != FULL or not ex
    for k in ex:
        assert k in counts, f"{stage} {sid(shape)}: exemption for an unknown situation {k}"
    missing = [k for k, n in counts.items() if n == 0 and k not in ex]
    assert not missing, f"{stage} {sid(shape)}: planted situations that do not occur: {missing}"
    stale = [k for k in ex if counts[k] != 0]
    assert not stale, f"{stage} {sid(shape)}: exempt situations that do occur: {stale}"


# =========================================================================================================================================
# 2a. left-right check
# =========================================================================================================================================
LR_KINDS = ("roundtrip", "off_x", "off_y", "at_w", "at_h", "neg_x", "neg_y", "far_x", "far_y", "invalid", "roundtrip2")


@functools.lru_cache(None)
def lr_inputs(w, h):
    """(nnf1, cost1, nnf2, cost2).  A random bijection of the pixels makes every target round-trip (and every pixel, the last row and
    column included, a target); then pixel k of a random order gets kind k mod len(LR_KINDS): its nnf2 entry is moved by one in x or in
    y, or its own target is put at x == w, at y == h, at a negative x or y, far outside (w + 300, h + 40) or at kInvalid."""
    rng = np.random.default_rng([w, h, 11])
    n = w * h
    P = rng.permutation(n)                                   # nnf1[p] = P[p], nnf2[P[p]] = p
    x1, y1 = (P % w).astype(np.int64), (P // w).astype(np.int64)
    x2, y2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    x2[P], y2[P] = np.arange(n) % w, np.arange(n) // w
    # (the pixel of the last row and column stays a round trip's target)
    for k, p in enumerate([p for p in rng.permutation(n) if P[p] != n - 1]):
        kind = LR_KINDS[k % len(LR_KINDS)]
        q = P[p]
        if kind == "off_x": x2[q] += 1 if k % 2 else -1
        elif kind == "off_y": y2[q] += 1 if k % 2 else -1
        elif kind == "at_w": x1[p] = w
        elif kind == "at_h": y1[p] = h
        elif kind == "neg_x": x1[p] = -1 - (k % 3)
        elif kind == "neg_y": y1[p] = -1 - (k % 3)
        elif kind == "far_x": x1[p] = w + 300
        elif kind == "far_y": y1[p] = h + 40
        elif kind == "invalid": x1[p] = y1[p] = KINV
    nnf1, nnf2 = short2(x1.reshape(h, w), y1.reshape(h, w)), short2(x2.reshape(h, w), y2.reshape(h, w))
    c1, c2 = rng.random((h, w), dtype=np.float32), rng.random((h, w), dtype=np.float32)
    return nnf1, c1, nnf2, c2


def lr_ledger(w, h):
    O = _O()
    nnf1, c1, nnf2, c2 = lr_inputs(w, h)
    a, b, c, d = O.left_right_check(nnf1, c1, nnf2, c2)
    xs, ys = grid(w, h)
    tx, ty = nnf1["x"].astype(int), nnf1["y"].astype(int)
    inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
    ex = np.where(inside, nnf2["x"][np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], 0).astype(int)
    ey = np.where(inside, nnf2["y"][np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], 0).astype(int)
    trip = inside & (ex == xs) & (ey == ys)
    # the second pass: nnf2's target p lies inside, and nnf1[p] was valid on entry and carries the first pass's mark now
    ux, uy = nnf2["x"].astype(int), nnf2["y"].astype(int)
    in2 = (ux >= 0) & (ux < w) & (uy >= 0) & (uy < h)
    cy, cx = np.clip(uy, 0, h - 1), np.clip(ux, 0, w - 1)
    marked = in2 & (a["x"][cy, cx] == KINV) & (nnf1["x"][cy, cx] != KINV)
    counts = {
        "roundtrip": int(trip.sum()),
        "off_by_one_x_only": int((inside & (np.abs(ex - xs) == 1) & (ey == ys)).sum()),
        "off_by_one_y_only": int((inside & (np.abs(ey - ys) == 1) & (ex == xs)).sum()),
        "last_row": int((trip & (ty == h - 1)).sum()),
        "last_column": int((trip & (tx == w - 1)).sum()),
        "x_eq_w": int(((tx == w) & (ty >= 0) & (ty < h)).sum()),
        "y_eq_h": int(((ty == h) & (tx >= 0) & (tx < w)).sum()),
        "negative_x_only": int(((tx < 0) & (ty >= 0) & (ty < h)).sum()),
        "negative_y_only": int(((ty < 0) & (tx >= 0) & (tx < w)).sum()),
        "far_x": int((tx == w + 300).sum()),
        "far_y": int((ty == h + 40).sum()),
        "at_invalid": int(((tx == KINV) & (ty == KINV)).sum()),
        "second_pass_sees_mark": int(marked.sum()),
        # what the oracle made of them
        "kept": int((a["x"] != KINV).sum()),
        "kept2": int((c["x"] != KINV).sum()),
    }
    # the oracle keeps exactly the round trips, with their cost, and marks the rest
    assert np.array_equal(a["x"] != KINV, trip) and np.array_equal(b == np.float32(np.finfo(np.float32).max), ~trip)
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_lr_ledger(shape):
    check_ledger("lr", shape, lr_ledger(*shape))


# =========================================================================================================================================
# 2b. outlier removal
# =========================================================================================================================================
def rel16(nnf):
    """relative flows in the reference's short arithmetic"""
    h, w = nnf.shape
    xs, ys = grid(w, h)
    return (nnf["x"].astype(np.int64) - xs).astype(np.int16).astype(np.int64), (nnf["y"].astype(np.int64) - ys).astype(np.int16).astype(np.int64)


def votes(fx, fy, sim=SIM_THRESH):
    """(count, window size) per pixel of the 13x13 vote on the relative flows fx, fy"""
    h, w = fx.shape
    cnt, win = np.zeros((h, w), int), np.zeros((h, w), int)
    for dy in range(-VOTE_R, VOTE_R + 1):
        for dx in range(-VOTE_R, VOTE_R + 1):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            c, n = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            cnt[c] += (np.abs(fx[n] - fx[c]) <= sim) & (np.abs(fy[n] - fy[c]) <= sim)
            win[c] += 1
    return cnt, win


def votes_of_mask(mask):
    """per pixel, the number of set pixels of mask in its 13x13 window"""
    h, w = mask.shape
    out = np.zeros((h, w), int)
    for dy in range(-VOTE_R, VOTE_R + 1):
        for dx in range(-VOTE_R, VOTE_R + 1):
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] += mask[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


@functools.lru_cache(None)
def outlier_inputs(w, h):
    """(nnf, cost).  Background: every pixel its own relative flow (5x, 5y), so nothing agrees by accident.  On a plane that holds them
    (48x21 at least): 12x7 blocks of one relative flow each -- a pixel at a block's centre columns sees the whole block, so its vote is
    the block's size: 83, 84 and 85, in the interior (full window) and against the top edge (cut window); blocks whose 84 votes hold
    four at a distance of exactly 2 (kept) or exactly 3 (dropped); a block whose targets all have a negative x; a block whose relative
    flow is coherent only after the int16 wrap of nnf - x.  Sprinkled everywhere else: both-negative pixels (skipped), one-negative pixels
    (voted on), adjacent kInvalid pixels, and an adjacent 32767 / -32768 pair that agrees only through the wrap."""
    rng = np.random.default_rng([w, h, 12])
    xs, ys = grid(w, h)
    tx, ty = 6 * xs, 6 * ys                                     # relative flow (5x, 5y)
    free = np.ones((h, w), bool)
    if w >= 48 and h >= 21:
        def block(x0, y0, fx, fy, size, extra_row):
            sl = (slice(y0, y0 + 7), slice(x0, x0 + 12))
            tx[sl], ty[sl] = xs[sl] + fx, ys[sl] + fy
            free[sl] = False
            if size == 83:                                      # a corner pixel goes back to the background
                tx[y0, x0], ty[y0, x0] = 6 * x0, 6 * y0
            if size == 85:                                      # one more pixel, in the row past the block, under its centre
                tx[extra_row, x0 + 5], ty[extra_row, x0 + 5] = x0 + 5 + fx, extra_row + fy
                free[extra_row, x0 + 5] = False
            return sl
        for k, size in enumerate((83, 84, 85)):
            block(12 * k, 0, 0, 200 + 10 * k, size, 7)          # against the top edge (the first also against the left edge)
            block(36 + 12 * k, 7, 0, 300 + 10 * k, size, 14)    # interior rows 7..13: the centre row's window is rows 4..16
        for k, off in enumerate((2, 3)):                        # 80 pixels + the four corners at a distance of exactly `off`
            sl = block(12 * k, 14, 7, 400 + 10 * k, 84, None)
            cy, cx = [sl[0].start, sl[0].stop - 1], [sl[1].start, sl[1].stop - 1]
            tx[cy[0], cx[0]] += off; tx[cy[1], cx[1]] -= off; ty[cy[0], cx[1]] += off; ty[cy[1], cx[0]] -= off
        block(24, 14, -100, 450, 84, None)                      # every target x negative: not skipped, kept
        sl = block(36, 14, 32767 - 41, 17, 84, None)            # columns 36..41: 32767 - 41 + x <= 32767; columns 42..47 wrap to -32768 + ...
        assert (tx[sl] > 32767).sum() == 42
    # sprinkles on the free pixels, in a fixed random order
    fy_, fx_ = np.nonzero(free)
    order = rng.permutation(len(fx_))
    pts = [(int(fx_[i]), int(fy_[i])) for i in order]
    # adjacent pairs on free pixels: kInvalid next to kInvalid; 32767 next to -32768 (along x when the plane has two columns, else along y)
    dx, dy = (1, 0) if w > 1 else (0, 1)
    def pair():
        for (x, y) in pts[::-1]:
            if x + dx < w and y + dy < h and free[y, x] and free[y + dy, x + dx]:
                free[y, x] = free[y + dy, x + dx] = False
                return x, y, x + dx, y + dy
        raise AssertionError("no free pair left")
    x, y, xn, yn = pair()
    tx[y, x] = ty[y, x] = tx[yn, xn] = ty[yn, xn] = KINV
    x, y, xn, yn = pair()
    if w > 1:
        tx[y, x], tx[yn, xn] = 32767, -32768
        ty[y, x] = ty[yn, xn] = y + 1
    else:
        ty[y, x], ty[yn, xn] = 32767, -32768
        tx[y, x] = tx[yn, xn] = 0
    for off in (2, 3):                                          # neighbours whose relative flows differ by exactly 2, by exactly 3
        x, y, xn, yn = pair()
        tx[y, x], ty[y, x] = x + 40, y + 40 * off
        tx[yn, xn], ty[yn, xn] = xn + 40 + (off if w > 1 else 0), yn + 40 * off - (0 if w > 1 else off)
    kinds = ("both_neg_invalid", "both_neg_other", "neg_x", "neg_y")
    for k, (x, y) in enumerate([q for q in pts if free[q[1], q[0]]][:max(4, len(pts) // 8)]):
        kind = kinds[k % 4]
        if kind == "both_neg_invalid": tx[y, x] = ty[y, x] = KINV
        elif kind == "both_neg_other": tx[y, x], ty[y, x] = -1 - k % 5, -3
        elif kind == "neg_x": tx[y, x] = -2 - k % 7
        else: ty[y, x] = -1 - k % 7
    tx = ((tx + 32768) % 65536 - 32768)                         # the block that relies on the wrap stores the wrapped targets
    return short2(tx, ty), rng.random((h, w), dtype=np.float32)


def outlier_ledger(w, h):
    O = _O()
    nnf, cost = outlier_inputs(w, h)
    on, oc = O.outlier_removal(nnf, cost)
    X, Y = nnf["x"].astype(int), nnf["y"].astype(int)
    skipped = (X < 0) & (Y < 0)
    voted = ~skipped
    one_neg = (X < 0) ^ (Y < 0)
    fx, fy = rel16(nnf)
    cnt, win = votes(fx, fy)
    cnt1, _ = votes(fx, fy, SIM_THRESH - 1)
    cnt3, _ = votes(fx, fy, SIM_THRESH + 1)
    xs, ys = grid(w, h)
    nowrap, _ = votes(X - xs, Y - ys)                           # the same vote without the short arithmetic
    full = win == 169
    kept = voted & (cnt >= VOTE_THRESH)
    # the restated vote is the oracle's decision
    assert np.array_equal(on["x"] == KINV, (voted & ~kept) | (X == KINV) & skipped)
    assert np.array_equal(on[skipped], nnf[skipped]) and np.array_equal(on[kept], nnf[kept])
    inv = (X == KINV) & (Y == KINV)
    adj = np.zeros((h, w), bool)
    adj[:, :-1] |= inv[:, :-1] & inv[:, 1:]
    adj[:-1, :] |= inv[:-1, :] & inv[1:, :]
    # per voted pixel: kInvalid pixels in its window that have a kInvalid neighbour (their relative flows differ by one: they agree)
    near_adj = votes_of_mask(adj)
    wraps = (X - xs < -32768) | (Y - ys < -32768)
    counts = {
        "vote83_full": int((voted & full & (cnt == 83)).sum()), "vote84_full": int((voted & full & (cnt == 84)).sum()),
        "vote85_full": int((voted & full & (cnt == 85)).sum()),
        "vote83_cut": int((voted & ~full & (cnt == 83)).sum()), "vote84_cut": int((voted & ~full & (cnt == 84)).sum()),
        "vote85_cut": int((voted & ~full & (cnt == 85)).sum()),
        "kept_by_diff2": int((kept & (cnt1 < VOTE_THRESH)).sum()),            # a neighbour at a distance of exactly 2 decides: kept
        "dropped_by_diff3": int((voted & ~kept & (cnt3 >= VOTE_THRESH)).sum()),  # one at exactly 3 would have: dropped
        "diff_exactly_2": int((cnt > cnt1).sum()), "diff_exactly_3": int((cnt3 > cnt).sum()),
        "skipped_invalid": int((skipped & inv).sum()), "skipped_other_negative": int((skipped & ~inv).sum()),
        "one_negative_voted": int((one_neg & voted).sum()),
        "kept_one_negative": int((one_neg & kept).sum()),
        "invalid_neighbours_agree": int((voted & (near_adj >= 1)).sum()),
        "wrap": int(wraps.sum()),
        "wrap_pair_agrees": int((voted & (cnt > nowrap)).sum()),
        "kept_by_wrap": int((kept & (nowrap < VOTE_THRESH)).sum()),
    }
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_outlier_ledger(shape):
    check_ledger("outlier", shape, outlier_ledger(*shape))


# =========================================================================================================================================
# 2c. weighted median
# =========================================================================================================================================
WMF_RUNS = ((1, True), (2, True), (3, True), (20, True), (1, False), (3, False))     # (launches, occlusion only)


def invalid_px(nnf):
    return (nnf["x"] < 0) | (nnf["y"] < 0)


@functools.lru_cache(None)
def wmf_fields(w, h):
    """{name: (nnf, img)}.
    front:    low contrast; only the first two columns (rows, on a one-column plane) are valid: four more are filled per launch, the
              list shrinks from launch to launch and every filled pixel is carried one launch as "copy only"; some valid pixels have one
              negative component (skipped as taps, processed as centres).
    dense:    all valid but for isolated invalid pixels (kInvalid, negative x only, negative y only): windows with more than 64 valid taps.
    tie:      constant colour; all invalid but two columns (rows) two pixels either side of the middle one, each of one flow: for the
              pixels between them the two candidates' costs are one product each, of equal weights: an exact tie, the first in row-major
              order must win.
    rejected: only the last column (row) is valid and its relative flow maps every other pixel to a negative target: every winner is
              rejected, the first launch changes nothing and the remaining ones take the early exit.
    zero:     a one-pixel checker of 0 and 255; the black pixels are invalid, the white ones valid: every range weight of an invalid
              centre's window underflows to 0, weightSum == 0."""
    O = _O()
    rng = np.random.default_rng([w, h, 13])
    xs, ys = grid(w, h)
    along_x = w > 1
    out = {}
    # front
    tx, ty = np.full((h, w), KINV), np.full((h, w), KINV)
    first = (xs < 2) if along_x else (ys < 2)
    tx[first] = (xs + rng.integers(0, 4, (h, w)))[first]
    ty[first] = (ys + rng.integers(0, 4, (h, w)))[first]
    if along_x and h > 2:
        tx[h // 2, 1] = -1                                       # one negative component among the valid columns
    out["front"] = (short2(tx, ty), low_contrast(w, h, 1))
    # dense
    tx, ty = xs + 2 + (xs // 7) % 3, ys + 1 + (ys // 5) % 2
    n = w * h
    holes = rng.permutation(n)[:max(3, n // 60)]
    for k, p in enumerate(holes):
        y, x = divmod(int(p), w)
        if k % 3 == 0: tx[y, x] = ty[y, x] = KINV
        elif k % 3 == 1: tx[y, x] = -1
        else: ty[y, x] = -2
    if w >= 9 and h >= 9:                                        # one hole whose whole window lies inside the plane
        tx[h // 2, w // 2] = ty[h // 2, w // 2] = KINV
    out["dense"] = (short2(tx, ty), low_contrast(w, h, 2))
    # tie
    tx, ty = np.full((h, w), KINV), np.full((h, w), KINV)
    if along_x:
        c = w // 2
        tx[:, c - 2], ty[:, c - 2] = xs[:, c - 2] + 3, ys[:, c - 2] + 1
        tx[:, c + 2], ty[:, c + 2] = xs[:, c + 2] - 2, ys[:, c + 2] + 4
    else:
        c = h // 2
        tx[c - 2], ty[c - 2] = xs[c - 2] + 3, ys[c - 2] + 1
        tx[c + 2], ty[c + 2] = xs[c + 2] + 1, ys[c + 2] - 2
    grey = np.zeros((h, w, 3), np.uint8) + np.uint8(100)
    out["tie"] = (short2(tx, ty), O.rgb2rgba(grey))
    # rejected
    tx, ty = np.full((h, w), KINV), np.full((h, w), KINV)
    if along_x:
        tx[:, w - 1], ty[:, w - 1] = 0, ys[:, w - 1]
    else:
        tx[h - 1], ty[h - 1] = 0, 0
    out["rejected"] = (short2(tx, ty), low_contrast(w, h, 3))
    # zero
    white = (xs + ys) % 2 == 1
    tx, ty = np.where(white, xs + 1, KINV), np.where(white, ys + 2, KINV)
    chk = np.zeros((h, w, 3), np.uint8)
    chk[white] = 255
    out["zero"] = (short2(tx, ty), O.rgb2rgba(chk))
    return out


def wmf_weights(img, x, y):
    """numpy restatement of the bilateral weight (refine :198-204) of every tap of (x, y)'s window inside the image: {(dx, dy): float32}"""
    O = _O()
    h, w = img.shape
    g = O.wmf_lut()
    u = lambda p: np.array([p["x"], p["y"], p["z"]], np.float32) / np.float32(255)  # noqa: E731
    c = u(img[y, x])
    out = {}
    for dy in range(-WMF_R, WMF_R + 1):
        for dx in range(-WMF_R, WMF_R + 1):
            cy, cx = y + dy, x + dx
            if 0 <= cx < w and 0 <= cy < h:
                d = np.abs(c - u(img[cy, cx])).max().astype(np.float32)
                coef_r = O.fast_exp(np.array([-(d * d) / (np.float32(0.02) * np.float32(0.02))], np.float32))[0]
                out[(dx, dy)] = np.float32(coef_r * np.float32(g[abs(dx)] * g[abs(dy)]))
    return out


@functools.lru_cache(None)
def wmf_oracle(w, h, name, iters, only_occ):
    nnf, img = wmf_fields(w, h)[name]
    return _O().weighted_median(nnf, img, iters, only_occ)


def wmf_ledger(w, h):
    F = wmf_fields(w, h)
    counts = {}

    def taps(nnf, x, y):
        return [(dx, dy) for dy in range(-WMF_R, WMF_R + 1) for dx in range(-WMF_R, WMF_R + 1)
                if 0 <= x + dx < w and 0 <= y + dy < h and nnf["x"][y + dy, x + dx] >= 0 and nnf["y"][y + dy, x + dx] >= 0]

    # front: progress over at least three launches, the carry, short windows, one-negative taps
    nnf, img = F["front"]
    valid = [int((~invalid_px(wmf_oracle(w, h, "front", k, True))).sum()) for k in (1, 2, 3)]
    v0 = int((~invalid_px(nnf)).sum())
    counts["progressive"] = int(v0 < valid[0] < valid[1] < valid[2])
    inv = np.argwhere(invalid_px(nnf))
    ntap = {(int(x), int(y)): len(taps(nnf, int(x), int(y))) for y, x in inv}
    counts["taps_1_to_64"] = sum(1 for n in ntap.values() if 1 <= n <= 64)
    one_neg = (nnf["x"] < 0) ^ (nnf["y"] < 0)
    counts["one_negative_tap_skipped"] = int(sum(1 for y, x in inv if one_neg[max(0, y - WMF_R):y + WMF_R + 1, max(0, x - WMF_R):x + WMF_R + 1].any()
                                                 and ntap[(int(x), int(y))] > 0))
    # dense: windows with more than 64 valid taps (both lane halves hold candidates)
    nnf, img = F["dense"]
    inv = np.argwhere(invalid_px(nnf))
    counts["taps_over_64"] = sum(1 for y, x in inv if len(taps(nnf, int(x), int(y))) > 64)
    o1 = wmf_oracle(w, h, "dense", 1, True)
    counts["dense_filled"] = int((invalid_px(nnf) & ~invalid_px(o1)).sum())
    d1 = (nnf["x"] < 0) ^ (nnf["y"] < 0)
    counts["one_negative_centre"] = int(d1.sum())
    if not counts["one_negative_tap_skipped"]:
        counts["one_negative_tap_skipped"] = int(d1.sum() and len(inv) > 1)
    # tie: two candidates, one product each, equal weights, different flows; the first in row-major order wins
    nnf, img = F["tie"]
    o1 = wmf_oracle(w, h, "tie", 1, True)
    ties = 0
    for y, x in np.argwhere(invalid_px(nnf)):
        t = taps(nnf, int(x), int(y))
        flows = [(int(nnf["x"][y + dy, x + dx]) - (x + dx), int(nnf["y"][y + dy, x + dx]) - (y + dy)) for dx, dy in t]
        if len(set(flows)) != 2 or flows.count(flows[0]) * 2 != len(flows):
            continue
        wg = wmf_weights(img, int(x), int(y))
        a = [wg[p] for p, f in zip(t, flows) if f == flows[0]]
        b = [wg[p] for p, f in zip(t, flows) if f != flows[0]]
        if a == b and all(v > 0 for v in a):                     # the same weights in the same order: the sequential sums are the same floats
            ties += 1
            assert (int(o1["x"][y, x]), int(o1["y"][y, x])) == (x + flows[0][0], y + flows[0][1]), "the first candidate wins the tie"
    counts["exact_tie"] = ties
    # rejected: every invalid pixel with valid taps of non-zero weight stays invalid, for ever
    nnf, img = F["rejected"]
    o20 = wmf_oracle(w, h, "rejected", 20, True)
    assert np.array_equal(o20, nnf)
    rej = 0
    for y, x in np.argwhere(invalid_px(nnf)):
        t = taps(nnf, int(x), int(y))
        if t and all(int(nnf["x"][y + dy, x + dx]) - dx < 0 or int(nnf["y"][y + dy, x + dx]) - dy < 0 for dx, dy in t):
            wg = wmf_weights(img, int(x), int(y))
            rej += sum(wg[p] for p in t) > 0
    counts["winner_rejected"] = int(rej)
    # zero: weightSum == 0
    nnf, img = F["zero"]
    o20 = wmf_oracle(w, h, "zero", 20, True)
    assert np.array_equal(o20, nnf)
    zero = 0
    for y, x in np.argwhere(invalid_px(nnf)):
        t = taps(nnf, int(x), int(y))
        wg = wmf_weights(img, int(x), int(y))
        zero += bool(t) and all(wg[p] == 0 for p in t)
    counts["weight_sum_zero"] = int(zero)
    # all pixels, three launches: untested before; it must differ from one launch somewhere, or it tests nothing more
    counts["all_pixels_3_differs_from_1"] = int(sum((wmf_oracle(w, h, n, 3, False) != wmf_oracle(w, h, n, 1, False)).sum() for n in F))
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_wmf_ledger(shape):
    check_ledger("wmf", shape, wmf_ledger(*shape))


# =========================================================================================================================================
# 2d. hole filling
# =========================================================================================================================================
@functools.lru_cache(None)
def fill_fields(w, h):
    """{name: (nnf, img)}.
    all_invalid: nothing valid in any direction, anywhere.
    cross:       a fully invalid first row and a fully invalid middle column in a valid plane (the pixel where they meet sees nothing in
                 four directions, the others of the row nothing in three, of the column nothing in two), holes against the other edges and
                 in the corners, a 32767 next to a hole (the result wraps), one-negative pixels inside and next to holes.
    run:         the middle row is invalid from the third pixel to the last but one; its left end is a 32767: the nearest valid pixel of the
                 holes at the right end lies more than 64 pixels away, across the tile border, and the result wraps.
    tie:         constant colour, every third pixel of a diagonal pattern a hole: all directions offer the same colour distance, the first
                 in the order left, right, up, down wins."""
    O = _O()
    rng = np.random.default_rng([w, h, 14])
    xs, ys = grid(w, h)

    def valid():
        return xs + rng.integers(0, 9, (h, w)), ys + rng.integers(0, 9, (h, w))
    out = {}
    out["all_invalid"] = (short2(np.full((h, w), KINV), np.full((h, w), KINV)), low_contrast(w, h, 4))
    tx, ty = valid()
    if h > 1:
        tx[0], ty[0] = KINV, KINV
    if w > 1:
        tx[:, w // 2], ty[:, w // 2] = KINV, KINV
    for (x, y) in ((0, h // 2), (w - 1, h // 2), (w // 4, h - 1), (0, h - 1), (w - 1, h - 1), (0, 0), (w - 1, 0), (w // 4, min(1, h - 1))):
        tx[y, x] = ty[y, x] = KINV
    if w >= 5:                                                   # one-negative pixels: holes themselves, and no end of a walk
        y = h // 2
        tx[y, 1] = -1
        tx[y, w - 2], ty[y, w - 2] = w, -3
    if h >= 5:
        x = w // 4
        ty[h - 2, x] = -1
    if w >= 5:
        tx[h - 1, w // 4 + 1] = 32767                            # right of the hole at (w // 4, h - 1): nothing wraps; left of ...
        tx[h - 1, w - 2] = 32767                                 # ... the corner hole (w - 1, h - 1): 32767 + 1 wraps
    else:
        ty[max(h - 2, 0), 0] = 32767
    out["cross"] = (short2(tx, ty), low_contrast(w, h, 5))
    tx, ty = valid()
    if w > 4:
        y = h // 2
        tx[y, 2:w - 1] = KINV; ty[y, 2:w - 1] = KINV
        tx[y, 1] = 32767
        tx[y, 5 % (w - 1) or 2] = -5; ty[y, 5 % (w - 1) or 2] = 3          # a one-negative pixel inside the run
    else:
        x = w // 2
        tx[2:h - 1, x] = KINV; ty[2:h - 1, x] = KINV
        ty[1, x] = 32767
        if h > 7:
            ty[5, x] = 3; tx[5, x] = -5
    out["run"] = (short2(tx, ty), low_contrast(w, h, 6))
    tx, ty = valid()
    hole = (xs + 2 * ys) % 3 == 1
    tx[hole], ty[hole] = KINV, KINV
    grey = np.zeros((h, w, 3), np.uint8) + np.uint8(77)
    out["tie"] = (short2(tx, ty), O.rgb2rgba(grey))
    return out


def fill_walk(nnf, img):
    """Restatement of refine :297-371 for the ledger: per hole, what each direction offers.  Returns a list of dicts."""
    h, w = nnf.shape
    X, Y = nnf["x"].astype(int), nnf["y"].astype(int)
    ok = (X >= 0) & (Y >= 0)
    u = lambda p: np.array([p["x"], p["y"], p["z"]], np.float32) / np.float32(255)  # noqa: E731
    res = []
    for y, x in np.argwhere(~ok):
        y, x = int(y), int(x)
        dirs = []
        for (sx, sy) in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            cx, cy, found, over_one_neg = x + sx, y + sy, None, False
            while 0 <= cx < w and 0 <= cy < h:
                if ok[cy, cx]:
                    found = (cx, cy)
                    break
                over_one_neg |= bool((X[cy, cx] < 0) ^ (Y[cy, cx] < 0))
                cx, cy = cx + sx, cy + sy
            dirs.append((found, over_one_neg))
        best, bestd, tied = None, None, False
        for found, _ in dirs:
            if found is None:
                continue
            d = np.abs(u(img[y, x]) - u(img[found[1], found[0]])).max()
            if best is None or d < bestd:
                best, bestd, tied = found, d, False
            elif d == bestd and (X[found[1], found[0]] - found[0], Y[found[1], found[0]] - found[1]) != (X[best[1], best[0]] - best[0], Y[best[1], best[0]] - best[1]):
                tied = True                                       # a later direction offers the same distance and another flow
        if best is None:
            rx, ry = X[y, x] + x, Y[y, x] + y
        else:
            rx, ry = X[best[1], best[0]] - best[0] + x, Y[best[1], best[0]] - best[1] + y
        res.append(dict(x=x, y=y, missing=sum(f is None for f, _ in dirs), over_one_neg=any(o and f is not None for f, o in dirs), tied=tied,
                        far=max([abs(f[0] - x) + abs(f[1] - y) for f, _ in dirs if f is not None] or [0]),
                        far_crosses_tile=any(f is not None and f[0] // 64 != x // 64 for f, _ in dirs),
                        won_far=best is not None and abs(best[0] - x) + abs(best[1] - y) > 64,
                        result=(rx, ry), wraps=not (-32768 <= rx <= 32767 and -32768 <= ry <= 32767)))
    return res


def fill_ledger(w, h):
    O = _O()
    counts = dict(missing_1=0, missing_2=0, missing_3=0, missing_4=0, all_invalid_plane=0, tie_first_wins=0, far_over_64=0, over_one_negative=0,
                  wraps=0, one_negative_hole=0)
    for name, (nnf, img) in fill_fields(w, h).items():
        want = O.fill_holes(nnf, img)
        walk = fill_walk(nnf, img)
        for r in walk:                                           # the restatement is the oracle's result
            wx, wy = (r["result"][0] + 32768) % 65536 - 32768, (r["result"][1] + 32768) % 65536 - 32768
            assert (int(want["x"][r["y"], r["x"]]), int(want["y"][r["y"], r["x"]])) == (wx, wy), (name, r)
            if 1 <= r["missing"] <= 4:
                counts["missing_%d" % r["missing"]] += 1
            counts["tie_first_wins"] += r["tied"]
            counts["far_over_64"] += r["far"] > 64 and r["far_crosses_tile"]
            counts["over_one_negative"] += r["over_one_neg"]
            counts["wraps"] += r["wraps"]
        counts["one_negative_hole"] += int(((nnf["x"] < 0) ^ (nnf["y"] < 0)).sum())
        if name == "all_invalid":
            counts["all_invalid_plane"] += int(all(r["missing"] == 4 for r in walk) and len(walk) == w * h)
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_fill_ledger(shape):
    check_ledger("fill", shape, fill_ledger(*shape))


# =========================================================================================================================================
# 2e. NNF -> flow
# =========================================================================================================================================
N2F_VALUES = (KINV, KINV + 1, KINV - 1, -1, -32768, 0, 32767)


@functools.lru_cache(None)
def nnf2flow_input(w, h):
    """every value of N2F_VALUES in x only, in y only and in both (first the same value in both, then the mixed pairs), one case per pixel
    in a fixed random pixel order; the other pixels hold ordinary targets"""
    rng = np.random.default_rng([w, h, 15])
    xs, ys = grid(w, h)
    tx, ty = xs + rng.integers(0, 5, (h, w)), ys + rng.integers(0, 5, (h, w))
    cases = [(v, None) for v in N2F_VALUES] + [(None, v) for v in N2F_VALUES] + [(v, v) for v in N2F_VALUES] + \
            [(a, b) for a in N2F_VALUES for b in N2F_VALUES if a != b]
    for (vx, vy), p in zip(cases, rng.permutation(w * h)):
        y, x = divmod(int(p), w)
        if vx is not None: tx[y, x] = vx
        if vy is not None: ty[y, x] = vy
        if vy is None and ty[y, x] in N2F_VALUES: ty[y, x] = y + 1      # (an ordinary target on row / column 0 is a 0)
        if vx is None and tx[y, x] in N2F_VALUES: tx[y, x] = x + 1
    return short2(tx, ty)


def nnf2flow_ledger(w, h):
    nnf = nnf2flow_input(w, h)
    X, Y = nnf["x"].astype(int), nnf["y"].astype(int)
    sx, sy = np.isin(X, N2F_VALUES), np.isin(Y, N2F_VALUES)
    counts = {}
    for v in N2F_VALUES:
        counts["x_only_%d" % v] = int(((X == v) & ~sy).sum())
        counts["y_only_%d" % v] = int(((Y == v) & ~sx).sum())
    counts["both"] = int(all(((X == v) & (Y == v)).any() for v in N2F_VALUES))
    f = _O().nnf2flow(nnf)
    unknown = f["x"] == np.float32(1e10)
    assert np.array_equal(unknown, (X <= KINV) | (Y <= KINV)) and np.array_equal(unknown, f["y"] == np.float32(1e10))
    counts["known_negative"] = int((~unknown & ((X < 0) | (Y < 0))).sum())       # a component in (kInvalid, 0): a known vector
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_nnf2flow_ledger(shape):
    check_ledger("nnf2flow", shape, nnf2flow_ledger(*shape))


# =========================================================================================================================================
# 3. prepare kernels
# =========================================================================================================================================
BLUR_RADII = (0, 2, 6)
TINY_SIGMA = 0.05            # -(1) / (2 * 0.05^2) = -200: every off-centre weight underflows to 0, the sum is the centre's 1
BLUR_SIGMAS = (0.5, 1.0, 2.0, TINY_SIGMA)
BLUR_INPUTS = ("random_rgba", "zeros", "full", "checker")


@functools.lru_cache(None)
def blur_input(name, w, h):
    O = _O()
    a = np.zeros((h, w), O.uchar4)
    if name == "random_rgba":
        rng = np.random.default_rng([w, h, 16])
        for ch in ("x", "y", "z"):
            a[ch] = rng.integers(0, 256, (h, w))
        a["w"] = rng.integers(1, 256, (h, w))                    # alpha: non-zero, varying
    elif name == "full":
        for ch in ("x", "y", "z", "w"):
            a[ch] = 255
    elif name == "checker":
        xs, ys = grid(w, h)
        for ch in ("x", "y", "z", "w"):
            a[ch] = np.where((xs + ys) % 2 == 0, 255, 0)
    return a


def test_blur_ledger():
    O = _O()
    assert set(BLUR_RADII) == {0, 2, 6}
    s2 = np.float32(TINY_SIGMA) * np.float32(TINY_SIGMA) * np.float32(2)
    assert O.fast_exp(np.array([-np.float32(1) / s2], np.float32))[0] == 0        # the nearest off-centre tap, hence all
    assert O.fast_exp(np.array([-np.float32(0) / s2], np.float32))[0] == 1
    for s in (0.5, 1.0, 2.0):
        assert O.fast_exp(np.array([-np.float32(1) / (np.float32(s) * np.float32(s) * 2)], np.float32))[0] > 0
    for (w, h) in PREPARE_SHAPES:
        a = blur_input("random_rgba", w, h)
        assert a["w"].min() >= 1 and (w * h < 4 or len(np.unique(a["w"])) > 1)
        got = O.gauss_filter_rgba(a, 1.0, 2)
        assert (got["w"] > 0).all()                               # the fourth channel is filtered like the others
        full = O.gauss_filter_rgba(blur_input("full", w, h), 2.0, 6)
        assert full["x"].min() >= 254 and np.array_equal(full["x"], full["w"])   # the truncation of 255 * sum / sum
        tiny = O.gauss_filter_rgba(a, TINY_SIGMA, 6)
        assert np.array_equal(tiny, a)


# (name, ratio as the float32 the launcher receives).  The two inexact ratios are formed as a context forms them for the level below an
# odd-width level (ctx_images.cpp: (float)pow(ratio, i) * W[0] / W[j]).
RESIZE_RATIOS = (("half", np.float32(0.5)), ("quarter", np.float32(0.25)), ("one", np.float32(1.0)), ("two", np.float32(2.0)),
                 ("157_over_78", np.float32(0.25) * np.float32(157) / np.float32(78)), ("158_over_39", np.float32(0.125) * np.float32(158) / np.float32(39)))


@functools.lru_cache(None)
def resize_cases():
    """(w, h, name, ratio, outW, outH) with the output size pyr_init_dim gives that ratio; a case whose output plane would be empty is
    no launch and is listed in resize_empty()"""
    O = _O()
    out = []
    for (w, h) in PREPARE_SHAPES:
        for name, r in RESIZE_RATIOS:
            ah, aw = O.pyr_init_dim(h, w, 2, float(r))
            if ah[1] >= 1 and aw[1] >= 1:
                out.append((w, h, name, float(r), aw[1], ah[1]))
    return tuple(out)


def test_resize_ledger():
    cases = resize_cases()
    have = {(c[0], c[1], c[2]) for c in cases}
    # every ratio runs on the full shape and on 160x120; an up-sampling ratio on every shape
    for s in (FULL, (160, 120)):
        assert all((s[0], s[1], n) in have for n, _ in RESIZE_RATIOS)
    for s in PREPARE_SHAPES:
        assert (s[0], s[1], "one") in have and (s[0], s[1], "two") in have
    # the cases that are no launch: one-pixel planes shrunk, and 5x3 by a quarter
    empty = {(w, h, n) for (w, h) in PREPARE_SHAPES for n, _ in RESIZE_RATIOS} - have
    assert empty == {(1, 37, n) for n in ("half", "quarter", "157_over_78", "158_over_39")} | \
        {(70, 1, n) for n in ("half", "quarter", "157_over_78", "158_over_39")} | {(5, 3, "quarter")}
    r = dict(RESIZE_RATIOS)
    assert r["157_over_78"] != 0.5 and r["158_over_39"] != 0.5 and abs(float(r["157_over_78"]) - 0.5) < 0.01
    # ratio 2: fx = (x + 1) / 2 - 1 is negative at x = 0 and truncates toward zero
    assert int(np.float32(1) * (np.float32(1) / np.float32(2)) - 1) == 0 and (np.float32(1) * (np.float32(1) / np.float32(2)) - 1) < 0


@functools.lru_cache(None)
def resize_rgba_input(w, h):
    return blur_input("random_rgba", w, h)


@functools.lru_cache(None)
def resize_flow_input(w, h):
    """known vectors with negative components next to unknown ones (1e10)"""
    O = _O()
    rng = np.random.default_rng([w, h, 17])
    f = np.zeros((h, w), O.float2)
    f["x"] = rng.normal(0, 6, (h, w)).astype(np.float32)
    f["y"] = rng.normal(-2, 6, (h, w)).astype(np.float32)
    m = rng.random((h, w))
    f["x"][m < 0.25] = 1e10; f["y"][m < 0.25] = 1e10
    f["x"].flat[0] = 1e10; f["y"].flat[0] = 1e10
    f["x"].flat[-1] = -3.25; f["y"].flat[-1] = -0.5
    return f


def test_resize_flow_input_ledger():
    for (w, h) in PREPARE_SHAPES:
        f = resize_flow_input(w, h)
        unk = f["x"] > 1e9
        assert unk.any() and (~unk).any() and (f["x"][~unk] < 0).any() and (f["y"][~unk] < 0).any()
        if w * h >= 15:                                           # an unknown vector with a known neighbour
            assert (unk[:, 1:] != unk[:, :-1]).any() or (unk[1:] != unk[:-1]).any()


def lum32(r, g, b):
    """.3R + .6G + .1B on unorm floats, left to right, in float32"""
    u = lambda v: (np.asarray(v, np.float32) / np.float32(255)).astype(np.float32)  # noqa: E731
    return ((np.float32(0.3) * u(r) + np.float32(0.6) * u(g)).astype(np.float32) + np.float32(0.1) * u(b)).astype(np.float32)


@functools.lru_cache(None)
def equal_lum_colours():
    """groups of distinct colours whose float32 luminance is the same float: [(lum, [(r, g, b), ...])], the largest groups first"""
    v = np.arange(0, 256, 5)
    r, g, b = [a.ravel() for a in np.meshgrid(v, v, v, indexing="ij")]
    lum = lum32(r, g, b)
    order = np.argsort(lum, kind="stable")
    groups, i = [], 0
    while i < len(order):
        j = i
        while j + 1 < len(order) and lum[order[j + 1]] == lum[order[i]]:
            j += 1
        if j > i:
            groups.append((float(lum[order[i]]), [(int(r[k]), int(g[k]), int(b[k])) for k in order[i:j + 1]]))
        i = j + 1
    groups.sort(key=lambda t: -len(t[1]))
    return groups


@functools.lru_cache(None)
def census_planes(w, h):
    """(img1, img2).  img1: areas of one colour (equal luminance: the strict > gives 0), patches of DISTINCT colours of equal float
    luminance, and extremes either side of the 64-pixel tile border and on the last row and column.  img2: noise quantised to few
    levels (many exact ties) with the same extremes."""
    O = _O()
    rng = np.random.default_rng([w, h, 18])
    xs, ys = grid(w, h)
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[:] = (60, 120, 30)
    groups = equal_lum_colours()
    cols = np.array(groups[0][1][:4] if len(groups[0][1]) >= 3 else groups[0][1] + groups[1][1])
    sel = ((xs // 2 + ys) % len(cols))
    if max(w, h) >= 48:                                          # alternate: constant area / equal-luminance mosaic
        area = ((xs // 12) + (ys // 12)) % 2 == 1
    else:
        area = (xs >= max(1, w // 4)) if w > 1 else (ys >= h // 4)
    rgb[area] = cols[sel[area]]
    noise = rng.integers(0, 4, (h, w, 3)).astype(np.uint8) * 60
    ext = [(x, y) for x in (63, 64, w - 1) for y in (0, h // 2, h - 1) if 0 <= x < w] + [(x, h - 1) for x in (0, w // 2, 62, 65) if 0 <= x < w]
    for k, (x, y) in enumerate(dict.fromkeys(ext)):
        rgb[y, x] = 255 if k % 2 == 0 else 0
        noise[y, x] = 0 if k % 2 == 0 else 255
    a, b = O.rgb2rgba(rgb), O.rgb2rgba(noise)
    a["w"] = rng.integers(0, 256, (h, w))                        # the census ignores alpha
    return a, b


def test_census_ledger():
    O = _O()
    groups = equal_lum_colours()
    assert groups and len(groups[0][1]) >= 2
    lum, cols = groups[0]
    assert len(set(cols)) == len(cols) and len({lum32(*c).tobytes() for c in cols}) == 1
    for (w, h) in PREPARE_SHAPES:
        a, b = census_planes(w, h)
        ca, cb = O.census(a), O.census(b)
        rgb = np.stack([a["x"], a["y"], a["z"]], -1).astype(int)
        L = lum32(a["x"], a["y"], a["z"])
        if w > 1:                                                 # neighbours of distinct colour and equal luminance: bit 16 (right) stays 0
            tie = (L[:, 1:] == L[:, :-1]) & (rgb[:, 1:] != rgb[:, :-1]).any(-1)
            assert tie.any() and not (ca[:, :-1][tie] & 16).any()
        if h > 1:
            tie = (L[1:] == L[:-1]) & (rgb[1:] != rgb[:-1]).any(-1)
            assert tie.any() and not (ca[:-1][tie] & 64).any()
        assert (ca == 0).sum() >= (w * h) // 8                    # large areas of equal luminance
        if w * h > 1:
            assert (ca != 0).any() and (cb != 0).any()
        if w > 64:
            assert ca[:, 62:64].any() and ca[:, 64:66].any()        # an extreme either side of the tile border shows in its neighbours' codes
        if w > 1 and h > 1:
            assert ca[h - 1].any() and ca[:, w - 1].any() or ca[h - 2].any()


# =========================================================================================================================================
# 4. the context's own prepare path
# =========================================================================================================================================
CTX_CASES = ((160, 120, 3), (77, 53, 3), (78, 54, 4), (75, 21, 3))       # (w, h, levels)
G_MAXR = 6


def prepare_branches(w, h, levels):
    """per level >= 1: "fused" (k_gauss_decimate2) or "blur_resize", restating gauss_decimate2_ok (k_prepare.hip) and the step table of a
    context's prepare (ctx_images.cpp) from pyr_init_dim"""
    H, W = _O().pyr_init_dim(h, w, levels)
    ratio = np.float32(0.5)
    n = 1                                                        # (int)(log(0.25) / logf(0.5f)): DESIGN.md 3.3
    out = []
    for i in range(1, levels):
        j = 0 if i <= n else i - n
        sigma = np.float32(1) * (i if i <= n else n)
        r = np.float32(float(ratio) ** i) if i <= n else np.float32(np.float32(np.float32(float(ratio) ** i) * np.float32(W[0])) / np.float32(W[j]))
        radius = int(sigma * 3)
        ok = r == np.float32(0.5) and radius <= G_MAXR and 2 * (W[i] - 1) + 1 <= W[j] - 1 and 2 * (H[i] - 1) + 1 <= H[j] - 1
        out.append("fused" if ok else "blur_resize")
    return out, H, W


def test_context_branch_ledger():
    want = {(160, 120, 3): ["fused", "fused"], (77, 53, 3): ["fused", "blur_resize"], (78, 54, 4): ["fused", "fused", "blur_resize"],
            (75, 21, 3): ["fused", "blur_resize"]}
    for case in CTX_CASES:
        got, H, W = prepare_branches(*case)
        assert got == want[case], (case, got)
    _, H, W = prepare_branches(77, 53, 3)
    assert W[0] % 2 == 1 and W[1] == 38                          # level 1 fused from an odd-width source
    _, H, W = prepare_branches(78, 54, 4)
    assert W[1] == 39 and W[2] == 19                             # level 2 fused from the 39-wide level
    assert {b for c in CTX_CASES for b in prepare_branches(*c)[0]} == {"fused", "blur_resize"}


@functools.lru_cache(None)
def ctx_image(w, h, k):
    """image k of a size: a smooth colour field with texture and hard edges, (h, w, 3) uint8"""
    rng = np.random.default_rng([w, h, 19, k])
    xs, ys = grid(w, h)
    base = np.stack([128 + 100 * np.sin((xs + 3 * k) / 9.0 + ys / 17.0), 128 + 100 * np.cos(xs / 13.0 - (ys + 2 * k) / 7.0),
                     (xs * 5 + ys * 3 + 40 * k) % 256], -1)
    img = np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
    img[h // 3:h // 3 + 2, :] = 255 if k % 2 else 0
    img[:, w - 1] = rng.integers(0, 256, (h, 3))
    return img


@functools.lru_cache(None)
def ctx_raw(w, h, k, alpha):
    """the raw RGBA plane of image k: rgb2rgba (alpha 0), or with a varying non-zero alpha for the device entry points"""
    raw = _O().rgb2rgba(ctx_image(w, h, k))
    if alpha:
        raw["w"] = np.random.default_rng([w, h, 20, k]).integers(1, 256, (h, w))
    return raw


@functools.lru_cache(None)
def ctx_oracle(w, h, levels, k, alpha=False):
    """(imgs, census) of image k at every level under the oracle"""
    return _O().prepare(ctx_raw(w, h, k, alpha), levels)


def test_context_inputs_ledger():
    for (w, h, levels) in CTX_CASES:
        imgs, cens = ctx_oracle(w, h, levels, 0, True)
        assert all((im["w"] > 0).any() for im in imgs)            # the alpha byte travels through every level
        assert all(c.any() for c in cens)
        assert any(not np.array_equal(ctx_oracle(w, h, levels, 0)[0][l], ctx_oracle(w, h, levels, 1)[0][l]) for l in range(levels))
