"""Plain numpy restatements of the accumulator kernels (csrc/rt_accum_kernels.h), written from the text of
include/rtr_hip.h and of the kernel header's comments, and the synthetic tile state the tests feed them and the device
with (tests/test_accum_planes_cpu.py holds each restatement to a scalar loop; tests/test_accum_planes.py holds the
device to the restatements, bit for bit).

Layout, as the accumulator keeps it: per owned tile (order of rtr_accum_tiles: ascending tile id of the reference's
dispatch numbering, renderer.h:61-62) sum[3][256] and q[256]; lane = 16 * row + column of the tile, row 0 its LOWEST
pixel row; tile t of a tiles_x * tiles_y grid sits at column t % tiles_x and at row (tiles_y - 1) - t // tiles_x from the
bottom.  Every function here takes the arrays of all the tiles it is given; `select` cuts a case down to a shard."""
import numpy as np

BLOCK = 256
INT_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")

# the geometry of every case: 5 x 4 tiles; the left tile column keeps one active column (i = 15), the right one two, the
# top tile row one active row (j = 48), the bottom one rows 3..15, six interior tiles all 256 lanes
W, H, REGION = 80, 64, (15, 3, 66, 49)
SHARDS = ((0, 1), (1, 3))  # (tile_first, tile_stride): every tile, and tiles 1, 4, 7, ...


# ---- tiles, lanes, pixels ------------------------------------------------------------------------------------------


def owned_tiles(w, h, region, first=0, stride=1):
    """the tiles that touch the region, every stride-th from `first`, ascending"""
    tx, ty = (w + 15) // 16, (h + 15) // 16
    x0, y0, x1, y1 = region
    out = []
    for t in range(first, tx * ty, max(stride, 1)):
        xs, ys = (t % tx) * 16, ((ty - 1) - t // tx) * 16
        if xs + 16 <= x0 or xs >= x1 or ys + 16 <= y0 or ys >= y1:
            continue
        out.append(t)
    return out


def tile_origin(w, h, t):
    tx, ty = (w + 15) // 16, (h + 15) // 16
    return (t % tx) * 16, ((ty - 1) - t // tx) * 16


def lane_pixels(w, h, ids):
    """(i, j) of every lane: two (n, 256) int arrays"""
    lane = np.arange(BLOCK)
    org = np.array([tile_origin(w, h, t) for t in ids], dtype=np.int64).reshape(len(ids), 2)
    return org[:, 0:1] + (lane & 15)[None, :], org[:, 1:2] + (lane >> 4)[None, :]


def tile_boxes(w, h, region, ids):
    """per tile (row0, row1, col0, col1): the rows and columns of the TILE (0..16) that lie inside the region"""
    x0, y0, x1, y1 = region
    out = np.zeros((len(ids), 4), dtype=np.int64)
    for k, t in enumerate(ids):
        xs, ys = tile_origin(w, h, t)
        out[k] = (max(ys, y0) - ys, min(ys + 16, y1) - ys, max(xs, x0) - xs, min(xs + 16, x1) - xs)
    return out


def box_mask(boxes):
    """(n, 256) bool: the lanes inside the boxes"""
    lane = np.arange(BLOCK)
    row, col = (lane >> 4)[None, :], (lane & 15)[None, :]
    b = np.asarray(boxes).reshape(-1, 4)
    return (row >= b[:, 0:1]) & (row < b[:, 1:2]) & (col >= b[:, 2:3]) & (col < b[:, 3:4])


def tiles_to_region(w, h, region, ids, counts, tiles, out, flip=False):
    """what the host scatter loops and k_accum_resolve_scatter do: the lanes inside the region of every tile that holds
    samples (counts None: of every tile) from `tiles` (n, 256) or (n, 256, C) into out[j - y0, i - x0] -- or with `flip`
    into out[y1 - 1 - j, i - x0], the top row first; the other pixels of `out` stay.  Returns out."""
    x0, y0, x1, y1 = region
    ii, jj = lane_pixels(w, h, ids)
    inside = box_mask(tile_boxes(w, h, region, ids))
    for k in range(len(ids)):
        if counts is not None and counts[k] == 0:
            continue
        m = inside[k]
        rows = (y1 - 1 - jj[k][m]) if flip else (jj[k][m] - y0)
        out[rows, ii[k][m] - x0] = tiles[k][m]
    return out


def owner_image(w, h, region, ids):
    """(y1 - y0, x1 - x0) ints: the slot of the tile that owns each pixel of the region, -1 where none of `ids` does"""
    slots = np.repeat(np.arange(len(ids))[:, None], BLOCK, axis=1)
    return tiles_to_region(w, h, region, ids, None, slots, np.full((region[3] - region[1], region[2] - region[0]), -1))


def select(case, ids):
    """the tiles `ids` of a case generated for every tile: its per-tile arrays cut down, in the order of ids"""
    slot = {int(t): k for k, t in enumerate(case["ids"])}
    pick = np.array([slot[int(t)] for t in ids], dtype=np.int64)
    out = dict(case)
    for name, v in case.items():
        if isinstance(v, np.ndarray) and v.shape[:1] == (len(case["ids"]),):
            out[name] = np.ascontiguousarray(v[pick])
    out["ids"] = np.array(ids, dtype=np.int64)
    return out


# ---- the restatements ----------------------------------------------------------------------------------------------


def lum(m0, m1, m2):
    return 0.2126 * m0 + 0.7152 * m1 + 0.0722 * m2


def errors(sum, q, count, boxes):
    """rtr_accum_errors: per tile the largest pixel error inside the box, +inf below 2 samples.  max(a, b) of the header
    is a > b ? a : b: a NaN d gives var 0, a NaN y_m the floor 1e-4; a pixel's error is then never NaN."""
    inside = box_mask(boxes)
    out = np.empty(len(count))
    with np.errstate(all="ignore"):
        for k, n in enumerate(count):
            if n < 2:
                out[k] = np.inf
                continue
            scale = 1.0 / float(n)
            ym = lum(scale * sum[k, 0], scale * sum[k, 1], scale * sum[k, 2])
            d = scale * q[k] - ym * ym
            var = np.where(d > 0.0, d, 0.0) / float(int(n) - 1)
            e = np.sqrt(var) / (2.0 * np.sqrt(np.where(ym > 1e-4, ym, 1e-4)))
            e = np.where(inside[k], e, 0.0)
            assert not np.isnan(e).any()
            out[k] = np.max(e)
    return out


def plan(count, err, tile_s1, mode, spp=0, spp_min=1, spp_max=1, threshold=1.0):
    """k_accum_plan: (targets (n,) int32, the set of active slots).  Mode 2 is the rule of rtr_accum_refine, min(spp_max,
    2 * n) taken in exact integers; `e > threshold` is false for a NaN e, so such a tile stops once it holds spp_min."""
    c = np.asarray(count).astype(np.int64)
    if mode == 0:
        target = np.asarray(tile_s1).astype(np.int64)
    elif mode == 1:
        target = np.maximum(c, int(spp))
    else:
        with np.errstate(invalid="ignore"):
            above = np.asarray(err, dtype=np.float64) > threshold
        target = np.where(c < spp_min, spp_min, np.where(above & (c < spp_max), np.minimum(spp_max, 2 * c), c))
    return target.astype(np.int32), set(np.flatnonzero(target > c).tolist())


def buckets(target, count):
    """floor(log2(target - count)) per slot, -1 where nothing is pending"""
    pend = np.asarray(target).astype(np.int64) - np.asarray(count).astype(np.int64)
    return np.array([int(p).bit_length() - 1 if p > 0 else -1 for p in pend], dtype=np.int64)


def commit(active, n_active, done, tile_s1, partial, q_part, sum, q, count):
    """k_accum_commit: the slots active[:n_active] whose pass ran to the end take its sums, moments and target"""
    sum, count = sum.copy(), count.copy()
    q = None if q is None else q.copy()
    for b in range(int(n_active)):
        s = int(active[b])
        if not done[s]:
            continue
        sum[s] = partial[s]
        if q is not None:
            q[s] = q_part[s]
        count[s] = tile_s1[s]
    return sum, q, count


def resolve_linear(sum, count):
    """(1.0 / count) * sum, (n, 3, 256); tiles with count 0 are not resolved (zeros here)"""
    out = np.zeros_like(sum)
    with np.errstate(all="ignore"):
        for k, n in enumerate(count):
            if n > 0:
                out[k] = (1.0 / float(n)) * sum[k]
    return out


def resolve_rgb8(mean):
    """the 8-bit store: uchar(clamp(sqrt(m), 0, 1) * 255), truncated.  Returns (bytes, defined): the byte of a mean with
    !(m >= 0) -- NaN or negative, whose sqrt is NaN -- is not defined by the reference's C++ and reads 0 here."""
    with np.errstate(all="ignore"):
        defined = mean >= 0.0
        g = np.sqrt(np.where(defined, mean, 0.0))
        g = np.where(g < 0.0, 0.0, np.where(g > 1.0, 1.0, g))
        return (g * 255).astype(np.uint8), defined


# ---- case: errors --------------------------------------------------------------------------------------------------

ERR_COUNTS = (0, 1, 2, 3, 7, 1000, INT_MAX)  # of tile t: ERR_COUNTS[t % 7]
WIN_LANES = (0, 63, 64, 127, 128, 191, 192, 255)  # first and last lane of each of the four waves
ZERO_TILE = 16  # only zero-error active pixels, three poisoned rows
VALUE_CLASSES = ("d_pos", "d_le", "d_neg", "ym_above", "ym_below", "ym_zero", "ym_neg", "sum_nan", "sum_inf", "sum_ninf",
                 "q_nan", "q_neg", "subnormal")
ZERO_CLASSES = ("d_le", "d_neg", "zero", "sum_nan", "sum_inf", "sum_ninf", "q_nan", "q_neg")
POISONS = ("huge", "q_inf", "nan", "negative")


def _ym(s3, n):
    scale = 1.0 / float(n)
    return lum(scale * s3[0], scale * s3[1], scale * s3[2])


def _d(s3, q, n):
    ym = _ym(s3, n)
    return (1.0 / float(n)) * q - ym * ym


def _up(x):
    return float(np.nextafter(x, INF))


def _down(x):
    return float(np.nextafter(x, -INF))


def _q_around_zero_d(s3, n):
    """(the smallest q with d > 0, the q below it: d <= 0, the largest q with d < 0)"""
    ym = _ym(s3, n)
    q = ym * ym * float(n)
    for _ in range(64):
        if _d(s3, q, n) > 0.0:
            break
        q = _up(q)
    for _ in range(64):
        if not _d(s3, _down(q), n) > 0.0:
            break
        q = _down(q)
    assert _d(s3, q, n) > 0.0 and not _d(s3, _down(q), n) > 0.0
    le = neg = _down(q)
    for _ in range(64):
        if _d(s3, neg, n) < 0.0:
            break
        neg = _down(neg)
    assert _d(s3, neg, n) < 0.0
    return q, le, neg


def _sum_around_1e4(n):
    """(sums with y_m just above 1e-4, sums with y_m at or just below it): a nextafter walk on the green sum"""
    s = [1e-4 * float(n)] * 3
    for _ in range(4096):
        if not _ym(s, n) > 1e-4:
            break
        s[1] = _down(s[1])
    for _ in range(4096):
        if _ym(s, n) > 1e-4:
            break
        s[1] = _up(s[1])
    below = [s[0], _down(s[1]), s[2]]
    assert _ym(s, n) > 1e-4 and not _ym(below, n) > 1e-4
    return s, below


def _lane_value(cls, n, salt):
    """(three sums, q) of a pixel of class `cls` in a tile holding n samples; every class stays below an error of 0.01"""
    fn = float(n)
    y = 0.25 + 0.5 * ((salt * 37) % 64) / 64.0
    tame = [y * fn, 0.5 * y * fn, 1.5 * y * fn]
    if cls in ("d_pos", "d_le", "d_neg"):
        qs = _q_around_zero_d(tame, n)
        return tame, qs[("d_pos", "d_le", "d_neg").index(cls)]
    if cls in ("ym_above", "ym_below"):
        above, below = _sum_around_1e4(n)
        return (above if cls == "ym_above" else below), 2e-8 * fn
    if cls == "ym_zero":
        return [0.0, 0.0, 0.0], 1e-8 * fn * (fn - 1.0)
    if cls == "zero":
        return [0.0, 0.0, 0.0], 0.0
    if cls == "ym_neg":
        return [-0.3 * fn] * 3, fn * (0.09 + 1e-8 * (fn - 1.0))
    if cls == "sum_nan":
        return [NAN, tame[1], tame[2]], 1e6 * fn
    if cls == "sum_inf":
        return [tame[0], INF, tame[2]], 1.0
    if cls == "sum_ninf":
        return [-INF, tame[1], tame[2]], 1e6 * fn
    if cls == "q_nan":
        return tame, NAN
    if cls == "q_neg":
        return tame, -1e6 * fn
    if cls == "subnormal":
        return [3 * 5e-324, 5e-324, 7 * 5e-324], 5e-324 * (salt % 5 + 1)
    if cls == "w_fin":  # the winner: an error near 0.5, another one in every tile
        return [0.5 * fn] * 3, fn * (0.25 + (fn - 1.0) * 0.5 * (1.0 + (salt % 64) / 64.0))
    if cls == "w_inf":  # ... or +inf
        return tame, INF
    raise KeyError(cls)


def _poison(kind, n):
    """a lane outside the region; read as a pixel, "huge", "q_inf" and "negative" give an error above every winner's (a NaN
    lane gives 0 by the formula and shows where lanes are masked by arithmetic instead of a test)"""
    fn = float(n)
    if kind == "huge":
        return [1e150] * 3, 1e308
    if kind == "q_inf":
        return [0.5 * fn] * 3, INF
    if kind == "nan":
        return [NAN] * 3, NAN
    return [-1e6 * fn] * 3, 1e300


def _nearest_in_box(lane, box):
    r0, r1, c0, c1 = (int(v) for v in box)
    row, col = lane >> 4, lane & 15
    if r0 <= row < r1 and c0 <= col < c1:
        return lane
    r = r0 if abs(row - r0) <= abs(row - (r1 - 1)) else r1 - 1
    c = c0 if abs(col - c0) <= abs(col - (c1 - 1)) else c1 - 1
    return 16 * r + c


def errors_case():
    """sums, moments and counts of all 20 tiles for rtr_accum_errors, with per lane the class it was made as
    (cls: (n, 256) strings; winner: the winner's lane per tile, -1 without one)"""
    ids = owned_tiles(W, H, REGION)
    boxes = tile_boxes(W, H, REGION, ids)
    inside = box_mask(boxes)
    n = len(ids)
    s, q = np.zeros((n, 3, BLOCK)), np.zeros((n, BLOCK))
    count = np.array([ERR_COUNTS[t % 7] for t in ids], dtype=np.int32)
    cls = np.empty((n, BLOCK), dtype=object)
    winner = np.full(n, -1, dtype=np.int64)
    k = 0  # tiles with a winner so far
    for slot, t in enumerate(ids):
        m = max(int(count[slot]), 2)  # the tiles below 2 samples hold the values of a 2-sample tile
        if count[slot] >= 2 and t != ZERO_TILE:
            k += 1  # (from lane 63 on: then each of the eight lanes lies inside the box of some tile that asks for it)
            winner[slot] = _nearest_in_box(WIN_LANES[k % 8], boxes[slot])
        classes = ZERO_CLASSES if t == ZERO_TILE else VALUE_CLASSES
        idx = t  # every tile starts the cycle elsewhere
        for lane in range(BLOCK):
            if not inside[slot, lane]:
                cls[slot, lane] = "poison_" + POISONS[(lane + t) % 4]
                s3, qq = _poison(POISONS[(lane + t) % 4], m)
            elif lane == winner[slot]:
                cls[slot, lane] = "w_inf" if k % 4 == 0 else "w_fin"
                s3, qq = _lane_value(cls[slot, lane], m, t)
            else:
                cls[slot, lane] = classes[idx % len(classes)]
                s3, qq = _lane_value(cls[slot, lane], m, lane + t)
                idx += 1
            s[slot, :, lane], q[slot, lane] = s3, qq
    return dict(ids=np.array(ids, dtype=np.int64), boxes=boxes, sum=s, q=q, count=count, cls=cls, winner=winner)


# ---- case: resolve -------------------------------------------------------------------------------------------------

RESOLVE_EMPTY = (0, 7)  # tiles with count 0: a corner and an interior one
RESOLVE_ODD_TILE = 13   # the one tile with NaN and negative means (count 3)
RESOLVE_COUNT1 = (2, 4, 10, 12, 14, 17, 19)  # the other tiles hold 3 samples
RESOLVE_ODD_PIXELS = 8


def byte_step_means():
    """for every byte step b the double (b / 255)^2 and its two neighbours; then the special means"""
    out = []
    for b in range(1, 256):
        v = (b / 255.0) * (b / 255.0)
        out += [_down(v), v, _up(v)]
    return out + [0.0, -0.0, 5e-324, 1.0, _down(1.0), _up(1.0), 4.0, INF]


def resolve_case():
    """sums and counts whose means, with count 1 and with count 3, walk byte_step_means(): with count 1 the sum is the
    mean; with count 3 the sums are 3 * v and its two neighbours on either side, the closest means (1.0 / 3) * sum reaches.
    Lanes outside the region hold junk that must never show."""
    ids = owned_tiles(W, H, REGION)
    inside = box_mask(tile_boxes(W, H, REGION, ids))
    n = len(ids)
    s = np.zeros((n, 3, BLOCK))
    count = np.array([0 if t in RESOLVE_EMPTY else (1 if t in RESOLVE_COUNT1 else 3) for t in ids], dtype=np.int32)
    v1 = byte_step_means()
    v3 = []
    for v in v1:
        lo, hi = _down(3.0 * v), _up(3.0 * v)
        # (around 0 the walk would reach a negative mean: those belong to the odd tile alone, -0.0 stands in)
        v3 += [x if (1.0 / 3.0) * x >= 0.0 else -0.0 for x in (_down(lo), lo, 3.0 * v, hi, _up(hi))]
    pos = {1: 0, 3: 0, 0: 0}
    stream = {1: v1, 3: v3, 0: v1}
    junk = (NAN, 1e300, -1.0, INF)
    odd = [(NAN, 1.5, 1.5), (1.5, NAN, 1.5), (1.5, 1.5, NAN), (NAN, NAN, NAN), (-3.0, 1.5, 1.5), (1.5, -INF, 1.5),
           (1.5, 1.5, -1.5e-323), (-3e-300, -3.0, NAN)]
    assert len(odd) == RESOLVE_ODD_PIXELS
    for slot, t in enumerate(ids):
        c = int(count[slot])
        n_odd = 0
        for lane in range(BLOCK):
            if not inside[slot, lane]:
                s[slot, :, lane] = junk[(lane + t) % 4]
            elif t == RESOLVE_ODD_TILE and n_odd < len(odd):
                s[slot, :, lane] = odd[n_odd]
                n_odd += 1
            else:
                for ch in range(3):
                    s[slot, ch, lane] = stream[c][pos[c] % len(stream[c])]
                    pos[c] += 1
    return dict(ids=np.array(ids, dtype=np.int64), sum=s, count=count, slots_used=dict(pos))


# ---- case: refine through the product ----------------------------------------------------------------------------------

REFINE_COUNTS = (1, 2, 3, 4, 8, 16)
REFINE_MIN, REFINE_MAX = 2, 16
REFINE_TILE = 10  # the tile whose error is the threshold: count 4, in both shards


def refine_case():
    """tame state with moments for rtr_accum_refine: counts from REFINE_COUNTS, every tile's error set by one pixel of its
    box -- 0 in a third of the tiles, near 7e-4 in another, from 0.07 up and growing with the tile id in the last"""
    ids = owned_tiles(W, H, REGION)
    boxes = tile_boxes(W, H, REGION, ids)
    n = len(ids)
    count = np.array([REFINE_COUNTS[(t + t // 3) % 6] for t in ids], dtype=np.int32)
    s, q = np.zeros((n, 3, BLOCK)), np.zeros((n, BLOCK))
    for slot, t in enumerate(ids):
        fn = float(count[slot])
        s[slot] = 0.5 * fn
        q[slot] = 0.2 * fn  # below n * y_m^2: d < 0, error 0
        level = (0.0, 1e-3, 0.1)[(t // 2) % 3] * (1.0 + t / 40.0)
        lane = _nearest_in_box(WIN_LANES[t % 8], boxes[slot])
        if level > 0.0 and count[slot] >= 2:
            q[slot, lane] = fn * (0.25 + (fn - 1.0) * level * level)
    return dict(ids=np.array(ids, dtype=np.int64), boxes=boxes, sum=s, q=q, count=count)


def refine_outcomes(count, err, target, spp_min, spp_max, threshold):
    """the rule's outcome per tile, by name"""
    out = []
    for c, e, t in zip(count, err, target):
        if c < spp_min:
            out.append("below_min")
        elif c >= spp_max:
            out.append("at_max")
        elif not e > threshold:
            out.append("stopped")
        elif e == INF and c == 1:
            out.append("inf_at_one")
        elif t == spp_max:
            out.append("capped")
        else:
            out.append("doubling")
    return out


# ---- cases: the plan kernel alone ------------------------------------------------------------------------------------

PLAN_SIZES = (1, 31, 1023, 1024, 1025, 5000)
PLAN_THRESHOLD = 0.01
PLAN_MODE2 = {  # name -> (spp_min, spp_max, threshold, counts)
    "classes": (2, 16, PLAN_THRESHOLD, (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 1000, INT_MAX)),
    "overflow": (1, INT_MAX, PLAN_THRESHOLD, (0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, INT_MAX - 1, INT_MAX)),
    "inf_threshold": (4, 100, INF, (0, 3, 4, 50, 100, 101)),
}


def _shuffled(n, seed):
    return np.random.default_rng(seed).permutation(n)


def plan_case_mode0(n, variant):
    """targets as given: pendings 2^b and 2^(b+1) - 1 for every b in 0..30 and idle slots, in shuffled order.  variant
    "mixed", "idle" (target == count everywhere) or "all" (no idle slot)"""
    rng = np.random.default_rng(1000 + n)
    kinds = _shuffled(n, n) % (62 if variant == "all" else 63)
    pend = np.array([0 if k == 62 else ((1 << (k // 2)) if k % 2 == 0 else (1 << (k // 2 + 1)) - 1) for k in kinds],
                    dtype=np.int64)
    if variant == "idle":
        pend[:] = 0
    count = (rng.random(n) * (INT_MAX - pend + 1)).astype(np.int64)
    count = np.minimum(count, INT_MAX - pend)
    return dict(count=count.astype(np.int32), err=np.zeros(n), tile_s1=(count + pend).astype(np.int32), mode=0)


def plan_case_mode1(n):
    order = _shuffled(n, 7 * n)
    count = np.array([(0, 37, 99, 100, 101, 5000, INT_MAX)[k % 7] for k in order], dtype=np.int32)
    return dict(count=count, err=np.zeros(n), tile_s1=np.full(n, -5, dtype=np.int32), mode=1, spp=100)


def plan_case_mode2(n, name):
    spp_min, spp_max, thr, counts = PLAN_MODE2[name]
    errs = (-0.0, 0.0, thr, _up(thr) if thr < INF else 1e308, _down(thr) if thr < INF else 1e300, INF, NAN, 1e300)
    order = _shuffled(n, 13 * n + len(name))
    count = np.array([counts[k % len(counts)] for k in order], dtype=np.int32)
    err = np.array([errs[(k // len(counts)) % len(errs)] for k in order])
    return dict(count=count, err=err, tile_s1=np.full(n, -5, dtype=np.int32), mode=2, spp_min=spp_min, spp_max=spp_max,
                threshold=thr)


def plan_cases(n):
    """name -> the keyword arguments of `plan` (and of Context.accum_plan)"""
    out = {"mode0-" + v: plan_case_mode0(n, v) for v in ("mixed", "idle", "all")}
    out["mode1"] = plan_case_mode1(n)
    out.update({"mode2-" + name: plan_case_mode2(n, name) for name in PLAN_MODE2})
    return out


# ---- cases: the commit kernel alone ----------------------------------------------------------------------------------

COMMIT_SIZES = (1, 7, 300)
COMMIT_LISTS = ("none", "all", "half")


def _random_bits(rng, shape):
    a = rng.integers(0, 2 ** 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    flat[:2] = (0x7FF8000000000123, 0xFFF0000000000001)  # a quiet and a signalling NaN with payloads
    return a.view(np.float64)


def commit_case(n, with_q, lists):
    """random bit patterns (NaN payloads among them) as pass results and as the state they may replace"""
    rng = np.random.default_rng(50 * n + 2 * COMMIT_LISTS.index(lists) + int(with_q))
    active = rng.permutation(n).astype(np.int32)
    n_active = {"none": 0, "all": n, "half": (n + 1) // 2}[lists]
    done = rng.integers(0, 2, n).astype(np.int32)
    if n == 1:
        done[0] = 1 if with_q else 0
    else:
        listed = active[:max(n_active, 2)]
        done[listed[0]], done[listed[1]] = 1, 0  # both values, among the listed slots where there are two
    if lists == "half":
        done[active[n_active:]] = 1  # finished, but not on the list: must not commit
    return dict(active=active, n_active=n_active, done=done, tile_s1=rng.integers(0, INT_MAX, n).astype(np.int32),
                partial=_random_bits(rng, (n, 3, BLOCK)), q_part=_random_bits(rng, (n, BLOCK)) if with_q else None,
                sum=_random_bits(rng, (n, 3, BLOCK)), q=_random_bits(rng, (n, BLOCK)) if with_q else None,
                count=rng.integers(0, INT_MAX, n).astype(np.int32))
