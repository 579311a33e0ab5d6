"""CPU-only: the numpy restatements of tests/_accum_ref.py against scalar Python loops written from the header text
(include/rtr_hip.h: the error formula, the refinement rule, the 8-bit store; csrc/rt_accum_kernels.h: the plan and the
commit), on the very inputs tests/test_accum_planes.py feeds the device; and the generators of those inputs reach what
they claim -- every class is counted.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _accum_ref as R
import _golden as G

rtr = G.rtr
ROOT = G.ROOT

X0, Y0, X1, Y1 = R.REGION


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _b(v):
    return int(np.float64(v).view(np.uint64))


def _pixel(t, lane):
    """tile t, lane -> (i, j, inside the region): renderer.h:61-62 for the 5 x 4 tiles of the 80 x 64 image"""
    i, j = (t % 5) * 16 + lane % 16, (3 - t // 5) * 16 + lane // 16
    return i, j, X0 <= i < X1 and Y0 <= j < Y1


def _pixel_error(s3, q, n):
    """include/rtr_hip.h, per pixel, in Python floats: (err, d, y_m)"""
    scale = 1.0 / n
    m = [scale * float(x) for x in s3]
    ym = 0.2126 * m[0] + 0.7152 * m[1] + 0.0722 * m[2]
    d = scale * float(q) - ym * ym
    var = (d if d > 0.0 else 0.0) / (n - 1)
    return math.sqrt(var) / (2.0 * math.sqrt(ym if ym > 1e-4 else 1e-4)), d, ym


@pytest.fixture(scope="module")
def ecase():
    return R.errors_case()


@pytest.fixture(scope="module")
def rcase():
    return R.resolve_case()


def test_geometry_is_the_one_the_cases_are_written_for():
    ids = R.owned_tiles(R.W, R.H, R.REGION)
    assert ids == list(range(20))
    assert R.owned_tiles(R.W, R.H, R.REGION, 1, 3) == [1, 4, 7, 10, 13, 16, 19]
    inside = R.box_mask(R.tile_boxes(R.W, R.H, R.REGION, ids))
    ii, jj = R.lane_pixels(R.W, R.H, ids)
    for t in ids:
        for lane in range(R.BLOCK):
            assert (int(ii[t, lane]), int(jj[t, lane]), bool(inside[t, lane])) == _pixel(t, lane)
    n_in = inside.sum(axis=1)
    assert sorted(np.flatnonzero(n_in == 256).tolist()) == [6, 7, 8, 11, 12, 13]  # six interior tiles
    assert n_in[5] == n_in[10] == 16 and n_in[9] == n_in[14] == 32       # one active column left, two right
    assert n_in[1] == n_in[2] == n_in[3] == 16 and n_in[0] == 1 and n_in[4] == 2  # one active row on top
    assert n_in[16] == n_in[17] == n_in[18] == 13 * 16 and n_in[15] == 13 and n_in[19] == 26  # rows 3..15 at the bottom
    assert int(n_in.sum()) == (X1 - X0) * (Y1 - Y0)
    # the scatter of the restatement puts lane (i, j) at out[j - y0, i - x0], or top row first
    img = R.tiles_to_region(R.W, R.H, R.REGION, ids, None, ii * 1000 + jj, np.full((Y1 - Y0, X1 - X0), -1))
    top = R.tiles_to_region(R.W, R.H, R.REGION, ids, None, ii * 1000 + jj, np.full((Y1 - Y0, X1 - X0), -1), flip=True)
    want = (np.arange(X0, X1) * 1000)[None, :] + np.arange(Y0, Y1)[:, None]
    assert np.array_equal(img, want) and np.array_equal(top, want[::-1])


def test_errors_restatement_is_the_scalar_formula_and_the_case_reaches_its_classes(ecase):
    c = ecase
    got = R.errors(c["sum"], c["q"], c["count"], c["boxes"])
    seen = {"d>0": 0, "d==0": 0, "d<0": 0, "ym>1e-4": 0, "ym<=1e-4 near": 0, "winners": set(), "poison wins": 0,
            "poison nan": 0, "zero tile": 0, "below 2": 0}
    classes = set()
    for slot, t in enumerate(c["ids"]):
        n = int(c["count"][slot])
        if n < 2:
            assert got[slot] == math.inf
            seen["below 2"] += 1
            continue
        best, where = 0.0, -1
        poison = []
        for lane in range(R.BLOCK):
            e, d, ym = _pixel_error(c["sum"][slot, :, lane], c["q"][slot, lane], n)
            cls = c["cls"][slot, lane]
            if not _pixel(int(t), lane)[2]:
                assert cls.startswith("poison_")
                poison.append((cls, e))
                continue
            assert not math.isnan(e) and not cls.startswith("poison_")
            classes.add(cls)
            if cls in ("d_pos", "d_le", "d_neg"):
                seen["d>0" if d > 0.0 else ("d==0" if d == 0.0 else "d<0")] += 1
                assert (cls == "d_pos") == (d > 0.0) and (cls != "d_neg" or d < 0.0)
            if cls == "ym_above":
                assert ym > 1e-4 and ym <= float(np.nextafter(1e-4, 1.0)) * (1 + 1e-12)
                seen["ym>1e-4"] += 1
            if cls == "ym_below":
                assert ym <= 1e-4 and ym >= 1e-4 * (1 - 1e-12)
                seen["ym<=1e-4 near"] += 1
            if cls == "ym_neg":
                assert ym < 0.0 and e > 0.0
            if e > best:
                best, where = e, lane
        assert _b(got[slot]) == _b(best), (t, got[slot], best)
        if t == R.ZERO_TILE:
            assert where == -1 and _b(got[slot]) == _b(0.0) and poison
            seen["zero tile"] += 1
        else:  # the winner is where it was placed, and alone up there
            assert where == c["winner"][slot] and c["cls"][slot, where] in ("w_fin", "w_inf")
            seen["winners"].add(where)
            assert all(_pixel_error(c["sum"][slot, :, lane], c["q"][slot, lane], n)[0] < 0.01 for lane in range(R.BLOCK)
                       if _pixel(int(t), lane)[2] and lane != where)
        for cls, e in poison:  # read as a pixel, a poisoned lane would beat the tile's error (a NaN lane: by arithmetic only)
            if cls == "poison_nan":
                seen["poison nan"] += 1
            elif c["cls"][slot, max(where, 0)] != "w_inf":
                assert e > best and e > 1.0, (t, cls, e, best)
                seen["poison wins"] += 1
    assert seen["winners"] >= set(R.WIN_LANES), seen["winners"]
    assert classes >= set(R.VALUE_CLASSES) | set(R.ZERO_CLASSES) | {"w_fin", "w_inf"}
    assert all(v >= 1 for k, v in seen.items() if k != "winners"), seen
    assert set(c["count"].tolist()) == set(R.ERR_COUNTS)
    # ... in the shard as well: every count, a winner, the zero tile, tiles below 2 samples
    shard = R.select(c, R.owned_tiles(R.W, R.H, R.REGION, 1, 3))
    assert set(shard["count"].tolist()) == set(R.ERR_COUNTS) and R.ZERO_TILE in shard["ids"] and (shard["winner"] >= 0).sum() >= 3
    assert np.array_equal(_bits(R.errors(shard["sum"], shard["q"], shard["count"], shard["boxes"])),
                          _bits(got[shard["ids"]]))


def test_byte_store_restatement_is_the_scalar_store_and_the_case_walks_every_byte_step(rcase):
    c = rcase
    mean = R.resolve_linear(c["sum"], c["count"])
    byte, defined = R.resolve_rgb8(mean)
    inside = R.box_mask(R.tile_boxes(R.W, R.H, R.REGION, c["ids"]))
    steps = R.byte_step_means()
    assert len(steps) == 3 * 255 + 8 and c["slots_used"][1] >= len(steps) and c["slots_used"][3] >= 5 * len(steps)
    produced = {1: set(), 3: set()}
    means = {1: set(), 3: set()}
    undefined_pixels = 0
    for slot, t in enumerate(c["ids"]):
        n = int(c["count"][slot])
        if n == 0:
            assert t in R.RESOLVE_EMPTY
            continue
        for lane in range(R.BLOCK):
            px_defined = True
            for ch in range(3):
                v = (1.0 / n) * float(c["sum"][slot, ch, lane])
                assert _b(v) == _b(mean[slot, ch, lane])
                if not v >= 0.0:
                    assert not defined[slot, ch, lane]
                    px_defined = False
                    continue
                g = math.sqrt(v)
                g = 0.0 if g < 0.0 else (1.0 if g > 1.0 else g)
                assert defined[slot, ch, lane] and int(g * 255) == byte[slot, ch, lane], (t, lane, ch, v)
                if inside[slot, lane]:
                    produced[n].add(int(g * 255))
                    means[n].add(_b(v))
            if inside[slot, lane] and not px_defined:
                assert t == R.RESOLVE_ODD_TILE
                undefined_pixels += 1
    assert produced[1] == set(range(256)) and produced[3] == set(range(256))
    assert means[1] >= {_b(v) for v in steps}  # -0.0 and 0.0 apart
    assert 1 <= undefined_pixels == R.RESOLVE_ODD_PIXELS <= 16  # the one exclusion of the byte comparison
    # with 3 samples a mean is (1.0 / 3) * sum, which does not reach every double: each step value or a neighbour of it
    for v in steps:
        near = {_b(v)} if v in (0.0, math.inf) else {_b(np.nextafter(v, -np.inf)), _b(v), _b(np.nextafter(v, np.inf))}
        assert near & means[3], v
    shard = R.select(c, R.owned_tiles(R.W, R.H, R.REGION, 1, 3))
    assert set(shard["count"].tolist()) == {0, 1, 3} and R.RESOLVE_ODD_TILE in shard["ids"]


def _plan_scalar(count, err, tile_s1, mode, spp=0, spp_min=1, spp_max=1, threshold=1.0):
    """csrc/rt_accum_kernels.h / rtr_accum_refine, tile by tile, in Python integers"""
    target = []
    for c, e, s1 in zip(count.tolist(), err.tolist(), tile_s1.tolist()):
        if mode == 0:
            target.append(s1)
        elif mode == 1:
            target.append(max(c, spp))
        elif c < spp_min:
            target.append(spp_min)
        elif e > threshold and c < spp_max:
            target.append(min(spp_max, 2 * c))
        else:
            target.append(c)
    return target, {t for t, (c, x) in enumerate(zip(count.tolist(), target)) if x > c}


@pytest.mark.parametrize("n", R.PLAN_SIZES)
def test_plan_restatement_is_the_scalar_rule(n):
    for name, case in R.plan_cases(n).items():
        target, active = R.plan(**case)
        want_t, want_a = _plan_scalar(**case)
        assert target.tolist() == want_t and active == want_a, name
        assert all(0 <= x <= R.INT_MAX for x in want_t), name  # every target is an int32 the kernel can hold
        b = R.buckets(target, case["count"])
        for t in range(n):
            p = want_t[t] - int(case["count"][t])
            assert b[t] == (int(math.floor(math.log2(p))) if p > 0 else -1)
        if name == "mode0-idle":
            assert not active
        if name == "mode0-all":
            assert len(active) == n


def test_plan_cases_reach_every_bucket_and_every_outcome():
    n = 5000
    cases = R.plan_cases(n)
    for variant in ("mixed", "all"):
        c = cases["mode0-" + variant]
        pend = c["tile_s1"].astype(np.int64) - c["count"]
        assert set(R.buckets(c["tile_s1"], c["count"]).tolist()) - {-1} == set(range(31))
        for b in range(31):  # both ends of every bucket
            assert (pend == 1 << b).any() and (pend == (1 << (b + 1)) - 1).any()
        assert (pend == 0).any() == (variant == "mixed")
    for n_small in (1023, 1024, 1025):  # the sizes around blockDim still hold every bucket
        c = R.plan_case_mode0(n_small, "mixed")
        assert set(R.buckets(c["tile_s1"], c["count"]).tolist()) == set(range(-1, 31))
    c = cases["mode1"]
    assert (c["count"] < 100).any() and (c["count"] == 100).any() and (c["count"] > 100).any()
    # mode 2: every outcome with every kind of error
    c = cases["mode2-classes"]
    target, _ = R.plan(**c)
    thr = c["threshold"]
    outcomes = set(R.refine_outcomes(c["count"], c["err"], target, c["spp_min"], c["spp_max"], thr))
    assert outcomes == {"below_min", "at_max", "stopped", "capped", "doubling"}
    cnt, err = c["count"].astype(np.int64), c["err"]
    mid = (cnt >= c["spp_min"]) & (cnt < c["spp_max"])
    for e, moves in ((-0.0, False), (0.0, False), (thr, False), (float(np.nextafter(thr, 1.0)), True), (math.inf, True)):
        sel = mid & (_bits(err) == _bits(e))
        assert sel.any() and ((target[sel] > cnt[sel]).all() if moves else (target[sel] == cnt[sel]).all()), e
    sel = mid & np.isnan(err)
    assert sel.any() and (target[sel] == cnt[sel]).all()  # a NaN error stops the tile
    assert (np.isnan(err) & (cnt < c["spp_min"])).any()       # ... unless it is below spp_min
    assert ((2 * cnt > c["spp_max"]) & mid & (target == c["spp_max"])).any()  # truly capped: 2 n > spp_max
    over = cnt > c["spp_max"]
    assert over.any() and (target[over] == cnt[over]).all()  # a count above spp_max stays
    c = cases["mode2-overflow"]
    target, _ = R.plan(**c)
    cnt = c["count"].astype(np.int64)
    up = c["err"] > c["threshold"]
    assert "inf_at_one" in R.refine_outcomes(c["count"], c["err"], target, c["spp_min"], c["spp_max"], c["threshold"])
    for n0, want in ((2 ** 30 - 1, 2 ** 31 - 2), (2 ** 30, R.INT_MAX), (2 ** 30 + 1, R.INT_MAX), (R.INT_MAX - 1, R.INT_MAX),
                     (R.INT_MAX, R.INT_MAX)):
        assert (cnt == n0).any() and (target[(cnt == n0) & up] == want).all() and ((cnt == n0) & up).any()
    c = cases["mode2-inf_threshold"]
    target, active = R.plan(**c)
    assert active == set(np.flatnonzero(c["count"] < c["spp_min"]).tolist()) and np.isinf(c["err"]).any()


def test_refine_case_reaches_every_outcome():
    c = R.refine_case()
    err = R.errors(c["sum"], c["q"], c["count"], c["boxes"])
    k = int(np.flatnonzero(c["ids"] == R.REFINE_TILE)[0])
    assert 2 <= c["count"][k] <= 8 and 0.0 < err[k] < math.inf
    assert set(c["count"].tolist()) == set(R.REFINE_COUNTS)
    at, _ = R.plan(c["count"], err, c["count"], 2, spp_min=R.REFINE_MIN, spp_max=R.REFINE_MAX, threshold=err[k])
    below, _ = R.plan(c["count"], err, c["count"], 2, spp_min=R.REFINE_MIN, spp_max=R.REFINE_MAX,
                      threshold=float(np.nextafter(err[k], 0.0)))
    one, _ = R.plan(c["count"], err, c["count"], 2, spp_min=1, spp_max=R.REFINE_MAX, threshold=err[k])
    assert at[k] == c["count"][k] and below[k] == 2 * c["count"][k]
    assert np.array_equal(np.delete(at, k), np.delete(below, k))
    seen = set(R.refine_outcomes(c["count"], err, at, R.REFINE_MIN, R.REFINE_MAX, err[k]))
    assert seen == {"below_min", "doubling", "capped", "at_max", "stopped"}, seen
    assert "inf_at_one" in R.refine_outcomes(c["count"], err, one, 1, R.REFINE_MAX, err[k])
    assert (one[c["count"] == 1] == 2).all()
    shard = R.owned_tiles(R.W, R.H, R.REGION, 1, 3)
    assert R.REFINE_TILE in shard
    moved = set(c["ids"][at > c["count"]].tolist())
    assert moved & set(shard) and set(shard) - moved  # the shard refines some of its tiles and keeps others


@pytest.mark.parametrize("n", R.COMMIT_SIZES)
def test_commit_restatement_and_its_cases(n):
    for with_q in (False, True):
        for lists in R.COMMIT_LISTS:
            c = R.commit_case(n, with_q, lists)
            s, q, cnt = R.commit(**c)
            listed = c["active"][:c["n_active"]].tolist()
            for slot in range(n):
                took = slot in listed and c["done"][slot] != 0
                assert np.array_equal(_bits(s[slot]), _bits((c["partial"] if took else c["sum"])[slot]))
                assert cnt[slot] == (c["tile_s1"] if took else c["count"])[slot]
                if with_q:
                    assert np.array_equal(_bits(q[slot]), _bits((c["q_part"] if took else c["q"])[slot]))
            assert sorted(c["active"].tolist()) == list(range(n))
            assert np.isnan(c["partial"]).any() and not np.array_equal(_bits(c["partial"]), _bits(c["sum"]))
            if n > 1:
                assert set(c["done"].tolist()) == {0, 1}
            if lists == "half":
                assert (c["done"][c["active"][c["n_active"]:]] == 1).all() and 0 < c["n_active"] <= n
                if n > 1:
                    assert not np.array_equal(cnt, c["tile_s1"])  # finished slots that are not listed kept their state


def test_the_seam_and_the_unit_entries_are_exported_where_they_belong():
    names = ("rtr_test_accum_load", "rtr_test_accum_plan", "rtr_test_accum_commit")
    header = open(os.path.join(ROOT, "include", "rtr_hip_test.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib, test_lib = rtr.native.lib(), rtr.native.test_lib()
    for name in names:
        assert name in rtr.native.TEST_EXPORTS and re.search(r"\b%s\s*\(" % name, header)
        assert getattr(test_lib, name) is not None and not hasattr(lib, name)
    assert hasattr(lib, "rtr_debug_accum_load")  # the seam of csrc/rt_debug.h: in the product, not in include/
    for public in ("rtr_hip.h", "rtr_hip_test.h"):
        assert "rtr_debug_accum_load" not in open(os.path.join(ROOT, "include", public)).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", rtr.native.library_path()], stdout=subprocess.PIPE).stdout.decode()
    assert "k_test_" not in syms and "k_stream8" not in syms and "rtr_test_" not in syms
    assert hasattr(rtr.native.Accumulator, "load_state") and hasattr(rtr.native.Context, "accum_plan")
    assert hasattr(rtr.native.Context, "accum_commit")
