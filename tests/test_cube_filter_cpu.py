"""Filtered cube maps (include/rtr_hip.h: rtr_cube_filter*, rtr_cube_chain_*) without a GPU: the declarations and record
layouts, the parameter and chain checks, and the host-only rtr_cube_filter_one, rtr_cube_chain_plan and
rtr_cube_chain_lookup_one against the numpy restatement of the contract (tests/_cube_filter_ref.py) bit for bit, with
properties that do not depend on the restatement beside them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _cube_filter_ref as FR
import _golden as G

rtr = G.rtr
A = rtr._abi
N = rtr.native

NAMES = ("rtr_cube_filter_defaults", "rtr_cube_filter", "rtr_cube_filter_device", "rtr_cube_filter_one", "rtr_cube_chain_plan",
         "rtr_cube_chain_lookup", "rtr_cube_chain_lookup_device", "rtr_cube_chain_lookup_one")
SHAPES = ((1, 1), (3, 2), (4, 8), (8, 5), (8, 8))  # (S_in, S_out)
ALPHAS = (2.0 ** -10, 0.0625, 1.0)
CUTS = (0.0, 0.5)
INV = A.RTR_ERR_INVALID


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def texels(S, n=1, seed=5):
    """n cubes [n, 6, S, S] of valid records with negative values and magnitudes from 2^-40 to 2^40"""
    rng = np.random.default_rng(seed + 1000 * S)
    t = np.zeros((n, 6, S, S), dtype=A.GATHER_OUT_DTYPE)
    t["v"] = rng.uniform(-1.0, 1.0, t.shape + (3,)) * 2.0 ** rng.integers(-40, 41, t.shape + (3,))
    t["count"], t["valid"] = 4, 1
    return t


def test_declared_exported_and_the_abi_version_stays():
    text = _header()
    lib = N.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in N.EXPORTS
        getattr(lib, name)
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert re.search(r"#define RTR_ABI_VERSION 4\b", text)
    # the header owns up to what the seam-aware filter is and is not
    flat = re.sub(r"\s*\n\s*\*\s?", " ", text)
    assert "continuous across cube edges" in flat and "NOT a true three-face filter at the corners" in flat


def _body(name):
    body = re.search(r"typedef struct %s \{[^\n]*\n(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return " ".join(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split())


def test_struct_layouts_and_defaults():
    assert _body("rtr_cube_filter_params") == "int32_t face_in, face_out; double alpha; double cos_cut; int32_t pad[2];"
    assert _body("rtr_cube_level") == "int32_t face_size, pad; int64_t offset; double alpha;"
    assert _body("rtr_cube_query") == "double d[3]; double alpha;"
    assert C.sizeof(A.CubeFilterParamsC) == 32 == A.CUBE_FILTER_PARAMS_SIZE
    assert C.sizeof(A.CubeLevelC) == 24 == A.CUBE_LEVEL_SIZE
    assert A.CUBE_QUERY_DTYPE.itemsize == 32
    assert [n for n, _ in A.CubeFilterParamsC._fields_] == ["face_in", "face_out", "alpha", "cos_cut", "pad"]
    assert [n for n, _ in A.CubeLevelC._fields_] == ["face_size", "pad", "offset", "alpha"]
    p = N.cube_filter_defaults()
    assert (p.face_in, p.face_out, p.alpha, p.cos_cut, tuple(p.pad)) == (32, 16, 0.25, 0.0, (0, 0))
    assert math.copysign(1.0, p.cos_cut) == 1.0
    with pytest.raises(TypeError):
        N.cube_filter_defaults(samples=1)
    N.lib().rtr_cube_filter_defaults(None)  # tolerated


def test_every_entry_wants_a_context_before_any_device_work():
    lib = N.lib()
    fp = N.cube_filter_defaults(face_in=1, face_out=1)
    rec = np.zeros(12, dtype=A.GATHER_OUT_DTYPE)
    q = N.cube_queries(np.ones((2, 3)), 0.0)
    lv, n_rec = N.cube_chain_plan(1, 1)
    assert lib.rtr_cube_filter(None, C.byref(fp), rec.ctypes.data, rec.ctypes.data + 192, 1) == INV
    assert lib.rtr_cube_filter_device(None, C.byref(fp), rec.ctypes.data, rec.ctypes.data + 192, 1, 1) == INV
    assert lib.rtr_cube_chain_lookup(None, C.byref(lv), 1, rec.ctypes.data, n_rec, q.ctypes.data, rec.ctypes.data + 192, 2) == INV
    assert lib.rtr_cube_chain_lookup_device(None, C.byref(lv), 1, rec.ctypes.data, n_rec, q.ctypes.data, rec.ctypes.data + 192, 2,
                                            1) == INV


GOOD = dict(face_in=2, face_out=2, alpha=0.5, cos_cut=0.25)
BAD = (dict(face_in=0), dict(face_in=513), dict(face_out=0), dict(face_out=513), dict(alpha=2.0 ** -20 * (1 - 2.0 ** -53)),
       dict(alpha=1.0 + 2.0 ** -52), dict(alpha=math.nan), dict(cos_cut=-0.0), dict(cos_cut=-2.0 ** -1074), dict(cos_cut=1.0),
       dict(cos_cut=math.nan))
EDGE = (dict(face_in=1), dict(face_in=512), dict(face_out=1), dict(face_out=512), dict(alpha=2.0 ** -20), dict(alpha=1.0),
        dict(cos_cut=0.0), dict(cos_cut=1.0 - 2.0 ** -53))


def _one(fp, src, face=0, a=0, b=0):
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    return N.lib().rtr_cube_filter_one(C.byref(fp), src.ctypes.data, face, a, b, out.ctypes.data), out


def test_each_parameter_bound_on_both_sides():
    src = np.zeros(6 * 512 * 512, dtype=A.GATHER_OUT_DTYPE)
    src["valid"] = 1
    src["v"] = 1.0
    for over in BAD:
        assert _one(N.cube_filter_defaults(**dict(GOOD, **over)), src)[0] == INV, over
    for over in EDGE:
        assert _one(N.cube_filter_defaults(**dict(GOOD, **over)), src)[0] == 0, over
    fp = N.cube_filter_defaults(**GOOD)
    for k in range(2):
        fp.pad[k] = 1
        assert _one(fp, src)[0] == INV
        fp.pad[k] = 0
    for face, a, b in ((-1, 0, 0), (6, 0, 0), (0, -1, 0), (0, 2, 0), (0, 0, -1), (0, 0, 2)):
        assert _one(fp, src, face, a, b)[0] == INV
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    assert N.lib().rtr_cube_filter_one(None, src.ctypes.data, 0, 0, 0, out.ctypes.data) == INV
    assert N.lib().rtr_cube_filter_one(C.byref(fp), None, 0, 0, 0, out.ctypes.data) == INV
    assert N.lib().rtr_cube_filter_one(C.byref(fp), src.ctypes.data, 0, 0, 0, None) == INV


@pytest.mark.parametrize("cos_cut", CUTS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_filter_one_equals_the_restatement(shape, alpha, cos_cut):
    S_in, S_out = shape
    src = texels(S_in)
    got = N.cube_filter_host(src, face_in=S_in, face_out=S_out, alpha=alpha, cos_cut=cos_cut)
    want = FR.filter_cubes(src, S_out, alpha, cos_cut)
    assert got.shape == (1, 6, S_out, S_out)
    assert _same_bits(got, want)
    assert (got["valid"] == 1).all() and (got["count"] > 0).all()


@pytest.mark.parametrize("S_in", (3, 8))
def test_a_constant_cube_comes_back_constant(S_in):
    """Independent of the restatement.  v = (1 / wsum) * sum(w x) with x constant: both sums round alike term by term
    (ceil(6 S_in^2 / 64) adds per lane and 6 in the tree, relative 2^-53 each at worst on positive terms), the product
    w * x, the reciprocal and the last multiply add one rounding each: (ceil(6 S_in^2 / 64) + 9) * 2^-52 bounds it."""
    src = texels(S_in)
    value = np.array([0.75, 3.0, 1e-3])
    src["v"] = value
    bound = (-(-6 * S_in * S_in // 64) + 9) * 2.0 ** -52
    worst = 0.0
    for alpha in ALPHAS:
        got = N.cube_filter_host(src, face_in=S_in, face_out=4, alpha=alpha, cos_cut=0.0)
        assert (got["valid"] == 1).all()
        worst = max(worst, np.abs(got["v"] / value - 1.0).max())
    print("constant cube, S_in = %d: relative error %.3g (bound %.3g)" % (S_in, worst, bound))
    assert worst <= bound


def test_a_sharp_lobe_returns_the_source():
    """alpha = 2^-10 at equal sizes: D at the texel's own centre is alpha^-4 = 2^40 times the weight a neighbour's
    centre gets, so the filter is the identity within 1e-6 (on values of one magnitude)."""
    src = texels(8)
    src["v"] = np.random.default_rng(3).uniform(0.5, 1.0, src["v"].shape)
    got = N.cube_filter_host(src, face_in=8, face_out=8, alpha=2.0 ** -10, cos_cut=0.0)
    assert np.abs(got["v"] - src["v"]).max() < 1e-6


def test_a_cut_that_leaves_nothing_gives_the_zero_record():
    """1 -> 8 with cos_cut 0.9: the corner texels of every output face are further than acos(0.9) from all six source
    centres (cosine 0.68 to the nearest), so they use nothing; the texels around the face centres use exactly one."""
    src = texels(1)
    got = N.cube_filter_host(src, face_in=1, face_out=8, alpha=0.5, cos_cut=0.9)[0]
    for f in range(6):
        for b in (0, 7):
            for a in (0, 7):
                assert got[f, b, a]["count"] == 0 and got[f, b, a]["valid"] == 0 and not got[f, b, a]["v"].any()
        assert got[f, 3, 3]["count"] == 1 and got[f, 3, 3]["valid"] == 1
        assert np.allclose(got[f, 3, 3]["v"], src[0, f, 0, 0]["v"], rtol=1e-15)


def test_an_invalid_source_texel_invalidates_exactly_the_outputs_that_use_it():
    S_in, S_out, cut = 4, 8, 0.5
    src = texels(S_in)
    bad = (2, 1, 3)  # face, row, column
    src["valid"][0][bad] = 0
    src["v"][0][bad] = np.nan
    got = N.cube_filter_host(src, face_in=S_in, face_out=S_out, alpha=0.25, cos_cut=cut)[0]
    # which outputs use it, from unit vectors made here: the margin keeps rounding out of the decision
    def unit(S, f, b, a):
        u, v = (2 * (a + 0.5)) / S - 1, (2 * (b + 0.5)) / S - 1
        d = np.array([(1, -v, -u), (-1, -v, u), (u, 1, v), (u, -1, -v), (u, -v, 1), (-u, -v, -1)][f], dtype=np.float64)
        return d / np.linalg.norm(d)
    L = unit(S_in, *bad)
    n_bad = 0
    for f in range(6):
        for b in range(S_out):
            for a in range(S_out):
                c = float(unit(S_out, f, b, a) @ L)
                assert abs(c - cut) > 1e-9
                assert got[f, b, a]["valid"] == (0 if c > cut else 1), (f, b, a)
                n_bad += c > cut
    assert 0 < n_bad < 6 * S_out * S_out
    assert not got["v"][got["valid"] == 0].any() and np.isfinite(got["v"]).all()


# ---- chains ----

def _levels(plan):
    return [(lv.face_size, lv.offset, lv.alpha) for lv in plan]


@pytest.mark.parametrize("S,n", ((8, 4), (8, 1), (4096, 13), (1, 3), (5, 5)))
def test_chain_plan(S, n):
    plan, n_records = N.cube_chain_plan(S, n)
    want, want_records = FR.plan(S, n)
    assert _levels(plan) == want and n_records == want_records
    assert all(lv.pad == 0 for lv in plan)
    assert plan[0].face_size == S and plan[0].offset == 0 and plan[0].alpha == 0.0
    if n > 1:
        assert plan[n - 1].alpha == 1.0 and plan[n - 1].face_size == max(S >> (n - 1), 1)
    only = C.c_int64()
    assert N.lib().rtr_cube_chain_plan(S, n, None, C.byref(only)) == 0 and only.value == n_records


def test_chain_plan_rejects():
    lv = (A.CubeLevelC * 16)()
    n = C.c_int64()
    for S, k in ((0, 1), (4097, 1), (8, 0), (8, 14)):
        assert N.lib().rtr_cube_chain_plan(S, k, C.byref(lv), C.byref(n)) == INV
    assert N.lib().rtr_cube_chain_plan(8, 2, C.byref(lv), None) == INV


def chain(S, n_levels, seed=11):
    """(levels as triples, records): every level its own random texels -- a lookup does not care how they were made"""
    levels, n_records = FR.plan(S, n_levels)
    rec = np.zeros(n_records, dtype=A.GATHER_OUT_DTYPE)
    for i, (s, at, _) in enumerate(levels):
        rec[at:at + 6 * s * s] = texels(s, seed=seed + i).reshape(-1)
    return levels, rec


def directions(S):
    """every texel centre, points on every edge, all eight corners, the six axes, exact major-axis ties, unnormalised
    directions, and zero, NaN and inf"""
    d = [FR.centres(S)[0]]
    e = np.linspace(-1.0, 1.0, 2 * S + 3)
    for s1 in (-1.0, 1.0):
        for s2 in (-1.0, 1.0):
            for t in e:  # the twelve edges, corners included; on each two components tie
                d.append([[s1, s2, t], [s1, t, s2], [t, s1, s2]])
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    d.append(axes)
    d.append([[1, 1, 0.25], [1, -0.5, 1], [-0.3, 1, 1], [-1, 1, -1], [2, 2, 2], [-3, 0.1, 3]])  # ties
    rng = np.random.default_rng(S)
    r = rng.standard_normal((40, 3))
    d.append(r * 2.0 ** rng.integers(-30, 31, (40, 1)))
    d.append(axes * (1 - 2.0 ** -53) + np.roll(axes, 1, axis=1))  # a hair off an edge
    d.append([[0, 0, 0], [math.nan, 1, 0], [1, math.inf, 0], [0, 1, -math.inf], [1e-200, 0, 0], [1e200, 1e200, 0]])
    return np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in d])


def chain_queries(levels, S):
    """the directions at alphas below, above, on and between the level alphas; and non-finite alphas"""
    d = directions(S)
    alphas = [-1.0, 2.0, 0.3, 0.017] + [a for _, _, a in levels] + [(a + b) / 2 for (_, _, a), (_, _, b) in zip(levels, levels[1:])]
    q = [N.cube_queries(d, a) for a in alphas]
    q.append(N.cube_queries(d[:8], [math.nan, math.inf, -math.inf, 0.5] * 2))
    return np.concatenate(q)


@pytest.mark.parametrize("n_levels", (1, 4))
@pytest.mark.parametrize("S", (1, 2, 8))
def test_chain_lookup_one_equals_the_restatement(S, n_levels):
    levels, rec = chain(S, n_levels)
    q = chain_queries(levels, S)
    got = N.cube_chain_lookup_host(levels, rec, q)
    want = FR.chain_lookup(levels, rec, q)
    assert _same_bits(got, want)
    assert (got["valid"] == 1).sum() > len(q) * 0.9 and (got["valid"] == 0).sum() >= 6
    assert set(np.unique(got["count"])) <= {0, 1, 2, 3, 4, 5, 6, 7, 8}


def test_a_poisoned_next_level_does_not_matter_on_a_level_alpha():
    levels, rec = chain(8, 4)
    d = directions(8)[:200]
    clean = N.cube_chain_lookup_host(levels, rec, N.cube_queries(d, levels[1][2]))
    s, at, _ = levels[2]
    rec[at:at + 6 * s * s]["valid"] = 0
    rec[at:at + 6 * s * s]["v"] = np.nan
    assert _same_bits(N.cube_chain_lookup_host(levels, rec, N.cube_queries(d, levels[1][2])), clean)
    assert (clean["valid"] == 1).all()
    between = N.cube_chain_lookup_host(levels, rec, N.cube_queries(d, (levels[1][2] + levels[2][2]) / 2))
    assert (between["valid"] == 0).all() and not between["v"].any()
    # clamped below the chain: level 0 alone; above it: t = 1 reads the last two levels
    assert (N.cube_chain_lookup_host(levels, rec, N.cube_queries(d, -3.0))["valid"] == 1).all()


def test_bad_chains_are_rejected():
    rec = np.zeros(6 * 64 + 6 * 16, dtype=A.GATHER_OUT_DTYPE)
    q = N.cube_queries(np.ones((1, 3)), 0.5)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    one = N.lib().rtr_cube_chain_lookup_one

    def rc(levels, n=None):
        lv = N.cube_levels(levels)
        return one(C.byref(lv), len(levels) if n is None else n, rec.ctypes.data, q.ctypes.data, out.ctypes.data)
    good = [(8, 0, 0.0), (4, 384, 1.0)]
    assert rc(good) == 0
    assert rc(good, 0) == INV and rc(good * 7, 14) == INV
    assert rc([(8, 0, 0.5), (4, 384, 0.5)]) == INV and rc([(8, 0, 0.5), (4, 384, 0.25)]) == INV  # not strictly increasing
    assert rc([(8, 0, 0.0), (4, 384, math.nan)]) == INV and rc([(8, 0, -math.inf), (4, 384, 1.0)]) == INV
    assert rc([(0, 0, 0.0)]) == INV and rc([(4097, 0, 0.0)]) == INV and rc([(8, -1, 0.0)]) == INV
    lv = N.cube_levels(good)
    lv[1].pad = 1
    assert one(C.byref(lv), 2, rec.ctypes.data, q.ctypes.data, out.ctypes.data) == INV
    lv[1].pad = 0
    assert one(None, 2, rec.ctypes.data, q.ctypes.data, out.ctypes.data) == INV
    assert one(C.byref(lv), 2, None, q.ctypes.data, out.ctypes.data) == INV
    assert one(C.byref(lv), 2, rec.ctypes.data, None, out.ctypes.data) == INV
    assert one(C.byref(lv), 2, rec.ctypes.data, q.ctypes.data, None) == INV
    # a chain with alphas of its own, not starting at 0, is fine
    assert rc([(8, 0, 0.125), (4, 384, 0.75)]) == 0


def _edge_taps(S):
    """(face, ia, ib) of every tap one step outside a face across an edge (not a corner): 4 S per face"""
    for f in range(6):
        for i in range(S):
            yield f, -1, i
            yield f, S, i
            yield f, i, -1
            yield f, i, S


@pytest.mark.parametrize("S", (1, 2, 3, 8, 16))
def test_seam_taps_land_on_edge_texels_of_another_face(S):
    """Every out-of-face tap lands on an edge texel of another face.  Through the library where texel centres are exact
    (S a power of two): a level whose texel values are their own indices, looked up ON the edge beside the tap's texel,
    where the inside texel and the tap get weight 1/2 each: the result is the mean of the two edge texels."""
    level = texels(S)[0]
    ident = np.arange(6 * S * S, dtype=np.float64).reshape(6, S, S)
    level["v"] = ident[..., None]
    levels = [(S, 0, 0.0)]
    for f, ia, ib in _edge_taps(S):
        f2, row, col = FR.tap(f, ia, ib, S)
        assert f2 != f and (row in (0, S - 1) or col in (0, S - 1))
        # the point of the face between the inside texel and the tap, on the edge, at the inside texel's other coordinate
        if S & (S - 1):
            continue
        ja, jb = min(max(ia, 0), S - 1), min(max(ib, 0), S - 1)
        u = (2.0 * (ja + 0.5)) / S - 1.0 if ia == ja else float(np.sign(ia))
        v = (2.0 * (jb + 0.5)) / S - 1.0 if ib == jb else float(np.sign(ib))
        got = N.cube_chain_lookup_host(levels, level, N.cube_queries([FR.face_d0(f, u, v)], 0.0))[0]
        assert got["valid"] == 1 and got["count"] == 2
        assert got["v"][0] == 0.5 * ident[f, jb, ja] + 0.5 * ident[f2, row, col], (f, ia, ib)


def test_seam_taps_are_symmetric():
    """S = 8: for each of the 6 x 4 x 8 / 2 x 2 = 96 edge taps, the neighbour's outward tap returns to the starting texel"""
    S, n = 8, 0
    for f, ia, ib in _edge_taps(S):
        ja, jb = min(max(ia, 0), S - 1), min(max(ib, 0), S - 1)  # the texel the tap starts from
        f2, row, col = FR.tap(f, ia, ib, S)
        back = [FR.tap(f2, col + da, row + db, S) for da, db in ((-1, 0), (1, 0), (0, -1), (0, 1))
                if not (0 <= col + da < S and 0 <= row + db < S)]
        assert (f, jb, ja) in back, (f, ia, ib)
        n += 1
    assert n == 6 * 4 * S == 2 * 96


# ---- faces ----

def test_prefilter_and_lookup_without_a_context_are_the_loops_of_the_one_forms():
    src = texels(4)[0]
    cube = rtr.Cubemap(src)
    ch = cube.prefilter(levels=3, cos_cut=0.0)
    assert isinstance(ch, rtr.CubeChain) and len(ch) == 3
    levels, n_records = FR.plan(4, 3)
    assert [(lv.face_size, lv.offset, lv.alpha) for lv in ch.levels] == levels and len(ch.records) == n_records
    assert _same_bits(ch.level(0).texels, src)
    for i in (1, 2):
        s, at, alpha = levels[i]
        want = N.cube_filter_host(src, face_in=4, face_out=s, alpha=alpha, cos_cut=0.0)[0]
        assert _same_bits(ch.level(i).texels, want) and ch.level(i).face_size == s
        assert _same_bits(want, FR.filter_cube(src, s, alpha, 0.0))
    d = directions(4)[:150]
    rough = np.linspace(0.0, 1.0, len(d))
    want = N.cube_chain_lookup_host(levels, ch.records, N.cube_queries(d, rough * rough))
    assert _same_bits(ch.lookup_records(d, rough), want)
    assert _same_bits(ch.lookup(d, rough), want["v"])
    assert _same_bits(ch.lookup(d[:5], 0.5), N.cube_chain_lookup_host(levels, ch.records, N.cube_queries(d[:5], 0.25))["v"])


def test_chain_save_hdr_names(tmp_path):
    ch = rtr.Cubemap(texels(2)[0]).prefilter(levels=3)
    paths = ch.save_hdr(str(tmp_path / "env"), 8, 4)
    assert [os.path.basename(p) for p in paths] == ["env.hdr", "env.L1.hdr", "env.L2.hdr"]
    for i, p in enumerate(paths):
        want = tmp_path / "want.hdr"
        ch.level(i).save_hdr(str(want), 8, 4)
        assert open(p, "rb").read() == want.read_bytes()
