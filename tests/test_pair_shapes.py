"""The pair cast below the image level (csrc/rt_device.h: trace_pair; include/rtr_hip_test.h: rtr_test_pair_cast): one ray
pair per lane through trace_pair and, for the same lanes, through the two single casts of the flat kernels, whose text
the frame shapes do not touch.  Reference, instance and the bits of t of ray A and "occluded" of ray B must agree on every
lane -- in frames of every shape, on waves that take the pair path and on waves where one lane sends everybody to the
fallback.  (tests/test_pair_frames.py holds whole renders to the split casts; this file is its unit-level companion.)"""
import numpy as np
import pytest

import _flatscenes as F
import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr
WAVE = 64

THREE_AT = np.array([0.5, 5.0, 0.0])  # roughly where the three-op cluster of three_op_scene stands


def three_op_scene():
    """the room of _flatscenes with three clusters -- in the world frame, under T(R(.)) and under T(R(T(.))), a chain the
    pair cast has no shape for -- and so few instances that it still is a pair-cast scene (F.flat_scene(extra="three")
    has five: instance boxes, the split casts)"""
    b = R.Builder(np.random.default_rng(0))
    top = [b.sphere([0.0, 0.0, 0.0], 14.0, F._grey(b, 0.9))]
    top.append(F._cluster(b, F.chain_of("none", "TR")[1], False))
    (_, off), (_, deg) = F.chain_of("two", "TR")[0]
    top.append(b.translate(b.rotate_y(F._cluster(b, np.zeros(3), False), deg), off))
    top.append(b.translate(b.rotate_y(b.translate(F._cluster(b, np.zeros(3), True), (0.5, 0.0, 0.0)), 20.0), (0.0, 5.0, 0.0)))
    b.quad_light([-2.0, 9.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    return F._scene(b, top)


SCENES = {"scene21": (lambda: G.scene(21), None), "scene23": (lambda: G.scene(23), None), "three": (three_op_scene, "TR")}
for _two in ("TR", "RT"):
    for _flips in range(8):
        SCENES["flips%d_%s" % (_flips, _two)] = ((lambda f=_flips, t=_two: F.flat_scene(f, t)), _two)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base_rays(name, sc, two):
    if two is None:
        o, d = F.golden_rays(int(name[5:]), sc, seed=3, n=4096)
    else:
        o, d, _ = F.rays_for(sc, two)
    n = 4096
    reps = -(-n // len(o))
    o, d = np.tile(o, (reps, 1))[:n], np.tile(d, (reps, 1))[:n]
    if name == "three":  # every fourth ray at the three-op cluster
        rng = np.random.default_rng(9)
        aim = np.arange(n) % 4 == 1
        d[aim] = THREE_AT + rng.uniform(-1.2, 1.2, (int(aim.sum()), 3)) - o[aim]
    return o, d


def _pad(parts):
    """every class of lanes starts on a wave of its own"""
    out = []
    for p in parts:
        n = len(p["ao"])
        fill = (-n) % WAVE
        out.append({k: np.concatenate([v, v[:1].repeat(fill, axis=0)]) for k, v in p.items()})
    return {k: np.concatenate([p[k] for p in out]) for k in out[0]}


def pair_cases(o, d):
    """lanes of the test: ordinary pairs; waves where one lane carries an unsafe divisor on the A side, on the B side, as a
    large, a tiny, a zero or a NaN component; y exactly +-0; an origin at 2^81; the dummy ray on either side and on both"""
    n = len(o)
    rng = np.random.default_rng(5)
    bo, bd = np.roll(o, 7, axis=0), np.roll(d, 7, axis=0)
    bt = np.where(np.arange(n) % 3 == 0, np.inf, rng.uniform(0.5, 12.0, n))
    inf = np.full(n, np.inf)

    def case(sl, **changes):
        p = {"ao": o[sl].copy(), "ad": d[sl].copy(), "bo": bo[sl].copy(), "bd": bd[sl].copy(), "at": inf[sl].copy(),
             "bt": bt[sl].copy()}
        for k, fn in changes.items():
            fn(p[k])
        return p

    def one_lane(comp, value):
        def fn(a):
            for w in range(0, len(a), WAVE):
                a[w + (w // WAVE * 7) % WAVE, comp] = value
        return fn

    def every_lane(comp, values):
        def fn(a):
            a[:, comp] = np.resize(values, len(a))
        return fn

    def dummy_o(a):
        a[:] = 0.0

    def dummy_d(a):
        a[:] = 1.0

    def zero_t(a):
        a[:] = 0.0

    k = 4 * WAVE
    parts = [case(slice(0, n))]
    for q, (side, comp, value) in enumerate([("ad", 0, 2.0 ** -120), ("ad", 2, 2.0 ** 120), ("bd", 0, 2.0 ** 101),
                                             ("bd", 2, 2.0 ** -101), ("ad", 1, 2.0 ** -101), ("bd", 1, 0.0), ("ad", 0, 0.0),
                                             ("ad", 2, -0.0), ("ad", 0, np.nan), ("bd", 2, np.inf), ("ad", 0, 2.0 ** 99),
                                             ("bd", 2, 2.0 ** -100)]):
        parts.append(case(slice(q * k, (q + 1) * k), **{side: one_lane(comp, value)}))
    parts.append(case(slice(0, k), ad=every_lane(1, [0.0, -0.0]), bd=every_lane(1, [-0.0, 0.0, 0.0])))
    parts.append(case(slice(k, 2 * k), ao=one_lane(0, 2.0 ** 81)))
    parts.append(case(slice(2 * k, 3 * k), bo=one_lane(2, -2.0 ** 81)))
    parts.append(case(slice(3 * k, 4 * k), ao=dummy_o, ad=dummy_d, at=zero_t))
    parts.append(case(slice(4 * k, 5 * k), bo=dummy_o, bd=dummy_d, bt=zero_t))
    parts.append(case(slice(5 * k, 6 * k), ao=dummy_o, ad=dummy_d, at=zero_t, bo=dummy_o, bd=dummy_d, bt=zero_t))
    return _pad(parts)


def check_pair_equals_single(r):
    assert np.array_equal(r["a_ref"], r["s_a_ref"])
    assert np.array_equal(r["a_inst"], r["s_a_inst"])
    assert np.array_equal(_bits(r["a_t"]), _bits(r["s_a_t"]))
    assert np.array_equal(r["b_hit"], r["s_b_hit"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_pair_cast_equals_single_casts(ctx, name):
    make, two = SCENES[name]
    sc = make()
    assert rtr.native.scene_plan(sc)["pair_cast"] == 1
    if name == "three":
        assert sorted(rtr.native.pair_frames(sc)) == ["TR", "none", "other"]
    ctx.upload(sc)
    o, d = _base_rays(name, sc, two)
    c = pair_cases(o, d)
    r = ctx.pair_cast(c["ao"], c["ad"], c["bo"], c["bd"], c["at"], c["bt"])
    check_pair_equals_single(r)
    ordinary = slice(0, len(o))
    assert (r["a_ref"][ordinary] >= 0).mean() > 0.9  # the rays are aimed: the agreement is not one of misses
    assert 0 < r["b_hit"][ordinary].sum() < len(o)
    dummies = slice(len(r) - 3 * 4 * WAVE, len(r))
    assert not r["b_hit"][dummies][4 * WAVE:].any() and (r["a_ref"][dummies][:4 * WAVE] == -1).all()


@pytest.mark.gpu
def test_scene21_pair_cast_equals_queries(ctx):
    """... and the public ray queries, which tests/test_queries.py holds to the reference"""
    sc = G.scene(21)
    ctx.upload(sc)
    o, d = _base_rays("scene21", sc, None)
    bo, bd = np.roll(o, 7, axis=0), np.roll(d, 7, axis=0)
    bt = np.random.default_rng(5).uniform(0.5, 12.0, len(o))
    r = ctx.pair_cast(o, d, bo, bd, np.inf, bt)
    check_pair_equals_single(r)
    hits = ctx.query_closest(o, d)
    assert np.array_equal(hits["hit"] != 0, r["a_ref"] >= 0)
    hit = hits["hit"] != 0
    assert hit.mean() > 0.9 and np.array_equal(_bits(hits["t"][hit]), _bits(r["a_t"][hit]))
    occ = ctx.query_occluded(bo, bd, t_max=bt)
    assert np.array_equal(occ, r["b_hit"] != 0) and 0 < occ.sum() < len(occ)
