"""The run loop of the lean pair-cast kernels as one routine (csrc/rt_device.h: pair_runs_lean).  A frame without spheres
of a kernel of the lean material set runs its rect and box runs through one assembly statement that decodes the run word,
fetches the records and keeps the hit state of both rays in place; every other pair-cast kernel keeps pair_runs<...>.

rtr_test_pair_cast_text runs either text of the product on one ray pair per lane -- recast = 1: the lean kernels' (through
the routine), recast = 0: the fallback's (through pair_runs) -- next to the two single casts of the flat kernels.  Every
comparison here is bit equality: reference, instance, the bits of t of ray A and "occluded" of ray B of the pair cast
against the single casts, and of one text against the other.  The scenes are flat, lit, hold no sphere (an instance with a
sphere takes pair_runs<true> in every kernel) and at most four instances; what lowering made of each is checked through
rtr_test_scene_plan and rtr_test_pair_frames, and the run list of every instance -- restated here from lowering's rule:
consecutive references of one type, six sides of one box as one record -- is printed."""
import numpy as np
import pytest

import _golden as G
import _randscene as R
import _flatscenes as F

A = G.A
rtr = G.rtr
WAVE = 64
KIND = {"yz": 0, "xz": 1, "xy": 2}  # FFin::kind of a rect

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
# an instance: (chain, prims); chain: [] or [("T", offset), ("R", degrees)], outermost first; a prim: ("xy" | "xz" | "yz", a0,
# a1, b0, b1, k) or ("box", p0, p1)
def build(instances):
    """-> (Scene, run lists [(type, count)] per instance, first reference per instance)"""
    b = R.Builder(np.random.default_rng(0))
    top, runs, firsts, kinds = [], [], [], []
    for chain, prims in instances:
        firsts.append(len(kinds))
        nodes, rl = [], []
        for p in prims:
            m = F._grey(b, 0.2 + 0.05 * (len(kinds) % 12))
            if p[0] == "box":
                p0, p1 = p[1], p[2]
                nodes.append(b.hlist([b.rect("xy", p0[0], p1[0], p0[1], p1[1], p1[2], m), b.rect("xy", p0[0], p1[0], p0[1], p1[1], p0[2], m),
                                      b.rect("xz", p0[0], p1[0], p0[2], p1[2], p1[1], m), b.rect("xz", p0[0], p1[0], p0[2], p1[2], p0[1], m),
                                      b.rect("yz", p0[1], p1[1], p0[2], p1[2], p1[0], m), b.rect("yz", p0[1], p1[1], p0[2], p1[2], p0[0], m)]))
                kinds += [2, 2, 1, 1, 0, 0]
            else:
                nodes.append(b.rect(*p, m))
                kinds.append(KIND[p[0]])
            if rl and rl[-1][0] == p[0]:
                rl[-1][1] += 1
            else:
                rl.append([p[0], 1])
        runs.append([tuple(r) for r in rl])
        if chain:
            node = b.hlist(nodes)
            for kind, arg in reversed(chain):
                node = b.translate(node, arg) if kind == "T" else b.rotate_y(node, arg)
            top.append(node)
        else:
            top += nodes
    b.quad_light([-2.0, 9.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    sc = F._scene(b, top)
    plan = rtr.native.scene_plan(sc)
    shapes = rtr.native.pair_frames(sc)
    print("run lists:", runs, "frames:", shapes, "references:", plan["n_refs"])
    assert plan["pair_cast"] == 1 and plan["flat_scene"] == 1 and plan["lean_materials"] == 1 and plan["mega_pair"] == 1
    assert plan["n_refs"] == len(kinds) and plan["n_tie_refs"] == 0
    assert shapes == ["".join(k for k, _ in c) or "none" for c, _ in instances]
    assert [int(k) for k in plan["finish"]["kind"]] == kinds  # lowering kept the references in list order
    sc.instances = instances
    return sc, runs, firsts


TR = [("T", (1.5, -0.5, 2.0)), ("R", 35.0)]


def rect_of(axis, q):
    """the q-th rect of a run along ``axis``: planes a step apart, side by side (each can be met from either side), extents
    that differ from rect to rect"""
    return (axis, -1.0 + 2.2 * q, 1.0 + 2.25 * q, -0.9 - 0.05 * q, 1.1 + 0.1 * q, 0.5 + 0.7 * q)


def point_on(prim, u, v, side=None):
    """a point of a prim in its instance's frame; box: on side ``side`` (list order z1 z0 y1 y0 x1 x0)"""
    if prim[0] == "box":
        p0, p1 = np.array(prim[1], dtype=np.float64), np.array(prim[2], dtype=np.float64)
        axis, hi = (2, 1, 0)[side // 2], side % 2 == 0
        p = p0 + np.array([u, v, u * v + 0.3])[:3] % 1.0 * (p1 - p0)
        p[axis] = p1[axis] if hi else p0[axis]
        return p
    ax, a0, a1, b0, b1, k = prim
    a, c = a0 + u * (a1 - a0), b0 + v * (b1 - b0)
    return np.array({"xy": [a, c, k], "xz": [a, k, c], "yz": [k, a, c]}[ax])


def aimed_pairs(instances, n, seed, reach=(0.3, 2.5)):
    """n ray pairs aimed at points of the prims, lane by lane through all of them (box sides included), from origins
    around the scene; every fourth A and every fifth B is a random direction; B's t_max around the distance to its target"""
    rng = np.random.default_rng(seed)
    targets = []
    for chain, prims in instances:
        for p in prims:
            for side in (range(6) if p[0] == "box" else [None]):
                targets.append((chain, p, side))

    def rays(shift):
        o = rng.uniform(-6.0, 6.0, (n, 3))
        d = np.zeros((n, 3))
        for k in range(n):
            chain, p, side = targets[(k + shift) % len(targets)]
            d[k] = F.to_world(chain, point_on(p, rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95), side)) - o[k]
        return o, d

    ao, ad = rays(0)
    bo, bd = rays(3)
    ad[::4] = rng.normal(size=ad[::4].shape)
    bd[::5] = rng.normal(size=bd[::5].shape)
    for d in (ad, bd):
        d[np.abs(d) < 0.01] = 0.01
    return {"ao": ao, "ad": ad, "bo": bo, "bd": bd, "at": np.full(n, np.inf), "bt": rng.uniform(*reach, n)}


def both_texts(ctx, c, n=None):
    """the cases through the lean text (the routine) and through the fallback's (pair_runs): each equal to the single casts
    beside it and the two equal to each other, bit for bit; no vote fails, so the lean text is the pair path alone"""
    sl = slice(0, n)
    out = []
    for recast in (True, False):
        r = ctx.pair_cast(c["ao"][sl], c["ad"][sl], c["bo"][sl], c["bd"][sl], c["at"][sl], c["bt"][sl], recast=recast)
        assert (r["recasts"] == 0).all()
        assert np.array_equal(r["a_ref"], r["s_a_ref"]) and np.array_equal(r["a_inst"], r["s_a_inst"])
        assert np.array_equal(_bits(r["a_t"]), _bits(r["s_a_t"]))
        assert np.array_equal(r["b_hit"], r["s_b_hit"])
        out.append(r)
    lean, plain = out
    for k in ("a_ref", "a_inst", "b_hit"):
        assert np.array_equal(lean[k], plain[k]), k
    assert np.array_equal(_bits(lean["a_t"]), _bits(plain["a_t"]))
    return lean


# ---- rect counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("axis", ["xy", "xz", "yz"])
def test_rect_runs_of_every_length(ctx, axis, count):
    """One world instance: a run of 1 .. 5 rects of one type -- the odd record alone, one trip, trip and odd record, two
    trips, two trips and the odd record -- and one rect of the next type behind it, whose reference follows the run's."""
    other = {"xy": "xz", "xz": "yz", "yz": "xy"}[axis]
    inst = [([], [rect_of(axis, q) for q in range(count)] + [(other, -2.0, 2.0, -2.0, 2.0, -1.5)])]
    sc, runs, _ = build(inst)
    assert runs == [[(axis, count), (other, 1)]]
    ctx.upload(sc)
    r = both_texts(ctx, aimed_pairs(inst, 2 * WAVE, seed=count))
    assert set(r["a_ref"].tolist()) >= set(range(count + 1))  # every record of the run is somebody's closest hit
    assert 0 < r["b_hit"].sum() < len(r)


# ---- boxes ----------------------------------------------------------------------------------------------------------------
BOX1 = ("box", (-0.8, -0.7, -0.9), (0.9, 0.8, 0.7))
BOX2 = ("box", (1.4, -0.5, -0.6), (2.6, 1.2, 0.8))


@pytest.mark.parametrize("boxes", [1, 2])
@pytest.mark.parametrize("frame", ["world", "TR"])
def test_box_runs(ctx, frame, boxes):
    """1 and 2 boxes as one run, in the world frame and under T(R(.)); the world frame holds a floor besides, so that the
    scene has a run in each of two instances in the TR case"""
    chain = [] if frame == "world" else TR
    inst = [(chain, [BOX1, BOX2][:boxes])]
    if frame == "TR":
        inst = [([], [("xz", -8.0, 8.0, -8.0, 8.0, -3.0)])] + inst
    sc, runs, firsts = build(inst)
    assert runs[-1] == [("box", boxes)]
    ctx.upload(sc)
    r = both_texts(ctx, aimed_pairs(inst, 2 * WAVE, seed=10 + boxes))
    sides = set(range(firsts[-1], firsts[-1] + 6 * boxes))
    assert len(sides & set(r["a_ref"].tolist())) >= 5 * boxes and 0 < r["b_hit"].sum() < len(r)
    assert (r["a_inst"][r["a_ref"] >= firsts[-1]] == len(inst) - 1).all()


def test_references_behind_a_box_run(ctx):
    """Rect runs, a box run and rect runs again in one instance, and a second instance behind it: a box takes six
    references, and everything behind it is numbered from there."""
    inst = [([], [("xz", -3.0, 3.0, -3.0, 3.0, -2.0), ("xz", -3.0, 3.0, -3.0, 3.0, 3.0), ("xz", -1.0, 1.0, -1.0, 1.0, 2.5), BOX1,
                  ("xy", -3.0, 3.0, -2.0, 3.0, 3.0)]),
            (TR, [BOX1, ("yz", -1.0, 1.0, -1.0, 1.0, 1.6), ("yz", -1.2, 1.2, -1.2, 1.2, -1.9)])]
    sc, runs, firsts = build(inst)
    assert runs == [[("xz", 3), ("box", 1), ("xy", 1)], [("box", 1), ("yz", 2)]] and firsts == [0, 10]
    ctx.upload(sc)
    r = both_texts(ctx, aimed_pairs(inst, 4 * WAVE, seed=20))
    seen = set(r["a_ref"].tolist())
    assert {9, 16, 17} <= seen and len(seen & set(range(3, 9))) >= 5 and len(seen & set(range(10, 16))) >= 5
    assert (r["a_inst"] == np.where(r["a_ref"] < 0, -1, (r["a_ref"] >= 10).astype(np.int32))).all()


# ---- ties -----------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_later_reference(ctx):
    """Two rects of one run in the same plane, written as z = +0 and z = -0 (the same plane and the same t for every ray
    that does not start on it; lowering compares the bits of the planes and flags no tie), and a rect in the plane of a
    box's z0 side behind the box run: the test accepts t == t_max, so ray A ends on the later reference."""
    inst = [([], [("xy", -1.0, 1.0, -1.0, 1.0, 0.0), ("xy", -0.5, 1.5, -0.5, 1.5, -0.0)]),
            (TR, [("box", (-0.5, -0.5, 0.0), (0.5, 0.5, 1.0)), ("xy", -0.4, 0.4, -0.4, 0.4, -0.0)])]
    sc, runs, firsts = build(inst)
    assert runs == [[("xy", 2)], [("box", 1), ("xy", 1)]]
    ctx.upload(sc)
    rng = np.random.default_rng(31)
    n = 2 * WAVE
    # first wave: at the overlap of the two world rects from z < 0; second: at the small rect on the box's z0 side from below it
    target = np.concatenate([np.stack([rng.uniform(-0.4, 0.9, WAVE), rng.uniform(-0.4, 0.9, WAVE), np.zeros(WAVE)], axis=1),
                             np.array([F.to_world(TR, [u, v, 0.0]) for u, v in rng.uniform(-0.35, 0.35, (WAVE, 2))])])
    ao = target + np.concatenate([np.stack([rng.uniform(-0.3, 0.3, WAVE), rng.uniform(-0.3, 0.3, WAVE), rng.uniform(-0.4, -0.2, WAVE)], axis=1),
                                  np.array([F.to_world([TR[1]], [u, v, -0.3]) for u, v in rng.uniform(-0.05, 0.05, (WAVE, 2))])])
    c = {"ao": ao, "ad": target - ao, "bo": ao.copy(), "bd": target - ao, "at": np.full(n, np.inf), "bt": np.full(n, 1.5)}
    r = both_texts(ctx, c)
    assert (r["a_ref"][:WAVE] == 1).all()  # not 0, which it meets first at the same t
    assert (r["a_ref"][WAVE:] == firsts[1] + 6).all() and (r["a_inst"][WAVE:] == 1).all()  # not the box's z0 side, firsts[1] + 1
    assert r["b_hit"].all()


# ---- origins on planes, directions along them -----------------------------------------------------------------------------
def test_origins_on_planes_and_rays_along_them(ctx):
    """A ray that starts on a rect's plane (t = 0 < t_min: that rect is not hit, what lies behind it is), and one that
    runs along a plane with the smallest component that still passes the verdict (|d| = 2^-100: t is huge and finite)."""
    far = [("T", (-6.0, 0.5, -5.0)), ("R", 35.0)]
    inst = [([], [("xy", -2.0, 2.0, -2.0, 2.0, 1.0), ("xy", -2.0, 2.0, -2.0, 2.0, 2.0), ("xz", -2.0, 2.0, 0.0, 3.0, -3.0)]), (far, [BOX1])]
    sc, _, _ = build(inst)
    ctx.upload(sc)
    c = aimed_pairs(inst, 2 * WAVE, seed=41)
    on = np.arange(2 * WAVE) % 2 == 0
    c["ao"][on, 2] = 1.0  # on the first rect's plane, inside it
    c["ao"][on, :2] = np.random.default_rng(42).uniform(-1.5, 1.5, (int(on.sum()), 2))
    c["ad"][on] = [0.01, 0.02, 1.0]
    c["bo"][on] = c["ao"][on]
    c["bd"][on] = [0.01, 0.02, 1.0]
    c["bt"][on] = 1.5
    c["ad"][1::8, 2] = 2.0 ** -100
    c["bd"][3::8, 1] = -2.0 ** -100
    r = both_texts(ctx, c)
    assert (r["a_ref"][on] == 1).all() and r["b_hit"][on].all()  # the second rect, one unit on


# ---- ray B ----------------------------------------------------------------------------------------------------------------
def test_ray_b_dead_alone_and_at_the_edge_of_its_reach(ctx):
    inst = [([], [("yz", -1.0, 1.0, -1.0, 1.0, -5.0 - 0.7 * q) for q in range(3)] + [("xz", -8.0, 8.0, -8.0, 8.0, -3.0)]),
            (TR, [BOX1, BOX2])]
    sc, _, _ = build(inst)
    ctx.upload(sc)
    base = aimed_pairs(inst, WAVE, seed=51)
    live = both_texts(ctx, base)

    dead = {k: v.copy() for k, v in base.items()}
    dead["bt"][:] = 0.0  # no lane casts B: every side leaves through the wave-level exit
    r = both_texts(ctx, dead)
    assert not r["b_hit"].any()
    assert np.array_equal(r["a_ref"], live["a_ref"]) and np.array_equal(_bits(r["a_t"]), _bits(live["a_t"]))

    lane = int(np.flatnonzero(live["b_hit"])[0])
    one = {k: v.copy() for k, v in dead.items()}
    one["bt"][lane] = base["bt"][lane]  # B lives in one lane alone
    r = both_texts(ctx, one)
    assert r["b_hit"][lane] == 1 and r["b_hit"].sum() == 1
    assert np.array_equal(r["a_ref"], live["a_ref"])

    # every lane: B straight at a point of a side of the first box from 0.3 in front of it (d = target - origin: t = 1 at
    # the side), its reach just short of the side and just beyond it
    rng = np.random.default_rng(52)
    edge = {k: v.copy() for k, v in base.items()}
    for k in range(WAVE):
        side = k % 6
        target = point_on(BOX1, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), side)
        out = np.array([0.05, 0.07, 0.06])  # oblique: no direction component is 0 in any frame
        out[(2, 1, 0)[side // 2]] = 0.3 if side % 2 == 0 else -0.3
        edge["bo"][k] = F.to_world(TR, target + out)
        edge["bd"][k] = F.to_world(TR, target) - edge["bo"][k]
    short, beyond = {k: v.copy() for k, v in edge.items()}, {k: v.copy() for k, v in edge.items()}
    short["bt"][:] = 1.0 - 2.0 ** -20
    beyond["bt"][:] = 1.0 + 2.0 ** -20
    assert not both_texts(ctx, short)["b_hit"].any()
    assert both_texts(ctx, beyond)["b_hit"].all()


# ---- partial waves --------------------------------------------------------------------------------------------------------
def test_partial_waves(ctx):
    """n = 1, 63, 65 and 128 records of the same list: a lane returns what it returns in the full launch whoever else is
    there, and the one lane of the second wave of n = 65 what it returns alone"""
    inst = [([], [rect_of("xz", q) for q in range(3)] + [rect_of("xy", 0)]), (TR, [BOX1])]
    sc, _, _ = build(inst)
    ctx.upload(sc)
    c = aimed_pairs(inst, 2 * WAVE, seed=61)
    full = both_texts(ctx, c)
    assert (full["a_ref"] >= 0).sum() > WAVE and 0 < full["b_hit"].sum() < 2 * WAVE
    for n in (1, 63, 65):
        r = both_texts(ctx, c, n)
        for k in ("a_ref", "a_inst", "b_hit"):
            assert np.array_equal(r[k], full[k][:n]), (n, k)
        assert np.array_equal(_bits(r["a_t"]), _bits(full["a_t"][:n]))
    alone = both_texts(ctx, {k: v[WAVE:WAVE + 1] for k, v in c.items()})
    for k in ("a_ref", "a_inst", "b_hit"):
        assert alone[k][0] == full[k][WAVE]
    assert _bits(alone["a_t"])[0] == _bits(full["a_t"])[WAVE]


# ---- misses, and the last side of the last box ----------------------------------------------------------------------------
def test_waves_that_miss_and_waves_that_end_on_the_last_side(ctx):
    inst = [([], [("xz", -3.0, 3.0, -3.0, 3.0, -2.0)]), (TR, [BOX1, BOX2])]
    sc, _, firsts = build(inst)
    ctx.upload(sc)
    rng = np.random.default_rng(71)
    n = 2 * WAVE
    ao, ad = np.zeros((n, 3)), np.zeros((n, 3))
    # first wave: from above everything, upwards
    ao[:WAVE] = rng.uniform(-2.0, 2.0, (WAVE, 3)) + [0.0, 6.0, 0.0]
    ad[:WAVE] = rng.uniform(-0.5, 0.5, (WAVE, 3)) + [0.0, 1.0, 0.0]
    # second: at the x0 side of the second box -- the last side of the last box -- from outside it; the first box lies on
    # the far side of it, so the closest hit is that side
    for k in range(WAVE, n):
        target = point_on(BOX2, rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), 5)
        ao[k] = F.to_world(TR, target + [-0.1, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
        ad[k] = F.to_world(TR, target) - ao[k]
    ad[np.abs(ad) < 1e-3] = 1e-3
    c = {"ao": ao, "ad": ad, "bo": ao.copy(), "bd": ad.copy(), "at": np.full(n, np.inf), "bt": np.full(n, 1.5)}
    r = both_texts(ctx, c)
    assert (r["a_ref"][:WAVE] == -1).all() and (r["a_inst"][:WAVE] == -1).all() and not r["b_hit"][:WAVE].any()
    assert np.isinf(r["a_t"][:WAVE]).all()
    assert (r["a_ref"][WAVE:] == firsts[1] + 11).all() and (r["a_inst"][WAVE:] == 1).all() and r["b_hit"][WAVE:].all()


# ---- renders --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene21_render():
    sc = G.scene(21)
    p = A.make_params(32, 32, 8, integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    ref, rst = G.oracle_render(sc, p, threads=0)
    return sc, ref, rst


@pytest.mark.parametrize("flags", [0, A.FLAG_STATIC_GRID])
def test_scene21_renders_equal_the_oracle(ctx, scene21_render, flags):
    """scene 21, 32 x 32, spp 8, through the job-queue kernel and through the static grid: the oracle's bits"""
    sc, ref, rst = scene21_render
    ctx.upload(sc)
    p = A.make_params(32, 32, 8, integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)
    out = ctx.render(p)
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    assert np.array_equal(_bits(out), _bits(ref))
    assert (st["closest_segments"], st["shadow_segments"]) == (rst["closest_segments"], rst["shadow_segments"])


def test_scene21_accumulator_passes_equal_one_render(ctx, scene21_render):
    """the accumulator twin of the kernel: passes of 3 + 5 samples are the one-shot render of 8"""
    sc, ref, _ = scene21_render
    ctx.upload(sc)
    p = A.make_params(32, 32, 8, integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    one = ctx.render(p)
    with ctx.accumulator(p) as acc:
        acc.render(3)
        acc.render(8)
        got = acc.resolve()
    assert np.array_equal(_bits(got), _bits(one)) and np.array_equal(_bits(got), _bits(ref))
