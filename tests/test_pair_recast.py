"""The recast of the pair cast (csrc/rt_device.h: trace_pair, pair_recast).  trace_pair holds the pair path alone: at the
first frame where some lane of the wave fails a shared-division verdict it stops, and the caller casts both rays of every
lane again through the single casts of the split-cast kernels.  These tests hold whole waves -- the lane that fails the
vote and the 63 that ride along -- to the CPU oracle: rto_hits gives hit and t of ray A (t_max = inf) and, for ray B,
whether a closest hit exists within b_tmax.  The oracle's hit record names no reference or instance: on scene 21 the
expected instance comes from the oracle's hit point (on which box it lies, if on any), and a_ref is held to the hook's
single-cast column beside it.
The product keeps two texts of the pair cast: the recast in the kernels of the lean material set, the per-frame fallback
(trace_pair_frames) in all the others.  Every case below runs through both, the unsafe-lane waves of
tests/test_pair_shapes.py go through the fallback here as well, and renders with an all-horizontal camera make the
QuadLights-only and the full-set kernels fail votes."""
import numpy as np
import pytest

import _golden as G
import _queue_resident_cases as Q
import test_pair_shapes as S

A = G.A
rtr = G.rtr
WAVE = 64
BAD = 9  # the lane of the wave that fails a vote

TEXTS = ["recast", "frames"]  # rtr_test_pair_cast_text: the lean kernels' text, the other pair-cast kernels'

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _away_from_zero(d, least=0.05):
    return np.where(d < 0.0, d - least, d + least)


def room_pairs(n, seed):
    """ordinary ray pairs of scene 21: A from inside the room towards the walls and boxes (never through the open front),
    B from inside the room to a point of the light, t_max just short of it; no direction component near zero"""
    rng = np.random.default_rng(seed)
    ao = rng.uniform(30.0, 525.0, (n, 3))
    ad = _away_from_zero(rng.normal(size=(n, 3)))
    ad[:, 2] = np.abs(ad[:, 2])
    bo = rng.uniform(30.0, 525.0, (n, 3))
    bd = np.stack([rng.uniform(213.0, 343.0, n), np.full(n, 554.0), rng.uniform(227.0, 332.0, n)], axis=1) - bo
    bd[np.abs(bd) < 0.05] = 0.05
    return {"ao": ao, "ad": ad, "bo": bo, "bd": bd, "at": np.full(n, np.inf), "bt": np.full(n, 0.999)}


def sphere_pairs(n, seed):
    """ordinary ray pairs of scene 23: A downwards onto the spheres and the ground, B upwards with a finite reach"""
    rng = np.random.default_rng(seed)
    ao = rng.uniform([-6.0, 0.3, -6.0], [6.0, 8.0, 6.0], (n, 3))
    ad = _away_from_zero(rng.normal(size=(n, 3)))
    ad[:, 1] = -np.abs(ad[:, 1])
    bo = rng.uniform([-5.0, 0.1, -3.0], [5.0, 1.0, 3.0], (n, 3))
    bd = _away_from_zero(rng.normal(size=(n, 3)))
    return {"ao": ao, "ad": ad, "bo": bo, "bd": bd, "at": np.full(n, np.inf), "bt": rng.uniform(0.5, 12.0, n)}


def oracle_pairs(sc, c):
    """(A hit, A t or a_tmax, A hit point, B occluded) of the CPU oracle"""
    def hits(o, d, t_max):
        recs = np.zeros(len(o), dtype=A.HIT_DTYPE)
        recs["o"], recs["d"], recs["t_min"], recs["t_max"], recs["rng_in"] = o, d, 0.001, t_max, 1
        return G.oracle_records(sc, "rto_hits", recs)
    a, b = hits(c["ao"], c["ad"], c["at"]), hits(c["bo"], c["bd"], c["bt"])
    return a["hit"] != 0, np.where(a["hit"] != 0, a["t"], c["at"]), a["p"], b["hit"] != 0


def check_against_oracle(sc, c, r, rooms=False):
    """hit, the bits of t and B's verdict from the oracle; rooms: scene 21, the instance from the oracle's hit point"""
    hit, t, point, occluded = oracle_pairs(sc, c)
    assert np.array_equal(r["a_ref"] >= 0, hit)
    assert np.array_equal(_bits(r["a_t"]), _bits(t))
    assert np.array_equal(r["b_hit"] != 0, occluded)
    assert np.array_equal(r["a_ref"], r["s_a_ref"]) and np.array_equal(r["a_inst"], r["s_a_inst"])
    assert np.array_equal((r["a_inst"] >= 0), hit)
    if rooms:
        where = hit_places(sc, point, hit)
        assert np.array_equal(r["a_inst"] == 0, where == 0)  # the room is instance 0
        # each box is one instance: a bijection between the places 1, 2 and the instances 1, 2
        pairs = set(zip(where[where > 0].tolist(), r["a_inst"][where > 0].tolist()))
        assert len(pairs) == 2 and {p for p, _ in pairs} == {1, 2} and {i for _, i in pairs} == {1, 2}, pairs
        return hit, occluded, where
    return hit, occluded


def cast(ctx, c, text="recast"):
    return ctx.pair_cast(c["ao"], c["ad"], c["bo"], c["bd"], c["at"], c["bt"], recast=text == "recast")


def hit_places(sc, point, hit):
    """where the oracle's hit points of scene 21 lie: -1 no hit, 0 the room, 1 + k on the box of box_frames(sc)[k] (its
    six rects, taken into the box's frame as translate and rotate_y take a ray's origin)"""
    where = np.where(hit, 0, -1)
    for k, (off, (sn, cs, _), lo, hi) in enumerate(box_frames(sc, extents=True)):
        q = point - np.array(off)
        f = np.stack([cs * q[:, 0] - sn * q[:, 2], q[:, 1], sn * q[:, 0] + cs * q[:, 2]], axis=1)
        tol = 1e-6
        inside = ((f >= lo - tol) & (f <= hi + tol)).all(axis=1)
        on_face = ((np.abs(f - lo) <= tol) | (np.abs(f - hi) <= tol)).any(axis=1)
        where[hit & inside & on_face] = 1 + k
    return where


def box_frames(sc, extents=False):
    """operands (offset, (sin, cos, 0)) of the translate(rotate_y(.)) chains of the scene, in node order; extents: and the
    corners (lo, hi) of the box below, from its XY rects (x0, x1, y0, y1, k)"""
    out = []
    for k in np.flatnonzero(sc.nodes["type"] == A.NODE_TRANSLATE):
        child = int(sc.nodes["a"][k])
        if int(sc.nodes["type"][child]) != A.NODE_ROTATE_Y:
            continue
        ops = (tuple(sc.nodes["f"][k][:3]), (sc.nodes["f"][child][0], sc.nodes["f"][child][1], 0.0))
        if extents:
            lst = sc.nodes[int(sc.nodes["a"][child])]
            assert int(lst["type"]) == A.NODE_LIST
            sides = sc.nodes[sc.list_children[int(lst["a"]):int(lst["a"]) + int(lst["b"])]]
            xy = sides[sides["type"] == A.NODE_XY_RECT]["f"]
            assert len(xy) == 2
            lo = np.array([xy[0][0], xy[0][2], min(xy[0][4], xy[1][4])])
            hi = np.array([xy[0][1], xy[0][3], max(xy[0][4], xy[1][4])])
            ops = ops + (lo, hi)
        out.append(ops)
    return out


def _safe(x):
    return (np.abs(x) >= 2.0 ** -100) & (np.abs(x) <= 2.0 ** 100)


def _fails_only_rotated(sc, o, d):
    """the direction passes every verdict in the world frame and fails one in the frame of a rotated box (host build of
    the frame block); returns the sines of the frames where it fails"""
    assert _safe(d).all()
    failing = []
    for ops in box_frames(sc):
        f = rtr.native.pair_frame_host("TR", ops, o[None], d[None], o[None], d[None])[0]
        assert f["same_frame"] == 1
        if not _safe(f["fd"]).all():
            failing.append(ops[1][0])
    return failing


# A of the bad lane: from the middle of the room; where it ends is the case
CENTRE = np.array([278.0, 278.0, 100.0])
EDGE = 1.2 * 2.0 ** -100  # |d.x| = |d.z|: safe in the world frame, c * x - s * z below 2^-100 after the 15 degree rotate_y


def _bad_lane_cases(sc):
    """name -> function that makes lane BAD of a wave of ordinary pairs the bad one"""
    def a_dir(v):
        def fn(c):
            c["ao"][BAD], c["ad"][BAD] = CENTRE, v
        return fn

    def b_dir(v):
        def fn(c):
            c["bd"][BAD] = v
        return fn

    def a_origin(c):
        c["ao"][BAD, 0] = 2.0 ** 81

    cases = {
        "a_dx_zero_world": a_dir([0.0, -0.3, 1.0]),
        "a_rotated_only": a_dir([EDGE, -1.0, EDGE]),
        "b_rotated_only": b_dir([EDGE, 1.0, EDGE]),
        "origin_beyond_2_80": a_origin,
        # A from the centre with d.x = 0 (fails in the world frame): ends on the back wall, on the tall box (the 15
        # degree one, the first box instance), on the short box (the second), and leaves through the open front
        "a_hits_world": a_dir([0.0, 0.9, 1.0]),
        "a_hits_first_box": a_dir([0.0, -0.05, 1.0]),
        "a_hits_second_box": a_dir([0.0, -0.9, 0.05]),
        "a_misses": a_dir([0.0, 0.1, -1.0]),
    }
    return cases


BAD_CASES = ["a_dx_zero_world", "a_rotated_only", "b_rotated_only", "origin_beyond_2_80", "a_hits_world", "a_hits_first_box",
             "a_hits_second_box", "a_misses"]


@pytest.mark.parametrize("text", TEXTS)
@pytest.mark.parametrize("name", BAD_CASES)
def test_scene21_one_bad_lane_recasts_the_wave(ctx, name, text):
    """One wave of scene 21: 63 ordinary pairs and one lane that fails a vote -- in the world frame, only after a
    rotate_y, on the B side, by its origin -- with A ending on a wall, in either box, or nowhere.  The wave recasts (or,
    in the other text, takes the single-ray scans of the frames that fail), and every lane equals the oracle."""
    sc = G.scene(21)
    c = room_pairs(WAVE, seed=21)
    _bad_lane_cases(sc)[name](c)
    if name == "a_rotated_only":
        assert any(s > 0.25 for s in _fails_only_rotated(sc, c["ao"][BAD], c["ad"][BAD]))  # sin 15 degrees: that box
    if name == "b_rotated_only":
        assert len(_fails_only_rotated(sc, c["bo"][BAD], c["bd"][BAD])) >= 1
    ctx.upload(sc)
    r = cast(ctx, c, text)
    assert (r["recasts"] == (1 if text == "recast" else 0)).all()
    hit, occluded, where = check_against_oracle(sc, c, r, rooms=True)
    others = np.arange(WAVE) != BAD
    assert hit[others].all() and 0 < occluded[others].sum() < WAVE - 1  # walls, boxes, lit and shadowed
    # where the bad lane's A ends: the tall box is the 15 degree one (sin > 0)
    tall = 1 + [k for k, ops in enumerate(box_frames(sc)) if ops[1][0] > 0][0]
    want = {"a_hits_world": 0, "a_hits_first_box": tall, "a_hits_second_box": 3 - tall, "a_misses": -1, "a_rotated_only": 0}
    if name in want:
        assert int(where[BAD]) == want[name]


@pytest.mark.parametrize("text", TEXTS)
def test_recast_and_pair_path_agree_on_the_other_lanes(ctx, text):
    """The same wave twice in one launch, the second time with the bad lane made ordinary: the first recasts, the second
    takes the pair path, and the 63 other lanes get the same bits from both."""
    sc = G.scene(21)
    one = room_pairs(WAVE, seed=22)
    two = {k: v.copy() for k, v in one.items()}
    one["ad"][BAD] = [0.0, -0.3, 1.0]
    c = {k: np.concatenate([one[k], two[k]]) for k in one}
    ctx.upload(sc)
    r = cast(ctx, c, text)
    assert (r["recasts"][:WAVE] == (1 if text == "recast" else 0)).all() and (r["recasts"][WAVE:] == 0).all()
    check_against_oracle(sc, c, r, rooms=True)
    others = np.arange(WAVE) != BAD
    for k in ("a_ref", "a_inst", "b_hit"):
        assert np.array_equal(r[k][:WAVE][others], r[k][WAVE:][others])
    assert np.array_equal(_bits(r["a_t"][:WAVE][others]), _bits(r["a_t"][WAVE:][others]))


@pytest.mark.parametrize("text", TEXTS)
def test_scene23_sphere_verdict_recasts(ctx, text):
    """Scene 23 (spheres in the world frame), two waves: one lane of the first has a direction whose components are safe
    and whose |d|^2 is above 2^100.  The sphere verdict sends that wave to the recast; the second runs the
    spheres-carrying pair scan."""
    sc = G.scene(23)
    c = sphere_pairs(2 * WAVE, seed=23)
    c["ad"][BAD] *= 2.0 ** 51
    assert _safe(c["ad"][BAD]).all() and (c["ad"][BAD] ** 2).sum() > 2.0 ** 100
    ctx.upload(sc)
    r = cast(ctx, c, text)
    assert (r["recasts"][:WAVE] == (1 if text == "recast" else 0)).all() and (r["recasts"][WAVE:] == 0).all()
    hit, occluded = check_against_oracle(sc, c, r)
    assert not hit[BAD]  # (its t is 2^-51 of the others': below t_min)
    assert hit.mean() > 0.8 and len(np.unique(r["a_ref"][hit])) >= 4 and 0 < occluded.sum() < len(occluded)


@pytest.mark.parametrize("flags", [0, A.FLAG_STATIC_GRID])
def test_all_horizontal_camera_recasts_every_camera_ray(ctx, flags):
    """Scene 21 through a camera whose rays all have d.y = 0: every cast of a camera ray recasts, later bounces pair.
    Through the job-queue kernel and through the static grid, bit-equal to the oracle with its segment counts."""
    sc = G.scene(21)
    flat = type(sc).from_bytes(sc.to_bytes())
    flat.camera["vertical"][0] = (0.0, 0.0, 0.0)
    flat.camera["lower_left_corner"][0, 1] = flat.camera["origin"][0, 1]
    ctx.upload(flat)
    p = A.make_params(32, 32, 8, integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)
    out = ctx.render(p)
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    ref, rst = G.oracle_render(flat, p, threads=0)
    assert np.array_equal(_bits(out), _bits(ref))
    assert (st["closest_segments"], st["shadow_segments"]) == (rst["closest_segments"], rst["shadow_segments"])


def test_dead_request_does_not_pin_the_wave_to_the_recast(ctx):
    """The job-queue kernel keeps its shadow request resident while it is dead.  Lane BAD of a wave casts one unsafe B
    (d.x = 0) and then eight more pair casts with no new request: the first cast recasts and retires the stale direction,
    the eight others take the pair path -- 1 recast, not 9."""
    sc = G.scene(21)
    c = room_pairs(WAVE, seed=25)
    c["bd"][BAD, 0] = 0.0
    ctx.upload(sc)
    r = ctx.pair_resident(c["ao"], c["ad"], c["bo"], c["bd"], c["at"], c["bt"], casts=9)
    assert (r["recasts"] == 1).all()
    check_against_oracle(sc, c, r, rooms=True)
    ordinary = room_pairs(WAVE, seed=25)
    r = ctx.pair_resident(ordinary["ao"], ordinary["ad"], ordinary["bo"], ordinary["bd"], ordinary["at"], ordinary["bt"], casts=9)
    assert (r["recasts"] == 0).all()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_unsafe_lanes_through_the_per_frame_fallback(ctx, name):
    """The waves of tests/test_pair_shapes.py -- one lane with an unsafe divisor on either side, signed zeros, NaN, an
    origin at 2^81, dummies -- through the text the kernels outside the lean set run (that file's own test goes through
    the lean kernels' text): reference, instance, the bits of t and B's verdict of the two single casts."""
    make, two = S.SCENES[name]
    sc = make()
    ctx.upload(sc)
    o, d = S._base_rays(name, sc, two)
    c = S.pair_cases(o, d)
    r = ctx.pair_cast(c["ao"], c["ad"], c["bo"], c["bd"], c["at"], c["bt"], recast=False)
    assert (r["recasts"] == 0).all()
    S.check_pair_equals_single(r)
    ordinary = slice(0, len(o))
    assert (r["a_ref"][ordinary] >= 0).mean() > 0.9 and 0 < r["b_hit"][ordinary].sum() < len(o)


def _horizontal(sc, height=None):
    """the scene through a camera whose rays all have d.y exactly 0: every cast of a camera ray fails the vote.  height:
    the camera's y (scene 23's own camera stands above its spheres: level rays from there meet nothing)"""
    flat = type(sc).from_bytes(sc.to_bytes())
    assert flat.camera["lens_radius"][0] == 0.0 and flat.camera["horizontal"][0, 1] == 0.0
    if height is not None:
        flat.camera["origin"][0, 1] = height
    flat.camera["vertical"][0] = (0.0, 0.0, 0.0)
    flat.camera["lower_left_corner"][0, 1] = flat.camera["origin"][0, 1]
    return flat


@pytest.mark.parametrize("flags", [0, A.FLAG_STATIC_GRID])
@pytest.mark.parametrize("name", ["23", "flat_full"])
def test_failed_votes_in_the_kernels_that_keep_the_fallback(ctx, name, flags):
    """Scene 23 (QuadLights-only material set) and a pair scene of the full set through the all-horizontal camera: their
    kernels take the per-frame fallback at every camera ray.  Same bits and segment counts as the split casts, through
    the job-queue kernel and the static grid."""
    ctx.upload(_horizontal(Q.scene(G, name), height=1.0 if name == "23" else None))
    kw = dict(integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    out = ctx.render(A.make_params(32, 32, 8, flags=flags, **kw))
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    split = ctx.render(A.make_params(32, 32, 8, flags=flags | A.FLAG_SPLIT_CASTS, **kw))
    ss = ctx.stats()
    assert ss["flags_in_effect"] & A.FLAG_SPLIT_CASTS
    assert np.array_equal(_bits(out), _bits(split))
    assert (st["samples"], st["closest_segments"], st["shadow_segments"]) == \
        (ss["samples"], ss["closest_segments"], ss["shadow_segments"])
    assert st["shadow_segments"] > 0
