"""Random scenes (tests/_randscene.py) through the C ABI against the pinned CPU oracle: hit records of every
traversal and small renders of every integrator on both pipelines.  The golden scenes are the reference's
forty demo scenes; these graphs add what none of them contains -- coplanar overlapping rects (exact ties in t),
media in the middle of the visiting order next to transformed boxes, dozens of small instances, nested lists
under transforms -- with the oracle (bit-exact against the reference on every golden vector) as the checker."""
import gzip
import os

import numpy as np
import pytest

import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr

CASES = [(11, {}), (12, {}), (13, dict(n_objects=90)), (14, dict(media=True)), (15, dict(media=True, n_objects=60)),
         (16, dict(hollow=True)), (17, dict(n_objects=8, ties=True)), (18, dict(media=True, hollow=True)),
         (19, dict(n_objects=200)), (20, dict(n_objects=40)), (21, dict(media=True, n_objects=12)),
         (22, dict(n_objects=3)), (23, dict(media=True, n_objects=100)), (24, dict(n_objects=60)),
         (25, dict(media=True)), (26, dict(n_objects=30, hollow=True)),
         (27, dict(delta_lights=True)), (28, dict(delta_lights=True, media=True)), (29, dict(delta_lights=True, n_objects=70)),
         (30, dict(lens=0.12)), (31, dict(lens=0.05, media=True, n_objects=40)),
         (32, dict(moved_media=True)), (33, dict(moved_media=True, media=True, n_objects=50))]


# sha256 of every scene above (and of TOP_CASES' big groups) as the generator drew them before it had palettes: the
# default palette must keep drawing the same numbers in the same order
DEFAULT_PALETTE_SHA256 = {
    11: "7515fb056f5ea279cc00e2c31e760743776365928007e0235540dd8dc3dc3d81",
    12: "17ee3e2e091d9b3f01ce85300ead9e6e3c9c905d83105cf1c0eb60da05345a77",
    13: "37e940aa32bb0ed308524b6ef092792dc715281e1235b45aeb014252d77a30e8",
    14: "422a96b1fbef462da4b7d61807ce4a697858af2679533c0132d5361843063633",
    15: "dc0ace99baeedbbb9b96b9bcd677bb62953a66115c68fd35246bb86f2d4d6855",
    16: "6c3cbad091f786bfd2729fe6c5effea01180e153c9da38dec72a79911448fb43",
    17: "fb934a4125d92dfe77f17042ad5b297dfa42c7757b0fbf5a408dcdaa35509877",
    18: "2193c4595285e1230a18e768ce9ed9ed5f1c260086a00e539fe2cddc028112b7",
    19: "e4132255f1784e4033e6096480231a4d2e4edf23c5c96b65496e26db2e814f10",
    20: "89edfb3199bd918a32e65cb836280f5b33cca493f0f0cf0a38be0caf03186f81",
    21: "d76b496fca0efedbd7d6e9a6cb143aafef2d58305fd7f99c9e769515257a101c",
    22: "a82f70b90ff3acbf7e29e2bae2f3fe4161bbf62dca6ba974626eda369e50da71",
    23: "4421fee78d693494168224d89b6a97c0604029c1916e3c1cd8ed40bc1fcab22a",
    24: "e88f743a061b2c5e389ca60694efc4820c7db884c14bdb0cbbd7ec5f789e8967",
    25: "362d55e3d16e39347b7c5f5ee572db700acd776eb75e836dbe750b82418eceb0",
    26: "67c423845707da6df9ac431504bd310a17f7da83de1e593ef1f45f6146b20591",
    27: "8cb9e962549fc0cc0e8218fcea6295542c7787ad7d2dad40477d62fe82776e06",
    28: "686ceec8456f2547b158d8a10eb7e224095cef875cc278ab0d3b4942fec0e6ee",
    29: "2fe17c29ba2fd1f7671d7698afa1e8a8fc8bf0bfd9720398661cef86296e283b",
    30: "458257391f2c118ec0a0f01a4eb1aa2258b6dc17e2c7b8120466c5216ecf0377",
    31: "fe55f3ddc0c7305854a28933880cc631e23ae53adc9275c9ad49390413a048f8",
    32: "b4614150b1f687f3050ab413be3e8c5fdfd6b6396298e0dc393f0711c4ab1c87",
    33: "938dea6ea0b761588756be7b74be9cee3b16c2e565cac443137c33cd5d19e66c",
    41: "8905623d856ddf1bb2fc2de94d45b2ad96d59730837da977d1a800dd6e8d39d5",
    42: "178ee16123b8f7f53ab8821abffae5abc126bb75bac5dbd9bddcad12eca5c3ef",
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_default_palette_reproduces_every_scene_byte_for_byte():
    """CPU: random_scene(seed, **kw) and random_scene(seed, palette="full", **kw) give the scenes they always gave --
    same RNG draws in the same order -- so every seed of CASES and every committed random_<seed> fixture keeps its scene."""
    for seed, kw in CASES + [(41, dict(big_group=True)), (42, dict(big_group=True, n_objects=70))]:
        sc = R.random_scene(seed, **kw)
        assert sc.sha256() == DEFAULT_PALETTE_SHA256[seed], (seed, kw)
        assert R.random_scene(seed, palette="full", **kw).to_bytes() == sc.to_bytes(), (seed, kw)
    assert len(DEFAULT_PALETTE_SHA256) == len(CASES) + 2
    for seed, kw in CASES:  # the fixtures the reference answered (tests/test_random_reference.py)
        path = os.path.join(G.GOLD, "random_%02d.rtrs.gz" % seed)
        if os.path.exists(path):
            with gzip.open(path, "rb") as f:
                assert f.read() == R.random_scene(seed, **kw).to_bytes(), seed


def _hollow_count(sc, kw):
    """hollow spheres the generator's knobs ask for, checked against the scene: exactly 1 / 0 for `hollow` alone"""
    n = int(((sc.nodes["type"] == A.NODE_SPHERE) & (sc.nodes["f"][:, 3] < 0)).sum())
    lists = kw.get("hollow_lists", 0)
    fixed = (1 if kw.get("hollow") else 0) + kw.get("hollow_pairs", 0) + kw.get("bare_hollows", 0)
    assert fixed + 2 * lists <= n <= fixed + 4 * lists, (n, kw)
    return n


@pytest.mark.parametrize("seed,kw", CASES)
def test_random_scenes_validate_and_run_on_the_oracle(seed, kw):
    """CPU: the generator's scenes are well-formed and the oracle traces them (no GPU)."""
    sc = R.random_scene(seed, **kw)
    info = rtr.native.validate_scene(sc)
    assert info["has_media"] == bool(kw.get("media") or kw.get("moved_media")) and info["inverted_boxes"] == _hollow_count(sc, kw)
    if not kw.get("media") and not kw.get("hollow") and not kw.get("moved_media"):
        assert info["fast_ok"] and info["fast_refs"] >= 3
        # dozens of transformed instances sit in a box tree of their own (FSub::top_root): seeds 13 / 19 / 24 / 29
        # are the cases that put the per-lane instance walk in front of the oracle
        assert info["top_trees"] == (1 if kw.get("n_objects", 24) >= 200 else 0)  # seed 19: 80 instances
    if kw.get("media") and not kw.get("hollow") and not kw.get("moved_media"):
        assert info["program_steps"] >= 4  # media under lists only: the step program exists
    if kw.get("hollow"):
        # transformed boxes next to the hollow sphere: no single scan in visiting order -> a guarded step (FStep kind 3)
        assert not info["fast_ok"] and info["program_steps"] >= 2
    if kw.get("moved_media"):
        assert info["program_steps"] >= 4  # a medium under translate / rotate_y: a step with a transform chain
    rays = R.random_rays(seed, 500)
    out = G.oracle_records(sc, "rto_hits", rays)
    assert 50 < int(out["hit"].sum()) <= 500
    img, st = G.oracle_render(sc, A.make_params(24, 16, 2, integrator=4, seed=seed))
    assert np.isfinite(img).all() and img.mean() > 0 and st["samples"] == 24 * 16 * 2


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", CASES)
def test_random_scene_hit_records_equal_the_oracle(ctx, seed, kw):
    sc = R.random_scene(seed, **kw)
    ctx.upload(sc)
    rays = R.random_rays(seed, 6000)
    ora = G.oracle_records(sc, "rto_hits", rays)
    h = ora["hit"] == 1
    # moving_sphere::hit writes no (u,v) (moving_sphere.h:36-62): nothing to compare there
    moving = np.isin(ora["material"], sc.nodes["a"][sc.nodes["type"] == A.NODE_MOVING_SPHERE])
    for exact_order in (False, True):
        ctx.reference_order(exact_order)
        dev = ctx.test_records("hits", rays)
        ctx.reference_order(False)
        tag = "random%02d.%s" % (seed, "reference_order" if exact_order else "compiled")
        assert np.array_equal(dev["hit"], ora["hit"]), tag
        for f in ("front_face", "material", "rng_out"):
            assert np.array_equal(dev[f][h] if f != "rng_out" else dev[f], ora[f][h] if f != "rng_out" else ora[f]), (tag, f)
        # a constant_medium's t is t1 + hit_distance / |d| with hit_distance = -1/density * log(random)
        # (constant_medium.h:88-96): OCML's log against glibc's, last bits; surfaces are +-*/sqrt only
        fog = h & np.isin(ora["material"], np.flatnonzero(sc.materials["type"] == A.MAT_ISOTROPIC))
        surf = h & ~fog
        for f in ("t", "p", "n"):
            bad = int((_bits(dev[f][surf]) != _bits(ora[f][surf])).reshape(int(surf.sum()), -1).any(axis=1).sum())
            assert bad == 0, (tag, f, bad)
            assert np.allclose(dev[f][fog], ora[f][fog], rtol=1e-13, atol=1e-13), (tag, f, "medium")
        uv = surf & ~moving
        # sphere (u,v) go through acos / atan2 (OCML on the device, glibc in the oracle): last bits may differ
        for f in ("u", "v"):
            assert np.allclose(dev[f][uv], ora[f][uv], rtol=0, atol=1e-12), (tag, f)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", CASES)
def test_random_scene_renders_equal_the_oracle(ctx, seed, kw):
    sc = R.random_scene(seed, **kw)
    ctx.upload(sc)
    info = rtr.native.validate_scene(sc)
    wavefront = info["fast_ok"] or info["program_steps"] > 0
    worst = 0.0
    for integ in (0, 1, 2, 3, 4):
        p = A.make_params(48, 32, 4, integrator=integ, seed=100 + seed)
        want, wst = G.oracle_render(sc, p)
        runs = [(A.PIPELINE_MEGAKERNEL, 0), (A.PIPELINE_MEGAKERNEL, A.FLAG_REFERENCE_ORDER)]
        if wavefront:
            runs.append((A.PIPELINE_WAVEFRONT, 0))
        for pipe, flags in runs:
            got = ctx.render(A.make_params(48, 32, 4, integrator=integ, seed=100 + seed, pipeline=pipe, flags=flags))
            st = ctx.stats()
            tag = "random%02d.i%d.pipe%d.flags%d" % (seed, integ, pipe, flags)
            assert st["closest_segments"] == wst["closest_segments"] and st["shadow_segments"] == wst["shadow_segments"], tag
            err = G.rel_l2(got, want)
            worst = max(worst, err)
            assert err <= 1e-12, (tag, err)  # same paths (segment counts equal); libm last bits only
    G.residue("random%02d.renders.worst_rel_l2" % seed, worst, 1e-12)


TOP_CASES = [c for c in CASES if not (c[1].get("media") or c[1].get("hollow") or c[1].get("moved_media"))] + \
            [(41, dict(big_group=True)), (42, dict(big_group=True, n_objects=70))]


@pytest.fixture
def forced_top_tree(monkeypatch):
    """RTR_TOP_MIN=2 (read at every upload, rt_compile.h): a sub-scene with two transformed instances already gets its
    top tree, so every media-free random scene goes through the per-lane instance walk (RT_TRAV_TOP)."""
    monkeypatch.setenv("RTR_TOP_MIN", "2")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", TOP_CASES)
def test_top_tree_walk_equals_the_oracle(ctx, forced_top_tree, seed, kw):
    """The many-instance path (FSub::top_root, trace_top: one box tree over the transformed instances and the leaves
    of the untransformed instance's tree, walked per lane, instance records through vector loads, packed runs with
    per-lane shared reciprocals) against the oracle's in-order scan: hit records bit for bit -- including the exact ties
    between coplanar rects, which this walk meets in tree order -- and small renders of integrators 1 and 4."""
    sc = R.random_scene(seed, **kw)
    assert rtr.native.validate_scene(sc)["top_trees"] == (1 if rtr.native.validate_scene(sc)["fast_instances"] >= 3 else 0)
    ctx.upload(sc)
    rays = R.random_rays(seed, 6000)
    ora = G.oracle_records(sc, "rto_hits", rays)
    dev = ctx.test_records("hits", rays)
    h = ora["hit"] == 1
    assert np.array_equal(dev["hit"], ora["hit"])
    for f in ("front_face", "material"):
        assert np.array_equal(dev[f][h], ora[f][h]), f
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(dev[f][h]), _bits(ora[f][h])), f
    for integ in (1, 4):
        p = A.make_params(48, 32, 4, integrator=integ, seed=200 + seed, pipeline=A.PIPELINE_MEGAKERNEL)
        want, wst = G.oracle_render(sc, p)
        got = ctx.render(p)
        st = ctx.stats()
        assert st["closest_segments"] == wst["closest_segments"] and st["shadow_segments"] == wst["shadow_segments"]
        assert G.rel_l2(got, want) <= 1e-12


@pytest.mark.gpu
def test_top_tree_resolves_ties_across_transform_chains_like_the_reference(ctx, forced_top_tree):
    """tests/_randscene.cross_instance_tie_scene: faces of translated boxes in the planes of rects the list visits before
    and after them.  With a top tree the instances are met in tree order, so every such pair carries its visiting
    position (RT_TIE_FLAG) and the later visit wins, as in the reference's in-order scan."""
    sc = R.cross_instance_tie_scene()
    assert rtr.native.validate_scene(sc)["top_trees"] == 1
    ctx.upload(sc)
    rays = R.cross_instance_tie_rays()
    ora = G.oracle_records(sc, "rto_hits", rays)
    dev = ctx.test_records("hits", rays)
    h = ora["hit"] == 1
    assert np.array_equal(dev["hit"], ora["hit"])
    assert np.array_equal(dev["material"][h], ora["material"][h])
    assert np.array_equal(_bits(dev["t"][h]), _bits(ora["t"][h]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(16, dict(hollow=True)), (32, dict(moved_media=True))])
def test_traversal_machine_refuses_what_it_cannot_run(ctx, seed, kw):
    """Step programs with a guarded step (hollow sphere under bvh_nodes next to transformed boxes) or a medium under
    translate / rotate_y run on the megakernel and the lockstep wavefront stages (the render test above); the
    persistent-threads machine (RTR_FLAG_WF_PERSISTENT) has no such step and says so instead of rendering something else."""
    ctx.upload(R.random_scene(seed, **kw))
    p = A.make_params(32, 16, 2, integrator=4, seed=1, pipeline=A.PIPELINE_WAVEFRONT, flags=A.FLAG_WF_PERSISTENT)
    with pytest.raises(rtr.RtrError) as e:
        ctx.render(p)
    assert e.value.code == A.RTR_ERR_UNSUPPORTED
    ctx.render(A.make_params(32, 16, 2, integrator=4, seed=1, pipeline=A.PIPELINE_WAVEFRONT))


# Several hollow spheres under bvh_nodes (R.bvh_over_top: a tree like bvh_node's over the scene's list, built without
# the reference): nested lists of hollow spheres -- where testing the boxes above one with the running t_max differs
# from the reference's t_max at each node's entry -- and, as controls, hollow-in-glass pairs and bare ones straight
# under the tree, where the two rules agree and the guarded linear scan (RT_TRAV_FLAT_GUARD) must stay.
GUARD_SWEEP = [(s_, dict(spheres_only=True, n_objects=20, hollow_lists=4)) for s_ in (101, 103, 104, 106)] + \
              [(107, dict(spheres_only=True, n_objects=16, hollow_lists=2, bare_hollows=3)),
               (110, dict(spheres_only=True, n_objects=20, hollow_pairs=4, bare_hollows=2)),
               (109, dict(spheres_only=True, n_objects=30, hollow_pairs=3))]


def _guard_scene(seed, kw):
    return R.bvh_over_top(R.random_scene(seed, **kw), seed)


@pytest.mark.parametrize("seed,kw", GUARD_SWEEP)
def test_guard_sweep_scenes_separate_the_rules_and_take_their_paths(seed, kw):
    """CPU: the sweep's scenes with lists of hollow spheres hold rays on which the two box rules differ, and upload
    sends them to the reference-order walk; the pairs-only controls hold none and keep the guarded linear scan."""
    sc = _guard_scene(seed, kw)
    info = rtr.native.validate_scene(sc)
    assert info["inverted_boxes"] == _hollow_count(sc, kw) and not info["has_media"]
    differ = len(R.guard_rule_split(sc, R.random_rays(100000 + seed, 65536)))
    if kw.get("hollow_lists"):
        assert differ > 0 and not info["fast_ok"] and info["program_steps"] == 0, (differ, info)
    else:
        assert differ == 0 and info["fast_ok"], (differ, info)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", GUARD_SWEEP)
def test_guard_sweep_equals_the_oracle(ctx, seed, kw):
    """The device against the oracle on the sweep's scenes: hit records bit for bit on rays the discriminator picked
    (half of them rays where the running-t_max rule would differ), both reference_order settings; MIS and RR renders
    on every pipeline that runs the scene, the MIS one also with RTR_FLAG_SPLIT_CASTS (a guarded scene has no pair cast)."""
    sc = _guard_scene(seed, kw)
    ctx.upload(sc)
    info = rtr.native.validate_scene(sc)
    rays = R.discriminating_rays(sc, seed, 2048)
    ora = G.oracle_records(sc, "rto_hits", rays)
    h = ora["hit"] == 1
    for exact_order in (False, True):
        ctx.reference_order(exact_order)
        dev = ctx.test_records("hits", rays)
        ctx.reference_order(False)
        tag = "guard%d.%s" % (seed, "reference_order" if exact_order else "compiled")
        assert np.array_equal(dev["hit"], ora["hit"]), (tag, int((dev["hit"] != ora["hit"]).sum()))
        for f in ("front_face", "material"):
            assert np.array_equal(dev[f][h], ora[f][h]), (tag, f, int((dev[f][h] != ora[f][h]).sum()))
        for f in ("t", "p", "n"):
            assert np.array_equal(_bits(dev[f][h]), _bits(ora[f][h])), (tag, f)
        for f in ("u", "v"):  # acos / atan2: OCML against glibc
            assert np.allclose(dev[f][h], ora[f][h], rtol=0, atol=1e-12), (tag, f)
    pipes = [A.PIPELINE_MEGAKERNEL] + ([A.PIPELINE_WAVEFRONT] if info["fast_ok"] or info["program_steps"] > 0 else [])
    worst = 0.0
    for integ in (1, 4):
        p = A.make_params(48, 32, 4, integrator=integ, seed=300 + seed)
        want, wst = G.oracle_render(sc, p)
        runs = [(pipe, 0) for pipe in pipes] + ([(A.PIPELINE_MEGAKERNEL, A.FLAG_SPLIT_CASTS)] if integ == 4 else [])
        for pipe, flags in runs:
            got = ctx.render(A.make_params(48, 32, 4, integrator=integ, seed=300 + seed, pipeline=pipe, flags=flags))
            st = ctx.stats()
            tag = "guard%d.i%d.pipe%d.flags%d" % (seed, integ, pipe, flags)
            assert st["closest_segments"] == wst["closest_segments"] and st["shadow_segments"] == wst["shadow_segments"], tag
            assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0, tag
            err = G.rel_l2(got, want)
            worst = max(worst, err)
            assert err <= 1e-12, (tag, err)
    G.residue("guard%d.renders.worst_rel_l2" % seed, worst, 1e-12)
