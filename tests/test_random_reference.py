"""Random scenes answered by the UNMODIFIED reference (oracle/gen_random_golden.py: the harness builds the
reference's own classes from the scene file): hit records and small images of ten seeded scenes that none of its
demo builders produces.  CPU: the oracle reproduces them bit for bit (its pin beyond the forty demo scenes).
GPU: the HIP path against the same vectors, through the C ABI."""
import gzip
import os

import numpy as np
import pytest

import _golden as G

A = G.A
rtr = G.rtr
# "<seed>": a flat hittable_list as generated; "<seed>b": the same objects under the reference's own bvh_node
# 32 / 33: a constant_medium UNDER translate / rotate_y (a step with a transform chain, FStep::xf_first)
# 54: lean materials (palette="lean") with a top tree over its instances; 64: QuadLights-only materials with media
# 02 / 01b / 03b / 04b / 05b: several hollow spheres (GUARD_CASES below)
SEEDS = ["11", "13", "14", "15", "16", "17", "18", "19", "27", "28", "32", "33", "54", "64",
         "13b", "15b", "16b", "18b", "19b", "23b", "26b", "28b", "32b", "33b", "02", "01b", "03b", "04b", "05b"]
# Several hollow spheres (negative radius: an inverted bounding box).  The reference tests each bvh_node box above one
# with the t_max that node was entered with (bvh.h:40-50); testing them all with the running t_max at the sphere's
# visit (the oracle's rto_hits_running_guard) differs where an earlier hollow sphere under the same bvh_node, with no
# box entered in between, was hit outside that node's box.  The fixtures' rays start with such rays.
#   03b, 05b  nested lists of hollow spheres next to solid spheres only: the rule differs; would be one linear scan
#   01b       the same next to transformed boxes: the rule differs; would be guarded program steps (FStep kind 3)
#   04b       hollow-in-glass pairs and bare hollow spheres straight under the tree: the rules agree, the guarded
#             linear scan (RT_TRAV_FLAT_GUARD) stays
#   02        lists of hollow spheres without a bvh_node: nothing to guard
GUARD_CASES = {"03b": "differs", "05b": "differs", "01b": "differs", "04b": "agrees", "02": "agrees"}
W, H, SPP = 48, 32, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _scene(seed):
    with gzip.open(os.path.join(G.GOLD, "random_%s.rtrs.gz" % seed), "rb") as f:
        return rtr.Scene.from_bytes(f.read())


def _writes_uv(sc, gold):
    """moving_sphere::hit and constant_medium::hit write no (u,v) (moving_sphere.h:36-62, constant_medium.h:95-101):
    the reference's record then holds whatever an earlier object left in the hittable_list's temp_rec -- no
    material of these scenes reads it (checker and noise textures take p), so it is not part of the comparison."""
    moving = np.isin(gold["material"], sc.nodes["a"][sc.nodes["type"] == A.NODE_MOVING_SPHERE])
    fog = np.isin(gold["material"], np.flatnonzero(sc.materials["type"] == A.MAT_ISOTROPIC))
    return ~moving & ~fog & ~np.isnan(gold["u"])


def _image(seed, integ):
    return np.fromfile(os.path.join(G.GOLD, "random_%s_i%d.f64" % (seed, integ)), dtype="<f8").reshape(H, W, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_equals_the_reference_on_random_scenes(seed):
    sc = _scene(seed)
    gold = G.records("random_%s_hits.bin" % seed, A.HIT_DTYPE)
    out = G.oracle_records(sc, "rto_hits", gold)
    h = gold["hit"] == 1
    assert 150 < h.sum() and np.array_equal(out["hit"], gold["hit"]) and np.array_equal(out["rng_out"], gold["rng_out"])
    for f in ("front_face", "material"):
        assert np.array_equal(out[f][h], gold[f][h]), f
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(out[f][h]), _bits(gold[f][h])), f
    uv = h & _writes_uv(sc, gold)
    for f in ("u", "v"):
        assert np.array_equal(_bits(out[f][uv]), _bits(gold[f][uv])), f
    for integ in (1, 4):
        info = G.MANIFEST["files"]["random_%s_i%d.f64" % (seed, integ)]["info"]
        img, st = G.oracle_render(sc, A.make_params(W, H, SPP, integrator=integ, seed=100 + int(seed.rstrip("b"))))
        assert np.array_equal(_bits(img), _bits(_image(seed, integ))), integ
        # (the harness counts a cast as a shadow ray by its finite t_max: rays towards a directional or
        # environment light have none, so the split differs there; the sum does not)
        assert st["closest_segments"] + st["shadow_segments"] == info["closest_segments"] + info["shadow_segments"]


@pytest.mark.parametrize("seed", sorted(GUARD_CASES))
def test_guard_fixtures_separate_the_two_box_rules(seed):
    """CPU: the reference's records against the running-t_max rule (rto_hits_running_guard) on the hollow-sphere
    fixtures -- a regeneration that loses the rays on which the rules differ makes this fail, not the GPU test vacuous."""
    sc = _scene(seed)
    gold = G.records("random_%s_hits.bin" % seed, A.HIT_DTYPE)
    run = G.oracle_records(sc, "rto_hits_running_guard", gold)
    differ = int(((run["hit"] != gold["hit"]) | (run["material"] != gold["material"]) |
                  (_bits(run["t"]) != _bits(gold["t"]))).sum())
    if GUARD_CASES[seed] == "differs":
        assert differ >= 8, (seed, differ)
    else:
        assert differ == 0, (seed, differ)


@pytest.mark.parametrize("seed", sorted(GUARD_CASES))
def test_guard_fixtures_take_their_paths(seed):
    """CPU: which traversal upload picks.  Where the running t_max would decide differently from the reference (03b /
    05b / 01b) neither the guarded linear scan nor guarded program steps may run: the reference-order walk answers.
    The control 04b keeps the guarded linear scan, 02 (no bvh_node) the plain one."""
    sc = _scene(seed)
    info = rtr.native.validate_scene(sc)
    hollow = int(((sc.nodes["type"] == A.NODE_SPHERE) & (sc.nodes["f"][:, 3] < 0)).sum())
    assert hollow >= 6 and info["inverted_boxes"] == hollow, (info, hollow)
    if GUARD_CASES[seed] == "differs":
        assert not info["fast_ok"] and info["program_steps"] == 0, info
    else:
        assert info["fast_ok"] and info["program_steps"] == 0, info
    if seed == "04b":
        assert (sc.nodes["type"] == A.NODE_BVH).sum() >= 10


def _xties():
    with gzip.open(os.path.join(G.GOLD, "xties.rtrs.gz"), "rb") as f:
        sc = rtr.Scene.from_bytes(f.read())
    return sc, G.records("xties_hits.bin", A.HIT_DTYPE)


def test_oracle_resolves_ties_across_transform_chains_like_the_reference():
    """Faces of translated / rotated boxes in the planes of rects the list visits before AND after them: the
    material of the reference's record says which object its walk kept (the later one)."""
    sc, gold = _xties()
    out = G.oracle_records(sc, "rto_hits", gold)
    h = gold["hit"] == 1
    assert h.all() and np.array_equal(out["hit"], gold["hit"])
    assert np.array_equal(out["material"], gold["material"]) and np.array_equal(out["front_face"], gold["front_face"])
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(out[f]), _bits(gold[f])), f
    assert len(np.unique(gold["material"])) >= 5  # walls before, walls after and boxes all win somewhere


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_the_reference_on_random_scenes(ctx, seed):
    sc = _scene(seed)
    ctx.upload(sc)
    info = rtr.native.validate_scene(sc)
    gold = G.records("random_%s_hits.bin" % seed, A.HIT_DTYPE)
    h = gold["hit"] == 1
    fog = h & np.isin(gold["material"], np.flatnonzero(sc.materials["type"] == A.MAT_ISOTROPIC))
    surf = h & ~fog
    for ref_order in (False, True):
        ctx.reference_order(ref_order)
        out = ctx.test_records("hits", gold)
        ctx.reference_order(False)
        assert np.array_equal(out["hit"], gold["hit"]) and np.array_equal(out["rng_out"], gold["rng_out"]), ref_order
        for f in ("front_face", "material"):
            assert np.array_equal(out[f][h], gold[f][h]), (f, ref_order)
        for f in ("t", "p", "n"):
            assert np.array_equal(_bits(out[f][surf]), _bits(gold[f][surf])), (f, ref_order)
            assert np.allclose(out[f][fog], gold[f][fog], rtol=1e-13, atol=1e-13), (f, ref_order)  # OCML log
        uv = surf & _writes_uv(sc, gold)
        for f in ("u", "v"):
            assert np.allclose(out[f][uv], gold[f][uv], rtol=0, atol=1e-12), (f, ref_order)  # OCML acos / atan2
    worst = 0.0
    pipes = [A.PIPELINE_MEGAKERNEL] + ([A.PIPELINE_WAVEFRONT] if info["fast_ok"] or info["program_steps"] > 0 else [])
    for integ in (1, 4):
        want = _image(seed, integ)
        for pipe in pipes:
            got = ctx.render(A.make_params(W, H, SPP, integrator=integ, seed=100 + int(seed.rstrip("b")), pipeline=pipe))
            err = G.rel_l2(got, want)
            worst = max(worst, err)
            assert err <= 1e-12, (seed, integ, pipe, err)
    G.residue("random%s.vs_reference.worst_rel_l2" % seed, worst, 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sorted(GUARD_CASES))
def test_split_casts_leave_guarded_scenes_alone(ctx, seed):
    """The pair cast (one instance pass for the shadow ray and the next closest-hit ray) runs on the plain linear scan
    only: on the hollow-sphere fixtures (guarded references, or the reference-order walk) RTR_FLAG_SPLIT_CASTS changes
    no kernel, and the MIS image equals the reference's either way."""
    sc = _scene(seed)
    ctx.upload(sc)
    want = _image(seed, 4)
    kw = dict(integrator=4, seed=100 + int(seed.rstrip("b")), pipeline=A.PIPELINE_MEGAKERNEL)
    out = ctx.render(A.make_params(W, H, SPP, **kw))
    st = ctx.stats()
    split = ctx.render(A.make_params(W, H, SPP, flags=A.FLAG_SPLIT_CASTS, **kw))
    ss = ctx.stats()
    assert np.array_equal(_bits(out), _bits(split))
    assert (st["closest_segments"], st["shadow_segments"]) == (ss["closest_segments"], ss["shadow_segments"])
    assert ss["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    assert G.rel_l2(split, want) <= 1e-12


@pytest.mark.gpu
def test_device_resolves_ties_across_transform_chains_like_the_reference(ctx):
    """The compiled traversal scans instances (one per transform chain) in the order their FIRST primitive is visited;
    where that contradicts the visiting order of two coplanar faces (floor_b sits in the first instance but is
    visited after the box whose bottom lies in its plane) upload flags the pair and their visiting positions decide."""
    sc, gold = _xties()
    ctx.upload(sc)
    assert rtr.native.validate_scene(sc)["fast_ok"]
    for ref_order in (False, True):
        ctx.reference_order(ref_order)
        out = ctx.test_records("hits", gold)
        ctx.reference_order(False)
        assert np.array_equal(out["hit"], gold["hit"]), ref_order
        wrong = int((out["material"] != gold["material"]).sum())
        assert wrong == 0, (ref_order, wrong)
        assert np.array_equal(out["front_face"], gold["front_face"]), ref_order
        for f in ("t", "p", "n"):
            assert np.array_equal(_bits(out[f]), _bits(gold[f])), (f, ref_order)
    want, _ = G.oracle_render(sc, A.make_params(W, H, SPP, integrator=1, seed=9))
    for pipe in (A.PIPELINE_MEGAKERNEL, A.PIPELINE_WAVEFRONT):
        got = ctx.render(A.make_params(W, H, SPP, integrator=1, seed=9, pipeline=pipe))
        assert np.array_equal(_bits(got), _bits(want)), pipe
