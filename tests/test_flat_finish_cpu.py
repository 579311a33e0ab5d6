"""Finish records of flat scenes (csrc/rt_lower.h: build_finish; include/rtr_hip_test.h: rtr_finish_record), without a GPU.

Every expected value is restated here from the record's documented meaning and from the scene description: the primitive
the reference visits at a reference's visiting position (tests/_flatscenes.reference_visits), the wrappers above it, and
for the reduced flip bit a brute-force replay of the wrapper chain over every outcome its set_face_normal calls can have."""
import itertools

import numpy as np
import pytest

import _flatscenes as F
import _golden as G

A = G.A
rtr = G.rtr
plan_of = rtr.native.scene_plan
TIE, GUARD = 1 << 30, 1 << 29  # RT_TIE_FLAG, RT_GUARD_FLAG (csrc/rt_device.h)
KIND = {A.NODE_YZ_RECT: 0, A.NODE_XZ_RECT: 1, A.NODE_XY_RECT: 2, A.NODE_SPHERE: 3}

SCENES = {"scene7": lambda: G.scene(7), "scene21": lambda: G.scene(21), "scene23": lambda: G.scene(23)}
for _two in ("TR", "RT"):
    for _flips in range(8):
        SCENES["flips%d_%s" % (_flips, _two)] = (lambda f=_flips, t=_two: F.flat_scene(f, t))


def replay_front(wrapper_types, first_front, outcomes):
    """`front` of the hit record after the wrappers' epilogues, innermost first (hittable.h:58-61,142-155,168): a flip_face
    inverts it, a translate / rotate_y assigns what its set_face_normal finds (``outcomes``, one per transform)."""
    front, k = first_front, 0
    for t in wrapper_types:
        if t == A.NODE_FLIP_FACE:
            front = not front
        else:
            front, k = outcomes[k], k + 1
    return front


def check_records(sc, plan):
    visits = F.reference_visits(sc)
    fin = plan["finish"]
    assert plan["n_finish"] == plan["n_refs"] == len(fin) > 0
    shapes = set()
    for r in range(plan["n_refs"]):
        node, wrappers = visits[int(plan["ref_flags"][r]) & ~(TIE | GUARD)]
        n, rec = sc.nodes[node], fin[r]
        assert rec["kind"] == KIND[int(n["type"])] and rec["material"] == int(n["a"])
        xf = [w for w in wrappers if int(sc.nodes[w]["type"]) != A.NODE_FLIP_FACE]  # outermost first, like the levels
        assert (rec["levels"] & 3) == len(xf) <= 2
        for k, w in enumerate(xf):
            rot = int(sc.nodes[w]["type"]) == A.NODE_ROTATE_Y
            assert bool(rec["levels"] & (4 << k)) == rot
            want = sc.nodes[w]["f"][:3] if not rot else np.array([sc.nodes[w]["f"][0], sc.nodes[w]["f"][1], 0.0])
            assert rec["op"][k].tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes()
        assert (rec["levels"] >> 2) < (1 << len(xf)) and not rec["op"][len(xf):].any()
        assert rec["g"].tobytes() == np.ascontiguousarray(n["f"][:4]).tobytes()
        # the flip bit: `front` is the last assignment, or the primitive's own, inverted or not
        inner_first = [int(sc.nodes[w]["type"]) for w in reversed(wrappers)]
        assert rec["flip"] in (0, 1)
        for first_front in (False, True):
            for outcomes in itertools.product((False, True), repeat=len(xf)):
                last = outcomes[-1] if xf else first_front
                assert replay_front(inner_first, first_front, outcomes) == (last != bool(rec["flip"]))
        shapes.add("".join("R" if int(sc.nodes[w]["type"]) == A.NODE_ROTATE_Y else "T" for w in xf))
    return shapes


@pytest.mark.parametrize("name", sorted(SCENES))
def test_finish_records_restated(name):
    sc = SCENES[name]()
    plan = plan_of(sc)
    assert plan["flat_scene"] and plan["pick_trav"] == 4  # RT_TRAV_FLAT
    shapes = check_records(sc, plan)
    if name.startswith("flips"):
        assert shapes == {"", "T", "R", name[-2:]}
        flips = int(name[5])
        # the cases the reduction is about are really there: a flip inside a level with none outside it has bit 0
        fin = plan["finish"]
        with_levels = fin[(fin["levels"] & 3) > 0]
        assert set(with_levels["flip"]) == {flips & 1}
        assert set(fin[(fin["levels"] & 3) == 0]["flip"]) == ({0, 1})  # box and sphere differ by the sphere's own flip


def test_golden_scene_chains():
    """scenes 7 and 21: the two blocks are translate(rotate_y(box)), the walls stand in the world frame, and the light of
    scene 21 is a flip_face(xz_rect); scene 23 is spheres and rectangles in the world frame"""
    for scene_id, shapes, kinds in ((7, {"", "TR"}, {0, 1, 2}), (21, {"", "TR"}, {0, 1, 2}), (23, {""}, {0, 1, 3})):
        sc = G.scene(scene_id)
        plan = plan_of(sc)
        assert check_records(sc, plan) == shapes and set(plan["finish"]["kind"]) == kinds
    assert set(plan_of(G.scene(7))["finish"]["flip"]) == {0} and set(plan_of(G.scene(21))["finish"]["flip"]) == {0, 1}


def test_guarded_scene_has_records():
    """a hollow sphere under bvh_nodes next to a cluster with flip_faces: RT_TRAV_FLAT_GUARD in the megakernel, one record
    per reference, none with a level (guard mode compiles world-frame scenes only), the hollow sphere's radius negative"""
    sc = F.guarded_scene()
    plan = plan_of(sc)
    assert plan["flat_guarded"] and not plan["flat_scene"] and plan["mega_trav"] == 7 and plan["n_guard_refs"] == 1
    assert check_records(sc, plan) == {""}
    fin = plan["finish"]
    guarded = fin[(plan["ref_flags"] & GUARD) != 0]
    assert len(guarded) == 1 and guarded["kind"][0] == 3 and guarded["g"][0, 3] == F.HOLLOW_R and guarded["flip"][0] == 1
    assert set(fin["flip"]) == {0, 1}


@pytest.mark.parametrize("extra", ["three", "moving"])
def test_scene_that_does_not_fit_has_no_records(extra):
    """a chain of three transforms, a moving sphere: the scene stays flat and keeps the loads of FInst + fprim"""
    sc = F.flat_scene(0, "TR", extra=extra)
    plan = plan_of(sc)
    assert plan["flat_scene"] and plan["n_refs"] > 0
    assert plan["n_finish"] == 0 and len(plan["finish"]) == 0


def test_scene_that_is_not_flat_has_no_records():
    """scene 9 has box trees: no flat kernel, no records"""
    plan = plan_of(G.scene(9))
    assert not plan["flat_scene"] and not plan["flat_guarded"] and plan["n_finish"] == 0
