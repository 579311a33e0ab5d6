"""Frame shapes of the pair cast (csrc/rt_device.h: FInst::shape, pair_frame; csrc/rt_lower.h: frame_shape), without a GPU.

Shapes: lowering names the transform chain of every instance -- none, T, R, TR (translate outermost), RT, other -- and
the pair cast switches on that name.  The expected names are restated here from the scene description: the chain of
translate / rotate_y wrappers above each primitive the reference visits (tests/_flatscenes.reference_visits).

Frames: the straight-line block of a shape must give the bits of the ray taken down op by op, as translate::hit and
rotate_y::hit do.  The host build of the device function (native.pair_frame_host) is run over all triples of edge
values per component, through every shape with several angles, on either side of the pair, and held to a restatement in
numpy as well.  (The pair cast keeps rcp_safe per component as its verdict: there is no verdict of its own to test.)"""
import itertools
from collections import Counter

import numpy as np
import pytest

import _flatscenes as F
import _golden as G

A = G.A
rtr = G.rtr
frames_of = rtr.native.pair_frames
frame_host = rtr.native.pair_frame_host


def expected_shapes(sc):
    """Counter of shape names, one per distinct chain of transform wrappers above the primitives of ``sc``"""
    chains = {}
    for _, wrappers in F.reference_visits(sc):
        xf = tuple(w for w in wrappers if int(sc.nodes[w]["type"]) != A.NODE_FLIP_FACE)  # outermost first
        name = "".join("R" if int(sc.nodes[w]["type"]) == A.NODE_ROTATE_Y else "T" for w in xf)
        chains[xf] = name if name in ("", "T", "R", "TR", "RT") else "other"
    return Counter(v or "none" for v in chains.values())


@pytest.mark.parametrize("scene_id", [7, 21, 23])
def test_golden_scene_shapes(scene_id):
    sc = G.scene(scene_id)
    got = frames_of(sc)
    assert Counter(got) == expected_shapes(sc)
    if scene_id == 21:  # the room, then the two boxes under translate(rotate_y(.))
        assert got == ["none", "TR", "TR"]
    if scene_id == 23:
        assert got == ["none"]


@pytest.mark.parametrize("two", ["TR", "RT"])
@pytest.mark.parametrize("flips", range(8))
def test_synthetic_scene_shapes(flips, two):
    sc = F.flat_scene(flips, two)
    got = frames_of(sc)
    assert Counter(got) == Counter(["none", "T", "R", two]) == expected_shapes(sc)


def test_three_ops_are_other():
    sc = F.flat_scene(0, "TR", extra="three")
    got = frames_of(sc)
    assert Counter(got) == Counter(["none", "T", "R", "TR", "other"]) == expected_shapes(sc)


def test_two_of_a_kind_are_other():
    """T(T(.)) and R(R(.)) have no block of their own"""
    sc = F.flat_scene(0, "TR")
    two = [k for k in np.flatnonzero(sc.nodes["type"] == A.NODE_TRANSLATE)
           if int(sc.nodes["type"][int(sc.nodes["a"][k])]) == A.NODE_ROTATE_Y]
    assert len(two) == 1  # the translate of the T(R(.)) chain: make its child a translate, too
    inner = int(sc.nodes["a"][two[0]])
    sc.nodes["type"][inner] = A.NODE_TRANSLATE
    assert Counter(frames_of(sc)) == Counter(["none", "T", "R", "other"]) == expected_shapes(sc)


# ---- frames ----------------------------------------------------------------------------------------------------------------
TINY = np.nextafter(0.0, 1.0)
EDGE = [0.0, -0.0, np.nan, np.inf, -np.inf]
for _m in (2.0 ** -101, 2.0 ** -100, 2.0 ** 100, 2.0 ** 101, 2.0 ** 98, 2.0 ** 99, TINY, 2.0 ** -1040):
    EDGE += [_m, -_m]
ORDINARY = [1.0, -0.3]  # so that an edge value also meets ordinary neighbours
TRIPLES = np.array(list(itertools.product(EDGE + ORDINARY, repeat=3)))
ANGLES = [0.0, 35.0, 45.0, 90.0, 100.0, 200.0]
OFFSET = (-3.5, 2.0, 4.0)
SHAPES = ["none", "T", "R", "TR", "RT"]


def _ops(shape, deg):
    rad = deg * np.pi / 180.0
    rot, tr = (np.sin(rad), np.cos(rad), 0.0), OFFSET
    return {"none": (tr, tr), "T": (tr, rot), "R": (rot, tr), "TR": (tr, rot), "RT": (rot, tr)}[shape]


def _ordinary(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-6.0, 6.0, (n, 3)), rng.normal(size=(n, 3))


def restated(shape, ops, o, d):
    """the ray in the frame, op by op, outermost first (hittable.h:53,128-138), in numpy's IEEE doubles"""
    o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
    for kind, f in zip({"none": "", "T": "T", "R": "R", "TR": "TR", "RT": "RT"}[shape], ops):
        if kind == "T":
            o = o - np.array(f)
        else:
            sn, cs = f[0], f[1]
            ox, oz = cs * o[:, 0] - sn * o[:, 2], sn * o[:, 0] + cs * o[:, 2]
            dx, dz = cs * d[:, 0] - sn * d[:, 2], sn * d[:, 0] + cs * d[:, 2]
            o, d = np.stack([ox, o[:, 1], oz], axis=1), np.stack([dx, d[:, 1], dz], axis=1)
    return o, d


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return (a == b).all(axis=1)


@pytest.mark.parametrize("shape", SHAPES)
def test_frame_block_equals_the_chain_op_by_op(shape):
    n = len(TRIPLES)
    o, other = _ordinary(n, 1)
    finite = np.isfinite(TRIPLES).all(axis=1)  # (NaN payloads are nobody's contract)
    with np.errstate(all="ignore"):
        for deg in ANGLES:
            ops = _ops(shape, deg)
            for side in ("A", "B"):
                r = frame_host(shape, ops, TRIPLES if side == "A" else o, TRIPLES if side == "A" else other,
                               o if side == "A" else TRIPLES, other if side == "A" else TRIPLES)
                assert (r["same_frame"][finite] != 0).all(), (shape, deg, side)
                wo, wd = restated(shape, ops, r["ao"], r["ad"])
                assert _same_bits(r["fo"], wo)[finite].all() and _same_bits(r["fd"], wd)[finite].all(), (shape, deg, side)


@pytest.mark.parametrize("shape", SHAPES)
def test_ordinary_rays(shape):
    o, d = _ordinary(4096, 2)
    for deg in ANGLES:
        ops = _ops(shape, deg)
        r = frame_host(shape, ops, o, d, o[::-1], d[::-1])
        wo, wd = restated(shape, ops, o, d)
        assert (r["same_frame"] != 0).all() and _same_bits(r["fo"], wo).all() and _same_bits(r["fd"], wd).all()


def test_signed_zeros_survive_every_shape():
    """-0 components of origin and direction: a shape run as another one with identity operands would return +0"""
    axes = np.concatenate([np.eye(3), -np.eye(3)])  # (-0.0 in the negative ones)
    d = np.tile(axes, (8, 1))
    o = -0.0 * np.ones_like(d)
    for shape in ("none", "T", "R"):
        r = frame_host(shape, _ops(shape, 0.0) if shape == "R" else ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), o, d, o, d[::-1])
        assert (r["same_frame"] != 0).all()
        if shape != "R":  # nothing may touch the direction, and x - (+0) keeps every x
            assert _same_bits(r["fd"], d).all() and _same_bits(r["fo"], o).all()
    for shape in SHAPES:
        for deg in ANGLES:
            r = frame_host(shape, _ops(shape, deg), o, d, o, d[::-1])
            wo, wd = restated(shape, _ops(shape, deg), o, d)
            assert (r["same_frame"] != 0).all() and _same_bits(r["fo"], wo).all() and _same_bits(r["fd"], wd).all(), (shape, deg)
