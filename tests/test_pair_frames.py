"""Frames of the pair cast (csrc/rt_device.h: trace_pair).  The reciprocal of the world direction's y is made once per
cast and shared by every frame whose chain keeps d.y (FInst flag RT_INST_KEEP_Y), and the rcp_safe verdicts of both
rays are voted on once per frame.  These tests hold that to the split casts (RTR_FLAG_SPLIT_CASTS) bit for bit, with
the same closest / shadow segment counts, on scenes with translated, rotated and nested frames and on directions at
the 2^-100 edge of the shared divisions."""
import numpy as np
import pytest

import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _pair_and_split(ctx, W=64, H=48, spp=8, **kw):
    """(image, stats, ran the pair cast) of the default MIS kernel, checked against the split casts"""
    kw = dict(integrator=4, seed=11, pipeline=A.PIPELINE_MEGAKERNEL, **kw)
    out = ctx.render(A.make_params(W, H, spp, **kw))
    st = ctx.stats()
    split = ctx.render(A.make_params(W, H, spp, flags=A.FLAG_SPLIT_CASTS, **kw))
    ss = ctx.stats()
    assert np.array_equal(_bits(out), _bits(split))
    assert (st["samples"], st["closest_segments"], st["shadow_segments"]) == \
        (ss["samples"], ss["closest_segments"], ss["shadow_segments"])
    return out, st, bool(ss["flags_in_effect"] & A.FLAG_SPLIT_CASTS)


@pytest.mark.gpu
def test_random_transformed_scenes_pair_equals_split(ctx):
    """Random flat scenes of boxes under translate / rotate_y chains, spheres and rects: at least five of them run
    the pair cast, and every one renders the split casts' bits and counts."""
    paired = 0
    for seed in range(1200, 1300):
        sc = R.random_scene(seed, n_objects=4, ties=False)
        if sc.has_media():
            continue
        ctx.upload(sc)
        paired += _pair_and_split(ctx, spp=6)[2]
        if paired >= 5:
            break
    assert paired >= 5


def _edge_camera(sc, scale):
    """scene 21 through a camera whose ray directions have y in [-scale, scale] (x, z as before)"""
    tw = type(sc).from_bytes(sc.to_bytes())
    tw.camera["vertical"][0] = (0.0, 2.0 * scale, 0.0)
    tw.camera["lower_left_corner"][0, 1] = tw.camera["origin"][0, 1] - scale
    return tw


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [2.0 ** -100, 2.0 ** -99, 2.0 ** -101])
def test_directions_at_the_shared_division_edge(ctx, scale):
    """Camera rays with |d.y| around 2^-100: the world verdict on d.y decides every frame of scene 21 (the walls and
    both rotated boxes keep d.y); some waves pair, some fall back, all give the split casts' bits."""
    ctx.upload(_edge_camera(G.scene(21), scale))
    assert _pair_and_split(ctx)[2] is True
    assert _pair_and_split(ctx, spp_chunks=2, tile_first=1, tile_stride=2)[2] is True


@pytest.mark.gpu
def test_scene21_pair_cast_equals_oracle(ctx):
    """The pair-cast kernel on scene 21 (no libm call on its path) against the CPU oracle, bit for bit."""
    sc = G.scene(21)
    ctx.upload(sc)
    p = A.make_params(48, 40, 6, integrator=4, seed=5, pipeline=A.PIPELINE_MEGAKERNEL)
    out = ctx.render(p)
    assert ctx.stats()["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    ref, _ = G.oracle_render(sc, p, threads=0)
    assert np.array_equal(_bits(out), _bits(ref))
