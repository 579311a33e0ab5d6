"""The pair cast (csrc/rt_device.h: trace_pair; csrc/rt_kernels.h: k_mega's PAIR branch): the MIS kernels of flat scenes
cast a bounce's shadow ray and the next closest-hit ray in one pass over the instances.  It is a re-scheduling of the
split casts that RTR_FLAG_SPLIT_CASTS still selects: same image bit for bit and the same closest / shadow segment
counts.  stats()["flags_in_effect"] reports the flag exactly where it changed the kernel, i.e. where the pair cast
is what runs without it."""
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


def _both(ctx, integ, W=96, H=80, spp=12, **kw):
    """(image, stats) of the default kernel and of the split casts; asserts that they agree"""
    kw = dict(integrator=integ, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, **kw)
    out = ctx.render(A.make_params(W, H, spp, **kw))
    st = ctx.stats()
    split = ctx.render(A.make_params(W, H, spp, flags=A.FLAG_SPLIT_CASTS, **kw))
    ss = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    assert np.array_equal(_bits(out), _bits(split))
    assert (st["samples"], st["closest_segments"], st["shadow_segments"]) == \
        (ss["samples"], ss["closest_segments"], ss["shadow_segments"])
    return bool(ss["flags_in_effect"] & A.FLAG_SPLIT_CASTS)


@pytest.mark.gpu
@pytest.mark.parametrize("sid,integ,paired", [(21, 4, True), (21, 3, False), (7, 4, False), (7, 3, False), (23, 4, True)])
def test_golden_scene_pair_cast_equals_split_casts(ctx, sid, integ, paired):
    """Scenes 21 (the Cornell box: three instances of rects and rotated boxes) and 23 (spheres) take the pair cast with
    the MIS integrator; scene 7 (the same box without a light: no shadow ray to pair) and integrator 3 (no flat kernel)
    keep the split casts."""
    ctx.upload(G.scene(sid))
    assert _both(ctx, integ) == paired
    assert _both(ctx, integ, spp_chunks=3, tile_first=1, tile_stride=2) == paired


@pytest.mark.gpu
def test_pair_cast_accumulator_passes_equal_split_casts(ctx):
    """The pair-cast kernels of the accumulator passes (with and without moments) continue the one-shot image, and the
    split casts give the same sums."""
    ctx.upload(G.scene(21))
    kw = dict(integrator=4, seed=3, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    ref = ctx.render(A.make_params(64, 48, 10, **kw))
    for flags in (0, A.FLAG_SPLIT_CASTS):
        for moments in (False, True):
            with ctx.accumulator(A.make_params(64, 48, 10, flags=flags, **kw), moments=moments) as acc:
                acc.render(4)
                acc.render(10)
                assert np.array_equal(_bits(acc.resolve()), _bits(ref)), (flags, moments)


@pytest.mark.gpu
def test_random_flat_scenes_pair_cast_equals_split_casts(ctx):
    """Random scenes of a few objects -- boxes under translate / rotate_y, spheres, rects: those that qualify for the
    pair cast (at most four instances, no moving sphere) render the same bits both ways, and so do the others (the
    split casts either way).  At least two of each kind are met."""
    paired, split = [], []
    for seed in range(600, 640):
        sc = R.random_scene(seed, n_objects=3, ties=False)
        if sc.has_media():
            continue
        ctx.upload(sc)
        (paired if _both(ctx, 4, W=64, H=48, spp=8) else split).append(seed)
        if len(paired) >= 3 and len(split) >= 2:
            break
    assert len(paired) >= 2, (paired, split)
    assert len(split) >= 1, (paired, split)


def _static_twin(sc):
    """a copy of the scene with every moving_sphere replaced by a sphere at its first centre (same radius, material)"""
    tw = type(sc).from_bytes(sc.to_bytes())
    m = tw.nodes["type"] == A.NODE_MOVING_SPHERE
    tw.nodes["f"][m, 3] = tw.nodes["f"][m, 8]
    tw.nodes["type"][m] = A.NODE_SPHERE
    return tw


@pytest.mark.gpu
def test_moving_spheres_fall_back_to_split_casts(ctx):
    """A flat scene with a moving sphere is not a pair-cast scene: the flag changes nothing and is not reported.  The
    same scene with its moving spheres made static IS one, so the moving sphere alone is what keeps it out."""
    for seed in range(700, 800):
        sc = R.random_scene(seed, n_objects=3, ties=False)
        if sc.has_media() or A.NODE_MOVING_SPHERE not in set(int(t) for t in sc.nodes["type"]):
            continue
        ctx.upload(_static_twin(sc))
        if _both(ctx, 4, W=64, H=48, spp=8):
            break
    else:
        pytest.fail("no scene among the seeds whose moving spheres alone keep it from the pair cast")
    ctx.upload(sc)
    assert _both(ctx, 4, W=64, H=48, spp=8) is False


@pytest.mark.gpu
def test_pair_cast_frames_without_shared_divisions(ctx):
    """trace_pair's per-frame fallback: where a ray's direction has a component below 2^-100 (RayDiv::fast false for the
    wave) both rays of that frame take trace_fast's single-ray scans.  Scene 21 through a camera whose rays are all
    horizontal (direction y exactly 0): every camera-ray frame falls back, the later bounces pair; same bits and counts
    as the split casts."""
    sc = G.scene(21)
    flat = type(sc).from_bytes(sc.to_bytes())
    flat.camera["vertical"][0] = (0.0, 0.0, 0.0)
    flat.camera["lower_left_corner"][0, 1] = flat.camera["origin"][0, 1]
    ctx.upload(flat)
    assert _both(ctx, 4) is True
    assert _both(ctx, 4, spp_chunks=2, tile_first=0, tile_stride=3) is True
