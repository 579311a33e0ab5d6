"""Hit records of the flat kernels (csrc/rt_device.h: fast_finish_flat, from one finish record per reference) against the
reference-order walk, bit for bit as 64-bit patterns.

The ray queries and the per-ray kernels walk flat scenes with RT_TRAV_FAST, which keeps the two loads of FInst + fprim, so
the compiled side here is the thin entry rtr_test_flat_hits (include/rtr_hip_test.h; ``Context.flat_hits``): the
closest-hit cast of the flat kernels, cast_closest<RT_TRAV_FLAT>, with (u, v) on.  The reference side is
``Context.query_closest(reference_order=True)``.  Scenes and rays: tests/_flatscenes.py."""
import numpy as np
import pytest

import _flatscenes as F
import _golden as G

A = G.A
rtr = G.rtr


REL_L2_BAR = 1e-3  # BASELINE.json north_star tolerance (scene 23 calls libm: tests/test_gpu_parity.py)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _compare(ctx, sc, o, d, want_finish=True, no_uv=None):
    """both casts over the rays; asserts that every ray hits and that the records agree in every bit.  -> reference records.
    ``no_uv(ref)``: mask of the hits on a primitive whose hit() writes no (u, v) -- a moving sphere: the reference-order
    walk keeps those of an earlier, farther hit there, the compiled casts report NaN (include/rtr_testrec.h)"""
    ctx.upload(sc)
    ref = ctx.query_closest(o, d, reference_order=True)
    recs = np.zeros(len(o), dtype=A.HIT_DTYPE)
    recs["o"], recs["d"], recs["t_min"], recs["t_max"], recs["rng_in"] = o, d, 0.001, np.inf, 1
    got, used = ctx.flat_hits(recs)
    assert used == want_finish
    n_hit = int((ref["hit"] != 0).sum())
    print("rays %d, reference hits %d, front faces %d" % (len(o), n_hit, int(ref["front_face"].sum())))
    assert n_hit == len(o) and int((got["hit"] != 0).sum()) == len(o)
    unset = np.zeros(len(o), dtype=bool) if no_uv is None else no_uv(ref)
    for name in ("t", "p", "n", "u", "v"):
        differ = (_bits(got[name]) != _bits(ref[name])).reshape(len(o), -1).any(axis=1)
        if name in ("u", "v"):
            assert np.isnan(got[name][unset]).all()
            differ &= ~unset
        bad = np.nonzero(differ)[0]
        assert len(bad) == 0, (name, len(bad), bad[:8], got[name][bad[:3]], ref[name][bad[:3]])
    assert np.array_equal(got["front_face"], ref["front_face"]), np.nonzero(got["front_face"] != ref["front_face"])[0][:8]
    assert np.array_equal(got["material"], ref["material"])
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("two", ["TR", "RT"])
@pytest.mark.parametrize("flips", range(8))
def test_synthetic_chains_and_flips(ctx, flips, two):
    """Chains none, T, R and T(R) / R(T), a box and a sphere under each, a flip_face at every place of the chain (and two in
    a row on the spheres): random rays, axis-parallel ones, +0 / -0 components, rays from inside each box, rays at its
    edges and corners and at each of its six sides.  Every material is one (chain, side): all of them must be hit."""
    sc = F.flat_scene(flips, two)
    o, d, classes = F.rays_for(sc, two, seed=flips)
    ref = _compare(ctx, sc, o, d)
    hit = set(int(m) for m in ref["material"])
    assert hit == set(range(len(sc.materials))), sorted(set(range(len(sc.materials))) - hit)
    assert set(ref["front_face"]) == {0, 1}
    for name in ("inside_box", "sides", "spheres"):
        assert set(ref["front_face"][classes[name]]) == {0, 1}, name
    # signed zeros reach the records: some normal or point component of an axis-parallel ray's hit is -0
    zero = classes["axis"]
    assert (_bits(ref["n"][zero]) == np.uint64(1 << 63)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_id", [7, 21, 23])
def test_golden_scenes(ctx, scene_id):
    sc = G.scene(scene_id)
    o, d = F.golden_rays(scene_id, sc, seed=scene_id)
    ref = _compare(ctx, sc, o, d)
    assert set(int(m) for m in ref["material"]) == set(range(len(sc.materials)))
    assert set(ref["front_face"]) == {0, 1}


@pytest.mark.gpu
def test_guarded_scene(ctx):
    """a hollow sphere inside a glass shell under bvh_nodes: the flat cast is cast_closest<RT_TRAV_FLAT_GUARD>, the kernel a
    MIS render of it runs, and its hit records come from finish records too.  Both spheres of the shell must be hit, from
    both sides."""
    sc = F.guarded_scene()
    o, d = F.guarded_rays(seed=5)
    ref = _compare(ctx, sc, o, d)
    shell, hollow = len(sc.materials) - 2, len(sc.materials) - 1
    for m in (shell, hollow):
        assert set(ref["front_face"][ref["material"] == m]) == {0, 1}, m
    ctx.render(A.make_params(16, 16, 1, integrator=4, seed=1, pipeline=A.PIPELINE_MEGAKERNEL))
    assert ctx.last_kernel()["trav"] == 7  # RT_TRAV_FLAT_GUARD


@pytest.mark.gpu
@pytest.mark.parametrize("extra", ["three", "moving"])
def test_scene_without_records_takes_the_two_loads(ctx, extra):
    """a flat scene that gets no finish records (a chain of three transforms; a moving sphere): same kernel, the records of
    FInst + fprim, same bits"""
    sc = F.flat_scene(3, "TR", extra=extra)
    o, d, _ = F.rays_for(sc, "TR", seed=11)

    def on_moving_sphere(ref):  # tests/_flatscenes.py: centre (0, 5, 0) at time 0, radius 0.5
        return np.abs(np.linalg.norm(ref["p"] - np.array([0.0, 5.0, 0.0]), axis=1) - 0.5) < 1e-9

    ref = _compare(ctx, sc, o, d, want_finish=False, no_uv=on_moving_sphere if extra == "moving" else None)
    if extra == "moving":
        assert 0 < int(on_moving_sphere(ref).sum()) < 64


@pytest.mark.gpu
def test_scene_that_is_not_flat_is_refused(ctx):
    ctx.upload(G.scene(9))
    with pytest.raises(rtr.native.RtrError) as e:
        ctx.flat_hits(np.zeros(1, dtype=A.HIT_DTYPE))
    assert e.value.code == A.RTR_ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("scene_id", [7, 21, 23])
def test_golden_renders_with_pair_and_split_casts(ctx, scene_id):
    """64x64 spp 16, MIS, megakernel, with the pair cast (where the scene takes it) and with the split casts: the stored
    image of the reference bit for bit for scenes 7 and 21; scene 23 calls sin / cos / pow, where the device's library
    and the reference's differ in a last bit (tests/test_gpu_parity.py: REL_L2_BAR), so there both casts give the same
    bits and those are within that bar of the stored image"""
    img, info = G.image("img_scene%02d_i4_64_spp16.f64" % scene_id)
    ctx.upload(G.scene(scene_id))
    outs = []
    paired = scene_id != 7  # (scene 7 has no light: no shadow ray to pair, tests/test_pair_cast.py)
    for flags in (0, A.FLAG_SPLIT_CASTS):
        p = A.make_params(info["width"], info["height"], info["spp"], integrator=4, seed=info["seed"],
                          pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)
        outs.append(ctx.render(p))
        assert ctx.last_kernel()["trav"] == 4  # RT_TRAV_FLAT: the kernels that read the finish records
        # the flag is reported in effect exactly where it took the pair kernel away: flags = 0 ran the pair loop of a
        # scene that has one, FLAG_SPLIT_CASTS the split loop
        in_effect = bool(ctx.stats()["flags_in_effect"] & A.FLAG_SPLIT_CASTS)
        assert in_effect == (paired and flags != 0), (scene_id, flags)
        assert rtr.native.scene_plan(G.scene(scene_id), 4, flags)["mega_pair"] == (paired and flags == 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    if scene_id == 23:
        assert G.rel_l2(outs[0], img) <= REL_L2_BAR
    else:
        assert np.array_equal(_bits(outs[0]), _bits(img))
