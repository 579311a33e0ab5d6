"""Probe distance maps (include/rtr_hip.h: rtr_probe_depth, rtr_probe_lookup_visible and their device-pointer forms) on
the GPU.  The maps are held bit for bit to the contract's own reference: the restatement's reduction
(tests/_probe_depth_ref.py) of rtr_query_closest over the rays and states of rtr_probe_depth_ray.  Batch shapes, bad probes,
the device entries behind a queued render, the lookup kernel against the host form, a baked two-room scene and the
command-line tool follow.

csrc/rtr_probe_depth.hip holds five k_probe_depth<traversal>, one per traversal of k_query_closest; which one a call
launched the context records on the host (Context.last_probe_depth).  The parameter block has no flags, so the
reference-order walks run on the scenes that need them whatever the flags: RT_TRAV_EXACT where a moving sphere carries a
material that reads (u, v), RT_TRAV_MEDIA where hollow spheres under a bvh_node cannot be compiled.  The last test asserts
that the tests of this module launched, and compared, every one of the five."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _probe_depth_ref as DR
import _probe_ref as PR
import _randscene as R
from test_probe_depth_cpu import CASES, _reference

rtr = G.rtr
A = G.A
N = rtr.native

pytestmark = pytest.mark.gpu

SEED = 7
DISPLACE = {21: 5.0, 9: 5.0, 23: 0.05}
T_MAX = {21: 250.0, 9: 250.0, 23: 0.6}  # short enough that rays miss, long enough that rays hit
INSIDE_TALL_BOX_21 = np.array([[365.0, 165.0, 353.0]])  # inside the tall block of the Cornell box
WIDTH_SAMPLES = (2, 3, 4, 9, 16, 17, 32, 33, 65, 129)

# RT_TRAV_* of csrc/rt_device.h
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)
TRAV_NAME = ["EXACT", "MEDIA", "FAST", "PROGRAM", "FLAT", "TOP", "PROGRAM_EXT", "FLAT_GUARD"]
DEPTH_TABLE = {FAST, TOP, PROGRAM_EXT, MEDIA, EXACT}
SEEN = set()  # what the tests of this module launched and compared


def _note(ctx, samples):
    g = ctx.last_probe_depth()
    assert g is not None and 1 << g["lg"] == GR.group_size(samples), (samples, g)
    SEEN.add(g["trav"])
    return g["trav"]


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _points(sid, n):
    return PR.displaced_points(sid, DISPLACE[sid], n)


def _want(ctx, pts, **kw):
    """The maps the contract defines, PROBE_DEPTH_DTYPE [n, T, T]: rtr_query_closest over the rays of rtr_probe_depth_ray,
    reduced by the restatement.  The scene must be uploaded."""
    rays = ctx.probe_depth_rays(pts, **kw)
    hits = ctx.query_closest(rays.reshape(-1)).reshape(rays.shape)
    return DR.reduce(hits["hit"], hits["t"], hits["front_face"], kw["t_max"]), hits


def _case(ctx, pts, **kw):
    want, hits = _want(ctx, pts, **kw)
    out = ctx.probe_depth(pts, **kw)
    trav = _note(ctx, kw["samples"])
    assert out.shape == want.shape
    assert _same_bits(out, want), kw
    assert (out["valid"] == 1).all() and (out["pad"] == 0).all()
    return trav, out, hits


@pytest.mark.parametrize("T,samples", ((1, 1), (3, 5), (8, 64), (3, 100), (1, 130)))
@pytest.mark.parametrize("sid", (21, 23))
def test_maps_equal_the_reduction_of_the_closest_hits(ctx, sid, T, samples):
    ctx.upload(G.scene(sid))
    n = 2 if T == 8 else 3
    trav, out, hits = _case(ctx, _points(sid, n), map_size=T, samples=samples, seed=SEED, t_max=T_MAX[sid], time=0.25)
    assert trav == FAST
    if T * T * samples >= 45:
        assert (hits["hit"] == 1).any() and (hits["hit"] == 0).any()  # some rays end on a surface, some at t_max
        top = T_MAX[sid] * (1.0 + 16 * 2.0 ** -53)  # (1.0 / N) * (N x t_max) is t_max up to the ten roundings of lane sums, tree and scale
        assert (out["mean"] > 0).all() and (out["mean"] <= top).all() and (out["mean2"] >= out["mean"] ** 2 * (1 - 1e-12)).all()
        assert (out["hits"] <= samples).all() and (out["back"] <= out["hits"]).all()


@pytest.mark.parametrize("samples", WIDTH_SAMPLES)
def test_every_group_width(ctx, samples):
    ctx.upload(G.scene(21))
    assert _case(ctx, _points(21, 3), map_size=3, samples=samples, seed=SEED, t_max=T_MAX[21])[0] == FAST


def test_without_jitter_and_from_inside_a_transformed_box(ctx):
    """front_face is the reference's: translate::hit and rotate_y::hit set it again from the normal that already faces the
    ray (geometry/hittable.h:59, 153), so under a transform every hit is a front face, from inside the block too.  (A probe
    inside a box that stands under no transform does see back faces: test_classify_drops_the_probe_inside_a_box.)"""
    ctx.upload(G.scene(21))
    kw = dict(map_size=4, samples=5, seed=SEED, t_max=400.0)
    _, plain, _ = _case(ctx, INSIDE_TALL_BOX_21, **kw)
    _, fixed, hits = _case(ctx, INSIDE_TALL_BOX_21, jitter=0, **kw)
    assert not _same_bits(plain, fixed)
    assert (fixed["hits"] == 5).all() and (fixed["mean"] < 240.0).all()  # every ray ends on the block: its diagonal is 404
    assert (hits["front_face"] == 0).sum() == fixed["back"].sum() == 0
    # all five samples of a texel are one ray: the mean is its distance (5 x t / 5 is t up to two roundings)
    assert np.abs(fixed["mean"] / hits["t"][..., 0] - 1.0).max() <= 8 * 2.0 ** -53


@pytest.mark.parametrize("t_min", (0.0, -1.0))
def test_below_the_shared_division_bound(ctx, t_min):
    """t_min < 2^-100: the launch takes the plain divisions, as rtr_query_closest does for such rays"""
    ctx.upload(G.scene(21))
    _case(ctx, _points(21, 3), map_size=3, samples=5, seed=SEED, t_min=t_min, t_max=T_MAX[21])


def _uv_order_scene():
    """a moving sphere whose material reads (u, v): only the reference-order walk is right (RT_TRAV_EXACT without a flag)"""
    b = R.Builder(np.random.default_rng(0))
    base = G.scene(23)
    t = np.zeros(1, dtype=A.TEXTURE_DTYPE)
    t["type"], t["a"] = A.TEX_IMAGE, 0
    b.texs.append(t)
    image = len(b.texs) - 1
    grey = b.material(A.MAT_LAMBERTIAN, [b.solid([0.5, 0.5, 0.5])])
    b.quad_light([-2.0, 6.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    top = [b.rect("xz", -5.0, 5.0, -5.0, 5.0, 0.0, grey), b.sphere([0.0, 1.0, 0.0], 0.5, grey), b.sphere([2.0, 1.0, 0.0], 0.5, grey),
           b.moving_sphere([0.0, 1.0, -2.0], [0.0, 1.5, -2.0], 0.5, b.material(A.MAT_LAMBERTIAN, [image]))]
    images = np.zeros(1, dtype=A.IMAGE_DTYPE)
    images["width"], images["height"], images["offset"] = 2, 2, 0
    return rtr.Scene(b.hlist(top), R._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), R._cat(b.mats, A.MATERIAL_DTYPE),
                     R._cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], images, np.full(12, 128, dtype=np.uint8),
                     R._cat(b.lights, A.LIGHT_DTYPE), base.camera.copy(), np.array([0.5, 0.6, 0.8]))


def _other_scene(key):
    if key == "top":
        return R.random_scene(19, n_objects=200)
    if key == "hollow":
        return R.random_scene(16, hollow=True)
    if key == "uv order":
        return _uv_order_scene()
    with gzip.open(os.path.join(G.GOLD, "random_03b.rtrs.gz"), "rb") as f:  # hollow spheres the compiled scene cannot hold
        return rtr.Scene.from_bytes(f.read())


@pytest.mark.parametrize("key,want", (("top", TOP), ("hollow", PROGRAM_EXT), ("uv order", EXACT), ("guarded", MEDIA)))
def test_the_other_traversals(ctx, key, want):
    ctx.upload(_other_scene(key))
    pts = np.array([[0.3, 1.7, -1.1], [1.1, 0.9, -2.4], [-2.0, 2.5, 0.5]])
    trav, out, hits = _case(ctx, pts, map_size=3, samples=9, seed=SEED, t_max=4.0, time=0.5)
    assert trav == want, TRAV_NAME[trav]
    assert (hits["hit"] == 1).any() and (hits["hit"] == 0).any()


def test_media_draw_inside_the_cast(ctx):
    ctx.upload(G.scene(9))
    pts = _points(9, 3)
    trav, out, hits = _case(ctx, pts, map_size=3, samples=9, seed=SEED, t_max=T_MAX[9])
    assert trav == PROGRAM_EXT
    rays = ctx.probe_depth_rays(pts, map_size=3, samples=9, seed=SEED, t_max=T_MAX[9])
    assert (hits["rng_out"] != rays["rng_state"]).any()  # the media drew


def test_sharding_by_point_base_and_an_empty_batch(ctx):
    ctx.upload(G.scene(21))
    pts = _points(21, 5)
    kw = dict(map_size=3, samples=5, seed=SEED, t_max=T_MAX[21])
    whole = ctx.probe_depth(pts, **kw)
    for cut in (1, 2, 4):
        split = np.concatenate([ctx.probe_depth(pts[:cut], **kw), ctx.probe_depth(pts[cut:], point_base=cut, **kw)])
        assert _same_bits(split, whole), cut
    assert not _same_bits(ctx.probe_depth(pts[2:], **kw), whole[2:])  # (the base matters)
    wrap = ctx.probe_depth(pts[[1, 0]], point_base=0xFFFFFFFF, **kw)  # k is taken modulo 2^32
    assert _same_bits(wrap[1], whole[0]) and not _same_bits(wrap[0], whole[1])
    assert ctx.probe_depth(pts[:0], **kw).shape == (0, 3, 3)


def test_device_entry_behind_a_render_bad_probes_and_alignment(ctx):
    """T = 3 and 5 samples: 8 lanes per texel, so a wave holds 8 texels, of two probes where 9 k is no multiple of 8, and
    the last wave of every batch is partly past the end"""
    import torch
    ctx.upload(G.scene(21))
    T, S, n = 3, 5, 4
    rec = T * T
    kw = dict(map_size=T, samples=S, seed=SEED, t_max=T_MAX[21])
    pts = N.probe_points(_points(21, n))
    host = ctx.probe_depth(pts, **kw)
    W = H = 128
    rp = A.make_params(W, H, 8, seed=3)
    want_img = ctx.render(rp)
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    d_out = torch.full(((n * rec + 1) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    fb = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.render_into(rp, fb.data_ptr(), W, blocking=False)
    ctx.probe_depth_into(d_pts.data_ptr(), d_out.data_ptr(), n, blocking=False, **kw)
    ctx.synchronize()
    raw = d_out.cpu().numpy()
    assert _same_bits(raw[:n * rec * 32].view(A.PROBE_DEPTH_DTYPE).reshape(n, T, T), host)
    assert (raw[n * rec * 32:] == 0xA5).all()  # nothing behind the batch is written
    assert _same_bits(fb.cpu().numpy(), want_img) and ctx.stats()["samples"] == W * H * 8  # and the render is the render
    bad = pts.copy()
    bad["p"][1, 0] = np.nan
    bad["p"][2, 2] = -np.inf
    d_bad = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    for m in (0, 1, 2, 3, 4):
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.probe_depth_into(d_bad.data_ptr(), d_out.data_ptr(), m, blocking=True, **kw)
        raw = d_out.cpu().numpy()
        got = raw[:m * rec * 32].view(A.PROBE_DEPTH_DTYPE).reshape(m, T, T)
        assert (raw[m * rec * 32:] == 0xA5).all(), m
        for k in range(m):
            assert _same_bits(got[k], np.zeros((T, T), dtype=A.PROBE_DEPTH_DTYPE) if k in (1, 2) else host[k]), (m, k)
    assert _same_bits(d_bad.cpu().numpy(), bad.view(np.uint8))  # the input is not written
    with pytest.raises(rtr.RtrError) as e:
        ctx.probe_depth_into(d_pts.data_ptr() + 4, d_out.data_ptr(), 1, blocking=True, **kw)
    assert e.value.code == A.RTR_ERR_INVALID and "aligned" in e.value.message
    with pytest.raises(rtr.RtrError):
        ctx.probe_depth_into(d_pts.data_ptr(), d_out.data_ptr() + 4, 1, blocking=True, **kw)
    # the host entry rejects the batch, names the index and leaves the output
    out = np.zeros((n, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    with pytest.raises(rtr.RtrError) as e:
        ctx.probe_depth(bad, out=out, **kw)
    assert e.value.code == A.RTR_ERR_INVALID and "index 1" in e.value.message and (out.view(np.uint8) == 0xA5).all()


def test_a_slice_boundary_inside_a_call(ctx):
    """257 probes at T = 64 and one sample: 1 052 672 texels, so the host entry's second slice (2^20 texels each) starts
    with probe 256, whose number under the seed the slice must carry on.  The device entry serves the call in one launch."""
    import torch
    ctx.upload(G.scene(21))
    rng = np.random.default_rng(5)
    pts = N.probe_points(np.array([100.0, 300.0, 100.0]) + rng.random((257, 3)) * 300.0)
    kw = dict(map_size=64, samples=1, seed=SEED, t_max=300.0)
    host = ctx.probe_depth(pts, **kw)
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(host.size * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_depth_into(d_pts.data_ptr(), d_out.data_ptr(), len(pts), blocking=True, **kw)
    assert (host["valid"] == 1).all() and _same_bits(host, d_out.cpu().numpy().view(A.PROBE_DEPTH_DTYPE).reshape(host.shape))
    last, _ = _want(ctx, pts[256:], point_base=256, **kw)  # the probe the boundary falls in, against the closest hits
    assert _same_bits(host[256:], last)


def test_before_upload_and_params():
    pts = N.probe_points(_points(21, 2))
    out = np.zeros(2 * 4, dtype=A.PROBE_DEPTH_DTYPE)
    with rtr.Context(0) as c:
        L = c._L

        def calls(dp, pts_ptr=pts.ctypes.data, out_ptr=out.ctypes.data, m=2):
            return (L.rtr_probe_depth(c._h, C.byref(dp), pts_ptr, out_ptr, m),
                    L.rtr_probe_depth_device(c._h, C.byref(dp), pts_ptr, out_ptr, m, 1))

        base = dict(map_size=2, samples=3, t_max=100.0)
        ok = N.probe_depth_defaults(**base)
        assert calls(ok) == (A.RTR_ERR_NO_SCENE,) * 2
        assert calls(N.probe_depth_defaults(map_size=0, t_max=1.0)) == (A.RTR_ERR_INVALID,) * 2  # params before the scene
        c.upload(G.scene(21))
        invalid = (A.RTR_ERR_INVALID,) * 2
        for kw in (dict(map_size=0), dict(map_size=65), dict(samples=0), dict(samples=(1 << 20) + 1), dict(jitter=2), dict(jitter=-1),
                   dict(time=np.nan), dict(time=np.inf), dict(t_min=np.nan), dict(t_min=-np.inf), dict(t_max=np.inf),
                   dict(t_max=np.nan), dict(t_max=0.001), dict(t_max=0.0)):
            assert calls(N.probe_depth_defaults(**dict(base, **kw))) == invalid, kw
        assert calls(N.probe_depth_defaults(map_size=2, samples=3)) == invalid  # t_max has no default
        padded = N.probe_depth_defaults(**base)
        padded.pad = 1
        assert calls(padded) == invalid
        assert calls(ok, m=-1) == invalid and calls(ok, pts_ptr=None) == invalid and calls(ok, out_ptr=None) == invalid
        assert L.rtr_probe_depth(c._h, None, pts.ctypes.data, out.ctypes.data, 2) == A.RTR_ERR_INVALID
        assert not out.view(np.uint8).any()  # nothing ran
        assert calls(ok, pts_ptr=None, out_ptr=None, m=0) == (A.RTR_OK,) * 2  # n == 0: no launch, nothing read
        assert c.last_probe_depth() is None  # none of this launched anything
        assert L.rtr_probe_depth(c._h, C.byref(ok), pts.ctypes.data, out.ctypes.data, 2) == A.RTR_OK and (out["valid"] == 1).all()


def test_maps_leave_renders_and_accumulators_alone(ctx):
    ctx.upload(G.scene(21))
    kw = dict(map_size=3, samples=5, seed=SEED, t_max=T_MAX[21])
    p8 = A.make_params(64, 64, 8, seed=11)
    a = ctx.render(p8)
    samples = ctx.stats()["samples"]
    maps = ctx.probe_depth(_points(21, 2), **kw)
    assert ctx.stats()["samples"] == samples
    assert _same_bits(a, ctx.render(p8))
    with ctx.accumulator(A.make_params(64, 64, 1, seed=11)) as acc:
        acc.render(8)
        assert _same_bits(ctx.probe_depth(_points(21, 2), **kw), maps)
        acc.render(16)
        got = acc.resolve()
    assert _same_bits(got, ctx.render(A.make_params(64, 64, 16, seed=11, spp_chunks=1)))


# ---- the visible lookup ----

@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_lookup_kernel_equals_the_host_form(ctx, case):
    import torch
    name, grid, host, probes, depth, bias, pts, nrm = case
    want = N.probe_lookup_visible_host(grid, probes, depth, pts, nrm, normal_bias=bias)
    assert _same_bits(want, _reference(case))
    assert _same_bits(ctx.probe_lookup_visible(grid, probes, depth, pts, nrm, normal_bias=bias), want), name
    # the device form, with a bad query in the middle: valid 0 for it, the others unchanged
    q = N.gather_points(pts, nrm)
    q = np.concatenate([q, q[:1], q])
    q["n"][len(pts)] = 0.0
    d_probes = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    d_depth = torch.from_numpy(depth.reshape(-1).view(np.uint8).copy()).cuda()
    d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    d_out = torch.full(((len(q) + 1) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vp = N.probe_visible_params(depth.shape[1], bias)
    ctx.probe_lookup_visible_into(grid, d_probes.data_ptr(), d_depth.data_ptr(), vp, d_q.data_ptr(), d_out.data_ptr(), len(q),
                                  blocking=True)
    raw = d_out.cpu().numpy()
    dev = raw[:len(q) * 32].view(A.GATHER_OUT_DTYPE)
    assert (raw[len(q) * 32:] == 0xA5).all()
    assert _same_bits(dev[:len(pts)], want) and _same_bits(dev[len(pts) + 1:], want), name
    assert _same_bits(dev[len(pts)], np.zeros(1, dtype=A.GATHER_OUT_DTYPE)[0])
    with pytest.raises(rtr.RtrError) as e:
        ctx.probe_lookup_visible(grid, probes, depth, q, normal_bias=bias)
    assert e.value.code == A.RTR_ERR_INVALID and "index %d" % len(pts) in e.value.message


def test_lookup_needs_no_scene_and_checks_its_arguments():
    case = CASES[0]
    name, grid, host, probes, depth, bias, pts, nrm = case
    with rtr.Context(0) as c:
        assert _same_bits(c.probe_lookup_visible(grid, probes, depth, pts, nrm, normal_bias=bias), _reference(case))
        L = c._L
        out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
        q = N.gather_points(pts[:1], nrm[:1])
        flat = depth.reshape(-1)
        vp = N.probe_visible_params(depth.shape[1], bias)
        good = [C.byref(grid), probes.ctypes.data, flat.ctypes.data, C.byref(vp), q.ctypes.data, out.ctypes.data]
        for k in range(6):
            args = [None if i == k else a for i, a in enumerate(good)]
            assert L.rtr_probe_lookup_visible(c._h, *args, 1) == A.RTR_ERR_INVALID, k
            assert L.rtr_probe_lookup_visible_device(c._h, *args, 1, 1) == A.RTR_ERR_INVALID, k
        assert L.rtr_probe_lookup_visible(c._h, *good, -1) == A.RTR_ERR_INVALID
        assert L.rtr_probe_lookup_visible(c._h, good[0], None, None, good[3], None, None, 0) == A.RTR_OK  # n == 0: nothing read
        assert L.rtr_probe_lookup_visible_device(c._h, good[0], None, None, good[3], None, None, 0, 1) == A.RTR_OK
        for bad in (dict(map_size=0), dict(map_size=65), dict(pad=1), dict(normal_bias=-1.0), dict(normal_bias=np.nan)):
            vb = N.probe_visible_params(depth.shape[1], bias)
            for k, v in bad.items():
                setattr(vb, k, v)
            args = good[:3] + [C.byref(vb)] + good[4:]
            assert L.rtr_probe_lookup_visible(c._h, *args, 1) == A.RTR_ERR_INVALID, bad
            assert L.rtr_probe_lookup_visible_device(c._h, *args, 1, 1) == A.RTR_ERR_INVALID, bad
        misaligned = [good[0], probes.ctypes.data + 4] + good[2:]
        assert L.rtr_probe_lookup_visible_device(c._h, *misaligned, 1, 1) == A.RTR_ERR_INVALID
        assert not out.view(np.uint8).any()


# ---- two rooms ----

def _flipped(b, rect):
    return b.flip_face(rect)


def _two_rooms():
    """Two rooms of 2 x 2 x 2 side by side along x, every wall facing into its room: room A (x in 0 .. 2) with a quad light
    under its ceiling, room B (x in 2 .. 4) dark, a wall of two sheets between them at x = 1.99 and 2.01; and in room B a
    solid box (sides facing out) for a probe to stand in."""
    b = R.Builder(np.random.default_rng(0))
    base = G.scene(23)
    white = b.material(A.MAT_LAMBERTIAN, [b.solid([0.7, 0.7, 0.7])])
    emit = b.material(A.MAT_DIFFUSE_LIGHT, [b.solid([9.0, 9.0, 9.0])])
    top = []
    for x0, x1 in ((0.0, 1.99), (2.01, 4.0)):
        top += [b.rect("yz", 0.0, 2.0, 0.0, 2.0, x0, white), _flipped(b, b.rect("yz", 0.0, 2.0, 0.0, 2.0, x1, white)),
                b.rect("xz", x0, x1, 0.0, 2.0, 0.0, white), _flipped(b, b.rect("xz", x0, x1, 0.0, 2.0, 2.0, white)),
                b.rect("xy", x0, x1, 0.0, 2.0, 0.0, white), _flipped(b, b.rect("xy", x0, x1, 0.0, 2.0, 2.0, white))]
    top.append(_flipped(b, b.rect("xz", 0.5, 1.5, 0.5, 1.5, 1.98, emit)))
    b.quad_light([0.5, 1.98, 0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [9.0, 9.0, 9.0])
    p0, p1 = (3.2, 0.01, 0.2), (3.8, 0.6, 0.8)
    top += [b.rect("xy", p0[0], p1[0], p0[1], p1[1], p1[2], white), _flipped(b, b.rect("xy", p0[0], p1[0], p0[1], p1[1], p0[2], white)),
            b.rect("xz", p0[0], p1[0], p0[2], p1[2], p1[1], white), _flipped(b, b.rect("xz", p0[0], p1[0], p0[2], p1[2], p0[1], white)),
            b.rect("yz", p0[1], p1[1], p0[2], p1[2], p1[0], white), _flipped(b, b.rect("yz", p0[1], p1[1], p0[2], p1[2], p0[0], white))]
    return rtr.Scene(b.hlist(top), R._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), R._cat(b.mats, A.MATERIAL_DTYPE),
                     R._cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], base.images[:0], base.image_bytes[:0],
                     R._cat(b.lights, A.LIGHT_DTYPE), base.camera.copy(), np.array([0.0, 0.0, 0.0]))


def test_two_rooms(ctx):
    """A 2 x 1 x 1 grid straddling the wall, half a spacing from it on either side.  In the dark room, a quarter spacing
    and more behind the wall, the plain lookup still takes up to a quarter of its light from the probe in the lit room.  The
    visibility is tested at pb = p + normal_bias * w, not at p, so it is pb that has to stand a quarter spacing behind the
    wall: a query whose normal faces the wall is moved back by the bias (0.25, a quarter of the smallest spacing)."""
    ctx.upload(_two_rooms())
    prm = A.make_params(64, 64, 1, integrator=4)
    grid = rtr.ProbeGrid((1.25, 1.0, 1.0), (1.5, 1.0, 1.0), (2, 1, 1))
    grid.bake(ctx, prm, samples=64, seed=SEED, depth=8)
    _note(ctx, 8)
    assert grid.depth.shape == (2, 8, 8) and (grid.depth["valid"] == 1).all()
    t_max = 1.5 * float(np.sqrt(1.5 * 1.5 + 1.0 + 1.0))
    want, _ = _want(ctx, grid.positions(), map_size=8, samples=8, seed=SEED, t_max=t_max)
    assert _same_bits(grid.depth, want)
    assert (grid.depth["hits"] == 8).all() and (grid.depth["back"] == 0).all()  # closed rooms whose walls face inwards
    assert (grid.coefficients["c"][0, 0] > 0).all() and not grid.coefficients["c"][1].any()  # no light crosses the wall
    normals = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.3, 1.0]])
    pts, nrm = [], []
    for n in normals:
        back = max(0.0, -0.25 * n[0] / np.sqrt(n @ n))  # what the bias takes off the distance to the wall
        xs = np.linspace(2.375 + back, 2.72, 4)  # a quarter spacing and more behind the wall, short of the dark probe at 2.75
        pts += [(x, y, z) for x in xs for y in (0.6, 1.0, 1.5) for z in (0.7, 1.2)]
        nrm += [n] * 24
    pts, nrm = np.array(pts), np.array(nrm)
    plain = grid.irradiance(pts, nrm, visible=False)
    vis = grid.irradiance(pts, nrm)  # maps were baked: visible by default
    assert _same_bits(vis, grid.irradiance(pts, nrm, visible=True))
    ref = DR.lookup_visible(grid.origin, grid.spacing, grid.dims, grid.coefficients, grid.depth, 0.25, pts, nrm)
    assert (ref["valid"] == 1).all() and _same_bits(vis, ref["v"])
    assert _same_bits(plain, PR.lookup(grid.origin, grid.spacing, grid.dims, grid.coefficients, pts, nrm)["v"])
    assert (plain > 0).all()  # these normals see the lit probe's light: the leak is there to be cut
    ratio = (vis / plain)[:, 0].reshape(len(normals), 4, -1)
    for k, n in enumerate(normals):
        print("two rooms: normal %s, visible / plain from the nearest x to the farthest: %s" %
              (n.tolist(), ["%.2e" % r for r in ratio[k].max(axis=1)]))
    print("two rooms: light leaked into the dark room, visible / plain: at most %.3e, median %.3e" % (ratio.max(), np.median(ratio)))
    assert (vis < plain).all()
    assert _same_bits(grid.irradiance(pts, nrm, normal_bias=0.1),
                      DR.lookup_visible(grid.origin, grid.spacing, grid.dims, grid.coefficients, grid.depth, 0.1, pts, nrm)["v"])
    # without maps the grid is what it was
    plain_grid = rtr.ProbeGrid((1.25, 1.0, 1.0), (1.5, 1.0, 1.0), (2, 1, 1)).bake(ctx, prm, samples=64, seed=SEED)
    assert plain_grid.depth is None and _same_bits(plain_grid.coefficients, grid.coefficients)
    assert _same_bits(plain_grid.irradiance(pts, nrm), plain)
    with pytest.raises(ValueError):
        plain_grid.irradiance(pts, nrm, visible=True)


def test_classify_drops_the_probe_inside_a_box(ctx):
    ctx.upload(_two_rooms())
    prm = A.make_params(64, 64, 1, integrator=4)
    grid = rtr.ProbeGrid((1.0, 0.3, 0.5), (1.25, 1.0, 1.0), (3, 1, 1))  # x = 1.0 (room A), 2.25 (room B), 3.5 (inside the box)
    grid.bake(ctx, prm, samples=16, seed=SEED, depth=8, max_distance=3.0)
    assert (grid.coefficients["valid"] == 1).all()
    _, maps, _ = _case(ctx, grid.positions(), map_size=8, samples=8, seed=SEED, t_max=3.0)
    assert _same_bits(maps, grid.depth)
    hits, back = grid.depth["hits"].reshape(3, -1).sum(axis=1), grid.depth["back"].reshape(3, -1).sum(axis=1)
    assert back[0] == 0 and back[1] == 0 and back[2] == hits[2] == 8 * 64
    assert grid.classify().tolist() == [False, False, True]
    assert grid.coefficients["valid"].tolist() == [1, 1, 0]
    again = rtr.ProbeGrid((1.0, 0.3, 0.5), (1.25, 1.0, 1.0), (3, 1, 1)).bake(ctx, prm, samples=16, seed=SEED, depth=8,
                                                                             max_distance=3.0, classify=True)
    assert _same_bits(again.coefficients, grid.coefficients) and _same_bits(again.depth, grid.depth)
    q, n = np.array([[3.4, 0.3, 0.5]]), np.array([[0.0, 1.0, 0.0]])  # next to the dropped probe: one corner left
    out = ctx.probe_lookup_visible(grid.grid(), grid.coefficients, grid.depth, q, n, normal_bias=0.25)
    assert out["count"][0] == 1 and out["valid"][0] == 1


def test_cli_depth_maps_equal_the_python_route(ctx, tmp_path):
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    box = "100,400,100,450,500,450"
    common = [cli, "21", "4", "--probes", "3,2,2", "--probe-box", box, "--probe-samples", "16", "--seed", "7"]
    plain = subprocess.run(common, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert plain.returncode == 0, plain.stderr.decode()
    out = str(tmp_path / "depth.bin")
    r = subprocess.run(common + ["--probe-depth", "8", "--probe-depth-samples", "4", "--probe-depth-out", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == plain.stdout  # the coefficients are printed as they always were
    ctx.upload(rtr.hostscene.build_scene(21))
    grid = rtr.ProbeGrid.in_box((100.0, 400.0, 100.0), (450.0, 500.0, 450.0), (3, 2, 2))
    grid.bake(ctx, A.make_params(64, 64, 1, integrator=4), samples=16, seed=7, depth=8, depth_samples=4)
    assert open(out, "rb").read() == grid.depth.tobytes()
    assert (grid.depth["hits"] > 0).any() and (grid.depth["valid"] == 1).all()
    for args in (["--probe-depth", "8"], ["--probe-depth-out", out], ["--probe-depth", "0", "--probe-depth-out", out],
                 ["--probe-depth", "65", "--probe-depth-out", out], ["--probe-depth-samples", "4"],
                 ["--probe-depth", "8", "--probe-depth-samples", "0", "--probe-depth-out", out]):
        r = subprocess.run(common + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, args
    r = subprocess.run([cli, "21", "4", "--probe-depth", "8", "--probe-depth-out", out], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 2  # maps belong to a probe grid


def test_every_depth_kernel_ran_and_was_compared():
    """The union of what the tests above launched is the whole of DEPTH_TABLE: every k_probe_depth<T> of
    csrc/rtr_probe_depth.hip ran under a test that compares its output."""
    missing = sorted(TRAV_NAME[t] for t in DEPTH_TABLE - SEEN)
    extra = sorted(TRAV_NAME[t] for t in SEEN - DEPTH_TABLE)
    print("depth kernels: %d / %d" % (len(SEEN & DEPTH_TABLE), len(DEPTH_TABLE)))
    assert not missing and not extra, "depth kernels not launched: %s; launched but not in the table: %s" % (missing, extra)
