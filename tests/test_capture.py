"""Environment captures (include/rtr_hip.h: rtr_capture_cube, its device-pointer form, rtr_cube_lookup) on the GPU.  The
radiance is held bit for bit to the contract's own reference: the restatement's reduction (tests/_capture_ref.py) of
rtr_li_rays over the rays and states of rtr_capture_ray, under the same render params, flags included.  The orientation
of the faces is checked without the restatement, through rtr_query_closest.  Batch shapes, bad centres, the device entry
behind a queued accumulator pass, a slice boundary inside a capture and the command-line tool follow.

csrc/rtr_capture.hip holds 17 k_capture_li<integrator, traversal> (CAPTURE_TABLE below restates its list, the k_li family
rule of csrc/rt_select.h); which one a call launched the context records on the host (Context.last_capture).  The last
test asserts that the tests of this module launched, and compared, every one of them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _capture_ref as CR
import _gather_ref as GR
import _golden as G
import _probe_ref as PR
import _randscene as R
from test_capture_cpu import lookup_cases

rtr = G.rtr
A = G.A

pytestmark = pytest.mark.gpu

SEED = 7
# scenes 21 and 9 are Cornell boxes of side 555, scene 23 is of unit scale: centres in free space next to surfaces
DISPLACE = {21: 5.0, 9: 5.0, 23: 0.05}
INSIDE_21 = np.array([[278.0, 400.0, 400.0]])  # above the two boxes of the Cornell box, towards its back wall

# RT_TRAV_* of csrc/rt_device.h
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)
TRAV_NAME = ["EXACT", "MEDIA", "FAST", "PROGRAM", "FLAT", "TOP", "PROGRAM_EXT", "FLAT_GUARD"]
TRAVS_LI = (FAST, PROGRAM_EXT, MEDIA, EXACT)
TRAVS_N1 = (FAST, PROGRAM_EXT, MEDIA)
CAPTURE_TABLE = {(i, t) for i in (4, 1) for t in TRAVS_LI} | {(i, t) for i in (0, 2, 3) for t in TRAVS_N1}
assert len(CAPTURE_TABLE) == 17
SEEN = set()  # what the tests of this module launched and compared


def capture_name(g):
    return "k_capture_li<%d, %s>" % (g[0], TRAV_NAME[g[1]])


def _note(ctx, samples, integrator):
    g = ctx.last_capture()
    assert g is not None and g["integ"] == integrator
    assert 1 << g["lg"] == GR.group_size(samples), (samples, g)
    SEEN.add((g["integ"], g["trav"]))
    return g["integ"], g["trav"]


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _centres(sid, n):
    return PR.displaced_points(sid, DISPLACE[sid], n)


_WANT = {}


def _reference(ctx, sid, integrator, S, N, order, n, jitter=1, base=0):
    """The capture the contract defines, [n, 6, S, S, 3]: rtr_li_rays over the rays of rtr_capture_ray, reduced by the
    restatement.  The scene must be uploaded.  Computed once per case."""
    key = (sid, integrator, S, N, order, n, jitter, base)
    if key not in _WANT:
        prm = A.make_params(64, 64, 1, integrator=integrator, flags=A.FLAG_REFERENCE_ORDER if order else 0)
        rays = ctx.capture_rays(_centres(sid, n), face_size=S, samples=N, seed=SEED, time=0.25, jitter=jitter, point_base=base)
        d, st = CR.rays(n, S, N, SEED, base, jitter)  # the host form is the restatement's: tests/test_capture_cpu.py
        assert np.array_equal(_bits(rays["direction"]), _bits(d)) and np.array_equal(rays["rng_state"], st)
        flat = rays.reshape(-1)
        L = ctx.li_rays(prm, flat["origin"], flat["direction"], flat["time"], flat["rng_state"])
        _WANT[key] = CR.reduce(L.reshape(n, 6, S, S, N, 3))
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _case(ctx, sid, integrator, S, N, order=False, n=2, jitter=1):
    ctx.upload(G.scene(sid))
    want = _reference(ctx, sid, integrator, S, N, order, n, jitter)
    prm = A.make_params(64, 64, 1, integrator=integrator, flags=A.FLAG_REFERENCE_ORDER if order else 0)
    out = ctx.capture_cube_records(prm, _centres(sid, n), face_size=S, samples=N, seed=SEED, time=0.25, jitter=jitter)
    name = _note(ctx, N, integrator)
    assert out.shape == (n, 6, S, S)
    assert np.array_equal(_bits(out["v"]), _bits(want)), (sid, integrator, S, N, order)
    assert (out["count"] == N).all() and (out["valid"] == 1).all()
    return name, out


# G = 1; a group with idle lanes on a last wave that is partly past the end (54 texels on 432 lanes); a full wave; several
# samples per lane
SHAPES = ((1, 1), (3, 5), (4, 64), (1, 130), (3, 130))


@pytest.mark.parametrize("S,N", SHAPES)
@pytest.mark.parametrize("order", (False, True))
@pytest.mark.parametrize("integrator", (4, 1))
def test_scene_21_mis_and_rr_in_both_orders(ctx, integrator, order, S, N):
    name, out = _case(ctx, 21, integrator, S, N, order, n=3 if S == 1 else 2)
    assert name == (integrator, EXACT if order else FAST)
    if N >= 64:
        assert (out["v"] >= 0).all() and (out["v"] > 0).any()
    if order:  # the reference-order walk gives this scene's bits
        assert _same_bits(out, _case(ctx, 21, integrator, S, N, False, n=3 if S == 1 else 2)[1])


@pytest.mark.parametrize("S,N", ((3, 5), (4, 64)))
@pytest.mark.parametrize("sid,integrator", ((21, 0), (21, 2), (21, 3), (23, 4), (23, 1)))
def test_other_integrators_and_scene_23(ctx, sid, integrator, S, N):
    assert _case(ctx, sid, integrator, S, N)[0] == (integrator, FAST)


@pytest.mark.parametrize("order", (False, True))
@pytest.mark.parametrize("integrator", range(5))
def test_media(ctx, integrator, order):
    """Scene 9 (smoke boxes): the general program kernel, and with FLAG_REFERENCE_ORDER the media walk, which integrators 0,
    2 and 3 also take for the reference order of scenes without media (csrc/rt_select.h: li_trav)."""
    assert _case(ctx, 9, integrator, 3, 5, order)[0] == (integrator, MEDIA if order else PROGRAM_EXT)


@pytest.mark.parametrize("integrator", (0, 2, 3))
def test_reference_order_without_media_takes_the_media_kernel(ctx, integrator):
    name, out = _case(ctx, 21, integrator, 3, 5, True)
    assert name == (integrator, MEDIA)
    assert _same_bits(out, _case(ctx, 21, integrator, 3, 5, False)[1])


def test_without_jitter(ctx):
    name, out = _case(ctx, 21, 4, 4, 5, jitter=0)
    assert name == (4, FAST)
    assert not _same_bits(out, _case(ctx, 21, 4, 4, 5, jitter=1)[1])


def test_face_orientation_through_closest_hits(ctx):
    """Independent of the restatement: from a centre inside the Cornell box, the hit point of every texel's ray (jitter 0)
    lies on the side of the centre the ray's face index names: the axis of largest |hit - centre|, x before y before z, and
    its sign."""
    ctx.upload(G.scene(21))
    S = 4
    rays = ctx.capture_rays(INSIDE_21, face_size=S, samples=1, jitter=0)[0, ..., 0]  # [6, S, S]
    hits = ctx.query_closest(rays.reshape(-1)).reshape(6, S, S)
    assert (hits["hit"] == 1).sum() >= 5 * S * S  # the box is open towards -z only
    rel = hits["p"] - INSIDE_21[0]
    mag = np.abs(rel)
    axis = np.where((mag[..., 0] >= mag[..., 1]) & (mag[..., 0] >= mag[..., 2]), 0, np.where(mag[..., 1] >= mag[..., 2], 1, 2))
    sign = np.take_along_axis(rel, axis[..., None], -1)[..., 0]
    face = 2 * axis + (sign < 0)
    want = np.broadcast_to(np.arange(6)[:, None, None], face.shape)
    hit = hits["hit"] == 1
    assert np.array_equal(face[hit], want[hit])
    for f in range(5):  # and inside a face: columns run along +u, rows along +v of the header's table
        assert hit[f].all(), f
    p = rel / np.take_along_axis(mag, axis[..., None], -1)  # back onto the cube: the hit distance drops out
    assert (np.diff(p[0][..., 2], axis=1) < 0).all() and (np.diff(p[0][..., 1], axis=0) < 0).all()   # +x: u = -z, v = -y
    assert (np.diff(p[1][..., 2], axis=1) > 0).all() and (np.diff(p[1][..., 1], axis=0) < 0).all()   # -x: u = +z, v = -y
    assert (np.diff(p[2][..., 0], axis=1) > 0).all() and (np.diff(p[2][..., 2], axis=0) > 0).all()   # +y: u = +x, v = +z
    assert (np.diff(p[3][..., 0], axis=1) > 0).all() and (np.diff(p[3][..., 2], axis=0) < 0).all()   # -y: u = +x, v = -z
    assert (np.diff(p[4][..., 0], axis=1) > 0).all() and (np.diff(p[4][..., 1], axis=0) < 0).all()   # +z: u = +x, v = -y
    # and the capture's texels are the radiance of exactly these rays
    prm = A.make_params(64, 64, 1)
    out = ctx.capture_cube_records(prm, INSIDE_21, face_size=S, samples=1, jitter=0)
    flat = ctx.capture_rays(INSIDE_21, face_size=S, samples=1, jitter=0).reshape(-1)
    L = ctx.li_rays(prm, flat["origin"], flat["direction"], flat["time"], flat["rng_state"])
    assert np.array_equal(_bits(out["v"].reshape(-1, 3)), _bits(L))


def _sky_scene():
    """A uniform background and one unit sphere a million units down the -y axis, where no texel of an even face looks"""
    b = R.Builder(np.random.default_rng(0))
    base = G.scene(23)
    far = b.sphere([0.0, -1e6, 0.0], 1.0, b.material(A.MAT_LAMBERTIAN, [b.solid([0.5, 0.5, 0.5])]))
    return rtr.Scene(b.hlist([far]), R._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), R._cat(b.mats, A.MATERIAL_DTYPE),
                     R._cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], base.images[:0], base.image_bytes[:0],
                     R._cat(b.lights, A.LIGHT_DTYPE), base.camera.copy(), np.array([0.3, 0.625, 1.75]))


@pytest.mark.parametrize("integrator", range(5))
def test_uniform_sky(ctx, integrator):
    """Nothing in reach: every ray returns the background, and with N a power of two the mean is exact"""
    ctx.upload(_sky_scene())
    prm = A.make_params(64, 64, 1, integrator=integrator)
    for S, N, jitter in ((2, 1, 0), (4, 8, 1), (2, 128, 1)):
        v, valid = ctx.capture_cube(prm, np.array([[0.0, 0.0, 0.0], [3.0, -2.0, 1.0]]), face_size=S, samples=N, seed=SEED, jitter=jitter)
        assert v.shape == (2, 6, S, S, 3) and valid.shape == (2, 6, S, S) and valid.all()
        assert np.array_equal(_bits(v), _bits(np.broadcast_to(np.array([0.3, 0.625, 1.75]), v.shape))), (integrator, S, N)


def test_sharding_by_point_base(ctx):
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1)
    pts = _centres(21, 5)
    kw = dict(face_size=3, samples=5, seed=SEED)
    whole = ctx.capture_cube_records(prm, pts, **kw)
    for cut in (1, 2, 4):
        split = np.concatenate([ctx.capture_cube_records(prm, pts[:cut], **kw),
                                ctx.capture_cube_records(prm, pts[cut:], point_base=cut, **kw)])
        assert _same_bits(split, whole), cut
    assert not _same_bits(ctx.capture_cube_records(prm, pts[2:], **kw), whole[2:])  # (the base matters)
    wrap = ctx.capture_cube_records(prm, pts[[1, 0]], point_base=0xFFFFFFFF, **kw)  # k is taken modulo 2^32
    assert _same_bits(wrap[1], whole[0]) and not _same_bits(wrap[0], whole[1])
    assert ctx.capture_cube_records(prm, pts[:0], **kw).shape == (0, 6, 3, 3)


def test_device_entry_behind_an_accumulator_pass_bad_centres_and_alignment(ctx):
    import torch
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1, integrator=1)
    S, N, n = 3, 5, 4
    rec = 6 * S * S
    pts = rtr.native.probe_points(_centres(21, n))
    host = ctx.capture_cube_records(prm, pts, face_size=S, samples=N, seed=SEED)
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    d_out = torch.full(((n * rec + 1) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    ap = A.make_params(128, 128, 1, seed=11)
    want_img = ctx.render(A.make_params(128, 128, 8, seed=11, spp_chunks=1))
    torch.cuda.synchronize()
    with ctx.accumulator(ap) as acc:
        acc.render(8, blocking=False)
        ctx.capture_cube_into(prm, d_pts.data_ptr(), d_out.data_ptr(), n, face_size=S, samples=N, seed=SEED, blocking=False)
        ctx.synchronize()
        raw = d_out.cpu().numpy()
        assert _same_bits(raw[:n * rec * 32].view(A.GATHER_OUT_DTYPE).reshape(n, 6, S, S), host)
        assert (raw[n * rec * 32:] == 0xA5).all()  # nothing behind the batch is written
        assert np.array_equal(_bits(acc.resolve()), _bits(want_img))  # and the pass is the pass
    # bad centres: zero records with valid 0 for their texels, the neighbours untouched by them
    bad = pts.copy()
    bad["p"][1, 0] = np.nan
    bad["p"][2, 2] = -np.inf
    d_bad = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    for m in (0, 1, 2, 3, 4):
        d_out.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.capture_cube_into(prm, d_bad.data_ptr(), d_out.data_ptr(), m, face_size=S, samples=N, seed=SEED, blocking=True)
        raw = d_out.cpu().numpy()
        got = raw[:m * rec * 32].view(A.GATHER_OUT_DTYPE).reshape(m, 6, S, S)
        assert (raw[m * rec * 32:] == 0xA5).all(), m
        for k in range(m):
            assert _same_bits(got[k], np.zeros((6, S, S), dtype=A.GATHER_OUT_DTYPE) if k in (1, 2) else host[k]), (m, k)
    assert _same_bits(d_bad.cpu().numpy(), bad.view(np.uint8))  # the input is not written
    with pytest.raises(rtr.RtrError) as e:
        ctx.capture_cube_into(prm, d_pts.data_ptr() + 4, d_out.data_ptr(), 1, face_size=S, samples=N, blocking=True)
    assert e.value.code == A.RTR_ERR_INVALID and "aligned" in e.value.message
    with pytest.raises(rtr.RtrError):
        ctx.capture_cube_into(prm, d_pts.data_ptr(), d_out.data_ptr() + 4, 1, face_size=S, samples=N, blocking=True)


def test_host_entry_rejects_bad_centres_and_leaves_the_output(ctx):
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1)
    pts = rtr.native.probe_points(_centres(21, 4))
    for k, a, value in ((2, 1, np.nan), (0, 2, -np.inf), (3, 0, np.inf)):
        bad = pts.copy()
        bad["p"][k, a] = value
        out = np.zeros((4, 6, 2, 2), dtype=A.GATHER_OUT_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        with pytest.raises(rtr.RtrError) as e:
            ctx.capture_cube_records(prm, bad, face_size=2, samples=3, out=out)
        assert e.value.code == A.RTR_ERR_INVALID and "index %d" % k in e.value.message, k
        assert (out.view(np.uint8) == 0xA5).all()


def test_a_slice_boundary_inside_a_capture_leaves_no_seam(ctx):
    """One centre, S = 512: 1 572 864 texels, so the host entry's second slice (2^20 texels each) starts inside face 4.  The
    device entry serves the same capture in one launch."""
    import torch
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1)
    S = 512
    host = ctx.capture_cube_records(prm, INSIDE_21, face_size=S, samples=1, seed=SEED)
    d_pts = torch.from_numpy(rtr.native.probe_points(INSIDE_21).view(np.uint8).copy()).cuda()
    d_out = torch.zeros(6 * S * S * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.capture_cube_into(prm, d_pts.data_ptr(), d_out.data_ptr(), 1, face_size=S, samples=1, seed=SEED, blocking=True)
    dev = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE).reshape(1, 6, S, S)
    assert (host["valid"] == 1).all() and _same_bits(host, dev)
    flat = host.reshape(-1)
    around = slice((1 << 20) - 64, (1 << 20) + 64)  # the texels on both sides of the boundary against rtr_li_rays
    e = np.arange(6 * S * S)[around]
    rays = np.concatenate([rtr.native.capture_ray(INSIDE_21[0], t // (S * S), t % S, t // S % S, face_size=S, samples=1, seed=SEED)
                           for t in e])
    L = ctx.li_rays(prm, rays["origin"], rays["direction"], rays["time"], rays["rng_state"])
    assert np.array_equal(_bits(flat["v"][around]), _bits(L))


@pytest.mark.parametrize("case", lookup_cases(), ids=lambda c: c[0])
def test_lookup_on_the_device_equals_the_host_form(ctx, case):
    import torch
    name, texels, dirs = case
    S = texels.shape[1]
    want = rtr.native.cube_lookup_host(texels, dirs)
    assert _same_bits(ctx.cube_lookup(texels, dirs), want), name
    q = rtr.native.probe_points(dirs)
    d_t = torch.from_numpy(texels.reshape(-1).view(np.uint8).copy()).cuda()
    d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    d_out = torch.full(((len(q) + 1) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.cube_lookup_into(S, d_t.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True)
    raw = d_out.cpu().numpy()
    assert _same_bits(raw[:len(q) * 32].view(A.GATHER_OUT_DTYPE), want), name
    assert (raw[len(q) * 32:] == 0xA5).all()


def test_lookup_entries_check_their_arguments(ctx):
    t = np.zeros(24, dtype=A.GATHER_OUT_DTYPE)
    q = rtr.native.probe_points(np.ones((2, 3)))
    out = np.zeros(2, dtype=A.GATHER_OUT_DTYPE)
    with rtr.Context(0) as c:  # no scene is needed
        L = c._L
        assert L.rtr_cube_lookup(c._h, 2, t.ctypes.data, q.ctypes.data, out.ctypes.data, 2) == A.RTR_OK
        assert L.rtr_cube_lookup(c._h, 2, None, None, None, 0) == A.RTR_OK
        for args in ((0, t.ctypes.data, q.ctypes.data, out.ctypes.data, 2), (4097, t.ctypes.data, q.ctypes.data, out.ctypes.data, 2),
                     (2, None, q.ctypes.data, out.ctypes.data, 2), (2, t.ctypes.data, None, out.ctypes.data, 2),
                     (2, t.ctypes.data, q.ctypes.data, None, 2), (2, t.ctypes.data, q.ctypes.data, out.ctypes.data, -1)):
            assert L.rtr_cube_lookup(c._h, *args) == A.RTR_ERR_INVALID, args
            assert L.rtr_cube_lookup_device(c._h, *args, 1) == A.RTR_ERR_INVALID, args
        assert L.rtr_cube_lookup_device(c._h, 2, t.ctypes.data + 4, q.ctypes.data, out.ctypes.data, 1, 1) == A.RTR_ERR_INVALID


def test_before_upload_and_params():
    pts = rtr.native.probe_points(_centres(21, 2))
    out = np.zeros(2 * 24, dtype=A.GATHER_OUT_DTYPE)
    prm = A.make_params(64, 64, 1)
    with rtr.Context(0) as c:
        L = c._L

        def calls(cp, rp=prm, pts_ptr=pts.ctypes.data, out_ptr=out.ctypes.data, m=2):
            r = C.byref(rp) if rp is not None else None
            return (L.rtr_capture_cube(c._h, r, C.byref(cp), pts_ptr, out_ptr, m),
                    L.rtr_capture_cube_device(c._h, r, C.byref(cp), pts_ptr, out_ptr, m, 1))

        ok = rtr.native.capture_defaults(face_size=2, samples=3)
        assert calls(ok) == (A.RTR_ERR_NO_SCENE,) * 2
        c.upload(G.scene(21))
        invalid = (A.RTR_ERR_INVALID,) * 2
        for kw in (dict(face_size=0), dict(face_size=-3), dict(face_size=4097), dict(samples=0), dict(samples=(1 << 20) + 1),
                   dict(jitter=2), dict(jitter=-1), dict(time=np.nan), dict(time=np.inf)):
            assert calls(rtr.native.capture_defaults(**dict(dict(face_size=2, samples=3), **kw))) == invalid, kw
        for k in range(3):
            cp = rtr.native.capture_defaults(face_size=2, samples=3)
            if k == 2:
                cp.pad = 1
            else:
                cp.reserved[k] = 1.0
            assert calls(cp) == invalid
        assert calls(ok, m=-1) == invalid and calls(ok, pts_ptr=None) == invalid and calls(ok, out_ptr=None) == invalid
        assert calls(ok, rp=None) == invalid
        assert calls(ok, rp=A.make_params(64, 64, 1, integrator=9)) == (A.RTR_ERR_UNSUPPORTED,) * 2  # as for a gather
        assert L.rtr_capture_cube(c._h, C.byref(prm), None, pts.ctypes.data, out.ctypes.data, 2) == A.RTR_ERR_INVALID
        assert not out.view(np.uint8).any()  # nothing ran
        assert calls(ok, pts_ptr=None, out_ptr=None, m=0) == (A.RTR_OK,) * 2  # n == 0: no launch, nothing read
        assert c.last_capture() is None  # none of this launched anything


def test_captures_leave_renders_and_statistics_alone(ctx):
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1)
    p8 = A.make_params(64, 64, 8, seed=11)
    a = ctx.render(p8)
    samples = ctx.stats()["samples"]
    cube = ctx.capture_cube_records(prm, _centres(21, 2), face_size=3, samples=5, seed=SEED)
    assert ctx.stats()["samples"] == samples
    assert np.array_equal(_bits(a), _bits(ctx.render(p8)))
    assert _same_bits(cube, ctx.capture_cube_records(prm, _centres(21, 2), face_size=3, samples=5, seed=SEED))


def test_renderer_capture_environment_and_the_command_line(ctx, tmp_path):
    """rtr_cli --capture writes the bytes Cubemap.save_hdr writes for the same capture"""
    cli = os.path.join(os.path.dirname(rtr.native.library_path()), "rtr_cli")
    out = str(tmp_path / "cli.hdr")
    r = subprocess.run([cli, "21", "4", "--capture", "278,400,400", "--face", "8", "--capture-spp", "4", "--seed", "7",
                        "--capture-out", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    sc = rtr.hostscene.build_scene(21)
    ren = rtr.Renderer(context=ctx)
    ren.seed = 7
    cube = ren.capture_environment(sc, (278.0, 400.0, 400.0), face_size=8, samples=4)
    ctx.upload(sc)
    rec = ctx.capture_cube_records(A.make_params(64, 64, 1, integrator=4), INSIDE_21, face_size=8, samples=4, seed=7)
    assert _same_bits(cube.texels, rec[0]) and (cube.radiance > 0).any()
    mine = str(tmp_path / "py.hdr")
    cube.save_hdr(mine, 32, 16)
    assert open(out, "rb").read() == open(mine, "rb").read()
    assert np.array_equal(_bits(cube.lookup(np.eye(3), ctx=ctx)), _bits(cube.lookup(np.eye(3))))
    sized = str(tmp_path / "sized.hdr")
    r = subprocess.run([cli, "21", "4", "--capture", "278,400,400", "--face", "8", "--capture-spp", "4", "--seed", "7",
                        "--capture-out", sized, "--latlong", "20,10"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    cube.save_hdr(mine, 20, 10)
    assert open(sized, "rb").read() == open(mine, "rb").read()
    for args in (["--capture", "1,2,3"], ["--capture-out", out], ["--face", "8"], ["--capture", "1,2", "--capture-out", out],
                 ["--capture", "1,2,3", "--capture-out", out, "--face", "0"],
                 ["--capture", "1,2,3", "--capture-out", out, "--latlong", "0,4"],
                 ["--capture", "1,2,3", "--capture-out", out, "--ao", "8"]):
        r = subprocess.run([cli, "21", "4"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, args


def test_every_capture_kernel_ran_and_was_compared():
    """The union of what the tests above launched is the whole of CAPTURE_TABLE: every k_capture_li<I, T> of
    csrc/rtr_capture.hip ran under a test that compares its output."""
    missing = sorted(map(capture_name, CAPTURE_TABLE - SEEN))
    extra = sorted(map(capture_name, SEEN - CAPTURE_TABLE))
    print("capture kernels: %d / %d" % (len(SEEN & CAPTURE_TABLE), len(CAPTURE_TABLE)))
    G.residue("capture_kernels_not_compared", len(missing) + len(extra), 0)
    assert not missing and not extra, "capture kernels not launched: %s; launched but not in the table: %s" % (missing, extra)
