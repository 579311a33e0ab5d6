"""Capture sets (include/rtr_hip.h: rtr_capture_set*) on the GPU: the device and host entries against the host-only _one
forms bit for bit (which tests/test_capture_set_cpu.py holds to numpy), the old behaviour as a special case, the preview
against the host's reduction of its samples, and a bake in stream order closed against the path tracer in a room whose
walls emit six different colours."""
import ctypes as C

import numpy as np
import pytest

import _capture_set_cases as SC
import _capture_set_ref as SR
import _cube_filter_ref as FR
import _golden as G
import _ibl_cases as IC
import _preview_ref as PR
import _randscene as RS

rtr = G.rtr
A = G.A
N = rtr.native

pytestmark = pytest.mark.gpu
INV = A.RTR_ERR_INVALID
REC = 32
FRAME = dict(W=40, H=30, region=(8, 5, 32, 25), grid=2)  # 24 x 20 at (8, 5): ragged against the 16 x 16 blocks


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _sentinel(n_bytes):
    import torch
    return torch.full((n_bytes,), 0xA5, dtype=torch.uint8, device="cuda")


def _records_from(t, n):
    raw = t.cpu().numpy()
    assert (raw[n * REC:] == 0xA5).all()
    return raw[:n * REC].view(A.GATHER_OUT_DTYPE)


def _lookup_into(ctx, cset, levels, d_rec, n_records, q):
    import torch
    d_q, d_out = _dev(q), _sentinel((len(q) + 1) * REC)
    torch.cuda.synchronize()
    ctx.capture_set_lookup_into(cset, levels, d_rec.data_ptr(), n_records, d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True)
    return _records_from(d_out, len(q))


def _shade_into(ctx, ne, cset, q):
    import torch
    d_q, d_out = _dev(q), _sentinel((len(q) + 1) * REC)
    torch.cuda.synchronize()
    ctx.shade_ibl_into(ne, d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True, captures=cset)
    return _records_from(d_out, len(q))


def _device_env(env, parts, count):
    held = {"table": IC.table_records(env["tab"])}
    if parts & 1:
        held["probes"] = env["probes"]
        if env["depth"] is not None:
            held["depth"] = env["depth"]
    if parts & 2:
        held["chain"] = env["records"]
    dev = {name: _dev(a) for name, a in held.items()}
    return SC.native_env(env, parts, count, {name: t.data_ptr() for name, t in dev.items()}), dev


# ---- 1. the entries equal the one form ----

@pytest.mark.parametrize("chain", SC.CHAINS)
@pytest.mark.parametrize("count", SC.COUNTS)
def test_lookup_entries_equal_the_one_form(ctx, monkeypatch, count, chain):
    """n = 300: two workgroups and a ragged tail; the BAD queries among them give zero records; the host entry with the
    slice lowered to 64 takes five slices and keeps the bits"""
    vols = SC.volumes(count)
    levels, rec = SC.records(count, chain)
    q = SC.queries(count, chain[0], 300)
    fallback = count - 1 if chain[0] == 1 else -1
    cset = N.capture_set(vols, fallback)
    want = N.capture_set_lookup_host(cset, levels, rec, q)
    assert want["valid"].any() and not want["valid"].all()
    got = _lookup_into(ctx, cset, levels, _dev(rec), len(rec) // count, q)
    assert _same_bits(got, want)
    assert _same_bits(ctx.capture_set_lookup(cset, levels, rec, q), want)
    monkeypatch.setenv("RTR_SET_SLICE", "64")
    assert _same_bits(ctx.capture_set_lookup(cset, levels, rec, q), want)


@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("count", SC.COUNTS)
def test_shade_entries_equal_the_one_form(ctx, monkeypatch, count, parts):
    chain = (4, 3)
    env = dict(SC.shade_environment(count, chain), parts=parts)
    cset = N.capture_set(SC.volumes(count), 0 if count == 2 else -1)
    good = IC.queries(env, 300)
    bad = IC.bad_queries(good[20])
    q = good.copy()
    q[100:100 + len(bad)] = bad
    host = SC.native_env(env, parts, count)
    want = N.shade_ibl_set_one(host, cset, good)
    want[100:100 + len(bad)] = np.zeros(len(bad), dtype=A.GATHER_OUT_DTYPE)
    ne, dev = _device_env(env, parts, count)
    got = _shade_into(ctx, ne, cset, q)
    assert _same_bits(got, want) and got["valid"].any()
    want_good = N.shade_ibl_set_one(host, cset, good)
    assert _same_bits(ctx.shade_ibl(host, good, captures=cset), want_good)
    monkeypatch.setenv("RTR_SET_SLICE", "64")
    assert _same_bits(ctx.shade_ibl(host, good, captures=cset), want_good)
    with pytest.raises(rtr.RtrError) as e:
        ctx.shade_ibl(host, q, captures=cset)
    assert e.value.code == INV and "index 100" in str(e.value)


# ---- 2. the old behaviour as a special case ----

def test_a_set_that_reaches_nothing_is_the_plain_entry(ctx):
    import torch
    chain = (4, 3)
    levels, rec = SC.records(1, chain)
    cset = N.capture_set(SC.no_reach_volumes(), 0)
    q = SC.queries(1, 4, 300)
    finite = np.isfinite(q["p"]).all(axis=1)
    q = q[finite]  # a non-finite p is BAD for the set alone
    d_rec = _dev(rec)
    got = _lookup_into(ctx, cset, levels, d_rec, len(rec), q)
    cq = N.cube_queries(q["d"], q["alpha"])
    d_q, d_out = _dev(cq), _sentinel((len(q) + 1) * REC)
    torch.cuda.synchronize()
    ctx.cube_chain_lookup_into(levels, d_rec.data_ptr(), len(rec), d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True)
    assert _same_bits(got, _records_from(d_out, len(q))) and got["valid"].any()
    for parts in (2, 3):
        env = dict(SC.shade_environment(1, chain), parts=parts)
        sq = IC.queries(env, 300)
        ne, dev = _device_env(env, parts, 1)
        assert _same_bits(_shade_into(ctx, ne, cset, sq), _shade_into(ctx, ne, None, sq))


def _upload(ctx, sid):
    ctx.upload(G.scene(sid))
    return ctx.scene


def _frame_params():
    return N.preview_params(FRAME["W"], FRAME["H"], FRAME["grid"], region=FRAME["region"])


def _frame_into(ctx, p, ne, cset, stride):
    import torch
    h, w = p.y1 - p.y0, p.x1 - p.x0
    d_lin, d_lit = _sentinel((h * stride + 1) * 24), _sentinel((h * stride + 1) * 4)
    torch.cuda.synchronize()
    ctx.preview_into(p, ne, d_lin.data_ptr(), stride, d_lit.data_ptr(), blocking=True, captures=cset)
    raw_lin, raw_lit = d_lin.cpu().numpy(), d_lit.cpu().numpy()
    assert (raw_lin[h * stride * 24:] == 0xA5).all() and (raw_lit[h * stride * 4:] == 0xA5).all()
    lin = raw_lin.view(np.float64)[:h * stride * 3].reshape(h, stride, 3)
    lit = raw_lit.view(np.int32)[:h * stride].reshape(h, stride)
    assert (lit[:, w:] == np.int32(-1515870811)).all()  # the row padding
    return lin[:, :w].copy(), lit[:, :w].copy()


def _scene_environment(samples, count):
    surf = samples["kind"] == PR.SURFACE
    env = PR.environment(samples["q"]["p"][surf], True)
    env["levels"], env["records"] = SC.records(count, (4, 3))
    return env


def test_preview_under_a_set_that_reaches_nothing_is_the_plain_preview(ctx):
    _upload(ctx, 21)
    p = _frame_params()
    env = _scene_environment(ctx.preview_samples(p), 1)
    far = SC.volume((5000.0,) * 3, (4000.0,) * 3, (6000.0,) * 3, (4500.0,) * 3, (5500.0,) * 3, 0.0)
    cset = N.capture_set(np.array([far]), 0)
    for parts in (2, 3):
        ne, dev = _device_env(env, parts, 1)
        lin, lit = _frame_into(ctx, p, ne, cset, 29)
        plain_lin, plain_lit = _frame_into(ctx, p, ne, None, 29)
        assert _same_bits(lin, plain_lin) and _same_bits(lit, plain_lit)
        assert (lit > 0).any() and (lin != 0).any()


# ---- 3. the preview against the host's reduction ----

def _frame_of(host_env, cset, samples):
    """PIXEL of the preview contract over [h, w, k * k] samples, the SURFACE ones through rtr_shade_ibl_set_one"""
    h, w, kk = samples.shape
    s = np.ascontiguousarray(samples.reshape(-1))
    v, added = s["direct"].copy(), s["kind"] != PR.SURFACE
    L = N.lib()
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    for k in np.flatnonzero(s["kind"] == PR.SURFACE):
        rc = L.rtr_shade_ibl_set_one(C.byref(host_env), C.byref(cset), s.ctypes.data + s.itemsize * int(k), out.ctypes.data)
        if rc == 0 and out["valid"][0]:
            v[k], added[k] = out["v"][0], True
        else:
            v[k] = 0.0
    v, added = v.reshape(h, w, kk, 3), added.reshape(h, w, kk)
    acc = np.zeros((h, w, 3))
    for i in range(kk):
        acc = np.where(added[:, :, i, None], acc + v[:, :, i], acc)
    return np.float64(1.0 / kk) * acc, added.sum(axis=2).astype(np.int32)


@pytest.mark.parametrize("parts", (2, 3))
def test_preview_equals_the_reduction_of_the_host_shader(ctx, parts):
    """C = 3: two volumes that overlap over the Cornell box, one out of reach"""
    _upload(ctx, 21)
    p = _frame_params()
    samples = ctx.preview_samples(p)
    env = _scene_environment(samples, 3)
    room_lo, room_hi = (-1.0,) * 3, (556.0,) * 3
    vols = np.array([SC.volume((278.0, 278.0, 278.0), room_lo, room_hi, room_lo, room_hi, 100.0),
                     SC.volume((200.0, 300.0, 350.0), room_lo, room_hi, (-1.0,) * 3, (400.0, 556.0, 556.0), 0.0),
                     SC.volume((5000.0,) * 3, (4000.0,) * 3, (6000.0,) * 3, (4500.0,) * 3, (5500.0,) * 3, 0.0)])
    cset = N.capture_set(vols, -1)
    host = SC.native_env(env, parts, 3)
    want_lin, want_lit = _frame_of(host, cset, samples)
    assert (want_lit > 0).any() and (want_lin != 0).any()
    lin, lit = ctx.preview(p, host, return_lit=True, captures=cset)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    ne, dev = _device_env(env, parts, 3)
    lin, lit = _frame_into(ctx, p, ne, cset, 31)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    one = N.capture_set(vols[:1], -1)  # the test can see the set: the first capture alone gives another frame
    env1 = dict(env, records=SR.chain_of(env["levels"], env["records"], 3, 0))
    assert not _same_bits(ctx.preview(p, SC.native_env(env1, parts, 1), captures=one), want_lin)


# ---- 4. a bake in stream order, closed against the path tracer ----

COLOURS = ((1.0, 0.25, 0.125), (0.125, 1.0, 0.25), (0.25, 0.125, 1.0), (1.0, 1.0, 0.125), (0.125, 1.0, 1.0), (1.0, 0.125, 1.0))


def _room_scene():
    """a cubic room of six diffuse_light rectangles of six colours; the three far-side walls under flip_face, so every wall
    shows its front face to the room"""
    b = RS.Builder(np.random.default_rng(0), "lean")
    lo = [c - SC.ROOM_HALF for c in SC.ROOM_CENTRE]
    hi = [c + SC.ROOM_HALF for c in SC.ROOM_CENTRE]
    mats = [b.material(A.MAT_DIFFUSE_LIGHT, [b.solid(c)]) for c in COLOURS]
    top = [b.rect("yz", lo[1], hi[1], lo[2], hi[2], lo[0], mats[0]), b.flip_face(b.rect("yz", lo[1], hi[1], lo[2], hi[2], hi[0], mats[1])),
           b.rect("xz", lo[0], hi[0], lo[2], hi[2], lo[1], mats[2]), b.flip_face(b.rect("xz", lo[0], hi[0], lo[2], hi[2], hi[1], mats[3])),
           b.rect("xy", lo[0], hi[0], lo[1], hi[1], lo[2], mats[4]), b.flip_face(b.rect("xy", lo[0], hi[0], lo[1], hi[1], hi[2], mats[5]))]
    root = b.hlist(top)
    base = G.scene(23)
    return rtr.Scene(root, RS._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), RS._cat(b.mats, A.MATERIAL_DTYPE),
                     RS._cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], base.images[:0], base.image_bytes[:0],
                     RS._cat(b.lights, A.LIGHT_DTYPE), base.camera.copy(), np.array([0.0, 0.0, 0.0]))


def test_a_bake_in_stream_order_is_closed_against_the_path_tracer(ctx):
    """rtr_capture_cube_device (S = 8, one sample, no jitter) writes the set's array and rtr_capture_set_lookup_device reads
    it at alpha 0 with no host wait between them: every texel is the emission of the wall it sees, so away from the seams
    the lookup is the radiance of the ray (p, d) itself -- within 1e-14 relative, the bilinear sum of four equal values"""
    import torch
    ctx.upload(_room_scene())
    prm = A.make_params(64, 64, 1, integrator=A.INTEGRATOR_MIS)
    S = SC.ROOM_FACE
    levels, n_records = FR.plan(S, 1)
    cset = N.capture_set(SC.room_volume(), -1)
    q = SC.room_queries(1)
    hit, kept, other = SC.room_classes(q)
    n = len(q)
    d_centre, d_q = _dev(N.probe_points(np.array([SC.ROOM_CENTRE]))), _dev(q)
    d_set, d_out = _sentinel((n_records + 1) * REC), _sentinel((n + 1) * REC)
    torch.cuda.synchronize()
    ctx.capture_cube_into(prm, d_centre.data_ptr(), d_set.data_ptr(), 1, face_size=S, samples=1, jitter=0, blocking=False)
    ctx.capture_set_lookup_into(cset, levels, d_set.data_ptr(), n_records, d_q.data_ptr(), d_out.data_ptr(), n, blocking=False)
    ctx.synchronize()
    got = _records_from(d_out, n)
    rec = _records_from(d_set, n_records)
    assert rec["valid"].all() and got["valid"].all()
    li = ctx.li_rays(prm, q["p"], q["d"], np.zeros(n), np.ones(n, dtype=np.uint32))
    assert set(map(tuple, li)) == set(COLOURS)  # the six walls, their front faces
    err = (np.abs(got["v"] - li) / li)[kept].max()
    print("compared %.3f, another face %.3f, max relative error %.3g" % (kept.mean(), other[kept].mean(), err))
    assert err <= 1e-14
    assert kept.mean() >= 0.75 and other[kept].mean() >= 0.2
    cq = N.cube_queries(q["d"], 0.0)
    d_cq, d_plain = _dev(cq), _sentinel((n + 1) * REC)
    torch.cuda.synchronize()
    ctx.cube_chain_lookup_into(levels, d_set.data_ptr(), n_records, d_cq.data_ptr(), d_plain.data_ptr(), n, blocking=True)
    plain = _records_from(d_plain, n)
    assert (np.abs(plain["v"] - li).max(axis=1)[kept & other] > 0.5).all()  # along d itself: another wall's colour


def test_a_two_capture_three_level_bake_equals_the_host_path(ctx):
    """C = 2 (the room, and an off-centre volume with fade > 0), faces 8, 4, 2: one capture call and one filter call per
    level with n_cubes = 2 into the level-major array, then the lookup, all without a host wait; the host path
    (rtr_capture_cube, rtr_cube_filter, rtr_capture_set_lookup) gives the same bits"""
    import torch
    ctx.upload(_room_scene())
    prm = A.make_params(64, 64, 1, integrator=A.INTEGRATOR_MIS)
    S = SC.ROOM_FACE
    levels, n_records = FR.plan(S, 3)
    room = SC.room_volume()[0]
    c2 = (SC.ROOM_CENTRE[0] + 0.5, SC.ROOM_CENTRE[1] - 0.25, SC.ROOM_CENTRE[2] + 0.75)
    second = SC.volume(c2, room["proxy_lo"], room["proxy_hi"], tuple(c - 1.0 for c in c2), tuple(min(c + 1.0, h) for c, h in zip(c2, room["proxy_hi"])), 0.5)
    vols = np.array([room, second])
    cset = N.capture_set(vols, -1)
    centres = N.probe_points(vols["centre"])
    q = SC.room_queries(2)
    q["alpha"] = np.random.default_rng(4).uniform(0.0, 1.0, len(q))
    n = len(q)
    d_centres, d_q = _dev(centres), _dev(q)
    d_set, d_out = _sentinel((2 * n_records + 1) * REC), _sentinel((n + 1) * REC)
    torch.cuda.synchronize()
    base = d_set.data_ptr()
    ctx.capture_cube_into(prm, d_centres.data_ptr(), base, 2, face_size=S, samples=1, jitter=0, blocking=False)
    for Si, at, alpha in levels[1:]:
        ctx.cube_filter_into(base, base + 2 * at * REC, 2, face_in=S, face_out=Si, alpha=alpha, blocking=False)
    ctx.capture_set_lookup_into(cset, levels, base, n_records, d_q.data_ptr(), d_out.data_ptr(), n, blocking=False)
    ctx.synchronize()
    got = _records_from(d_out, n)
    host = np.zeros(2 * n_records, dtype=A.GATHER_OUT_DTYPE)
    host[:2 * 6 * S * S] = ctx.capture_cube_records(prm, centres, face_size=S, samples=1, jitter=0).reshape(-1)
    for Si, at, alpha in levels[1:]:
        host[2 * at:2 * at + 2 * 6 * Si * Si] = ctx.cube_filter(host[:2 * 6 * S * S], face_in=S, face_out=Si, alpha=alpha).reshape(-1)
    assert _same_bits(_records_from(d_set, 2 * n_records), host)
    want = ctx.capture_set_lookup(cset, levels, host, q)
    assert _same_bits(got, want) and got["valid"].all()
    assert _same_bits(want, N.capture_set_lookup_host(cset, levels, host, q))
    assert len(set(got["count"])) > 1  # one capture and two, one level and two


# ---- 5. checks that need a context ----

def test_entries_check_their_arguments(ctx):
    import torch
    L, h = ctx._L, ctx._h
    levels, rec = SC.records(2, (4, 3))
    lv = N.cube_levels(levels)
    n_records = len(rec) // 2
    cset = N.capture_set(SC.volumes(2), -1)
    q = SC.queries(2, 4, 8)
    out = np.zeros(8, dtype=A.GATHER_OUT_DTYPE)
    d_rec, d_q, d_out = _dev(rec), _dev(q), _sentinel(8 * REC)
    torch.cuda.synchronize()
    rp, qp, op = C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_q.data_ptr()), C.c_void_p(d_out.data_ptr())
    s, l = C.byref(cset), C.byref(lv)
    assert L.rtr_capture_set_lookup(h, s, l, 3, rec.ctypes.data, n_records, q.ctypes.data, out.ctypes.data, -1) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, None, n_records, q.ctypes.data, out.ctypes.data, 8) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, rec.ctypes.data, n_records, None, out.ctypes.data, 8) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, rec.ctypes.data, n_records, q.ctypes.data, None, 8) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, rec.ctypes.data, n_records - 1, q.ctypes.data, out.ctypes.data, 8) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, rec.ctypes.data, -1, q.ctypes.data, out.ctypes.data, 8) == INV
    assert L.rtr_capture_set_lookup(h, None, l, 3, rec.ctypes.data, n_records, q.ctypes.data, out.ctypes.data, 8) == INV
    assert L.rtr_capture_set_lookup(h, s, l, 3, None, n_records, None, None, 0) == 0  # n == 0
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, op, -1, 1) == INV
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, None, 8, 1) == INV
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, None, n_records, None, None, 0, 1) == 0
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, C.c_void_p(d_out.data_ptr() + 4), 7, 1) == INV  # alignment
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, qp, 8, 1) == INV  # out over the queries
    # out over the second capture's records: the overlap rule uses C * n_records
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, C.c_void_p(d_rec.data_ptr() + (2 * n_records - 1) * REC), 8, 1) == INV
    bad = N.capture_set(SC.volumes(2), 2)
    assert L.rtr_capture_set_lookup_device(h, C.byref(bad), l, 3, rp, n_records, qp, op, 8, 1) == INV
    assert not out.view(np.uint8).any() and (d_out.cpu().numpy() == 0xA5).all()
    assert _same_bits(d_rec.cpu().numpy(), rec.view(np.uint8))
    assert L.rtr_capture_set_lookup_device(h, s, l, 3, rp, n_records, qp, op, 8, 1) == 0
    # the shader and the preview: the set's rules behind the environment's, for the specular part only
    env = SC.shade_environment(2, (4, 3))
    sq = IC.queries(env, 8)
    ne, dev = _device_env(env, 3, 2)
    d_sq = _dev(sq)
    torch.cuda.synchronize()
    sqp = C.c_void_p(d_sq.data_ptr())
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne), C.byref(bad), sqp, op, 8, 1) == INV
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne), None, sqp, op, 8, 1) == INV
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne), s, sqp, op, -1, 1) == INV
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne), s, sqp, op, 0, 1) == 0
    over = C.c_void_p(dev["chain"].data_ptr() + (2 * n_records - 1) * REC)  # in the second capture's records
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne), s, sqp, over, 8, 1) == INV
    ne1, dev1 = _device_env(dict(env, parts=1), 1, 2)
    assert L.rtr_shade_ibl_set_device(h, C.byref(ne1), None, sqp, op, 8, 1) == 0  # a NULL set with SPECULAR off
    host = SC.native_env(env, 3, 2)
    assert L.rtr_shade_ibl_set(h, C.byref(host), C.byref(bad), sq.ctypes.data, out.ctypes.data, 8) == INV
    assert L.rtr_shade_ibl_set(h, C.byref(host), s, sq.ctypes.data, out.ctypes.data, -1) == INV
    _upload(ctx, 21)
    p = N.preview_params(8, 6, 1)
    lin = np.zeros((6, 8, 3))
    assert L.rtr_preview_set(h, C.byref(p), C.byref(host), C.byref(bad), lin.ctypes.data, 8, None) == INV
    assert L.rtr_preview_set(h, C.byref(p), C.byref(host), None, lin.ctypes.data, 8, None) == INV
    assert L.rtr_preview_set(h, C.byref(p), C.byref(host), s, lin.ctypes.data, 7, None) == INV
    assert L.rtr_preview_set_device(h, C.byref(p), C.byref(ne), C.byref(bad), over, 8, None, 1) == INV
    assert L.rtr_preview_set_device(h, C.byref(p), C.byref(ne), s, over, 8, None, 1) == INV  # linear in the second capture
    assert not lin.any()


# ---- 6. upper layers ----

CORNELL = dict(lo=(0.0,) * 3, hi=(555.0,) * 3)


def _cornell_volumes():
    lo, hi = CORNELL["lo"], CORNELL["hi"]
    return np.array([SC.volume((278.0, 400.0, 400.0), lo, hi, lo, hi, 50.0),
                     SC.volume((150.0, 300.0, 150.0), lo, hi, lo, (300.0, 555.0, 300.0), 0.0)])


def test_python_faces(ctx):
    """CaptureSet.bake makes the level-major array with one capture call and one filter call per level; chain(k) is what
    the single-capture route makes of centre k; lookup and an IblEnvironment over the set run the set entries"""
    sc = _upload(ctx, 21)
    prm = A.make_params(2, 2, 1, integrator=4, seed=7)
    vols = _cornell_volumes()
    cs = rtr.CaptureSet.bake(ctx, prm, vols, face_size=8, samples=2, levels=3, fallback=0, seed=7)
    assert len(cs) == 2 and cs.n_records == FR.plan(8, 3)[1] and len(cs.records) == 2 * cs.n_records
    for k in range(2):
        cube = rtr.Cubemap(ctx.capture_cube_records(prm, vols["centre"], face_size=8, samples=2, seed=7)[k])
        assert _same_bits(cs.chain(k).records, cube.prefilter(levels=3, ctx=ctx).records)
    rng = np.random.default_rng(2)
    p, d = rng.uniform(20.0, 530.0, (40, 3)), rng.normal(size=(40, 3))
    got = cs.lookup_records(p, d, 0.3, ctx=ctx)
    assert _same_bits(got, cs.lookup_records(p, d, 0.3)) and got["valid"].all()
    assert _same_bits(cs.lookup(p, d, 0.3, ctx=ctx), got["v"])
    grid = rtr.ProbeGrid.in_box((100.0,) * 3, (450.0,) * 3, (2, 2, 2))
    grid.bake(ctx, prm, samples=16, seed=7)
    table = rtr.BrdfTable.make(4, 3, 16, ctx=ctx)
    ibl = rtr.IblEnvironment(grid, cs, table)
    assert ibl.captures is cs.set() and ibl.env().n_records == cs.n_records
    n = rng.normal(size=(40, 3))
    rec = ibl.shade_records(p, n, d, (0.8, 0.6, 0.4), 0.4, 0.5, ctx=ctx)
    assert _same_bits(rec, N.shade_ibl_set_one(ibl.env(), cs.set(), N.shade_queries(p, n, d, (0.8, 0.6, 0.4), 0.4, 0.5)))
    pp = N.preview_params(32, 32, 1)
    lin = ibl.render(ctx, pp)
    assert _same_bits(lin, ctx.preview(pp, ibl.env(), captures=cs.set())) and (lin != 0).any()
    r = rtr.Renderer(context=ctx)
    buf = rtr.RenderBuffer(32, 32)
    r.render_preview(sc, ibl, buf, grid=1)
    assert _same_bits(buf.linear, lin)
    shown = rtr.RenderBuffer(32, 32)
    r.render_preview(sc, ibl, shown, grid=1, display=N.display_defaults())  # the device route: rtr_preview_set_device
    assert _same_bits(shown.linear, lin)
    single = rtr.IblEnvironment(grid, cs.chain(0), table).render(ctx, pp)
    assert not _same_bits(single, lin)  # the single capture at the first centre gives another frame


def test_the_command_line_writes_the_python_path_s_pixels(ctx, tmp_path):
    """rtr_cli --capture-set FILE --capture-fallback 0 --preview 1 on scene 21 at 32 x 32 writes the frame the Python route
    makes of the same bake"""
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    out, path = str(tmp_path / "preview.ppm"), tmp_path / "set.txt"
    vols = _cornell_volumes()
    path.write_text("# two volumes in the Cornell box\n" + "".join(
        " ".join(repr(float(x)) for name in A.CAPTURE_VOLUME_DTYPE.names for x in np.atleast_1d(v[name])) + "\n" for v in vols))
    bake = ["--probes", "2,2,2", "--probe-box", "100,100,100,450,450,450", "--probe-samples", "16", "--capture-set", str(path),
            "--capture-fallback", "0", "--face", "8", "--capture-spp", "2", "--capture-levels", "3", "--brdf-table", "4,3",
            "--brdf-nodes", "16"]
    r = subprocess.run([cli, "21", "4", "--width", "32", "--seed", "7", "--preview", "1", "--out", out] + bake,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert b"capture set: 2 volumes, fallback 0" in r.stdout
    sc = rtr.hostscene.build_scene(21)
    ctx.upload(sc)
    prm = A.make_params(2, 2, 1, integrator=4, seed=7)
    grid = rtr.ProbeGrid.in_box((100.0,) * 3, (450.0,) * 3, (2, 2, 2))
    grid.bake(ctx, prm, samples=16, seed=7)
    cs = rtr.CaptureSet.bake(ctx, prm, vols, face_size=8, samples=2, levels=3, fallback=0, seed=7)
    ibl = rtr.IblEnvironment(grid, cs, rtr.BrdfTable.make(4, 3, 16, ctx=ctx))
    buf = rtr.RenderBuffer(32, 32)
    rtr.Renderer(context=ctx).render_preview(sc, ibl, buf, grid=1)
    assert (buf.linear != 0).any()
    assert open(out, "rb").read()[-32 * 32 * 3:] == buf.to_rgb8().tobytes()
