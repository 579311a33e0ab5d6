"""Light probes (include/rtr_hip.h: rtr_probe_visibility / rtr_probe_radiance, their device-pointer forms and
rtr_probe_lookup) on the GPU.  Visibility is held to the pinned CPU oracle (rto_hits on the rays of the contract, restated
in tests/_probe_ref.py) and to the restatement's projection and reduction bit for bit; scenes with media to the library's
own any-hit query on the same rays; radiance to the projection and reduction of rtr_li_rays on the same rays and states.
Batch shapes, bad points, the device entries behind a queued render, renders and accumulator passes around a probe call,
the parameter checks, the grid lookup and the command-line driver complete the contract.

csrc/rtr_probe.hip holds 5 k_probe_any<traversal> and 17 k_probe_li<integrator, traversal> (PROBE_TABLE below restates its
lists); which one a call launched the context records on the host (Context.last_probe).  The last test asserts that the
tests of this module launched, and compared, every one of them: run the module as a whole.

The probes are the golden hit points of a scene moved DISPLACE[scene] along their normal, so that they sit in free space
in front of the surface they were found on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _probe_ref as PR
import _randscene as R
from test_probes_cpu import lookup_cases

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SEED = 7
SAMPLES = (1, 5, 64, 100)
WIDTH_SAMPLES = (2, 3, 4, 9, 16, 17, 32, 33, 65, 129)
# scenes 21 and 9 are Cornell boxes of side 555, scene 23 is of unit scale
DISPLACE = {21: 5.0, 9: 5.0, 23: 0.05}
FINITE_T_MAX = {21: 150.0, 23: 1.0}

# RT_TRAV_* of csrc/rt_device.h
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)
TRAV_NAME = ["EXACT", "MEDIA", "FAST", "PROGRAM", "FLAT", "TOP", "PROGRAM_EXT", "FLAT_GUARD"]
TRAVS_TOP = (FAST, TOP, PROGRAM_EXT, MEDIA, EXACT)
TRAVS_LI = (FAST, PROGRAM_EXT, MEDIA, EXACT)
TRAVS_N1 = (FAST, PROGRAM_EXT, MEDIA)
# (integrator or -1 for k_probe_any, traversal)
PROBE_TABLE = {(-1, t) for t in TRAVS_TOP} | {(i, t) for i in (4, 1) for t in TRAVS_LI} | {(i, t) for i in (0, 2, 3) for t in TRAVS_N1}
assert len(PROBE_TABLE) == 5 + 17
SEEN = set()  # what the tests of this module launched


def probe_name(g):
    i, t = g
    return "k_probe_any<%s>" % TRAV_NAME[t] if i < 0 else "k_probe_li<%d, %s>" % (i, TRAV_NAME[t])


def _note(ctx, samples, radiance):
    """Enters the probe kernel the last call launched into SEEN and returns (integrator, traversal)."""
    g = ctx.last_probe()
    assert g is not None
    assert 1 << g["lg"] == GR.group_size(samples), (samples, g)
    assert (g["integ"] >= 0) == radiance and (radiance or g["integ"] == -1), g
    name = (g["integ"], g["trav"])
    SEEN.add(name)
    return name


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _points(sid, n=48):
    return PR.displaced_points(sid, DISPLACE[sid], n)


_ORACLE = {}


def _oracle(sid, samples, t_max, t_min=0.001):
    """(count, c) the contract gives with the oracle's hits, computed once per case"""
    key = (sid, samples, t_max, t_min)
    if key not in _ORACLE:
        p = _points(sid)
        d, st = PR.rays(len(p), samples, SEED)
        ora = G.oracle_records(G.scene(sid), "rto_hits", GR.hit_records(p, d, st, t_min, t_max))
        _ORACLE[key] = PR.visibility(d, (ora["hit"] == 1).reshape(len(p), samples))
    return _ORACLE[key]


def _assert_visibility(out, count, c, tag):
    assert np.array_equal(out["count"], count), tag
    assert np.array_equal(_bits(out["c"]), _bits(c)), tag
    assert (out["valid"] == 1).all(), tag


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("sid,t_max", ((21, np.inf), (21, FINITE_T_MAX[21]), (23, np.inf), (23, FINITE_T_MAX[23])))
def test_visibility_equals_the_oracle(ctx, sid, t_max, samples):
    ctx.upload(G.scene(sid))
    p = _points(sid)
    count, c = _oracle(sid, samples, t_max)
    for order in (False, True):
        out = ctx.probe_visibility(p, samples=samples, seed=SEED, t_max=t_max, reference_order=order)
        assert _note(ctx, samples, False) == (-1, EXACT if order else FAST)
        _assert_visibility(out, count, c, (sid, t_max, samples, order))


@pytest.mark.parametrize("samples", WIDTH_SAMPLES)
def test_visibility_equals_the_oracle_at_every_group_width(ctx, samples):
    test_visibility_equals_the_oracle(ctx, 21, np.inf, samples)


@pytest.mark.parametrize("sid", (21, 23))
def test_inputs_are_not_trivial(sid):
    """At each t_max of a scene at least twenty probes are neither fully blocked nor fully open (the boxes are closed on five
    sides: no probe inside sees only sky; test_nothing_blocked_gives_the_reduction_of_the_basis has count == N)."""
    for t_max in (np.inf, FINITE_T_MAX[sid]):
        count, _ = _oracle(sid, 64, t_max)
        assert int(((count > 0) & (count < 64)).sum()) >= 20, (sid, t_max)


@pytest.mark.parametrize("samples", (5, 100))
def test_nothing_blocked_gives_the_reduction_of_the_basis(ctx, samples):
    """t_max just above t_min: no surface lies that close to a displaced probe"""
    ctx.upload(G.scene(21))
    p = _points(21)
    d, _ = PR.rays(len(p), samples, SEED)
    out = ctx.probe_visibility(p, samples=samples, seed=SEED, t_min=0.001, t_max=0.0010001)
    _note(ctx, samples, False)
    assert (out["count"] == samples).all() and (out["valid"] == 1).all()
    assert np.array_equal(_bits(out["c"]), _bits(GR.reduce(PR.basis(d))))


@pytest.mark.parametrize("t_min", (0.0, -1.0))
def test_visibility_below_the_shared_division_bound(ctx, t_min):
    """t_min < 2^-100: the launch takes the plain divisions"""
    ctx.upload(G.scene(21))
    p = _points(21)
    count, c = _oracle(21, 64, np.inf, t_min)
    for order in (False, True):
        out = ctx.probe_visibility(p, samples=64, seed=SEED, t_min=t_min, reference_order=order)
        _assert_visibility(out, count, c, (t_min, order))


def test_scene_with_media_equals_the_any_hit_query(ctx):
    """Inside a medium the reference is the library's own pinned any-hit form on the rays of rtr_probe_ray, draws included."""
    ctx.upload(G.scene(9))
    p = _points(9)
    rays = ctx.probe_rays(p, samples=64, seed=SEED)
    for order in (False, True):
        occ, rng = ctx.query_occluded(rays.reshape(-1), reference_order=order, return_rng=True)
        assert (rng != rays["rng_state"].reshape(-1)).any()  # the media drew
        count, c = PR.visibility(rays["direction"], occ.reshape(rays.shape))
        assert ((count > 0) & (count < 64)).any()
        out = ctx.probe_visibility(p, samples=64, seed=SEED, reference_order=order)
        assert _note(ctx, 64, False) == (-1, MEDIA if order else PROGRAM_EXT)
        _assert_visibility(out, count, c, order)


_SCENES = {}


def _scene_points(key, m):
    """(scene, p) with ``m`` probes: golden scene ``key``, or the random scenes "top" (200 objects under a top tree) and
    "hollow" (a guarded hollow sphere) with the oracle's hits of random rays, moved 0.01 along their normal"""
    if key not in _SCENES:
        if isinstance(key, int):
            _SCENES[key] = (G.scene(key), None)
        else:
            seed, kw, what = {"top": (19, dict(n_objects=200), "top_trees"), "hollow": (16, dict(hollow=True), "inverted_boxes")}[key]
            sc = R.random_scene(seed, **kw)
            assert rtr.native.validate_scene(sc)[what] > 0
            hits = G.oracle_records(sc, "rto_hits", R.random_rays(seed, 512))
            _SCENES[key] = (sc, hits[hits["hit"] == 1])
    sc, hits = _SCENES[key]
    if hits is None:
        return sc, _points(key, m)
    assert len(hits) >= m
    return sc, hits["p"][:m] + 0.01 * hits["n"][:m]


@pytest.mark.parametrize("key", ("top", "hollow"))
def test_random_scenes_equal_the_oracle(ctx, key):
    sc, p = _scene_points(key, 8)
    d, st = PR.rays(len(p), 64, SEED)
    ora = G.oracle_records(sc, "rto_hits", GR.hit_records(p, d, st))
    blocked = (ora["hit"] == 1).reshape(len(p), 64)
    assert 0 < int(blocked.sum()) < blocked.size
    count, c = PR.visibility(d, blocked)
    ctx.upload(sc)
    for order in (False, True):
        out = ctx.probe_visibility(p, samples=64, seed=SEED, reference_order=order)
        want = {("top", False): TOP, ("top", True): EXACT, ("hollow", False): PROGRAM_EXT, ("hollow", True): MEDIA}[key, order]
        assert _note(ctx, 64, False) == (-1, want)
        _assert_visibility(out, count, c, (key, order))


def _radiance_case(ctx, key, integrator, samples, order, m=16):
    """one radiance call against the contract's own reference: the projection and reduction of rtr_li_rays on the rays of
    rtr_probe_ray with the same render params, flags included.  Returns (the kernel's name, the output records)."""
    sc, p = _scene_points(key, m)
    ctx.upload(sc)
    prm = A.make_params(64, 64, 1, integrator=integrator, flags=A.FLAG_REFERENCE_ORDER if order else 0)
    rays = ctx.probe_rays(p, samples=samples, seed=SEED, time=0.25)
    flat = rays.reshape(-1)
    L = ctx.li_rays(prm, flat["origin"], flat["direction"], flat["time"], flat["rng_state"]).reshape(m, samples, 3)
    assert (L != 0).any() or (key == 9 and samples < 64), (key, integrator, samples)
    out = ctx.probe_radiance(prm, p, samples=samples, seed=SEED, time=0.25)
    name = _note(ctx, samples, True)
    want = PR.radiance(rays["direction"], L)
    assert want.shape == (m, 9, 3)
    assert np.array_equal(_bits(out["c"]), _bits(want)), (key, integrator, samples, order)
    assert (out["count"] == samples).all() and (out["valid"] == 1).all()
    return name, out


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("sid,integrator", [(21, 0), (21, 1), (21, 2), (21, 3), (21, 4), (23, 4), (9, 1)])
def test_radiance_equals_the_reduction_of_li_rays(ctx, sid, integrator, samples):
    name, out = _radiance_case(ctx, sid, integrator, samples, False)
    assert name == (integrator, PROGRAM_EXT if sid == 9 else FAST)
    if sid == 21 and samples == 64:
        band0 = out["c"][:, 0, :]  # K0 times the mean radiance: never negative, zero only for a probe shut inside a box
        assert (band0 >= 0).all() and (band0 > 0).sum() >= band0.size // 2


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("order", (False, True))
@pytest.mark.parametrize("integrator", range(5))
@pytest.mark.parametrize("key", (9, "hollow"))
def test_radiance_with_media_and_guarded_steps(ctx, key, integrator, order, samples):
    """Every integrator on a scene with media and on one with a guarded hollow sphere: the general program kernel, and with
    FLAG_REFERENCE_ORDER in the render params the media walk (k_probe_li<I, PROGRAM_EXT> / <I, MEDIA>)."""
    name, _ = _radiance_case(ctx, key, integrator, samples, order)
    assert name == (integrator, MEDIA if order else PROGRAM_EXT)


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("sid,integrator", [(21, 0), (21, 1), (21, 2), (21, 3), (21, 4), (23, 1), (23, 4)])
def test_radiance_in_reference_order(ctx, sid, integrator, samples):
    """FLAG_REFERENCE_ORDER on scenes without media: k_probe_li<I, EXACT> for MIS and RR; integrators 0, 2 and 3 take the
    media kernel in its place (csrc/rt_select.h: li_trav), like the gathers."""
    name, out = _radiance_case(ctx, sid, integrator, samples, True)
    assert name == (integrator, EXACT if integrator in (1, 4) else MEDIA)
    if sid == 21:
        plain_name, plain = _radiance_case(ctx, sid, integrator, samples, False)
        assert plain_name == (integrator, FAST)
        assert _same_bits(out, plain), (integrator, samples)


@pytest.mark.parametrize("samples", (2, 3, 4, 9, 16, 17, 32, 33, 65, 129))
def test_radiance_at_every_group_width(ctx, samples):
    assert _radiance_case(ctx, 21, 4, samples, False)[0] == (4, FAST)


@pytest.mark.parametrize("key", ("top", "hollow"))
def test_radiance_on_random_scenes(ctx, key):
    for integrator in (4, 1):
        name, _ = _radiance_case(ctx, key, integrator, 17, False, m=8)
        assert name == (integrator, PROGRAM_EXT if key == "hollow" else FAST)


@pytest.mark.parametrize("samples", (5, 100))  # G = 8: eight points per wave; G = 64
def test_batch_shapes(ctx, samples):
    ctx.upload(G.scene(21))
    p = _points(21, 257)
    pts = rtr.native.probe_points(p)
    keep = pts.copy()
    whole = ctx.probe_visibility(pts, samples=samples, seed=SEED)
    assert _same_bits(pts, keep)  # the input is not written
    assert (whole["valid"] == 1).all() and 0 < whole["count"].sum() < 257 * samples
    prm = A.make_params(64, 64, 1)
    whole_rad = ctx.probe_radiance(prm, pts[:65], samples=samples, seed=SEED)
    for m in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        out = np.zeros(m + 1, dtype=A.PROBE_VIS_DTYPE)
        out.view(np.uint8)[:] = 0xA5  # sentinels
        got = ctx.probe_visibility(pts[:m].copy(), samples=samples, seed=SEED, out=out)
        assert got is out and _same_bits(out[:m], whole[:m]), m
        assert (out[m:].view(np.uint8) == 0xA5).all(), m
        if m <= 65:
            rad = np.zeros(m + 1, dtype=A.PROBE_SH_DTYPE)
            rad.view(np.uint8)[:] = 0xA5
            ctx.probe_radiance(prm, pts[:m].copy(), samples=samples, seed=SEED, out=rad)
            assert _same_bits(rad[:m], whole_rad[:m]) and (rad[m:].view(np.uint8) == 0xA5).all(), m
    for cut in (64, 129):  # two half-batches with point_base give the bits of the whole
        split = np.concatenate([ctx.probe_visibility(pts[:cut].copy(), samples=samples, seed=SEED),
                                ctx.probe_visibility(pts[cut:].copy(), samples=samples, seed=SEED, point_base=cut)])
        assert _same_bits(split, whole), cut
    split = np.concatenate([ctx.probe_radiance(prm, pts[:33].copy(), samples=samples, seed=SEED),
                            ctx.probe_radiance(prm, pts[33:65].copy(), samples=samples, seed=SEED, point_base=33)])
    assert _same_bits(split, whole_rad)
    assert not _same_bits(ctx.probe_visibility(pts[64:].copy(), samples=samples, seed=SEED), whole[64:])  # (base matters)


@pytest.mark.parametrize("samples", (3, 17))  # G = 4: sixteen points per wave; G = 32: two
def test_batch_shapes_with_several_points_per_wave(ctx, samples):
    """Batches that end inside a wave, at its end and just behind it, through the device entries (the host entries refuse
    a bad point; the kernels answer it with valid = 0): a bad point in a group that shares its wave with good ones."""
    import torch
    ctx.upload(G.scene(21))
    p = _points(21)
    count, c = _oracle(21, samples, np.inf)
    pts = rtr.native.probe_points(p)[:33]
    whole = ctx.probe_visibility(pts, samples=samples, seed=SEED)
    assert _note(ctx, samples, False) == (-1, FAST)
    _assert_visibility(whole, count[:33], c[:33], samples)
    prm = A.make_params(64, 64, 1)
    whole_rad = ctx.probe_radiance(prm, pts, samples=samples, seed=SEED)
    assert _note(ctx, samples, True) == (4, FAST)
    rays = ctx.probe_rays(pts, samples=samples, seed=SEED)
    flat = rays.reshape(-1)
    L = ctx.li_rays(prm, flat["origin"], flat["direction"], flat["time"], flat["rng_state"]).reshape(33, samples, 3)
    assert np.array_equal(_bits(whole_rad["c"]), _bits(PR.radiance(rays["direction"], L)))
    bad = pts.copy()
    bad["p"][5, 0] = np.inf    # wave 0 at both widths
    bad["p"][16, 1] = np.nan   # G = 4: wave 1 (its first group); G = 32: wave 8
    d_pts = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    for m in (0, 1, 15, 16, 17, 31, 32, 33):
        ok = ~np.isin(np.arange(m), (5, 16))
        for dtype, want in ((A.PROBE_VIS_DTYPE, whole), (A.PROBE_SH_DTYPE, whole_rad)):
            size = dtype.itemsize
            d_out = torch.full(((m + 1) * size,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if dtype is A.PROBE_SH_DTYPE:
                ctx.probe_radiance_into(prm, d_pts.data_ptr(), d_out.data_ptr(), m, samples=samples, seed=SEED, blocking=True)
            else:
                ctx.probe_visibility_into(d_pts.data_ptr(), d_out.data_ptr(), m, samples=samples, seed=SEED, blocking=True)
            raw = d_out.cpu().numpy()
            got = raw[:m * size].view(dtype)
            assert (raw[m * size:] == 0xA5).all(), (m, size)  # nothing behind the batch is written
            assert _same_bits(got[ok], want[:m][ok]), (m, size)
            assert _same_bits(got[~ok], np.zeros(int((~ok).sum()), dtype=dtype)), (m, size)
    assert _same_bits(d_pts.cpu().numpy(), bad.view(np.uint8))


def test_bad_points_are_rejected_by_the_host_entries(ctx):
    ctx.upload(G.scene(21))
    pts = rtr.native.probe_points(_points(21, 16))
    prm = A.make_params(64, 64, 1)
    for k, a, value in ((5, 1, np.nan), (0, 2, -np.inf), (15, 0, np.inf)):
        bad = pts.copy()
        bad["p"][k, a] = value
        vis = np.zeros(16, dtype=A.PROBE_VIS_DTYPE)
        sh = np.zeros(16, dtype=A.PROBE_SH_DTYPE)
        vis.view(np.uint8)[:] = 0xA5
        sh.view(np.uint8)[:] = 0xA5
        for call in (lambda: ctx.probe_visibility(bad, samples=5, seed=SEED, out=vis),
                     lambda: ctx.probe_radiance(prm, bad, samples=5, seed=SEED, out=sh)):
            with pytest.raises(rtr.RtrError) as e:
                call()
            assert e.value.code == A.RTR_ERR_INVALID and "index %d" % k in e.value.message, k
        assert (vis.view(np.uint8) == 0xA5).all() and (sh.view(np.uint8) == 0xA5).all()


def test_device_entries_equal_the_host_entries_and_queue_behind_a_render(ctx):
    import torch
    for sid in (21, 9):
        ctx.upload(G.scene(sid))
        pts = rtr.native.probe_points(_points(sid))
        m = len(pts)
        prm = A.make_params(64, 64, 1, integrator=1)
        host = ctx.probe_visibility(pts, samples=64, seed=SEED)
        host_rad = ctx.probe_radiance(prm, pts, samples=5, seed=SEED)
        W = H = 256
        rp = A.make_params(W, H, 16, seed=3)
        want = ctx.render(rp)
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_vis = torch.zeros(m * A.PROBE_VIS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_rad = torch.zeros(m * A.PROBE_SH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        fb = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.render_into(rp, fb.data_ptr(), W, blocking=False)
        ctx.probe_visibility_into(d_pts.data_ptr(), d_vis.data_ptr(), m, samples=64, seed=SEED, blocking=False)
        ctx.probe_radiance_into(prm, d_pts.data_ptr(), d_rad.data_ptr(), m, samples=5, seed=SEED, blocking=False)
        ctx.synchronize()
        assert _same_bits(d_vis.cpu().numpy().view(A.PROBE_VIS_DTYPE), host), sid
        assert _same_bits(d_rad.cpu().numpy().view(A.PROBE_SH_DTYPE), host_rad), sid
        assert np.array_equal(_bits(fb.cpu().numpy()), _bits(want)), sid
        assert ctx.stats()["samples"] == W * H * 16  # the render's statistics survive the probe calls


def test_probes_do_not_interfere_with_renders_and_accumulators(ctx):
    ctx.upload(G.scene(21))
    p = _points(21)
    prm = A.make_params(64, 64, 1)
    p8 = A.make_params(64, 64, 8, seed=11)
    a = ctx.render(p8)
    vis = ctx.probe_visibility(p, samples=64, seed=SEED)
    rad = ctx.probe_radiance(prm, p, samples=5, seed=SEED)
    assert np.array_equal(_bits(a), _bits(ctx.render(p8)))
    with ctx.accumulator(A.make_params(64, 64, 1, seed=11)) as acc:
        acc.render(8)
        assert _same_bits(ctx.probe_visibility(p, samples=64, seed=SEED), vis)
        assert _same_bits(ctx.probe_radiance(prm, p, samples=5, seed=SEED), rad)
        acc.render(16)
        got = acc.resolve()
    want = ctx.render(A.make_params(64, 64, 16, seed=11, spp_chunks=1))
    assert np.array_equal(_bits(got), _bits(want))


def test_before_upload_flags_and_params():
    pts = rtr.native.probe_points(_points(21, 4))
    vis = np.zeros(4, dtype=A.PROBE_VIS_DTYPE)
    sh = np.zeros(4, dtype=A.PROBE_SH_DTYPE)
    prm = A.make_params(64, 64, 1)
    with rtr.Context(0) as c:
        L = c._L

        def calls(gp, pts_ptr=pts.ctypes.data, out=True, m=4):
            g = C.byref(gp)
            v, s = (vis.ctypes.data, sh.ctypes.data) if out else (None, None)
            return (L.rtr_probe_visibility(c._h, g, pts_ptr, v, m),
                    L.rtr_probe_radiance(c._h, C.byref(prm), g, pts_ptr, s, m),
                    L.rtr_probe_visibility_device(c._h, g, pts_ptr, v, m, 1),
                    L.rtr_probe_radiance_device(c._h, C.byref(prm), g, pts_ptr, s, m, 1))

        assert calls(rtr.native.gather_defaults()) == (A.RTR_ERR_NO_SCENE,) * 4
        c.upload(G.scene(21))
        invalid = (A.RTR_ERR_INVALID,) * 4
        for bit in range(1, 31):  # every unknown flag bit, alone and next to the known one
            assert calls(rtr.native.gather_defaults(flags=1 << bit)) == invalid, bit
            assert calls(rtr.native.gather_defaults(flags=1 | 1 << bit)) == invalid, bit
        for kw in (dict(samples=0), dict(samples=-1), dict(samples=(1 << 20) + 1), dict(t_min=np.nan), dict(t_min=np.inf),
                   dict(t_max=np.nan), dict(time=np.nan), dict(time=-np.inf)):
            assert calls(rtr.native.gather_defaults(**kw)) == invalid, kw
        for k in range(2):
            gp = rtr.native.gather_defaults()
            gp.reserved[k] = 1.0
            assert calls(gp) == invalid
        gp = rtr.native.gather_defaults(samples=5)
        assert calls(gp, m=-1) == invalid
        assert calls(gp, pts_ptr=None) == invalid and calls(gp, out=False) == invalid
        assert L.rtr_probe_visibility(c._h, None, pts.ctypes.data, vis.ctypes.data, 4) == A.RTR_ERR_INVALID
        assert L.rtr_probe_radiance(c._h, None, C.byref(gp), pts.ctypes.data, sh.ctypes.data, 4) == A.RTR_ERR_INVALID
        assert not vis.view(np.uint8).any() and not sh.view(np.uint8).any()  # nothing ran
        assert calls(gp, pts_ptr=None, out=False, m=0) == (A.RTR_OK,) * 4  # n == 0: no launch, nothing read
        assert L.rtr_probe_visibility_device(c._h, C.byref(gp), pts.ctypes.data + 4, vis.ctypes.data, 4, 1) == A.RTR_ERR_INVALID
        assert c.last_probe() is None  # none of this launched anything


@pytest.mark.parametrize("case", lookup_cases(), ids=lambda c: c[0])
def test_lookup_kernel_equals_the_restatement(ctx, case):
    import torch
    name, grid, (origin, spacing, dims), probes, pts, nrm = case
    want = PR.lookup(origin, spacing, dims, probes, pts, nrm)
    got = ctx.probe_lookup(grid, probes, pts, nrm)
    assert _same_bits(got, want), name
    # the device form, with a bad query in the middle: valid 0 for it, the others unchanged
    q = rtr.native.gather_points(pts, nrm)
    q = np.concatenate([q, q[:1], q])
    q["p"][len(pts), 1] = np.nan
    d_probes = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    d_out = torch.full(((len(q) + 1) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.probe_lookup_into(grid, d_probes.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True)
    raw = d_out.cpu().numpy()
    dev = raw[:len(q) * 32].view(A.GATHER_OUT_DTYPE)
    assert (raw[len(q) * 32:] == 0xA5).all()
    assert _same_bits(dev[:len(pts)], want) and _same_bits(dev[len(pts) + 1:], want), name
    assert _same_bits(dev[len(pts)], np.zeros(1, dtype=A.GATHER_OUT_DTYPE)[0])
    bad = q.copy()
    with pytest.raises(rtr.RtrError) as e:
        ctx.probe_lookup(grid, probes, bad)
    assert e.value.code == A.RTR_ERR_INVALID and "index %d" % len(pts) in e.value.message


def test_lookup_in_a_baked_grid(ctx):
    """a 3 x 2 x 2 grid baked on scene 21, 64 queries: ProbeGrid.bake / irradiance against the restatement on the baked
    records, and the baked records against the projection of rtr_li_rays"""
    ctx.upload(G.scene(21))
    grid = rtr.ProbeGrid.in_box((100.0, 400.0, 100.0), (450.0, 500.0, 450.0), (3, 2, 2))
    prm = A.make_params(64, 64, 1)
    grid.bake(ctx, prm, samples=16, seed=SEED)
    assert _note(ctx, 16, True) == (4, FAST)
    pos = grid.positions()
    rays = ctx.probe_rays(pos, samples=16, seed=SEED)
    flat = rays.reshape(-1)
    L = ctx.li_rays(prm, flat["origin"], flat["direction"], flat["time"], flat["rng_state"]).reshape(12, 16, 3)
    assert np.array_equal(_bits(grid.coefficients["c"]), _bits(PR.radiance(rays["direction"], L)))
    assert (grid.coefficients["valid"] == 1).all() and (grid.coefficients["c"][:, 0, :] > 0).all()
    rng = np.random.default_rng(3)
    q = 50.0 + rng.random((64, 3)) * 450.0  # some outside the grid's box: clamped
    n = rng.standard_normal((64, 3))
    E = grid.irradiance(q, n)
    want = PR.lookup(grid.origin, grid.spacing, grid.dims, grid.coefficients, q, n)
    assert (want["valid"] == 1).all()
    assert np.array_equal(_bits(E), _bits(want["v"]))
    c = grid.grid()
    for bad in (lambda g: g.spacing.__setitem__(0, 0.0), lambda g: g.dims.__setitem__(1, 0), lambda g: setattr(g, "pad", 3)):
        g = grid.grid()
        bad(g)
        with pytest.raises(rtr.RtrError) as e:
            ctx.probe_lookup(g, grid.coefficients[:1].repeat(g.dims[0] * g.dims[1] * g.dims[2]), q, n)
        assert e.value.code == A.RTR_ERR_INVALID
    assert _same_bits(ctx.probe_lookup(c, grid.coefficients, q, n)["v"], E)


def test_lookup_needs_no_scene():
    name, grid, (origin, spacing, dims), probes, pts, nrm = lookup_cases()[0]
    with rtr.Context(0) as c:
        assert _same_bits(c.probe_lookup(grid, probes, pts, nrm), PR.lookup(origin, spacing, dims, probes, pts, nrm))
        L = c._L
        out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
        q = rtr.native.gather_points(pts[:1], nrm[:1])
        assert L.rtr_probe_lookup(c._h, C.byref(grid), probes.ctypes.data, q.ctypes.data, out.ctypes.data, -1) == A.RTR_ERR_INVALID
        assert L.rtr_probe_lookup(c._h, C.byref(grid), None, q.ctypes.data, out.ctypes.data, 1) == A.RTR_ERR_INVALID
        assert L.rtr_probe_lookup(c._h, C.byref(grid), probes.ctypes.data, None, out.ctypes.data, 1) == A.RTR_ERR_INVALID
        assert L.rtr_probe_lookup(c._h, C.byref(grid), None, None, None, 0) == A.RTR_OK  # n == 0: nothing read
        assert L.rtr_probe_lookup_device(c._h, C.byref(grid), None, None, None, 0, 1) == A.RTR_OK
        assert L.rtr_probe_lookup_device(c._h, C.byref(grid), probes.ctypes.data + 4, q.ctypes.data, out.ctypes.data, 1, 1) == A.RTR_ERR_INVALID
        assert not out.view(np.uint8).any()


def test_cli_probes_equal_the_python_route(ctx):
    cli = os.path.join(os.path.dirname(rtr.native.library_path()), "rtr_cli")
    box = "100,400,100,450,500,450"
    r = subprocess.run([cli, "21", "4", "--probes", "3,2,2", "--probe-box", box, "--probe-samples", "16", "--seed", "7"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    ctx.upload(rtr.hostscene.build_scene(21))
    grid = rtr.ProbeGrid.in_box((100.0, 400.0, 100.0), (450.0, 500.0, 450.0), (3, 2, 2))
    grid.bake(ctx, A.make_params(64, 64, 1, integrator=4), samples=16, seed=7)
    lines = ["%d %d " % (rec["valid"], rec["count"]) + " ".join("%.17g" % v for v in rec["c"].reshape(-1)) for rec in grid.coefficients]
    assert r.stdout.decode().splitlines() == lines
    assert (grid.coefficients["c"][:, 0, :] > 0).all()
    for extra in (["--pick", "1,1"], ["--ao", "8"], ["--adaptive", "0.01"], ["--turntable", "2"]):
        r = subprocess.run([cli, "21", "4", "--probes", "2,2,2", "--probe-box", box] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, extra
    for args in (["--probes", "2,2,2"], ["--probe-box", box], ["--probes", "0,1,1", "--probe-box", box],
                 ["--probes", "2,2,2", "--probe-box", "0,0,0,1,1"], ["--probes", "2,2,2", "--probe-box", "0,0,0,0,1,1"]):
        r = subprocess.run([cli, "21", "4"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, args


def test_every_probe_kernel_ran_and_was_compared():
    """The union of what the tests above launched is the whole of PROBE_TABLE: every k_probe_any<T> and every
    k_probe_li<I, T> of csrc/rtr_probe.hip ran under a test that compares its output."""
    missing = sorted(map(probe_name, PROBE_TABLE - SEEN))
    extra = sorted(map(probe_name, SEEN - PROBE_TABLE))
    print("probe kernels: %d / %d" % (len(SEEN & PROBE_TABLE), len(PROBE_TABLE)))
    assert not missing and not extra, "probe kernels not launched: %s; launched but not in the table: %s" % (missing, extra)
