"""Hemisphere gathers (include/rtr_hip.h: rtr_gather_occlusion / rtr_gather_radiance and their device-pointer forms) on the
GPU.  Occlusion counts are held to the pinned CPU oracle (rto_hits on the rays of the contract, restated in
tests/_gather_ref.py) exactly and the bent normal to the restatement's reduction bit for bit; scenes with media to the
library's own any-hit query on the same rays; radiance to the reduction of rtr_li_rays on the same rays and states.  Batch
shapes, bad points, the device entries behind a queued render, renders and accumulator passes around a gather, the
parameter checks and the command-line driver complete the contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SEED = 7
SAMPLES = (1, 5, 64, 100)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _points(p, n):
    return rtr.native.gather_points(p, n)


_ORACLE = {}


def _oracle(sid, samples, t_max, t_min=0.001):
    """(count, v) the contract gives with the oracle's hits, computed once per case"""
    key = (sid, samples, t_max, t_min)
    if key not in _ORACLE:
        p, n = GR.golden_points(sid)
        d, blocked = GR.oracle_blocked(G.scene(sid), p, n, samples, seed=SEED, t_min=t_min, t_max=t_max)
        _ORACLE[key] = GR.occlusion(d, blocked)
    return _ORACLE[key]


def _assert_occlusion(out, count, v, tag):
    assert np.array_equal(out["count"], count), tag
    assert np.array_equal(_bits(out["v"]), _bits(v)), tag
    assert (out["valid"] == 1).all(), tag


@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("sid,t_max", ((21, np.inf), (21, 150.0), (23, np.inf), (23, 1.0)))
def test_occlusion_equals_the_oracle(ctx, sid, t_max, samples):
    ctx.upload(G.scene(sid))
    p, n = GR.golden_points(sid)
    count, v = _oracle(sid, samples, t_max)
    for order in (False, True):
        out = ctx.gather_occlusion(p, n, samples=samples, seed=SEED, t_max=t_max, reference_order=order)
        _assert_occlusion(out, count, v, (sid, t_max, samples, order))


@pytest.mark.parametrize("t_min", (0.0, -1.0))
def test_occlusion_below_the_shared_division_bound(ctx, t_min):
    """t_min < 2^-100: the launch takes the plain divisions"""
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21)
    count, v = _oracle(21, 64, np.inf, t_min)
    for order in (False, True):
        out = ctx.gather_occlusion(p, n, samples=64, seed=SEED, t_min=t_min, reference_order=order)
        _assert_occlusion(out, count, v, (t_min, order))


def test_scene_with_media_equals_the_any_hit_query(ctx):
    """OCML log inside a medium is the one place where device and oracle may differ in a last bit: the reference here is
    the library's own pinned any-hit form on the rays of rtr_gather_ray, draws included."""
    ctx.upload(G.scene(9))
    p, n = GR.golden_points(9)
    rays = ctx.gather_rays(p, n, samples=64, seed=SEED)
    for order in (False, True):
        occ, rng = ctx.query_occluded(rays.reshape(-1), reference_order=order, return_rng=True)
        assert (rng != rays["rng_state"].reshape(-1)).any()  # the media drew
        count, v = GR.occlusion(rays["direction"], occ.reshape(rays.shape))
        assert ((count > 0) & (count < 64)).any()
        out = ctx.gather_occlusion(p, n, samples=64, seed=SEED, reference_order=order)
        _assert_occlusion(out, count, v, order)


@pytest.mark.parametrize("seed,kw,what", [(19, dict(n_objects=200), "top_trees"), (16, dict(hollow=True), "inverted_boxes")])
def test_random_scenes_equal_the_oracle(ctx, seed, kw, what):
    sc = R.random_scene(seed, **kw)
    assert rtr.native.validate_scene(sc)[what] > 0
    first = G.oracle_records(sc, "rto_hits", R.random_rays(seed, 64))
    first = first[first["hit"] == 1]
    assert len(first) >= 8
    p, n = first["p"].copy(), first["n"].copy()
    d, blocked = GR.oracle_blocked(sc, p, n, 64, seed=SEED)
    count, v = GR.occlusion(d, blocked)
    assert 0 < int(blocked.sum()) < blocked.size
    ctx.upload(sc)
    for order in (False, True):
        out = ctx.gather_occlusion(p, n, samples=64, seed=SEED, reference_order=order)
        _assert_occlusion(out, count, v, (seed, order))


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("sid,integrator", [(21, 0), (21, 1), (21, 2), (21, 3), (21, 4), (23, 4), (9, 1)])
def test_radiance_equals_the_reduction_of_li_rays(ctx, sid, integrator, samples):
    ctx.upload(G.scene(sid))
    p, n = GR.golden_points(sid, 16)
    prm = A.make_params(64, 64, 1, integrator=integrator)
    rays = ctx.gather_rays(p, n, samples=samples, seed=SEED, time=0.25).reshape(-1)
    L = ctx.li_rays(prm, rays["origin"], rays["direction"], rays["time"], rays["rng_state"]).reshape(16, samples, 3)
    assert (L != 0).any()
    out = ctx.gather_radiance(prm, p, n, samples=samples, seed=SEED, time=0.25)
    assert np.array_equal(_bits(out["v"]), _bits(GR.reduce(L))), (sid, integrator, samples)
    assert (out["count"] == samples).all() and (out["valid"] == 1).all()


def test_a_point_facing_away_from_the_scene_sees_the_background(ctx):
    sc = G.scene(1)
    bg = np.asarray(sc.background, dtype=np.float64)
    assert (bg > 0).all()  # not black
    ctx.upload(sc)
    p, n = np.array([[0.0, 5000.0, 0.0]]), np.array([[0.0, 3.0, 0.0]])  # far above everything, looking up
    for samples in (1, 5, 64, 100):
        out = ctx.gather_occlusion(p, n, samples=samples, seed=SEED)
        assert out["count"][0] == samples and out["valid"][0] == 1
        for integrator in range(5):
            rad = ctx.gather_radiance(A.make_params(64, 64, 1, integrator=integrator), p, n, samples=samples, seed=SEED)
            assert rad["count"][0] == samples
            # N <= 100 equal addends and one product: each rounds within 2^-53 relative
            assert np.abs(rad["v"][0] / bg - 1.0).max() <= 1e-13, (samples, integrator)


@pytest.mark.parametrize("samples", (5, 100))  # G = 8: eight points per wave; G = 64
def test_batch_shapes(ctx, samples):
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21, 257)
    pts = _points(p, n)
    keep = pts.copy()
    whole = ctx.gather_occlusion(pts, samples=samples, seed=SEED)
    assert _same_bits(pts, keep)  # the input is not written
    assert (whole["valid"] == 1).all() and 0 < whole["count"].sum() < 257 * samples
    prm = A.make_params(64, 64, 1)
    whole_rad = ctx.gather_radiance(prm, pts[:65], samples=samples, seed=SEED)
    for m in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        out = np.zeros(m + 1, dtype=A.GATHER_OUT_DTYPE)
        out.view(np.uint8)[:] = 0xA5  # sentinels
        got = ctx.gather_occlusion(pts[:m].copy(), samples=samples, seed=SEED, out=out)
        assert got is out and _same_bits(out[:m], whole[:m]), m
        assert (out[m:].view(np.uint8) == 0xA5).all(), m
        if m <= 65:
            out.view(np.uint8)[:] = 0xA5
            ctx.gather_radiance(prm, pts[:m].copy(), samples=samples, seed=SEED, out=out)
            assert _same_bits(out[:m], whole_rad[:m]) and (out[m:].view(np.uint8) == 0xA5).all(), m
    for cut in (64, 129):  # two half-batches with point_base give the bits of the whole
        split = np.concatenate([ctx.gather_occlusion(pts[:cut].copy(), samples=samples, seed=SEED),
                                ctx.gather_occlusion(pts[cut:].copy(), samples=samples, seed=SEED, point_base=cut)])
        assert _same_bits(split, whole), cut
    assert not _same_bits(ctx.gather_occlusion(pts[64:].copy(), samples=samples, seed=SEED), whole[64:])  # (base matters)
    assert _same_bits(pts, keep)


def test_bad_points(ctx):
    import torch
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21, 16)
    pts = _points(p, n)
    prm = A.make_params(64, 64, 1)
    good = ctx.gather_occlusion(pts, samples=5, seed=SEED)
    good_rad = ctx.gather_radiance(prm, pts, samples=5, seed=SEED)
    for field, k, a, value in (("p", 5, 1, np.nan), ("n", 2, 0, np.inf), ("p", 0, 2, -np.inf), ("n", 15, 2, np.nan)):
        bad = pts.copy()
        bad[field][k, a] = value
        out = np.zeros(16, dtype=A.GATHER_OUT_DTYPE)
        out.view(np.uint8)[:] = 0xA5
        for call in (lambda: ctx.gather_occlusion(bad, samples=5, seed=SEED, out=out),
                     lambda: ctx.gather_radiance(prm, bad, samples=5, seed=SEED, out=out)):
            with pytest.raises(rtr.RtrError) as e:
                call()
            assert e.value.code == A.RTR_ERR_INVALID and "index %d" % k in e.value.message, (field, k)
            assert (out.view(np.uint8) == 0xA5).all()
    zero = pts.copy()
    zero["n"][7] = 0.0
    with pytest.raises(rtr.RtrError) as e:
        ctx.gather_occlusion(zero, samples=5)
    assert "index 7" in e.value.message
    # the device entries cannot see the data: the kernel answers a bad point with valid = 0 and casts the others -- those
    # in the same wave included (G = 8: indices 2 and 9 share their wave with six good points each)
    bad = pts.copy()
    bad["p"][2, 1] = np.nan
    bad["n"][9] = 0.0
    d_pts = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    ok = ~np.isin(np.arange(16), (2, 9))
    for radiance, want in ((False, good), (True, good_rad)):
        d_out = torch.full((16 * A.GATHER_OUT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if radiance:
            ctx.gather_radiance_into(prm, d_pts.data_ptr(), d_out.data_ptr(), 16, samples=5, seed=SEED, blocking=True)
        else:
            ctx.gather_occlusion_into(d_pts.data_ptr(), d_out.data_ptr(), 16, samples=5, seed=SEED, blocking=True)
        got = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE)
        assert _same_bits(got[~ok], np.zeros(2, dtype=A.GATHER_OUT_DTYPE)), radiance
        assert _same_bits(got[ok], want[ok]), radiance
    assert _same_bits(d_pts.cpu().numpy(), bad.view(np.uint8))


def test_device_entries_equal_the_host_entries_and_queue_behind_a_render(ctx):
    import torch
    for sid in (21, 9):
        ctx.upload(G.scene(sid))
        p, n = GR.golden_points(sid)
        pts = _points(p, n)
        m = len(pts)
        prm = A.make_params(64, 64, 1, integrator=1)
        host = ctx.gather_occlusion(pts, samples=64, seed=SEED)
        host_rad = ctx.gather_radiance(prm, pts, samples=5, seed=SEED)
        W = H = 256
        rp = A.make_params(W, H, 16, seed=3)
        want = ctx.render(rp)
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_occ = torch.zeros(m * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_rad = torch.zeros(m * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        fb = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.render_into(rp, fb.data_ptr(), W, blocking=False)
        ctx.gather_occlusion_into(d_pts.data_ptr(), d_occ.data_ptr(), m, samples=64, seed=SEED, blocking=False)
        ctx.gather_radiance_into(prm, d_pts.data_ptr(), d_rad.data_ptr(), m, samples=5, seed=SEED, blocking=False)
        ctx.synchronize()
        assert _same_bits(d_occ.cpu().numpy().view(A.GATHER_OUT_DTYPE), host), sid
        assert _same_bits(d_rad.cpu().numpy().view(A.GATHER_OUT_DTYPE), host_rad), sid
        assert np.array_equal(_bits(fb.cpu().numpy()), _bits(want)), sid
        assert ctx.stats()["samples"] == W * H * 16  # the render's statistics survive the gathers


def test_gathers_do_not_interfere_with_renders_and_accumulators(ctx):
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21)
    prm = A.make_params(64, 64, 1)
    p8 = A.make_params(64, 64, 8, seed=11)
    a = ctx.render(p8)
    occ = ctx.gather_occlusion(p, n, samples=64, seed=SEED)
    rad = ctx.gather_radiance(prm, p, n, samples=5, seed=SEED)
    assert np.array_equal(_bits(a), _bits(ctx.render(p8)))
    with ctx.accumulator(A.make_params(64, 64, 1, seed=11)) as acc:
        acc.render(8)
        assert _same_bits(ctx.gather_occlusion(p, n, samples=64, seed=SEED), occ)
        assert _same_bits(ctx.gather_radiance(prm, p, n, samples=5, seed=SEED), rad)
        acc.render(16)
        got = acc.resolve()
    want = ctx.render(A.make_params(64, 64, 16, seed=11, spp_chunks=1))
    assert np.array_equal(_bits(got), _bits(want))


def test_before_upload_flags_and_params():
    p, n = GR.golden_points(21, 4)
    pts = _points(p, n)
    out = np.zeros(4, dtype=A.GATHER_OUT_DTYPE)
    prm = A.make_params(64, 64, 1)
    with rtr.Context(0) as c:
        L = c._L

        def calls(gp, pts_ptr=pts.ctypes.data, out_ptr=out.ctypes.data, m=4):
            g = C.byref(gp)
            return (L.rtr_gather_occlusion(c._h, g, pts_ptr, out_ptr, m),
                    L.rtr_gather_radiance(c._h, C.byref(prm), g, pts_ptr, out_ptr, m),
                    L.rtr_gather_occlusion_device(c._h, g, pts_ptr, out_ptr, m, 1),
                    L.rtr_gather_radiance_device(c._h, C.byref(prm), g, pts_ptr, out_ptr, m, 1))

        assert calls(rtr.native.gather_defaults()) == (A.RTR_ERR_NO_SCENE,) * 4
        c.upload(G.scene(21))
        invalid = (A.RTR_ERR_INVALID,) * 4
        for bit in range(1, 31):  # every unknown flag bit, alone and next to the known one
            assert calls(rtr.native.gather_defaults(flags=1 << bit)) == invalid, bit
            assert calls(rtr.native.gather_defaults(flags=1 | 1 << bit)) == invalid, bit
        assert calls(rtr.native.gather_defaults(flags=-(1 << 31))) == invalid
        for kw in (dict(samples=0), dict(samples=-1), dict(samples=(1 << 20) + 1), dict(t_min=np.nan), dict(t_min=np.inf),
                   dict(t_max=np.nan), dict(time=np.nan), dict(time=-np.inf)):
            assert calls(rtr.native.gather_defaults(**kw)) == invalid, kw
        for k in range(2):
            gp = rtr.native.gather_defaults()
            gp.reserved[k] = 1.0
            assert calls(gp) == invalid
        gp = rtr.native.gather_defaults(samples=5)
        assert calls(gp, m=-1) == invalid
        assert calls(gp, pts_ptr=None) == invalid and calls(gp, out_ptr=None) == invalid
        assert L.rtr_gather_occlusion(c._h, None, pts.ctypes.data, out.ctypes.data, 4) == A.RTR_ERR_INVALID
        assert L.rtr_gather_radiance(c._h, None, C.byref(gp), pts.ctypes.data, out.ctypes.data, 4) == A.RTR_ERR_INVALID
        assert not out.view(np.uint8).any()  # nothing ran
        assert calls(gp, pts_ptr=None, out_ptr=None, m=0) == (A.RTR_OK,) * 4  # n == 0: no launch, nothing read
        assert L.rtr_gather_occlusion_device(c._h, C.byref(gp), pts.ctypes.data + 4, out.ctypes.data, 4, 1) == A.RTR_ERR_INVALID


def test_cli_ao_equals_the_python_route(ctx, tmp_path):
    cli = os.path.join(os.path.dirname(rtr.native.library_path()), "rtr_cli")
    path = str(tmp_path / "ao.ppm")
    r = subprocess.run([cli, "21", "4", "--ao", "64", "--width", "64", "--out", path], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    ctx.upload(rtr.hostscene.build_scene(21))
    W = H = 64
    prm = A.make_params(W, H, 1)
    rays = np.concatenate([ctx.camera_ray(prm, i, j) for j in range(H) for i in range(W)])
    hits = ctx.query_closest(rays)
    hit = hits["hit"] == 1
    assert 0 < hit.sum()
    ao = ctx.gather_occlusion(hits["p"][hit], hits["n"][hit], samples=64)
    grey = np.ones(W * H)
    grey[hit] = ao["count"] / 64
    assert 0 < (grey < 1).sum()
    buf = rtr.RenderBuffer(W, H)
    buf.store_linear(np.repeat(grey.reshape(H, W, 1), 3, axis=2))
    want = b"P6\n%d %d\n255\n" % (W, H) + buf.to_rgb8().tobytes()
    with open(path, "rb") as f:
        assert f.read() == want
    for extra in (["--pick", "1,1"], ["--adaptive", "0.01"], ["--turntable", "2"]):
        r = subprocess.run([cli, "21", "4", "--ao", "8", "--width", "64"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120)
        assert r.returncode == 2, extra


def test_broadcast_form_gives_the_same_bits(ctx, monkeypatch):
    """k_gather_any<T, true> (RTR_GATHER_BROADCAST=1: one load per group and a broadcast), the form tools/time_gather.py
    measures against the one the library launches; bad points and a ragged last wave included."""
    import torch
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21, 257)
    pts = _points(p, n)
    pts["n"][9] = 0.0
    pts["p"][130, 2] = np.nan
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    for samples in (5, 100):
        got = []
        for form in ("0", "1"):
            monkeypatch.setenv("RTR_GATHER_BROADCAST", form)
            d_out = torch.full((257 * A.GATHER_OUT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.gather_occlusion_into(d_pts.data_ptr(), d_out.data_ptr(), 257, samples=samples, seed=SEED, blocking=True)
            got.append(d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE))
        assert _same_bits(got[0], got[1]), samples
        assert got[0]["valid"].sum() == 255 and got[0]["valid"][9] == 0 and got[0]["valid"][130] == 0
