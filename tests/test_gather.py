"""Hemisphere gathers (include/rtr_hip.h: rtr_gather_occlusion / rtr_gather_radiance and their device-pointer forms) on the
GPU.  Occlusion counts are held to the pinned CPU oracle (rto_hits on the rays of the contract, restated in
tests/_gather_ref.py) exactly and the bent normal to the restatement's reduction bit for bit; scenes with media to the
library's own any-hit query on the same rays; radiance to the reduction of rtr_li_rays on the same rays and states.  Batch
shapes, bad points, the device entries behind a queued render, renders and accumulator passes around a gather, the
parameter checks and the command-line driver complete the contract.

csrc/rtr_gather.hip holds 10 k_gather_any<traversal, broadcast> and 17 k_gather_li<integrator, traversal> (GATHER_TABLE
below restates its lists); which one a call launched, and over how many lanes per point, the context records on the host
(Context.last_gather).  The last test asserts that the tests of this module launched, and compared, every one of them:
run the module as a whole."""
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
# lanes per point 2, 4, 16 and 32 (the xor butterfly of gather_end over a part of a wave), each full and with a ragged
# last round, and a second and a third round at 64
WIDTH_SAMPLES = (2, 3, 4, 9, 16, 17, 32, 33, 65, 129)

# RT_TRAV_* of csrc/rt_device.h
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)
TRAV_NAME = ["EXACT", "MEDIA", "FAST", "PROGRAM", "FLAT", "TOP", "PROGRAM_EXT", "FLAT_GUARD"]
# the TravSets of csrc/rtr_gather.hip: TravsTop (k_gather_any, both forms), TravsLi (MIS = 4, RR = 1), TravsN1 (0, 2, 3)
TRAVS_TOP = (FAST, TOP, PROGRAM_EXT, MEDIA, EXACT)
TRAVS_LI = (FAST, PROGRAM_EXT, MEDIA, EXACT)
TRAVS_N1 = (FAST, PROGRAM_EXT, MEDIA)
# (integrator or -1 for k_gather_any, traversal, broadcast)
GATHER_TABLE = {(-1, t, b) for t in TRAVS_TOP for b in (0, 1)} | {(i, t, 0) for i in (4, 1) for t in TRAVS_LI} | \
               {(i, t, 0) for i in (0, 2, 3) for t in TRAVS_N1}
assert len(GATHER_TABLE) == 10 + 17
SEEN = set()  # what the tests of this module launched


def gather_name(g):
    i, t, b = g
    return "k_gather_any<%s, %s>" % (TRAV_NAME[t], "true" if b else "false") if i < 0 else "k_gather_li<%d, %s>" % (i, TRAV_NAME[t])


def _note(ctx, samples, radiance=None):
    """Enters the gather kernel the last call launched into SEEN and returns (integrator, traversal, broadcast).  The lanes
    per point are min(64, the next power of two >= samples) (include/rtr_hip.h), restated here."""
    g = ctx.last_gather()
    assert g is not None
    width = 1
    while width < samples and width < 64:
        width *= 2
    assert 1 << g["lg"] == width, (samples, g)
    if radiance is not None:
        assert (g["integ"] >= 0) == radiance and (radiance or g["integ"] == -1), g
    assert not (g["broadcast"] and g["integ"] >= 0), g
    name = (g["integ"], g["trav"], g["broadcast"])
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
        assert _note(ctx, samples, False) == (-1, EXACT if order else FAST, 0)
        _assert_occlusion(out, count, v, (sid, t_max, samples, order))


@pytest.mark.parametrize("samples", WIDTH_SAMPLES)
def test_occlusion_equals_the_oracle_at_every_group_width(ctx, samples):
    test_occlusion_equals_the_oracle(ctx, 21, np.inf, samples)


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
        assert _note(ctx, 64, False) == (-1, MEDIA if order else PROGRAM_EXT, 0)
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
        want = {("top_trees", False): TOP, ("top_trees", True): EXACT, ("inverted_boxes", False): PROGRAM_EXT,
                ("inverted_boxes", True): MEDIA}[what, order]  # (a guarded hollow sphere: a step program / the media walk)
        assert _note(ctx, 64, False) == (-1, want, 0)
        _assert_occlusion(out, count, v, (seed, order))


_SCENES = {}


def _scene_points(key, m):
    """(scene, p, n) with ``m`` surface points: golden scene ``key``, or the random scenes "top" (200 objects under a top
    tree) and "hollow" (a guarded hollow sphere) with the oracle's hits of random rays"""
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
        return (sc,) + GR.golden_points(key, m)
    assert len(hits) >= m
    return sc, hits["p"][:m].copy(), hits["n"][:m].copy()


def _radiance_case(ctx, key, integrator, samples, order, m=16):
    """one radiance gather against the contract's own reference: GR.reduce of rtr_li_rays on the rays of rtr_gather_ray with
    the same render params, flags included.  Returns (the kernel's name, the output records)."""
    sc, p, n = _scene_points(key, m)
    ctx.upload(sc)
    prm = A.make_params(64, 64, 1, integrator=integrator, flags=A.FLAG_REFERENCE_ORDER if order else 0)
    rays = ctx.gather_rays(p, n, samples=samples, seed=SEED, time=0.25).reshape(-1)
    L = ctx.li_rays(prm, rays["origin"], rays["direction"], rays["time"], rays["rng_state"]).reshape(m, samples, 3)
    # (scene 9 has no light list and a black background: five samples at sixteen points can all miss its one emitter)
    assert (L != 0).any() or (key == 9 and samples < 64), (key, integrator, samples)
    out = ctx.gather_radiance(prm, p, n, samples=samples, seed=SEED, time=0.25)
    name = _note(ctx, samples, True)
    assert np.array_equal(_bits(out["v"]), _bits(GR.reduce(L))), (key, integrator, samples, order)
    assert (out["count"] == samples).all() and (out["valid"] == 1).all()
    return name, out


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
    assert _note(ctx, samples, True) == (integrator, PROGRAM_EXT if sid == 9 else FAST, 0)
    assert np.array_equal(_bits(out["v"]), _bits(GR.reduce(L))), (sid, integrator, samples)
    assert (out["count"] == samples).all() and (out["valid"] == 1).all()


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("order", (False, True))
@pytest.mark.parametrize("integrator", range(5))
@pytest.mark.parametrize("key", (9, "hollow"))
def test_radiance_with_media_and_guarded_steps(ctx, key, integrator, order, samples):
    """Every integrator on a scene with media and on one with a guarded hollow sphere: the general program kernel, and with
    FLAG_REFERENCE_ORDER in the render params the media walk (k_gather_li<I, PROGRAM_EXT> / <I, MEDIA>)."""
    name, _ = _radiance_case(ctx, key, integrator, samples, order)
    assert name == (integrator, MEDIA if order else PROGRAM_EXT, 0)


@pytest.mark.parametrize("samples", (5, 64))
@pytest.mark.parametrize("sid,integrator", [(21, 0), (21, 1), (21, 2), (21, 3), (21, 4), (23, 1), (23, 4)])
def test_radiance_in_reference_order(ctx, sid, integrator, samples):
    """FLAG_REFERENCE_ORDER on scenes without media: k_gather_li<I, EXACT> for MIS and RR; integrators 0, 2 and 3 have no
    such kernel and take the media kernel in its place (csrc/rt_select.h: li_trav).  On scene 21 the walk in reference order and
    the compiled traversal give the same bits (tests/test_gpu_parity.py holds the two to each other there)."""
    name, out = _radiance_case(ctx, sid, integrator, samples, True)
    assert name == (integrator, EXACT if integrator in (1, 4) else MEDIA, 0)
    if sid == 21:
        plain_name, plain = _radiance_case(ctx, sid, integrator, samples, False)
        assert plain_name == (integrator, FAST, 0)
        assert _same_bits(out, plain), (integrator, samples)


@pytest.mark.parametrize("samples", (2, 3, 4, 9, 16, 17, 32, 33))
def test_radiance_at_every_group_width(ctx, samples):
    """2, 4, 16 and 32 lanes per point, each full and with a ragged last round"""
    assert _radiance_case(ctx, 21, 4, samples, False)[0] == (4, FAST, 0)


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


@pytest.mark.parametrize("samples", (3, 17))  # G = 4: sixteen points per wave; G = 32: two
def test_batch_shapes_with_several_points_per_wave(ctx, samples):
    """Batches that end inside a wave, at its end and just behind it, through the device entries (the host entries refuse
    a bad point; the kernels answer it with valid = 0): a bad point in a group that shares its wave with good ones."""
    import torch
    ctx.upload(G.scene(21))
    p, n = GR.golden_points(21)
    count, v = _oracle(21, samples, np.inf)
    pts = _points(p, n)[:33]
    whole = ctx.gather_occlusion(pts, samples=samples, seed=SEED)
    assert _note(ctx, samples, False) == (-1, FAST, 0)
    _assert_occlusion(whole, count[:33], v[:33], samples)
    prm = A.make_params(64, 64, 1)
    whole_rad = ctx.gather_radiance(prm, pts, samples=samples, seed=SEED)
    assert _note(ctx, samples, True) == (4, FAST, 0)
    rays = ctx.gather_rays(pts, samples=samples, seed=SEED).reshape(-1)
    L = ctx.li_rays(prm, rays["origin"], rays["direction"], rays["time"], rays["rng_state"]).reshape(33, samples, 3)
    assert np.array_equal(_bits(whole_rad["v"]), _bits(GR.reduce(L)))
    bad = pts.copy()
    bad["n"][5] = 0.0          # wave 0 at both widths
    bad["p"][16, 1] = np.nan   # G = 4: wave 1 (its first group); G = 32: wave 8
    d_pts = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    size = A.GATHER_OUT_DTYPE.itemsize
    for m in (0, 1, 15, 16, 17, 31, 32, 33):
        ok = ~np.isin(np.arange(m), (5, 16))
        for radiance, want in ((False, whole), (True, whole_rad)):
            d_out = torch.full(((m + 1) * size,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if radiance:
                ctx.gather_radiance_into(prm, d_pts.data_ptr(), d_out.data_ptr(), m, samples=samples, seed=SEED, blocking=True)
            else:
                ctx.gather_occlusion_into(d_pts.data_ptr(), d_out.data_ptr(), m, samples=samples, seed=SEED, blocking=True)
            raw = d_out.cpu().numpy()
            got = raw[:m * size].view(A.GATHER_OUT_DTYPE)
            assert (raw[m * size:] == 0xA5).all(), (m, radiance)  # nothing behind the batch is written
            assert _same_bits(got[ok], want[:m][ok]), (m, radiance)
            assert _same_bits(got[~ok], np.zeros(int((~ok).sum()), dtype=A.GATHER_OUT_DTYPE)), (m, radiance)
    assert _same_bits(d_pts.cpu().numpy(), bad.view(np.uint8))


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


# (scene, reference order) -> the traversal of k_gather_any: all five of its list
BROADCAST_CASES = [(21, False, FAST), (9, False, PROGRAM_EXT), ("top", False, TOP), ("hollow", False, PROGRAM_EXT),
                   (21, True, EXACT), (9, True, MEDIA)]


def test_broadcast_form_gives_the_same_bits(ctx, monkeypatch):
    """k_gather_any<T, true> (RTR_GATHER_BROADCAST=1: one load per group and a broadcast), the form tools/time_gather.py
    measures against the one the library launches, for every traversal; bad points and a ragged last wave included.  The
    form the library launches is held to the oracle (or, with media, to the any-hit query) on the same points first."""
    import torch
    for key, order, trav in BROADCAST_CASES:
        sc, p, n = _scene_points(key, 257)
        ctx.upload(sc)
        pts = _points(p, n)
        rays = ctx.gather_rays(pts, samples=5, seed=SEED)
        if key == 9:
            occ = ctx.query_occluded(rays.reshape(-1), reference_order=order).reshape(rays.shape) != 0
        else:
            _, occ = GR.oracle_blocked(sc, p, n, 5, seed=SEED)
        want5 = GR.occlusion(rays["direction"], occ)
        pts["n"][9] = 0.0
        pts["p"][130, 2] = np.nan
        good = ~np.isin(np.arange(257), (9, 130))
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        for samples in (5, 100):
            got = []
            for form in ("0", "1"):
                monkeypatch.setenv("RTR_GATHER_BROADCAST", form)
                d_out = torch.full((257 * A.GATHER_OUT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.gather_occlusion_into(d_pts.data_ptr(), d_out.data_ptr(), 257, samples=samples, seed=SEED,
                                          reference_order=order, blocking=True)
                assert _note(ctx, samples, False) == (-1, trav, int(form)), (key, order)
                got.append(d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE))
            assert _same_bits(got[0], got[1]), (key, order, samples)
            assert got[0]["valid"].sum() == 255 and got[0]["valid"][9] == 0 and got[0]["valid"][130] == 0
            if samples == 5:
                _assert_occlusion(got[0][good], want5[0][good], want5[1][good], (key, order))


def test_every_gather_kernel_ran_and_was_compared():
    """The union of what the tests above launched is the whole of GATHER_TABLE: every k_gather_any<T, broadcast> and every
    k_gather_li<I, T> of csrc/rtr_gather.hip ran under a test that compares its output."""
    missing = sorted(map(gather_name, GATHER_TABLE - SEEN))
    extra = sorted(map(gather_name, SEEN - GATHER_TABLE))
    print("gather kernels: %d / %d" % (len(SEEN & GATHER_TABLE), len(GATHER_TABLE)))
    assert not missing and not extra, "gather kernels not launched: %s; launched but not in the table: %s" % (missing, extra)
