"""Ray queries (include/rtr_hip.h: rtr_query_closest / rtr_query_occluded and their device-pointer forms) on the GPU.

Closest hits are held to the reference's own hit vectors (tests/golden/hits_scene*.bin) and to the device unit kernel
rtr_test_hits, bit for bit; intervals other than [0.001, inf) and random scenes to the pinned CPU oracle (rto_hits);
occlusion to the closest query's hit flag and generator state.  Batch shapes, bad rays, the device-pointer entries behind
a queued render, and renders / accumulator passes around a query complete the contract."""
import os
import subprocess

import numpy as np
import pytest

import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

MEDIA_FREE = (21, 23, 1, 35, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1012, 1013)
MEDIA = (8, 9, 1009, 1010)
OUT_FIELDS = ("hit", "front_face", "material", "rng_out", "t", "p", "n", "u", "v")


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _rays(recs):
    """rtr_ray of golden hit records (rtr_hit_record inputs)"""
    rays = np.zeros(len(recs), dtype=A.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["time"] = recs["o"], recs["d"], recs["time"]
    rays["t_min"], rays["t_max"], rays["rng_state"] = recs["t_min"], recs["t_max"], recs["rng_in"]
    return rays


def _gold(sid):
    return G.records("hits_scene%02d.bin" % sid, A.HIT_DTYPE)


def _assert_equals_unit_kernel(q, dev, tag):
    for f in OUT_FIELDS:  # NaNs of (u, v) compared as bits
        assert _same_bits(q[f], dev[f]), (tag, f)


@pytest.mark.parametrize("sid", MEDIA_FREE)
def test_golden_records_equal_the_reference_and_the_unit_kernel(ctx, sid):
    ctx.upload(G.scene(sid))
    gold = _gold(sid)
    assert len(gold) <= 2048
    rays = _rays(gold)
    h = gold["hit"] == 1
    for order in (False, True):
        q = ctx.query_closest(rays, reference_order=order)
        assert np.array_equal(q["hit"], gold["hit"]), (sid, order)
        for f in ("front_face", "material"):
            assert np.array_equal(q[f][h], gold[f][h]), (sid, order, f)
        for f in ("t", "p", "n"):
            bad = int((_bits(q[f][h]) != _bits(gold[f][h])).reshape(int(h.sum()), -1).any(axis=1).sum())
            assert bad == 0, (sid, order, f, bad)
        ctx.reference_order(order)
        dev = ctx.test_records("hits", gold)
        ctx.reference_order(False)
        _assert_equals_unit_kernel(q, dev, (sid, order))
        assert np.array_equal(q["rng_out"], rays["rng_state"])  # no media: the generator is not touched
        occ, rng = ctx.query_occluded(rays, reference_order=order, return_rng=True)
        assert np.array_equal(occ, q["hit"] == 1) and np.array_equal(rng, q["rng_out"]), (sid, order)


@pytest.mark.parametrize("sid", MEDIA)
def test_media_records_equal_the_unit_kernel_and_occlusion_equals_closest(ctx, sid):
    ctx.upload(G.scene(sid))
    gold = _gold(sid)
    rays = _rays(gold)
    for order in (False, True):
        q = ctx.query_closest(rays, reference_order=order)
        ctx.reference_order(order)
        dev = ctx.test_records("hits", gold)
        ctx.reference_order(False)
        _assert_equals_unit_kernel(q, dev, (sid, order))
        assert (q["rng_out"] != rays["rng_state"]).any()  # the media drew
        occ, rng = ctx.query_occluded(rays, reference_order=order, return_rng=True)
        assert np.array_equal(occ, q["hit"] == 1), (sid, order)
        assert np.array_equal(rng, q["rng_out"]), (sid, order)


def test_finite_intervals_equal_the_oracle(ctx):
    """Scene 21: t_max at half, exactly, one ulp above and twice the golden t (t_max == t is the rectangles' inclusive
    bound), t_min at the integrators' 0.001 and at 0, 1e-120 and -1 (below 2^-100: the wave takes the plain divisions).
    Once with waves of one t_min each and once shuffled, so waves mix them."""
    sc = G.scene(21)
    ctx.upload(sc)
    gold = _gold(21)
    gold = gold[gold["hit"] == 1]
    parts = []
    for t_min in (0.001, 0.0, 1e-120, -1.0):
        for k in range(4):
            r = gold.copy()
            t = gold["t"]
            r["t_max"] = (0.5 * t, t, np.nextafter(t, np.inf), 2.0 * t)[k]
            r["t_min"] = t_min
            parts.append(r)
    recs = np.concatenate(parts)
    recs = np.concatenate([recs, recs[np.random.default_rng(5).permutation(len(recs))]])
    ora = G.oracle_records(sc, "rto_hits", recs)
    assert 0 < int(ora["hit"].sum()) < len(ora)
    rays = _rays(recs)
    h = ora["hit"] == 1
    for order in (False, True):
        q = ctx.query_closest(rays, reference_order=order)
        assert int((q["hit"] != ora["hit"]).sum()) == 0, order
        for f in ("front_face", "material"):
            assert np.array_equal(q[f][h], ora[f][h]), (order, f)
        for f in ("t", "p", "n"):
            bad = int((_bits(q[f][h]) != _bits(ora[f][h])).reshape(int(h.sum()), -1).any(axis=1).sum())
            assert bad == 0, (order, f, bad)
        occ = ctx.query_occluded(rays, reference_order=order)
        assert int((occ != h).sum()) == 0, order


RANDOM = [(19, dict(n_objects=200), "top_trees"), (16, dict(hollow=True), "inverted_boxes"),
          (32, dict(moved_media=True), "moved_media")]


@pytest.mark.parametrize("seed,kw,what", RANDOM)
def test_random_scenes_equal_the_oracle(ctx, seed, kw, what):
    """One scene with a top tree, one with a guarded step (a hollow sphere), one with a medium under translate / rotate_y;
    the acceptance of tests/test_random_scenes.py for rtr_test_hits."""
    sc = R.random_scene(seed, **kw)
    info = rtr.native.validate_scene(sc)
    if what == "moved_media":
        assert info["has_media"] and info["program_steps"] >= 4
        t = sc.nodes["type"]
        rot_of_medium = (t == A.NODE_ROTATE_Y) & (t[np.clip(sc.nodes["a"], 0, len(t) - 1)] == A.NODE_MEDIUM)
        moved = (t == A.NODE_TRANSLATE) & np.isin(sc.nodes["a"], np.flatnonzero(rot_of_medium))
        assert moved.any()  # translate(rotate_y(constant_medium))
    else:
        assert info[what] > 0
    ctx.upload(sc)
    recs = R.random_rays(seed, 1024)
    ora = G.oracle_records(sc, "rto_hits", recs)
    rays = _rays(recs)
    h = ora["hit"] == 1
    fog = h & np.isin(ora["material"], np.flatnonzero(sc.materials["type"] == A.MAT_ISOTROPIC))
    surf = h & ~fog
    for order in (False, True):
        q = ctx.query_closest(rays, reference_order=order)
        assert np.array_equal(q["hit"], ora["hit"]), order
        assert np.array_equal(q["rng_out"], ora["rng_out"]), order
        for f in ("front_face", "material"):
            assert np.array_equal(q[f][h], ora[f][h]), (order, f)
        for f in ("t", "p", "n"):
            bad = int((_bits(q[f][surf]) != _bits(ora[f][surf])).reshape(int(surf.sum()), -1).any(axis=1).sum())
            assert bad == 0, (order, f, bad)
            assert np.allclose(q[f][fog], ora[f][fog], rtol=1e-13, atol=1e-13), (order, f, "medium")
        occ, rng = ctx.query_occluded(rays, reference_order=order, return_rng=True)
        assert np.array_equal(occ, h) and np.array_equal(rng, ora["rng_out"]), order


def test_batch_shapes(ctx):
    ctx.upload(G.scene(21))
    rays = _rays(_gold(21)[:257])
    keep = rays.copy()
    whole = ctx.query_closest(rays)
    assert _same_bits(rays, keep)  # the input is not written
    split = np.concatenate([ctx.query_closest(rays[:64].copy()), ctx.query_closest(rays[64:].copy())])
    assert _same_bits(whole, split)
    for n in (0, 1, 63, 64, 65, 256, 257):
        out = np.zeros(n + 1, dtype=A.RAY_HIT_DTYPE)
        out.view(np.uint8)[:] = 0xA5  # sentinels
        got = ctx.query_closest(rays[:n].copy(), out=out)
        assert got is out and _same_bits(out[:n], whole[:n]), n
        assert (out[n:].view(np.uint8) == 0xA5).all(), n
        occ = np.full(n + 1, 0xA5, dtype=np.uint8)
        rng = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32)
        part = np.ascontiguousarray(rays[:n])
        ctx._chk(ctx._L.rtr_query_occluded(ctx._h, part.ctypes.data, occ.ctypes.data, rng.ctypes.data, n, 0))
        assert np.array_equal(occ[:n], whole["hit"][:n]) and occ[n] == 0xA5, n
        assert np.array_equal(rng[:n], whole["rng_out"][:n]) and rng[n] == 0xA5A5A5A5, n
    assert _same_bits(rays, keep)


def test_bad_rays(ctx):
    import torch
    ctx.upload(G.scene(21))
    rays = _rays(_gold(21)[:9])
    good = ctx.query_closest(rays)
    bad = rays.copy()
    bad["origin"][5, 1] = np.nan
    out = np.zeros(9, dtype=A.RAY_HIT_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    with pytest.raises(rtr.RtrError) as e:
        ctx.query_closest(bad, out=out)
    assert e.value.code == A.RTR_ERR_INVALID and "index 5" in e.value.message
    assert (out.view(np.uint8) == 0xA5).all()
    occ = np.full(9, 0xA5, dtype=np.uint8)
    assert ctx._L.rtr_query_occluded(ctx._h, bad.ctypes.data, occ.ctypes.data, None, 9, 0) == A.RTR_ERR_INVALID
    assert "index 5" in ctx._L.rtr_last_error(ctx._h).decode() and (occ == 0xA5).all()
    for field, value in (("direction", np.inf), ("time", np.nan), ("t_min", -np.inf), ("t_max", np.nan)):
        r = rays.copy()
        if r[field].ndim == 2:
            r[field][2, 0] = value
        else:
            r[field][2] = value
        with pytest.raises(rtr.RtrError) as e:
            ctx.query_closest(r)
        assert e.value.code == A.RTR_ERR_INVALID and "index 2" in e.value.message, field
    # the device entries cannot see the data: the kernel answers the bad lane with a miss and casts the others
    d_rays = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
    d_hits = torch.full((9 * A.RAY_HIT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    d_occ = torch.full((9,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), 9, blocking=True)
    ctx.query_occluded_into(d_rays.data_ptr(), d_occ.data_ptr(), 9, blocking=True)
    got = d_hits.cpu().numpy().view(A.RAY_HIT_DTYPE)
    miss = np.zeros(1, dtype=A.RAY_HIT_DTYPE)
    miss["material"], miss["rng_out"] = -1, bad["rng_state"][5]
    assert _same_bits(got[5:6], miss)
    ok = np.arange(9) != 5
    assert _same_bits(got[ok], good[ok])
    assert np.array_equal(d_occ.cpu().numpy(), np.where(ok, good["hit"], 0).astype(np.uint8))
    # a zero generator state matters only where the scene has media
    zero = rays.copy()
    zero["rng_state"][3] = 0
    z = ctx.query_closest(zero)
    assert z["rng_out"][3] == 0  # handed back as it came
    z["rng_out"][3] = good["rng_out"][3]
    assert _same_bits(z, good)
    ctx.upload(G.scene(9))
    z9 = _rays(_gold(9)[:9])
    z9["rng_state"][3] = 0
    with pytest.raises(rtr.RtrError) as e:
        ctx.query_closest(z9)
    assert e.value.code == A.RTR_ERR_INVALID and "index 3" in e.value.message


def test_device_entries_equal_the_host_entries_and_queue_behind_a_render(ctx):
    import torch
    for sid in (21, 9):
        ctx.upload(G.scene(sid))
        rays = _rays(_gold(sid))
        n = len(rays)
        host = ctx.query_closest(rays)
        h_occ, h_rng = ctx.query_occluded(rays, return_rng=True)
        W = H = 256
        p = A.make_params(W, H, 16, seed=3)
        want = ctx.render(p)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_hits = torch.zeros(n * A.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_occ = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        d_rng = torch.zeros(n, dtype=torch.int32, device="cuda")
        fb = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.render_into(p, fb.data_ptr(), W, blocking=False)
        ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), n, blocking=False)
        ctx.query_occluded_into(d_rays.data_ptr(), d_occ.data_ptr(), n, rng_out_ptr=d_rng.data_ptr(), blocking=False)
        ctx.synchronize()
        assert _same_bits(d_hits.cpu().numpy().view(A.RAY_HIT_DTYPE), host), sid
        assert np.array_equal(d_occ.cpu().numpy().astype(bool), h_occ), sid
        assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), h_rng), sid
        assert np.array_equal(_bits(fb.cpu().numpy()), _bits(want)), sid
        assert ctx.stats()["samples"] == W * H * 16  # the render's statistics survive the queries


def test_queries_do_not_interfere_with_renders_and_accumulators(ctx):
    ctx.upload(G.scene(21))
    rays = _rays(_gold(21))
    p = A.make_params(64, 64, 8, seed=11)
    a = ctx.render(p)
    q = ctx.query_closest(rays)
    b = ctx.render(p)
    assert np.array_equal(_bits(a), _bits(b))
    with ctx.accumulator(A.make_params(64, 64, 1, seed=11)) as acc:
        acc.render(8)
        assert _same_bits(ctx.query_closest(rays), q)
        assert np.array_equal(ctx.query_occluded(rays), q["hit"] == 1)
        acc.render(16)
        got = acc.resolve()
    want = ctx.render(A.make_params(64, 64, 16, seed=11, spp_chunks=1))
    assert np.array_equal(_bits(got), _bits(want))


def test_before_upload_and_unknown_flags():
    rays = _rays(_gold(21)[:4])
    with rtr.Context(0) as c:
        with pytest.raises(rtr.RtrError) as e:
            c.query_closest(rays)
        assert e.value.code == A.RTR_ERR_NO_SCENE
        with pytest.raises(rtr.RtrError) as e:
            c.query_occluded(rays)
        assert e.value.code == A.RTR_ERR_NO_SCENE
        c.upload(G.scene(21))
        hits = np.zeros(4, dtype=A.RAY_HIT_DTYPE)
        occ = np.zeros(4, dtype=np.uint8)
        L = c._L
        for flags in (2, 4, 8, 16, 1 | 32):
            assert L.rtr_query_closest(c._h, rays.ctypes.data, hits.ctypes.data, 4, flags) == A.RTR_ERR_INVALID
            assert L.rtr_query_occluded(c._h, rays.ctypes.data, occ.ctypes.data, None, 4, flags) == A.RTR_ERR_INVALID
            assert L.rtr_query_closest_device(c._h, rays.ctypes.data, hits.ctypes.data, 4, flags, 1) == A.RTR_ERR_INVALID
            assert L.rtr_query_occluded_device(c._h, rays.ctypes.data, occ.ctypes.data, None, 4, flags, 1) == A.RTR_ERR_INVALID
        assert L.rtr_query_closest(c._h, rays.ctypes.data, hits.ctypes.data, -1, 0) == A.RTR_ERR_INVALID
        assert L.rtr_query_closest(c._h, None, hits.ctypes.data, 4, 0) == A.RTR_ERR_INVALID
        assert L.rtr_query_closest(c._h, rays.ctypes.data, None, 4, 0) == A.RTR_ERR_INVALID
        assert L.rtr_query_occluded(c._h, rays.ctypes.data, None, None, 4, 0) == A.RTR_ERR_INVALID
        assert L.rtr_query_closest(c._h, rays.ctypes.data, hits.ctypes.data, 0, 0) == A.RTR_OK


def test_cli_pick_prints_the_query_of_the_pixel_centre_ray(ctx):
    cli = os.path.join(os.path.dirname(rtr.native.library_path()), "rtr_cli")
    r = subprocess.run([cli, "21", "4", "--pick", "32,32", "--width", "64"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    line = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(line) == 1, r.stdout.decode()
    ctx.upload(rtr.hostscene.build_scene(21))
    h = ctx.query_closest(ctx.camera_ray(A.make_params(64, 64, 1), 32, 32))[0]
    assert h["hit"] == 1
    want = "%d %d %d " % (h["hit"], h["front_face"], h["material"]) + " ".join(
        "%.17g" % x for x in [h["t"], *h["p"], *h["n"]])
    assert line[0].strip() == want
