"""The host entries of the queries, gathers and probes across a slice boundary (csrc/rt_batch.h: staged_slices).  A host
entry sends its records through one staging buffer in slices of 2^20 points or 2^22 rays; every batch here is one slice and
65 records, one batch per record shape: 48-byte points to 32-byte results (gather), 24-byte points to 80-byte records
(probe visibility), the lookup with its grid kept at the head of the buffer, and rays to two output streams (occlusion
and generator states).  The references are routes that do not slice: the device entry over the same array in one call, the
host entry called once per slice with its own ``point_base``, and for rays, whose answer does not depend on the position
in the batch, the answer of the 4 096 rays the batch repeats.  All on scene 21: no media, so a record's answer depends on
its position only through ``point_base``.  The last test holds the record check in front of the staging: a bad last record
fails the call before anything is copied."""
import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _probe_ref as PR

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SEED = 7
POINT_SLICE = 1 << 20  # kGatherSlice, kProbeSlice
RAY_SLICE = 1 << 22    # kQuerySlice
OVER = 65
T_MAX = 150.0  # of the gathers and probes: open and blocked samples both occur among the points


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    c.upload(G.scene(21))
    yield c
    c.close()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _sentinel_out(n, dtype, extra=3):
    out = np.zeros(n + extra, dtype=dtype)
    out.view(np.uint8)[:] = 0xA5
    return out


def _device_route(records, out_dtype, call):
    """``call(points pointer, out pointer, n)`` over a torch upload of ``records``: the ``out_dtype`` records it wrote, with
    the bytes behind them checked"""
    import torch
    n = len(records)
    d_in = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    d_out = torch.full(((n + 1) * out_dtype.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(d_in.data_ptr(), d_out.data_ptr(), n)
    raw = d_out.cpu().numpy()
    assert (raw[n * out_dtype.itemsize:] == 0xA5).all()
    return raw[:n * out_dtype.itemsize].view(out_dtype)


def test_gather_occlusion_across_a_slice(ctx):
    n = POINT_SLICE + OVER
    p, nrm = GR.golden_points(21)
    pts = np.resize(rtr.native.gather_points(p, nrm), n)
    out = _sentinel_out(n, A.GATHER_OUT_DTYPE)
    got = ctx.gather_occlusion(pts, samples=1, seed=SEED, t_max=T_MAX, out=out)
    assert got is out and (out[n:].view(np.uint8) == 0xA5).all()
    assert (out["valid"][:n] == 1).all()
    dev = _device_route(pts, A.GATHER_OUT_DTYPE,
                        lambda i, o, m: ctx.gather_occlusion_into(i, o, m, samples=1, seed=SEED, t_max=T_MAX, blocking=True))
    assert _same_bits(out[:n], dev)
    head = ctx.gather_occlusion(pts[:POINT_SLICE], samples=1, seed=SEED, t_max=T_MAX)
    tail = ctx.gather_occlusion(pts[POINT_SLICE:], samples=1, seed=SEED, t_max=T_MAX, point_base=POINT_SLICE)
    assert _same_bits(out[:POINT_SLICE], head) and _same_bits(out[POINT_SLICE:n], tail)
    # the tail is not the answer of the same points at the head of a call: point_base reached the second slice
    assert not _same_bits(tail, ctx.gather_occlusion(pts[POINT_SLICE:], samples=1, seed=SEED, t_max=T_MAX))


def test_probe_visibility_across_a_slice(ctx):
    n = POINT_SLICE + OVER
    pts = np.resize(rtr.native.probe_points(PR.displaced_points(21, 5.0)), n)
    assert A.PROBE_VIS_DTYPE.itemsize == 80
    out = _sentinel_out(n, A.PROBE_VIS_DTYPE)
    got = ctx.probe_visibility(pts, samples=1, seed=SEED, t_max=T_MAX, out=out)
    assert got is out and (out[n:].view(np.uint8) == 0xA5).all()
    assert (out["valid"][:n] == 1).all()
    dev = _device_route(pts, A.PROBE_VIS_DTYPE,
                        lambda i, o, m: ctx.probe_visibility_into(i, o, m, samples=1, seed=SEED, t_max=T_MAX, blocking=True))
    assert _same_bits(out[:n], dev)
    head = ctx.probe_visibility(pts[:POINT_SLICE], samples=1, seed=SEED, t_max=T_MAX)
    tail = ctx.probe_visibility(pts[POINT_SLICE:], samples=1, seed=SEED, t_max=T_MAX, point_base=POINT_SLICE)
    assert _same_bits(out[:POINT_SLICE], head) and _same_bits(out[POINT_SLICE:n], tail)
    assert not _same_bits(tail, ctx.probe_visibility(pts[POINT_SLICE:], samples=1, seed=SEED, t_max=T_MAX))


def test_probe_lookup_across_a_slice(ctx):
    import torch
    n = POINT_SLICE + OVER
    rng = np.random.default_rng(5)
    origin, spacing, dims = (-1.0, 0.5, 2.0), (0.5, 1.25, 2.0), (2, 2, 2)
    grid = rtr.native.probe_grid(origin, spacing, dims)
    probes = np.zeros(8, dtype=A.PROBE_SH_DTYPE)
    probes["c"] = rng.standard_normal((8, 9, 3))
    probes["count"], probes["valid"] = 64, 1
    # in and around the grid's box, every query its own position and normal
    q = rtr.native.gather_points(np.asarray(origin) + (rng.random((n, 3)) * 2.0 - 0.5) * np.asarray(spacing),
                                 rng.standard_normal((n, 3)))
    out = _sentinel_out(n, A.GATHER_OUT_DTYPE)
    got = ctx.probe_lookup(grid, probes, q, out=out)
    assert got is out and (out[n:].view(np.uint8) == 0xA5).all()
    assert (out["valid"][:n] == 1).all()
    d_probes = torch.from_numpy(probes.view(np.uint8).copy()).cuda()
    dev = _device_route(q, A.GATHER_OUT_DTYPE,
                        lambda i, o, m: ctx.probe_lookup_into(grid, d_probes.data_ptr(), i, o, m, blocking=True))
    assert _same_bits(out[:n], dev)
    # the first and the last records against the host form of the contract
    for part in (slice(0, 64), slice(n - OVER, n)):
        assert _same_bits(out[part], rtr.native.probe_lookup_host(grid, probes, q[part]))


def test_query_occluded_across_a_slice(ctx):
    """two output streams of different record sizes for one input stream; then query_closest over the same rays"""
    n = RAY_SLICE + OVER
    prm = A.make_params(64, 64, 1)
    rays = np.concatenate([ctx.camera_ray(prm, i, j) for j in range(64) for i in range(64)])
    assert len(rays) == 4096
    # every ray its own generator state, which a scene without media hands back, and every third one too short to hit
    rays["rng_state"] = 1 + np.arange(4096, dtype=np.uint32)
    rays["t_max"][::3] = 1.0
    occ, rng = ctx.query_occluded(rays, return_rng=True)
    assert occ.any() and not occ.all() and len(np.unique(rng)) == 4096
    big = np.resize(rays, n)
    want_occ, want_rng = np.resize(occ, n), np.resize(rng, n)
    # 2^22 is a multiple of 4 096: the second slice gets other rays than the head of the batch
    big[RAY_SLICE:] = rays[1000:1000 + OVER]
    want_occ[RAY_SLICE:], want_rng[RAY_SLICE:] = occ[1000:1000 + OVER], rng[1000:1000 + OVER]
    got_occ, got_rng = ctx.query_occluded(big, return_rng=True)
    assert len(got_occ) == n and np.array_equal(got_occ, want_occ)
    assert np.array_equal(got_rng, want_rng)
    # rng_out = NULL: the second stream is not copied back, the first one is the same
    assert np.array_equal(ctx.query_occluded(big), got_occ)
    del got_occ, got_rng
    hits = ctx.query_closest(rays)
    assert np.array_equal(hits["hit"].astype(bool), occ)
    want = np.resize(hits, n)
    want[RAY_SLICE:] = hits[1000:1000 + OVER]
    out = _sentinel_out(n, A.RAY_HIT_DTYPE)
    assert ctx.query_closest(big, out=out) is out and (out[n:].view(np.uint8) == 0xA5).all()
    assert _same_bits(out[:n], want)


def test_a_bad_last_record_fails_before_anything_is_copied(ctx):
    n = 70000
    p, nrm = GR.golden_points(21)
    pts = np.resize(rtr.native.gather_points(p, nrm), n)
    pts["n"][n - 1] = 0.0
    out = _sentinel_out(n, A.GATHER_OUT_DTYPE, extra=0)
    with pytest.raises(rtr.RtrError) as e:
        ctx.gather_radiance(A.make_params(64, 64, 1), pts, samples=1, seed=SEED, out=out)
    assert e.value.code == A.RTR_ERR_INVALID and "index 69999" in e.value.message
    assert (out.view(np.uint8) == 0xA5).all()
