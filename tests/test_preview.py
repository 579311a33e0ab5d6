"""Baked previews (include/rtr_hip.h: rtr_preview_*) on the GPU, bit for bit against the restatement of the contract
(tests/_preview_ref.py): the samples against rtr_query_closest over rtr_preview_ray rays + the scene description +
rtr_li_rays for the rays that miss, the frame against the reduction of the host shader (rtr_shade_ibl_one) over those
samples.  tests/test_preview_cpu.py holds the rays to numpy and shows that the inputs reach every branch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _cube_filter_ref as FR
import _golden as G
import _ibl_cases as IC
import _preview_ref as PR
import _temporal_ref as T

rtr = G.rtr
A = G.A
N = rtr.native

pytestmark = pytest.mark.gpu
INV = A.RTR_ERR_INVALID
SAMPLE = A.PREVIEW_SAMPLE_DTYPE
REC, ENTRY = 32, 16


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


def _upload(ctx, sid):
    if getattr(ctx, "_preview_sid", None) != sid or ctx.camera_updated:
        ctx.upload(G.scene(sid))
        ctx._preview_sid = sid
    return ctx.scene


_CASES = {}


def _case(ctx, sid, W, k, region=None, reference_order=False):
    """the samples of one call, made once: (params, the device's records [h, w, k^2] -- host and device entry agree --,
    the restated records, the mask of the fully restated ones)"""
    key = (sid, W, k, region, reference_order)
    sc = _upload(ctx, sid)
    if key in _CASES:
        return _CASES[key]
    import torch
    p = N.preview_params(W, W, k, region=region, reference_order=reference_order)
    rays = ctx.preview_rays(p)
    hits = ctx.query_closest(rays.reshape(-1), reference_order=reference_order)
    miss = rays.reshape(-1)[hits["hit"] == 0]
    direct = ctx.li_rays(A.make_params(W, W, 1, integrator=A.INTEGRATOR_MIS), miss["origin"], miss["direction"], miss["time"],
                         miss["rng_state"]) if len(miss) else None
    want, full = PR.samples_of(sc, rays, hits, direct)
    n = want.size
    buf = np.zeros(n + 1, dtype=SAMPLE)
    buf["kind"][n] = -7
    got = ctx.preview_samples(p, out=buf)
    assert buf["kind"][n] == -7 and not buf["direct"][n].any()
    d_out = _sentinel((n + 1) * SAMPLE.itemsize)
    torch.cuda.synchronize()
    ctx.preview_samples_into(p, d_out.data_ptr(), blocking=True)
    raw = d_out.cpu().numpy()
    assert (raw[n * SAMPLE.itemsize:] == 0xA5).all()
    assert _same_bits(raw[:n * SAMPLE.itemsize], got)
    _CASES[key] = (p, got.copy(), want, full)
    return _CASES[key]


# ---- 1. samples ----

def _assert_samples(got, want, full):
    for name in ("kind", "material"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("p", "n", "v"):
        assert _same_bits(got["q"][name], want["q"][name]), name
    assert _same_bits(got[full], want[full])
    rest = got[~full]  # a textured value: not restated, but of the right kind
    assert np.isfinite(rest["q"]["base"]).all() and np.isfinite(rest["direct"]).all()
    other = got[got["kind"] != PR.SURFACE]
    assert not any(np.ascontiguousarray(other["q"]).tobytes()) and not got["direct"][got["kind"] == PR.SURFACE].any()


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("sid", PR.SCENES)
def test_samples_equal_the_restatement(ctx, sid, k):
    """every field, scenes without textures: miss (background, environment map), emitter front and back, lambertian,
    metal, dielectric, PBR"""
    p, got, want, full = _case(ctx, sid, 32, k)
    assert full.all()
    _assert_samples(got, want, full)
    if k == 1:
        assert PR.counts_of(ctx.scene, got) == PR.COUNTS[sid]


@pytest.mark.parametrize("shape", ((32, 2, PR.RAGGED, False), (32, 2, (17, 9, 18, 10), False), (16, 8, None, False),
                                   (32, 2, None, True), (32, 1, PR.RAGGED, True)))
@pytest.mark.parametrize("sid", (21, 23))
def test_samples_of_regions_grids_and_the_reference_order(ctx, sid, shape):
    """a ragged region (blocks with idle lanes on every side), a 1 x 1 region, k = 8 (s up to 63) on 16 x 16, and the
    reference-order traversal"""
    W, k, region, ref = shape
    p, got, want, full = _case(ctx, sid, W, k, region, ref)
    _assert_samples(got, want, full)
    if region is not None and not ref:
        x0, y0, x1, y1 = region
        whole = _case(ctx, sid, W, k)[1]
        assert _same_bits(got, whole[y0:y1, x0:x1])


@pytest.mark.parametrize("sid", PR.TEXTURED)
def test_samples_of_textured_scenes(ctx, sid):
    """q.n is the query's normal (no normal map), kind and material agree; base is a texture's value"""
    p, got, want, full = _case(ctx, sid, 32, 1)
    assert not full.all()
    _assert_samples(got, want, full)
    assert (got["q"]["base"][~full & (got["kind"] == PR.SURFACE)] != 0).any()


# ---- 2. frame ----

def _host_env(got, parts, depth):
    surf = got["kind"] == PR.SURFACE
    env = PR.environment(got["q"]["p"][surf], depth)
    return env, IC.native_env(env, parts)


def _device_env(env, parts):
    held = {"table": IC.table_records(env["tab"])}
    if parts & 1:
        held["probes"] = env["probes"]
        if env["depth"] is not None:
            held["depth"] = env["depth"]
    if parts & 2:
        held["chain"] = env["records"]
    dev = {name: _dev(a) for name, a in held.items()}
    return IC.native_env(env, parts, {name: t.data_ptr() for name, t in dev.items()}), dev, held


def _frame_into(ctx, p, ne, stride, with_lit=True):
    """rtr_preview_device into buffers whose rows are `stride` pixels apart, sentinels everywhere else"""
    import torch
    h, w = p.y1 - p.y0, p.x1 - p.x0
    d_lin, d_lit = _sentinel((h * stride + 1) * 24), _sentinel((h * stride + 1) * 4)
    torch.cuda.synchronize()
    ctx.preview_into(p, ne, d_lin.data_ptr(), stride, d_lit.data_ptr() if with_lit else None, blocking=True)
    lin = d_lin.cpu().numpy().view(np.float64)[:h * stride * 3].reshape(h, stride, 3)
    lit = d_lit.cpu().numpy().view(np.int32)[:h * stride].reshape(h, stride)
    pad = np.frombuffer(b"\xa5" * 8, dtype=np.float64)[0]
    assert (d_lin.cpu().numpy()[h * stride * 24:] == 0xA5).all() and (d_lit.cpu().numpy()[h * stride * 4:] == 0xA5).all()
    assert _same_bits(lin[:, w:], np.full((h, stride - w, 3), pad))  # the row padding
    if with_lit:
        assert (lit[:, w:] == np.int32(-1515870811)).all()
    else:
        assert (d_lit.cpu().numpy() == 0xA5).all()
    return lin[:, :w], lit[:, :w]


@pytest.mark.parametrize("depth", (True, False))
@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("case", tuple((sid, 32, 2, None) for sid in PR.SCENES) + tuple((sid, 32, 1, None) for sid in PR.TEXTURED) +
                         ((21, 32, 2, PR.RAGGED), (23, 32, 1, (17, 9, 18, 10)), (23, 16, 8, None)))
def test_frame_equals_the_reduction_of_the_host_shader(ctx, case, parts, depth):
    sid, W, k, region = case
    p, got, _, _ = _case(ctx, sid, W, k, region)
    whole = _case(ctx, sid, W, k)[1] if region is not None else got
    _upload(ctx, sid)
    env, host = _host_env(whole, parts, depth)
    want_lin, want_lit = PR.frame_of(host, got)
    h, w = want_lit.shape
    # the host entry: a view with strided rows inside an array of sentinels
    big = np.full((h + 1, w + 3, 3), -7.0)
    lin, lit = ctx.preview(p, host, out=big[:h, :w], return_lit=True)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    assert (big[h:] == -7.0).all() and (big[:, w:] == -7.0).all()
    assert _same_bits(ctx.preview(p, host), want_lin)  # lit NULL, packed rows
    # the device entry
    ne, dev, held = _device_env(env, parts)
    lin, lit = _frame_into(ctx, p, ne, w + 5)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    assert _same_bits(_frame_into(ctx, p, ne, w, with_lit=False)[0], want_lin)
    for name, t in dev.items():
        assert _same_bits(t.cpu().numpy(), np.ascontiguousarray(held[name]).reshape(-1).view(np.uint8)), name
    surf = (got["kind"] == PR.SURFACE).sum(axis=2)
    assert (want_lit <= k * k).all() and (want_lit >= k * k - surf).all()
    if region is None and parts & 1:
        assert (want_lit < k * k).any() and (want_lit[surf == k * k] > 0).any()  # unlit and lit surface samples


# ---- 3. camera ----

def test_a_camera_update_is_an_upload_with_that_camera(ctx):
    sc = G.scene(23)
    cam = T.camera_dict(sc.camera)
    step = 0.03 * np.sqrt(cam["horizontal"] @ cam["horizontal"])
    cam2 = T.moved_camera(cam, translate=step * cam["u"] + 0.5 * step * cam["v"], yaw_deg=4.0)
    p = N.preview_params(32, 32, 2)
    before = _case(ctx, 23, 32, 2)[1]
    env, host = _host_env(before, 3, True)
    _upload(ctx, 23)
    ctx.set_camera(cam2)
    moved_s, moved = ctx.preview_samples(p), ctx.preview(p, host, return_lit=True)
    assert _same_bits(ctx.preview_rays(p), N.preview_rays(cam2, p))
    with rtr.Context(0) as other:
        other.upload(T.scene_with_camera(sc, cam2))
        assert _same_bits(other.preview_samples(p), moved_s)
        lin, lit = other.preview(p, host, return_lit=True)
    assert _same_bits(lin, moved[0]) and _same_bits(lit, moved[1])
    assert not _same_bits(moved_s, before)
    ctx.set_camera(sc.camera)
    assert _same_bits(ctx.preview_samples(p), before)


# ---- 4. stream order ----

CENTRE = (278.0, 400.0, 400.0)  # above the two boxes of the Cornell box of scene 21
LO, HI = (100.0, 100.0, 100.0), (450.0, 450.0, 450.0)


def test_bake_preview_and_display_in_stream_order(ctx):
    """capture_cube_into, two cube_filter_into levels, probe_radiance_into over a 2 x 2 x 2 grid, brdf_table_into,
    preview_into and display_into queued back to back without a wait, one synchronise at the end: the frame and the bytes
    equal the blocking entries fed the host copies of what the calls before them wrote"""
    import torch
    _upload(ctx, 21)
    prm = A.make_params(64, 64, 1, integrator=4)
    levels, n_records = FR.plan(8, 3)
    grid = rtr.ProbeGrid.in_box(LO, HI, (2, 2, 2))
    pts = N.probe_points(grid.positions())
    W = 32
    p = N.preview_params(W, W, 2)
    d_centre, d_pts = _dev(N.probe_points(np.array([CENTRE]))), _dev(pts)
    d_chain, d_sh, d_table = _sentinel((n_records + 1) * REC), _sentinel(9 * 224), _sentinel(13 * ENTRY)
    d_lin, d_lit, d_rgb = _sentinel((W * W + 1) * 24), _sentinel((W * W + 1) * 4), _sentinel(W * W * 3 + 1)
    torch.cuda.synchronize()
    base = d_chain.data_ptr()
    ne = N.shade_env(d_table.data_ptr(), grid=grid.grid(), probes=d_sh.data_ptr(), levels=levels, chain=base, n_records=n_records,
                     n_mu=4, n_rough=3)
    dp = N.display_defaults()
    ctx.capture_cube_into(prm, d_centre.data_ptr(), base, 1, face_size=8, samples=2, seed=7, blocking=False)
    for S, at, alpha in levels[1:]:
        ctx.cube_filter_into(base, base + at * REC, 1, face_in=8, face_out=S, alpha=alpha, blocking=False)
    ctx.probe_radiance_into(prm, d_pts.data_ptr(), d_sh.data_ptr(), 8, samples=16, seed=5, blocking=False)
    ctx.brdf_table_into(d_table.data_ptr(), 4, 3, 16, blocking=False)
    ctx.preview_into(p, ne, d_lin.data_ptr(), W, d_lit.data_ptr(), blocking=False)
    ctx.display_into(d_lin.data_ptr(), W, W, W, d_rgb.data_ptr(), dp, blocking=False)
    ctx.synchronize()
    chain = d_chain.cpu().numpy()[:n_records * REC].view(A.GATHER_OUT_DTYPE)
    sh = d_sh.cpu().numpy()[:8 * 224].view(A.PROBE_SH_DTYPE)
    table = d_table.cpu().numpy()[:12 * ENTRY].view(A.BRDF_ENTRY_DTYPE).reshape(3, 4)
    for t, n in ((d_chain, n_records * REC), (d_sh, 8 * 224), (d_table, 12 * ENTRY), (d_lin, W * W * 24), (d_lit, W * W * 4),
                 (d_rgb, W * W * 3)):
        assert (t.cpu().numpy()[n:] == 0xA5).all()
    assert _same_bits(table, ctx.brdf_table(4, 3, 16)) and _same_bits(sh, ctx.probe_radiance(prm, pts, samples=16, seed=5))
    host = N.shade_env(table, grid=grid.grid(), probes=sh, levels=levels, chain=chain)
    lin = d_lin.cpu().numpy()[:W * W * 24].view(np.float64).reshape(W, W, 3)
    lit = d_lit.cpu().numpy()[:W * W * 4].view(np.int32).reshape(W, W)
    want_lin, want_lit = ctx.preview(p, host, return_lit=True)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    assert _same_bits(d_rgb.cpu().numpy()[:W * W * 3].reshape(W, W, 3), ctx.display(want_lin, dp)[0])
    assert (lit > 0).any() and (lin != 0).any()


# ---- 5. checks ----

def test_entries_check_their_arguments(ctx):
    import torch
    _upload(ctx, 21)
    L, h = ctx._L, ctx._h
    good = lambda: N.preview_params(8, 6, 2)  # noqa: E731
    got = _case(ctx, 21, 32, 1)[1]
    env, host = _host_env(got, 3, True)
    ne, dev, held = _device_env(env, 3)
    n = 8 * 6 * 4
    s_out, lin, lit = np.zeros(n, dtype=SAMPLE), np.zeros((6, 8, 3)), np.zeros((6, 8), dtype=np.int32)
    d_s, d_lin, d_lit = _sentinel(n * 144), _sentinel(6 * 8 * 24), _sentinel(6 * 8 * 4)
    torch.cuda.synchronize()
    sp, lp, tp = C.c_void_p(d_s.data_ptr()), C.c_void_p(d_lin.data_ptr()), C.c_void_p(d_lit.data_ptr())

    def every(p, want, env_h=host, env_d=ne, stride=8):
        pp = C.byref(p) if p is not None else None
        eh, ed = (C.byref(env_h) if env_h is not None else None), (C.byref(env_d) if env_d is not None else None)
        assert L.rtr_preview_samples(h, pp, s_out.ctypes.data) == want
        assert L.rtr_preview_samples_device(h, pp, sp, 1) == want
        assert L.rtr_preview(h, pp, eh, lin.ctypes.data, stride, lit.ctypes.data) == want
        assert L.rtr_preview_device(h, pp, ed, lp, stride, tp, 1) == want

    every(None, INV)
    for kw in (dict(image_width=1), dict(image_height=1), dict(x1=0), dict(x0=-1), dict(y1=7), dict(x1=9), dict(y0=6), dict(x0=8),
               dict(grid=0), dict(grid=9), dict(flags=2), dict(flags=5), dict(t_min=np.nan), dict(t_min=np.inf), dict(t_min=-np.inf),
               dict(t_min=2.0 ** -101), dict(t_min=0.0)):
        p = good()
        for name, value in kw.items():
            setattr(p, name, value)
        every(p, INV)
    for r in range(3):
        p = good()
        p.reserved[r] = 0.5
        every(p, INV)
    p = good()
    pp = C.byref(p)
    assert L.rtr_preview_samples(h, pp, None) == INV and L.rtr_preview_samples_device(h, pp, None, 1) == INV
    assert L.rtr_preview(h, pp, C.byref(host), None, 8, None) == INV and L.rtr_preview_device(h, pp, C.byref(ne), None, 8, None, 1) == INV
    assert L.rtr_preview(h, pp, None, lin.ctypes.data, 8, None) == INV and L.rtr_preview_device(h, pp, None, lp, 8, None, 1) == INV
    assert L.rtr_preview(h, pp, C.byref(host), lin.ctypes.data, 7, None) == INV  # row_stride below the width
    assert L.rtr_preview_device(h, pp, C.byref(ne), lp, 7, tp, 1) == INV
    # the environment: the rules of rtr_shade_ibl
    for parts in (0, 4):
        bad_h, bad_d = IC.native_env(env, 3), IC.native_env(env, 3, {k: t.data_ptr() for k, t in dev.items()})
        bad_h.parts = bad_d.parts = parts
        assert L.rtr_preview(h, pp, C.byref(bad_h), lin.ctypes.data, 8, None) == INV
        assert L.rtr_preview_device(h, pp, C.byref(bad_d), lp, 8, tp, 1) == INV
    for member in ("grid", "probes", "levels", "chain", "table", "depth"):
        bad_h, bad_d = IC.native_env(env, 3), IC.native_env(env, 3, {k: t.data_ptr() for k, t in dev.items()})
        setattr(bad_h, member, None)
        setattr(bad_d, member, None)
        assert L.rtr_preview(h, pp, C.byref(bad_h), lin.ctypes.data, 8, None) == INV, member
        assert L.rtr_preview_device(h, pp, C.byref(bad_d), lp, 8, tp, 1) == INV, member
    # device pointers: alignment and overlap
    assert L.rtr_preview_samples_device(h, pp, C.c_void_p(d_s.data_ptr() + 4), 1) == INV
    assert L.rtr_preview_device(h, pp, C.byref(ne), C.c_void_p(d_lin.data_ptr() + 4), 8, tp, 1) == INV
    assert L.rtr_preview_device(h, pp, C.byref(ne), lp, 8, C.c_void_p(d_lit.data_ptr() + 2), 1) == INV
    odd = IC.native_env(env, 3, dict({k: t.data_ptr() for k, t in dev.items()}, chain=dev["chain"].data_ptr() + 4))
    assert L.rtr_preview_device(h, pp, C.byref(odd), lp, 8, tp, 1) == INV
    assert L.rtr_preview_device(h, pp, C.byref(ne), C.c_void_p(dev["chain"].data_ptr()), 8, tp, 1) == INV  # linear over the chain
    assert L.rtr_preview_device(h, pp, C.byref(ne), lp, 8, C.c_void_p(dev["table"].data_ptr() + 16), 1) == INV  # lit in the table
    assert L.rtr_preview_device(h, pp, C.byref(ne), C.c_void_p(dev["probes"].data_ptr() - 8), 8, None, 1) == INV  # ... reaches the probes
    assert L.rtr_preview_device(h, pp, C.byref(ne), lp, 8, lp, 1) == INV  # lit over linear
    # nothing was written
    assert not s_out.view(np.uint8).any() and not lin.any() and not lit.any()
    for t in (d_s, d_lin, d_lit):
        assert (t.cpu().numpy() == 0xA5).all()
    for name, t in dev.items():
        assert _same_bits(t.cpu().numpy(), np.ascontiguousarray(held[name]).reshape(-1).view(np.uint8)), name
    # and the good call goes through
    assert L.rtr_preview_device(h, pp, C.byref(ne), lp, 8, tp, 1) == 0 and L.rtr_preview_samples_device(h, pp, sp, 1) == 0
    with pytest.raises(rtr.RtrError) as e:
        ctx.preview(N.preview_params(8, 6, 9), host)
    assert e.value.code == INV and "grid" in str(e.value)


def test_media_and_a_missing_scene(ctx):
    p = N.preview_params(8, 6, 1)
    got = _case(ctx, 21, 32, 1)[1]
    env, host = _host_env(got, 3, False)
    s_out, lin = np.zeros(48, dtype=SAMPLE), np.zeros((6, 8, 3))
    with rtr.Context(0) as fresh:
        L, h = fresh._L, fresh._h
        assert L.rtr_preview_samples(h, C.byref(p), s_out.ctypes.data) == A.RTR_ERR_NO_SCENE
        assert L.rtr_preview(h, C.byref(p), C.byref(host), lin.ctypes.data, 8, None) == A.RTR_ERR_NO_SCENE
        bad = N.preview_params(8, 6, 0)
        assert L.rtr_preview_samples(h, C.byref(bad), s_out.ctypes.data) == INV  # the params come first
        fresh.upload(G.scene(9))
        assert L.rtr_preview_samples(h, C.byref(p), s_out.ctypes.data) == A.RTR_ERR_UNSUPPORTED
        assert L.rtr_preview(h, C.byref(p), C.byref(host), lin.ctypes.data, 8, None) == A.RTR_ERR_UNSUPPORTED
        with pytest.raises(rtr.RtrError) as e:
            fresh.preview_samples(p)
        assert e.value.code == A.RTR_ERR_UNSUPPORTED and "media" in str(e.value)
    assert not s_out.view(np.uint8).any() and not lin.any()


# ---- 6. upper layers ----

def _ibl(env):
    grid = rtr.ProbeGrid(env["origin"], env["spacing"], env["dims"], env["probes"])
    grid.depth = env["depth"]
    return rtr.IblEnvironment(grid, rtr.CubeChain(N.cube_levels(env["levels"]), env["records"]),
                              rtr.BrdfTable(IC.table_records(env["tab"])), normal_bias=env["normal_bias"])


@pytest.mark.parametrize("depth", (True, False))
def test_python_faces(ctx, depth):
    p, got, _, _ = _case(ctx, 23, 32, 2)
    env, host = _host_env(got, 3, depth)
    want_lin, want_lit = PR.frame_of(host, got)
    ibl = _ibl(env)
    lin, lit = ibl.render(ctx, p, return_lit=True)
    assert _same_bits(lin, want_lin) and _same_bits(lit, want_lit)
    r = rtr.Renderer(context=ctx)
    buf = rtr.RenderBuffer(32, 32)
    assert r.render_preview(ctx.scene, ibl, buf, grid=2) is buf
    assert _same_bits(buf.linear, want_lin)
    dp = N.display_defaults()
    shown = rtr.RenderBuffer(32, 32)
    r.render_preview(ctx.scene, ibl, shown, grid=2, display=dp)
    assert _same_bits(shown.linear, want_lin)
    assert _same_bits(shown.display_rgb8, ctx.display(want_lin, dp)[0])
    with pytest.raises(ValueError):
        r.render_preview(ctx.scene, ibl, shown, display=3)


def test_the_command_line_writes_the_python_path_s_pixels(ctx, tmp_path):
    """rtr_cli --preview 2 with --probes, --probe-depth, --capture --capture-levels and --brdf-table bakes the three parts
    and writes the frame the Python route makes of the same bake"""
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    out = str(tmp_path / "preview.ppm")
    box = "100,100,100,450,450,450"
    bake = ["--probes", "2,2,2", "--probe-box", box, "--probe-samples", "16", "--probe-depth", "4", "--capture", "278,400,400",
            "--face", "8", "--capture-spp", "2", "--capture-levels", "3", "--brdf-table", "4,3", "--brdf-nodes", "16"]
    r = subprocess.run([cli, "21", "4", "--width", "32", "--seed", "7", "--preview", "2", "--out", out] + bake,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    sc = rtr.hostscene.build_scene(21)
    ctx.upload(sc)
    ctx._preview_sid = None
    prm = A.make_params(2, 2, 1, integrator=4, seed=7)
    grid = rtr.ProbeGrid.in_box((100.0,) * 3, (450.0,) * 3, (2, 2, 2))
    grid.bake(ctx, prm, samples=16, seed=7, depth=4)
    cube = rtr.Cubemap(ctx.capture_cube_records(prm, np.array([CENTRE]), face_size=8, samples=2, seed=7)[0])
    ibl = rtr.IblEnvironment(grid, cube.prefilter(levels=3, ctx=ctx), rtr.BrdfTable.make(4, 3, 16, ctx=ctx))
    buf = rtr.RenderBuffer(32, 32)
    rtr.Renderer(context=ctx).render_preview(sc, ibl, buf, grid=2)
    assert (buf.linear != 0).any()
    data = open(out, "rb").read()
    assert data[-32 * 32 * 3:] == buf.to_rgb8().tobytes()
    # a missing part: the grid (its companions go with it), the centre, the chain's levels, the table
    for first, count in ((0, 8), (8, 2), (14, 2), (16, 4)):
        args = bake[:first] + bake[first + count:]
        r = subprocess.run([cli, "21", "4", "--width", "32", "--preview", "2", "--out", out] + args, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2 and b"--preview needs" in r.stderr, bake[first]
    for extra in (["--pick", "1,1"], ["--ao", "8"], ["--adaptive", "0.01"], ["--turntable", "2"], ["--preview", "9"]):
        r = subprocess.run([cli, "21", "4", "--width", "32", "--preview", "2", "--out", out] + bake + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, extra
