"""The chunked launcher of the batch units (csrc/rt_batch.h: launch_records) across a launch boundary.  A call is cut into
launches of at most 2^24 records, which no test reaches; RTR_LAUNCH_RECORDS=n, read at every call, lowers that cap, so the
per-launch steps -- the pointer offsets, the ``point_base`` carry of the gathers and probes, the texel numbering of the
captures and distance maps -- run here at sizes that take a second.  Every entry that goes through the launcher is computed
with the hook unset, by its host form and by its ``_into`` form over torch buffers, and must give the same bytes, with the
0xA5 sentinel behind its output untouched, under every cap:

  point families   150 records, samples = 4: groups of 4 lanes, so a launch of 70 records ends inside a wave; caps 64, 70, 1
  captures         3 centres of face_size 3, 162 texels, samples = 2; cap 40 cuts inside a face, cap 54 on a centre boundary
  distance maps    5 probes of map_size 4, 80 texels, samples = 2; caps 27 and 16
  lookups, shader  200 queries over a 2 x 2 x 2 grid, an 8 -> 4 -> 2 chain and a 5 x 3 table; caps 64 and 1

All on scene 21.  The lookups and the shader are held to the host form of their contract as well.  That a cap took effect
shows in the number of launches the context counted for its last call (rtr_debug_last_launches of csrc/rt_debug.h, the seam
of the test library in the product): ceil(records / cap) under a cap, 1 without one and under a value that is no cap."""
import ctypes as C

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _ibl_cases as IC
import _probe_ref as PR

A = G.A
rtr = G.rtr
N = rtr.native

pytestmark = pytest.mark.gpu

HOOK = "RTR_LAUNCH_RECORDS"
SEED = 7
T_MAX = 150.0  # of the occlusion gathers and visibility probes: open and blocked samples both occur among the points
N_POINTS, POINT_CAPS = 150, (64, 70, 1)
N_QUERIES, QUERY_CAPS = 200, (64, 1)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    c.upload(G.scene(21))
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _launches(ctx):
    f = N.lib().rtr_debug_last_launches
    f.argtypes, f.restype = [C.c_void_p], C.c_int64
    return f(ctx._h)


class Case:
    """One entry: ``host(out)`` writes ``n`` records of ``dtype`` into the numpy array ``out``, ``into(out_ptr)`` the same
    records at a device pointer (its inputs are torch uploads the case keeps alive)."""

    def __init__(self, ctx, dtype, n, host, into, keep=()):
        self.ctx, self.dtype, self.n, self.host, self.into, self.keep = ctx, dtype, n, host, into, keep

    def run(self, cap=None):
        """the bytes of the n records, which both forms agree on; the sentinel behind them stays in both, and each form's
        call made the launches of ``cap`` records (None: one launch)"""
        want = 1 if cap is None else -(-self.n // cap)
        import torch
        n, size = self.n, self.dtype.itemsize
        out = np.zeros(n + 3, dtype=self.dtype)
        out.view(np.uint8)[:] = 0xA5
        self.host(out)
        assert _launches(self.ctx) == want
        assert (out[n:].view(np.uint8) == 0xA5).all()
        d_out = torch.full(((n + 1) * size,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.into(d_out.data_ptr())
        assert _launches(self.ctx) == want
        raw = d_out.cpu().numpy()
        assert (raw[n * size:] == 0xA5).all()
        host = out[:n].tobytes()
        assert raw[:n * size].tobytes() == host
        return host


def _same_under_every_cap(monkeypatch, case, caps, record=None):
    """the uncapped bytes; every cap, and the values that are no cap, give the same.  ``record()``: the kernel record of the
    family's last launch, which a value that is no cap leaves as the uncapped call left it"""
    monkeypatch.delenv(HOOK, raising=False)
    whole = case.run()
    kernel = record() if record else None
    for cap in caps:
        monkeypatch.setenv(HOOK, str(cap))
        assert case.run(cap) == whole, cap
    for ignored in (str(1 << 24), str(1 << 30), "-5"):
        monkeypatch.setenv(HOOK, ignored)
        assert case.run() == whole, ignored
        if record:
            assert record() == kernel and kernel is not None, ignored
    monkeypatch.delenv(HOOK)
    return whole


# ---- gathers and probes ----

def _li_params():
    return A.make_params(64, 64, 1, integrator=4)


def _point_entries(ctx):
    """name -> (points, output dtype, host(points, out, point_base), into(points_ptr, out_ptr, n, point_base), record)"""
    p, nrm = GR.golden_points(21)
    gpts = np.resize(N.gather_points(p, nrm), N_POINTS)
    ppts = np.resize(N.probe_points(PR.displaced_points(21, 5.0)), N_POINTS)
    prm = _li_params()
    any_kw = dict(samples=4, seed=SEED, t_max=T_MAX)
    li_kw = dict(samples=4, seed=SEED)
    return {
        "gather_occlusion": (gpts, A.GATHER_OUT_DTYPE,
                             lambda pts, out, base: ctx.gather_occlusion(pts, out=out, point_base=base, **any_kw),
                             lambda i, o, n, base: ctx.gather_occlusion_into(i, o, n, blocking=True, point_base=base, **any_kw),
                             ctx.last_gather),
        "gather_radiance": (gpts, A.GATHER_OUT_DTYPE,
                            lambda pts, out, base: ctx.gather_radiance(prm, pts, out=out, point_base=base, **li_kw),
                            lambda i, o, n, base: ctx.gather_radiance_into(prm, i, o, n, blocking=True, point_base=base, **li_kw),
                            ctx.last_gather),
        "probe_visibility": (ppts, A.PROBE_VIS_DTYPE,
                             lambda pts, out, base: ctx.probe_visibility(pts, out=out, point_base=base, **any_kw),
                             lambda i, o, n, base: ctx.probe_visibility_into(i, o, n, blocking=True, point_base=base, **any_kw),
                             ctx.last_probe),
        "probe_radiance": (ppts, A.PROBE_SH_DTYPE,
                           lambda pts, out, base: ctx.probe_radiance(prm, pts, out=out, point_base=base, **li_kw),
                           lambda i, o, n, base: ctx.probe_radiance_into(prm, i, o, n, blocking=True, point_base=base, **li_kw),
                           ctx.last_probe),
    }


def _point_case(ctx, entry, first=0, base=0):
    pts, dtype, host, into, _ = entry
    pts = pts[first:]
    d_pts = _dev(pts)
    return Case(ctx, dtype, len(pts), lambda out: host(pts, out, base), lambda o: into(d_pts.data_ptr(), o, len(pts), base), (d_pts,))


@pytest.mark.parametrize("name", ("gather_occlusion", "gather_radiance", "probe_visibility", "probe_radiance"))
def test_point_families(ctx, monkeypatch, name):
    entry = _point_entries(ctx)[name]
    size = entry[1].itemsize
    whole = _same_under_every_cap(monkeypatch, _point_case(ctx, entry), POINT_CAPS, record=entry[4])
    assert np.frombuffer(whole, dtype=entry[1])["valid"].all()
    assert entry[4]()["lg"] == 2  # groups of 4 lanes: 70 records end in lane 24 of a wave
    # the second launch under cap 70 serves the points 70 .. 149 at their numbers under the seed: those records are a call
    # of their own on these points with point_base = 70 ...
    tail = _point_case(ctx, entry, first=70, base=70).run()
    assert whole[70 * size:] == tail
    # ... and not the same call at point_base = 0: the numbers matter, so point_base reached the second launch
    assert _point_case(ctx, entry, first=70, base=0).run() != tail


# ---- captures and distance maps: a record is a texel ----

def test_capture_cube(ctx, monkeypatch):
    pts = N.probe_points(PR.displaced_points(21, 5.0, 3))
    d_pts = _dev(pts)
    prm = _li_params()
    kw = dict(face_size=3, samples=2, seed=SEED)
    case = Case(ctx, A.GATHER_OUT_DTYPE, 3 * 54, lambda out: ctx.capture_cube_records(prm, pts, out=out, **kw),
                lambda o: ctx.capture_cube_into(prm, d_pts.data_ptr(), o, 3, blocking=True, **kw))
    whole = np.frombuffer(_same_under_every_cap(monkeypatch, case, (40, 54), record=ctx.last_capture), dtype=A.GATHER_OUT_DTYPE)
    assert whole["valid"].all()
    # the three captures differ: a launch that numbered its texels from 0 again would repeat the first centre
    faces = whole.reshape(3, 54)
    assert faces[0].tobytes() != faces[1].tobytes() and faces[1].tobytes() != faces[2].tobytes()


def test_probe_depth(ctx, monkeypatch):
    pts = N.probe_points(PR.displaced_points(21, 5.0, 5))
    d_pts = _dev(pts)
    kw = dict(map_size=4, samples=2, seed=SEED, t_max=250.0)
    case = Case(ctx, A.PROBE_DEPTH_DTYPE, 5 * 16, lambda out: ctx.probe_depth(pts, out=out, **kw),
                lambda o: ctx.probe_depth_into(d_pts.data_ptr(), o, 5, blocking=True, **kw))
    whole = np.frombuffer(_same_under_every_cap(monkeypatch, case, (27, 16), record=ctx.last_probe_depth), dtype=A.PROBE_DEPTH_DTYPE)
    assert whole["valid"].all()
    maps = whole.reshape(5, 16)
    assert len({m.tobytes() for m in maps}) == 5


# ---- the lookups and the shader: one lane per query ----

@pytest.fixture(scope="module")
def env():
    """a 2 x 2 x 2 grid with 4 x 4 distance maps, an 8 -> 4 -> 2 chain, a table of n_mu = 5 by n_rough = 3"""
    return IC.environment((2, 2, 2), (8, 3), (3, 5), 4)


def _lookup_cases(ctx, env):
    """name -> (Case, the host form of the contract over the same queries)"""
    grid = N.probe_grid(env["origin"], env["spacing"], env["dims"])
    vp = N.probe_visible_params(4, env["normal_bias"])
    sq = IC.queries(env, N_QUERIES)
    gq = N.gather_points(sq["p"], sq["n"])
    rng = np.random.default_rng(5)
    dirs = N.probe_points(rng.standard_normal((N_QUERIES, 3)))
    cq = N.cube_queries(dirs["p"], rng.uniform(0.0, 1.0, N_QUERIES))
    cube = env["records"][:6 * 8 * 8]  # level 0 of the chain is a capture of face size 8
    dev = {name: _dev(a) for name, a in dict(probes=env["probes"], depth=env["depth"], chain=env["records"],
                                             table=IC.table_records(env["tab"]), gq=gq, dirs=dirs, cq=cq, sq=sq).items()}
    ptr = {name: t.data_ptr() for name, t in dev.items()}
    host_env = IC.native_env(env, 3)
    dev_env = IC.native_env(env, 3, ptr)
    R = A.GATHER_OUT_DTYPE
    return {
        "probe_lookup": (Case(ctx, R, N_QUERIES, lambda out: ctx.probe_lookup(grid, env["probes"], gq, out=out),
                              lambda o: ctx.probe_lookup_into(grid, ptr["probes"], ptr["gq"], o, N_QUERIES, blocking=True), dev),
                         lambda: N.probe_lookup_host(grid, env["probes"], gq)),
        "probe_lookup_visible": (Case(ctx, R, N_QUERIES,
                                      lambda out: ctx.probe_lookup_visible(grid, env["probes"], env["depth"], gq, params=vp, out=out),
                                      lambda o: ctx.probe_lookup_visible_into(grid, ptr["probes"], ptr["depth"], vp, ptr["gq"], o,
                                                                              N_QUERIES, blocking=True), dev),
                                 lambda: N.probe_lookup_visible_host(grid, env["probes"], env["depth"], gq, params=vp)),
        "cube_lookup": (Case(ctx, R, N_QUERIES, lambda out: ctx.cube_lookup(cube, dirs, face_size=8, out=out),
                             lambda o: ctx.cube_lookup_into(8, ptr["chain"], ptr["dirs"], o, N_QUERIES, blocking=True), dev),
                        lambda: N.cube_lookup_host(cube, dirs, face_size=8)),
        "cube_chain_lookup": (Case(ctx, R, N_QUERIES, lambda out: ctx.cube_chain_lookup(env["levels"], env["records"], cq, out=out),
                                   lambda o: ctx.cube_chain_lookup_into(env["levels"], ptr["chain"], len(env["records"]), ptr["cq"], o,
                                                                        N_QUERIES, blocking=True), dev),
                              lambda: N.cube_chain_lookup_host(env["levels"], env["records"], cq)),
        "shade_ibl": (Case(ctx, R, N_QUERIES, lambda out: ctx.shade_ibl(host_env, sq, out=out),
                           lambda o: ctx.shade_ibl_into(dev_env, ptr["sq"], o, N_QUERIES, blocking=True), (dev, host_env, dev_env)),
                      lambda: N.shade_ibl_one(host_env, sq)),
    }


@pytest.mark.parametrize("name", ("probe_lookup", "probe_lookup_visible", "cube_lookup", "cube_chain_lookup", "shade_ibl"))
def test_lookups_and_the_shader(ctx, env, monkeypatch, name):
    case, one_form = _lookup_cases(ctx, env)[name]
    whole = _same_under_every_cap(monkeypatch, case, QUERY_CAPS)
    want = one_form()
    assert whole == np.ascontiguousarray(want).tobytes()
    # the queries have answers of their own: a launch that began at query 0 again would show
    assert want["valid"].sum() > N_QUERIES // 2 and len({r.tobytes() for r in want[want["valid"] == 1]}) > N_QUERIES // 2
