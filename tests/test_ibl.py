"""Image-based shading (include/rtr_hip.h: rtr_brdf_table, rtr_shade_ibl and their device-pointer forms) on the GPU, bit
for bit against the numpy restatement of the contract (tests/_ibl_ref.py) and the host-only _one forms.  All inputs are
synthetic (tests/_ibl_cases.py) but for the stream-order test, which bakes scene 21.

A batch of 4099 queries is held to rtr_shade_ibl_one, which tests/test_ibl_cpu.py holds to the restatement; its first 65
are held to the restatement here as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _cube_filter_ref as FR
import _golden as G
import _ibl_cases as IC
import _ibl_ref as IR

rtr = G.rtr
A = G.A
N = rtr.native

pytestmark = pytest.mark.gpu
REC, ENTRY, QUERY = 32, 16, 112
INV = A.RTR_ERR_INVALID


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


def _sentinel(n_records, size=REC):
    import torch
    return torch.full(((n_records + 1) * size,), 0xA5, dtype=torch.uint8, device="cuda")


# ---- the table ----

def _table_into(ctx, n_mu, n_rough, M):
    """the device entry's records [n_rough, n_mu]; one sentinel record behind them must stay"""
    import torch
    n = n_mu * n_rough
    d_out = _sentinel(n, ENTRY)
    torch.cuda.synchronize()
    ctx.brdf_table_into(d_out.data_ptr(), n_mu, n_rough, M, blocking=True)
    raw = d_out.cpu().numpy()
    assert (raw[n * ENTRY:] == 0xA5).all()
    return raw[:n * ENTRY].view(A.BRDF_ENTRY_DTYPE).reshape(n_rough, n_mu)


def _host_table(ctx, n_mu, n_rough, M):
    """the host entry's records, written into an array with a sentinel record behind them"""
    buf = np.full((n_mu * n_rough + 1) * 2, -7.0).view(A.BRDF_ENTRY_DTYPE)
    got = ctx.brdf_table(n_mu, n_rough, M, out=buf)
    assert buf["a"][-1] == -7.0 and buf["b"][-1] == -7.0
    return got


def _want(n_mu, n_rough, M):
    return IC.table_records(IR.table(n_mu, n_rough, M))


@pytest.mark.parametrize("shape", IC.TABLE_SHAPES + ((2, 2, 64),))
def test_table_entries_equal_the_restatement_and_the_one_form(ctx, shape):
    """M = 5: 50 nodes, lanes without one; M = 11: 242, a ragged last round; M = 64: 128 nodes per lane"""
    n_mu, n_rough, M = shape
    want = _want(*shape)
    assert _same_bits(N.brdf_table_host(*shape), want)
    assert _same_bits(_host_table(ctx, *shape), want)
    assert _same_bits(_table_into(ctx, *shape), want)


@pytest.mark.parametrize("shape", ((256, 1, 1), (1, 256, 1)))
def test_table_at_its_limits(ctx, shape):
    want = _want(*shape)
    assert _same_bits(_host_table(ctx, *shape), want)
    assert _same_bits(_table_into(ctx, *shape), want)


def test_launch_split_changes_no_bit(ctx, monkeypatch):
    """RTR_TABLE_NODES lowers the nodes per launch.  (5, 3, 11): an entry has 242 nodes; one entry per launch, 1 node (one
    entry still), three entries (cuts every row: columns 0..2, 3..4), seven (one whole row at a time), eleven (two rows,
    then one)"""
    shape = (5, 3, 11)
    monkeypatch.delenv("RTR_TABLE_NODES", raising=False)
    whole = ctx.brdf_table(*shape)
    assert _same_bits(whole, _want(*shape))
    for nodes in (242, 1, 242 * 3, 242 * 7, 242 * 11):
        monkeypatch.setenv("RTR_TABLE_NODES", str(nodes))
        assert _same_bits(ctx.brdf_table(*shape), whole), nodes
        assert _same_bits(_table_into(ctx, *shape), whole), nodes
    monkeypatch.setenv("RTR_TABLE_NODES", "-5")  # not a cap: ignored
    assert _same_bits(ctx.brdf_table(*shape), whole)


def test_table_entries_check_their_arguments(ctx):
    import torch
    L, h = ctx._L, ctx._h
    out = np.zeros(8, dtype=A.BRDF_ENTRY_DTYPE)
    d_buf = _sentinel(8, ENTRY)
    torch.cuda.synchronize()
    p = d_buf.data_ptr()
    for kw in (dict(nodes=0), dict(nodes=257), dict(n_mu=0), dict(n_mu=257), dict(n_rough=0), dict(n_rough=257)):
        bp = N.brdf_params(**dict(dict(n_mu=2, n_rough=2, nodes=2), **kw))
        assert L.rtr_brdf_table(h, C.byref(bp), out.ctypes.data) == INV, kw
        assert L.rtr_brdf_table_device(h, C.byref(bp), C.c_void_p(p), 1) == INV, kw
    bp = N.brdf_params(2, 2, 2)
    bp.pad = 1
    assert L.rtr_brdf_table(h, C.byref(bp), out.ctypes.data) == INV and L.rtr_brdf_table_device(h, C.byref(bp), C.c_void_p(p), 1) == INV
    bp.pad = 0
    assert L.rtr_brdf_table(h, None, out.ctypes.data) == INV and L.rtr_brdf_table(h, C.byref(bp), None) == INV
    assert L.rtr_brdf_table_device(h, C.byref(bp), None, 1) == INV
    assert L.rtr_brdf_table_device(h, C.byref(bp), C.c_void_p(p + 4), 1) == INV  # misaligned, before any launch
    assert not out.view(np.uint8).any() and (d_buf.cpu().numpy() == 0xA5).all()


# ---- the shader ----

@pytest.fixture(scope="module")
def envs():
    return [IC.environment(*e) for e in IC.ENVIRONMENTS]


def _env_over(env, parts, dev):
    return IC.native_env(env, parts, {name: t.data_ptr() for name, t in dev.items()})


def _device_env(env, parts):
    """(rtr_shade_env over device copies of the arrays of the selected parts, the copies and their host bytes)"""
    held = {"table": IC.table_records(env["tab"])}
    if parts & 1:
        held["probes"] = env["probes"]
        if env["depth"] is not None:
            held["depth"] = env["depth"]
    if parts & 2:
        held["chain"] = env["records"]
    dev = {name: _dev(a) for name, a in held.items()}
    return _env_over(env, parts, dev), dev, held


def _shade_into(ctx, ne, dev, held, q):
    """the device entry's records; one sentinel record behind them must stay, and every input keeps its bytes"""
    import torch
    n = len(q)
    d_q, d_out = _dev(q) if n else _sentinel(0, QUERY), _sentinel(n)
    torch.cuda.synchronize()
    ctx.shade_ibl_into(ne, d_q.data_ptr(), d_out.data_ptr(), n, blocking=True)
    raw = d_out.cpu().numpy()
    assert (raw[n * REC:] == 0xA5).all()
    if n:
        assert _same_bits(d_q.cpu().numpy(), q.view(np.uint8))
    for name, t in dev.items():
        assert _same_bits(t.cpu().numpy(), np.ascontiguousarray(held[name]).reshape(-1).view(np.uint8)), name
    return raw[:n * REC].view(A.GATHER_OUT_DTYPE)


@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("which", range(len(IC.ENVIRONMENTS)))
def test_shader_entries_equal_the_restatement_and_the_one_form(ctx, envs, which, parts):
    env = dict(envs[which], parts=parts)
    host_env = IC.native_env(env, parts)
    ne, dev, held = _device_env(env, parts)
    for n in (0, 1, 63, 65, 4099):
        q = IC.queries(env, n)
        one = N.shade_ibl_one(host_env, q)
        m = min(n, 65)
        assert _same_bits(one[:m], IR.shade(env, q[:m], A.GATHER_OUT_DTYPE)), n
        buf = np.zeros(n + 1, dtype=A.GATHER_OUT_DTYPE)
        buf["count"][n] = -7
        got = ctx.shade_ibl(host_env, q, out=buf)
        assert _same_bits(got[:n], one) and buf["count"][n] == -7 and not buf["v"][n].any(), n
        assert _same_bits(_shade_into(ctx, ne, dev, held, q), one), n
        if n >= 63:
            assert one["valid"].sum() > n // 2
            if parts & 2 and env["levels"][0][0] > 1:
                assert one["valid"][12] == 0  # the invalid texel under a tap


def test_host_entry_across_a_slice(ctx, envs):
    """2^20 + 77 queries: the second slice of the host entry finds the records the first one staged at the head of the buffer"""
    env = envs[2]
    n = (1 << 20) + 77
    q = IC.queries(env, n)
    host_env = IC.native_env(env, 3)
    buf = np.zeros(n + 1, dtype=A.GATHER_OUT_DTYPE)
    buf["count"][n] = -7
    got = ctx.shade_ibl(host_env, q, out=buf)
    assert buf["count"][n] == -7 and not buf["v"][n].any()
    ne, dev, held = _device_env(env, 3)
    assert _same_bits(got[:n], _shade_into(ctx, ne, dev, held, q))
    for part in (slice(0, 64), slice(n - 77, n)):  # the first and the last records against the host form of the contract
        assert _same_bits(got[part], N.shade_ibl_one(host_env, q[part]))


def test_bad_queries(ctx, envs):
    """the host entry names the first bad query and leaves `out` untouched; the device entry writes valid 0 for it"""
    env = envs[2]
    host_env = IC.native_env(env, 3)
    ne, dev, held = _device_env(env, 3)
    good = IC.queries(env, 70)
    bad = IC.bad_queries(good[5])
    want = N.shade_ibl_one(host_env, good)
    for k, at in ((0, 0), (7, 69), (13, 64)):
        q = good.copy()
        q[at] = bad[k]
        out = np.full(70 * 4, -3.0).view(A.GATHER_OUT_DTYPE)
        with pytest.raises(rtr.RtrError) as e:
            ctx.shade_ibl(host_env, q, out=out)
        assert e.value.code == INV and "index %d " % at in str(e.value)
        assert (out["v"] == -3.0).all()
    q = good.copy()
    q[1:1 + len(bad)] = bad
    expect = want.copy()
    expect[1:1 + len(bad)] = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)[0]
    assert _same_bits(_shade_into(ctx, ne, dev, held, q), expect)


def test_shader_entries_check_their_arguments(ctx, envs):
    import torch
    env = envs[2]
    L, h = ctx._L, ctx._h
    q = IC.queries(env, 4)
    out = np.zeros(4, dtype=A.GATHER_OUT_DTYPE)
    ne, dev, held = _device_env(env, 3)
    d_q, d_out = _dev(q), _sentinel(4)
    torch.cuda.synchronize()
    qp, op = C.c_void_p(d_q.data_ptr()), C.c_void_p(d_out.data_ptr())
    host_env = IC.native_env(env, 3)
    assert L.rtr_shade_ibl(h, C.byref(host_env), None, None, 0) == A.RTR_OK  # n == 0: nothing read, no launch
    assert L.rtr_shade_ibl_device(h, C.byref(ne), None, None, 0, 1) == A.RTR_OK
    for args in ((None, q.ctypes.data, out.ctypes.data, 4), (C.byref(host_env), None, out.ctypes.data, 4),
                 (C.byref(host_env), q.ctypes.data, None, 4), (C.byref(host_env), q.ctypes.data, out.ctypes.data, -1)):
        assert L.rtr_shade_ibl(h, *args) == INV
    for parts in (0, 4):
        bad = IC.native_env(env, 3)
        bad.parts = parts
        assert L.rtr_shade_ibl(h, C.byref(bad), q.ctypes.data, out.ctypes.data, 4) == INV
    for member, part in (("grid", 1), ("probes", 1), ("levels", 2), ("chain", 2), ("table", 3)):
        for parts in (1, 2, 3):
            e_host, e_dev = IC.native_env(env, 3), _env_over(env, 3, dev)
            for e in (e_host, e_dev):
                e.parts = parts
                setattr(e, member, None)
            want = INV if parts & part else A.RTR_OK  # a NULL array of a part that is not selected is accepted
            assert L.rtr_shade_ibl(h, C.byref(e_host), q.ctypes.data, out.ctypes.data, 4) == want, (member, parts)
            assert L.rtr_shade_ibl_device(h, C.byref(e_dev), qp, op, 4, 1) == want, (member, parts)
    out[:] = 0
    d_out.fill_(0xA5)
    torch.cuda.synchronize()
    assert L.rtr_shade_ibl_device(h, C.byref(ne), C.c_void_p(d_q.data_ptr() + 4), op, 4, 1) == INV  # misaligned
    assert L.rtr_shade_ibl_device(h, C.byref(ne), qp, qp, 4, 1) == INV  # out over the queries
    assert L.rtr_shade_ibl_device(h, C.byref(ne), qp, C.c_void_p(dev["chain"].data_ptr()), 4, 1) == INV  # ... over the chain
    assert L.rtr_shade_ibl_device(h, C.byref(ne), qp, C.c_void_p(dev["table"].data_ptr() + 16), 1, 1) == INV  # ... inside the table
    assert (d_out.cpu().numpy() == 0xA5).all()
    for name, t in dev.items():
        assert _same_bits(t.cpu().numpy(), np.ascontiguousarray(held[name]).reshape(-1).view(np.uint8)), name


# ---- behind a bake, and the other faces ----

CENTRE = (278.0, 400.0, 400.0)  # above the two boxes of the Cornell box of scene 21
LO, HI = (100.0, 100.0, 100.0), (450.0, 450.0, 450.0)


def test_bake_and_shade_in_stream_order(ctx):
    """capture_cube_into (S = 8, 2 samples), two cube_filter_into levels, probe_radiance_into over a 2 x 2 x 2 grid,
    brdf_table_into and shade_ibl_into queued back to back without a wait between them, one synchronise at the end: the
    records equal the host entries fed the host copies of what the calls before them wrote"""
    import torch
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1, integrator=4)
    levels, n_records = FR.plan(8, 3)
    grid = rtr.ProbeGrid.in_box(LO, HI, (2, 2, 2))
    pts = N.probe_points(grid.positions())
    rng = np.random.default_rng(21)
    q = N.shade_queries(rng.uniform(LO, HI, (300, 3)), rng.normal(size=(300, 3)), rng.normal(size=(300, 3)),
                        rng.uniform(0.0, 1.0, (300, 3)), rng.uniform(0.0, 1.0, 300), rng.choice([0.0, 1.0, 0.5], 300))
    d_centre, d_pts, d_q = _dev(N.probe_points(np.array([CENTRE]))), _dev(pts), _dev(q)
    d_chain, d_sh, d_table, d_out = _sentinel(n_records), _sentinel(8, 224), _sentinel(12, ENTRY), _sentinel(300)
    torch.cuda.synchronize()
    base = d_chain.data_ptr()
    ne = N.shade_env(d_table.data_ptr(), grid=grid.grid(), probes=d_sh.data_ptr(), levels=levels, chain=base, n_records=n_records,
                     n_mu=4, n_rough=3)
    assert ne.parts == 3
    ctx.capture_cube_into(prm, d_centre.data_ptr(), base, 1, face_size=8, samples=2, seed=7, blocking=False)
    for S, at, alpha in levels[1:]:
        ctx.cube_filter_into(base, base + at * REC, 1, face_in=8, face_out=S, alpha=alpha, blocking=False)
    ctx.probe_radiance_into(prm, d_pts.data_ptr(), d_sh.data_ptr(), 8, samples=16, seed=5, blocking=False)
    ctx.brdf_table_into(d_table.data_ptr(), 4, 3, 16, blocking=False)
    ctx.shade_ibl_into(ne, d_q.data_ptr(), d_out.data_ptr(), 300, blocking=False)
    ctx.synchronize()
    chain = d_chain.cpu().numpy()[:n_records * REC].view(A.GATHER_OUT_DTYPE)
    sh = d_sh.cpu().numpy()[:8 * 224].view(A.PROBE_SH_DTYPE)
    table = d_table.cpu().numpy()[:12 * ENTRY].view(A.BRDF_ENTRY_DTYPE).reshape(3, 4)
    for t, n, size in ((d_chain, n_records, REC), (d_sh, 8, 224), (d_table, 12, ENTRY), (d_out, 300, REC)):
        assert (t.cpu().numpy()[n * size:] == 0xA5).all()
    assert _same_bits(table, ctx.brdf_table(4, 3, 16)) and _same_bits(sh, ctx.probe_radiance(prm, pts, samples=16, seed=5))
    assert _same_bits(chain[:384].reshape(6, 8, 8), ctx.capture_cube_records(prm, np.array([CENTRE]), face_size=8, samples=2, seed=7)[0])
    host = N.shade_env(table, grid=grid.grid(), probes=sh, levels=levels, chain=chain)
    got = d_out.cpu().numpy()[:300 * REC].view(A.GATHER_OUT_DTYPE)
    assert _same_bits(got, ctx.shade_ibl(host, q)) and _same_bits(got, N.shade_ibl_one(host, q))
    assert got["valid"].all() and (got["v"] != 0).any()


def test_python_faces_on_a_context(ctx, envs):
    env = envs[2]
    assert _same_bits(rtr.BrdfTable.make(5, 3, 11, ctx=ctx).entries, rtr.BrdfTable.make(5, 3, 11).entries)
    grid = rtr.ProbeGrid(IC.ORIGIN, IC.SPACING, env["dims"], env["probes"])
    grid.depth = env["depth"]
    ibl = rtr.IblEnvironment(grid, rtr.CubeChain(N.cube_levels(env["levels"]), env["records"]),
                             rtr.BrdfTable(IC.table_records(env["tab"])), normal_bias=IC.BIAS)
    q = IC.queries(env, 100)
    args = (q["p"], q["n"], q["v"], q["base"], q["roughness"], q["metallic"])
    assert _same_bits(ibl.shade_records(*args, ctx=ctx), ibl.shade_records(*args))
    assert _same_bits(ibl.shade(*args, ctx=ctx), N.shade_ibl_one(IC.native_env(env, 3), q)["v"])


def test_the_command_line_writes_the_table(ctx, tmp_path):
    """rtr_cli --brdf-table 4,4 --brdf-nodes 8 --brdf-out (Renderer::brdf_table) writes the restatement's bytes"""
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    out = str(tmp_path / "table.bin")
    r = subprocess.run([cli, "21", "4", "--brdf-table", "4,4", "--brdf-nodes", "8", "--brdf-out", out], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert open(out, "rb").read() == IR.table(4, 4, 8).astype("<f8").tobytes()
    for args in (["--brdf-table", "4,4"], ["--brdf-out", out], ["--brdf-table", "0,4", "--brdf-out", out],
                 ["--brdf-table", "4,257", "--brdf-out", out], ["--brdf-table", "4,4", "--brdf-out", out, "--brdf-nodes", "257"],
                 ["--brdf-nodes", "8"], ["--brdf-table", "4,4", "--brdf-out", out, "--capture", "1,2,3", "--capture-out", out]):
        r = subprocess.run([cli, "21", "4"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, args
