"""Image-based shading (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*) without a GPU: the declarations and record layouts,
the parameter and environment checks, and the host-only rtr_brdf_entry_one, rtr_brdf_fetch_one and rtr_shade_ibl_one
against the numpy restatement of the contract (tests/_ibl_ref.py) bit for bit; what the table's quadrature means, against
a brute-force integration of the reference's own specular term; what the shader's sum means at its two ends."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _golden as G
import _ibl_cases as IC
import _ibl_ref as IR

rtr = G.rtr
A = rtr._abi
N = rtr.native

NAMES = ("rtr_brdf_table", "rtr_brdf_table_device", "rtr_brdf_entry_one", "rtr_brdf_fetch_one", "rtr_shade_ibl",
         "rtr_shade_ibl_device", "rtr_shade_ibl_one")
INV = A.RTR_ERR_INVALID


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _body(name):
    body = re.search(r"typedef struct %s \{[^\n]*\n(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return " ".join(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split())


def test_declared_exported_and_the_abi_version_stays():
    text = _header()
    lib = N.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in N.EXPORTS
        getattr(lib, name)
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert re.search(r"#define RTR_ABI_VERSION 4\b", text)
    assert re.search(r"#define RTR_SHADE_DIFFUSE 1\b", text) and re.search(r"#define RTR_SHADE_SPECULAR 2\b", text)
    assert (A.SHADE_DIFFUSE, A.SHADE_SPECULAR) == (1, 2)


def test_struct_layouts():
    assert _body("rtr_brdf_params") == "int32_t n_mu, n_rough; int32_t nodes; int32_t pad; double reserved[2];"
    assert _body("rtr_brdf_entry") == "double a, b;"
    assert _body("rtr_shade_query") == "double p[3]; double n[3]; double v[3]; double base[3]; double roughness, metallic;"
    assert _body("rtr_shade_env") == ("int32_t parts; int32_t n_levels; const rtr_probe_grid* grid; const rtr_probe_sh* probes; "
                                      "const rtr_probe_depth_texel* depth; const rtr_probe_visible_params* visible; "
                                      "const rtr_cube_level* levels; const rtr_gather_out* chain; int64_t n_records; "
                                      "const rtr_brdf_entry* table; int32_t n_mu, n_rough;")
    assert C.sizeof(A.BrdfParamsC) == 32 == A.BRDF_PARAMS_SIZE and C.sizeof(A.ShadeEnvC) == 80 == A.SHADE_ENV_SIZE
    assert A.BRDF_ENTRY_DTYPE.itemsize == 16 and A.SHADE_QUERY_DTYPE.itemsize == 112
    assert [n for n, _ in A.BrdfParamsC._fields_] == ["n_mu", "n_rough", "nodes", "pad", "reserved"]
    assert [n for n, _ in A.ShadeEnvC._fields_] == ["parts", "n_levels", "grid", "probes", "depth", "visible", "levels", "chain",
                                                    "n_records", "table", "n_mu", "n_rough"]
    assert list(A.SHADE_QUERY_DTYPE.names) == ["p", "n", "v", "base", "roughness", "metallic"]


# ---- the table ----

@pytest.mark.parametrize("shape", IC.TABLE_SHAPES)
def test_entry_one_equals_the_restatement(shape):
    n_mu, n_rough, M = shape
    got = N.brdf_table_host(n_mu, n_rough, M)
    want = IR.table(n_mu, n_rough, M)
    assert _same_bits(got["a"], want[..., 0]) and _same_bits(got["b"], want[..., 1])
    assert (got["a"] > 0).all() and (got["b"] > 0).all() and (got["a"] + got["b"] < 1.05).all()


def _entry(bp, r=0, c=0):
    out = np.zeros(1, dtype=A.BRDF_ENTRY_DTYPE)
    return N.lib().rtr_brdf_entry_one(C.byref(bp), r, c, out.ctypes.data)


def test_table_parameters_are_checked_on_both_sides():
    for kw in (dict(nodes=0), dict(nodes=257), dict(n_mu=0), dict(n_mu=257), dict(n_rough=0), dict(n_rough=257)):
        assert _entry(N.brdf_params(**dict(dict(n_mu=2, n_rough=2, nodes=2), **kw))) == INV, kw
    for kw in (dict(nodes=1), dict(nodes=256), dict(n_mu=1), dict(n_mu=256), dict(n_rough=1), dict(n_rough=256)):
        assert _entry(N.brdf_params(**dict(dict(n_mu=2, n_rough=2, nodes=2), **kw))) == 0, kw
    bp = N.brdf_params(2, 2, 2)
    bp.pad = 1
    assert _entry(bp) == INV
    bp.pad = 0
    for k in range(2):
        bp.reserved[k] = 1.0
        assert _entry(bp) == INV
        bp.reserved[k] = 0.0
    for r, c in ((-1, 0), (2, 0), (0, -1), (0, 2)):
        assert _entry(bp, r, c) == INV
    assert _entry(bp, 1, 1) == 0
    lib = N.lib()
    assert lib.rtr_brdf_entry_one(None, 0, 0, np.zeros(2).ctypes.data) == INV
    assert lib.rtr_brdf_entry_one(C.byref(bp), 0, 0, None) == INV
    out = np.zeros(4, dtype=A.BRDF_ENTRY_DTYPE)
    assert lib.rtr_brdf_table(None, C.byref(bp), out.ctypes.data) == INV  # a context before any device work
    assert lib.rtr_brdf_table_device(None, C.byref(bp), out.ctypes.data, 1) == INV


def _fetch_points(n):
    """coordinates along one axis of n texels: the centres, both clamped ends, the exact texel boundaries, and between"""
    pts = [(i + 0.5) / n for i in range(n)] + [i / n for i in range(n + 1)] + [-0.25, 0.0, 1.0, 1.5, 0.5 / n, 1.0 - 0.5 / n]
    return pts + [0.37, 0.81]


@pytest.mark.parametrize("shape", ((1, 1), (1, 4), (5, 1), (3, 5), (4, 4)))
def test_fetch_equals_the_restatement(shape):
    n_rough, n_mu = shape
    tab = np.random.default_rng(7).uniform(-1.0, 1.0, (n_rough, n_mu, 2))
    rec = IC.table_records(tab)
    for mu in _fetch_points(n_mu):
        for rough in _fetch_points(n_rough):
            got, want = N.brdf_fetch_one(rec, mu, rough), IR.fetch(tab, mu, rough)
            assert _same_bits(np.array(got), np.array(want)), (mu, rough)
    for i in range(n_mu):  # a texel centre gives the texel
        for j in range(n_rough):
            if (i + 0.5) / n_mu * n_mu - 0.5 == i and (j + 0.5) / n_rough * n_rough - 0.5 == j:
                assert N.brdf_fetch_one(rec, (i + 0.5) / n_mu, (j + 0.5) / n_rough) == tuple(tab[j, i])
    assert N.brdf_fetch_one(rec, -3.0, -3.0) == tuple(tab[0, 0]) and N.brdf_fetch_one(rec, 3.0, 3.0) == tuple(tab[-1, -1])


def test_fetch_reads_no_tap_of_weight_zero_and_checks_its_arguments():
    tab = np.random.default_rng(8).uniform(0.0, 1.0, (3, 3, 2))
    rec = IC.table_records(tab)
    rec[1, 2] = (math.nan, math.nan)  # column 2, row 1: next to the centre texel, weight 0 at the centre
    rec[2, 1] = (math.nan, math.nan)
    assert N.brdf_fetch_one(rec, 0.5, 0.5) == tuple(tab[1, 1])
    lib = N.lib()
    out = np.zeros(1, dtype=A.BRDF_ENTRY_DTYPE)
    t, o = rec.ctypes.data, out.ctypes.data
    for args in ((0, 3, t, 0.5, 0.5, o), (257, 3, t, 0.5, 0.5, o), (3, 0, t, 0.5, 0.5, o), (3, 257, t, 0.5, 0.5, o),
                 (3, 3, None, 0.5, 0.5, o), (3, 3, t, 0.5, 0.5, None), (3, 3, t, math.nan, 0.5, o), (3, 3, t, 0.5, math.inf, o)):
        assert lib.rtr_brdf_fetch_one(*args) == INV, args


CHECKS = ((0.9, 0.5), (0.3, 0.5), (0.9, 1.0), (0.05, 0.7), (0.5, 0.3))
# (n, index) with (index + 0.5) / n equal to the coordinate, where there is one
AXIS = {0.9: (5, 4), 0.3: (5, 1), 0.05: (10, 0), 0.5: (1, 0), 0.7: (5, 3)}


@pytest.fixture(scope="module")
def brute():
    return {point: IR.brute_force(*point) for point in CHECKS}


def test_the_quadrature_is_the_integral_of_the_reference_term(brute):
    """The table at M = 128 against the brute-force integration over light directions of D G (F-part) n.l / (4 n.v n.l +
    0.0001) on a 3000 x 6000 (cos theta, phi) midpoint grid: |da|, |db| <= 1e-4 (the issue's bound: five times what its
    author measured, the brute-force side being a quadrature itself).  A point that is an entry of some table goes through
    rtr_brdf_entry_one, (0.9, 1.0) -- no (r + 0.5) / n is 1 -- through the restatement's node sums, which the tests above
    hold to the library bit for bit."""
    for mu, rough in CHECKS:
        want = brute[(mu, rough)]
        got = IR.entry_at(mu, rough, 128)
        if rough in AXIS:
            (n_mu, c), (n_rough, r) = AXIS[mu], AXIS[rough]
            assert (c + 0.5) / n_mu == mu and (r + 0.5) / n_rough == rough
            out = np.zeros(1, dtype=A.BRDF_ENTRY_DTYPE)
            assert N.lib().rtr_brdf_entry_one(C.byref(N.brdf_params(n_mu, n_rough, 128)), r, c, out.ctypes.data) == 0
            assert (float(out["a"][0]), float(out["b"][0])) == got
        print("mu %.2f rough %.2f: a %.6f b %.6f, brute force %.6f %.6f, |da| %.2e |db| %.2e" %
              (mu, rough, got[0], got[1], want[0], want[1], abs(got[0] - want[0]), abs(got[1] - want[1])))
        assert abs(got[0] - want[0]) <= 1e-4 and abs(got[1] - want[1]) <= 1e-4, (mu, rough)


# ---- the shader ----

@pytest.fixture(scope="module")
def envs():
    return [IC.environment(*e) for e in IC.ENVIRONMENTS]


@pytest.mark.parametrize("parts", (1, 2, 3))
@pytest.mark.parametrize("which", range(len(IC.ENVIRONMENTS)))
def test_shade_one_equals_the_restatement(envs, which, parts):
    env = dict(envs[which], parts=parts)
    q = IC.queries(env, 24)
    got = N.shade_ibl_one(IC.native_env(env, parts), q)
    want = IR.shade(env, q, A.GATHER_OUT_DTYPE)
    assert _same_bits(got, want)
    assert got["valid"].any()
    if parts & 2 and env["levels"][0][0] > 1:
        assert got["valid"][12] == 0 and not got["v"][12].any() and got["count"][12] == 0  # the invalid texel under a tap
    if parts == 1:
        assert got["valid"].all()
        if len(env["probes"]) > 1:  # the invalid probe among the corners: seven of eight, or three of four in a flat grid
            assert got["count"][10] == (7 if env["dims"] == (2, 2, 2) else 3)


def test_bad_queries_are_rejected(envs):
    env = envs[2]
    ne = IC.native_env(env, 3)
    one = IC.queries(env, 1)
    good = one[0]
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    lib = N.lib()
    assert lib.rtr_shade_ibl_one(C.byref(ne), one.ctypes.data, out.ctypes.data) == 0
    bad = IC.bad_queries(good)
    assert len(bad) == 20
    for k in range(len(bad)):
        assert IR.query_bad(bad[k])
        assert lib.rtr_shade_ibl_one(C.byref(ne), bad[k:k + 1].ctypes.data, out.ctypes.data) == INV, k
    assert lib.rtr_shade_ibl_one(C.byref(ne), None, out.ctypes.data) == INV
    assert lib.rtr_shade_ibl_one(C.byref(ne), bad.ctypes.data, None) == INV
    assert lib.rtr_shade_ibl_one(None, bad.ctypes.data, out.ctypes.data) == INV


def _shade_rc(ne, q):
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    return N.lib().rtr_shade_ibl_one(C.byref(ne), q.ctypes.data, out.ctypes.data)


def test_the_environment_is_checked_for_the_selected_parts_only(envs):
    env = envs[2]  # grid (3, 2, 1), maps T = 4, chain S = 4 with three levels, table 3 x 5
    q = IC.queries(env, 1)
    for parts in (1, 2, 3):
        assert _shade_rc(IC.native_env(env, parts), q) == 0
    for parts in (0, 4, -1):
        ne = IC.native_env(env, 3)
        ne.parts = parts
        assert _shade_rc(ne, q) == INV, parts
    selected = {"grid": 1, "probes": 1, "levels": 2, "chain": 2, "table": 3}
    for member, part in selected.items():
        for parts in (1, 2, 3):
            ne = IC.native_env(env, 3)
            ne.parts = parts
            setattr(ne, member, None)
            assert _shade_rc(ne, q) == (INV if parts & part else 0), (member, parts)  # NULL: rejected iff its part is selected
    for member in ("depth", "visible"):  # one without the other
        ne = IC.native_env(env, 3)
        setattr(ne, member, None)
        assert _shade_rc(ne, q) == INV
        ne.parts = 2
        assert _shade_rc(ne, q) == 0
    ne = IC.native_env(env, 3)
    ne.depth = ne.visible = None  # both NULL: the plain lookup
    plain = dict(env, depth=None)
    out = N.shade_ibl_one(ne, q)
    assert _same_bits(out, IR.shade(plain, q, A.GATHER_OUT_DTYPE))
    for member, value in (("n_mu", 0), ("n_mu", 257), ("n_rough", 0), ("n_rough", 257), ("n_levels", 0), ("n_levels", 14),
                          ("n_records", -1), ("n_records", len(env["records"]) - 1)):
        ne = IC.native_env(env, 3)
        setattr(ne, member, value)
        assert _shade_rc(ne, q) == INV, member
    lib = N.lib()
    ne = IC.native_env(env, 3)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    assert lib.rtr_shade_ibl(None, C.byref(ne), q.ctypes.data, out.ctypes.data, 1) == INV  # a context before any device work
    assert lib.rtr_shade_ibl_device(None, C.byref(ne), q.ctypes.data, out.ctypes.data, 1, 1) == INV


def _lookup_x(env, q):
    """X of the restatement for the queries' reflection vectors"""
    out = []
    for k in range(len(q)):
        n, v = q["n"][k], q["v"][k]
        N_ = n * (1.0 / math.sqrt(float(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])))
        V_ = v * (1.0 / math.sqrt(float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])))
        mu = float((N_[0] * V_[0] + N_[1] * V_[1]) + N_[2] * V_[2])
        rough = min(max(float(q["roughness"][k]), 0.01), 1.0)
        x = IR.CF.chain_lookup_one(env["levels"], env["records"], (2.0 * mu) * N_ - V_, rough * rough)
        out.append((x, IR.fetch(env["tab"], max(mu, 0.0), rough)))
    return out


def test_the_sum_at_its_two_ends(envs):
    """metallic 1 and the specular part alone: out = X (base a + b); metallic 0, base 0 and both parts: out = X (0.04 a + b)"""
    env = envs[1]
    q = IC.queries(env, 40)
    q = q[IR.shade(dict(env, parts=3), q, A.GATHER_OUT_DTYPE)["valid"] == 1]
    assert len(q) > 20
    metal = q.copy()
    metal["metallic"] = 1.0
    got = N.shade_ibl_one(IC.native_env(env, 2), metal)
    for k, (x, (a, b)) in enumerate(_lookup_x(env, metal)):
        assert got["valid"][k] == 1 and got["count"][k] == x[1]
        assert _same_bits(got["v"][k], x[0] * ((0.0 * 0.04 + 1.0 * metal["base"][k]) * a + b))
    black = q.copy()
    black["metallic"], black["base"] = 0.0, 0.0
    got = N.shade_ibl_one(IC.native_env(env, 3), black)
    for k, (x, (a, b)) in enumerate(_lookup_x(env, black)):
        assert got["valid"][k] == 1
        assert _same_bits(got["v"][k], x[0] * (0.04 * a + b) + 0.0)


def test_python_faces_on_the_host():
    tab = rtr.BrdfTable.make(3, 2, 5)
    assert _same_bits(tab.entries, N.brdf_table_host(3, 2, 5)) and tab.fetch(0.5, 0.75) == N.brdf_fetch_one(tab.entries, 0.5, 0.75)
    env = IC.environment(*IC.ENVIRONMENTS[2])
    grid = rtr.ProbeGrid(IC.ORIGIN, IC.SPACING, env["dims"], env["probes"])
    grid.depth = env["depth"]
    chain = rtr.CubeChain(N.cube_levels(env["levels"]), env["records"])
    table = rtr.BrdfTable(IC.table_records(env["tab"]))
    q = IC.queries(env, 16)
    ibl = rtr.IblEnvironment(grid, chain, table, normal_bias=IC.BIAS)
    rec = ibl.shade_records(q["p"], q["n"], q["v"], q["base"], q["roughness"], q["metallic"])
    assert _same_bits(rec, IR.shade(env, q, A.GATHER_OUT_DTYPE))
    assert _same_bits(ibl.shade(q["p"], q["n"], q["v"], q["base"], q["roughness"], q["metallic"]), rec["v"])
    only = rtr.IblEnvironment(None, chain, table).shade_records(q["p"], q["n"], q["v"], q["base"], q["roughness"], q["metallic"])
    assert _same_bits(only, IR.shade(dict(env, parts=2), q, A.GATHER_OUT_DTYPE))
    with pytest.raises(ValueError):
        rtr.IblEnvironment(None, None, table)
