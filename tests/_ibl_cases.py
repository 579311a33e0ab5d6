"""Synthetic inputs of the image-based shading tests (tests/test_ibl_cpu.py, tests/test_ibl.py): probe grids, distance maps,
cube chains and tables from a seeded generator, the query set of the issue, and the two forms of one environment: the dict
tests/_ibl_ref.py reads and the rtr_shade_env the library reads."""
import math

import numpy as np

import _cube_filter_ref as FR
import _golden as G

A = G.A
N = G.rtr.native

TABLE_SHAPES = ((1, 1, 1), (3, 2, 5), (4, 4, 8), (5, 3, 11))  # (n_mu, n_rough, M)
ORIGIN, SPACING = (-1.0, -0.5, 0.25), (0.5, 0.75, 1.0)
BIAS = 0.0625
# (grid dims, chain (S, levels), table (n_rough, n_mu), map size T or 0)
ENVIRONMENTS = (((1, 1, 1), (1, 1), (1, 1), 0), ((2, 2, 2), (4, 3), (4, 4), 1), ((3, 2, 1), (4, 3), (3, 5), 4),
                ((2, 2, 2), (1, 1), (3, 5), 0), ((3, 2, 1), (4, 3), (1, 1), 1))


def environment(dims, chain, table_shape, T, seed=11):
    """the dict of one environment with every part (tests/_ibl_ref.py: shade_one); probe 1 (if there is one) is invalid
    and holds NaN, and so is texel (row 0, column 0) of face 3 of level 0 of a chain with S > 1"""
    rng = np.random.default_rng(seed + 100 * T + dims[0])
    n = dims[0] * dims[1] * dims[2]
    probes = np.zeros(n, dtype=A.PROBE_SH_DTYPE)
    probes["c"] = rng.uniform(-1.0, 1.0, (n, 9, 3))
    probes["c"][:, 0, :] += 2.0
    probes["count"], probes["valid"] = 64, 1
    if n > 1:
        probes["valid"][1], probes["c"][1] = 0, np.nan
    depth = None
    if T:
        depth = np.zeros((n, T, T), dtype=A.PROBE_DEPTH_DTYPE)
        depth["mean"] = rng.uniform(0.2, 1.5, depth.shape)
        depth["mean2"] = depth["mean"] * depth["mean"] + rng.uniform(0.0, 0.1, depth.shape)
        depth["hits"], depth["valid"] = 8, 1
    S, n_levels = chain
    levels, n_records = FR.plan(S, n_levels)
    records = np.zeros(n_records, dtype=A.GATHER_OUT_DTYPE)
    records["v"] = rng.uniform(0.0, 2.0, (n_records, 3))
    records["count"], records["valid"] = 4, 1
    if S > 1:
        records["valid"][3 * S * S], records["v"][3 * S * S] = 0, np.nan
    tab = rng.uniform(0.0, 1.0, table_shape + (2,))
    return dict(parts=3, origin=ORIGIN, spacing=SPACING, dims=dims, probes=probes, depth=depth, normal_bias=BIAS,
                levels=levels, records=records, tab=tab)


def native_env(env, parts, arrays=None):
    """the rtr_shade_env of the dict over its host arrays, or over the device pointers ``arrays`` = dict(probes=, depth=,
    chain=, table=); only the members of the selected parts are set"""
    a = arrays or {}
    kw = dict(parts=parts, n_rough=env["tab"].shape[0], n_mu=env["tab"].shape[1])
    if parts & 1:
        kw.update(grid=N.probe_grid(env["origin"], env["spacing"], env["dims"]), probes=a.get("probes", env["probes"]))
        if env["depth"] is not None:
            kw.update(depth=a.get("depth", env["depth"]), visible=N.probe_visible_params(env["depth"].shape[-1], env["normal_bias"]))
    if parts & 2:
        kw.update(levels=env["levels"], chain=a.get("chain", env["records"]), n_records=len(env["records"]))
    return N.shade_env(a.get("table", table_records(env["tab"])), **kw)


def table_records(tab):
    t = np.zeros(tab.shape[:2], dtype=A.BRDF_ENTRY_DTYPE)
    t["a"], t["b"] = tab[..., 0], tab[..., 1]
    return t


def special_queries(env):
    """the named queries of the issue: every one is not BAD"""
    S = env["levels"][0][0]
    inside = tuple(ORIGIN[a] + 0.3 * SPACING[a] for a in range(3))
    rows = [
        # p, n, v, base, roughness, metallic
        (inside, (0, 0, 2.0), (3.0, 0, 0), (0.8, 0.5, 0.2), 0.5, 0.0),          # mu exactly 0
        (inside, (0, 0, 1.0), (1.0, 0, -1.0), (0.8, 0.5, 0.2), 0.5, 0.5),       # mu negative
        (inside, (0, 4.0, 0), (0, 0.25, 0), (0.8, 0.5, 0.2), 0.5, 1.0),         # mu = 1
        (inside, (1.0, 2.0, 3.0), (2.0, 1.0, 3.0), (0.1, 0.9, 0.4), 0.0, 0.0),  # roughness 0, 0.01, 1, 7
        (inside, (1.0, 2.0, 3.0), (2.0, 1.0, 3.0), (0.1, 0.9, 0.4), 0.01, 1.0),
        (inside, (1.0, 2.0, 3.0), (2.0, 1.0, 3.0), (0.1, 0.9, 0.4), 1.0, 0.0),
        (inside, (1.0, 2.0, 3.0), (2.0, 1.0, 3.0), (0.1, 0.9, 0.4), 7.0, 1.0),
        (inside, (1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.5, 0.5, 0.5), 0.3, 1.0),  # R along a cube edge
        (inside, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), 0.3, 0.0),  # ... and a corner
        ((-50.0, 60.0, 70.0), (0.3, -1.0, 0.2), (0.0, -1.0, 0.5), (1.0, 1.0, 1.0), 0.6, 0.25),  # outside the grid
        # next to the invalid probe 1 (all its weight on the x axis): an invalid probe among the corners
        ((ORIGIN[0] + 0.9 * SPACING[0], ORIGIN[1] + 0.1, ORIGIN[2] + 0.1), (0, 1.0, 0), (0.2, 1.0, 0), (0.3, 0.3, 0.3), 0.2, 0.5),
        (inside, (0, 0, 1.0), (0, 0, 1.0), (0.0, 0.0, 0.0), 0.4, 0.0),          # base 0, metallic 0
    ]
    if S > 1:  # R = n = v towards texel (0, 0) of face 3 (-y; u = x, v = -z): an invalid texel under a tap at roughness 0
        u = (2.0 * 0.5) / S - 1.0
        rows.append((inside, (u, -1.0, -u), (u, -1.0, -u), (0.5, 0.5, 0.5), 0.0, 0.5))
    q = np.zeros(len(rows), dtype=A.SHADE_QUERY_DTYPE)
    for k, row in enumerate(rows):
        q[k] = row
    return q


def queries(env, n, seed=3):
    """n queries: the named ones first, random ones behind them (positions in and around the grid)"""
    rng = np.random.default_rng(seed + n)
    special = special_queries(env)
    q = np.zeros(n, dtype=A.SHADE_QUERY_DTYPE)
    m = min(n, len(special))
    q[:m] = special[:m]
    k = n - m
    lo = np.array(ORIGIN) - 0.5
    hi = np.array(ORIGIN) + (np.array(env["dims"]) - 1) * np.array(SPACING) + 0.5
    q["p"][m:] = rng.uniform(lo, hi, (k, 3))
    q["n"][m:] = rng.normal(size=(k, 3)) * 2.0 ** rng.integers(-3, 4, (k, 1))
    q["v"][m:] = rng.normal(size=(k, 3))
    q["base"][m:] = rng.uniform(0.0, 1.0, (k, 3))
    q["roughness"][m:] = rng.uniform(-0.1, 1.2, k)
    q["metallic"][m:] = rng.choice([0.0, 1.0, 0.5, 0.25], k)
    return q


def bad_queries(good):
    """(field, component or None, value) spoiled copies of ``good``, one BAD query each"""
    out = []
    for name in ("p", "n", "v", "base"):
        for comp, value in ((0, math.nan), (1, math.inf), (2, -math.inf)):
            q = good.copy()
            q[name][comp] = value
            out.append(q)
    for name in ("roughness", "metallic"):
        for value in (math.nan, math.inf):
            q = good.copy()
            q[name] = value
            out.append(q)
    for name in ("n", "v"):
        q = good.copy()
        q[name] = 0.0
        out.append(q)
        q = good.copy()
        q[name] = 1e200  # its length overflows
        out.append(q)
    return np.array(out, dtype=A.SHADE_QUERY_DTYPE)
