"""Synthetic inputs of the capture-set tests (tests/test_capture_set_cpu.py, tests/test_capture_set.py): seeded sets in the
manner of _ibl_cases.environment -- volumes, the level-major records of their chains -- the named queries of the contract,
the wall-point cube of the meaning test, and the forms the library reads."""
import math

import numpy as np

import _capture_ref as CR
import _cube_filter_ref as FR
import _golden as G
import _ibl_cases as IC

A = G.A
N = G.rtr.native

CHAINS = ((1, 1), (4, 3))  # (S, levels)
COUNTS = (1, 2, 3)


def volume(centre, proxy_lo, proxy_hi, reach_lo, reach_hi, fade):
    v = np.zeros((), dtype=A.CAPTURE_VOLUME_DTYPE)
    v["centre"], v["proxy_lo"], v["proxy_hi"], v["reach_lo"], v["reach_hi"], v["fade"] = centre, proxy_lo, proxy_hi, reach_lo, reach_hi, fade
    return v


# volume 0: faded, around the origin; volume 1: unfaded, overlaps volume 0 in [0, 1]^3; volume 2: far from both
V0 = volume((0.125, -0.25, 0.375), (-2.0,) * 3, (2.0,) * 3, (-1.0,) * 3, (1.0,) * 3, 0.5)
V1 = volume((0.75, 0.5, 1.0), (-1.5,) * 3, (2.5,) * 3, (0.0,) * 3, (2.0,) * 3, 0.0)
V2 = volume((10.0, 10.5, 9.75), (8.0,) * 3, (12.0,) * 3, (9.0,) * 3, (11.0,) * 3, 0.25)


def volumes(C):
    return np.array([V0, V1, V2][:C], dtype=A.CAPTURE_VOLUME_DTYPE)


def records(C, chain, seed=5):
    """(levels of one capture, the level-major records of C chains): texel (row 0, column 0) of face 3 of level 0 of the
    last capture is invalid and holds NaN when S > 1"""
    S, n_levels = chain
    levels, n = FR.plan(S, n_levels)
    rng = np.random.default_rng(seed + 10 * C + S)
    rec = np.zeros(C * n, dtype=A.GATHER_OUT_DTYPE)
    rec["v"] = rng.uniform(0.0, 2.0, (C * n, 3))
    rec["count"], rec["valid"] = 4, 1
    if S > 1:
        at = (C - 1) * 6 * S * S + 3 * S * S
        rec["valid"][at], rec["v"][at] = 0, np.nan
    return levels, rec


def towards_invalid(S):
    """the direction of the centre of texel (0, 0) of face 3 (-y; u = x, v = -z)"""
    u = (2.0 * 0.5) / S - 1.0
    return (u, -1.0, -u)


def special_queries(C, S):
    """the named queries of the issue, (p, d, alpha) each"""
    c0, c1 = tuple(V0["centre"]), tuple(V1["centre"])
    last = [V0, V1, V2][C - 1]
    bad_d = towards_invalid(max(S, 2))
    rows = [
        ((1.0, 0.25, 0.5), (0.3, -1.0, 0.2), 0.1),      # 0: on a reach face of the faded volume 0: left out (volume 1 takes it)
        ((-1.0, 0.25, 0.5), (0.3, -1.0, 0.2), 0.1),     # 1: the same on the far face: nobody reaches it
        ((2.0, 1.5, 1.5), (-0.3, 1.0, 0.2), 0.1),       # 2: on a reach face of the unfaded volume 1: taken in
        (c0, (0.3, 0.2, -1.0), 0.0),                    # 3: p at a centre
        (c1, (0.3, 0.2, -1.0), 0.3),                    # 4
        ((0.5, 0.5, 0.5), (0.0, 1.0, 0.5), 0.2),        # 5: +0.0 in d
        ((0.5, 0.5, 0.5), (-0.0, 1.0, 0.5), 0.2),       # 6: -0.0 in d
        ((0.5, 0.5, 0.5), (-0.0, 0.0, -2.0), 0.2),      # 7: both
        ((0.0, 0.0, 0.0), (1.0, 1.0, 0.0), 0.0),        # 8: along a proxy edge of volume 0: two ta tie
        ((0.0, 0.0, 0.0), (-1.0, -1.0, -1.0), 0.0),     # 9: into a proxy corner: three tie
        ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), 0.5),        # 10: into the corner of both proxies, both weights 1
        ((0.25, 0.75, 0.125), (0.3, -0.2, 1.0), 0.6),   # 11: overlap, w0 = 0.5, w1 = 1; alpha between two levels
        ((0.25, 0.75, 0.125), (0.3, -0.2, 1.0), 0.25),  # 12: alpha on a level
        ((0.25, 0.75, 0.125), (0.3, -0.2, 1.0), 0.0),   # 13
        ((0.25, 0.75, 0.125), (0.3, -0.2, 1.0), 7.0),   # 14: clamped to the last level
        ((5.0, 5.0, 5.0), (0.3, -0.2, 1.0), 0.1),       # 15: no capture reaches p
        ((-0.5, -0.5, -0.5), (0.3, -0.2, 1.0), 0.1),    # 16: volume 0 alone
        (tuple(last["centre"]), bad_d, 0.0),            # 17: an invalid texel under a tap of a contributing capture (S > 1)
        ((-0.5, -0.5, -0.5), bad_d, 0.0),               # 18: ... of a capture that does not contribute (C > 1), or of the one
    ]
    q = np.zeros(len(rows), dtype=A.CAPTURE_QUERY_DTYPE)
    for k, (p, d, alpha) in enumerate(rows):
        q["p"][k], q["d"][k], q["alpha"][k] = p, d, alpha
    return q


def bad_queries():
    """every BAD spelling of a capture query"""
    good = np.zeros((), dtype=A.CAPTURE_QUERY_DTYPE)
    good["p"], good["d"], good["alpha"] = (0.25, 0.75, 0.125), (0.3, -0.2, 1.0), 0.3
    out = []
    for name in ("p", "d"):
        for comp in range(3):
            for value in (math.nan, math.inf, -math.inf):
                q = good.copy()
                q[name][comp] = value
                out.append(q)
    for value in (math.nan, math.inf, -math.inf):
        q = good.copy()
        q["alpha"] = value
        out.append(q)
    for d in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (1e200, 1e200, 0.0)):  # the length is 0, or overflows
        q = good.copy()
        q["d"] = d
        out.append(q)
    return np.array(out, dtype=A.CAPTURE_QUERY_DTYPE)


def queries(C, S, n, seed=7):
    """n queries: the named ones, the BAD ones (while there is room), random ones behind them"""
    rng = np.random.default_rng(seed + n)
    head = np.concatenate([special_queries(C, S), bad_queries()])[:n]
    q = np.zeros(n, dtype=A.CAPTURE_QUERY_DTYPE)
    m = len(head)
    q[:m] = head
    k = n - m
    q["p"][m:] = rng.uniform(-1.75, 2.25, (k, 3))
    q["d"][m:] = rng.normal(size=(k, 3)) * 2.0 ** rng.integers(-3, 4, (k, 1))
    q["alpha"][m:] = rng.uniform(-0.1, 1.2, k)
    return q


def shade_environment(C, chain, seed=11):
    """the dict of _ibl_cases.environment (grid (2, 2, 2), maps T = 1, table 4 x 4) with the records of a set of C captures"""
    env = IC.environment((2, 2, 2), chain, (4, 4), 1, seed=seed)
    env["levels"], env["records"] = records(C, chain)
    return env


def native_env(env, parts, C, arrays=None):
    """the rtr_shade_env of the dict: chain = the level-major array, n_records = one capture's count"""
    e = IC.native_env(env, parts, arrays)
    e.n_records = len(env["records"]) // C
    return e


def no_reach_volumes():
    """one volume that reaches none of the test queries"""
    return np.array([V2], dtype=A.CAPTURE_VOLUME_DTYPE)


# ---- the meaning test: a cube whose texels hold the wall point they see ----
ROOM_CENTRE, ROOM_HALF, ROOM_FACE = (1.0, -0.5, 2.0), 1.5, 8


def room_volume(centre=ROOM_CENTRE, half=ROOM_HALF):
    lo, hi = tuple(c - half for c in centre), tuple(c + half for c in centre)
    return np.array([volume(centre, lo, hi, lo, hi, 0.0)], dtype=A.CAPTURE_VOLUME_DTYPE)


def wall_point_cube(S=ROOM_FACE, centre=ROOM_CENTRE, half=ROOM_HALF):
    """6 S^2 records: v = centre + half * d0 of the texel's centre"""
    rec = np.zeros((6, S, S), dtype=A.GATHER_OUT_DTYPE)
    rec["count"], rec["valid"] = 1, 1
    for f in range(6):
        for b in range(S):
            for a in range(S):
                d0 = FR.face_d0(f, (2.0 * (a + 0.5)) / S - 1.0, (2.0 * (b + 0.5)) / S - 1.0)
                rec["v"][f, b, a] = [centre[x] + half * d0[x] for x in range(3)]
    return rec.reshape(-1)


def room_queries(seed, n=300, centre=ROOM_CENTRE, half=ROOM_HALF):
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=A.CAPTURE_QUERY_DTYPE)
    q["p"] = np.array(centre) + rng.uniform(-0.9 * half, 0.9 * half, (n, 3))
    q["d"] = rng.normal(size=(n, 3))
    return q


def room_classes(q, S=ROOM_FACE, centre=ROOM_CENTRE, half=ROOM_HALF):
    """per query: (hit point p + t d, kept by the seam rule, the lookup along d itself lands on another face)"""
    import _capture_set_ref as SR
    vol = room_volume(centre, half)[0]
    hit, kept, other = np.zeros((len(q), 3)), np.zeros(len(q), bool), np.zeros(len(q), bool)
    for k in range(len(q)):
        p, d = [float(x) for x in q["p"][k]], [float(x) for x in q["d"][k]]
        dk, t = SR.project(vol, p, d)
        hit[k] = [p[a] + t * d[a] for a in range(3)]
        f, u, v = CR.face_uv(np.array(dk))
        kept[k] = max(abs(u), abs(v)) <= 1.0 - 1.0 / S
        other[k] = CR.face_uv(np.array(d))[0] != f
    return hit, kept, other
