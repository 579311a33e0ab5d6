"""Numpy / Python restatement of the probe distance maps, written from the contract in include/rtr_hip.h
(rtr_probe_depth*, rtr_octa_*, rtr_probe_lookup_visible*): the octahedral map, the ray through a texel, the reduction, the
folded fetch and the visibility-weighted grid lookup.  Only + - * / sqrt, |x| and compares, in the header's operation
order, so the bits are the library's.  The seed and the xorshift32 step are the captures' (tests/_capture_ref.py), the
reduction the gathers' (tests/_gather_ref.py), the axis rule and the irradiance the probes' (tests/_probe_ref.py).  Test
infrastructure only."""
import math

import numpy as np

import _capture_ref as CR
import _gather_ref as GR
import _probe_ref as PR

M32 = GR.M32
FLOOR = 2.0 ** -20


def sg(t):
    return 1.0 if t >= 0 else -1.0


def decode(u, v):
    """DECODE: the unit direction (x, y, z) of the point (u, v) of the square"""
    z = (1.0 - abs(u)) - abs(v)
    if z >= 0:
        x, y = u, v
    else:
        x, y = (1.0 - abs(v)) * sg(u), (1.0 - abs(u)) * sg(v)
    r = 1.0 / math.sqrt((x * x + y * y) + z * z)
    return r * x, r * y, r * z


def encode(x, y, z):
    """ENCODE: the point (ox, oy) of the square of a direction that need not be unit"""
    s = (abs(x) + abs(y)) + abs(z)
    ox, oy = x / s, y / s
    if z < 0:
        ox, oy = (1.0 - abs(oy)) * sg(ox), (1.0 - abs(ox)) * sg(oy)
    return ox, oy


def rays(n_probes, map_size, samples, seed=0, point_base=0, jitter=1):
    """(directions [n, T, T, N, 3], generator states after the draws [n, T, T, N] uint32) of every ray of a call; axes:
    probe, row b, column a, sample s"""
    n, T, N = int(n_probes), int(map_size), int(samples)
    k = ((np.arange(n, dtype=np.uint64) + np.uint64(point_base)) & M32).reshape(n, 1, 1, 1)
    b = np.arange(T, dtype=np.uint64).reshape(1, T, 1, 1)
    a = np.arange(T, dtype=np.uint64).reshape(1, 1, T, 1)
    s = np.arange(N, dtype=np.uint64).reshape(1, 1, 1, N)
    e = b * np.uint64(T) + a
    state = np.broadcast_to(CR.sample_seed(seed, T * T, e, k, s), (n, T, T, N)).copy()
    if jitter:
        state = GR.xorshift(state)
        ju = state.astype(np.float64) * 2.0 ** -32
        state = GR.xorshift(state)
        jv = state.astype(np.float64) * 2.0 ** -32
    else:
        ju = jv = np.full(state.shape, 0.5)
    u = (2.0 * (a.astype(np.float64) + ju)) / float(T) - 1.0
    v = (2.0 * (b.astype(np.float64) + jv)) / float(T) - 1.0
    d = np.zeros(state.shape + (3,))
    for idx in np.ndindex(state.shape):
        d[idx] = decode(float(u[idx]), float(v[idx]))
    return d, state.astype(np.uint32)


def reduce(hit, t, front_face, t_max):
    """The PROBE_DEPTH_DTYPE records [...] of the maps whose rays [..., N] returned (hit, t, front_face): x_s = hit ? t :
    t_max, the gathers' reduction over the two sums and the two counts"""
    import _golden as G
    hit = np.asarray(hit) != 0
    shape = hit.shape
    x = np.where(hit, np.asarray(t, dtype=np.float64), float(t_max)).reshape(-1, shape[-1])
    back = (hit & (np.asarray(front_face) == 0)).reshape(-1, shape[-1])
    out = np.zeros(len(x), dtype=G.A.PROBE_DEPTH_DTYPE)
    out["mean"], out["mean2"] = GR.reduce(x), GR.reduce(x * x)
    out["hits"] = GR.reduce(hit.reshape(-1, shape[-1]).astype(np.int32), divide=False)
    out["back"] = GR.reduce(back.astype(np.int32), divide=False)
    out["valid"] = 1
    return out.reshape(shape[:-1])


def _axis(c, T):
    """(i0, w0, w1) of one axis of FETCH: no clamp"""
    g = ((c + 1.0) * float(T)) * 0.5 - 0.5
    i0 = -1 if g < 0 else int(g)
    t = g - float(i0)
    return i0, 1.0 - t, t


def fold(ia, ib, T):
    """the texel the tap (ia, ib), -1 <= ia, ib <= T, reads"""
    if ia < 0:
        ia, ib = 0, T - 1 - ib
    elif ia > T - 1:
        ia, ib = T - 1, T - 1 - ib
    if ib < 0:
        ib, ia = 0, T - 1 - ia
    elif ib > T - 1:
        ib, ia = T - 1, T - 1 - ia
    return ia, ib


def fetch(depth_map, d):
    """FETCH: (m1, m2, ok) of the map ``depth_map`` (PROBE_DEPTH_DTYPE [T, T]) along d"""
    T = depth_map.shape[0]
    ox, oy = encode(float(d[0]), float(d[1]), float(d[2]))
    ia0, *wa = _axis(ox, T)
    ib0, *wb = _axis(oy, T)
    m1, m2, ok = 0.0, 0.0, True
    for db in range(2):
        for da in range(2):
            w = wa[da] * wb[db]
            if w > 0:
                ia, ib = fold(ia0 + da, ib0 + db, T)
                t = depth_map[ib, ia]
                ok = ok and t["valid"] != 0
                m1 = m1 + w * float(t["mean"])
                m2 = m2 + w * float(t["mean2"])
    return m1, m2, ok


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def corner_weight(p, w, pb, P, depth_map):
    """(wb, c, branch) of the corner whose probe stands at P: the wrap weight, the visibility and which rule of the header
    gave it ("r2 == 0", "!ok", "r <= m1", "den == 0" or "chebyshev")"""
    e = [P[a] - p[a] for a in range(3)]
    el2 = _dot(e, e)
    cosn = _dot(e, w) / math.sqrt(el2) if el2 > 0 else 0.0
    h = (cosn + 1.0) * 0.5
    wb = h * h + 0.2
    dv = [pb[a] - P[a] for a in range(3)]
    r2 = _dot(dv, dv)
    if not r2 > 0:
        return wb, 1.0, "r2 == 0"
    r = math.sqrt(r2)
    m1, m2, ok = fetch(depth_map, dv)
    if not ok:
        return wb, 1.0, "!ok"
    if r <= m1:
        return wb, 1.0, "r <= m1"
    var = abs(m2 - m1 * m1)
    dd = r - m1
    den = var + dd * dd
    if not den > 0:
        return wb, 0.0, "den == 0"
    c = var / den
    return wb, (c * c) * c, "chebyshev"


def lookup_visible(origin, spacing, dims, probes, depth, normal_bias, points, normals, weights=None):
    """rtr_probe_lookup_visible: a GATHER_OUT_DTYPE array for the queries (points [n, 3], normals [n, 3]) in the grid whose
    probes (PROBE_SH_DTYPE) and maps (``depth``: PROBE_DEPTH_DTYPE [probes, T, T]) lie in the header's order.  ``weights``:
    a list that receives per query the (probe index, tri, wb, c, wv, branch, floored) of every candidate corner."""
    import _golden as G
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(points), dtype=G.A.GATHER_OUT_DTYPE)
    with np.errstate(invalid="ignore"):  # an invalid tap may hold NaN: its sum is never the result
        for q in range(len(points)):
            p = [float(x) for x in points[q]]
            n = [float(x) for x in normals[q]]
            rn = 1.0 / math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
            w = [rn * n[0], rn * n[1], rn * n[2]]
            pb = [p[a] + normal_bias * w[a] for a in range(3)]
            ax = [PR.axis(p[a], float(origin[a]), float(spacing[a]), int(dims[a])) for a in range(3)]
            wsum, used = 0.0, 0
            acc = np.zeros((9, 3))
            seen = []
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        i = (min(ax[0][0] + dx, dims[0] - 1), min(ax[1][0] + dy, dims[1] - 1), min(ax[2][0] + dz, dims[2] - 1))
                        tri = (ax[0][1 + dx] * ax[1][1 + dy]) * ax[2][1 + dz]
                        pi = i[0] + dims[0] * (i[1] + dims[1] * i[2])
                        probe = probes[pi]
                        if not (tri > 0 and probe["valid"] != 0):
                            continue
                        P = [float(origin[a]) + float(i[a]) * float(spacing[a]) for a in range(3)]
                        wb, c, branch = corner_weight(p, w, pb, P, depth[pi])
                        wv = wb * c
                        floored = not wv >= FLOOR
                        if floored:
                            wv = FLOOR
                        wgt = tri * wv
                        wsum = wsum + wgt
                        acc = acc + wgt * probe["c"]
                        used += 1
                        seen.append((pi, tri, wb, c, wv, branch, floored))
            if weights is not None:
                weights.append(seen)
            if used:
                out["v"][q] = PR.irradiance((1.0 / wsum) * acc, normals[q])
                out["count"][q], out["valid"][q] = used, 1
    return out


def flat_maps(n_probes, T, distance):
    """maps [n, T, T] that see ``distance`` in every direction without spread: mean = distance, mean2 = distance^2"""
    import _golden as G
    d = np.zeros((n_probes, T, T), dtype=G.A.PROBE_DEPTH_DTYPE)
    d["mean"], d["mean2"], d["valid"] = distance, distance * distance, 1
    return d


def plane_map(T, axis, offset, t_max, spread=0.0):
    """the map [T, T] of a probe that sees the plane x[axis] = offset (relative to the probe, offset != 0) and nothing else:
    the texel centre's distance offset / d[axis] where the ray meets it within t_max, else t_max; mean2 = mean^2 + spread"""
    import _golden as G
    m = np.zeros((T, T), dtype=G.A.PROBE_DEPTH_DTYPE)
    for b in range(T):
        for a in range(T):
            d = decode((2.0 * (a + 0.5)) / T - 1.0, (2.0 * (b + 0.5)) / T - 1.0)
            t = offset / d[axis] if d[axis] * offset > 0 else math.inf
            x = t if t < t_max else t_max
            m[b, a] = (x, x * x + spread, 1 if t < t_max else 0, 0, 1, 0)
    return m
