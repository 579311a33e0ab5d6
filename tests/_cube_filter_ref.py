"""Numpy / Python restatement of the filtered cube maps, written from the contract in include/rtr_hip.h (rtr_cube_filter*,
rtr_cube_chain_*): the GGX-weighted sum over all source texels with its 64 lanes and xor tree, the chain plan, the
seam-aware lookup of a level and the blend of two levels.  Only + - * / sqrt and compares, in the header's operation
order, so the bits are the library's; it calls nothing of the library.  Test infrastructure only."""
import math

import numpy as np

import _capture_ref as CR

LANES = 64


def face_d0(f, u, v):
    """the face table: the un-normalised direction of (u, v) on face f (numbers or arrays)"""
    one = np.ones_like(u) if isinstance(u, np.ndarray) else 1.0
    return ((one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one))[f]


def centres(S):
    """(unit centre directions [6 S^2, 3], solid-angle weights dw [6 S^2]) of the texels of an S x S cube in record order"""
    i = np.arange(S, dtype=np.float64)
    c = (2.0 * (i + 0.5)) / float(S) - 1.0
    u, v = np.broadcast_to(c[None, :], (S, S)), np.broadcast_to(c[:, None], (S, S))  # column a -> u, row b -> v
    L, dw = np.zeros((6, S, S, 3)), np.zeros((6, S, S))
    for f in range(6):
        x, y, z = (np.broadcast_to(np.asarray(t, dtype=np.float64), (S, S)) for t in face_d0(f, u, v))
        r2 = x * x + y * y + z * z
        root = np.sqrt(r2)
        r = 1.0 / root
        L[f, ..., 0], L[f, ..., 1], L[f, ..., 2] = r * x, r * y, r * z
        dw[f] = 1.0 / (r2 * root)
    return L.reshape(-1, 3), dw.reshape(-1)


def filter_cube(texels, face_out, alpha, cos_cut):
    """rtr_cube_filter of ONE cube: GATHER_OUT_DTYPE records [6, face_out, face_out] from ``texels`` [6, S_in, S_in]"""
    S_in = texels.shape[1]
    src = texels.reshape(-1)
    L, dw = centres(S_in)
    R, _ = centres(face_out)
    n_out, n_in = len(R), len(L)
    rows = -(-n_in // LANES)
    pad = rows * LANES - n_in

    def lanes(a):  # [n_in, ...] -> [rows, 64, ...]: lane l meets j = l, l + 64, ...
        return np.concatenate([a, np.zeros((pad,) + a.shape[1:], dtype=a.dtype)]).reshape((rows, LANES) + a.shape[1:])

    Ll, dwl, vl = lanes(L), lanes(dw), lanes(np.ascontiguousarray(src["v"]))
    invalid = lanes((src["valid"] == 0).astype(np.int64))
    there = lanes(np.ones(n_in, dtype=bool))
    a2m1 = alpha * alpha - 1.0
    acc = np.zeros((n_out, LANES, 3))
    wsum = np.zeros((n_out, LANES))
    count = np.zeros((n_out, LANES), dtype=np.int64)
    bad = np.zeros((n_out, LANES), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):  # NaN texels, empty sums: never the result
        for r in range(rows):
            c = (R[:, None, 0] * Ll[r, None, :, 0] + R[:, None, 1] * Ll[r, None, :, 1]) + R[:, None, 2] * Ll[r, None, :, 2]
            used = (c > cos_cut) & there[r][None, :]
            h2 = (1.0 + c) * 0.5
            den = h2 * a2m1 + 1.0
            w = (c * dwl[r][None, :]) / (den * den)
            acc = np.where(used[..., None], acc + w[..., None] * vl[r][None, :, :], acc)
            wsum = np.where(used, wsum + w, wsum)
            count += used
            bad += used & (invalid[r][None, :] != 0)
        off = LANES // 2
        while off:
            idx = np.arange(LANES) ^ off
            acc, wsum, count, bad = acc + acc[:, idx], wsum + wsum[:, idx], count + count[:, idx], bad + bad[:, idx]
            off //= 2
        acc, wsum, count, bad = acc[:, 0], wsum[:, 0], count[:, 0], bad[:, 0]
        ok = (count > 0) & (bad == 0) & (wsum > 0.0) & (wsum < np.inf)
        v = (1.0 / wsum)[:, None] * acc
    out = np.zeros(n_out, dtype=texels.dtype)
    out["v"] = np.where(ok[:, None], v, 0.0)
    out["count"], out["valid"] = np.where(ok, count, 0), ok
    return out.reshape(6, face_out, face_out)


def filter_cubes(texels, face_out, alpha, cos_cut):
    """the same for [n, 6, S_in, S_in]"""
    return np.stack([filter_cube(t, face_out, alpha, cos_cut) for t in texels])


def plan(face_size, n_levels):
    """rtr_cube_chain_plan: ([(face_size, offset, alpha)], n_records)"""
    levels, at = [], 0
    for i in range(n_levels):
        s = max(face_size >> i, 1)
        r = float(i) / (n_levels - 1) if n_levels > 1 else 0.0
        levels.append((s, at, r * r))
        at += 6 * s * s
    return levels, at


def tap(f, ia, ib, S):
    """(face, row, column) of the texel the tap (ia, ib) of face f reads"""
    if 0 <= ia < S and 0 <= ib < S:
        return f, ib, ia
    u1, v1 = (2.0 * (ia + 0.5)) / float(S) - 1.0, (2.0 * (ib + 0.5)) / float(S) - 1.0
    f2, u2, v2 = CR.face_uv(face_d0(f, u1, v1))
    col = min(max(int(((u2 + 1.0) * float(S)) * 0.5), 0), S - 1)
    row = min(max(int(((v2 + 1.0) * float(S)) * 0.5), 0), S - 1)
    return f2, row, col


def seam_lookup(level, d):
    """(v [3], count, valid) of the seam-aware lookup of the direction d in the records ``level`` [6, S, S]"""
    S = level.shape[1]
    fuv = CR.face_uv(d)
    if fuv is None:
        return np.zeros(3), 0, 0
    f, u, v = fuv
    i0, w = [], []
    for c in (u, v):
        g = ((c + 1.0) * float(S)) * 0.5 - 0.5
        fl = math.floor(g)
        t = g - float(fl)
        i0.append(fl)
        w.append((1.0 - t, t))
    acc = np.zeros(3)
    used, ok = 0, True
    for db in range(2):
        for da in range(2):
            wc = w[0][da] * w[1][db]
            if wc > 0:
                t = level[tap(f, i0[0] + da, i0[1] + db, S)]
                ok = ok and t["valid"] != 0
                used += 1
                acc = acc + wc * t["v"]
    if not ok:
        return np.zeros(3), 0, 0
    return acc, used, 1


def chain_lookup_one(levels, records, d, alpha):
    """rtr_cube_chain_lookup_one: levels = [(face_size, offset, alpha)], records the flat GATHER_OUT_DTYPE array"""
    zero = (np.zeros(3), 0, 0)
    if CR.face_uv(d) is None or not math.isfinite(alpha):
        return zero
    n = len(levels)
    a = min(max(float(alpha), levels[0][2]), levels[-1][2])
    i = max(k for k in range(n) if k == 0 or levels[k][2] <= a)
    if n >= 2:
        i = min(i, n - 2)
    t = (a - levels[i][2]) / (levels[i + 1][2] - levels[i][2]) if n >= 2 else 0.0

    def level(k):
        S, at, _ = levels[k]
        return records[at:at + 6 * S * S].reshape(6, S, S)

    x0 = seam_lookup(level(i), d)
    if t == 0:
        return x0
    x1 = seam_lookup(level(i + 1), d)
    if not (x0[2] and x1[2]):
        return zero
    return (1.0 - t) * x0[0] + t * x1[0], x0[1] + x1[1], 1


def chain_lookup(levels, records, queries):
    """rtr_cube_chain_lookup: a GATHER_OUT_DTYPE array for the CUBE_QUERY_DTYPE queries"""
    out = np.zeros(len(queries), dtype=records.dtype)
    with np.errstate(invalid="ignore"):
        for k, q in enumerate(queries):
            out["v"][k], out["count"][k], out["valid"][k] = chain_lookup_one(levels, records, q["d"], float(q["alpha"]))
    return out
