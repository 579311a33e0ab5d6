"""numpy restatement of the capture-set contract (include/rtr_hip.h: rtr_capture_set*), written from the header: the reach
test and the weight of a volume, the box projection, the blend in capture order, the fallback, and the set form of the
shader over the restatements of the lookups it composes (_cube_filter_ref, _ibl_ref).  Scalars are Python floats, so every
product is rounded before its add: the bits of the library."""
import math

import numpy as np

import _cube_filter_ref as CF
import _ibl_ref as IR
import _probe_depth_ref as PD
import _probe_ref as PR

INF = math.inf


def fmin(a, b):
    """min(a, b) of the header: b when b < a, else a"""
    return b if b < a else a


def chain_of(levels, records, C, k):
    """the chain of capture k of a level-major set array, in the chain layout of ``levels``"""
    parts = []
    for S, at, _ in levels:
        F = 6 * S * S
        parts.append(records[at * C + k * F:at * C + (k + 1) * F])
    return np.concatenate(parts)


def query_bad(p, d, alpha):
    if not all(math.isfinite(float(x)) for x in (*p, *d, alpha)):
        return True
    d = [float(x) for x in d]
    with np.errstate(over="ignore"):
        length = float(np.sqrt(np.float64((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    return not 0.0 < length < INF


def weight(vol, p):
    """w of the volume at p, or None when it does not reach p"""
    m = p[0] - float(vol["reach_lo"][0])
    m = fmin(m, float(vol["reach_hi"][0]) - p[0])
    for a in (1, 2):
        m = fmin(m, p[a] - float(vol["reach_lo"][a]))
        m = fmin(m, float(vol["reach_hi"][a]) - p[a])
    if m < 0:
        return None
    fade = float(vol["fade"])
    w = 1.0 if fade == 0 else fmin(m / fade, 1.0)
    return w if w > 0 else None


def project(vol, p, d):
    """(dk [3], t): the ray (p, d) met with the proxy box, as seen from the centre"""
    t = INF
    for a in range(3):
        if d[a] > 0:
            t = fmin(t, (float(vol["proxy_hi"][a]) - p[a]) / d[a])
        elif d[a] < 0:
            t = fmin(t, (float(vol["proxy_lo"][a]) - p[a]) / d[a])
    return [(p[a] + t * d[a]) - float(vol["centre"][a]) for a in range(3)], t


def set_lookup_one(volumes, fallback, levels, records, p, d, alpha):
    """SET LOOKUP: (v [3], count, valid).  volumes: CAPTURE_VOLUME_DTYPE records; records: the level-major array"""
    zero = (np.zeros(3), 0, 0)
    if query_bad(p, d, alpha):
        return zero
    p, d, alpha = [float(x) for x in p], [float(x) for x in d], float(alpha)
    C = len(volumes)
    acc, wsum, count, used = [0.0, 0.0, 0.0], 0.0, 0, 0
    with np.errstate(all="ignore"):
        for k in range(C):
            w = weight(volumes[k], p)
            if w is None:
                continue
            dk, _ = project(volumes[k], p, d)
            X = CF.chain_lookup_one(levels, chain_of(levels, records, C, k), np.array(dk), alpha)
            if not X[2]:
                return zero
            for ch in range(3):
                acc[ch] = acc[ch] + w * float(X[0][ch])
            wsum, count, used = wsum + w, count + int(X[1]), used + 1
        if used > 0:
            r = 1.0 / wsum
            return np.array([r * acc[0], r * acc[1], r * acc[2]]), count, 1
        if fallback >= 0:
            X = CF.chain_lookup_one(levels, chain_of(levels, records, C, fallback), np.array(d), alpha)
            return np.asarray(X[0], dtype=np.float64), int(X[1]), int(X[2])
    return zero


def set_lookup(volumes, fallback, levels, records, queries, out_dtype):
    """rtr_capture_set_lookup: a GATHER_OUT_DTYPE array for the CAPTURE_QUERY_DTYPE queries"""
    out = np.zeros(len(queries), dtype=out_dtype)
    for k, q in enumerate(queries):
        out["v"][k], out["count"][k], out["valid"][k] = set_lookup_one(volumes, fallback, levels, records, q["p"], q["d"], q["alpha"])
    return out


def shade_one(env, volumes, fallback, q):
    """rtr_shade_ibl_set_one of a query that is not BAD: the shader of the header with the SPECULAR record from the set.
    env as for _ibl_ref.shade_one, its records the level-major array"""
    zero = (np.zeros(3), 0, 0)
    n, v = [float(x) for x in q["n"]], [float(x) for x in q["v"]]
    base, metallic = [float(x) for x in q["base"]], float(q["metallic"])
    rn = 1.0 / math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    rv = 1.0 / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    N, Vd = [rn * x for x in n], [rv * x for x in v]
    mu = (N[0] * Vd[0] + N[1] * Vd[1]) + N[2] * Vd[2]
    muc = mu if mu > 0.0 else 0.0
    rough = min(max(float(q["roughness"]), 0.01), 1.0)
    parts = env["parts"]
    E, X, count = np.zeros(3), np.zeros(3), 0
    if parts & IR.DIFFUSE:
        if env.get("depth") is not None:
            rec = PD.lookup_visible(env["origin"], env["spacing"], env["dims"], env["probes"], env["depth"], env["normal_bias"],
                                    [q["p"]], [q["n"]])[0]
        else:
            rec = PR.lookup(env["origin"], env["spacing"], env["dims"], env["probes"], [q["p"]], [q["n"]])[0]
        if not rec["valid"]:
            return zero
        E, count = rec["v"].copy(), int(rec["count"])
    if parts & IR.SPECULAR:
        R = [(2.0 * mu) * N[a] - Vd[a] for a in range(3)]
        x = set_lookup_one(volumes, fallback, env["levels"], env["records"], q["p"], R, rough * rough)
        if not x[2]:
            return zero
        X, count = x[0], count + x[1]
    a, b = IR.fetch(env["tab"], muc, rough)
    out = np.zeros(3)
    om = 1.0 - metallic
    for ch in range(3):
        F0 = om * 0.04 + metallic * base[ch]
        kS = F0 * a + b
        kD = (1.0 - kS) * om
        diffuse = ((kD * base[ch]) * float(E[ch])) / IR.PI
        specular = float(X[ch]) * kS
        out[ch] = diffuse if parts == IR.DIFFUSE else specular if parts == IR.SPECULAR else diffuse + specular
    return out, count, 1


def shade(env, volumes, fallback, queries, out_dtype):
    """rtr_shade_ibl_set_device: a GATHER_OUT_DTYPE array; a BAD query has the all-zero record"""
    out = np.zeros(len(queries), dtype=out_dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, q in enumerate(queries):
            if not IR.query_bad(q):
                out["v"][k], out["count"][k], out["valid"][k] = shade_one(env, volumes, fallback, q)
    return out
