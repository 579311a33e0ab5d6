"""numpy restatement of the image-based shading contract (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*), written from the
header: the table's quadrature with its lane-order sums, the bilinear fetch, and the shader over the restatements of the
lookups it composes (_probe_ref, _probe_depth_ref, _cube_filter_ref).  Only + - * / sqrt: the bits of the library."""
import math

import numpy as np

import _cube_filter_ref as CF
import _probe_depth_ref as PD
import _probe_ref as PR

PI = 3.1415926535897932385
DIFFUSE, SPECULAR = 1, 2


def entry_at(mu, rough, M):
    """(a, b) of the quadrature with M nodes per axis at (mu, rough) themselves"""
    mu, rough = float(mu), float(rough)
    alpha = rough * rough
    a2 = alpha * alpha
    k = alpha * 0.5
    omk = 1.0 - k
    Vx, Vz = math.sqrt(1.0 - mu * mu), mu
    g1v = mu / (mu * omk + k)
    j = np.arange(2 * M * M)
    sx = np.where(j < M * M, 1.0, -1.0)
    jj = j % (M * M)
    s = (jj // M + 0.5) / M
    t = (jj % M + 0.5) / M
    with np.errstate(all="ignore"):  # a node that is not USED may divide by zero: its terms are never added
        den = a2 + (1.0 - a2) * (s * s)
        c2 = (s * s) / den
        Hz = np.sqrt(c2)
        sh = np.sqrt(np.maximum(1.0 - c2, 0.0))
        q = 1.0 + t * t
        Hx = sh * (sx * ((1.0 - t * t) / q))
        wphi = 1.0 / q
        vh = Vx * Hx + Vz * Hz
        nl = (2.0 * vh) * Hz - Vz
        used = (nl > 0) & (vh > 0)
        g = g1v * (nl / (nl * omk + k))
        e = (((g * nl) * (4.0 * vh)) * np.sqrt(den)) / ((4.0 * mu) * nl + 0.0001)
        x = 1.0 - vh
        fc = ((x * x) * (x * x)) * x
        terms = [wphi * s, np.where(used, wphi * (e * (1.0 - fc)), 0.0), np.where(used, wphi * (e * fc), 0.0)]
    sums = []
    for term in terms:  # lane l meets j = l, l + 64, ... in increasing order; + 0.0 where it has no term changes no bit
        rows = np.zeros(-(-len(term) // 64) * 64)
        rows[:len(term)] = term
        lanes = np.zeros(64)
        for row in rows.reshape(-1, 64):
            lanes = lanes + row
        off = 32
        while off:
            lanes[:off] = lanes[:off] + lanes[off:2 * off]
            off >>= 1
        sums.append(float(lanes[0]))
    W, A, B = sums
    return (1.0 / W) * A, (1.0 / W) * B


def entry(r, c, n_mu, n_rough, M):
    """ENTRY (r, c)"""
    return entry_at((c + 0.5) / n_mu, (r + 0.5) / n_rough, M)


def table(n_mu, n_rough, M):
    """the table [n_rough, n_mu, 2] of doubles"""
    return np.array([[entry(r, c, n_mu, n_rough, M) for c in range(n_mu)] for r in range(n_rough)], dtype=np.float64)


def fetch(tab, mu, rough):
    """FETCH: (a, b) at (mu, rough) in tab [n_rough, n_mu, 2]"""
    n_rough, n_mu = tab.shape[:2]
    ic, wc0, wc1 = PR.axis(float(mu) * n_mu - 0.5, 0.0, 1.0, n_mu)
    ir, wr0, wr1 = PR.axis(float(rough) * n_rough - 0.5, 0.0, 1.0, n_rough)
    a = b = 0.0
    for dr in (0, 1):
        for dc in (0, 1):
            w = (wc0, wc1)[dc] * (wr0, wr1)[dr]
            if w > 0:
                t = tab[min(ir + dr, n_rough - 1), min(ic + dc, n_mu - 1)]
                a, b = a + w * float(t[0]), b + w * float(t[1])
    return a, b


def query_bad(q):
    """BAD of one SHADE_QUERY_DTYPE record"""
    fields = [float(x) for name in ("p", "n", "v", "base") for x in q[name]] + [float(q["roughness"]), float(q["metallic"])]
    if not all(math.isfinite(x) for x in fields):
        return True
    with np.errstate(over="ignore"):
        for name in ("n", "v"):
            x = q[name]
            length = float(np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]))
            if not 0.0 < length < math.inf:
                return True
    return False


def shade_one(env, q):
    """(v [3], count, valid) of one query that is not BAD.  env: dict with parts, tab [n_rough, n_mu, 2], and per part
    origin / spacing / dims / probes / depth (or None) / normal_bias, levels [(face_size, offset, alpha)] / records"""
    zero = (np.zeros(3), 0, 0)
    n = [float(x) for x in q["n"]]
    v = [float(x) for x in q["v"]]
    base = [float(x) for x in q["base"]]
    metallic = float(q["metallic"])
    rn = 1.0 / math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    rv = 1.0 / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    N = [rn * x for x in n]
    Vd = [rv * x for x in v]
    mu = (N[0] * Vd[0] + N[1] * Vd[1]) + N[2] * Vd[2]
    muc = mu if mu > 0.0 else 0.0
    rough = min(max(float(q["roughness"]), 0.01), 1.0)
    alpha = rough * rough
    parts = env["parts"]
    E, X, count = np.zeros(3), np.zeros(3), 0
    if parts & DIFFUSE:
        if env.get("depth") is not None:
            rec = PD.lookup_visible(env["origin"], env["spacing"], env["dims"], env["probes"], env["depth"], env["normal_bias"],
                                    [q["p"]], [q["n"]])[0]
        else:
            rec = PR.lookup(env["origin"], env["spacing"], env["dims"], env["probes"], [q["p"]], [q["n"]])[0]
        if not rec["valid"]:
            return zero
        E, count = rec["v"].copy(), int(rec["count"])
    if parts & SPECULAR:
        R = np.array([(2.0 * mu) * N[a] - Vd[a] for a in range(3)])
        x = CF.chain_lookup_one(env["levels"], env["records"], R, alpha)
        if not x[2]:
            return zero
        X, count = np.asarray(x[0], dtype=np.float64), count + int(x[1])
    a, b = fetch(env["tab"], muc, rough)
    out = np.zeros(3)
    om = 1.0 - metallic
    for ch in range(3):
        F0 = om * 0.04 + metallic * base[ch]
        kS = F0 * a + b
        kD = (1.0 - kS) * om
        diffuse = ((kD * base[ch]) * float(E[ch])) / PI
        specular = float(X[ch]) * kS
        out[ch] = diffuse if parts == DIFFUSE else specular if parts == SPECULAR else diffuse + specular
    return out, count, 1


def shade(env, queries, out_dtype):
    """rtr_shade_ibl_device: a GATHER_OUT_DTYPE array; a BAD query has the all-zero record"""
    out = np.zeros(len(queries), dtype=out_dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, q in enumerate(queries):
            if not query_bad(q):
                out["v"][k], out["count"][k], out["valid"][k] = shade_one(env, q)
    return out


def brute_force(mu, rough, n_cos=3000, n_phi=6000, rows=250):
    """(a, b) by integrating the reference's own specular term D G (F-part) n.l / (4 n.v n.l + 0.0001) over the light
    directions of the upper hemisphere, a midpoint grid in (cos theta, phi): independent of the table's quadrature"""
    alpha = rough * rough
    a2 = alpha * alpha
    k = (rough * rough) / 2.0
    V = np.array([math.sqrt(1.0 - mu * mu), 0.0, mu])
    phi = (np.arange(n_phi) + 0.5) * (2.0 * math.pi / n_phi)
    cp, sp = np.cos(phi)[None, :], np.sin(phi)[None, :]
    A = B = 0.0
    for r0 in range(0, n_cos, rows):
        ct = ((np.arange(r0, min(r0 + rows, n_cos)) + 0.5) / n_cos)[:, None]
        st = np.sqrt(1.0 - ct * ct)
        Lx, Ly, Lz = st * cp, st * sp, ct + 0.0 * cp
        Hx, Hy, Hz = Lx + V[0], Ly + V[1], Lz + V[2]
        rl = 1.0 / np.sqrt(Hx * Hx + Hy * Hy + Hz * Hz)
        Hx, Hz = rl * Hx, rl * Hz
        nh = np.maximum(Hz, 0.0)
        vh = np.maximum(Hx * V[0] + Hz * V[2], 0.0)
        d = nh * nh * (a2 - 1.0) + 1.0
        D = a2 / (math.pi * d * d)
        G = (Lz / (Lz * (1.0 - k) + k)) * (mu / (mu * (1.0 - k) + k))
        f = D * G * Lz / (4.0 * mu * Lz + 0.0001)
        fc = (1.0 - vh) ** 5
        A += float((f * (1.0 - fc)).sum())
        B += float((f * fc).sum())
    dw = (1.0 / n_cos) * (2.0 * math.pi / n_phi)
    return A * dw, B * dw
