/*
 * rt_ibl.h -- image-based shading (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*): the arithmetic of that contract, written
 * once for host (the _one forms, the entries' checks) and device, and the host side of an rtr_shade_env: its rules, the
 * staging of its arrays and the overlap test of the _device forms, which rtr_ibl.hip and rtr_preview.hip share.  The two
 * kernels are rt_ibl_kernels.h's; rtr_preview.hip composes shade_ibl_one from here.  The lookups the shader composes are
 * rt_render.h's: nothing of them is restated here.
 */
#pragma once

#include "rt_render.h"

#define RTR_BRDF_MAX 256 /* n_mu, n_rough and nodes at most */

inline const char* brdf_params_why(const rtr_brdf_params* p) {
    if (!p) return "null brdf params";
    if (p->n_mu < 1 || p->n_mu > RTR_BRDF_MAX || p->n_rough < 1 || p->n_rough > RTR_BRDF_MAX) return "n_mu or n_rough outside 1 .. 256";
    if (p->nodes < 1 || p->nodes > RTR_BRDF_MAX) return "nodes outside 1 .. 256";
    if (p->pad != 0 || p->reserved[0] != 0 || p->reserved[1] != 0) return "pad and reserved must be 0";
    return nullptr;
}

/* ---- TABLE: the parts of a node by what they depend on ---- */
struct BrdfRow { /* of the roughness alone */
    double a2, oma2, k, omk;
};
struct BrdfCol { /* of (mu, roughness) */
    double mu, vx, g1v, mu4;
};
struct BrdfS { /* of (s, roughness) */
    double s, hz, sh, rden;
};
struct BrdfT { /* of t alone */
    double cx, wphi;
};
RT_HD BrdfRow brdf_row(int r, int n_rough) {
    const double rough = (r + 0.5) / n_rough;
    const double alpha = rough * rough;
    BrdfRow R;
    R.a2 = alpha * alpha, R.oma2 = 1.0 - R.a2;
    R.k = alpha * 0.5, R.omk = 1.0 - R.k;
    return R;
}
RT_HD BrdfCol brdf_col(int c, int n_mu, const BrdfRow& R) {
    BrdfCol C;
    C.mu = (c + 0.5) / n_mu;
    C.vx = __builtin_sqrt(1.0 - C.mu * C.mu);
    C.g1v = C.mu / (C.mu * R.omk + R.k);
    C.mu4 = 4.0 * C.mu;
    return C;
}
RT_HD BrdfS brdf_s(int i, int M, const BrdfRow& R) {
    BrdfS S;
    S.s = (i + 0.5) / M;
    const double ss = S.s * S.s;
    const double den = R.a2 + R.oma2 * ss;
    const double c2 = ss / den;
    const double x = 1.0 - c2;
    S.hz = __builtin_sqrt(c2);
    S.sh = __builtin_sqrt(x > 0.0 ? x : 0.0);
    S.rden = __builtin_sqrt(den);
    return S;
}
RT_HD BrdfT brdf_t(int i, int M) {
    const double t = (i + 0.5) / M;
    const double tt = t * t;
    const double q = 1.0 + tt;
    BrdfT T;
    T.cx = (1.0 - tt) / q, T.wphi = 1.0 / q;
    return T;
}
/* what a node adds to A and B of one entry (its wphi * s goes to W whether it is USED or not: the caller's line) */
RT_HD void brdf_node(const BrdfRow& R, const BrdfCol& C, const BrdfS& S, const BrdfT& T, double sx, double& A, double& B) {
    const double hx = S.sh * (sx * T.cx);
    const double vh = C.vx * hx + C.mu * S.hz;
    const double nl = (2.0 * vh) * S.hz - C.mu;
    if (!(nl > 0.0 && vh > 0.0)) return;
    const double g = C.g1v * (nl / (nl * R.omk + R.k));
    const double e = (((g * nl) * (4.0 * vh)) * S.rden) / (C.mu4 * nl + 0.0001);
    const double x = 1.0 - vh;
    const double fc = ((x * x) * (x * x)) * x;
    A = A + T.wphi * (e * (1.0 - fc)), B = B + T.wphi * (e * fc);
}
RT_HD rtr_brdf_entry brdf_result(double W, double A, double B) {
    const double r = 1.0 / W;
    rtr_brdf_entry o;
    o.a = r * A, o.b = r * B;
    return o;
}
/* FETCH; mu and rough are finite */
RT_HD rtr_brdf_entry brdf_fetch(int n_mu, int n_rough, const rtr_brdf_entry* __restrict__ table, double mu, double rough) {
    int i0[2];
    double w[2][2];
    probe_axis(mu * n_mu - 0.5, 0.0, 1.0, n_mu, i0[0], w[0][0], w[0][1]);
    probe_axis(rough * n_rough - 0.5, 0.0, 1.0, n_rough, i0[1], w[1][0], w[1][1]);
    rtr_brdf_entry o;
    o.a = 0.0, o.b = 0.0;
    for (int dr = 0; dr < 2; ++dr)
        for (int dc = 0; dc < 2; ++dc) {
            const int ic = i0[0] + dc < n_mu - 1 ? i0[0] + dc : n_mu - 1;
            const int ir = i0[1] + dr < n_rough - 1 ? i0[1] + dr : n_rough - 1;
            const double wc = w[0][dc] * w[1][dr];
            if (wc > 0) {
                const rtr_brdf_entry& t = table[ir * n_mu + ic];
                o.a = o.a + wc * t.a, o.b = o.b + wc * t.b;
            }
        }
    return o;
}

/* ---- SHADE ---- */
struct ShadeK { /* the environment as a kernel argument: the host structs by value, the arrays where the caller runs */
    int parts, visible; /* visible: depth and the two members behind it are set */
    rtr_probe_grid grid;
    const rtr_probe_sh* probes;
    const rtr_probe_depth_texel* depth;
    int T;
    double normal_bias;
    ChainK chain;
    const rtr_gather_out* texels;
    int n_mu, n_rough;
    const rtr_brdf_entry* table;
};
RT_HD bool shade_query_bad(const rtr_shade_query& q, double& nlen, double& vlen) {
    bool ok = __builtin_isfinite(q.roughness) && __builtin_isfinite(q.metallic);
    for (int a = 0; a < 3; ++a)
        ok = ok && __builtin_isfinite(q.p[a]) && __builtin_isfinite(q.n[a]) && __builtin_isfinite(q.v[a]) && __builtin_isfinite(q.base[a]);
    nlen = __builtin_sqrt(q.n[0] * q.n[0] + q.n[1] * q.n[1] + q.n[2] * q.n[2]);
    vlen = __builtin_sqrt(q.v[0] * q.v[0] + q.v[1] * q.v[1] + q.v[2] * q.v[2]);
    return !(ok && nlen > 0.0 && nlen < __builtin_huge_val() && vlen > 0.0 && vlen < __builtin_huge_val());
}
/* rtr_shade_ibl of one query that is not BAD.  The phases follow each other: the diffuse record is down to three doubles
 * and a count before the chain is read.  SET: rtr_shade_ibl_set -- K.texels holds the capture set *S level-major, K.chain the
 * plan of one capture, and the specular record is the set lookup of (q.p, R, alpha); every other line is shared */
template <bool SET = false>
RT_HD rtr_gather_out shade_ibl_one(const ShadeK& K, const rtr_shade_query& q, double nlen, double vlen, const SetK* S = nullptr) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    const double rn = 1 / nlen, rv = 1 / vlen;
    const double N[3] = {rn * q.n[0], rn * q.n[1], rn * q.n[2]};
    const double Vd[3] = {rv * q.v[0], rv * q.v[1], rv * q.v[2]};
    const double mu = (N[0] * Vd[0] + N[1] * Vd[1]) + N[2] * Vd[2];
    const double muc = mu > 0.0 ? mu : 0.0;
    double rough = q.roughness > 0.01 ? q.roughness : 0.01;
    rough = rough < 1.0 ? rough : 1.0;
    double E[3] = {0.0, 0.0, 0.0}, X[3] = {0.0, 0.0, 0.0};
    int count = 0;
    if (K.parts & RTR_SHADE_DIFFUSE) {
        rtr_gather_point gp;
        for (int a = 0; a < 3; ++a) gp.p[a] = q.p[a], gp.n[a] = q.n[a];
        const rtr_gather_out rec = K.visible ? probe_lookup_visible_one(K.grid, K.probes, K.depth, K.T, K.normal_bias, gp, nlen)
                                             : probe_lookup_one(K.grid, K.probes, gp, nlen);
        if (!rec.valid) return o;
        E[0] = rec.v[0], E[1] = rec.v[1], E[2] = rec.v[2], count = rec.count;
    }
    if (K.parts & RTR_SHADE_SPECULAR) {
        rtr_cube_query cq;
        for (int a = 0; a < 3; ++a) cq.d[a] = (2.0 * mu) * N[a] - Vd[a];
        cq.alpha = rough * rough;
        rtr_gather_out rec;
        if constexpr (SET)
            rec = capture_set_lookup_one(*S, K.chain.lv, K.chain.n, K.texels, q.p, cq.d, cq.alpha);
        else
            rec = cube_chain_lookup_one(K.chain.lv, K.chain.n, K.texels, cq, 1, 0);
        if (!rec.valid) return o;
        X[0] = rec.v[0], X[1] = rec.v[1], X[2] = rec.v[2], count += rec.count;
    }
    const rtr_brdf_entry ab = brdf_fetch(K.n_mu, K.n_rough, K.table, muc, rough);
    const double om = 1.0 - q.metallic;
    for (int ch = 0; ch < 3; ++ch) {
        const double F0 = om * 0.04 + q.metallic * q.base[ch];
        const double kS = F0 * ab.a + ab.b;
        const double kD = (1.0 - kS) * om;
        const double diffuse = ((kD * q.base[ch]) * E[ch]) / RT_PI;
        const double specular = X[ch] * kS;
        o.v[ch] = K.parts == RTR_SHADE_DIFFUSE ? diffuse : K.parts == RTR_SHADE_SPECULAR ? specular : diffuse + specular;
    }
    o.count = count, o.valid = 1;
    return o;
}

/* ---- ENVIRONMENT: host side, what the entries of rtr_ibl.hip and rtr_preview.hip check and build alike ---- */

/* why `env` is no environment, or nullptr: the rules of the lookups it names, for the selected parts only */
inline const char* env_why(const rtr_shade_env* e) {
    if (!e) return "null environment";
    if (e->parts < 1 || e->parts > (RTR_SHADE_DIFFUSE | RTR_SHADE_SPECULAR)) return "parts must be RTR_SHADE_DIFFUSE, RTR_SHADE_SPECULAR or both";
    if (e->n_mu < 1 || e->n_mu > RTR_BRDF_MAX || e->n_rough < 1 || e->n_rough > RTR_BRDF_MAX) return "table n_mu or n_rough outside 1 .. 256";
    if (!e->table) return "null table";
    if (e->parts & RTR_SHADE_DIFFUSE) {
        if (const char* why = probe_grid_why(e->grid)) return why;
        if (!e->probes) return "null probes";
        if ((e->depth != nullptr) != (e->visible != nullptr)) return "depth and visible go together";
        if (e->visible)
            if (const char* why = probe_maps_why(e->grid, e->visible)) return why;
    }
    if (e->parts & RTR_SHADE_SPECULAR) {
        if (e->n_records < 0) return "negative n_records";
        if (const char* why = cube_chain_why(e->levels, e->n_levels, e->n_records)) return why;
        if (!e->chain) return "null chain";
    }
    return nullptr;
}

/* the set forms (rtr_shade_ibl_set, rtr_preview_set): the environment's rules, and the set's when SPECULAR reads it */
inline const char* env_set_why(const rtr_shade_env* e, const rtr_capture_set* set) {
    if (const char* why = env_why(e)) return why;
    return e->parts & RTR_SHADE_SPECULAR ? capture_set_why(set) : nullptr;
}
/* the captures whose chains e->chain holds: the set's when SPECULAR reads it */
inline long long env_cubes(const rtr_shade_env* e, const rtr_capture_set* set) {
    return e->parts & RTR_SHADE_SPECULAR ? set->n_captures : 1;
}
/* the kernel's argument of the set of a valid pair: empty, and not read, without SPECULAR */
inline SetK env_set_k(const rtr_shade_env* e, const rtr_capture_set* set) {
    SetK none{};
    none.fallback = -1;
    return e->parts & RTR_SHADE_SPECULAR ? set_k(set) : none;
}

/* bytes of the arrays of a valid environment: of a part that is not selected 0.  `cubes`: e->chain holds that many chains
 * of e->n_records records each (a capture set) */
struct EnvBytes {
    size_t probes, depth, chain, table;
    size_t total() const { return probes + depth + chain + table; }
};
inline EnvBytes env_bytes(const rtr_shade_env* e, long long cubes = 1) {
    EnvBytes b{0, 0, 0, (size_t)e->n_mu * e->n_rough * sizeof(rtr_brdf_entry)};
    if (e->parts & RTR_SHADE_DIFFUSE) {
        b.probes = (size_t)grid_probes(e->grid) * sizeof(rtr_probe_sh);
        if (e->visible) b.depth = (size_t)grid_probes(e->grid) * e->visible->map_size * e->visible->map_size * sizeof(rtr_probe_depth_texel);
    }
    if (e->parts & RTR_SHADE_SPECULAR) b.chain = (size_t)cubes * (size_t)e->n_records * sizeof(rtr_gather_out);
    return b;
}
/* the kernel's argument of a valid environment whose arrays are at these addresses */
inline ShadeK shade_k(const rtr_shade_env* e, const void* probes, const void* depth, const void* chain, const void* table) {
    ShadeK K{};
    K.parts = e->parts;
    if (e->parts & RTR_SHADE_DIFFUSE) {
        K.grid = *e->grid, K.probes = static_cast<const rtr_probe_sh*>(probes);
        if (e->visible) {
            K.visible = 1, K.depth = static_cast<const rtr_probe_depth_texel*>(depth);
            K.T = e->visible->map_size, K.normal_bias = e->visible->normal_bias;
        }
    }
    if (e->parts & RTR_SHADE_SPECULAR) {
        for (int i = 0; i < e->n_levels; ++i) K.chain.lv[i] = e->levels[i];
        K.chain.n = e->n_levels, K.texels = static_cast<const rtr_gather_out*>(chain);
    }
    K.n_mu = e->n_mu, K.n_rough = e->n_rough, K.table = static_cast<const rtr_brdf_entry*>(table);
    return K;
}
/* The arrays of a valid environment packed behind `base` in the order probes, depth, chain, table, each 16-byte aligned
 * where base is: K is the kernel's argument of that layout, and with `copy` the arrays' copies from the host are queued on
 * `stream`.  rtr_shade_ibl and rtr_preview stage an environment this way */
inline hipError_t env_stage(const rtr_shade_env* e, const EnvBytes& b, char* base, bool copy, hipStream_t stream, ShadeK& K) {
    static_assert(sizeof(rtr_probe_sh) % 16 == 0 && sizeof(rtr_probe_depth_texel) % 16 == 0 && sizeof(rtr_gather_out) % 16 == 0 &&
                      sizeof(rtr_brdf_entry) % 16 == 0, "the arrays follow each other 16-byte aligned");
    char* const at[4] = {base, base + b.probes, base + b.probes + b.depth, base + b.probes + b.depth + b.chain};
    const void* const from[4] = {e->probes, e->depth, e->chain, e->table};
    const size_t bytes[4] = {b.probes, b.depth, b.chain, b.table};
    K = shade_k(e, at[0], at[1], at[2], at[3]);
    for (int i = 0; copy && i < 4; ++i)
        if (bytes[i])
            if (hipError_t err = hipMemcpyAsync(at[i], from[i], bytes[i], hipMemcpyHostToDevice, stream)) return err;
    return hipSuccess;
}
/* the _device forms: do two spans of bytes meet; does the span [o0, o0 + on) meet an array of a valid environment whose
 * arrays are on the device.  `bits` takes the arrays' addresses for the entry's alignment check */
inline bool spans_overlap(uintptr_t a0, size_t an, uintptr_t b0, size_t bn) { return an && bn && a0 < b0 + bn && b0 < a0 + an; }
inline bool env_overlaps(const rtr_shade_env* e, const EnvBytes& b, uintptr_t o0, size_t on, uintptr_t& bits) {
    const uintptr_t a0[4] = {(uintptr_t)e->probes, (uintptr_t)e->depth, (uintptr_t)e->chain, (uintptr_t)e->table};
    const size_t an[4] = {b.probes, b.depth, b.chain, b.table};
    bool meets = false;
    for (int i = 0; i < 4; ++i)
        if (an[i]) bits |= a0[i], meets = meets || spans_overlap(o0, on, a0[i], an[i]);
    return meets;
}
