/*
 * rt_ibl.h -- image-based shading (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*): the arithmetic of that contract, written
 * once for host (the _one forms, the entries' checks) and device, and the two kernels, instantiated and launched by
 * rtr_ibl.hip.  The lookups the shader composes are rt_render.h's: nothing of them is restated here.
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
 * and a count before the chain is read */
RT_HD rtr_gather_out shade_ibl_one(const ShadeK& K, const rtr_shade_query& q, double nlen, double vlen) {
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
        const rtr_gather_out rec = cube_chain_lookup_one(K.chain.lv, K.chain.n, K.texels, cq);
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

/* rtr_brdf_table: a wave owns an entry: lane l carries the contract's lane l of its three sums in registers, and the
 * butterfly ends in one 16-byte store.  The four waves of a workgroup take four neighbouring entries of one row (blockIdx.y)
 * and share the parts of a node that do not depend on mu: thread i works out BrdfS of s_i for the row's roughness (a
 * division, three square roots) and BrdfT of t_i (two divisions) once, into LDS, one array per member (12 KiB; the lanes of
 * a wave read at most two neighbouring s and consecutive t: no bank conflict).  What is left per (node, entry) is
 * brdf_node: two divisions for a USED node. */
struct TableK {
    rtr_brdf_entry* out; /* out[0] is entry `out_first` of the table (r * n_mu + c) */
    long long out_first;
    int row0;            /* blockIdx.y = 0 serves this row */
    int c0, c1;          /* the launch serves the columns [c0, c1) of each of its rows */
    int n_mu, n_rough, M;
};
__global__ void __launch_bounds__(RTR_BLOCK) k_brdf_table(const TableK K) {
    __shared__ double s_s[4][RTR_BRDF_MAX], s_t[2][RTR_BRDF_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = K.row0 + (int)blockIdx.y;
    const BrdfRow R = brdf_row(r, K.n_rough);
    if (tid < K.M) {
        const BrdfS S = brdf_s(tid, K.M, R);
        const BrdfT T = brdf_t(tid, K.M);
        s_s[0][tid] = S.s, s_s[1][tid] = S.hz, s_s[2][tid] = S.sh, s_s[3][tid] = S.rden;
        s_t[0][tid] = T.cx, s_t[1][tid] = T.wphi;
    }
    __syncthreads();
    const int c = K.c0 + (int)blockIdx.x * (RTR_BLOCK / 64) + wave;
    if (c >= K.c1) return;
    const BrdfCol C = brdf_col(c, K.n_mu, R);
    const int MM = K.M * K.M;
    double W = 0.0, A = 0.0, B = 0.0;
    for (int j = lane; j < 2 * MM; j += 64) {
        const int jj = j < MM ? j : j - MM;
        const int si = jj / K.M, ti = jj - si * K.M;
        BrdfS S;
        BrdfT T;
        S.s = s_s[0][si], S.hz = s_s[1][si], S.sh = s_s[2][si], S.rden = s_s[3][si];
        T.cx = s_t[0][ti], T.wphi = s_t[1][ti];
        W = W + T.wphi * S.s;
        brdf_node(R, C, S, T, j < MM ? 1.0 : -1.0, A, B);
    }
    for (int off = 32; off > 0; off >>= 1)
        W = W + __shfl_xor(W, off, 64), A = A + __shfl_xor(A, off, 64), B = B + __shfl_xor(B, off, 64);
    if (lane == 0) K.out[(long long)r * K.n_mu + c - K.out_first] = brdf_result(W, A, B);
}

/* rtr_shade_ibl: one lane per query, straight-line (shade_ibl_one) */
__global__ void __launch_bounds__(RTR_BLOCK) k_shade_ibl(const ShadeK K, const rtr_shade_query* __restrict__ queries,
                                                          rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const rtr_shade_query q = queries[k];
    double nlen, vlen;
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (!shade_query_bad(q, nlen, vlen)) o = shade_ibl_one(K, q, nlen, vlen);
    out[k] = o;
}
