/*
 * rt_ibl_kernels.h -- the kernels of image-based shading (rt_ibl.h has their arithmetic), the set form of the shader among
 * them, instantiated and launched by
 * rtr_ibl.hip alone: a unit that only composes shade_ibl_one (rtr_preview.hip) includes rt_ibl.h without them.
 */
#pragma once

#include "rt_ibl.h"

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

/* rtr_shade_ibl_set: the same lane per query; the specular record comes from the capture set S (capture_set_lookup_one) */
__global__ void __launch_bounds__(RTR_BLOCK) k_shade_ibl_set(const ShadeK K, const SetK S, const rtr_shade_query* __restrict__ queries,
                                                              rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const rtr_shade_query q = queries[k];
    double nlen, vlen;
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (!shade_query_bad(q, nlen, vlen)) o = shade_ibl_one<true>(K, q, nlen, vlen, &S);
    out[k] = o;
}
