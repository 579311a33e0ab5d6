/*
 * rt_cube.h -- the kernels of the filtered cube maps (include/rtr_hip.h: rtr_cube_filter*, rtr_cube_chain_lookup*,
 * rtr_capture_set_lookup*),
 * instantiated and launched by rtr_cube.hip.  Their arithmetic is rt_render.h's, shared with the host forms.
 */
#pragma once

#include "rt_render.h"

#define RTR_FILTER_TILE RTR_BLOCK /* source texels per LDS tile: one per thread */

struct FilterK {
    const rtr_gather_out* texels; /* the source cubes of the whole call */
    rtr_gather_out* out;          /* out[0] is output record `out_first` of the call (cube * Fout + e) */
    long long out_first;
    long long cube0;              /* blockIdx.y = 0 serves this cube */
    int e0, e1;                   /* the launch serves the output texels [e0, e1) of each of its cubes */
    int Sin, SSin, Fin;           /* source face size, its square, 6 x that */
    int Sout, SSout, Fout;
    double a2m1, cos_cut;         /* alpha * alpha - 1.0 */
};

/* rtr_cube_filter: all pairs (output texel, source texel) of one cube per blockIdx.y.  A wave owns T output texels, whose
 * directions and 64 x 5 running sums stay in registers: lane l carries the contract's lane l of every one of them, so a
 * source record read once feeds T weights.  The four waves of a workgroup share the source: tile by tile, thread t extends
 * record tile * 256 + t with its unit direction and solid-angle weight (a sqrt and two divisions, once per 4 T outputs) and
 * parks it in LDS, one array per member (15 KiB; consecutive lanes read consecutive doubles, no bank conflict); then every
 * wave walks the tile's four rows of 64, lane l taking record l of the row: j = l, l + 64, ... in increasing order, the
 * order of the contract.  A row none of whose 64 texels an output uses is skipped for that output under a vote (half the
 * sphere when cos_cut = 0): culling changes no bit.  Records past the end of the cube carry the direction 0, so
 * c = 0 > cos_cut fails.  The tree and the record are filter_result's: lane 0 stores. */
template <int T>
__global__ void __launch_bounds__(RTR_BLOCK) k_cube_filter(const FilterK K) {
    __shared__ double s_l[3][RTR_FILTER_TILE], s_dw[RTR_FILTER_TILE], s_v[3][RTR_FILTER_TILE];
    __shared__ int s_valid[RTR_FILTER_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long cube = K.cube0 + blockIdx.y;
    const int first = K.e0 + ((int)blockIdx.x * (RTR_BLOCK / 64) + wave) * T; /* this wave's output texels: first .. first + T */
    double rx[T], ry[T], rz[T];
    FilterAcc acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int e = first + t < K.e1 ? first + t : K.e1 - 1; /* a texel past the end: a copy that is not stored */
        const int f = e / K.SSout, r = e - f * K.SSout, b = r / K.Sout;
        double dw;
        cube_texel_centre(K.Sout, f, r - b * K.Sout, b, rx[t], ry[t], rz[t], dw);
        filter_acc_zero(acc[t]);
    }
    const rtr_gather_out* __restrict__ src = K.texels + cube * K.Fin;
    const bool wave_live = first < K.e1;
    for (int j0 = 0; j0 < K.Fin; j0 += RTR_FILTER_TILE) {
        const int j = j0 + tid;
        double lx = 0.0, ly = 0.0, lz = 0.0, dw = 0.0;
        rtr_gather_out rec;
        rec.v[0] = rec.v[1] = rec.v[2] = 0.0, rec.count = 0, rec.valid = 1;
        if (j < K.Fin) {
            const int f = j / K.SSin, r = j - f * K.SSin, b = r / K.Sin;
            cube_texel_centre(K.Sin, f, r - b * K.Sin, b, lx, ly, lz, dw);
            rec = src[j];
        }
        __syncthreads(); /* the waves are done with the tile before */
        s_l[0][tid] = lx, s_l[1][tid] = ly, s_l[2][tid] = lz, s_dw[tid] = dw;
        s_v[0][tid] = rec.v[0], s_v[1][tid] = rec.v[1], s_v[2][tid] = rec.v[2], s_valid[tid] = rec.valid;
        __syncthreads();
        if (!wave_live) continue;
        const int rows = (K.Fin - j0 + 63) >> 6;
        for (int row = 0; row < (rows < RTR_FILTER_TILE / 64 ? rows : RTR_FILTER_TILE / 64); ++row) {
            const int i = row * 64 + lane;
            const double Lx = s_l[0][i], Ly = s_l[1][i], Lz = s_l[2][i];
            const double Dw = s_dw[i], v0 = s_v[0][i], v1 = s_v[1][i], v2 = s_v[2][i];
            const int valid = s_valid[i];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const double c = (rx[t] * Lx + ry[t] * Ly) + rz[t] * Lz;
                const bool used = c > K.cos_cut;
                if (!__any(used)) continue;
                if (used) filter_add(acc[t], filter_weight(c, Dw, K.a2m1), v0, v1, v2, valid);
            }
        }
    }
    if (!wave_live) return;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        FilterAcc s = acc[t];
        for (int off = 32; off > 0; off >>= 1) {
            s.v[0] = s.v[0] + __shfl_xor(s.v[0], off, 64), s.v[1] = s.v[1] + __shfl_xor(s.v[1], off, 64);
            s.v[2] = s.v[2] + __shfl_xor(s.v[2], off, 64), s.wsum = s.wsum + __shfl_xor(s.wsum, off, 64);
            s.count = s.count + __shfl_xor(s.count, off, 64), s.bad = s.bad + __shfl_xor(s.bad, off, 64);
        }
        if (lane == 0 && first + t < K.e1) K.out[cube * K.Fout + (first + t) - K.out_first] = filter_result(s);
    }
}

/* rtr_cube_chain_lookup: one lane per query, straight-line (cube_chain_lookup_one of rt_render.h); at most eight records */
__global__ void __launch_bounds__(RTR_BLOCK) k_cube_chain_lookup(const ChainK C, const rtr_gather_out* __restrict__ texels,
                                                                  const rtr_cube_query* __restrict__ queries,
                                                                  rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    out[k] = cube_chain_lookup_one(C.lv, C.n, texels, queries[k], 1, 0);
}

/* rtr_capture_set_lookup: one lane per query (capture_set_lookup_one of rt_render.h): a loop over the captures with one chain
 * lookup in it; `texels` holds the set level-major */
__global__ void __launch_bounds__(RTR_BLOCK) k_capture_set_lookup(const SetK S, const ChainK C, const rtr_gather_out* __restrict__ texels,
                                                                   const rtr_capture_query* __restrict__ queries,
                                                                   rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const rtr_capture_query q = queries[k];
    out[k] = capture_set_lookup_one(S, C.lv, C.n, texels, q.p, q.d, q.alpha);
}
