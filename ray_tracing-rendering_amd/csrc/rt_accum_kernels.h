/*
 * rt_accum_kernels.h -- the non-template kernels of the progressive accumulators (rtr_accum_*); rtr_accum.hip includes
 * them for the product, and rtr_test.hip for the test library's own copies of k_accum_plan and k_accum_commit.
 *  k_accum_commit / k_accum_resolve(_scatter)   keep the sums of the tiles a pass finished, and turn sums + per-tile
 *                  sample counts into linear mean radiance and the 8-bit store.
 *  k_accum_errors / k_accum_plan   adaptive sampling: per-tile noise estimates from sums + second moments, and the
 *                  per-tile targets and active-tile list of the next pass, on the device.
 *  k_accum_features_scatter   the packed planes of k_features into a caller's device buffer.
 */
#pragma once

#include "rt_kernels.h" /* RTR_FEAT */

/* every accumulator pass, after its k_mega (chunks = 1, so cell = tile slot), workgroup b for the slot active[b]: a tile
 * whose workgroup ran to the end takes the pass's sums (and moments) and its target count; an interrupted one keeps its
 * old sums, moments and count (cancel is atomic per tile, in every variant: the sorted one sums in place in P.partial) */
__global__ void __launch_bounds__(RTR_BLOCK) k_accum_commit(const RenderK P, double* __restrict__ sum, double* __restrict__ q,
                                                            int* __restrict__ count) {
    if ((int)blockIdx.x >= *P.n_active) return; /* workgroup-uniform */
    const int slot = P.active[blockIdx.x];
    if (!P.done[slot]) return;
    const size_t o = (size_t)slot * 3 * RTR_BLOCK + threadIdx.x;
    sum[o] = P.partial[o];
    sum[o + RTR_BLOCK] = P.partial[o + RTR_BLOCK];
    sum[o + 2 * RTR_BLOCK] = P.partial[o + 2 * RTR_BLOCK];
    if (q) q[(size_t)slot * RTR_BLOCK + threadIdx.x] = P.q_part[(size_t)slot * RTR_BLOCK + threadIdx.x];
    if (threadIdx.x == 0) count[slot] = P.tile_s1[slot];
}

/* rtr_accum_errors / rtr_accum_refine: one workgroup per owned tile, the largest per-pixel error of the tile's pixels
 * inside the region (include/rtr_hip.h); +inf below 2 samples.  Only + - * / sqrt max: a numpy restatement gives the
 * same bits.  The header's max(a, b) is `a > b ? a : b` with the varying operand as a: a NaN difference gives var = 0 and
 * a NaN or negative y_m the floor 1e-4, so no pixel's error is NaN whatever the sums hold (+inf where Q is +inf over finite
 * sums) and the `>` folds below are a plain maximum; a tile whose pixels all have error 0 reports +0.0.  What the lanes
 * outside the region hold is never read. */
__global__ void __launch_bounds__(RTR_BLOCK) k_accum_errors(const AccumResolveK R, const double* __restrict__ q,
                                                            double* __restrict__ err) {
    __shared__ double wmax[RTR_BLOCK / 64];
    const int n = R.count[blockIdx.x];
    if (n < 2) { /* workgroup-uniform */
        if (threadIdx.x == 0) err[blockIdx.x] = __builtin_inf();
        return;
    }
    int i, j;
    bool active;
    tile_pixel(R.r, blockIdx.x, threadIdx.x, i, j, active);
    double e = 0.0;
    if (active) {
        const size_t in = (size_t)blockIdx.x * 3 * RTR_BLOCK + threadIdx.x;
        const double scale = 1.0 / n; /* the mean of k_accum_resolve */
        const V3 m = mk(scale * R.sum[in], scale * R.sum[in + RTR_BLOCK], scale * R.sum[in + 2 * RTR_BLOCK]);
        const double ym = luminance(m);
        const double d = scale * q[(size_t)blockIdx.x * RTR_BLOCK + threadIdx.x] - ym * ym;
        const double var = (d > 0.0 ? d : 0.0) / (double)(n - 1);
        e = __builtin_sqrt(var) / (2.0 * __builtin_sqrt(ym > 1e-4 ? ym : 1e-4));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(e, off, 64);
        e = o > e ? o : e;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wmax[0];
        for (int w = 1; w < RTR_BLOCK / 64; ++w) t = wmax[w] > t ? wmax[w] : t;
        err[blockIdx.x] = t;
    }
}

/* the plan of an accumulator pass, one workgroup: every slot's target tile_s1 and the active list (the slots with
 * target > count, the most pending samples first: by the bucket floor(log2(target - count)), descending; the order inside
 * a bucket does not matter, every tile is one workgroup).  The targets come from
 *   mode 0  tile_s1 as given (rtr_accum_render_tiles uploaded it)
 *   mode 1  max(count, spp) (rtr_accum_render)
 *   mode 2  the refinement rule of rtr_accum_refine on err: count < spp_min -> spp_min; err > threshold and count <
 *           spp_max -> min(spp_max, 2 * count); else count.  `err > threshold` is false at equality and for a NaN err
 *           (such a tile stops once it holds spp_min), true for +inf; the minimum is exact up to spp_max = INT32_MAX; a
 *           count above spp_max stays.
 * The slots of `active` from *n_active on are not written. */
struct AccumPlanK {
    int n_tiles, mode;
    const int* count;
    const double* err;
    int* tile_s1;
    int* active;
    int* n_active;
    int spp, spp_min, spp_max;
    double threshold;
};
__global__ void __launch_bounds__(1024) k_accum_plan(const AccumPlanK K) {
    __shared__ int bucket_n[32];
    if (threadIdx.x < 32) bucket_n[threadIdx.x] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < K.n_tiles; t += blockDim.x) {
        const int c = K.count[t];
        int target = c;
        if (K.mode == 0) {
            target = K.tile_s1[t];
        } else if (K.mode == 1) {
            target = K.spp > c ? K.spp : c;
        } else if (c < K.spp_min) {
            target = K.spp_min;
        } else if (K.err[t] > K.threshold && c < K.spp_max) {
            target = c < K.spp_max - c ? 2 * c : K.spp_max; /* min(spp_max, 2 * count) without overflow */
        }
        K.tile_s1[t] = target;
        if (target > c) atomicAdd(&bucket_n[31 - __builtin_clz((unsigned)(target - c))], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) { /* bucket b starts after every larger bucket */
        int base = 0;
        for (int b = 31; b >= 0; --b) {
            const int n = bucket_n[b];
            bucket_n[b] = base;
            base += n;
        }
        *K.n_active = base;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < K.n_tiles; t += blockDim.x) {
        const int c = K.count[t], target = K.tile_s1[t];
        if (target > c) K.active[atomicAdd(&bucket_n[31 - __builtin_clz((unsigned)(target - c))], 1)] = t;
    }
}

/* rtr_accum_resolve: (1 / count) * sum, the expression of k_resolve, and the reference's store of it
 * (renderer.h:126-140: sqrt gamma, clamp to [0, 1]; render_buffer.h:35-55: uchar(c * 255) truncation).  A mean above 1
 * or +inf stores 255 and -0.0 stores 0; the byte of a NaN or negative mean (sqrt: NaN) is unspecified, as the reference's
 * cast of a NaN is, but the same here and in k_accum_resolve_scatter */
__global__ void __launch_bounds__(RTR_BLOCK) k_accum_resolve(const AccumResolveK R) {
    const int n = R.count[blockIdx.x];
    if (n == 0) return; /* wave-uniform: the host leaves such a tile alone */
    const size_t in = (size_t)blockIdx.x * 3 * RTR_BLOCK + threadIdx.x;
    const size_t o = ((size_t)blockIdx.x * RTR_BLOCK + threadIdx.x) * 3;
    const double scale = 1.0 / n;
    const double v[3] = {scale * R.sum[in], scale * R.sum[in + RTR_BLOCK], scale * R.sum[in + 2 * RTR_BLOCK]};
    if (R.out) R.out[o] = v[0], R.out[o + 1] = v[1], R.out[o + 2] = v[2];
    if (R.rgb8)
        for (int c = 0; c < 3; ++c) {
            double g = __builtin_sqrt(v[c]); /* correctly rounded, like std::sqrt */
            g = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g); /* clamp (rtweekend.h): NaN passes through */
            R.rgb8[o + c] = static_cast<unsigned char>(g * 255);
        }
}

/* rtr_accum_resolve_device: the values of k_accum_resolve stored straight into the caller's region, R.out with
 * `row_stride` pixels from row to row and R.rgb8 in rows of x1 - x0 pixels, Y flipped (what the host form's scatter loop
 * does on the CPU).  One workgroup per owned tile; a tile with count 0 is not written, and that test is all the validity
 * there is: the host never reads the counts.  The lanes compute per pixel and store per element: through LDS, lane t
 * takes elements t, t + 256, t + 512 of the tile's [16][16][3], so the 48 doubles (384 B) and the 48 bytes of a tile row
 * leave as one run of consecutive lanes. */
__global__ void __launch_bounds__(RTR_BLOCK) k_accum_resolve_scatter(const AccumResolveK R, long long row_stride) {
    __shared__ double lin[3 * RTR_BLOCK];
    __shared__ unsigned char bytes[3 * RTR_BLOCK];
    const int n = R.count[blockIdx.x];
    if (n == 0) return; /* workgroup-uniform */
    const size_t in = (size_t)blockIdx.x * 3 * RTR_BLOCK + threadIdx.x;
    const double scale = 1.0 / n;
    const double v[3] = {scale * R.sum[in], scale * R.sum[in + RTR_BLOCK], scale * R.sum[in + 2 * RTR_BLOCK]};
    for (int c = 0; c < 3; ++c) {
        lin[3 * threadIdx.x + c] = v[c];
        if (!R.rgb8) continue;
        double g = __builtin_sqrt(v[c]); /* the store of k_accum_resolve */
        g = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
        bytes[3 * threadIdx.x + c] = static_cast<unsigned char>(g * 255);
    }
    __syncthreads();
    const RenderK& P = R.r;
    const int w = P.x1 - P.x0;
    for (int k = 0; k < 3; ++k) {
        const int e = k * RTR_BLOCK + threadIdx.x, c = e % 3;
        int i, j;
        bool active;
        tile_pixel(P, blockIdx.x, e / 3, i, j, active);
        if (!active) continue;
        if (R.out) R.out[((long long)(j - P.y0) * row_stride + (i - P.x0)) * 3 + c] = lin[e];
        if (R.rgb8) R.rgb8[((long long)(P.y1 - 1 - j) * w + (i - P.x0)) * 3 + c] = bytes[e];
    }
}

/* rtr_accum_features_device: the packed [tile][RTR_FEAT][RTR_BLOCK] planes of k_features -> the caller's [row][col][RTR_FEAT]
 * region, every owned tile (the features do not depend on the samples a tile holds).  Loads per plane, stores per
 * element like k_accum_resolve_scatter: a tile row is 16 * RTR_FEAT consecutive doubles. */
__global__ void __launch_bounds__(RTR_BLOCK) k_accum_features_scatter(const RenderK P, const double* __restrict__ feat,
                                                                      double* __restrict__ out, long long row_stride) {
    __shared__ double s[RTR_FEAT * RTR_BLOCK];
    const double* f = feat + (size_t)blockIdx.x * RTR_FEAT * RTR_BLOCK + threadIdx.x;
    for (int c = 0; c < RTR_FEAT; ++c) s[RTR_FEAT * threadIdx.x + c] = f[c * RTR_BLOCK];
    __syncthreads();
    for (int k = 0; k < RTR_FEAT; ++k) {
        const int e = k * RTR_BLOCK + threadIdx.x;
        int i, j;
        bool active;
        tile_pixel(P, blockIdx.x, e / RTR_FEAT, i, j, active);
        if (active) out[((long long)(j - P.y0) * row_stride + (i - P.x0)) * RTR_FEAT + e % RTR_FEAT] = s[e];
    }
}
