/*
 * rt_image_kernels.h -- the kernels that work on finished images; rtr_image.hip includes them, and no other unit of
 * librtr_hip.so (the test library takes its own copy for rtr_test_temporal_planes).
 *  k_denoise_gather / _prep / _pass / _pass_lds / _out   the a-trous denoiser (rtr_accum_denoise, rtr_denoise_host).
 *  k_temporal_blend / _store   reprojection of the last frame in front of the filter (rtr_accum_denoise_temporal).
 *  k_display_meter / _scale / _apply   the display transform (rtr_display_*).
 */
#pragma once

#include "rt_kernels.h" /* RTR_FEAT */

/* ---- rtr_accum_denoise / rtr_denoise_host: edge-avoiding a-trous filter (include/rtr_hip.h) ----
 * Every plane is row-major over the w x h region, pixel p = y * w + x (y = j - y0).  Inputs (AoS, the layout of the host
 * entry point): m [p][3] mean radiance, q [p] second moments, n [p] sample count (0 = not a tap, left alone), feat [p][7].
 * Working planes (SoA): c[b] [3][np] colour and v[b] [np] variance of ping-pong buffer b, a / nrm [3][np], z [np].
 * Only + - * / sqrt and compares: a numpy restatement gives the same bits. */
struct DenoiseK {
    int w, h, iterations;
    double sl2, sn2, sa2, sz2; /* sigma * sigma */
    double* m;
    double* q;
    int* n;
    double* feat;
    double* c[2];
    double* v[2];
    double* a;
    double* nrm;
    double* z;
    double* out;         /* null or [p][3] */
    unsigned char* rgb8; /* null or [p][3], Y flipped: region row h - 1 - y */
};

/* the accumulator's packed tiles -> the input planes; every pixel of the region is in an owned tile (tile_stride <= 1) */
__global__ void __launch_bounds__(RTR_BLOCK) k_denoise_gather(const AccumResolveK R, const double* __restrict__ q,
                                                              const double* __restrict__ feat, const DenoiseK D) {
    int i, j;
    bool active;
    tile_pixel(R.r, blockIdx.x, threadIdx.x, i, j, active);
    if (!active) return;
    const size_t p = (size_t)(j - R.r.y0) * D.w + (i - R.r.x0);
    const int n = R.count[blockIdx.x];
    D.n[p] = n;
    const size_t in = (size_t)blockIdx.x * 3 * RTR_BLOCK + threadIdx.x;
    const double* f = feat + (size_t)blockIdx.x * RTR_FEAT * RTR_BLOCK + threadIdx.x;
    double* fo = D.feat + p * RTR_FEAT;
    for (int c = 0; c < RTR_FEAT; ++c) fo[c] = f[c * RTR_BLOCK];
    if (n == 0) return;
    const double scale = 1.0 / n; /* the mean of k_accum_resolve */
    double* mo = D.m + p * 3;
    mo[0] = scale * R.sum[in], mo[1] = scale * R.sum[in + RTR_BLOCK], mo[2] = scale * R.sum[in + 2 * RTR_BLOCK];
    D.q[p] = q[(size_t)blockIdx.x * RTR_BLOCK + threadIdx.x];
}

/* the variance of the mean and demodulation by the albedo -> c[0], v[0]; the features -> a, nrm, z */
__global__ void __launch_bounds__(RTR_BLOCK) k_denoise_prep(const DenoiseK D) {
    const long long np = (long long)D.w * D.h, p = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (p >= np) return;
    const int n = D.n[p];
    if (n == 0) return;
    const double* f = D.feat + p * RTR_FEAT;
    const V3 a = mk(f[0], f[1], f[2]);
    const V3 m = mk(D.m[3 * p], D.m[3 * p + 1], D.m[3 * p + 2]);
    double var = 1e30;
    if (n >= 2) {
        const double scale = 1.0 / n, ym = luminance(m);
        const double d = scale * D.q[p] - ym * ym;
        var = (d > 0.0 ? d : 0.0) / (double)(n - 1) / (double)n;
    }
    double la = luminance(a);
    la = la > 1e-3 ? la : 1e-3;
    D.v[0][p] = var / (la * la);
    D.c[0][p] = a.x > 1e-3 ? m.x / a.x : m.x;
    D.c[0][p + np] = a.y > 1e-3 ? m.y / a.y : m.y;
    D.c[0][p + 2 * np] = a.z > 1e-3 ? m.z / a.z : m.z;
    for (int c = 0; c < 3; ++c) D.a[p + c * np] = f[c], D.nrm[p + c * np] = f[3 + c];
    D.z[p] = f[6];
}

/* one a-trous pass with step 2^k: 16 x 16 pixels per workgroup, buffer src -> src ^ 1 */
__global__ void __launch_bounds__(RTR_BLOCK) k_denoise_pass(const DenoiseK D, int step, int src) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= D.w || y >= D.h) return;
    const long long np = (long long)D.w * D.h, p = (long long)y * D.w + x;
    if (D.n[p] == 0) return;
    const double* __restrict__ c = D.c[src];
    const double* __restrict__ v = D.v[src];
    /* variance prefilter: 3 x 3 binomial average over the valid neighbours */
    const double k3[3] = {0.25, 0.5, 0.25};
    double gs = 0.0, gw = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= D.w || qy < 0 || qy >= D.h) continue;
            const long long q = (long long)qy * D.w + qx;
            if (D.n[q] == 0) continue;
            const double wk = k3[dx + 1] * k3[dy + 1];
            gs += wk * v[q];
            gw += wk;
        }
    const double g = gs / gw;
    const double h5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const double c0 = c[p], c1 = c[p + np], c2 = c[p + 2 * np];
    const double lp = 0.2126 * c0 + 0.7152 * c1 + 0.0722 * c2;
    const double n0 = D.nrm[p], n1 = D.nrm[p + np], n2 = D.nrm[p + 2 * np];
    const double a0 = D.a[p], a1 = D.a[p + np], a2 = D.a[p + 2 * np];
    const double zp = D.z[p], zz = zp > 1e-3 ? zp : 1e-3;
    const double l_den = D.sl2 * g + 1e-10, z_den = D.sz2 * ((double)step * (double)step) * (zz * zz);
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sv = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= D.h) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= D.w) continue;
            const long long q = (long long)qy * D.w + qx;
            if (D.n[q] == 0) continue;
            const double q0 = c[q], q1 = c[q + np], q2 = c[q + 2 * np];
            const double dl = lp - (0.2126 * q0 + 0.7152 * q1 + 0.0722 * q2);
            const double wl = 1.0 / (1.0 + dl * dl / l_den);
            const double e0 = n0 - D.nrm[q], e1 = n1 - D.nrm[q + np], e2 = n2 - D.nrm[q + 2 * np];
            const double wn = 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) / D.sn2);
            const double f0 = a0 - D.a[q], f1 = a1 - D.a[q + np], f2 = a2 - D.a[q + 2 * np];
            const double wa = 1.0 / (1.0 + (f0 * f0 + f1 * f1 + f2 * f2) / D.sa2);
            const double ez = zp - D.z[q];
            const double wz = 1.0 / (1.0 + ez * ez / z_den);
            const double wt = h5[dx + 2] * h5[dy + 2] * wl * wn * wa * wz;
            sw += wt;
            s0 += wt * q0, s1 += wt * q1, s2 += wt * q2;
            sv += wt * wt * v[q];
        }
    }
    double* co = D.c[src ^ 1];
    co[p] = s0 / sw, co[p + np] = s1 / sw, co[p + 2 * np] = s2 / sw;
    D.v[src ^ 1][p] = sv / (sw * sw);
}

/* k_denoise_pass for the small steps 1 and 2: the workgroup first stages its 16 x 16 pixels and a halo of 2 * STEP
 * (which holds the prefilter's 1-pixel halo) in LDS -- 20 x 20 or 24 x 24 pixels, 11 doubles and a validity flag each,
 * 37 / 53 KiB -- and then runs the arithmetic of k_denoise_pass, in its order, on the staged values: the same bits */
template <int STEP>
__global__ void __launch_bounds__(RTR_BLOCK) k_denoise_pass_lds(const DenoiseK D, int src) {
    constexpr int R = 2 * STEP, S = 16 + 2 * R, N = S * S;
    __shared__ double lc[3][N], lv[N], la[3][N], ln[3][N], lz[N];
    __shared__ int lok[N];
    const long long np = (long long)D.w * D.h;
    const int bx = blockIdx.x * 16 - R, by = blockIdx.y * 16 - R;
    const double* __restrict__ c = D.c[src];
    for (int k = threadIdx.x; k < N; k += RTR_BLOCK) {
        const int gx = bx + k % S, gy = by + k / S;
        const long long q = (long long)gy * D.w + gx;
        const bool ok = gx >= 0 && gx < D.w && gy >= 0 && gy < D.h && D.n[q] != 0;
        lok[k] = ok;
        if (ok) {
            for (int ch = 0; ch < 3; ++ch)
                lc[ch][k] = c[q + ch * np], la[ch][k] = D.a[q + ch * np], ln[ch][k] = D.nrm[q + ch * np];
            lv[k] = D.v[src][q], lz[k] = D.z[q];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x = blockIdx.x * 16 + tx, y = blockIdx.y * 16 + ty;
    const int l = (ty + R) * S + tx + R;
    if (x >= D.w || y >= D.h || !lok[l]) return;
    const long long p = (long long)y * D.w + x;
    const double k3[3] = {0.25, 0.5, 0.25};
    double gs = 0.0, gw = 0.0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int m = l + dy * S + dx;
            if (!lok[m]) continue;
            const double wk = k3[dx + 1] * k3[dy + 1];
            gs += wk * lv[m];
            gw += wk;
        }
    const double g = gs / gw;
    const double h5[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const double c0 = lc[0][l], c1 = lc[1][l], c2 = lc[2][l];
    const double lp = 0.2126 * c0 + 0.7152 * c1 + 0.0722 * c2;
    const double n0 = ln[0][l], n1 = ln[1][l], n2 = ln[2][l];
    const double a0 = la[0][l], a1 = la[1][l], a2 = la[2][l];
    const double zp = lz[l], zz = zp > 1e-3 ? zp : 1e-3;
    const double l_den = D.sl2 * g + 1e-10, z_den = D.sz2 * ((double)STEP * (double)STEP) * (zz * zz);
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sv = 0.0;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int m = l + STEP * (dy * S + dx);
            if (!lok[m]) continue;
            const double q0 = lc[0][m], q1 = lc[1][m], q2 = lc[2][m];
            const double dl = lp - (0.2126 * q0 + 0.7152 * q1 + 0.0722 * q2);
            const double wl = 1.0 / (1.0 + dl * dl / l_den);
            const double e0 = n0 - ln[0][m], e1 = n1 - ln[1][m], e2 = n2 - ln[2][m];
            const double wn = 1.0 / (1.0 + (e0 * e0 + e1 * e1 + e2 * e2) / D.sn2);
            const double f0 = a0 - la[0][m], f1 = a1 - la[1][m], f2 = a2 - la[2][m];
            const double wa = 1.0 / (1.0 + (f0 * f0 + f1 * f1 + f2 * f2) / D.sa2);
            const double ez = zp - lz[m];
            const double wz = 1.0 / (1.0 + ez * ez / z_den);
            const double wt = h5[dx + 2] * h5[dy + 2] * wl * wn * wa * wz;
            sw += wt;
            s0 += wt * q0, s1 += wt * q1, s2 += wt * q2;
            sv += wt * wt * lv[m];
        }
    double* co = D.c[src ^ 1];
    co[p] = s0 / sw, co[p + np] = s1 / sw, co[p + 2 * np] = s2 / sw;
    D.v[src ^ 1][p] = sv / (sw * sw);
}

/* remodulate (iterations = 0: the mean itself, the bits of k_accum_resolve) and store linear and / or 8-bit: D.out with
 * `row_stride` pixels from row to row (D.w for the host forms' plane, the caller's for the device forms, whose D.out and
 * D.rgb8 are the caller's buffers), D.rgb8 in rows of D.w pixels.  A pixel with n = 0 is not written: on the device forms
 * this test is the whole validity decision */
__global__ void __launch_bounds__(RTR_BLOCK) k_denoise_out(const DenoiseK D, int src, long long row_stride) {
    const long long np = (long long)D.w * D.h, p = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (p >= np || D.n[p] == 0) return;
    const int x = (int)(p % D.w), y = (int)(p / D.w);
    double o[3];
    for (int c = 0; c < 3; ++c) {
        if (D.iterations == 0) {
            o[c] = D.m[3 * p + c];
        } else {
            const double a = D.a[p + c * np], v = D.c[src][p + c * np];
            o[c] = a > 1e-3 ? v * a : v;
        }
    }
    if (D.out) {
        double* lo = D.out + ((long long)y * row_stride + x) * 3;
        lo[0] = o[0], lo[1] = o[1], lo[2] = o[2];
    }
    if (D.rgb8)
        for (int c = 0; c < 3; ++c) { /* the store of k_accum_resolve */
            double g = __builtin_sqrt(o[c]);
            g = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
            D.rgb8[((size_t)(D.h - 1 - y) * D.w + x) * 3 + c] = static_cast<unsigned char>(g * 255);
        }
}

/* ---- rtr_accum_denoise_temporal: reprojection of the last frame in front of the filter (include/rtr_hip.h) ----
 * A history plane set is AoS over the region, RTR_HIST doubles per pixel (c 0..2, mu1 3, mu2 4, n 5, z 6, nn 7..9): a tap
 * of the gather is 80 contiguous bytes, and rtr_history_planes is a plain copy. */
#define RTR_HIST 10
struct TemporalK {
    rtr_camera cam, prev;   /* the context's camera / the one the history was seen from */
    int W, H, x0, y0;       /* full image size, the region's origin (its size is DenoiseK's w x h) */
    int have;               /* 0: the history is cleared */
    double alpha_min, tau_z, tau_n, min_weight;
    const double* hist_in;  /* [p][RTR_HIST], the last frame */
    double* hist_out;       /* [p][RTR_HIST], this frame (k_temporal_store) */
    double* mom;            /* [3][np]: mu1', mu2', n' between k_temporal_blend and k_temporal_store */
};

RT_DEV double temporal_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* k_denoise_prep with the history blended in: c', var' -> c[0], v[0]; the features -> a, nrm, z; mu1', mu2', n' -> mom.
 * One workgroup per 16 x 16 pixels like k_denoise_pass; the four taps of a pixel come through L2. */
__global__ void __launch_bounds__(RTR_BLOCK) k_temporal_blend(const DenoiseK D, const TemporalK T) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= D.w || y >= D.h) return;
    const long long np = (long long)D.w * D.h, p = (long long)y * D.w + x;
    const int n = D.n[p];
    if (n == 0) return;
    const double* f = D.feat + p * RTR_FEAT;
    const V3 a = mk(f[0], f[1], f[2]);
    const V3 m = mk(D.m[3 * p], D.m[3 * p + 1], D.m[3 * p + 2]);
    const double nn[3] = {f[3], f[4], f[5]};
    const double z = f[6];
    double la = luminance(a);
    la = la > 1e-3 ? la : 1e-3;
    double c[3] = {a.x > 1e-3 ? m.x / a.x : m.x, a.y > 1e-3 ? m.y / a.y : m.y, a.z > 1e-3 ? m.z / a.z : m.z};
    double mu1 = luminance(m), mu2 = (1.0 / n) * D.q[p], ne = (double)n;
    if (T.have && z > 0.0) {
        const rtr_camera& cam = T.cam;
        const rtr_camera& pv = T.prev;
        const double su = ((T.x0 + x) + 0.5) / (T.W - 1), sv = ((T.y0 + y) + 0.5) / (T.H - 1);
        double d[3], q[3], e[3];
        for (int k = 0; k < 3; ++k)
            d[k] = cam.lower_left_corner[k] + su * cam.horizontal[k] + sv * cam.vertical[k] - cam.origin[k];
        const double len = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double zl = z / len;
        for (int k = 0; k < 3; ++k) {
            const double P = cam.origin[k] + zl * d[k];
            q[k] = P - pv.origin[k];
            e[k] = pv.lower_left_corner[k] - pv.origin[k];
        }
        const double zc = -temporal_dot3(q, pv.w);
        if (zc > 0.0) {
            const double F = -temporal_dot3(e, pv.w);
            const double kk = F / zc;
            const double s = (kk * temporal_dot3(q, pv.u) - temporal_dot3(e, pv.u)) / temporal_dot3(pv.horizontal, pv.u);
            const double t = (kk * temporal_dot3(q, pv.v) - temporal_dot3(e, pv.v)) / temporal_dot3(pv.vertical, pv.v);
            const double hx = s * (T.W - 1) - 0.5, hy = t * (T.H - 1) - 0.5;
            const double fx0 = __builtin_floor(hx), fy0 = __builtin_floor(hy);
            const double fx = hx - fx0, fy = hy - fy0;
            const double z_exp = __builtin_sqrt(temporal_dot3(q, q));
            const double z_tol = T.tau_z * (z_exp > 1e-3 ? z_exp : 1e-3);
            /* region bounds in binary64: a NaN or far-away position fails every compare and is never made an index */
            const double rx0 = (double)T.x0, ry0 = (double)T.y0, rx1 = (double)(T.x0 + D.w - 1), ry1 = (double)(T.y0 + D.h - 1);
            double sw = 0.0, hc[3] = {0.0, 0.0, 0.0}, h1 = 0.0, h2 = 0.0, hn = 0.0;
            for (int tap = 0; tap < 4; ++tap) {
                const double tx = fx0 + (double)(tap & 1), ty = fy0 + (double)(tap >> 1);
                if (!(tx >= rx0 && tx <= rx1 && ty >= ry0 && ty <= ry1)) continue;
                const double* h = T.hist_in + ((long long)((int)ty - T.y0) * D.w + ((int)tx - T.x0)) * RTR_HIST;
                if (!(h[5] > 0.0)) continue;
                const double ez = z_exp - h[6];
                if (!((ez < 0.0 ? -ez : ez) <= z_tol)) continue;
                const double e0 = nn[0] - h[7], e1 = nn[1] - h[8], e2 = nn[2] - h[9];
                if (!(e0 * e0 + e1 * e1 + e2 * e2 <= T.tau_n)) continue;
                const double w = ((tap & 1) ? fx : 1.0 - fx) * ((tap >> 1) ? fy : 1.0 - fy);
                sw += w;
                hc[0] += w * h[0], hc[1] += w * h[1], hc[2] += w * h[2];
                h1 += w * h[3], h2 += w * h[4], hn += w * h[5];
            }
            if (sw >= T.min_weight) {
                const double n_h = hn / sw;
                double alpha = ne / (ne + n_h);
                alpha = alpha > T.alpha_min ? alpha : T.alpha_min;
                const double beta = 1.0 - alpha;
                for (int k = 0; k < 3; ++k) c[k] = alpha * c[k] + beta * (hc[k] / sw);
                mu1 = alpha * mu1 + beta * (h1 / sw);
                mu2 = alpha * mu2 + beta * (h2 / sw);
                ne = ne / alpha;
            }
        }
    }
    double var = 1e30;
    if (!(ne < 2.0)) {
        const double dv = mu2 - mu1 * mu1;
        var = (dv > 0.0 ? dv : 0.0) / (ne - 1.0) / ne;
    }
    D.v[0][p] = var / (la * la);
    for (int k = 0; k < 3; ++k) D.c[0][p + k * np] = c[k], D.a[p + k * np] = f[k], D.nrm[p + k * np] = nn[k];
    D.z[p] = z;
    T.mom[p] = mu1, T.mom[p + np] = mu2, T.mom[p + 2 * np] = ne;
}

/* the write-back: what k_temporal_blend left in c[0], mom, nrm and z -> the history's other plane set (before the passes
 * overwrite c[0]); n = 0 where the pixel is invalid */
__global__ void __launch_bounds__(RTR_BLOCK) k_temporal_store(const DenoiseK D, const TemporalK T) {
    const long long np = (long long)D.w * D.h, p = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (p >= np) return;
    double* h = T.hist_out + p * RTR_HIST;
    if (D.n[p] == 0) {
        for (int k = 0; k < RTR_HIST; ++k) h[k] = 0.0;
        return;
    }
    for (int k = 0; k < 3; ++k) h[k] = D.c[0][p + k * np], h[7 + k] = D.nrm[p + k * np];
    h[3] = T.mom[p], h[4] = T.mom[p + np], h[5] = T.mom[p + 2 * np];
    h[6] = D.z[p];
}

/* ---- rtr_display_*: metered exposure, tone curve, 8-bit encoding (include/rtr_hip.h) ----
 * The input is row-major, 3 doubles per pixel, row 0 the lowest row, `row_stride` pixels from row to row.  Three
 * launches, ordered by the stream alone: k_display_meter (luminance histogram), k_display_scale (the quantile and the
 * scale into DisplayRec), k_display_apply (curve and encoding).  Only + - * / sqrt, compares and integer bit operations:
 * a numpy restatement gives the same bits. */
#define RTR_DISPLAY_BINS 512
#define RTR_DISPLAY_TRIPS 8 /* pixels per lane of k_display_meter at most: one flush per 2048 pixels */
struct DisplayRec { /* the layout of rtr_display_result */
    double scale, metered;
    long long n_metered, reserved;
};
struct DisplayK {
    int w, h;
    long long row_stride;
    const double* in;
    unsigned* hist;     /* [RTR_DISPLAY_BINS], zeroed on the stream before k_display_meter */
    DisplayRec* rec;
    const double* srgb; /* [256]: rtr_display_srgb_thresholds */
    int auto_exposure, permille, curve, encoding;
    double exposure, key, white;
    unsigned char* rgb8; /* null or [h][w][3], Y flipped */
    double* mapped;      /* null or [h][w][3] */
};

/* the bin of a pixel, -1 when it is not metered */
RT_DEV int display_bin(const double r, const double g, const double b) {
    const unsigned long long inf = 0x7FF0000000000000ull, mag = 0x7FFFFFFFFFFFFFFFull;
    if ((__double_as_longlong(r) & mag) >= inf || (__double_as_longlong(g) & mag) >= inf || (__double_as_longlong(b) & mag) >= inf)
        return -1;
    const double y = 0.2126 * r + 0.7152 * g + 0.0722 * b;
    if (!(y >= 0x1p-20)) return -1;
    if (y >= 0x1p12) return RTR_DISPLAY_BINS - 1;
    return (int)((unsigned long long)__double_as_longlong(y) >> 48) - 0x3EB0;
}

/* 256 lanes, one pixel per lane per trip; the workgroup's counts gather in LDS and each lane then adds its two bins to
 * the context's histogram (integer adds: the result does not depend on the order of arrival) */
__global__ void __launch_bounds__(RTR_BLOCK) k_display_meter(const DisplayK D) {
    static_assert(RTR_DISPLAY_BINS == 2 * RTR_BLOCK, "two bins per lane");
    __shared__ unsigned bins[RTR_DISPLAY_BINS];
    bins[threadIdx.x] = 0, bins[threadIdx.x + RTR_BLOCK] = 0;
    __syncthreads();
    const int np = D.w * D.h; /* <= 2^28 */
    for (long long p = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x; p < np; p += (long long)gridDim.x * RTR_BLOCK) {
        const int y = (int)p / D.w, x = (int)p - y * D.w;
        const double* c = D.in + ((long long)y * D.row_stride + x) * 3;
        const int m = display_bin(c[0], c[1], c[2]);
        if (m >= 0) atomicAdd(&bins[m], 1u);
    }
    __syncthreads();
    const unsigned n0 = bins[threadIdx.x], n1 = bins[threadIdx.x + RTR_BLOCK];
    if (n0) atomicAdd(&D.hist[threadIdx.x], n0);
    if (n1) atomicAdd(&D.hist[threadIdx.x + RTR_BLOCK], n1);
}

/* one wave: lane l sums bins 8l .. 8l+7, a scan over the lanes finds the lane holding the quantile, that lane walks its
 * bins.  Without auto exposure the histogram is not read (and was not built). */
__global__ void __launch_bounds__(64) k_display_scale(const DisplayK D) {
    const int lane = threadIdx.x;
    if (!D.auto_exposure) {
        if (lane == 0) D.rec->scale = D.exposure, D.rec->metered = 0.0, D.rec->n_metered = 0, D.rec->reserved = 0;
        return;
    }
    unsigned cnt[8];
    long long own = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cnt[k] = D.hist[lane * 8 + k], own += cnt[k];
    long long incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const long long n = __shfl(incl, 63, 64);
    if (n == 0) {
        if (lane == 0) D.rec->scale = D.exposure, D.rec->metered = 0.0, D.rec->n_metered = 0, D.rec->reserved = 0;
        return;
    }
    const long long T = (n * D.permille + 999) / 1000; /* 1 .. n */
    long long cum = incl - own;
    if (cum < T && T <= incl) { /* exactly one lane */
        int m = lane * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cum += cnt[k];
            if (cum >= T) break;
            ++m;
        }
        const double metered = __longlong_as_double((long long)((unsigned long long)(m + 0x3EB0) << 48));
        D.rec->scale = (D.exposure * D.key) / metered;
        D.rec->metered = metered, D.rec->n_metered = n, D.rec->reserved = 0;
    }
}

/* one lane per pixel: x = scale * c, the tone curve, the clamp, the code; the scale is one address for every lane */
__global__ void __launch_bounds__(RTR_BLOCK) k_display_apply(const DisplayK D) {
    static_assert(RTR_BLOCK == 256, "one threshold per lane");
    __shared__ double S[256];
    if (D.encoding == RTR_ENCODE_SRGB) { /* workgroup-uniform */
        S[threadIdx.x] = D.srgb[threadIdx.x];
        __syncthreads();
    }
    const int np = D.w * D.h, p = (int)(blockIdx.x * RTR_BLOCK + threadIdx.x);
    if (p >= np) return;
    const double scale = *as_const(&D.rec->scale);
    const int y = p / D.w, x = p - y * D.w;
    const double* in = D.in + ((long long)y * D.row_stride + x) * 3;
    const double ww = D.white * D.white;
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = in[c];
        const bool ok = (__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull) < 0x7FF0000000000000ull && v > 0.0;
        double e = scale * v;
        e = e < 1e30 ? e : 1e30;
        e = ok ? e : 0.0;
        double u = e;
        if (D.curve == RTR_TONE_REINHARD)
            u = e * (1.0 + e / ww) / (1.0 + e);
        else if (D.curve == RTR_TONE_ACES)
            u = (e * (2.51 * e + 0.03)) / (e * (2.43 * e + 0.59) + 0.14);
        t[c] = u > 0.0 ? (u < 1.0 ? u : 1.0) : 0.0; /* NaN -> 0 */
    }
    if (D.mapped) {
        double* o = D.mapped + (long long)p * 3;
        o[0] = t[0], o[1] = t[1], o[2] = t[2];
    }
    if (D.rgb8) {
        unsigned char* o = D.rgb8 + ((long long)(D.h - 1 - y) * D.w + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (D.encoding == RTR_ENCODE_SRGB) {
                int code = 0;
#pragma unroll
                for (int step = 128; step > 0; step >>= 1)
                    if (S[code + step] <= t[c]) code += step;
                o[c] = (unsigned char)code;
            } else {
                o[c] = static_cast<unsigned char>(__builtin_sqrt(t[c]) * 255);
            }
        }
    }
}
