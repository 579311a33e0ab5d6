/*
 * rt_render.h -- what every translation unit of the library shares about one render call: the kernel
 * parameter block, the tile -> pixel map of renderer/renderer.h:61-62, small wave helpers.
 */
#pragma once

#include "rt_device.h"

struct RenderK {
    int W, H;
    int x0, y0, x1, y1;
    int spp, max_depth, rr_start;
    uint32_t seed;
    int tiles_x, tiles_y;
    const int* tile_ids; /* owned tiles, reference dispatch numbering (renderer.h:61-62) */
    int n_tiles;
    int chunks;
    /* Guided chunks (megakernel, spp_chunks = 0): the first `n_big` chunks of a pixel hold `big_spp` samples each, the
     * others `small_spp` (the last one what is left), and the launch runs every tile's big chunks before any small
     * one, so the launch drains through short workgroups.  small_spp = 0: `chunks` equal parts. */
    int n_big, big_spp, small_spp;
    int integrator; /* RTR_INTEGRATOR_* (the wavefront's extend stage needs it for rays that miss) */
    double* partial;             /* [n_tiles*chunks][3][RTR_BLOCK] un-normalised sums */
    unsigned long long* stats;   /* samples, closest segments, shadow segments; [7] = workgroups (queue renders: waves) a cancel interrupted */
    const uint32_t* cancel;      /* rtr_cancel(): id of the newest render it covers; this render stops once *cancel >= render_id */
    uint32_t render_id;
    int* done;                   /* [n_tiles*chunks]: 1 = the workgroup finished every sample of its chunk; a queue render
                                    (k_mega_queue): the jobs of the cell that have finished, RTR_BLOCK when all have */
    /* Accumulator passes (rtr_accum_*: k_mega<..., ACC = 1 | 2>, chunks = 1); unused elsewhere.  Workgroup b renders
     * the tile slot active[b] if b < *n_active (k_accum_plan wrote both on the device), samples [tile_s0[slot],
     * tile_s1[slot]); acc_in: [n_tiles][3][RTR_BLOCK] sums the pass continues instead of starting from 0.  ACC = 2 also
     * continues the second moments q_in ([n_tiles][RTR_BLOCK]) and leaves them in q_part (same layout) */
    const int* tile_s0;
    const double* acc_in;
    const int* tile_s1;
    const int* active;
    const int* n_active;
    const double* q_in;
    double* q_part;
};

/* the luminance weights of the adaptive error (rtr_accum_refine), left to right */
RT_DEV double luminance(const V3 c) { return 0.2126 * c.x + 0.7152 * c.y + 0.0722 * c.z; }

RT_DEV bool render_cancelled(const RenderK& P) {
    return __hip_atomic_load(P.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.render_id;
}

RT_DEV void tile_pixel(const RenderK& P, int slot, int tid, int& i, int& j, bool& active) {
    const int tile = P.tile_ids[slot];
    const int tile_y = (P.tiles_y - 1) - tile / P.tiles_x; /* renderer.h:61-62 */
    const int tile_x = tile % P.tiles_x;
    i = tile_x * 16 + (tid & 15);
    j = tile_y * 16 + (tid >> 4);
    active = i >= P.x0 && i < P.x1 && j >= P.y0 && j < P.y1;
}

/* sample s of pixel (i, j): the generator under the per-sample seed, its two jitter draws and the camera ray
 * (renderer.h:73-75); rng goes on from its state after get_ray */
template <bool JOIN = false>
RT_DEV void camera_sample(const DScene& sc, const RenderK& P, int i, int j, int s, uint32_t& rng, V3& ro, V3& rd, Real& tm) {
    rng = rtr_sample_seed_inline(P.seed, P.W, i, j, s);
    const int region = RT_REGION_CURRENT();
    (void)region;
    RT_REGION(RG_CAMDIV);
    const Real u = (i + rng_next(rng)) / (P.W - 1);
    const Real v = (j + rng_next(rng)) / (P.H - 1);
    RT_REGION(region);
    camera_get_ray<JOIN>(sc.camera, u, v, rng, ro, rd, tm);
}
/* The divisors of camera_sample belong to the launch: (double)(W - 1), (double)(H - 1) and their refined reciprocals are
 * made once in a kernel's prologue (udiv).  The pixel is an int and the jitter below 1, so the numerators are bounded;
 * i + r = 0 takes udiv's plain division.  `safe` is decided on the integers, in scalar registers: a (double)(W - 1) is
 * within rcp_safe's range unless it is 0 (a one-pixel-wide image, which params_check refuses anyway). */
struct CameraDiv {
    UDiv w, h;
};
RT_DEV CameraDiv camera_div_make(int W, int H) {
    CameraDiv c;
    c.w = udiv_make((Real)(W - 1)), c.h = udiv_make((Real)(H - 1));
    c.w.safe = c.h.safe = (W != 1) & (H != 1);
    return c;
}
template <bool JOIN = false>
RT_DEV void camera_sample(const DScene& sc, const CameraDiv& cd, uint32_t seed, int W, int i, int j, int s, uint32_t& rng, V3& ro,
                          V3& rd, Real& tm) {
    rng = rtr_sample_seed_inline(seed, W, i, j, s);
    const int region = RT_REGION_CURRENT();
    (void)region;
    RT_REGION(RG_CAMDIV);
    const Real u = udiv<true>(i + rng_next(rng), cd.w);
    const Real v = udiv<true>(j + rng_next(rng), cd.h);
    RT_REGION(region);
    camera_get_ray<JOIN>(sc.camera, u, v, rng, ro, rd, tm);
}

/* samples [s0, s1) of chunk c of a pixel */
RT_HD void chunk_range(const RenderK& P, int c, int& s0, int& s1) {
    if (P.small_spp == 0) {
        s0 = (int)((long long)c * P.spp / P.chunks);
        s1 = (int)((long long)(c + 1) * P.spp / P.chunks);
    } else if (c < P.n_big) {
        s0 = c * P.big_spp, s1 = s0 + P.big_spp;
    } else {
        s0 = P.n_big * P.big_spp + (c - P.n_big) * P.small_spp, s1 = s0 + P.small_spp;
    }
    s0 = s0 < P.spp ? s0 : P.spp;
    s1 = s1 < P.spp ? s1 : P.spp;
    if (c == P.chunks - 1) s1 = P.spp;
}
/* which (owned tile, chunk) workgroup `b` of a megakernel launch renders: big chunks of every tile first */
RT_HD void mega_work(const RenderK& P, int b, int& tile_slot, int& c) {
    if (P.small_spp == 0) {
        tile_slot = b / P.chunks, c = b % P.chunks;
    } else if (b < P.n_tiles * P.n_big) {
        tile_slot = b / P.n_big, c = b % P.n_big;
    } else {
        const int n_small = P.chunks - P.n_big, q = b - P.n_tiles * P.n_big;
        tile_slot = q / n_small, c = P.n_big + q % n_small;
    }
}

/* The job queue of the pair-cast kernels (k_mega_queue).  A job is one pixel of one (tile, chunk) cell; a BLOCK is the
 * 64 jobs of one wave-quarter of a tile (rows 4q .. 4q + 3, the pixels wave q of a static workgroup renders) for one
 * chunk.  Blocks are numbered in the order mega_work gives workgroups: a launch has n_tiles * chunks * 4 of them, the
 * big chunks of every tile first.  Job k of a block is pixel (k & 15, 4q + (k >> 4)) of the tile. */
#define RT_QUEUE_JOBS 64 /* jobs per block */
struct QueueBlock {
    int slot, quarter, chunk; /* owned tile, wave-quarter of it, chunk */
    int s0, s1;               /* chunk_range of the chunk */
};
RT_HD QueueBlock queue_block(const RenderK& P, int b) {
    QueueBlock q;
    mega_work(P, b >> 2, q.slot, q.chunk);
    q.quarter = b & 3;
    chunk_range(P, q.chunk, q.s0, q.s1);
    return q;
}
/* what a lane keeps of its job in the parked word PK_PIXEL: the pixel, 16 bits each (a queue render's image is at most
 * 65 535 wide and high), and the end of the job's sample range */
RT_HD void queue_pack(int i, int j, int s_end, uint32_t& lo, uint32_t& hi) {
    lo = (uint32_t)i | ((uint32_t)j << 16), hi = (uint32_t)s_end;
}
RT_HD void queue_unpack(uint32_t lo, uint32_t hi, int& i, int& j, int& s_end) {
    i = (int)(lo & 0xffffu), j = (int)(lo >> 16), s_end = (int)hi;
}

RT_DEV unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

/* ---- hemisphere gathers (include/rtr_hip.h: rtr_gather_*) ----
 * The arithmetic of the contract, written once for host (rtr_gather_ray, the host entries' checks) and device
 * (k_gather_*): + - * / sqrt and compares only, no libm, the operation order of core/vec3.h. */
struct GatherK {
    const rtr_gather_point* pts;
    rtr_gather_out* out;
    long long n;
    int samples, lg;            /* N; log2 of the group size G = min(64, bit_ceil(N)) */
    uint32_t seed, point_base;
    double time, t_min, t_max;
    int max_depth, rr_start;    /* radiance only */
};
/* why `p` is no valid parameter block, or nullptr: the rules of the gathers, which the probes share with the block */
inline const char* gather_params_why(const rtr_gather_params* p) {
    if (!p) return "null gather params";
    if (p->samples < 1 || p->samples > (1 << 20)) return "samples outside 1 .. 2^20";
    if (p->flags & ~RTR_FLAG_REFERENCE_ORDER) return "unknown flag bits";
    if (!__builtin_isfinite(p->time) || !__builtin_isfinite(p->t_min)) return "time or t_min not finite";
    if (p->t_max != p->t_max) return "t_max is NaN";
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return "reserved must be 0";
    return nullptr;
}
RT_HD int gather_lg(int samples) {
    int lg = 0;
    while (lg < 6 && (1 << lg) < samples) ++lg;
    return lg;
}
RT_HD bool gather_point_bad(const rtr_gather_point& q, double& nlen) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = ok && __builtin_isfinite(q.p[a]) && __builtin_isfinite(q.n[a]);
    nlen = __builtin_sqrt(q.n[0] * q.n[0] + q.n[1] * q.n[1] + q.n[2] * q.n[2]);
    return !(ok && nlen > 0.0 && nlen < __builtin_huge_val());
}
/* direction of the sample whose generator is `rng` about the unit normal w; rng is left behind the draws */
RT_HD void gather_direction(double wx, double wy, double wz, uint32_t& rng, double& dx, double& dy, double& dz) {
    double x, y, z;
    for (;;) { /* vec3.h:226-233: z takes the first draw */
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        z = -1.0 + rng * 4.656612873077392578125e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        y = -1.0 + rng * 4.656612873077392578125e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        x = -1.0 + rng * 4.656612873077392578125e-10;
        if (!(x * x + y * y + z * z >= 1)) break;
    }
    const double ru = 1 / __builtin_sqrt(x * x + y * y + z * z);
    double sx = wx + ru * x, sy = wy + ru * y, sz = wz + ru * z;
    if (__builtin_fabs(sx) < 1e-8 && __builtin_fabs(sy) < 1e-8 && __builtin_fabs(sz) < 1e-8) sx = wx, sy = wy, sz = wz;
    const double rs = 1 / __builtin_sqrt(sx * sx + sy * sy + sz * sz);
    dx = rs * sx, dy = rs * sy, dz = rs * sz;
}

/* ---- light probes (include/rtr_hip.h: rtr_probe_*, rtr_sh_*) ----
 * The arithmetic of that contract, written once for host (rtr_probe_ray, rtr_sh_basis, rtr_sh_irradiance, the entries'
 * checks) and device (k_probe_*): the same rules as the gathers' above. */
struct ProbeK {
    const rtr_probe_point* pts;
    void* out;                  /* rtr_probe_vis (k_probe_any) or rtr_probe_sh (k_probe_li) records */
    long long n;
    int samples, lg;            /* N; log2 of the group size, the gathers' gather_lg */
    uint32_t seed, point_base;
    double time, t_min, t_max;
    int max_depth, rr_start;    /* radiance only */
    int sum_word;               /* radiance only: the word of the dynamic LDS at which the per-lane sums start */
};
RT_HD bool probe_point_bad(const rtr_probe_point& q) {
    return !(__builtin_isfinite(q.p[0]) && __builtin_isfinite(q.p[1]) && __builtin_isfinite(q.p[2]));
}
/* uniform on the sphere: the rejection loop of gather_direction, then unit; rng is left behind the draws */
RT_HD void probe_direction(uint32_t& rng, double& dx, double& dy, double& dz) {
    double x, y, z;
    for (;;) {
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        z = -1.0 + rng * 4.656612873077392578125e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        y = -1.0 + rng * 4.656612873077392578125e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        x = -1.0 + rng * 4.656612873077392578125e-10;
        if (!(x * x + y * y + z * z >= 1)) break;
    }
    const double ru = 1 / __builtin_sqrt(x * x + y * y + z * z);
    dx = ru * x, dy = ru * y, dz = ru * z;
}
/* the nine real spherical harmonics of bands 0..2 at the unit vector (x, y, z), in the header's order */
RT_HD void sh_basis(double x, double y, double z, double* Y) {
    const double K0 = 0.28209479177387814, K1 = 0.4886025119029199, K2 = 1.0925484305920792, K3 = 0.31539156525252005,
                 K4 = 0.5462742152960396;
    Y[0] = K0;
    Y[1] = K1 * y;
    Y[2] = K1 * z;
    Y[3] = K1 * x;
    Y[4] = K2 * (x * y);
    Y[5] = K2 * (y * z);
    Y[6] = K3 * (3.0 * (z * z) - 1.0);
    Y[7] = K2 * (x * z);
    Y[8] = K4 * (x * x - y * y);
}
/* irradiance E of the normal n (nlen = sqrt(n.n), in (0, inf): gather_point_bad) under the radiance coefficients c */
RT_HD void sh_irradiance(const double (*c)[3], const double* n, double nlen, double* E) {
    const double r = 1 / nlen;
    double y[9];
    sh_basis(r * n[0], r * n[1], r * n[2], y);
    const double A1 = 2.0943951023931953, A2 = 0.7853981633974483;
    const double A[9] = {3.141592653589793, A1, A1, A1, A2, A2, A2, A2, A2};
    for (int ch = 0; ch < 3; ++ch) {
        double e = 0.0;
        for (int i = 0; i < 9; ++i) e = e + (A[i] * y[i]) * c[i][ch];
        E[ch] = 12.566370614359172 * e;
    }
}
/* one axis of the grid lookup: the lower corner i0 and the weights of it and of its neighbour */
RT_HD void probe_axis(double p, double origin, double spacing, int dim, int& i0, double& w0, double& w1) {
    double f = (p - origin) / spacing;
    const double hi = (double)(dim - 1);
    f = f > 0.0 ? f : 0.0;
    f = f < hi ? f : hi;
    i0 = (int)f;
    if (i0 > dim - 2) i0 = dim - 2 > 0 ? dim - 2 : 0;
    const double t = dim == 1 ? 0.0 : f - (double)i0;
    w0 = 1.0 - t, w1 = t;
}
/* rtr_probe_lookup of one query that is not bad; probes: the grid's records */
RT_HD rtr_gather_out probe_lookup_one(const rtr_probe_grid& g, const rtr_probe_sh* __restrict__ probes, const rtr_gather_point& q,
                                      double nlen) {
    int i0[3];
    double w[3][2];
    for (int a = 0; a < 3; ++a) probe_axis(q.p[a], g.origin[a], g.spacing[a], g.dims[a], i0[a], w[a][0], w[a][1]);
    double acc[9][3];
    for (int i = 0; i < 9; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;
    double wsum = 0.0;
    int used = 0;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = i0[0] + dx < g.dims[0] - 1 ? i0[0] + dx : g.dims[0] - 1;
                const int iy = i0[1] + dy < g.dims[1] - 1 ? i0[1] + dy : g.dims[1] - 1;
                const int iz = i0[2] + dz < g.dims[2] - 1 ? i0[2] + dz : g.dims[2] - 1;
                const double wc = (w[0][dx] * w[1][dy]) * w[2][dz];
                const rtr_probe_sh& pr = probes[ix + (long long)g.dims[0] * (iy + (long long)g.dims[1] * iz)];
                if (wc > 0 && pr.valid != 0) {
                    wsum = wsum + wc, ++used;
                    for (int i = 0; i < 9; ++i)
                        for (int ch = 0; ch < 3; ++ch) acc[i][ch] = acc[i][ch] + wc * pr.c[i][ch];
                }
            }
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (used == 0) return o;
    const double rw = 1.0 / wsum;
    for (int i = 0; i < 9; ++i)
        for (int ch = 0; ch < 3; ++ch) acc[i][ch] = rw * acc[i][ch];
    sh_irradiance(acc, q.n, nlen, o.v);
    o.count = used, o.valid = 1;
    return o;
}

/* ---- probe distance maps (include/rtr_hip.h: rtr_probe_depth*, rtr_octa_*, rtr_probe_lookup_visible*) ----
 * The arithmetic of that contract, written once for host (rtr_probe_depth_ray, rtr_octa_*, rtr_probe_lookup_visible_one,
 * the entries' checks) and device (k_probe_depth, k_probe_lookup_visible): the same rules as the gathers' above. */
#define RTR_DEPTH_MAX_MAP 64
struct DepthK {
    const rtr_probe_point* pts; /* the probes of the whole call */
    rtr_probe_depth_texel* out; /* out[0] is the record of texel `first` of the call */
    long long first;            /* texels are numbered through the call: probe * T^2 + e */
    long long k0, n;            /* this launch serves the records [k0, n) of `out` */
    int T, TT;                  /* map size, T^2 */
    int samples, lg;            /* N; log2 of the group size, the gathers' gather_lg */
    uint32_t seed, point_base;
    int jitter;
    double time, t_min, t_max;
};
/* why `p` is no valid parameter block, or nullptr */
inline const char* probe_depth_params_why(const rtr_probe_depth_params* p) {
    if (!p) return "null probe depth params";
    if (p->map_size < 1 || p->map_size > RTR_DEPTH_MAX_MAP) return "map_size outside 1 .. 64";
    if (p->samples < 1 || p->samples > (1 << 20)) return "samples outside 1 .. 2^20";
    if (p->jitter != 0 && p->jitter != 1) return "jitter must be 0 or 1";
    if (p->pad != 0) return "pad must be 0";
    if (!__builtin_isfinite(p->time) || !__builtin_isfinite(p->t_min)) return "time or t_min not finite";
    if (!(__builtin_isfinite(p->t_max) && p->t_max > p->t_min)) return "t_max must be finite and > t_min";
    return nullptr;
}
inline const char* probe_visible_params_why(const rtr_probe_visible_params* p) {
    if (!p) return "null visible params";
    if (p->map_size < 1 || p->map_size > RTR_DEPTH_MAX_MAP) return "map_size outside 1 .. 64";
    if (p->pad != 0 || p->reserved[0] != 0 || p->reserved[1] != 0) return "pad and reserved must be 0";
    if (!(__builtin_isfinite(p->normal_bias) && p->normal_bias >= 0)) return "normal_bias must be finite and >= 0";
    return nullptr;
}
/* why `g` is no probe grid, or nullptr: the rule of rtr_probe_lookup, which every entry that takes a grid shares */
inline const char* probe_grid_why(const rtr_probe_grid* g) {
    if (!g) return "null grid";
    long long count = 1;
    for (int a = 0; a < 3; ++a) {
        if (!__builtin_isfinite(g->origin[a])) return "origin not finite";
        if (!(__builtin_isfinite(g->spacing[a]) && g->spacing[a] > 0)) return "spacing must be finite and > 0";
        if (g->dims[a] < 1 || g->dims[a] > (1 << 24)) return "dims must be >= 1 and their product <= 2^24";
        count *= g->dims[a];
        if (count > (1ll << 24)) return "dims must be >= 1 and their product <= 2^24";
    }
    if (g->pad != 0) return "pad must be 0";
    return nullptr;
}
inline long long grid_probes(const rtr_probe_grid* g) { return (long long)g->dims[0] * g->dims[1] * g->dims[2]; }
/* the maps' rules on top of a valid grid: the parameters, and the bound on the texels of all maps */
inline const char* probe_maps_why(const rtr_probe_grid* g, const rtr_probe_visible_params* vp) {
    if (const char* why = probe_visible_params_why(vp)) return why;
    if (grid_probes(g) * vp->map_size * vp->map_size > (1ll << 24)) return "probes * map_size^2 must be <= 2^24";
    return nullptr;
}
RT_HD double octa_sg(double t) { return t >= 0 ? 1.0 : -1.0; }
/* DECODE: the unit direction of the point (u, v) of the octahedral square */
RT_HD void octa_decode(double u, double v, double& dx, double& dy, double& dz) {
    const double z = (1.0 - __builtin_fabs(u)) - __builtin_fabs(v);
    double x = u, y = v;
    if (!(z >= 0)) x = (1.0 - __builtin_fabs(v)) * octa_sg(u), y = (1.0 - __builtin_fabs(u)) * octa_sg(v);
    const double r = 1 / __builtin_sqrt(x * x + y * y + z * z);
    dx = r * x, dy = r * y, dz = r * z;
}
/* ENCODE: the point of the square of a direction that need not be unit */
RT_HD void octa_encode(double x, double y, double z, double& ox, double& oy) {
    const double s = (__builtin_fabs(x) + __builtin_fabs(y)) + __builtin_fabs(z);
    ox = x / s, oy = y / s;
    if (z < 0) {
        const double fx = (1.0 - __builtin_fabs(oy)) * octa_sg(ox), fy = (1.0 - __builtin_fabs(ox)) * octa_sg(oy);
        ox = fx, oy = fy;
    }
}
/* direction of the ray through texel (a, b) of a T x T octahedral map whose generator is `rng`; rng is left behind the
 * jitter's draws (none without jitter), which are the captures' */
RT_HD void depth_direction(int T, int a, int b, int jitter, uint32_t& rng, double& dx, double& dy, double& dz) {
    double ju = 0.5, jv = 0.5;
    if (jitter) {
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        ju = rng * 2.3283064365386962890625e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        jv = rng * 2.3283064365386962890625e-10;
    }
    const double u = (2.0 * (a + ju)) / T - 1.0;
    const double v = (2.0 * (b + jv)) / T - 1.0;
    octa_decode(u, v, dx, dy, dz);
}
/* one axis of FETCH: no clamp, i0 in [-1, T - 1] */
RT_HD void octa_axis(double c, int T, int& i0, double& w0, double& w1) {
    const double g = ((c + 1.0) * T) * 0.5 - 0.5;
    i0 = g < 0 ? -1 : (int)g;
    const double t = g - (double)i0;
    w0 = 1.0 - t, w1 = t;
}
/* FETCH: the bilinear mean and mean of squares of one probe's T x T map along d, folded over the map's edge; false: a
 * used tap is not valid.  A tap is read only if its weight is > 0 (a NaN weight reads nothing). */
RT_HD bool octa_fetch(int T, const rtr_probe_depth_texel* __restrict__ map, double dx, double dy, double dz, double& m1, double& m2) {
    double ox, oy;
    octa_encode(dx, dy, dz, ox, oy);
    int i0[2];
    double w[2][2];
    octa_axis(ox, T, i0[0], w[0][0], w[0][1]);
    octa_axis(oy, T, i0[1], w[1][0], w[1][1]);
    m1 = 0.0, m2 = 0.0;
    bool ok = true;
    for (int db = 0; db < 2; ++db)
        for (int da = 0; da < 2; ++da) {
            const double wc = w[0][da] * w[1][db];
            if (!(wc > 0)) continue;
            int ia = i0[0] + da, ib = i0[1] + db;
            if (ia < 0) ia = 0, ib = T - 1 - ib;
            else if (ia > T - 1) ia = T - 1, ib = T - 1 - ib;
            if (ib < 0) ib = 0, ia = T - 1 - ia;
            else if (ib > T - 1) ib = T - 1, ia = T - 1 - ia;
            const rtr_probe_depth_texel& t = map[ib * T + ia];
            ok = ok && t.valid != 0;
            m1 = m1 + wc * t.mean, m2 = m2 + wc * t.mean2;
        }
    return ok;
}
/* rtr_probe_lookup_visible of one query that is not bad; probes, depth: the grid's records and their maps */
RT_HD rtr_gather_out probe_lookup_visible_one(const rtr_probe_grid& g, const rtr_probe_sh* __restrict__ probes,
                                              const rtr_probe_depth_texel* __restrict__ depth, int T, double normal_bias,
                                              const rtr_gather_point& q, double nlen) {
    int i0[3];
    double w[3][2];
    for (int a = 0; a < 3; ++a) probe_axis(q.p[a], g.origin[a], g.spacing[a], g.dims[a], i0[a], w[a][0], w[a][1]);
    const double rn = 1 / nlen;
    const double wn[3] = {rn * q.n[0], rn * q.n[1], rn * q.n[2]};
    const double pb[3] = {q.p[0] + normal_bias * wn[0], q.p[1] + normal_bias * wn[1], q.p[2] + normal_bias * wn[2]};
    double acc[9][3];
    for (int i = 0; i < 9; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;
    double wsum = 0.0;
    int used = 0;
    for (int dz = 0; dz < 2; ++dz)
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int ix = i0[0] + dx < g.dims[0] - 1 ? i0[0] + dx : g.dims[0] - 1;
                const int iy = i0[1] + dy < g.dims[1] - 1 ? i0[1] + dy : g.dims[1] - 1;
                const int iz = i0[2] + dz < g.dims[2] - 1 ? i0[2] + dz : g.dims[2] - 1;
                const double tri = (w[0][dx] * w[1][dy]) * w[2][dz];
                const long long pi = ix + (long long)g.dims[0] * (iy + (long long)g.dims[1] * iz);
                const rtr_probe_sh& pr = probes[pi];
                if (!(tri > 0 && pr.valid != 0)) continue;
                const double P[3] = {g.origin[0] + (double)ix * g.spacing[0], g.origin[1] + (double)iy * g.spacing[1],
                                     g.origin[2] + (double)iz * g.spacing[2]};
                const double e[3] = {P[0] - q.p[0], P[1] - q.p[1], P[2] - q.p[2]};
                const double el2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
                const double cosn = el2 > 0 ? (e[0] * wn[0] + e[1] * wn[1] + e[2] * wn[2]) / __builtin_sqrt(el2) : 0.0;
                const double h = (cosn + 1.0) * 0.5;
                const double wb = h * h + 0.2;
                const double dv[3] = {pb[0] - P[0], pb[1] - P[1], pb[2] - P[2]};
                const double r2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];
                double c = 1.0;
                if (r2 > 0) {
                    const double r = __builtin_sqrt(r2);
                    double m1, m2;
                    const bool ok = octa_fetch(T, depth + pi * T * T, dv[0], dv[1], dv[2], m1, m2);
                    if (ok && !(r <= m1)) {
                        const double var = __builtin_fabs(m2 - m1 * m1), dd = r - m1;
                        const double den = var + dd * dd;
                        c = den > 0 ? var / den : 0.0;
                        c = (c * c) * c;
                    }
                }
                double wv = wb * c;
                if (!(wv >= 0x1p-20)) wv = 0x1p-20;
                const double wgt = tri * wv;
                wsum = wsum + wgt, ++used;
                for (int i = 0; i < 9; ++i)
                    for (int ch = 0; ch < 3; ++ch) acc[i][ch] = acc[i][ch] + wgt * pr.c[i][ch];
            }
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (used == 0) return o;
    const double rw = 1.0 / wsum;
    for (int i = 0; i < 9; ++i)
        for (int ch = 0; ch < 3; ++ch) acc[i][ch] = rw * acc[i][ch];
    sh_irradiance(acc, q.n, nlen, o.v);
    o.count = used, o.valid = 1;
    return o;
}

/* ---- environment captures (include/rtr_hip.h: rtr_capture_*, rtr_cube_*) ----
 * The arithmetic of that contract, written once for host (rtr_capture_ray, rtr_cube_lookup_one, the entries' checks) and
 * device (k_capture_li, k_cube_lookup): the same rules as the gathers' above. */
#define RTR_CAPTURE_MAX_FACE 4096 /* rtr_hip.h: 6 S^2 and every texel of one centre fit an int32 */
struct CaptureK {
    const rtr_probe_point* pts; /* the centres of the whole call */
    rtr_gather_out* out;        /* out[0] is the record of texel `first` of the call */
    long long first;            /* texels are numbered through the call: centre * 6 S^2 + e */
    long long k0, n;            /* this launch serves the records [k0, n) of `out` */
    int S, SS, F;               /* face size, S^2, 6 S^2 */
    int samples, lg;            /* N; log2 of the group size, the gathers' gather_lg */
    uint32_t seed, point_base;
    int jitter;
    double time;
    int max_depth, rr_start;
};
/* why `p` is no valid parameter block, or nullptr */
inline const char* capture_params_why(const rtr_capture_params* p) {
    if (!p) return "null capture params";
    if (p->face_size < 1 || p->face_size > RTR_CAPTURE_MAX_FACE) return "face_size outside 1 .. 4096";
    if (p->samples < 1 || p->samples > (1 << 20)) return "samples outside 1 .. 2^20";
    if (p->jitter != 0 && p->jitter != 1) return "jitter must be 0 or 1";
    if (!__builtin_isfinite(p->time)) return "time not finite";
    if (p->pad != 0 || p->reserved[0] != 0 || p->reserved[1] != 0) return "pad and reserved must be 0";
    return nullptr;
}
/* direction of the ray through texel (a, b) of face f of an S x S cube map whose generator is `rng`; rng is left
 * behind the jitter's draws (none without jitter) */
RT_HD void capture_direction(int S, int f, int a, int b, int jitter, uint32_t& rng, double& dx, double& dy, double& dz) {
    double ju = 0.5, jv = 0.5;
    if (jitter) { /* random_double, core/rtweekend.h:24-34: one step, then state * 2^-32 */
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        ju = rng * 2.3283064365386962890625e-10;
        rng ^= rng << 13, rng ^= rng >> 17, rng ^= rng << 5;
        jv = rng * 2.3283064365386962890625e-10;
    }
    const double u = (2.0 * (a + ju)) / S - 1.0;
    const double v = (2.0 * (b + jv)) / S - 1.0;
    double x, y, z;
    switch (f) {
    case 0: x = 1.0, y = -v, z = -u; break;
    case 1: x = -1.0, y = -v, z = u; break;
    case 2: x = u, y = 1.0, z = v; break;
    case 3: x = u, y = -1.0, z = -v; break;
    case 4: x = u, y = -v, z = 1.0; break;
    default: x = -u, y = -v, z = -1.0; break;
    }
    const double r = 1 / __builtin_sqrt(x * x + y * y + z * z);
    dx = r * x, dy = r * y, dz = r * z;
}
/* rtr_cube_lookup of one direction over the 6 S^2 records of one capture */
RT_HD rtr_gather_out cube_lookup_one(int S, const rtr_gather_out* __restrict__ texels, const rtr_probe_point& q) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    const double x = q.p[0], y = q.p[1], z = q.p[2];
    const double len = __builtin_sqrt(x * x + y * y + z * z);
    if (probe_point_bad(q) || !(len > 0.0 && len < __builtin_huge_val())) return o;
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
    int f;
    double u, v;
    if (ax >= ay && ax >= az) {
        f = x > 0 ? 0 : 1;
        u = (x > 0 ? -z : z) / ax, v = -y / ax;
    } else if (ay >= az) {
        f = y > 0 ? 2 : 3;
        u = x / ay, v = (y > 0 ? z : -z) / ay;
    } else {
        f = z > 0 ? 4 : 5;
        u = (z > 0 ? x : -x) / az, v = -y / az;
    }
    int i0[2];
    double w[2][2];
    probe_axis(((u + 1.0) * S) * 0.5 - 0.5, 0.0, 1.0, S, i0[0], w[0][0], w[0][1]);
    probe_axis(((v + 1.0) * S) * 0.5 - 0.5, 0.0, 1.0, S, i0[1], w[1][0], w[1][1]);
    double acc[3] = {0.0, 0.0, 0.0};
    int used = 0;
    bool ok = true;
    for (int db = 0; db < 2; ++db)
        for (int da = 0; da < 2; ++da) {
            const int ia = i0[0] + da < S - 1 ? i0[0] + da : S - 1;
            const int ib = i0[1] + db < S - 1 ? i0[1] + db : S - 1;
            const double wc = w[0][da] * w[1][db];
            if (wc > 0) {
                const rtr_gather_out& t = texels[((long long)f * S + ib) * S + ia];
                ok = ok && t.valid != 0;
                ++used;
                for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + wc * t.v[ch];
            }
        }
    if (!ok) return o;
    o.v[0] = acc[0], o.v[1] = acc[1], o.v[2] = acc[2];
    o.count = used, o.valid = 1;
    return o;
}

/* ---- filtered cube maps (include/rtr_hip.h: rtr_cube_filter*, rtr_cube_chain_*) ----
 * The arithmetic of that contract, written once for host (the _one forms, the entries' checks) and device (k_cube_filter
 * and k_cube_chain_lookup of rt_cube.h). */
#define RTR_FILTER_MAX_FACE 512
#define RTR_CHAIN_MAX_LEVELS 13
inline const char* cube_filter_params_why(const rtr_cube_filter_params* p) {
    if (!p) return "null filter params";
    if (p->face_in < 1 || p->face_in > RTR_FILTER_MAX_FACE) return "face_in outside 1 .. 512";
    if (p->face_out < 1 || p->face_out > RTR_FILTER_MAX_FACE) return "face_out outside 1 .. 512";
    if (!(p->alpha >= 0x1p-20 && p->alpha <= 1.0)) return "alpha outside 2^-20 .. 1";
    if (!(p->cos_cut >= 0.0 && p->cos_cut < 1.0) || __builtin_signbit(p->cos_cut)) return "cos_cut outside [+0, 1)";
    if (p->pad[0] != 0 || p->pad[1] != 0) return "pad must be 0";
    return nullptr;
}
/* why the chain is none, or nullptr; n_records < 0: the levels' own ends are the only bound (rtr_cube_chain_lookup_one) */
inline const char* cube_chain_why(const rtr_cube_level* lv, int n_levels, long long n_records) {
    if (!lv) return "null levels";
    if (n_levels < 1 || n_levels > RTR_CHAIN_MAX_LEVELS) return "n_levels outside 1 .. 13";
    for (int i = 0; i < n_levels; ++i) {
        if (lv[i].face_size < 1 || lv[i].face_size > RTR_CAPTURE_MAX_FACE || lv[i].pad != 0) return "level face_size outside 1 .. 4096 or pad not 0";
        const long long recs = 6ll * lv[i].face_size * lv[i].face_size;
        if (lv[i].offset < 0 || (n_records >= 0 && (lv[i].offset > n_records || recs > n_records - lv[i].offset)))
            return "a level lies outside n_records";
        if (!__builtin_isfinite(lv[i].alpha) || (i > 0 && !(lv[i].alpha > lv[i - 1].alpha))) return "level alphas must be finite and strictly increasing";
    }
    return nullptr;
}
/* the face table of the captures: the un-normalised direction of (u, v) on face f */
RT_HD void cube_face_d0(int f, double u, double v, double& x, double& y, double& z) {
    switch (f) {
    case 0: x = 1.0, y = -v, z = -u; break;
    case 1: x = -1.0, y = -v, z = u; break;
    case 2: x = u, y = 1.0, z = v; break;
    case 3: x = u, y = -1.0, z = -v; break;
    case 4: x = u, y = -v, z = 1.0; break;
    default: x = -u, y = -v, z = -1.0; break;
    }
}
/* the centre of texel (a, b) of face f of an S x S cube: capture_direction without jitter, and the texel's solid-angle
 * weight dw = 1 / (r2 sqrt(r2)) beside the unit direction */
RT_HD void cube_texel_centre(int S, int f, int a, int b, double& lx, double& ly, double& lz, double& dw) {
    const double u = (2.0 * (a + 0.5)) / S - 1.0;
    const double v = (2.0 * (b + 0.5)) / S - 1.0;
    double x, y, z;
    cube_face_d0(f, u, v, x, y, z);
    const double r2 = x * x + y * y + z * z;
    const double root = __builtin_sqrt(r2);
    const double r = 1 / root;
    lx = r * x, ly = r * y, lz = r * z;
    dw = 1.0 / (r2 * root);
}
/* n / d of the filter's weight.  The device takes the short form of "IEEE division with a shared divisor" (rt_device.h):
 * the compiler's own sequence without the scales and the fixup, the same bits while |d| is in [2^-100, 2^100] and |n| in
 * [2^-300, 2^200].  Both hold for every USED pair: d = den * den with den = h2 (alpha^2 - 1) + 1, h2 within an ulp of
 * (1/2, 1] and alpha^2 in [2^-40, 1], so d is in [2^-84, 4]; n = c * dw with dw in [0.19, 1] and c > 0 a sum of three
 * products of components that are each at least 2^-10.5 or zero, hence a multiple of 2^-74 and at most 1 + 2^-50.  The
 * host divides. */
RT_HD double filter_quotient(double n, double d) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double r = rcp_refined(d);
    const double q = n * r;
    return __builtin_fma(__builtin_fma(-d, q, n), r, q);
#else
    return n / d;
#endif
}
/* the running sums of one lane for one output texel */
struct FilterAcc {
    double v[3], wsum;
    int count, bad;
};
RT_HD void filter_acc_zero(FilterAcc& s) { s.v[0] = s.v[1] = s.v[2] = s.wsum = 0.0, s.count = 0, s.bad = 0; }
/* w of the pair whose cosine c is USED */
RT_HD double filter_weight(double c, double dw, double a2m1) {
    const double h2 = (1.0 + c) * 0.5;
    const double den = h2 * a2m1 + 1.0;
    return filter_quotient(c * dw, den * den);
}
RT_HD void filter_add(FilterAcc& s, double w, double v0, double v1, double v2, int valid) {
    s.v[0] = s.v[0] + w * v0, s.v[1] = s.v[1] + w * v1, s.v[2] = s.v[2] + w * v2;
    s.wsum = s.wsum + w;
    s.count += 1, s.bad += valid == 0;
}
/* the record of the sums of all 64 lanes */
RT_HD rtr_gather_out filter_result(const FilterAcc& s) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (s.count == 0 || s.bad != 0 || !(s.wsum > 0.0 && s.wsum < __builtin_huge_val())) return o;
    const double r = 1.0 / s.wsum;
    o.v[0] = r * s.v[0], o.v[1] = r * s.v[1], o.v[2] = r * s.v[2];
    o.count = s.count, o.valid = 1;
    return o;
}

/* face and (u, v) of a direction with a major axis: the rule of cube_lookup_one (x over y over z on a tie), which keeps
 * its own lines so that k_cube_lookup stays the text it was */
RT_HD void cube_face_uv(double x, double y, double z, int& f, double& u, double& v) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
    if (ax >= ay && ax >= az) {
        f = x > 0 ? 0 : 1;
        u = (x > 0 ? -z : z) / ax, v = -y / ax;
    } else if (ay >= az) {
        f = y > 0 ? 2 : 3;
        u = x / ay, v = (y > 0 ? z : -z) / ay;
    } else {
        f = z > 0 ? 4 : 5;
        u = (z > 0 ? x : -x) / az, v = -y / az;
    }
}
RT_HD int cube_texel_of(double c, int S) {
    const int i = (int)(((c + 1.0) * S) * 0.5);
    return i < 0 ? 0 : (i > S - 1 ? S - 1 : i);
}
/* the seam-aware lookup of one level: its 6 S^2 records */
RT_HD rtr_gather_out cube_seam_lookup(int S, const rtr_gather_out* __restrict__ texels, double x, double y, double z) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    int f;
    double uv[2];
    cube_face_uv(x, y, z, f, uv[0], uv[1]);
    int i0[2];
    double w[2][2];
    for (int k = 0; k < 2; ++k) {
        const double g = ((uv[k] + 1.0) * S) * 0.5 - 0.5;
        const double fl = __builtin_floor(g);
        i0[k] = (int)fl;
        const double t = g - fl;
        w[k][0] = 1.0 - t, w[k][1] = t;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    int used = 0;
    bool ok = true;
    for (int db = 0; db < 2; ++db)
        for (int da = 0; da < 2; ++da) {
            const double wc = w[0][da] * w[1][db];
            if (wc > 0) {
                int ia = i0[0] + da, ib = i0[1] + db, ft = f;
                if (ia < 0 || ia >= S || ib < 0 || ib >= S) {
                    const double u1 = (2.0 * (ia + 0.5)) / S - 1.0, v1 = (2.0 * (ib + 0.5)) / S - 1.0;
                    double dx, dy, dz, u2, v2;
                    cube_face_d0(f, u1, v1, dx, dy, dz);
                    cube_face_uv(dx, dy, dz, ft, u2, v2);
                    ia = cube_texel_of(u2, S), ib = cube_texel_of(v2, S);
                }
                const rtr_gather_out& t = texels[((long long)ft * S + ib) * S + ia];
                ok = ok && t.valid != 0;
                ++used;
                for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + wc * t.v[ch];
            }
        }
    if (!ok) return o;
    o.v[0] = acc[0], o.v[1] = acc[1], o.v[2] = acc[2];
    o.count = used, o.valid = 1;
    return o;
}
/* the levels of a chain as a kernel argument */
struct ChainK {
    rtr_cube_level lv[RTR_CHAIN_MAX_LEVELS];
    int n;
};
/* where level `l` of cube `cube` starts in an array that holds `cubes` chains level-major (a capture set; include/rtr_hip.h:
 * CAPTURE SETS): a single chain is (1, 0), the level's own offset */
RT_HD long long cube_level_base(const rtr_cube_level& l, long long cubes, long long cube) {
    return l.offset * cubes + cube * (6ll * l.face_size * l.face_size);
}
/* rtr_cube_chain_lookup of one query over the records of a valid chain: chain `cube` of `cubes` */
RT_HD rtr_gather_out cube_chain_lookup_one(const rtr_cube_level* lv, int n, const rtr_gather_out* __restrict__ texels,
                                           const rtr_cube_query& q, long long cubes, long long cube) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    const double x = q.d[0], y = q.d[1], z = q.d[2];
    rtr_probe_point p;
    p.p[0] = x, p.p[1] = y, p.p[2] = z;
    const double len = __builtin_sqrt(x * x + y * y + z * z);
    if (probe_point_bad(p) || !(len > 0.0 && len < __builtin_huge_val()) || !__builtin_isfinite(q.alpha)) return o;
    double a = q.alpha > lv[0].alpha ? q.alpha : lv[0].alpha;
    a = a < lv[n - 1].alpha ? a : lv[n - 1].alpha;
    int i = 0;
    for (int k = 1; k < n; ++k)
        if (lv[k].alpha <= a) i = k;
    if (n >= 2 && i > n - 2) i = n - 2;
    const double t = n >= 2 ? (a - lv[i].alpha) / (lv[i + 1].alpha - lv[i].alpha) : 0.0;
    const rtr_gather_out x0 = cube_seam_lookup(lv[i].face_size, texels + cube_level_base(lv[i], cubes, cube), x, y, z);
    if (t == 0) return x0;
    const rtr_gather_out x1 = cube_seam_lookup(lv[i + 1].face_size, texels + cube_level_base(lv[i + 1], cubes, cube), x, y, z);
    if (!x0.valid || !x1.valid) return o;
    for (int ch = 0; ch < 3; ++ch) o.v[ch] = (1.0 - t) * x0.v[ch] + t * x1.v[ch];
    o.count = x0.count + x1.count, o.valid = 1;
    return o;
}

/* ---- capture sets (include/rtr_hip.h: rtr_capture_set*) ----
 * The arithmetic of that contract, written once for host (the _one forms, the entries' checks) and device
 * (k_capture_set_lookup of rt_cube.h, the set forms of the shader and of the preview). */
#define RTR_CAPTURE_SET_MAX 16
/* a valid set as a kernel argument, next to ChainK / ShadeK: 2056 bytes.  The loop below indexes it with a counter that is
 * the same in every lane, so a volume comes in through scalar loads */
struct SetK {
    int n, fallback;
    rtr_capture_volume vol[RTR_CAPTURE_SET_MAX];
};
/* why the set is none, or nullptr */
inline const char* capture_set_why(const rtr_capture_set* s) {
    if (!s) return "null capture set";
    if (s->n_captures < 1 || s->n_captures > RTR_CAPTURE_SET_MAX) return "n_captures outside 1 .. 16";
    if (s->fallback < -1 || s->fallback >= s->n_captures) return "fallback outside -1 .. n_captures - 1";
    if (!s->volumes) return "null volumes";
    for (int k = 0; k < s->n_captures; ++k) {
        const rtr_capture_volume& v = s->volumes[k];
        bool finite = __builtin_isfinite(v.fade);
        for (int a = 0; a < 3; ++a)
            finite = finite && __builtin_isfinite(v.centre[a]) && __builtin_isfinite(v.proxy_lo[a]) && __builtin_isfinite(v.proxy_hi[a]) &&
                     __builtin_isfinite(v.reach_lo[a]) && __builtin_isfinite(v.reach_hi[a]);
        if (!finite) return "a volume has a non-finite number";
        for (int a = 0; a < 3; ++a) {
            if (!(v.proxy_lo[a] < v.centre[a] && v.centre[a] < v.proxy_hi[a])) return "a centre is not strictly inside its proxy box";
            if (!(v.proxy_lo[a] <= v.reach_lo[a] && v.reach_lo[a] <= v.reach_hi[a] && v.reach_hi[a] <= v.proxy_hi[a]))
                return "a reach box is empty or leaves its proxy box";
        }
        if (!(v.fade >= 0.0) || __builtin_signbit(v.fade)) return "fade outside [+0, inf)";
    }
    return nullptr;
}
inline SetK set_k(const rtr_capture_set* s) {
    SetK S{};
    S.n = s->n_captures, S.fallback = s->fallback;
    for (int k = 0; k < s->n_captures; ++k) S.vol[k] = s->volumes[k];
    return S;
}
/* BAD: one of the seven numbers is not finite, or the length of d is not in (0, inf) */
RT_HD bool capture_query_bad(const double* p, const double* d, double alpha) {
    bool ok = __builtin_isfinite(alpha);
    for (int a = 0; a < 3; ++a) ok = ok && __builtin_isfinite(p[a]) && __builtin_isfinite(d[a]);
    const double len = __builtin_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    return !(ok && len > 0.0 && len < __builtin_huge_val());
}
/* SET LOOKUP of (p, d, alpha) over the level-major records of a valid set and the chain plan of one capture.  One loop with
 * one chain lookup in it: round S.n is the fallback's, taken when no capture reached p, so the lookup's text and registers
 * exist once.  A capture that does not reach p costs its six subtractions; a lane no capture reaches and without a fallback
 * reads no record */
RT_HD rtr_gather_out capture_set_lookup_one(const SetK& S, const rtr_cube_level* lv, int n, const rtr_gather_out* __restrict__ texels,
                                            const double* p, const double* d, double alpha) {
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (capture_query_bad(p, d, alpha)) return o;
    double acc[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
    int count = 0, used = 0;
#pragma unroll 1
    for (int k = 0; k <= S.n; ++k) {
        rtr_cube_query cq;
        cq.alpha = alpha;
        double w = 1.0;
        int cube = k;
        if (k < S.n) {
            const rtr_capture_volume& V = S.vol[k];
            double m = p[0] - V.reach_lo[0];
            for (int a = 0; a < 3; ++a) {
                if (a > 0) {
                    const double lo = p[a] - V.reach_lo[a];
                    m = lo < m ? lo : m;
                }
                const double hi = V.reach_hi[a] - p[a];
                m = hi < m ? hi : m;
            }
            if (m < 0) continue;
            if (V.fade != 0) {
                const double r = m / V.fade;
                w = 1.0 < r ? 1.0 : r;
            }
            if (!(w > 0)) continue;
            double t = __builtin_huge_val();
            for (int a = 0; a < 3; ++a) {
                if (d[a] > 0) {
                    const double ta = (V.proxy_hi[a] - p[a]) / d[a];
                    t = ta < t ? ta : t;
                } else if (d[a] < 0) {
                    const double ta = (V.proxy_lo[a] - p[a]) / d[a];
                    t = ta < t ? ta : t;
                }
            }
            for (int a = 0; a < 3; ++a) cq.d[a] = (p[a] + t * d[a]) - V.centre[a];
        } else {
            if (used > 0 || S.fallback < 0) break;
            for (int a = 0; a < 3; ++a) cq.d[a] = d[a];
            cube = S.fallback;
        }
        const rtr_gather_out X = cube_chain_lookup_one(lv, n, texels, cq, S.n, cube);
        if (k == S.n) return X;
        if (!X.valid) return o;
        for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + w * X.v[ch];
        wsum = wsum + w, count += X.count, ++used;
    }
    if (used == 0) return o;
    const double r = 1.0 / wsum;
    o.v[0] = r * acc[0], o.v[1] = r * acc[1], o.v[2] = r * acc[2];
    o.count = count, o.valid = 1;
    return o;
}

struct ResolveK {
    RenderK r;
    double* out; /* linear mean radiance, 3 doubles per pixel */
    long long row_stride; /* pixels per row of `out`; < 0: `out` is PACKED -- owned tile k of the call at out[k * 768 ...]
                             as 16 rows (lowest y first) of 16 pixels, and tile_done[k] = 1 once its sums are stored */
    unsigned char* tile_done;
    int done_full; /* a chunk ran to the end when its word of r.done is nonzero (0), or equals this count: the jobs of a
                      cell of a queue render (k_mega_queue), which count themselves there one by one */
};

/* rtr_accum_resolve: the accumulator's sums and sample counts (r.tile_ids = its owned tiles) -> packed tiles of linear
 * mean radiance and/or of the reference's 8-bit store; a tile with count 0 is not written */
struct AccumResolveK {
    RenderK r;
    const double* sum;    /* [n_tiles][3][RTR_BLOCK] */
    const int* count;     /* [n_tiles] */
    double* out;          /* null or [n_tiles][RTR_BLOCK][3], lowest row first */
    unsigned char* rgb8;  /* null or [n_tiles][RTR_BLOCK][3], lowest row first (the host flips Y) */
};

