/*
 * rtr_probe_depth.hip -- probe distance maps (include/rtr_hip.h: rtr_probe_depth*, rtr_octa_*, rtr_probe_lookup_visible*):
 * k_probe_depth over TravsTop (the set k_query_closest has: a map is a batch of closest-hit queries made in registers),
 * k_probe_lookup_visible and its launch, the entries, and the host-only pieces that need no context
 * (rtr_probe_depth_defaults, rtr_probe_depth_ray, rtr_octa_encode / _decode, rtr_probe_lookup_visible_one).  The arithmetic
 * and the grid rule are rt_render.h's, written once for host and device; the lane-to-record map is group_begin of
 * rt_kernels.h.  The entries' common checks, the staging of the host entries, the body of the device entries, the chunked
 * launcher and the single-ray entry are rt_batch.h's, shared with the other batch units.
 */
#include "rt_batch.h"

using namespace rtr;

/* rtr_probe_depth: a texel of a probe's map is a "point" of the gathers' mapping, as a texel of a capture is: global lane
 * g serves record K.k0 + g / G of K.out as lane g % G, a group never leaves its wave, lanes without a sample, of a bad
 * probe or past the end carry +0.0 / 0 through every __shfl_xor, lane 0 of a group stores the record.  The texel number
 * of the call (K.first + record) gives the probe (texel / T^2) and (row, column). */
struct DepthLane {
    long long k;    /* record of K.out of this lane's group */
    int l;          /* lane in the group */
    bool cast;      /* the texel exists and its probe is not bad */
    V3 p;
    int e, a, b;    /* texel of the probe's map: e = b * T + a */
    uint32_t probe; /* the probe's number under the seed: its index in the call + point_base */
};
RT_DEV bool depth_begin(const DepthK& K, DepthLane& L) {
    if (!group_begin(K.k0, K.n, K.lg, L.k, L.l)) return false;
    const bool live = L.k < K.n;
    const long long texel = K.first + (live ? L.k : K.k0);
    const long long c = texel / K.TT;
    L.e = (int)(texel - c * K.TT);
    L.b = L.e / K.T, L.a = L.e - L.b * K.T;
    L.probe = (uint32_t)c + K.point_base;
    rtr_probe_point q;
    for (int i = 0; i < 3; ++i) q.p[i] = 0.0;
    if (live) q = K.pts[c];
    L.cast = !probe_point_bad(q) && live;
    L.p = ld3(q.p);
    return true;
}
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_probe_depth(const DScene sc, const DepthK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    DepthLane L;
    if (!depth_begin(K, L)) return;
    double m1 = 0.0, m2 = 0.0;
    int hits = 0, back = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            uint32_t rng = rtr_sample_seed_inline(K.seed, K.TT, L.e, (int32_t)L.probe, s);
            V3 d;
            depth_direction(K.T, L.a, L.b, K.jitter, rng, d.x, d.y, d.z);
            Hit rec;
            rec.u = rec.v = __builtin_nan("");
            rec.mat = -1;
            rec.t = 0, rec.p = mk(0, 0, 0), rec.n = mk(0, 0, 0), rec.front = false;
            const bool hit = cast_closest<TRAV>(sc, L.p, d, K.time, rec, rng, st, K.t_min, K.t_max);
            const double x = hit ? rec.t : K.t_max;
            m1 = m1 + x, m2 = m2 + x * x;
            if (hit) ++hits, back += rec.front ? 0 : 1;
        }
    for (int off = (1 << K.lg) >> 1; off > 0; off >>= 1) {
        m1 = m1 + __shfl_xor(m1, off, 64), m2 = m2 + __shfl_xor(m2, off, 64);
        hits = hits + __shfl_xor(hits, off, 64), back = back + __shfl_xor(back, off, 64);
    }
    if (L.l != 0 || L.k >= K.n) return;
    rtr_probe_depth_texel o;
    const double scale = 1.0 / K.samples;
    o.mean = L.cast ? scale * m1 : 0.0, o.mean2 = L.cast ? scale * m2 : 0.0;
    o.hits = L.cast ? hits : 0, o.back = L.cast ? back : 0, o.valid = L.cast ? 1 : 0, o.pad = 0;
    K.out[L.k] = o;
}

/* rtr_probe_lookup_visible: one lane per query, straight-line (probe_lookup_visible_one of rt_render.h) */
__global__ void __launch_bounds__(RTR_BLOCK) k_probe_lookup_visible(const rtr_probe_grid g, const rtr_probe_sh* __restrict__ probes,
                                                                     const rtr_probe_depth_texel* __restrict__ depth, const int T,
                                                                     const double normal_bias,
                                                                     const rtr_gather_point* __restrict__ queries,
                                                                     rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const rtr_gather_point q = queries[k];
    double nlen;
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (!gather_point_bad(q, nlen)) o = probe_lookup_visible_one(g, probes, depth, T, normal_bias, q, nlen);
    out[k] = o;
}

namespace {

constexpr int64_t kDepthSlice = (int64_t)1 << 20; /* texels (queries of a lookup) per slice of the host entries */

/* what both map entries check before any device work, in the captures' order: context, params, n / NULL, scene */
int depth_check(rtr_context* c, const rtr_probe_depth_params* dp, const void* pts, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = probe_depth_params_why(dp)) return fail(c, RTR_ERR_INVALID, std::string("rtr_probe_depth: ") + why);
    if (int rc = batch_check(c, "rtr_probe_depth", n, pts && out)) return rc;
    return scene_check(c, "rtr_probe_depth");
}

/* launches over the device array of the call's probes on the context stream: the records [0, m) of d_out, which are the
 * texels first .. first + m of the call */
int depth_launch(rtr_context* c, const rtr_probe_depth_params* dp, const rtr_probe_point* d_pts, rtr_probe_depth_texel* d_out,
                 long long first, long long m) {
    const int trav = per_ray_trav(c->facts, c->info, 0, true); /* what rtr_query_closest walks */
    const size_t lds = stack_bytes(c->facts, c->info, trav);
    DScene ds = c->ds;
    if (!(dp->t_min >= 0x1p-100)) ds.shared_div = 0; /* the plain divisions, as k_query_* per wave */
    DepthK K{};
    K.pts = d_pts, K.out = d_out, K.first = first, K.k0 = 0, K.n = m;
    K.T = dp->map_size, K.TT = K.T * K.T;
    K.samples = dp->samples, K.lg = gather_lg(dp->samples), K.seed = dp->seed, K.point_base = dp->point_base;
    K.jitter = dp->jitter, K.time = dp->time, K.t_min = dp->t_min, K.t_max = dp->t_max;
    int rc = RTR_OK;
    if (!dispatch_trav(TravsTop{}, trav, [&](auto t) {
            rc = launch_records(c, "rtr_probe_depth", k_probe_depth<decltype(t)::value>, lds, K.n, K.lg, texel_args(ds, K));
        }))
        return no_per_ray_kernel(c, trav);
    if (rc == RTR_OK) c->last_batch[RTR_DEBUG_PROBE_DEPTH] = rtr_debug_batch{-1, trav, 0, K.lg};
    return rc;
}

/* the grid rule of rtr_probe_lookup, and the maps' rules on top of it */
const char* visible_grid_why(const rtr_probe_grid* g, const rtr_probe_visible_params* vp) {
    const char* why = probe_grid_why(g);
    return why ? why : probe_maps_why(g, vp);
}

/* what the lookup entries check before any device work, in this order: context, grid, params, n / NULL; no scene is needed */
int visible_check(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_visible_params* vp, bool arrays, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = visible_grid_why(g, vp)) return fail(c, RTR_ERR_INVALID, std::string("rtr_probe_lookup_visible: ") + why);
    return batch_check(c, "rtr_probe_lookup_visible", n, arrays);
}
int visible_launch(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_visible_params* vp, const rtr_probe_sh* d_probes,
                   const rtr_probe_depth_texel* d_depth, const rtr_gather_point* d_q, rtr_gather_out* d_out, int64_t n) {
    return launch_records(c, "rtr_probe_lookup_visible", k_probe_lookup_visible, 0, n, 0, [&](long long k0, long long m) {
        return std::make_tuple(*g, d_probes, d_depth, vp->map_size, vp->normal_bias, d_q + k0, d_out + k0, m);
    });
}

} // namespace

extern "C" {

void rtr_probe_depth_defaults(rtr_probe_depth_params* p) {
    if (!p) return;
    *p = rtr_probe_depth_params{};
    p->map_size = 16, p->samples = 8, p->jitter = 1, p->t_min = 0.001;
}

int rtr_probe_depth(rtr_context* c, const rtr_probe_depth_params* dp, const rtr_probe_point* pts, rtr_probe_depth_texel* out,
                    int64_t n) {
    if (int rc = depth_check(c, dp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_probe_depth", "probe", kPositionRule, n, [&](int64_t k) { return probe_point_bad(pts[k]); }))
        return rc;
    return staged_texels(c, pts, n, (long long)dp->map_size * dp->map_size, sizeof(rtr_probe_depth_texel), out, kDepthSlice,
                         [&](const rtr_probe_point* d_pts, void* d_out, long long first, long long m) {
                             return depth_launch(c, dp, d_pts, static_cast<rtr_probe_depth_texel*>(d_out), first, m);
                         });
}

int rtr_probe_depth_device(rtr_context* c, const rtr_probe_depth_params* dp, const rtr_probe_point* d_pts,
                           rtr_probe_depth_texel* d_out, int64_t n, int blocking) {
    if (int rc = depth_check(c, dp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_probe_depth_device", (uintptr_t)d_pts | (uintptr_t)d_out, blocking,
                        [&] { return depth_launch(c, dp, d_pts, d_out, 0, n * dp->map_size * dp->map_size); });
}

int rtr_probe_depth_ray(const rtr_probe_depth_params* dp, const rtr_probe_point* point, int64_t index_in_call, int32_t a, int32_t b,
                        int32_t s, rtr_ray* out) {
    if (probe_depth_params_why(dp)) return RTR_ERR_INVALID;
    const int T = dp->map_size;
    if (a < 0 || a >= T || b < 0 || b >= T) return RTR_ERR_INVALID;
    const RaySeed seed{dp->seed, dp->point_base, T * T, b * T + a, dp->samples, dp->time, dp->t_min, dp->t_max};
    return sample_ray(seed, point ? point->p : nullptr, index_in_call, s, out, [&](uint32_t& rng, double* d) {
        if (probe_point_bad(*point)) return false;
        depth_direction(T, a, b, dp->jitter, rng, d[0], d[1], d[2]);
        return true;
    });
}

void rtr_octa_encode(const double d[3], double uv[2]) {
    if (d && uv) octa_encode(d[0], d[1], d[2], uv[0], uv[1]);
}

void rtr_octa_decode(const double uv[2], double d[3]) {
    if (d && uv) octa_decode(uv[0], uv[1], d[0], d[1], d[2]);
}

int rtr_probe_lookup_visible_one(const rtr_probe_grid* g, const rtr_probe_sh* probes, const rtr_probe_depth_texel* depth,
                                 const rtr_probe_visible_params* vp, const rtr_gather_point* query, rtr_gather_out* out) {
    double nlen;
    if (visible_grid_why(g, vp) || !probes || !depth || !query || !out || gather_point_bad(*query, nlen)) return RTR_ERR_INVALID;
    *out = probe_lookup_visible_one(*g, probes, depth, vp->map_size, vp->normal_bias, *query, nlen);
    return RTR_OK;
}

int rtr_probe_lookup_visible(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* probes, const rtr_probe_depth_texel* depth,
                             const rtr_probe_visible_params* vp, const rtr_gather_point* q, rtr_gather_out* out, int64_t n) {
    if (int rc = visible_check(c, g, vp, probes && depth && q && out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_probe_lookup_visible", "query", kGatherPointRule, n, [&](int64_t k) {
            double nlen;
            return gather_point_bad(q[k], nlen);
        }))
        return rc;
    /* the SH records and behind them the maps stay at the head of the staging buffer for all slices: the first one brings them */
    static_assert(sizeof(rtr_probe_sh) % 16 == 0 && sizeof(rtr_probe_depth_texel) % 16 == 0, "StagedIO::head_bytes");
    const size_t sh_bytes = (size_t)grid_probes(g) * sizeof(rtr_probe_sh);
    const size_t map_bytes = (size_t)grid_probes(g) * vp->map_size * vp->map_size * sizeof(rtr_probe_depth_texel);
    const StagedIO io{sh_bytes + map_bytes, sizeof(rtr_gather_point), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kDepthSlice, io, [&](const Slice& s) {
        char* head = static_cast<char*>(s.head);
        if (s.k0 == 0) {
            HIPCHK(c, hipMemcpyAsync(head, probes, sh_bytes, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(head + sh_bytes, depth, map_bytes, hipMemcpyHostToDevice, c->stream));
        }
        return visible_launch(c, g, vp, reinterpret_cast<const rtr_probe_sh*>(head),
                              reinterpret_cast<const rtr_probe_depth_texel*>(head + sh_bytes),
                              static_cast<const rtr_gather_point*>(s.in), static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_probe_lookup_visible_device(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* d_probes,
                                    const rtr_probe_depth_texel* d_depth, const rtr_probe_visible_params* vp,
                                    const rtr_gather_point* d_q, rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = visible_check(c, g, vp, d_probes && d_depth && d_q && d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_probe_lookup_visible_device",
                        (uintptr_t)d_probes | (uintptr_t)d_depth | (uintptr_t)d_q | (uintptr_t)d_out, blocking,
                        [&] { return visible_launch(c, g, vp, d_probes, d_depth, d_q, d_out, n); });
}

} /* extern "C" */
