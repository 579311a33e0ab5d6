/*
 * rtr_probe.hip -- light probes (include/rtr_hip.h: rtr_probe_*, rtr_sh_*): the point checks, the kernel choice
 * among the 22 kernels held here (5 k_probe_any, 17 k_probe_li), k_probe_lookup and its launch, the entries, and the
 * host-only pieces that need no context (rtr_probe_ray, rtr_sh_basis, rtr_sh_irradiance, rtr_probe_lookup_one).  Which
 * k_probe_li a radiance call runs is the k_li family rule of rt_select.h, like the gathers'.  The grid rule is
 * rt_render.h's.  The entries' common checks, the staging of the host entries, the body of the device entries, the launch
 * set-up, the chunked launcher and the single-ray entry are rt_batch.h's, shared with the other batch units.
 */
#include "rt_batch.h"

using namespace rtr;

/* rtr_probe_lookup: one lane per query, eight records of 224 bytes each, straight-line (probe_lookup_one of rt_render.h) */
__global__ void __launch_bounds__(RTR_BLOCK) k_probe_lookup(const rtr_probe_grid g, const rtr_probe_sh* __restrict__ probes,
                                                             const rtr_gather_point* __restrict__ queries,
                                                             rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const rtr_gather_point q = queries[k];
    double nlen;
    rtr_gather_out o;
    o.v[0] = o.v[1] = o.v[2] = 0.0, o.count = 0, o.valid = 0;
    if (!gather_point_bad(q, nlen)) o = probe_lookup_one(g, probes, q, nlen);
    out[k] = o;
}

namespace {

constexpr int64_t kProbeSlice = (int64_t)1 << 20; /* points per slice of the host entries */

/* what every probe entry checks before any device work; `radiance`: rp is checked too (a NULL one is invalid) */
int probe_check(rtr_context* c, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp, const void* pts,
                const void* out, int64_t n) {
    return points_check(c, "rtr_probe_*", rp, radiance, gp, n, pts && out);
}
int probe_check_points(rtr_context* c, const rtr_probe_point* pts, int64_t n) {
    return records_check(c, "rtr_probe_*", "point", kPositionRule, n, [&](int64_t k) { return probe_point_bad(pts[k]); });
}

/* launches over device arrays on the context stream; rp: radiance probes (k_probe_li), else visibility (k_probe_any) */
int probe_launch(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, uint32_t point_base,
                 const rtr_probe_point* d_pts, void* d_out, int64_t n) {
    PointLaunch<ProbeK> L = point_launch<ProbeK>(c, rp, gp);
    L.k.pts = d_pts, L.k.out = d_out, L.k.n = (long long)n, L.k.point_base = point_base;
    /* the traversal stack, and behind it the per-lane sums of k_probe_li (rt_kernels.h: ProbeSums) */
    L.k.sum_word = (int)(L.stack / sizeof(int));
    const size_t lds = L.stack + (rp ? probe_sum_bytes() : 0);
    int rc = RTR_OK;
    const auto launch = [&](auto kernel, size_t out_rec) {
        rc = launch_records(c, "rtr_probe_*", kernel, lds, L.k.n, L.k.lg, point_args(L.ds, L.k, out_rec));
    };
    const bool found =
        rp ? dispatch_li(L.integ, L.trav, [&](auto i, auto t) { launch(k_probe_li<decltype(i)::value, decltype(t)::value>, sizeof(rtr_probe_sh)); })
           : dispatch_trav(TravsTop{}, L.trav, [&](auto t) { launch(k_probe_any<decltype(t)::value>, sizeof(rtr_probe_vis)); });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no probe kernel for traversal " + std::to_string(L.trav));
    if (rc == RTR_OK) c->last_batch[RTR_DEBUG_PROBE] = rtr_debug_batch{L.integ, L.trav, 0, L.k.lg};
    return rc;
}

/* slices of at most kProbeSlice points (staged_slices of rt_batch.h), each at its point_base */
int probe_host(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_probe_point* pts, void* out,
               int64_t n) {
    const StagedIO io{0, sizeof(rtr_probe_point), pts, {rp ? sizeof(rtr_probe_sh) : sizeof(rtr_probe_vis), 0}, {out, nullptr}};
    return staged_slices(c, n, kProbeSlice, io, [&](const Slice& s) {
        return probe_launch(c, rp, gp, gp->point_base + (uint32_t)s.k0, static_cast<const rtr_probe_point*>(s.in), s.out[0], s.m);
    });
}

int probe_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_probe_point* d_pts, void* d_out,
                 int64_t n, int blocking) {
    return device_entry(c, "rtr_probe_*_device", (uintptr_t)d_pts | (uintptr_t)d_out, blocking,
                        [&] { return probe_launch(c, rp, gp, gp->point_base, d_pts, d_out, n); });
}

/* what both lookup entries check before any device work, in this order: context, grid, n / NULL; no scene is needed */
int lookup_check(rtr_context* c, const rtr_probe_grid* g, const void* probes, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = probe_grid_why(g)) return fail(c, RTR_ERR_INVALID, std::string("rtr_probe_lookup: ") + why);
    return batch_check(c, "rtr_probe_lookup", n, probes && q && out);
}
int lookup_launch(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* d_probes, const rtr_gather_point* d_q,
                  rtr_gather_out* d_out, int64_t n) {
    return launch_records(c, "rtr_probe_lookup", k_probe_lookup, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(*g, d_probes, d_q + k0, d_out + k0, m); });
}

} // namespace

extern "C" {

int rtr_probe_visibility(rtr_context* c, const rtr_gather_params* gp, const rtr_probe_point* pts, rtr_probe_vis* out, int64_t n) {
    if (int rc = probe_check(c, nullptr, false, gp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = probe_check_points(c, pts, n)) return rc;
    return probe_host(c, nullptr, gp, pts, out, n);
}

int rtr_probe_radiance(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_probe_point* pts,
                       rtr_probe_sh* out, int64_t n) {
    if (int rc = probe_check(c, rp, true, gp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = probe_check_points(c, pts, n)) return rc;
    return probe_host(c, rp, gp, pts, out, n);
}

int rtr_probe_visibility_device(rtr_context* c, const rtr_gather_params* gp, const rtr_probe_point* d_pts, rtr_probe_vis* d_out,
                                int64_t n, int blocking) {
    if (int rc = probe_check(c, nullptr, false, gp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return probe_device(c, nullptr, gp, d_pts, d_out, n, blocking);
}

int rtr_probe_radiance_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp,
                              const rtr_probe_point* d_pts, rtr_probe_sh* d_out, int64_t n, int blocking) {
    if (int rc = probe_check(c, rp, true, gp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return probe_device(c, rp, gp, d_pts, d_out, n, blocking);
}

int rtr_probe_ray(const rtr_gather_params* params, const rtr_probe_point* point, int64_t index_in_call, int32_t s, rtr_ray* out) {
    return sample_ray(params, point ? point->p : nullptr, index_in_call, s, out, [&](uint32_t& rng, double* d) {
        if (probe_point_bad(*point)) return false;
        probe_direction(rng, d[0], d[1], d[2]);
        return true;
    });
}

void rtr_sh_basis(const double d[3], double y[9]) {
    if (d && y) sh_basis(d[0], d[1], d[2], y);
}

int rtr_sh_irradiance(const double c[9][3], const double n[3], double E[3]) {
    if (!c || !n || !E) return RTR_ERR_INVALID;
    rtr_gather_point q{};
    for (int a = 0; a < 3; ++a) q.n[a] = n[a];
    double nlen;
    if (gather_point_bad(q, nlen)) return RTR_ERR_INVALID;
    sh_irradiance(c, n, nlen, E);
    return RTR_OK;
}

int rtr_probe_lookup_one(const rtr_probe_grid* g, const rtr_probe_sh* probes, const rtr_gather_point* query, rtr_gather_out* out) {
    double nlen;
    if (probe_grid_why(g) || !probes || !query || !out || gather_point_bad(*query, nlen)) return RTR_ERR_INVALID;
    *out = probe_lookup_one(*g, probes, *query, nlen);
    return RTR_OK;
}

int rtr_probe_lookup(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* probes, const rtr_gather_point* q,
                     rtr_gather_out* out, int64_t n) {
    if (int rc = lookup_check(c, g, probes, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_probe_lookup", "query", kGatherPointRule, n, [&](int64_t k) {
            double nlen;
            return gather_point_bad(q[k], nlen);
        }))
        return rc;
    /* the grid stays at the head of the staging buffer for all slices: the first one brings it */
    static_assert(sizeof(rtr_probe_sh) % 16 == 0, "StagedIO::head_bytes");
    const size_t grid_bytes = (size_t)grid_probes(g) * sizeof(rtr_probe_sh);
    const StagedIO io{grid_bytes, sizeof(rtr_gather_point), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kProbeSlice, io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, probes, grid_bytes, hipMemcpyHostToDevice, c->stream));
        return lookup_launch(c, g, static_cast<const rtr_probe_sh*>(s.head), static_cast<const rtr_gather_point*>(s.in),
                             static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_probe_lookup_device(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* d_probes, const rtr_gather_point* d_q,
                            rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = lookup_check(c, g, d_probes, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_probe_lookup_device", (uintptr_t)d_probes | (uintptr_t)d_q | (uintptr_t)d_out, blocking,
                        [&] { return lookup_launch(c, g, d_probes, d_q, d_out, n); });
}

} /* extern "C" */
