/*
 * rtr_probe.hip -- light probes (include/rtr_hip.h: rtr_probe_*, rtr_sh_*): the point and grid checks, the kernel choice
 * among the 22 kernels held here (5 k_probe_any, 17 k_probe_li), k_probe_lookup and its launch, the entries, and the
 * host-only pieces that need no context (rtr_probe_ray, rtr_sh_basis, rtr_sh_irradiance, rtr_probe_lookup_one).  Which
 * k_probe_li a radiance call runs is the k_li family rule of rt_select.h, like the gathers'.  The entries' common checks,
 * the staging of the host entries, the body of the device entries, the launch set-up and the chunked launcher are
 * rt_batch.h's, shared with the gathers.
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
    for (int64_t k = 0; k < n; ++k)
        if (probe_point_bad(pts[k]))
            return fail(c, RTR_ERR_INVALID, "rtr_probe_*: bad point at index " + std::to_string(k) + " (non-finite position)");
    return RTR_OK;
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
    const bool found =
        rp ? dispatch_li(L.integ, L.trav, [&](auto i, auto t) {
                 rc = launch_points(c, k_probe_li<decltype(i)::value, decltype(t)::value>, L.ds, L.k, sizeof(rtr_probe_sh), lds);
             })
           : dispatch_trav(TravsTop{}, L.trav, [&](auto t) {
                 rc = launch_points(c, k_probe_any<decltype(t)::value>, L.ds, L.k, sizeof(rtr_probe_vis), lds);
             });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no probe kernel for traversal " + std::to_string(L.trav));
    if (rc == RTR_OK) c->last_probe = rtr_debug_probe{L.integ, L.trav, L.k.lg};
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

bool probe_grid_ok(const rtr_probe_grid* g, std::string& why) {
    if (!g) return (why = "null grid", false);
    long long count = 1;
    for (int a = 0; a < 3; ++a) {
        if (!__builtin_isfinite(g->origin[a])) return (why = "origin not finite", false);
        if (!(__builtin_isfinite(g->spacing[a]) && g->spacing[a] > 0)) return (why = "spacing must be finite and > 0", false);
        if (g->dims[a] < 1 || g->dims[a] > (1 << 24)) return (why = "dims must be >= 1 and their product <= 2^24", false);
        count *= g->dims[a];
        if (count > (1ll << 24)) return (why = "dims must be >= 1 and their product <= 2^24", false);
    }
    if (g->pad != 0) return (why = "pad must be 0", false);
    return true;
}

/* what both lookup entries check before any device work, in this order: context, grid, n / NULL; no scene is needed */
int lookup_check(rtr_context* c, const rtr_probe_grid* g, const void* probes, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    std::string why;
    if (!probe_grid_ok(g, why)) return fail(c, RTR_ERR_INVALID, "rtr_probe_lookup: " + why);
    return batch_check(c, "rtr_probe_lookup", n, probes && q && out);
}
int lookup_launch(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* d_probes, const rtr_gather_point* d_q,
                  rtr_gather_out* d_out, int64_t n) {
    for (int64_t k0 = 0; k0 < n; k0 += kLaunchPoints) {
        const long long m = std::min<long long>(n - k0, kLaunchPoints);
        hipLaunchKernelGGL(k_probe_lookup, dim3((unsigned)((m + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), 0, c->stream, *g,
                           d_probes, d_q + k0, d_out + k0, m);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("probe lookup launch: ") + hipGetErrorString(e));
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
    std::string why;
    double nlen;
    if (!probe_grid_ok(g, why) || !probes || !query || !out || gather_point_bad(*query, nlen)) return RTR_ERR_INVALID;
    *out = probe_lookup_one(*g, probes, *query, nlen);
    return RTR_OK;
}

int rtr_probe_lookup(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* probes, const rtr_gather_point* q,
                     rtr_gather_out* out, int64_t n) {
    if (int rc = lookup_check(c, g, probes, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    for (int64_t k = 0; k < n; ++k) {
        double nlen;
        if (gather_point_bad(q[k], nlen))
            return fail(c, RTR_ERR_INVALID, "rtr_probe_lookup: bad query at index " + std::to_string(k) +
                                                " (non-finite position / normal, or a normal whose length is not in (0, inf))");
    }
    /* the grid stays at the head of the staging buffer for all slices: the first one brings it */
    static_assert(sizeof(rtr_probe_sh) % 16 == 0, "StagedIO::head_bytes");
    const size_t grid_bytes = (size_t)g->dims[0] * g->dims[1] * g->dims[2] * sizeof(rtr_probe_sh);
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

int rtr_debug_last_probe(rtr_context* c, rtr_debug_probe* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_probe)) return RTR_ERR_INVALID;
    *out = c->last_probe;
    return RTR_OK;
}

} /* extern "C" */
