/*
 * rtr_probe.hip -- light probes (include/rtr_hip.h: rtr_probe_*, rtr_sh_*): the entries, their checks, the launcher and
 * the 22 kernels it picks from (5 k_probe_any, 17 k_probe_li), k_probe_lookup, and the host-only pieces that need no
 * context (rtr_probe_ray, rtr_sh_basis, rtr_sh_irradiance).  Which k_probe_li a radiance call runs is the k_li family
 * rule of rt_select.h, like the gathers'.
 */
#include "rt_context.h"

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

constexpr long long kLaunchPoints = 1ll << 24; /* points per launch: at most 2^22 workgroups */
constexpr int64_t kProbeSlice = (int64_t)1 << 20; /* points per slice of the host entries */

template <typename Kern>
int launch_probe(rtr_context* c, Kern kernel, const DScene& ds, const ProbeK& all, size_t rec, size_t lds) {
    if (int rc = set_lds(c, kernel, lds)) return rc;
    for (long long k0 = 0; k0 < all.n; k0 += kLaunchPoints) {
        ProbeK K = all;
        K.pts += k0, K.out = static_cast<char*>(all.out) + (size_t)k0 * rec, K.point_base += (uint32_t)k0;
        K.n = all.n - k0 < kLaunchPoints ? all.n - k0 : kLaunchPoints;
        const long long lanes = K.n << K.lg;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), lds, c->stream, ds, K);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("probe launch: ") + hipGetErrorString(e));
}

/* the gathers' parameter rules (rtr_gather_params is the block): RTR_OK, or RTR_ERR_INVALID with the reason in `err` */
int probe_params_check(const rtr_gather_params* p, std::string& err) {
    const char* why = gather_params_why(p);
    if (!why) return RTR_OK;
    err = std::string("rtr_probe_*: ") + why;
    return RTR_ERR_INVALID;
}

/* what every probe entry checks before any device work; `radiance`: rp is checked too (a NULL one is invalid) */
int probe_check(rtr_context* c, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp, const void* pts,
                const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = probe_params_check(gp, c->err)) return rc;
    if (n < 0 || (n > 0 && (!pts || !out))) return fail(c, RTR_ERR_INVALID, "rtr_probe_*: negative n or NULL array");
    if (radiance)
        if (int rc = params_check(c, rp)) return rc;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_probe_* before rtr_upload_scene");
    return RTR_OK;
}
int probe_check_points(rtr_context* c, const rtr_probe_point* pts, int64_t n) {
    for (int64_t k = 0; k < n; ++k)
        if (probe_point_bad(pts[k]))
            return fail(c, RTR_ERR_INVALID, "rtr_probe_*: bad point at index " + std::to_string(k) + " (non-finite position)");
    return RTR_OK;
}

size_t probe_record(bool radiance) { return radiance ? sizeof(rtr_probe_sh) : sizeof(rtr_probe_vis); }

/* launches over device arrays on the context stream; rp: radiance probes (k_probe_li), else visibility (k_probe_any) */
int probe_launch(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, uint32_t point_base,
                 const rtr_probe_point* d_pts, void* d_out, int64_t n) {
    const int integ = rp ? rp->integrator : -1;
    const int per_ray = per_ray_trav(c->facts, c->info, rp ? rp->flags : gp->flags, !rp);
    const int trav = rp ? li_trav(integ, per_ray) : per_ray;
    /* the traversal stack, and behind it the per-lane sums of k_probe_li (rt_kernels.h: ProbeSums) */
    const size_t stack = stack_bytes(c->facts, c->info, per_ray);
    const size_t lds = stack + (rp ? probe_sum_bytes() : 0);
    DScene ds = c->ds;
    if (!rp && !(gp->t_min >= 0x1p-100)) ds.shared_div = 0; /* the plain divisions, as the gathers */
    const ProbeK K{d_pts, d_out, (long long)n, gp->samples, gather_lg(gp->samples), gp->seed, point_base, gp->time, gp->t_min,
                   gp->t_max, rp ? rp->max_depth : 0, rp ? rp->rr_start_depth : 0, (int)(stack / sizeof(int))};
    int rc = RTR_OK;
    const bool found =
        rp ? dispatch_li(integ, trav, [&](auto i, auto t) {
                 rc = launch_probe(c, k_probe_li<decltype(i)::value, decltype(t)::value>, ds, K, sizeof(rtr_probe_sh), lds);
             })
           : dispatch_trav(TravsTop{}, trav, [&](auto t) {
                 rc = launch_probe(c, k_probe_any<decltype(t)::value>, ds, K, sizeof(rtr_probe_vis), lds);
             });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no probe kernel for traversal " + std::to_string(trav));
    if (rc == RTR_OK) c->last_probe = rtr_debug_probe{integ, trav, K.lg};
    return rc;
}

int probe_host(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_probe_point* pts, void* out,
               int64_t n) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    const size_t rec = probe_record(rp != nullptr);
    const int64_t slice = std::min(n, kProbeSlice);
    const size_t in_bytes = (size_t)slice * sizeof(rtr_probe_point);
    if (int rc = ensure(c, c->b_probe, in_bytes + (size_t)slice * rec)) return rc;
    rtr_probe_point* d_pts = static_cast<rtr_probe_point*>(c->b_probe.p);
    char* d_out = static_cast<char*>(c->b_probe.p) + in_bytes;
    for (int64_t k0 = 0; k0 < n; k0 += slice) {
        const int64_t m = std::min(slice, n - k0);
        HIPCHK(c, hipMemcpyAsync(d_pts, pts + k0, (size_t)m * sizeof(rtr_probe_point), hipMemcpyHostToDevice, c->stream));
        if (int rc = probe_launch(c, rp, gp, gp->point_base + (uint32_t)k0, d_pts, d_out, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(static_cast<char*>(out) + (size_t)k0 * rec, d_out, (size_t)m * rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* the next slice reuses the buffer */
    }
    return RTR_OK;
}

int probe_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_probe_point* d_pts, void* d_out,
                 int64_t n, int blocking) {
    if (((uintptr_t)d_pts | (uintptr_t)d_out) & 7) return fail(c, RTR_ERR_INVALID, "rtr_probe_*_device: pointers must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (int rc = probe_launch(c, rp, gp, gp->point_base, d_pts, d_out, n)) return rc;
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
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

/* what both lookup entries check before any device work */
int lookup_check(rtr_context* c, const rtr_probe_grid* g, const void* probes, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    std::string why;
    if (!probe_grid_ok(g, why)) return fail(c, RTR_ERR_INVALID, "rtr_probe_lookup: " + why);
    if (n < 0 || (n > 0 && (!probes || !q || !out))) return fail(c, RTR_ERR_INVALID, "rtr_probe_lookup: negative n or NULL array");
    return RTR_OK;
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
    std::string err;
    if (probe_params_check(params, err) || !point || !out || index_in_call < 0 || s < 0 || s >= params->samples)
        return RTR_ERR_INVALID;
    if (probe_point_bad(*point)) return RTR_ERR_INVALID;
    uint32_t rng = rtr_sample_seed_inline(params->seed, 1, 0, (int32_t)((uint32_t)index_in_call + params->point_base), s);
    rtr_ray ray{};
    probe_direction(rng, ray.direction[0], ray.direction[1], ray.direction[2]);
    for (int a = 0; a < 3; ++a) ray.origin[a] = point->p[a];
    ray.time = params->time, ray.t_min = params->t_min, ray.t_max = params->t_max;
    ray.rng_state = rng;
    *out = ray;
    return RTR_OK;
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
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    const size_t grid_bytes = (size_t)g->dims[0] * g->dims[1] * g->dims[2] * sizeof(rtr_probe_sh);
    const int64_t slice = std::min(n, kProbeSlice);
    const size_t in_bytes = (size_t)slice * sizeof(rtr_gather_point);
    if (int rc = ensure(c, c->b_probe, grid_bytes + in_bytes + (size_t)slice * sizeof(rtr_gather_out))) return rc;
    char* base = static_cast<char*>(c->b_probe.p);
    rtr_probe_sh* d_probes = reinterpret_cast<rtr_probe_sh*>(base);
    rtr_gather_point* d_q = reinterpret_cast<rtr_gather_point*>(base + grid_bytes);
    rtr_gather_out* d_out = reinterpret_cast<rtr_gather_out*>(base + grid_bytes + in_bytes);
    HIPCHK(c, hipMemcpyAsync(d_probes, probes, grid_bytes, hipMemcpyHostToDevice, c->stream));
    for (int64_t k0 = 0; k0 < n; k0 += slice) {
        const int64_t m = std::min(slice, n - k0);
        HIPCHK(c, hipMemcpyAsync(d_q, q + k0, (size_t)m * sizeof(rtr_gather_point), hipMemcpyHostToDevice, c->stream));
        if (int rc = lookup_launch(c, g, d_probes, d_q, d_out, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(out + k0, d_out, (size_t)m * sizeof(rtr_gather_out), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return RTR_OK;
}

int rtr_probe_lookup_device(rtr_context* c, const rtr_probe_grid* g, const rtr_probe_sh* d_probes, const rtr_gather_point* d_q,
                            rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = lookup_check(c, g, d_probes, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (((uintptr_t)d_probes | (uintptr_t)d_q | (uintptr_t)d_out) & 7)
        return fail(c, RTR_ERR_INVALID, "rtr_probe_lookup_device: pointers must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (int rc = lookup_launch(c, g, d_probes, d_q, d_out, n)) return rc;
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

int rtr_debug_last_probe(rtr_context* c, rtr_debug_probe* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_probe)) return RTR_ERR_INVALID;
    *out = c->last_probe;
    return RTR_OK;
}

} /* extern "C" */
