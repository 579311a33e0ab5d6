/*
 * rtr_gather.hip -- hemisphere gathers (include/rtr_hip.h: rtr_gather_*): the entries, their checks, the launcher and the
 * 27 kernels it picks from (10 k_gather_any, 17 k_gather_li), and the host-only pieces that need no context
 * (rtr_gather_defaults, rtr_gather_ray).  Which k_gather_li a radiance gather runs is the k_li family rule of rt_select.h.
 */
#include "rt_context.h"

using namespace rtr;

namespace {

constexpr long long kLaunchPoints = 1ll << 24; /* points per launch: at most 2^22 workgroups */

template <typename Kern>
int launch_gather(rtr_context* c, Kern kernel, const DScene& ds, const GatherK& all, size_t lds) {
    if (int rc = set_lds(c, kernel, lds)) return rc;
    for (long long k0 = 0; k0 < all.n; k0 += kLaunchPoints) {
        GatherK K = all;
        K.pts += k0, K.out += k0, K.point_base += (uint32_t)k0;
        K.n = all.n - k0 < kLaunchPoints ? all.n - k0 : kLaunchPoints;
        const long long lanes = K.n << K.lg;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), lds, c->stream, ds, K);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("gather launch: ") + hipGetErrorString(e));
}

/* RTR_OK, or RTR_ERR_INVALID with the reason in `err` */
int gather_params_check(const rtr_gather_params* p, std::string& err) {
    const char* why = gather_params_why(p);
    if (!why) return RTR_OK;
    err = std::string("rtr_gather_*: ") + why;
    return RTR_ERR_INVALID;
}

constexpr int64_t kGatherSlice = (int64_t)1 << 20; /* points per slice of the host entries */

/* what every gather entry checks before any device work; `radiance`: rp is checked too (a NULL one is invalid) */
int gather_check(rtr_context* c, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp, const void* pts,
                 const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = gather_params_check(gp, c->err)) return rc;
    if (n < 0 || (n > 0 && (!pts || !out))) return fail(c, RTR_ERR_INVALID, "rtr_gather_*: negative n or NULL array");
    if (radiance)
        if (int rc = params_check(c, rp)) return rc;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_gather_* before rtr_upload_scene");
    return RTR_OK;
}
int gather_check_points(rtr_context* c, const rtr_gather_point* pts, int64_t n) {
    for (int64_t k = 0; k < n; ++k) {
        double nlen;
        if (gather_point_bad(pts[k], nlen))
            return fail(c, RTR_ERR_INVALID, "rtr_gather_*: bad point at index " + std::to_string(k) +
                                                " (non-finite position / normal, or a normal whose length is not in (0, inf))");
    }
    return RTR_OK;
}

/* every lane of a group loads its point (k_gather_any<T, false>) unless RTR_GATHER_BROADCAST=1 asks for one load per group
 * and a broadcast (tools/time_gather.py measures both forms: DESIGN.md 4.8) */
bool gather_broadcast() {
    const char* e = getenv("RTR_GATHER_BROADCAST");
    return e ? e[0] != '0' : RTR_GATHER_BROADCAST_DEFAULT != 0;
}

/* launches over device arrays on the context stream; rp: a radiance gather (k_gather_li), else occlusion (k_gather_any) */
int gather_launch(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, uint32_t point_base,
                  const rtr_gather_point* d_pts, rtr_gather_out* d_out, int64_t n) {
    const int integ = rp ? rp->integrator : -1;
    const int per_ray = per_ray_trav(c->facts, c->info, rp ? rp->flags : gp->flags, !rp);
    const int trav = rp ? li_trav(integ, per_ray) : per_ray;
    const size_t lds = stack_bytes(c->facts, c->info, per_ray);
    const bool broadcast = !rp && gather_broadcast();
    DScene ds = c->ds;
    if (!rp && !(gp->t_min >= 0x1p-100)) ds.shared_div = 0; /* the plain divisions, as k_query_* per wave */
    const GatherK K{d_pts, d_out, (long long)n, gp->samples, gather_lg(gp->samples), gp->seed, point_base, gp->time, gp->t_min,
                    gp->t_max, rp ? rp->max_depth : 0, rp ? rp->rr_start_depth : 0};
    int rc = RTR_OK;
    const bool found =
        rp ? dispatch_li(integ, trav, [&](auto i, auto t) { rc = launch_gather(c, k_gather_li<decltype(i)::value, decltype(t)::value>, ds, K, lds); })
           : dispatch_trav(TravsTop{}, trav, [&](auto t) {
                 constexpr int T = decltype(t)::value;
                 rc = broadcast ? launch_gather(c, k_gather_any<T, true>, ds, K, lds) : launch_gather(c, k_gather_any<T, false>, ds, K, lds);
             });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no gather kernel for traversal " + std::to_string(trav));
    if (rc == RTR_OK) c->last_gather = rtr_debug_gather{integ, trav, broadcast, K.lg};
    return rc;
}

int gather_host(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_gather_point* pts,
                rtr_gather_out* out, int64_t n) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    const int64_t slice = std::min(n, kGatherSlice);
    const size_t in_bytes = (size_t)slice * sizeof(rtr_gather_point);
    if (int rc = ensure(c, c->b_gather, in_bytes + (size_t)slice * sizeof(rtr_gather_out))) return rc;
    rtr_gather_point* d_pts = static_cast<rtr_gather_point*>(c->b_gather.p);
    rtr_gather_out* d_out = reinterpret_cast<rtr_gather_out*>(static_cast<char*>(c->b_gather.p) + in_bytes);
    for (int64_t k0 = 0; k0 < n; k0 += slice) {
        const int64_t m = std::min(slice, n - k0);
        HIPCHK(c, hipMemcpyAsync(d_pts, pts + k0, (size_t)m * sizeof(rtr_gather_point), hipMemcpyHostToDevice, c->stream));
        if (int rc = gather_launch(c, rp, gp, gp->point_base + (uint32_t)k0, d_pts, d_out, m)) return rc;
        HIPCHK(c, hipMemcpyAsync(out + k0, d_out, (size_t)m * sizeof(rtr_gather_out), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* the next slice reuses the buffer */
    }
    return RTR_OK;
}

int gather_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_gather_point* d_pts,
                  rtr_gather_out* d_out, int64_t n, int blocking) {
    if (((uintptr_t)d_pts | (uintptr_t)d_out) & 7) return fail(c, RTR_ERR_INVALID, "rtr_gather_*_device: pointers must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (int rc = gather_launch(c, rp, gp, gp->point_base, d_pts, d_out, n)) return rc;
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

} // namespace

extern "C" {

int rtr_gather_occlusion(rtr_context* c, const rtr_gather_params* gp, const rtr_gather_point* pts, rtr_gather_out* out, int64_t n) {
    if (int rc = gather_check(c, nullptr, false, gp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = gather_check_points(c, pts, n)) return rc;
    return gather_host(c, nullptr, gp, pts, out, n);
}

int rtr_gather_radiance(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_gather_point* pts,
                        rtr_gather_out* out, int64_t n) {
    if (int rc = gather_check(c, rp, true, gp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = gather_check_points(c, pts, n)) return rc;
    return gather_host(c, rp, gp, pts, out, n);
}

int rtr_gather_occlusion_device(rtr_context* c, const rtr_gather_params* gp, const rtr_gather_point* d_pts, rtr_gather_out* d_out,
                                int64_t n, int blocking) {
    if (int rc = gather_check(c, nullptr, false, gp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return gather_device(c, nullptr, gp, d_pts, d_out, n, blocking);
}

int rtr_gather_radiance_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp,
                               const rtr_gather_point* d_pts, rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = gather_check(c, rp, true, gp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return gather_device(c, rp, gp, d_pts, d_out, n, blocking);
}

void rtr_gather_defaults(rtr_gather_params* p) {
    if (!p) return;
    *p = rtr_gather_params{};
    p->samples = 64;
    p->t_min = 0.001, p->t_max = __builtin_huge_val();
}

int rtr_gather_ray(const rtr_gather_params* params, const rtr_gather_point* point, int64_t index_in_call, int32_t s,
                   rtr_ray* out) {
    std::string err;
    if (gather_params_check(params, err) || !point || !out || index_in_call < 0 || s < 0 || s >= params->samples)
        return RTR_ERR_INVALID;
    double nlen;
    if (gather_point_bad(*point, nlen)) return RTR_ERR_INVALID;
    const double r = 1 / nlen;
    uint32_t rng = rtr_sample_seed_inline(params->seed, 1, 0, (int32_t)((uint32_t)index_in_call + params->point_base), s);
    rtr_ray ray{};
    gather_direction(r * point->n[0], r * point->n[1], r * point->n[2], rng, ray.direction[0], ray.direction[1], ray.direction[2]);
    for (int a = 0; a < 3; ++a) ray.origin[a] = point->p[a];
    ray.time = params->time, ray.t_min = params->t_min, ray.t_max = params->t_max;
    ray.rng_state = rng;
    *out = ray;
    return RTR_OK;
}

} /* extern "C" */
