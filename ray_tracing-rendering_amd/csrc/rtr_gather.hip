/*
 * rtr_gather.hip -- hemisphere gathers (include/rtr_hip.h: rtr_gather_*): the point check, the kernel choice among the
 * 27 kernels held here (10 k_gather_any, 17 k_gather_li), the entries, and the host-only pieces that need no context
 * (rtr_gather_defaults, rtr_gather_ray).  Which k_gather_li a radiance gather runs is the k_li family rule of rt_select.h.
 * The entries' common checks, the staging of the host entries, the body of the device entries, the launch set-up, the
 * chunked launcher and the single-ray entry are rt_batch.h's, shared with the other batch units.
 */
#include "rt_batch.h"

using namespace rtr;

namespace {

constexpr int64_t kGatherSlice = (int64_t)1 << 20; /* points per slice of the host entries */

/* what every gather entry checks before any device work; `radiance`: rp is checked too (a NULL one is invalid) */
int gather_check(rtr_context* c, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp, const void* pts,
                 const void* out, int64_t n) {
    return points_check(c, "rtr_gather_*", rp, radiance, gp, n, pts && out);
}
int gather_check_points(rtr_context* c, const rtr_gather_point* pts, int64_t n) {
    return records_check(c, "rtr_gather_*", "point", kGatherPointRule, n, [&](int64_t k) {
        double nlen;
        return gather_point_bad(pts[k], nlen);
    });
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
    PointLaunch<GatherK> L = point_launch<GatherK>(c, rp, gp);
    L.k.pts = d_pts, L.k.out = d_out, L.k.n = (long long)n, L.k.point_base = point_base;
    const bool broadcast = !rp && gather_broadcast();
    int rc = RTR_OK;
    const auto launch = [&](auto kernel) {
        rc = launch_records(c, "rtr_gather_*", kernel, L.stack, L.k.n, L.k.lg, point_args(L.ds, L.k, sizeof(rtr_gather_out)));
    };
    const bool found = rp ? dispatch_li(L.integ, L.trav, [&](auto i, auto t) { launch(k_gather_li<decltype(i)::value, decltype(t)::value>); })
                          : dispatch_trav(TravsTop{}, L.trav, [&](auto t) {
                                constexpr int T = decltype(t)::value;
                                broadcast ? launch(k_gather_any<T, true>) : launch(k_gather_any<T, false>);
                            });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no gather kernel for traversal " + std::to_string(L.trav));
    if (rc == RTR_OK) c->last_batch[RTR_DEBUG_GATHER] = rtr_debug_batch{L.integ, L.trav, broadcast, L.k.lg};
    return rc;
}

/* slices of at most kGatherSlice points (staged_slices of rt_batch.h), each at its point_base */
int gather_host(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_gather_point* pts,
                rtr_gather_out* out, int64_t n) {
    const StagedIO io{0, sizeof(rtr_gather_point), pts, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kGatherSlice, io, [&](const Slice& s) {
        return gather_launch(c, rp, gp, gp->point_base + (uint32_t)s.k0, static_cast<const rtr_gather_point*>(s.in),
                             static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int gather_device(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, const rtr_gather_point* d_pts,
                  rtr_gather_out* d_out, int64_t n, int blocking) {
    return device_entry(c, "rtr_gather_*_device", (uintptr_t)d_pts | (uintptr_t)d_out, blocking,
                        [&] { return gather_launch(c, rp, gp, gp->point_base, d_pts, d_out, n); });
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
    return sample_ray(params, point ? point->p : nullptr, index_in_call, s, out, [&](uint32_t& rng, double* d) {
        double nlen;
        if (gather_point_bad(*point, nlen)) return false;
        const double r = 1 / nlen;
        gather_direction(r * point->n[0], r * point->n[1], r * point->n[2], rng, d[0], d[1], d[2]);
        return true;
    });
}

} /* extern "C" */
