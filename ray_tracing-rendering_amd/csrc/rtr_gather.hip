/*
 * rtr_gather.hip -- hemisphere gathers (include/rtr_hip.h: rtr_gather_*): the k_gather_any / k_gather_li instantiations and
 * their launcher, and the host-only pieces that need no context (rtr_gather_defaults, rtr_gather_ray, the parameter
 * check).  A translation unit of its own so that the 27 kernels (10 k_gather_any, 17 k_gather_li) compile beside rtr_capi.hip, which holds the entries.
 */
#include "rt_kernels.h"
#include "rt_launch.h"

#include <type_traits>

namespace {

constexpr long long kLaunchPoints = 1ll << 24; /* points per launch: at most 2^22 workgroups */

template <typename Kern>
int launch_gather(Kern kernel, const GatherLaunch& L, std::string& err) {
    if (int rc = kernel_lds(kernel, L.lds, 0, err)) return rc;
    for (long long k0 = 0; k0 < L.K.n; k0 += kLaunchPoints) {
        GatherK K = L.K;
        K.pts += k0, K.out += k0, K.point_base += (uint32_t)k0;
        K.n = L.K.n - k0 < kLaunchPoints ? L.K.n - k0 : kLaunchPoints;
        const long long lanes = K.n << K.lg;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((lanes + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), L.lds, L.stream, L.ds, K);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return RTR_OK;
    err = std::string("gather launch: ") + hipGetErrorString(e);
    return RTR_ERR_DEVICE;
}

using TravsTop = TravSet<RT_TRAV_FAST, RT_TRAV_TOP, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>; /* the queries' */
using TravsLi = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>;              /* k_li's */
using TravsN1 = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA>;

template <int I, typename Travs>
bool launch_li(Travs travs, int trav, const GatherLaunch& L, std::string& err, int& rc) {
    return dispatch_trav(travs, trav, [&](auto t) { rc = launch_gather(k_gather_li<I, decltype(t)::value>, L, err); });
}

} // namespace

int rtr_gather_launch(const GatherLaunch& L, LaunchedGather* launched, std::string& err) {
    int rc = RTR_OK, trav = L.trav;
    bool found;
    if (L.integ < 0) {
        found = dispatch_trav(TravsTop{}, trav, [&](auto t) {
            constexpr int T = decltype(t)::value;
            rc = L.broadcast ? launch_gather(k_gather_any<T, true>, L, err) : launch_gather(k_gather_any<T, false>, L, err);
        });
    } else {
        /* integrators 0 / 2 / 3: the media kernel also serves the reference-order traversal (li_run) */
        const bool n1 = L.integ != RTR_INTEGRATOR_MIS && L.integ != RTR_INTEGRATOR_RR;
        if (n1 && trav == RT_TRAV_EXACT) trav = RT_TRAV_MEDIA;
        switch (L.integ) {
        case RTR_INTEGRATOR_MIS: found = launch_li<RTR_INTEGRATOR_MIS>(TravsLi{}, trav, L, err, rc); break;
        case RTR_INTEGRATOR_RR: found = launch_li<RTR_INTEGRATOR_RR>(TravsLi{}, trav, L, err, rc); break;
        case RTR_INTEGRATOR_PATH: found = launch_li<RTR_INTEGRATOR_PATH>(TravsN1{}, trav, L, err, rc); break;
        case RTR_INTEGRATOR_PBR: found = launch_li<RTR_INTEGRATOR_PBR>(TravsN1{}, trav, L, err, rc); break;
        default: found = launch_li<RTR_INTEGRATOR_NEE>(TravsN1{}, trav, L, err, rc); break;
        }
    }
    if (!found) {
        err = "no gather kernel for traversal " + std::to_string(trav);
        return RTR_ERR_UNSUPPORTED;
    }
    if (rc == RTR_OK && launched) *launched = LaunchedGather{L.integ < 0 ? -1 : L.integ, trav, L.integ < 0 && L.broadcast, L.K.lg};
    return rc;
}

int rtr_gather_params_check(const rtr_gather_params* p, std::string& err) {
    const char* why = nullptr;
    if (!p) why = "null gather params";
    else if (p->samples < 1 || p->samples > (1 << 20)) why = "samples outside 1 .. 2^20";
    else if (p->flags & ~RTR_FLAG_REFERENCE_ORDER) why = "unknown flag bits";
    else if (!__builtin_isfinite(p->time) || !__builtin_isfinite(p->t_min)) why = "time or t_min not finite";
    else if (p->t_max != p->t_max) why = "t_max is NaN";
    else if (p->reserved[0] != 0 || p->reserved[1] != 0) why = "reserved must be 0";
    if (!why) return RTR_OK;
    err = std::string("rtr_gather_*: ") + why;
    return RTR_ERR_INVALID;
}

extern "C" {

void rtr_gather_defaults(rtr_gather_params* p) {
    if (!p) return;
    *p = rtr_gather_params{};
    p->samples = 64;
    p->t_min = 0.001, p->t_max = __builtin_huge_val();
}

int rtr_gather_ray(const rtr_gather_params* params, const rtr_gather_point* point, int64_t index_in_call, int32_t s,
                   rtr_ray* out) {
    std::string err;
    if (rtr_gather_params_check(params, err) || !point || !out || index_in_call < 0 || s < 0 || s >= params->samples)
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
