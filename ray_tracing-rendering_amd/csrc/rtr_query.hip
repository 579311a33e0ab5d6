/*
 * rtr_query.hip -- ray queries (include/rtr_hip.h: rtr_query_*): hittable::hit of the scene root for caller-given rays,
 * closest hit and occlusion, from host or device arrays: the ray check, the launch and the k_query_closest / k_query_any
 * instantiations it picks from.  The entries' common checks, the staging of the host entries and the body of the device
 * entries are rt_batch.h's.
 */
#include "rt_batch.h"

using namespace rtr;

namespace {

constexpr int64_t kQuerySlice = (int64_t)1 << 22; /* rays per slice of the host entries */

/* what every query entry checks before any device work, in this order: context, flags, n / NULL, scene */
int query_check(rtr_context* c, const void* rays, const void* out, int64_t n, int32_t flags) {
    if (!c) return RTR_ERR_INVALID;
    if (flags & ~RTR_FLAG_REFERENCE_ORDER) return fail(c, RTR_ERR_INVALID, "rtr_query_*: unknown flag bits");
    if (int rc = batch_check(c, "rtr_query_*", n, rays && out)) return rc;
    return scene_check(c, "rtr_query_*");
}
int query_check_rays(rtr_context* c, const rtr_ray* rays, int64_t n) {
    const bool media = c->info.has_media != 0;
    for (int64_t k = 0; k < n; ++k)
        if (rtr_ray_bad(rays[k], media))
            return fail(c, RTR_ERR_INVALID, "rtr_query_*: bad ray at index " + std::to_string(k) +
                                                " (non-finite origin / direction / time / t_min, NaN t_max, or rng_state 0 in a "
                                                "scene with media)");
    return RTR_OK;
}

/* the staged record access (k_query_*<.., STAGED>) unless RTR_QUERY_STAGED=0 or the stack leaves no room for it
 * (tools/time_queries.py measures both forms: DESIGN.md 4.6) */
bool query_staged(size_t stack) {
    const char* e = getenv("RTR_QUERY_STAGED");
    const bool want = e ? e[0] != '0' : RTR_QUERY_STAGED_DEFAULT != 0;
    return want && stack + RTR_QUERY_STAGE_BYTES <= 160 * 1024;
}

/* one launch over device arrays on the context stream; hits != nullptr: closest hit, else occlusion */
int query_launch(rtr_context* c, const rtr_ray* d_rays, rtr_ray_hit* d_hits, uint8_t* d_occ, uint32_t* d_rng, int64_t n, int flags) {
    const int trav = per_ray_trav(c->facts, c->info, flags, true); /* what a render with `flags` walks */
    const size_t stack = stack_bytes(c->facts, c->info, trav);
    const bool staged = query_staged(stack);
    const size_t lds = stack + (staged ? RTR_QUERY_STAGE_BYTES : 0);
    const int stage_word = (int)(stack / sizeof(int));
    const int media = c->info.has_media != 0;
    DScene ds = c->ds;
    ds.needs_uv = 1; /* (u, v) of the hit record whether or not a texture reads them */
    const dim3 grid((unsigned)((n + RTR_BLOCK - 1) / RTR_BLOCK));
    int rc = RTR_OK;
    auto launch = [&](auto t, auto s) {
        constexpr int T = decltype(t)::value;
        constexpr bool S = decltype(s)::value;
        if (d_hits) {
            if ((rc = set_lds(c, k_query_closest<T, S>, lds))) return;
            hipLaunchKernelGGL((k_query_closest<T, S>), grid, dim3(RTR_BLOCK), lds, c->stream, ds, d_rays, d_hits, (long long)n, media,
                               stage_word);
        } else {
            if ((rc = set_lds(c, k_query_any<T, S>, lds))) return;
            hipLaunchKernelGGL((k_query_any<T, S>), grid, dim3(RTR_BLOCK), lds, c->stream, ds, d_rays, d_occ, d_rng, (long long)n, media,
                               stage_word);
        }
    };
    if (!dispatch_trav(TravsTop{}, trav, [&](auto t) { staged ? launch(t, std::true_type{}) : launch(t, std::false_type{}); }))
        return no_per_ray_kernel(c, trav);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return RTR_OK;
}

/* the host entries: slices of at most kQuerySlice rays (staged_slices of rt_batch.h); closest hit has one output stream,
 * occlusion two, of which rng_out may be NULL */
int query_host(rtr_context* c, const rtr_ray* rays, rtr_ray_hit* hits, uint8_t* occ, uint32_t* rng_out, int64_t n, int flags) {
    const StagedIO io = hits ? StagedIO{0, sizeof(rtr_ray), rays, {sizeof(rtr_ray_hit), 0}, {hits, nullptr}}
                             : StagedIO{0, sizeof(rtr_ray), rays, {sizeof(uint8_t), sizeof(uint32_t)}, {occ, rng_out}};
    return staged_slices(c, n, kQuerySlice, io, [&](const Slice& s) {
        const rtr_ray* d_rays = static_cast<const rtr_ray*>(s.in);
        return hits ? query_launch(c, d_rays, static_cast<rtr_ray_hit*>(s.out[0]), nullptr, nullptr, s.m, flags)
                    : query_launch(c, d_rays, nullptr, static_cast<uint8_t*>(s.out[0]), static_cast<uint32_t*>(s.out[1]), s.m, flags);
    });
}

int query_device(rtr_context* c, const rtr_ray* d_rays, rtr_ray_hit* d_hits, uint8_t* d_occ, uint32_t* d_rng, int64_t n, int flags,
                 int blocking) {
    return device_entry(c, nullptr, 0, blocking, [&] { return query_launch(c, d_rays, d_hits, d_occ, d_rng, n, flags); });
}

} // namespace

extern "C" {

int rtr_query_closest(rtr_context* c, const rtr_ray* rays, rtr_ray_hit* hits, int64_t n, int32_t flags) {
    if (int rc = query_check(c, rays, hits, n, flags)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = query_check_rays(c, rays, n)) return rc;
    return query_host(c, rays, hits, nullptr, nullptr, n, flags);
}

int rtr_query_occluded(rtr_context* c, const rtr_ray* rays, uint8_t* occluded, uint32_t* rng_out, int64_t n, int32_t flags) {
    if (int rc = query_check(c, rays, occluded, n, flags)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = query_check_rays(c, rays, n)) return rc;
    return query_host(c, rays, nullptr, occluded, rng_out, n, flags);
}

int rtr_query_closest_device(rtr_context* c, const rtr_ray* d_rays, rtr_ray_hit* d_hits, int64_t n, int32_t flags, int blocking) {
    if (int rc = query_check(c, d_rays, d_hits, n, flags)) return rc;
    if (n == 0) return RTR_OK;
    return query_device(c, d_rays, d_hits, nullptr, nullptr, n, flags, blocking);
}

int rtr_query_occluded_device(rtr_context* c, const rtr_ray* d_rays, uint8_t* d_occluded, uint32_t* d_rng_out, int64_t n,
                              int32_t flags, int blocking) {
    if (int rc = query_check(c, d_rays, d_occluded, n, flags)) return rc;
    if (n == 0) return RTR_OK;
    return query_device(c, d_rays, nullptr, d_occluded, d_rng_out, n, flags, blocking);
}

} /* extern "C" */
