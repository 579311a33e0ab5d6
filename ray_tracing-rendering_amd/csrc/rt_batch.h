/*
 * rt_batch.h -- host only: what the units that answer a batch of caller records share.  Those are rtr_query.hip,
 * rtr_gather.hip, rtr_probe.hip, rtr_probe_depth.hip, rtr_capture.hip, rtr_cube.hip, rtr_ibl.hip and rtr_preview.hip.
 * Here are
 *   - the entry checks they have in common, the first-bad-record loop among them;
 *   - the one path of a host entry from the caller's array to the kernel and back (staged_slices), and its form for
 *     records that are texels of centres which stay on the device (staged_texels);
 *   - the body of a device-pointer entry (device_entry);
 *   - the one chunked launcher (launch_records) with the argument steps of the point and texel kernels, and the cap
 *     that an environment variable lowers (env_cap);
 *   - the launch set-up of the gathers and probes, and the single-ray entry of every sampled family (sample_ray).
 * No device code; the kernels and which one a call runs stay with the units.
 */
#pragma once

#include "rt_context.h"

#include <cstdlib>
#include <tuple>

namespace rtr {

/* ---- entry checks: `who` is the subject's prefix in the message ("rtr_gather_*", "rtr_probe_lookup", ...) ---- */

/* the gathers' parameter rules (the probes share the block): RTR_OK, or RTR_ERR_INVALID with the reason in `err` */
inline int gather_params_check(const char* who, const rtr_gather_params* p, std::string& err) {
    const char* why = gather_params_why(p);
    if (!why) return RTR_OK;
    err = std::string(who) + ": " + why;
    return RTR_ERR_INVALID;
}
/* `arrays`: every array the entry needs when n > 0 is there */
inline int batch_check(rtr_context* c, const char* who, int64_t n, bool arrays) {
    if (n < 0 || (n > 0 && !arrays)) return fail(c, RTR_ERR_INVALID, std::string(who) + ": negative n or NULL array");
    return RTR_OK;
}
inline int scene_check(rtr_context* c, const char* who) {
    return c->has_scene ? RTR_OK : fail(c, RTR_ERR_NO_SCENE, std::string(who) + " before rtr_upload_scene");
}
/* what every gather and probe entry checks before any device work, in this order: context, gather params, n / NULL,
 * render params (`radiance`: a NULL rp is invalid), scene */
inline int points_check(rtr_context* c, const char* who, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp,
                        int64_t n, bool arrays) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = gather_params_check(who, gp, c->err)) return rc;
    if (int rc = batch_check(c, who, n, arrays)) return rc;
    if (radiance)
        if (int rc = params_check(c, rp)) return rc;
    return scene_check(c, who);
}

/* the first record k of n that is `bad(k)` fails the call: "<who>: bad <noun> at index k (<rule>)" */
constexpr const char* kGatherPointRule = "non-finite position / normal, or a normal whose length is not in (0, inf)";
constexpr const char* kPositionRule = "non-finite position";
template <typename Bad>
int records_check(rtr_context* c, const char* who, const char* noun, const char* rule, int64_t n, Bad bad) {
    for (int64_t k = 0; k < n; ++k)
        if (bad(k))
            return fail(c, RTR_ERR_INVALID, std::string(who) + ": bad " + noun + " at index " + std::to_string(k) + " (" + rule + ")");
    return RTR_OK;
}

/* ---- host entries ----
 * What a host entry does between the caller's arrays and the kernel: slices of at most `slice_len` records through
 * c->b_batch, everything stream-ordered on the context stream (behind a render that is still running; its workspace,
 * statistics and events are not touched).  Per slice: input to the device, `launch`, outputs back, and a wait, since the
 * next slice reuses the buffer; so the call returns with nothing of its own queued.  All record checks are the caller's
 * and come before this: a failing entry leaves the outputs untouched. */
struct StagedIO {
    size_t head_bytes;  /* kept at the head of the buffer for the caller (the grid of rtr_probe_lookup, the centres of
                           rtr_capture_cube), a multiple of 16 */
    size_t in_rec;      /* bytes per input record; 0: the slices have no input of their own (rtr_capture_cube: a record is
                           a texel, and its input is the centre at the head) */
    const void* in;
    size_t out_rec[2];  /* bytes per record of each output stream; 0: no such stream */
    void* out[2];       /* nullptr: the stream is staged for the kernel but not copied back (rng_out of rtr_query_occluded) */
};
struct Slice { /* device pointers of one slice: records k0 .. k0 + m of the call */
    void* head;
    void* in;
    void* out[2];
    int64_t k0, m;
};
template <typename Launch>
int staged_slices(rtr_context* c, int64_t n, int64_t slice_len, const StagedIO& io, Launch launch) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    const int64_t slice = std::min(n, slice_len);
    const auto room = [&](size_t rec) { return ((size_t)slice * rec + 15) & ~(size_t)15; };
    if (int rc = ensure(c, c->b_batch, io.head_bytes + room(io.in_rec) + room(io.out_rec[0]) + room(io.out_rec[1]))) return rc;
    char* base = static_cast<char*>(c->b_batch.p);
    Slice s{base, base + io.head_bytes, {nullptr, nullptr}, 0, 0};
    char* next = base + io.head_bytes + room(io.in_rec);
    for (int o = 0; o < 2; ++o)
        if (io.out_rec[o]) s.out[o] = next, next += room(io.out_rec[o]);
    for (s.k0 = 0; s.k0 < n; s.k0 += slice) {
        s.m = std::min(slice, n - s.k0);
        if (io.in_rec)
            HIPCHK(c, hipMemcpyAsync(s.in, static_cast<const char*>(io.in) + (size_t)s.k0 * io.in_rec, (size_t)s.m * io.in_rec,
                                     hipMemcpyHostToDevice, c->stream));
        if (int rc = launch(s)) return rc;
        for (int o = 0; o < 2; ++o)
            if (io.out_rec[o] && io.out[o])
                HIPCHK(c, hipMemcpyAsync(static_cast<char*>(io.out[o]) + (size_t)s.k0 * io.out_rec[o], s.out[o],
                                         (size_t)s.m * io.out_rec[o], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* the next slice reuses the buffer */
    }
    return RTR_OK;
}

/* rtr_capture_cube / rtr_probe_depth: a record is a texel, `per` of them to each of the n centres, and has no input of its
 * own.  The centres stay at the head of the staging buffer for all slices: the first one brings them.
 * launch(d_centres, d_out, first, m): the texels first .. first + m of the call into the records [0, m) of d_out */
template <typename Launch>
int staged_texels(rtr_context* c, const rtr_probe_point* pts, int64_t n, long long per, size_t out_rec, void* out,
                  int64_t slice_len, Launch launch) {
    const size_t bytes = (size_t)n * sizeof(rtr_probe_point);
    const StagedIO io{(bytes + 15) & ~(size_t)15, 0, nullptr, {out_rec, 0}, {out, nullptr}};
    return staged_slices(c, n * per, slice_len, io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, pts, bytes, hipMemcpyHostToDevice, c->stream));
        return launch(static_cast<const rtr_probe_point*>(s.head), s.out[0], s.k0, s.m);
    });
}

/* ---- device-pointer entries: `launch` on the context stream behind what is queued there.  `who` != nullptr: the entry
 * wants the pointers or-ed into `ptr_bits` 8-byte aligned ---- */
template <typename Launch>
int device_entry(rtr_context* c, const char* who, uintptr_t ptr_bits, int blocking, Launch launch) {
    if (who && (ptr_bits & 7)) return fail(c, RTR_ERR_INVALID, std::string(who) + ": pointers must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    if (int rc = launch()) return rc;
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

/* ---- launches over device arrays of records ---- */

/* a cap that an environment variable lowers (the test hooks RTR_LAUNCH_RECORDS, RTR_FILTER_PAIRS, RTR_TABLE_NODES, read at
 * every call): a value v is taken when 1 <= v < cap and ignored otherwise */
inline long long env_cap(const char* name, long long cap) {
    if (const char* e = getenv(name)) {
        const long long v = std::atoll(e);
        if (v >= 1 && v < cap) cap = v;
    }
    return cap;
}

constexpr long long kLaunchRecords = 1ll << 24; /* records per launch: at most 2^22 workgroups */

/* `kernel` over n records, 1 << lg lanes to each, in launches of at most kLaunchRecords (RTR_LAUNCH_RECORDS=v lowers that:
 * the bits do not depend on it).  args(k0, m): the kernel's arguments, a tuple, for the launch that serves the records
 * k0 .. k0 + m of the call.  `lds`: the kernel's dynamic LDS.  `who` names the entry in a launch failure.  The context keeps
 * the number of launches of its last call here (rtr_debug_last_launches: what shows a test that a cap took effect) */
template <typename Kern, typename Args>
int launch_records(rtr_context* c, const char* who, Kern kernel, size_t lds, long long n, int lg, Args args) {
    if (int rc = set_lds(c, kernel, lds)) return rc;
    const long long cap = env_cap("RTR_LAUNCH_RECORDS", kLaunchRecords);
    c->last_launches = (n + cap - 1) / cap;
    for (long long k0 = 0; k0 < n; k0 += cap) {
        const long long m = std::min(n - k0, cap);
        const dim3 grid((unsigned)(((m << lg) + RTR_BLOCK - 1) / RTR_BLOCK));
        std::apply([&](const auto&... a) { hipLaunchKernelGGL(kernel, grid, dim3(RTR_BLOCK), lds, c->stream, a...); }, args(k0, m));
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string(who) + " launch: " + hipGetErrorString(e));
}
/* the step of the gathers and probes (GatherK, ProbeK): the points, their numbers under the seed and the records of
 * all.out, `out_rec` bytes each, move on by k0.  The step refers to `ds` and `all`, which outlive the launch_records call */
template <typename K>
auto point_args(const DScene& ds, const K& all, size_t out_rec) {
    return [&ds, &all, out_rec](long long k0, long long m) {
        K k = all;
        k.pts += k0, k.point_base += (uint32_t)k0, k.n = m;
        k.out = (decltype(k.out))((char*)all.out + (size_t)k0 * out_rec);
        return std::tuple<const DScene&, K>(ds, k);
    };
}
/* the step of the captures and the probe distance maps (CaptureK, DepthK), whose records are texels: a launch serves the
 * records [k0, k0 + m) of all.out; the centre array and the texel numbering (all.first) stay where they are.  `ds` and
 * `all` outlive the call, as for point_args */
template <typename K>
auto texel_args(const DScene& ds, const K& all) {
    return [&ds, &all](long long k0, long long m) {
        K k = all;
        k.k0 = k0, k.n = k0 + m;
        return std::tuple<const DScene&, K>(ds, k);
    };
}

/* what gather_launch and probe_launch work out alike; K is GatherK or ProbeK with the members both have filled in but
 * pts, out, n and point_base, which the caller sets (and ProbeK's sum_word) */
template <typename K>
struct PointLaunch {
    int integ;    /* rp's, or -1: an any-hit call */
    int trav;     /* of the kernel: li_trav of the integrator for a radiance call */
    size_t stack; /* bytes of the traversal stack in the dynamic LDS */
    DScene ds;
    K k;
};
template <typename K>
PointLaunch<K> point_launch(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp) {
    const int integ = rp ? rp->integrator : -1;
    const int per_ray = per_ray_trav(c->facts, c->info, rp ? rp->flags : gp->flags, !rp);
    PointLaunch<K> L{integ, rp ? li_trav(integ, per_ray) : per_ray, stack_bytes(c->facts, c->info, per_ray), c->ds, K{}};
    if (!rp && !(gp->t_min >= 0x1p-100)) L.ds.shared_div = 0; /* the plain divisions, as k_query_* per wave */
    L.k.samples = gp->samples, L.k.lg = gather_lg(gp->samples), L.k.seed = gp->seed;
    L.k.time = gp->time, L.k.t_min = gp->t_min, L.k.t_max = gp->t_max;
    L.k.max_depth = rp ? rp->max_depth : 0, L.k.rr_start = rp ? rp->rr_start_depth : 0;
    return L;
}

/* ---- the single-ray entries (rtr_gather_ray, rtr_probe_ray, rtr_capture_ray, rtr_probe_depth_ray): sample `s` of record
 * `index_in_call` of a call, from `origin`.  The family's parameter block is valid: the caller has checked it ---- */
struct RaySeed { /* what of a parameter block the ray depends on */
    uint32_t seed, point_base;
    int32_t count, element; /* the (count, element) pair of the sample's seed: (1, 0), or the texels of a centre and this one */
    int32_t samples;
    double time, t_min, t_max;
};
/* direction(rng, d) draws the direction from the sample's generator, which it leaves behind the draws; false: a bad point */
template <typename Direction>
int sample_ray(const RaySeed& r, const double* origin, int64_t index_in_call, int32_t s, rtr_ray* out, Direction direction) {
    if (!origin || !out || index_in_call < 0 || s < 0 || s >= r.samples) return RTR_ERR_INVALID;
    uint32_t rng = rtr_sample_seed_inline(r.seed, r.count, r.element, (int32_t)((uint32_t)index_in_call + r.point_base), s);
    rtr_ray ray{};
    if (!direction(rng, ray.direction)) return RTR_ERR_INVALID;
    for (int a = 0; a < 3; ++a) ray.origin[a] = origin[a];
    ray.time = r.time, ray.t_min = r.t_min, ray.t_max = r.t_max;
    ray.rng_state = rng;
    *out = ray;
    return RTR_OK;
}
/* the gathers' and probes' form: `params` is the caller's block, checked here */
template <typename Direction>
int sample_ray(const rtr_gather_params* params, const double* origin, int64_t index_in_call, int32_t s, rtr_ray* out,
               Direction direction) {
    if (gather_params_why(params)) return RTR_ERR_INVALID;
    return sample_ray(RaySeed{params->seed, params->point_base, 1, 0, params->samples, params->time, params->t_min, params->t_max},
                      origin, index_in_call, s, out, direction);
}

} // namespace rtr
