/*
 * rtr_preview.hip -- baked previews (include/rtr_hip.h: rtr_preview_*): a frame shaded from a probe grid, a cube chain and
 * a BRDF table in one launch.  The parameter and region checks, the k_preview instantiations of rt_preview.h and the launch
 * that picks among them (the traversal rule of rt_select.h, as for k_query_closest), the entries, and the host-only
 * rtr_preview_ray; rtr_preview_set* are the frame entries with a capture set (k_preview_set).  The environment's rules, its staging and its overlap test are rt_ibl.h's, the staging of the host
 * entries and the body of the device entries rt_batch.h's.
 */
#include "rt_batch.h"
#include "rt_preview.h"

using namespace rtr;

namespace {

constexpr size_t kSampleSliceBytes = (size_t)1 << 28; /* records per slice of rtr_preview_samples, in bytes: whole rows */

struct Region {
    int w, h;
    long long pixels;
};
Region region_of(const rtr_preview_params* p) {
    return Region{p->x1 - p->x0, p->y1 - p->y0, (long long)(p->x1 - p->x0) * (p->y1 - p->y0)};
}

/* what every entry checks before any device work, in this order: context, params, NULL, scene, media */
int preview_check(rtr_context* c, const char* who, const rtr_preview_params* p, bool arrays) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = preview_params_why(p)) return fail(c, RTR_ERR_INVALID, std::string(who) + ": " + why);
    if (!arrays) return fail(c, RTR_ERR_INVALID, std::string(who) + ": NULL array");
    if (int rc = scene_check(c, who)) return rc;
    if (c->info.has_media)
        return fail(c, RTR_ERR_UNSUPPORTED, std::string(who) + ": the scene has media, whose free paths need the path's generator: "
                                                               "a preview has none");
    return RTR_OK;
}
/* the frame entries' own part behind preview_check: the environment (with_set: and the capture set its SPECULAR part reads)
 * and the row stride */
int frame_check(rtr_context* c, const char* who, const rtr_preview_params* p, const rtr_shade_env* env, bool with_set,
                const rtr_capture_set* set, int64_t row_stride) {
    if (const char* why = with_set ? env_set_why(env, set) : env_why(env)) return fail(c, RTR_ERR_INVALID, std::string(who) + ": " + why);
    if (row_stride < p->x1 - p->x0) return fail(c, RTR_ERR_INVALID, std::string(who) + ": row_stride below the region's width");
    return RTR_OK;
}

static_assert(sizeof(DScene) + sizeof(PreviewK) + sizeof(ShadeK) + sizeof(SetK) <= 4096, "the arguments of k_preview_set fit a launch");

/* one launch over device arrays on the context stream: the rows [y0, y1) of the region.  E == nullptr: the samples form;
 * S != nullptr: the frame form that reads a capture set */
int preview_launch(rtr_context* c, const rtr_preview_params* p, int y0, int y1, const ShadeK* E, rtr_preview_sample* d_samples,
                   double* d_linear, int32_t* d_lit, int64_t row_stride, const SetK* S = nullptr) {
    const int trav = per_ray_trav(c->facts, c->info, p->flags, true); /* what a render with `flags` walks */
    const size_t lds = stack_bytes(c->facts, c->info, trav);
    PreviewK P{};
    P.W = p->image_width, P.H = p->image_height;
    P.x0 = p->x0, P.y0 = y0, P.x1 = p->x1, P.y1 = y1;
    P.k = p->grid, P.t_min = p->t_min;
    P.samples = d_samples, P.linear = d_linear, P.lit = d_lit, P.row_stride = row_stride;
    const dim3 grid((unsigned)((P.x1 - P.x0 + 15) / 16), (unsigned)((P.y1 - P.y0 + 15) / 16));
    if (grid.y > 65535u || grid.x > 65535u * 32768u) return fail(c, RTR_ERR_UNSUPPORTED, "rtr_preview: more 16 x 16 blocks than a launch holds");
    const ShadeK none{};
    int rc = RTR_OK;
    auto launch = [&](auto t, auto s) {
        constexpr int T = decltype(t)::value;
        constexpr bool S = decltype(s)::value;
        if ((rc = set_lds(c, k_preview<T, S>, lds))) return;
        hipLaunchKernelGGL((k_preview<T, S>), grid, dim3(RTR_BLOCK), lds, c->stream, c->ds, P, E ? *E : none);
    };
    auto launch_set = [&](auto t) {
        constexpr int T = decltype(t)::value;
        if ((rc = set_lds(c, k_preview_set<T>, lds))) return;
        hipLaunchKernelGGL((k_preview_set<T>), grid, dim3(RTR_BLOCK), lds, c->stream, c->ds, P, *E, *S);
    };
    if (!dispatch_trav(TravsTop{}, trav, [&](auto t) { S ? launch_set(t) : E ? launch(t, std::false_type{}) : launch(t, std::true_type{}); }))
        return no_per_ray_kernel(c, trav);
    if (rc) return rc;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("preview launch: ") + hipGetErrorString(e));
}

/* rtr_preview and rtr_preview_set: with_set selects the set's rules, its chain bytes and its kernel */
int preview_host(rtr_context* c, const char* who, const rtr_preview_params* p, const rtr_shade_env* env, bool with_set,
                 const rtr_capture_set* set, double* h_linear, int64_t row_stride, int32_t* h_lit) {
    if (int rc = preview_check(c, who, p, h_linear != nullptr)) return rc;
    if (int rc = frame_check(c, who, p, env, with_set, set, row_stride)) return rc;
    /* the environment's arrays, then the frame and the counts, rows packed: one buffer, the gathers' */
    const Region R = region_of(p);
    const EnvBytes b = env_bytes(env, with_set ? env_cubes(env, set) : 1);
    const size_t frame_bytes = ((size_t)R.pixels * 3 * sizeof(double) + 15) & ~(size_t)15;
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    if (int rc = ensure(c, c->b_batch, b.total() + frame_bytes + (size_t)R.pixels * sizeof(int32_t))) return rc;
    char* base = static_cast<char*>(c->b_batch.p);
    double* d_linear = reinterpret_cast<double*>(base + b.total());
    int32_t* d_lit = reinterpret_cast<int32_t*>(base + b.total() + frame_bytes);
    ShadeK E;
    HIPCHK(c, env_stage(env, b, base, true, c->stream, E));
    SetK S;
    if (with_set) S = env_set_k(env, set);
    if (int rc = preview_launch(c, p, p->y0, p->y1, &E, nullptr, d_linear, h_lit ? d_lit : nullptr, R.w, with_set ? &S : nullptr)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(h_linear, (size_t)row_stride * 3 * sizeof(double), d_linear, (size_t)R.w * 3 * sizeof(double),
                               (size_t)R.w * 3 * sizeof(double), R.h, hipMemcpyDeviceToHost, c->stream));
    if (h_lit)
        HIPCHK(c, hipMemcpy2DAsync(h_lit, (size_t)row_stride * sizeof(int32_t), d_lit, (size_t)R.w * sizeof(int32_t),
                                   (size_t)R.w * sizeof(int32_t), R.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

/* rtr_preview_device and rtr_preview_set_device */
int preview_device(rtr_context* c, const char* who, const rtr_preview_params* p, const rtr_shade_env* env, bool with_set,
                   const rtr_capture_set* set, double* d_linear, int64_t row_stride, int32_t* d_lit, int blocking) {
    if (int rc = preview_check(c, who, p, d_linear != nullptr)) return rc;
    if (int rc = frame_check(c, who, p, env, with_set, set, row_stride)) return rc;
    const Region R = region_of(p);
    const EnvBytes b = env_bytes(env, with_set ? env_cubes(env, set) : 1);
    const size_t span = (size_t)(R.h - 1) * (size_t)row_stride + R.w; /* pixels from the first to behind the last one written */
    uintptr_t bits = (uintptr_t)d_linear | ((uintptr_t)d_lit << 1); /* the counts are 4-byte records */
    if (env_overlaps(env, b, (uintptr_t)d_linear, span * 3 * sizeof(double), bits) ||
        (d_lit && env_overlaps(env, b, (uintptr_t)d_lit, span * sizeof(int32_t), bits)))
        return fail(c, RTR_ERR_INVALID, std::string(who) + ": an output overlaps an array of the environment");
    if (d_lit && spans_overlap((uintptr_t)d_linear, span * 3 * sizeof(double), (uintptr_t)d_lit, span * sizeof(int32_t)))
        return fail(c, RTR_ERR_INVALID, std::string(who) + ": linear overlaps lit");
    const ShadeK E = shade_k(env, env->probes, env->depth, env->chain, env->table);
    SetK S;
    if (with_set) S = env_set_k(env, set);
    return device_entry(c, who, bits, blocking,
                        [&] { return preview_launch(c, p, p->y0, p->y1, &E, nullptr, d_linear, d_lit, row_stride, with_set ? &S : nullptr); });
}

} // namespace

extern "C" {

void rtr_preview_defaults(rtr_preview_params* p) {
    if (!p) return;
    *p = rtr_preview_params{};
    p->grid = 1;
    p->t_min = 0.001;
}

int rtr_preview_ray(const rtr_camera* cam, const rtr_preview_params* p, int32_t i, int32_t j, int32_t s, rtr_ray* out) {
    if (!cam || !out || preview_params_why(p)) return RTR_ERR_INVALID;
    if (i < 0 || i >= p->image_width || j < 0 || j >= p->image_height || s < 0 || s >= p->grid * p->grid) return RTR_ERR_INVALID;
    rtr_ray r{};
    preview_ray(*cam, p->image_width, p->image_height, p->grid, i, j, s, r.origin, r.direction);
    r.time = cam->time0, r.t_min = p->t_min, r.t_max = __builtin_huge_val();
    r.rng_state = 1;
    *out = r;
    return RTR_OK;
}

int rtr_preview_samples(rtr_context* c, const rtr_preview_params* p, rtr_preview_sample* out) {
    if (int rc = preview_check(c, "rtr_preview_samples", p, out != nullptr)) return rc;
    /* a record of the staging is one row of the region: whole rows per slice */
    const Region R = region_of(p);
    const size_t row_bytes = (size_t)R.w * p->grid * p->grid * sizeof(rtr_preview_sample);
    const int64_t rows = (int64_t)std::max<size_t>(1, kSampleSliceBytes / row_bytes);
    const StagedIO io{0, 0, nullptr, {row_bytes, 0}, {out, nullptr}};
    return staged_slices(c, R.h, rows, io, [&](const Slice& s) {
        return preview_launch(c, p, p->y0 + (int)s.k0, p->y0 + (int)(s.k0 + s.m), nullptr, static_cast<rtr_preview_sample*>(s.out[0]),
                              nullptr, nullptr, 0);
    });
}

int rtr_preview_samples_device(rtr_context* c, const rtr_preview_params* p, rtr_preview_sample* d_out, int blocking) {
    if (int rc = preview_check(c, "rtr_preview_samples_device", p, d_out != nullptr)) return rc;
    return device_entry(c, "rtr_preview_samples_device", (uintptr_t)d_out, blocking,
                        [&] { return preview_launch(c, p, p->y0, p->y1, nullptr, d_out, nullptr, nullptr, 0); });
}

int rtr_preview(rtr_context* c, const rtr_preview_params* p, const rtr_shade_env* env, double* h_linear, int64_t row_stride,
                int32_t* h_lit) {
    return preview_host(c, "rtr_preview", p, env, false, nullptr, h_linear, row_stride, h_lit);
}

int rtr_preview_device(rtr_context* c, const rtr_preview_params* p, const rtr_shade_env* env, double* d_linear, int64_t row_stride,
                       int32_t* d_lit, int blocking) {
    return preview_device(c, "rtr_preview_device", p, env, false, nullptr, d_linear, row_stride, d_lit, blocking);
}

int rtr_preview_set(rtr_context* c, const rtr_preview_params* p, const rtr_shade_env* env, const rtr_capture_set* set,
                    double* h_linear, int64_t row_stride, int32_t* h_lit) {
    return preview_host(c, "rtr_preview_set", p, env, true, set, h_linear, row_stride, h_lit);
}

int rtr_preview_set_device(rtr_context* c, const rtr_preview_params* p, const rtr_shade_env* env, const rtr_capture_set* set,
                           double* d_linear, int64_t row_stride, int32_t* d_lit, int blocking) {
    return preview_device(c, "rtr_preview_set_device", p, env, true, set, d_linear, row_stride, d_lit, blocking);
}

} /* extern "C" */
