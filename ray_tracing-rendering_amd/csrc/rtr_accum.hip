/*
 * rtr_accum.hip -- progressive accumulators (include/rtr_hip.h: rtr_accum_*): create / destroy / reset, the passes
 * (render, render_tiles, refine: render_core of rtr_capi.hip with the plan and commit kernels of this unit around its
 * megakernel), resolve, tiles, moments, errors and the first-hit features.  Holds the kernels of rt_accum_kernels.h
 * and the k_features instantiations.
 */
#include "rt_accum_kernels.h"
#include "rt_context.h"

#include <cstring>

using namespace rtr;

namespace rtr {

/* the host copy of an accumulator's counts, once every pass queued before has finished */
int refresh_counts(rtr_context* c, const rtr_accum* a) {
    if (!a->counts_stale || a->tiles.empty()) return RTR_OK;
    HIPCHK(c, hipMemcpyAsync(a->h_counts.data(), a->d_count.p, a->tiles.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    a->counts_stale = false;
    return RTR_OK;
}

/* the checks every rtr_accum_* call of a context makes */
int accum_check(rtr_context* c, const rtr_accum* a) {
    if (!a) return fail(c, RTR_ERR_INVALID, "null accumulator");
    if (a->ctx != c) return fail(c, RTR_ERR_INVALID, "the accumulator belongs to another context");
    return RTR_OK;
}

/* ... and those of the calls that render */
int accum_render_check(rtr_context* c, const rtr_accum* a) {
    if (int rc = accum_check(c, a)) return rc;
    if (!c->has_scene || a->scene_gen != c->scene_gen)
        return fail(c, RTR_ERR_INVALID, "the scene changed since the accumulator was created (rtr_upload_scene)");
    if (a->camera_gen != c->camera_gen)
        return fail(c, RTR_ERR_INVALID, "the camera changed since the accumulator was created or reset (rtr_set_camera): its "
                                        "samples belong to the old camera, call rtr_accum_reset");
    return RTR_OK;
}

/* an accumulator's sums and counts as kernel parameters (k_accum_resolve, k_accum_errors) */
AccumResolveK accum_view(const rtr_accum* a) {
    const rtr_render_params& p = a->params;
    AccumResolveK R{};
    R.r.W = p.image_width, R.r.H = p.image_height;
    R.r.x0 = p.x0, R.r.y0 = p.y0, R.r.x1 = p.x1, R.r.y1 = p.y1;
    R.r.tiles_x = a->tiles_x, R.r.tiles_y = a->tiles_y;
    R.r.tile_ids = static_cast<const int*>(a->d_tiles.p);
    R.r.n_tiles = (int)a->tiles.size();
    R.sum = static_cast<const double*>(a->d_sum.p);
    R.count = static_cast<const int*>(a->d_count.p);
    return R;
}

void free_accum(rtr_accum* a) {
    DevBuf* bufs[] = {&a->d_tiles, &a->d_sum, &a->d_count, &a->d_out, &a->d_q, &a->d_qpart, &a->d_s1, &a->d_active, &a->d_nactive, &a->d_err,
                      &a->d_feat};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    if (a->h_out) hipHostFree(a->h_out);
    delete a;
}

/* the features of K samples per pixel of every owned tile in a->d_feat, unless they are there already */
int accum_features(rtr_context* c, rtr_accum* a, int K) {
    const size_t n = a->tiles.size();
    if (a->feat_k == K || n == 0) return RTR_OK;
    a->feat_k = 0;
    if (int rc = ensure_behind_queue(c, a->d_feat, n * RTR_FEAT * RTR_BLOCK * sizeof(double))) return rc;
    RenderK P = accum_view(a).r;
    P.seed = a->params.seed;
    double* feat = static_cast<double*>(a->d_feat.p);
    const int trav = per_ray_trav(c->facts, c->info, a->params.flags, false); /* the traversals of k_li */
    const size_t lds = stack_bytes(c->facts, c->info, trav);
    int rc = RTR_OK;
    if (!dispatch_trav(TravsLi{}, trav, [&](auto t) {
            constexpr int T = decltype(t)::value;
            if ((rc = set_lds(c, k_features<T>, lds))) return;
            hipLaunchKernelGGL((k_features<T>), dim3((unsigned)n), dim3(RTR_BLOCK), lds, c->stream, c->ds, P, K, feat);
        }))
        return no_per_ray_kernel(c, trav);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    a->feat_k = K;
    return RTR_OK;
}

void accum_pass_plan(rtr_accum* acc, const AccumPlanK* plan, int n_tiles, hipStream_t stream, int* launches) {
    acc->counts_stale = true;
    AccumPlanK K = *plan;
    K.n_tiles = n_tiles;
    K.count = static_cast<const int*>(acc->d_count.p);
    K.err = static_cast<const double*>(acc->d_err.p);
    K.tile_s1 = static_cast<int*>(acc->d_s1.p);
    K.active = static_cast<int*>(acc->d_active.p);
    K.n_active = static_cast<int*>(acc->d_nactive.p);
    if (K.mode == 2) {
        hipLaunchKernelGGL(k_accum_errors, dim3((unsigned)n_tiles), dim3(RTR_BLOCK), 0, stream, accum_view(acc),
                           static_cast<const double*>(acc->d_q.p), static_cast<double*>(acc->d_err.p));
        ++*launches;
    }
    hipLaunchKernelGGL(k_accum_plan, dim3(1), dim3(1024), 0, stream, K);
    ++*launches;
}

void accum_pass_commit(rtr_accum* acc, const RenderK& P, hipStream_t stream) {
    hipLaunchKernelGGL(k_accum_commit, dim3((unsigned)P.n_tiles), dim3(RTR_BLOCK), 0, stream, P, static_cast<double*>(acc->d_sum.p),
                       static_cast<double*>(acc->moments ? acc->d_q.p : nullptr), static_cast<int*>(acc->d_count.p));
}

} // namespace rtr

namespace {

/* the device and pinned host staging of rtr_accum_resolve / rtr_accum_moments, at least `bytes` each */
int staging(rtr_context* c, rtr_accum* a, size_t bytes) {
    if (int rc = ensure(c, a->d_out, bytes)) return rc;
    if (bytes > a->h_out_cap) {
        if (a->h_out) HIPCHK(c, hipHostFree(a->h_out));
        a->h_out = nullptr, a->h_out_cap = 0;
        if (hipHostMalloc(&a->h_out, bytes, hipHostMallocDefault) != hipSuccess)
            return fail(c, RTR_ERR_NOMEM, "hipHostMalloc of the resolve staging buffer");
        a->h_out_cap = bytes;
    }
    return RTR_OK;
}

/* every row of an owned tile that holds samples, clipped to the region: f(slot, row in the tile, j, i0, i1, tile x0) --
 * where the host scatters packed tiles into a caller's region (its other pixels stay) */
template <class F>
void for_each_owned_row(const rtr_accum* a, F f) {
    const rtr_render_params& p = a->params;
    for (size_t k = 0; k < a->tiles.size(); ++k) {
        if (a->h_counts[k] == 0) continue;
        const int t = a->tiles[k];
        const int tx0 = (t % a->tiles_x) * 16, ty0 = ((a->tiles_y - 1) - t / a->tiles_x) * 16; /* renderer.h:61-62 */
        const int i0 = std::max(tx0, p.x0), i1 = std::min(tx0 + 16, p.x1);
        if (i0 >= i1) continue;
        for (int r = 0; r < 16; ++r) {
            const int j = ty0 + r;
            if (j >= p.y0 && j < p.y1) f(k, r, j, i0, i1, tx0);
        }
    }
}

/* an empty accumulator: sums, counts and moments zeroed on the stream (rtr_accum_create_ex, rtr_accum_reset) */
int accum_clear(rtr_context* c, rtr_accum* a) {
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    hipError_t e = hipMemsetAsync(a->d_sum.p, 0, n * 3 * RTR_BLOCK * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a->d_count.p, 0, n * sizeof(int), c->stream);
    if (e == hipSuccess && a->moments) e = hipMemsetAsync(a->d_q.p, 0, n * RTR_BLOCK * sizeof(double), c->stream);
    return e == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
}

} // namespace

extern "C" {

/* the seam of rt_debug.h: caller-given sums, moments and counts in place of what accum_clear zeroes */
int rtr_debug_accum_load(rtr_context* c, rtr_accum* a, const double* sum, const double* q, const int32_t* count, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!sum || !count) return fail(c, RTR_ERR_INVALID, "null sum or count");
    if ((q != nullptr) != a->moments) return fail(c, RTR_ERR_INVALID, "q must be given exactly when the accumulator keeps moments");
    if (n != (int64_t)a->tiles.size()) return fail(c, RTR_ERR_INVALID, "n is not the number of owned tiles");
    for (int64_t k = 0; k < n; ++k)
        if (count[k] < 0) return fail(c, RTR_ERR_INVALID, "negative sample count");
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* its queued passes */
    const size_t m = (size_t)n;
    HIPCHK(c, hipMemcpyAsync(a->d_sum.p, sum, m * 3 * RTR_BLOCK * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (q) HIPCHK(c, hipMemcpyAsync(a->d_q.p, q, m * RTR_BLOCK * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(a->d_count.p, count, m * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the arrays are the caller's */
    a->h_counts.assign(count, count + m);
    a->counts_stale = false;
    return RTR_OK;
}

int rtr_accum_create(rtr_context* c, const rtr_render_params* p, rtr_accum** out) { return rtr_accum_create_ex(c, p, 0, out); }

int rtr_accum_create_ex(rtr_context* c, const rtr_render_params* p, uint32_t accum_flags, rtr_accum** out) {
    if (!c) return RTR_ERR_INVALID;
    if (!out) return fail(c, RTR_ERR_INVALID, "null out");
    *out = nullptr;
    if (!p) return fail(c, RTR_ERR_INVALID, "null params");
    if (accum_flags & ~(uint32_t)RTR_ACCUM_MOMENTS) return fail(c, RTR_ERR_INVALID, "unknown accumulator flags");
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_accum_create before rtr_upload_scene");
    rtr_render_params q = *p;
    q.spp = 1, q.spp_chunks = 1; /* ignored: one running sum per pixel, targets come with the passes */
    if (int prc = params_check(c, &q)) return prc;
    if (q.pipeline == RTR_PIPELINE_WAVEFRONT) return fail(c, RTR_ERR_UNSUPPORTED, "accumulators run the megakernel pipeline only");
    HIPCHK(c, hipSetDevice(c->device));
    rtr_accum* a = new rtr_accum();
    a->ctx = c;
    a->params = q;
    a->scene_gen = c->scene_gen;
    a->camera_gen = c->camera_gen;
    a->moments = (accum_flags & RTR_ACCUM_MOMENTS) != 0;
    a->tiles = owned_tiles(q, a->tiles_x, a->tiles_y);
    const size_t n = a->tiles.size();
    a->h_counts.assign(n, 0);
    int rc = upload(c, a->d_tiles, a->tiles.data(), n * sizeof(int));
    if (!rc) rc = ensure(c, a->d_sum, n * 3 * RTR_BLOCK * sizeof(double));
    if (!rc) rc = ensure(c, a->d_count, n * sizeof(int));
    if (!rc) rc = ensure(c, a->d_s1, n * sizeof(int));
    if (!rc) rc = ensure(c, a->d_active, n * sizeof(int));
    if (!rc) rc = ensure(c, a->d_nactive, sizeof(int));
    if (!rc && a->moments) rc = ensure(c, a->d_q, n * RTR_BLOCK * sizeof(double));
    if (!rc && a->moments) rc = ensure(c, a->d_qpart, n * RTR_BLOCK * sizeof(double));
    if (!rc && a->moments) rc = ensure(c, a->d_err, n * sizeof(double));
    if (!rc) rc = accum_clear(c, a);
    if (rc) {
        free_accum(a);
        return rc;
    }
    c->accums.push_back(a);
    *out = a;
    return RTR_OK;
}

void rtr_accum_destroy(rtr_accum* a) {
    if (!a) return;
    rtr_context* c = a->ctx;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream); /* a pass may still use the buffers */
    c->accums.erase(std::remove(c->accums.begin(), c->accums.end(), a), c->accums.end());
    free_accum(a);
}

int rtr_accum_reset(rtr_context* c, rtr_accum* a, uint32_t seed) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!c->has_scene || a->scene_gen != c->scene_gen)
        return fail(c, RTR_ERR_INVALID, "the scene changed since the accumulator was created (rtr_upload_scene)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* its queued passes */
    if (int rc = accum_clear(c, a)) return rc;
    a->h_counts.assign(a->tiles.size(), 0);
    a->counts_stale = false;
    a->feat_k = 0;
    a->params.seed = seed;
    a->camera_gen = c->camera_gen;
    return RTR_OK;
}

int rtr_accum_render(rtr_context* c, rtr_accum* a, int32_t spp_target, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (spp_target < 0) return fail(c, RTR_ERR_INVALID, "negative target");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = refresh_counts(c, a)) return rc;
    bool behind = false;
    for (int n : a->h_counts) {
        if (spp_target < n) return fail(c, RTR_ERR_INVALID, "target below the sample count of a tile");
        behind = behind || n < spp_target;
    }
    if (!behind) return nothing_to_render(c); /* every tile is there */
    rtr_render_params q = a->params;
    q.spp = spp_target, q.spp_chunks = 1;
    AccumPlanK plan{};
    plan.mode = 1, plan.spp = spp_target;
    return render_core(c, &q, nullptr, 0, nullptr, blocking, a, &plan);
}

int rtr_accum_render_tiles(rtr_context* c, rtr_accum* a, const int32_t* targets, int64_t n, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (!targets) return fail(c, RTR_ERR_INVALID, "null targets");
    if (n != (int64_t)a->tiles.size()) return fail(c, RTR_ERR_INVALID, "n is not the number of owned tiles");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = refresh_counts(c, a)) return rc; /* (and the passes that read the old targets have finished) */
    bool behind = false;
    for (int64_t k = 0; k < n; ++k) {
        if (targets[k] < a->h_counts[k]) return fail(c, RTR_ERR_INVALID, "target below the sample count of a tile");
        behind = behind || a->h_counts[k] < targets[k];
    }
    if (!behind) return nothing_to_render(c);
    if (int rc = upload(c, a->d_s1, targets, (size_t)n * sizeof(int32_t))) return rc;
    rtr_render_params q = a->params;
    q.spp = *std::max_element(targets, targets + n), q.spp_chunks = 1;
    AccumPlanK plan{};
    plan.mode = 0;
    return render_core(c, &q, nullptr, 0, nullptr, blocking, a, &plan);
}

int rtr_accum_refine(rtr_context* c, rtr_accum* a, double threshold, int32_t spp_min, int32_t spp_max, int blocking,
                     int32_t* n_active) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (!a->moments) return fail(c, RTR_ERR_INVALID, "the accumulator keeps no moments (RTR_ACCUM_MOMENTS)");
    if (!(threshold > 0.0)) return fail(c, RTR_ERR_INVALID, "threshold must be > 0");
    if (spp_min < 1 || spp_max < spp_min) return fail(c, RTR_ERR_INVALID, "need 1 <= spp_min <= spp_max");
    if (n_active) *n_active = -1;
    HIPCHK(c, hipSetDevice(c->device));
    rtr_render_params q = a->params;
    q.spp = spp_max, q.spp_chunks = 1;
    AccumPlanK plan{};
    plan.mode = 2, plan.spp_min = spp_min, plan.spp_max = spp_max, plan.threshold = threshold;
    int rc = render_core(c, &q, nullptr, 0, nullptr, blocking, a, &plan);
    if ((rc == RTR_OK || rc == RTR_ERR_CANCELLED) && blocking && n_active && !a->tiles.empty()) {
        int na = 0;
        HIPCHK(c, hipMemcpy(&na, a->d_nactive.p, sizeof(int), hipMemcpyDeviceToHost));
        *n_active = na;
    } else if (rc == RTR_OK && n_active && a->tiles.empty()) {
        *n_active = 0;
    }
    return rc;
}

int rtr_accum_resolve(rtr_context* c, rtr_accum* a, double* h_linear, int64_t row_stride, uint8_t* h_rgb8) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    const rtr_render_params& p = a->params;
    const int w = p.x1 - p.x0;
    if (!h_linear && !h_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    if (h_linear && row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad output stride");
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = refresh_counts(c, a)) return rc; /* (waits for the passes queued before) */
    const size_t lin_bytes = n * RTR_BLOCK * 3 * sizeof(double), rgb_bytes = n * RTR_BLOCK * 3;
    if (int rc = staging(c, a, lin_bytes + rgb_bytes)) return rc;
    char* d = static_cast<char*>(a->d_out.p);
    char* h = static_cast<char*>(a->h_out);
    AccumResolveK R = accum_view(a);
    R.out = h_linear ? reinterpret_cast<double*>(d) : nullptr;
    R.rgb8 = h_rgb8 ? reinterpret_cast<unsigned char*>(d + lin_bytes) : nullptr;
    hipLaunchKernelGGL(k_accum_resolve, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, R);
    HIPCHK(c, hipGetLastError());
    if (h_linear) HIPCHK(c, hipMemcpyAsync(h, d, lin_bytes, hipMemcpyDeviceToHost, c->stream));
    if (h_rgb8) HIPCHK(c, hipMemcpyAsync(h + lin_bytes, d + lin_bytes, rgb_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    /* scatter the owned tiles that hold samples into the region (the caller's other pixels stay) */
    const double* lin = reinterpret_cast<const double*>(h);
    const unsigned char* rgb = reinterpret_cast<const unsigned char*>(h + lin_bytes);
    for_each_owned_row(a, [&](size_t k, int r, int j, int i0, int i1, int tx0) {
        const size_t src = (k * RTR_BLOCK + (size_t)r * 16 + (size_t)(i0 - tx0)) * 3, len = (size_t)(i1 - i0) * 3;
        if (h_linear)
            std::memcpy(h_linear + ((size_t)(j - p.y0) * (size_t)row_stride + (size_t)(i0 - p.x0)) * 3, lin + src,
                        len * sizeof(double));
        if (h_rgb8) /* Y flipped: the top row of the region first (render_buffer.h:40-41) */
            std::memcpy(h_rgb8 + ((size_t)(p.y1 - 1 - j) * (size_t)w + (size_t)(i0 - p.x0)) * 3, rgb + src, len);
    });
    return RTR_OK;
}

int rtr_accum_resolve_device(rtr_context* c, rtr_accum* a, double* d_linear, int64_t row_stride, uint8_t* d_rgb8, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    const rtr_render_params& p = a->params;
    if (!d_linear && !d_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    if (d_linear && row_stride < (int64_t)(p.x1 - p.x0)) return fail(c, RTR_ERR_INVALID, "bad output stride");
    if (reinterpret_cast<uintptr_t>(d_linear) % sizeof(double)) return fail(c, RTR_ERR_INVALID, "d_linear is not 8-byte aligned");
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    AccumResolveK R = accum_view(a); /* the counts stay on the device: the kernel leaves a tile without samples alone */
    R.out = d_linear, R.rgb8 = d_rgb8;
    hipLaunchKernelGGL(k_accum_resolve_scatter, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, R, (long long)row_stride);
    HIPCHK(c, hipGetLastError());
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

int rtr_accum_tiles(rtr_context* c, const rtr_accum* a, int32_t* tile_ids, int32_t* counts, int64_t cap, int64_t* n_tiles) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!n_tiles || cap < 0) return fail(c, RTR_ERR_INVALID, "null n_tiles or negative cap");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = refresh_counts(c, a)) return rc;
    const size_t n = a->tiles.size(), m = std::min(n, (size_t)cap);
    *n_tiles = (int64_t)n;
    if (tile_ids && m) std::memcpy(tile_ids, a->tiles.data(), m * sizeof(int32_t));
    if (counts && m) std::memcpy(counts, a->h_counts.data(), m * sizeof(int32_t));
    return RTR_OK;
}

int rtr_accum_moments(rtr_context* c, rtr_accum* a, double* h_q, int64_t row_stride) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!a->moments) return fail(c, RTR_ERR_INVALID, "the accumulator keeps no moments (RTR_ACCUM_MOMENTS)");
    const rtr_render_params& p = a->params;
    if (!h_q || row_stride < (int64_t)(p.x1 - p.x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = refresh_counts(c, a)) return rc;
    const size_t bytes = n * RTR_BLOCK * sizeof(double);
    if (int rc = staging(c, a, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(a->h_out, a->d_q.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double* q = static_cast<const double*>(a->h_out);
    for_each_owned_row(a, [&](size_t k, int r, int j, int i0, int i1, int tx0) {
        std::memcpy(h_q + (size_t)(j - p.y0) * (size_t)row_stride + (size_t)(i0 - p.x0),
                    q + k * RTR_BLOCK + (size_t)r * 16 + (size_t)(i0 - tx0), (size_t)(i1 - i0) * sizeof(double));
    });
    return RTR_OK;
}

int rtr_accum_errors(rtr_context* c, rtr_accum* a, double* tile_err, int64_t cap, int64_t* n_tiles) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!a->moments) return fail(c, RTR_ERR_INVALID, "the accumulator keeps no moments (RTR_ACCUM_MOMENTS)");
    if (!n_tiles || cap < 0) return fail(c, RTR_ERR_INVALID, "null n_tiles or negative cap");
    const size_t n = a->tiles.size(), m = std::min(n, (size_t)cap);
    *n_tiles = (int64_t)n;
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_accum_errors, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, accum_view(a),
                       static_cast<const double*>(a->d_q.p), static_cast<double*>(a->d_err.p));
    HIPCHK(c, hipGetLastError());
    if (tile_err && m) HIPCHK(c, hipMemcpyAsync(tile_err, a->d_err.p, m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

int rtr_accum_features(rtr_context* c, rtr_accum* a, int32_t feature_spp, double* h_feat, int64_t row_stride) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (feature_spp < 1) return fail(c, RTR_ERR_INVALID, "feature_spp must be >= 1");
    const rtr_render_params& p = a->params;
    if (!h_feat || row_stride < (int64_t)(p.x1 - p.x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = accum_features(c, a, feature_spp)) return rc;
    const size_t bytes = n * RTR_FEAT * RTR_BLOCK * sizeof(double);
    if (int rc = staging(c, a, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(a->h_out, a->d_feat.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double* f = static_cast<const double*>(a->h_out);
    for (size_t k = 0; k < n; ++k) { /* every owned tile, with or without samples */
        const int t = a->tiles[k];
        const int tx0 = (t % a->tiles_x) * 16, ty0 = ((a->tiles_y - 1) - t / a->tiles_x) * 16;
        for (int r = 0; r < 16; ++r) {
            const int j = ty0 + r;
            if (j < p.y0 || j >= p.y1) continue;
            for (int i = std::max(tx0, p.x0); i < std::min(tx0 + 16, p.x1); ++i)
                for (int ch = 0; ch < RTR_FEAT; ++ch)
                    h_feat[((size_t)(j - p.y0) * (size_t)row_stride + (size_t)(i - p.x0)) * RTR_FEAT + ch] =
                        f[(k * RTR_FEAT + ch) * RTR_BLOCK + (size_t)r * 16 + (size_t)(i - tx0)];
        }
    }
    return RTR_OK;
}

int rtr_accum_features_device(rtr_context* c, rtr_accum* a, int32_t feature_spp, double* d_feat, int64_t row_stride, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (feature_spp < 1) return fail(c, RTR_ERR_INVALID, "feature_spp must be >= 1");
    const rtr_render_params& p = a->params;
    if (!d_feat || row_stride < (int64_t)(p.x1 - p.x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    if (reinterpret_cast<uintptr_t>(d_feat) % sizeof(double)) return fail(c, RTR_ERR_INVALID, "d_feat is not 8-byte aligned");
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (int rc = accum_features(c, a, feature_spp)) return rc;
    hipLaunchKernelGGL(k_accum_features_scatter, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, accum_view(a).r,
                       static_cast<const double*>(a->d_feat.p), d_feat, (long long)row_stride);
    HIPCHK(c, hipGetLastError());
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

} /* extern "C" */
