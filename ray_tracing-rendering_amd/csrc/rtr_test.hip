/*
 * rtr_test.hip -- librtr_hip_test.so: the entry points of include/rtr_hip_test.h.  Test infrastructure, built next to
 * librtr_hip.so and linked against it; it reaches a context only through the seam of csrc/rt_debug.h.
 */
/* (a link unit of its own: rtr_test_temporal_planes launches its own copy of k_temporal_blend / _store, rtr_test_accum_plan
 * and rtr_test_accum_commit theirs of k_accum_plan and k_accum_commit) */
#include "rt_accum_kernels.h"
#include "rt_debug.h"
#include "rt_image_kernels.h"
#include "rt_launch.h"
#include "rt_test_kernels.h"
#include "rtr_hip_test.h"

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

struct TestState {
    void* buf = nullptr;
    size_t cap = 0;
    bool reference_order = false;
};
std::mutex g_mu;
std::map<rtr_context*, TestState> g_state; /* contexts are few and live as long as a test session */

TestState& state_of(rtr_context* c) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_state[c];
}
int fail(rtr_context* c, int code, const std::string& msg) {
    rtr_debug_set_error(c, msg.c_str());
    return code;
}
#define TCHK(ctx, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(ctx, RTR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int ensure(rtr_context* c, TestState& t, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (t.cap >= bytes) return RTR_OK;
    if (t.buf) TCHK(c, hipFree(t.buf));
    t.buf = nullptr, t.cap = 0;
    if (hipMalloc(&t.buf, bytes) != hipSuccess) return fail(c, RTR_ERR_NOMEM, "hipMalloc of the test record buffer");
    t.cap = bytes;
    return RTR_OK;
}
/* view of the context + the records on the device */
int begin(rtr_context* c, const void* recs, int64_t n, size_t rec_size, rtr_debug_view& v, TestState*& t, bool need_scene = true) {
    if (!c) return RTR_ERR_INVALID;
    t = &state_of(c);
    if (need_scene) {
        if (int rc = rtr_debug_view_get(c, t->reference_order ? RTR_FLAG_REFERENCE_ORDER : 0, &v, sizeof v)) return rc;
    }
    if (n < 0 || (n > 0 && !recs)) return fail(c, RTR_ERR_INVALID, "bad record array");
    if (int rc = rtr_synchronize(c)) return rc;
    if (int rc = ensure(c, *t, (size_t)n * rec_size)) return rc;
    if (n) TCHK(c, hipMemcpy(t->buf, recs, (size_t)n * rec_size, hipMemcpyHostToDevice));
    return RTR_OK;
}
int end(rtr_context* c, hipStream_t stream, TestState* t, void* recs, int64_t n, size_t rec_size) {
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    if (n) TCHK(c, hipMemcpy(recs, t->buf, (size_t)n * rec_size, hipMemcpyDeviceToHost));
    return RTR_OK;
}
dim3 grid_of(int64_t n) { return dim3((unsigned)((n + RTR_BLOCK - 1) / RTR_BLOCK)); }

template <typename K>
int set_lds(rtr_context* c, K kernel, size_t bytes) {
    std::string err;
    const int rc = kernel_lds(kernel, bytes, 0, err);
    return rc ? fail(c, rc, err) : RTR_OK;
}
/* a bare context: stream, device and CU count without a scene */
int bare(rtr_context* c, hipStream_t& stream, int& n_cus, TestState*& t) {
    if (!c) return RTR_ERR_INVALID;
    t = &state_of(c);
    if (int rc = rtr_synchronize(c)) return rc;
    stream = nullptr; /* the kernels below are self-contained: the null stream orders them after everything */
    hipDeviceProp_t prop;
    int dev = 0;
    TCHK(c, hipGetDevice(&dev));
    TCHK(c, hipGetDeviceProperties(&prop, dev));
    n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return RTR_OK;
}

/* 2^26 operand sets through k_test_lane<OP>: 1024 workgroups, 256 sets per lane */
template <int OP>
int lane_test(rtr_context* c, uint64_t* mismatches, uint64_t* tested, uint64_t* short_sets, uint64_t* first) {
    if (!c || !mismatches || !tested || !short_sets || !first) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 64))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, 64, stream));
    const unsigned blocks = 1024, per_thread = (unsigned)((1ull << 26) / ((unsigned long long)blocks * RTR_BLOCK));
    hipLaunchKernelGGL(k_test_lane<OP>, dim3(blocks), dim3(RTR_BLOCK), 0, stream, static_cast<unsigned long long*>(t->buf), per_thread);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream)); /* the kernel's stream, before the counters are read */
    unsigned long long h[8] = {0};
    TCHK(c, hipMemcpy(h, t->buf, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1], *short_sets = h[7];
    for (int k = 0; k < 4; ++k) first[k] = h[2] ? h[3 + k] : 0;
    return RTR_OK;
}
} // namespace

extern "C" {

int rtr_test_hits(rtr_context* c, rtr_hit_record* recs, int64_t n) {
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc || n == 0) return rc;
    TCHK(c, hipSetDevice(v.device));
    DScene ds = v.ds;
    ds.needs_uv = 1; /* the vectors pin u,v although no flattened texture of these scenes reads them */
    auto* d = static_cast<rtr_hit_record*>(t->buf);
    const size_t lds = v.stack_bytes;
    /* (rtr_debug_view::trav is a template value already: per_ray_trav of rt_select.h) */
    if (!dispatch_trav(TravSet<RT_TRAV_FAST, RT_TRAV_TOP, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>{}, v.trav, [&](auto t) {
            constexpr int T = decltype(t)::value;
            if ((rc = set_lds(c, k_test_hits<T>, lds))) return;
            hipLaunchKernelGGL(k_test_hits<T>, grid_of(n), dim3(RTR_BLOCK), lds, v.stream, ds, d, (long long)n);
        }))
        return fail(c, RTR_ERR_UNSUPPORTED, "no unit kernel for traversal " + std::to_string(v.trav));
    if (rc) return rc;
    return end(c, v.stream, t, recs, n, sizeof *recs);
}

int rtr_test_flat_hits(rtr_context* c, rtr_hit_record* recs, int64_t n, int with_uv, int32_t* used_finish) {
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc) return rc;
    if (v.flat_trav < 0) return fail(c, RTR_ERR_UNSUPPORTED, "no flat kernel runs this scene");
    if (used_finish) *used_finish = v.ds.ffin != nullptr;
    if (n == 0) return RTR_OK;
    TCHK(c, hipSetDevice(v.device));
    DScene ds = v.ds;
    ds.needs_uv = with_uv ? 1 : 0;
    auto* d = static_cast<rtr_hit_record*>(t->buf);
    const size_t lds = v.stack_bytes;
    if (!dispatch_trav(TravSet<RT_TRAV_FLAT, RT_TRAV_FLAT_GUARD>{}, v.flat_trav, [&](auto t) {
            constexpr int T = decltype(t)::value;
            if ((rc = set_lds(c, k_test_flat_hits<T>, lds))) return;
            hipLaunchKernelGGL(k_test_flat_hits<T>, grid_of(n), dim3(RTR_BLOCK), lds, v.stream, ds, d, (long long)n);
        }))
        return fail(c, RTR_ERR_UNSUPPORTED, "no unit kernel for traversal " + std::to_string(v.flat_trav));
    if (rc) return rc;
    return end(c, v.stream, t, recs, n, sizeof *recs);
}

/* the unit kernels of the shading functions, instantiated for material set `ms` as the render kernels are; a scene that
 * mega_variant would not give such a kernel is refused before anything is copied */
static int ms_refused(rtr_context* c, int ms) {
    rtr_debug_view v;
    if (ms != RT_MS_LEAN && ms != RT_MS_FULL && ms != RT_MS_QUADLIT) return fail(c, RTR_ERR_INVALID, "unknown material set");
    if (int rc = rtr_debug_view_get(c, 0, &v, sizeof v)) return rc;
    if (ms == RT_MS_LEAN && !v.lean_ok) return fail(c, RTR_ERR_UNSUPPORTED, "the uploaded scene gets no RT_MS_LEAN kernel");
    if (ms == RT_MS_QUADLIT && !v.quadlit_ok) return fail(c, RTR_ERR_UNSUPPORTED, "the uploaded scene gets no RT_MS_QUADLIT kernel");
    return RTR_OK;
}
#define RTR_LAUNCH_MS(KERNEL, ms, ...)                                                                        \
    do {                                                                                                       \
        if ((ms) == RT_MS_LEAN) hipLaunchKernelGGL(KERNEL<RT_MS_LEAN>, __VA_ARGS__);                           \
        else if ((ms) == RT_MS_QUADLIT) hipLaunchKernelGGL(KERNEL<RT_MS_QUADLIT>, __VA_ARGS__);                \
        else hipLaunchKernelGGL(KERNEL<RT_MS_FULL>, __VA_ARGS__);                                              \
    } while (0)

static int mat_records(rtr_context* c, rtr_mat_record* recs, int64_t n, int ms, bool scatter) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = ms_refused(c, ms)) return rc;
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc || n == 0) return rc;
    for (int64_t k = 0; k < n; ++k)
        if (recs[k].material < 0 || recs[k].material >= v.n_materials) return fail(c, RTR_ERR_INVALID, "material index out of range");
    TCHK(c, hipSetDevice(v.device));
    auto* d = static_cast<rtr_mat_record*>(t->buf);
    if (scatter)
        RTR_LAUNCH_MS(k_test_scatter, ms, grid_of(n), dim3(RTR_BLOCK), 0, v.stream, v.ds, d, (long long)n);
    else
        RTR_LAUNCH_MS(k_test_materials, ms, grid_of(n), dim3(RTR_BLOCK), 0, v.stream, v.ds, d, (long long)n);
    return end(c, v.stream, t, recs, n, sizeof *recs);
}
int rtr_test_materials_ms(rtr_context* c, rtr_mat_record* recs, int64_t n, int32_t ms) { return mat_records(c, recs, n, ms, false); }
int rtr_test_materials(rtr_context* c, rtr_mat_record* recs, int64_t n) { return mat_records(c, recs, n, RT_MS_FULL, false); }
int rtr_test_scatter_ms(rtr_context* c, rtr_mat_record* recs, int64_t n, int32_t ms) { return mat_records(c, recs, n, ms, true); }
int rtr_test_scatter(rtr_context* c, rtr_mat_record* recs, int64_t n) { return mat_records(c, recs, n, RT_MS_FULL, true); }

int rtr_test_lights_ms(rtr_context* c, rtr_light_record* recs, int64_t n, int32_t ms) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = ms_refused(c, ms)) return rc;
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc || n == 0) return rc;
    for (int64_t k = 0; k < n; ++k)
        if (recs[k].light < 0 || recs[k].light >= v.ds.n_lights) return fail(c, RTR_ERR_INVALID, "light index out of range");
    TCHK(c, hipSetDevice(v.device));
    RTR_LAUNCH_MS(k_test_lights, ms, grid_of(n), dim3(RTR_BLOCK), 0, v.stream, v.ds, static_cast<rtr_light_record*>(t->buf), (long long)n);
    return end(c, v.stream, t, recs, n, sizeof *recs);
}
int rtr_test_lights(rtr_context* c, rtr_light_record* recs, int64_t n) { return rtr_test_lights_ms(c, recs, n, RT_MS_FULL); }

int rtr_test_pow5(rtr_context* c, const double* x, double* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (n < 0 || (n > 0 && (!x || !out))) return fail(c, RTR_ERR_INVALID, "bad array");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc || n == 0) return rc;
    if ((rc = ensure(c, *t, (size_t)n * 16))) return rc;
    double* dx = static_cast<double*>(t->buf);
    double* dout = dx + n;
    TCHK(c, hipMemcpy(dx, x, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_pow5, grid_of(n), dim3(RTR_BLOCK), 0, stream, dx, dout, (long long)n);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    TCHK(c, hipMemcpy(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RTR_OK;
}

int rtr_test_pow5_host(const double* x, double* out, int64_t n) {
    if (n < 0 || (n > 0 && (!x || !out))) return RTR_ERR_INVALID;
    for (int64_t k = 0; k < n; ++k) out[k] = pow5(x[k]);
    return RTR_OK;
}

/* Integrator::Li per camera sample with the RNG state at exit and the segment counts: the product's own per-ray kernel
 * (rtr_li_samples runs the same one and drops those fields) */
int rtr_test_li(rtr_context* c, const rtr_render_params* p, rtr_li_record* recs, int64_t n) {
    if (!c || !p) return RTR_ERR_INVALID;
    if (n < 0 || (n > 0 && !recs)) return fail(c, RTR_ERR_INVALID, "bad record array");
    std::vector<int32_t> ijs((size_t)n * 3);
    for (int64_t k = 0; k < n; ++k) ijs[3 * k] = recs[k].i, ijs[3 * k + 1] = recs[k].j, ijs[3 * k + 2] = recs[k].s;
    std::vector<rtr_debug_li_out> out((size_t)n);
    rtr_render_params q = *p;
    if (state_of(c).reference_order) q.flags |= RTR_FLAG_REFERENCE_ORDER;
    int rc = rtr_debug_li(c, &q, ijs.data(), out.data(), n);
    if (rc) return rc;
    for (int64_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) recs[k].L[a] = out[(size_t)k].L[a];
        recs[k].rng_exit = out[(size_t)k].rng_exit;
        recs[k].n_closest = out[(size_t)k].n_closest, recs[k].n_shadow = out[(size_t)k].n_shadow;
    }
    return RTR_OK;
}

int rtr_test_last_kernel(rtr_context* c, rtr_kernel_record* out, size_t size) {
    static_assert(sizeof(rtr_kernel_record) == sizeof(rtr_debug_kernel), "one layout");
    if (size != sizeof(rtr_kernel_record)) return RTR_ERR_INVALID;
    return rtr_debug_last_kernel(c, reinterpret_cast<rtr_debug_kernel*>(out), sizeof(rtr_debug_kernel));
}

/* the four records of the batch families are views of the one rtr_debug_batch */
static int last_batch(rtr_context* c, int family, const void* out, size_t size, size_t record_size, rtr_debug_batch& b) {
    if (!out || size != record_size) return RTR_ERR_INVALID;
    return rtr_debug_last_batch(c, family, &b, sizeof b);
}
int rtr_test_last_gather(rtr_context* c, rtr_gather_record* out, size_t size) {
    rtr_debug_batch b;
    if (int rc = last_batch(c, RTR_DEBUG_GATHER, out, size, sizeof *out, b)) return rc;
    *out = rtr_gather_record{b.integ, b.trav, b.broadcast, b.lg};
    return RTR_OK;
}
int rtr_test_last_probe(rtr_context* c, rtr_probe_record* out, size_t size) {
    rtr_debug_batch b;
    if (int rc = last_batch(c, RTR_DEBUG_PROBE, out, size, sizeof *out, b)) return rc;
    *out = rtr_probe_record{b.integ, b.trav, b.lg};
    return RTR_OK;
}
int rtr_test_last_capture(rtr_context* c, rtr_capture_record* out, size_t size) {
    rtr_debug_batch b;
    if (int rc = last_batch(c, RTR_DEBUG_CAPTURE, out, size, sizeof *out, b)) return rc;
    *out = rtr_capture_record{b.integ, b.trav, b.lg};
    return RTR_OK;
}
int rtr_test_last_probe_depth(rtr_context* c, rtr_probe_depth_record* out, size_t size) {
    rtr_debug_batch b;
    if (int rc = last_batch(c, RTR_DEBUG_PROBE_DEPTH, out, size, sizeof *out, b)) return rc;
    *out = rtr_probe_depth_record{b.trav, b.lg};
    return RTR_OK;
}

int rtr_test_scene_plan(const rtr_scene_desc* scene, int32_t integrator, int32_t flags, rtr_scene_plan* out, int32_t* ref_flags,
                        int64_t cap, rtr_finish_record* finish, int64_t finish_cap) {
    static_assert(sizeof(rtr_scene_plan) == sizeof(rtr_debug_plan), "one layout");
    static_assert(sizeof(rtr_finish_record) == sizeof(FFin), "one layout");
    return rtr_debug_scene_plan(scene, integrator, flags, reinterpret_cast<rtr_debug_plan*>(out), sizeof(rtr_debug_plan),
                                ref_flags, cap, finish, finish_cap);
}

int rtr_test_pair_frames(const rtr_scene_desc* scene, int32_t* shapes, int64_t cap, int32_t* n_instances) {
    return rtr_debug_frame_shapes(scene, shapes, cap, n_instances);
}

int rtr_test_queue_blocks_host(int32_t n_tiles, int32_t spp, int32_t chunks, int32_t n_big, int32_t big_spp, int32_t small_spp,
                               rtr_queue_block_record* recs, int64_t n) {
    if (n_tiles < 1 || spp < 1 || chunks < 1 || n < 0 || n > (int64_t)n_tiles * chunks * 4 || (n > 0 && !recs)) return RTR_ERR_INVALID;
    RenderK P{};
    P.n_tiles = n_tiles, P.spp = spp, P.chunks = chunks;
    P.n_big = n_big, P.big_spp = big_spp, P.small_spp = small_spp;
    for (int64_t b = 0; b < n; ++b) {
        const QueueBlock q = queue_block(P, (int)b);
        rtr_queue_block_record& r = recs[b];
        r.slot = q.slot, r.quarter = q.quarter, r.chunk = q.chunk, r.s0 = q.s0, r.s1 = q.s1, r.pad = 0;
        chunk_range(P, q.chunk, r.ref_s0, r.ref_s1);
    }
    return RTR_OK;
}

int rtr_test_queue_pack_host(int32_t i, int32_t j, int32_t s_end, uint32_t* lo, uint32_t* hi, int32_t* out) {
    if (!lo || !hi || !out) return RTR_ERR_INVALID;
    queue_pack(i, j, s_end, *lo, *hi);
    queue_unpack(*lo, *hi, out[0], out[1], out[2]);
    return RTR_OK;
}

int rtr_test_pair_frame_host(int32_t shape, const double* ops, rtr_pair_frame_record* recs, int64_t n) {
    if (shape < RT_SHAPE_NONE || shape > RT_SHAPE_RT || !ops || n < 0 || (n > 0 && !recs)) return RTR_ERR_INVALID;
    /* the chain op by op, as hittable.h:53,128-138 pass a ray down: 1 = translate, 2 = rotate_y */
    const int kinds[5][2] = {{0, 0}, {1, 0}, {2, 0}, {1, 2}, {2, 1}};
    auto enter = [&](V3& o, V3& d) {
        for (int k = 0; k < 2; ++k) {
            const double* f = ops + 3 * k;
            if (kinds[shape][k] == 1) {
                o.x = o.x - f[0], o.y = o.y - f[1], o.z = o.z - f[2];
            } else if (kinds[shape][k] == 2) {
                const double sn = f[0], cs = f[1];
                const double ox = cs * o.x - sn * o.z, oz = sn * o.x + cs * o.z;
                const double dx = cs * d.x - sn * d.z, dz = sn * d.x + cs * d.z;
                o.x = ox, o.z = oz, d.x = dx, d.z = dz;
            }
        }
    };
    auto same = [](double a, double b) { return std::memcmp(&a, &b, 8) == 0; };
    for (int64_t q = 0; q < n; ++q) {
        rtr_pair_frame_record& r = recs[q];
        V3 ao{r.ao[0], r.ao[1], r.ao[2]}, ad{r.ad[0], r.ad[1], r.ad[2]}, bo{r.bo[0], r.bo[1], r.bo[2]}, bd{r.bd[0], r.bd[1], r.bd[2]};
        const PairFrame F = pair_frame(shape, ops, ops + 3, ao, ad, bo, bd);
        V3 eao = ao, ead = ad, ebo = bo, ebd = bd;
        enter(eao, ead), enter(ebo, ebd);
        r.fo[0] = F.ao.x, r.fo[1] = F.ao.y, r.fo[2] = F.ao.z, r.fd[0] = F.adx, r.fd[1] = ad.y, r.fd[2] = F.adz;
        r.same_frame = same(F.ao.x, eao.x) && same(F.ao.y, eao.y) && same(F.ao.z, eao.z) && same(F.bo.x, ebo.x) &&
                       same(F.bo.y, ebo.y) && same(F.bo.z, ebo.z) && same(F.adx, ead.x) && same(F.adz, ead.z) &&
                       same(F.bdx, ebd.x) && same(F.bdz, ebd.z) && same(ad.y, ead.y) && same(bd.y, ebd.y);
        r.pad = 0;
    }
    return RTR_OK;
}

int rtr_test_pair_cast_text(rtr_context* c, rtr_pair_record* recs, int64_t n, int32_t recast) {
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc) return rc;
    if (!v.ds.pair_cast) return fail(c, RTR_ERR_UNSUPPORTED, "the uploaded scene is no pair-cast scene");
    if (n == 0) return RTR_OK;
    TCHK(c, hipSetDevice(v.device));
    const size_t lds = v.stack_bytes;
    rtr_pair_record* d = static_cast<rtr_pair_record*>(t->buf);
    if (recast) {
        if ((rc = set_lds(c, k_test_pair<true>, lds))) return rc;
        hipLaunchKernelGGL(k_test_pair<true>, grid_of(n), dim3(RTR_BLOCK), lds, v.stream, v.ds, d, (long long)n);
    } else {
        if ((rc = set_lds(c, k_test_pair<false>, lds))) return rc;
        hipLaunchKernelGGL(k_test_pair<false>, grid_of(n), dim3(RTR_BLOCK), lds, v.stream, v.ds, d, (long long)n);
    }
    return end(c, v.stream, t, recs, n, sizeof *recs);
}

int rtr_test_pair_cast(rtr_context* c, rtr_pair_record* recs, int64_t n) { return rtr_test_pair_cast_text(c, recs, n, 1); }

int rtr_test_pair_resident(rtr_context* c, rtr_pair_record* recs, int64_t n, int32_t casts) {
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, recs, n, sizeof *recs, v, t);
    if (rc) return rc;
    if (casts < 1) return fail(c, RTR_ERR_INVALID, "casts < 1");
    if (!v.ds.pair_cast) return fail(c, RTR_ERR_UNSUPPORTED, "the uploaded scene is no pair-cast scene");
    if (n == 0) return RTR_OK;
    TCHK(c, hipSetDevice(v.device));
    const int stack_words = (int)(v.stack_bytes / (RTR_BLOCK * sizeof(int)));
    const size_t lds = (size_t)stack_words * RTR_BLOCK * sizeof(int) + (size_t)RT_PARK_WORDS * RTR_BLOCK * sizeof(double);
    if ((rc = set_lds(c, k_test_pair_resident, lds))) return rc;
    hipLaunchKernelGGL(k_test_pair_resident, grid_of(n), dim3(RTR_BLOCK), lds, v.stream, v.ds, static_cast<rtr_pair_record*>(t->buf),
                       (long long)n, stack_words, (int)casts);
    return end(c, v.stream, t, recs, n, sizeof *recs);
}

int rtr_test_reference_order(rtr_context* c, int on) {
    if (!c) return RTR_ERR_INVALID;
    state_of(c).reference_order = on != 0;
    return RTR_OK;
}

int rtr_test_stream8(rtr_context* c, int64_t n_doubles, int repeat) {
    if (!c || n_doubles <= 0 || repeat <= 0) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, (size_t)n_doubles * 16))) return rc;
    double* in = static_cast<double*>(t->buf);
    double* out = in + n_doubles;
    TCHK(c, hipMemsetAsync(in, 0, (size_t)n_doubles * 16, stream));
    for (int r = 0; r < repeat; ++r)
        hipLaunchKernelGGL(k_stream8, dim3((unsigned)(n_cus * 16)), dim3(RTR_BLOCK), 0, stream, in, out, (long long)n_doubles);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    return RTR_OK;
}

int rtr_test_sincos_exhaustive(rtr_context* c, uint64_t* mismatches, uint64_t* tested) {
    if (!c || !mismatches || !tested) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 16))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, 16, stream));
    hipLaunchKernelGGL(k_test_sincos, dim3((unsigned)(n_cus * 16)), dim3(RTR_BLOCK), 0, stream, static_cast<unsigned long long*>(t->buf));
    TCHK(c, hipGetLastError());
    /* (the context's stream is non-blocking: the null-stream copy below does not wait for it) */
    TCHK(c, hipStreamSynchronize(stream));
    unsigned long long h[2] = {0, 0};
    TCHK(c, hipMemcpy(h, t->buf, 16, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1];
    return RTR_OK;
}

int rtr_test_issue_rates(rtr_context* c, double* cycles_per_inst, int n) {
    if (!c || !cycles_per_inst || n < 0) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 32))) return rc;
    auto* d = static_cast<unsigned long long*>(t->buf);
    const int iters = 4096;
    const dim3 grid((unsigned)(n_cus * 4));
    for (int k = 0; k < n && k < 18; ++k) {
        TCHK(c, hipMemsetAsync(d, 0, 32, stream));
#define RTR_RATE(K) case K: hipLaunchKernelGGL(k_test_issue_rate<K>, grid, dim3(RTR_BLOCK), 0, stream, d, iters, 1.25); break
        switch (k) {
            RTR_RATE(0); RTR_RATE(1); RTR_RATE(2); RTR_RATE(3); RTR_RATE(4); RTR_RATE(5); RTR_RATE(6);
            RTR_RATE(7); RTR_RATE(8); RTR_RATE(9); RTR_RATE(10); RTR_RATE(11); RTR_RATE(12);
            RTR_RATE(13); RTR_RATE(14); RTR_RATE(15); RTR_RATE(16); RTR_RATE(17);
        }
#undef RTR_RATE
        TCHK(c, hipGetLastError());
        TCHK(c, hipStreamSynchronize(stream));
        unsigned long long h[2] = {0, 0};
        TCHK(c, hipMemcpy(h, d, 16, hipMemcpyDeviceToHost));
        cycles_per_inst[k] = h[1] ? (double)h[0] / (double)h[1] / (32.0 * iters * (k == 12 || k == 15 || k == 17 ? 2 : (k == 16 ? 4 : 1))) : 0.0;
    }
    return RTR_OK;
}

int rtr_test_shared_division(rtr_context* c, uint64_t* mismatches, uint64_t* tested) {
    if (!c || !mismatches || !tested) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 16))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, 16, stream));
    const unsigned blocks = 4096, per_thread = (unsigned)((1ull << 32) / ((unsigned long long)blocks * RTR_BLOCK));
    hipLaunchKernelGGL(k_test_shared_div, dim3(blocks), dim3(RTR_BLOCK), 0, stream, static_cast<unsigned long long*>(t->buf), per_thread);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    unsigned long long h[2] = {0, 0};
    TCHK(c, hipMemcpy(h, t->buf, 16, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1];
    return RTR_OK;
}

int rtr_test_udiv(rtr_context* c, const double* num, int64_t n, const double* div, int32_t m, uint64_t* mismatches, uint64_t* tested) {
    if (!c || !mismatches || !tested) return RTR_ERR_INVALID;
    if (n < 1 || m < 1 || !num || !div) return fail(c, RTR_ERR_INVALID, "bad array");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 16 + (size_t)(n + m) * 8))) return rc;
    auto* counts = static_cast<unsigned long long*>(t->buf);
    double* dnum = reinterpret_cast<double*>(counts + 2);
    double* ddiv = dnum + n;
    TCHK(c, hipMemsetAsync(counts, 0, 16, stream));
    TCHK(c, hipMemcpy(dnum, num, (size_t)n * 8, hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(ddiv, div, (size_t)m * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_udiv, grid_of(n), dim3(RTR_BLOCK), 0, stream, dnum, (long long)n, ddiv, (int)m, counts);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    unsigned long long h[2] = {0, 0};
    TCHK(c, hipMemcpy(h, counts, 16, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1];
    return RTR_OK;
}

int rtr_test_rcp_lane(rtr_context* c, uint64_t* mismatches, uint64_t* tested, uint64_t* short_sets, uint64_t* first) {
    return lane_test<0>(c, mismatches, tested, short_sets, first);
}
int rtr_test_sqrt_lane(rtr_context* c, uint64_t* mismatches, uint64_t* tested, uint64_t* short_sets, uint64_t* first) {
    return lane_test<1>(c, mismatches, tested, short_sets, first);
}

int rtr_test_lane_specials(uint64_t* out, int64_t cap) {
    if (cap < 0 || (cap > 0 && !out)) return -1;
    for (int64_t k = 0; k < cap && k < RT_LANE_SPECIALS; ++k) out[k] = lane_special((unsigned)k);
    return RT_LANE_SPECIALS;
}

int rtr_test_lane_host(int32_t op, int32_t coarse_bits, const double* a, double* out, int32_t* took_short, int64_t n) {
    if (coarse_bits < 0 || coarse_bits > 40) return RTR_ERR_INVALID;
    rt_host_seed_coarse = coarse_bits;
    if (op < 0 || op > 1 || n < 0 || (n > 0 && (!a || !out || !took_short))) return RTR_ERR_INVALID;
    for (int64_t k = 0; k < n; ++k) {
        const bool s = op == 0 ? lane_window<-100, 100>(a[k]) : RT_SQRT_WINDOW(a[k]);
        if (op == 0)
            out[k] = s ? rcp_short(a[k]) : 1.0 / a[k];
        else
            out[k] = s ? sqrt_short(a[k]) : __builtin_sqrt(a[k]);
        took_short[k] = s;
    }
    return RTR_OK;
}

int rtr_test_draw_forms(rtr_context* c, uint64_t* mismatches, uint64_t* tested, uint64_t* first) {
    if (!c || !mismatches || !tested || !first) return RTR_ERR_INVALID;
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 32))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, 32, stream));
    hipLaunchKernelGGL(k_test_draw_forms, dim3((unsigned)(n_cus * 16)), dim3(RTR_BLOCK), 0, stream, static_cast<unsigned long long*>(t->buf));
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream)); /* the kernel's stream, before the counters are read */
    unsigned long long h[4] = {0};
    TCHK(c, hipMemcpy(h, t->buf, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1], *first = h[2];
    return RTR_OK;
}

int rtr_test_draw_callers(rtr_context* c, uint64_t seed, int64_t n, uint64_t* mismatches, uint64_t* tested, uint64_t* first) {
    if (!c || !mismatches || !tested || !first) return RTR_ERR_INVALID;
    if (n < 1 || n > (1ll << 30)) return fail(c, RTR_ERR_INVALID, "bad lane count");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    if ((rc = ensure(c, *t, 32))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, 32, stream));
    hipLaunchKernelGGL(k_test_draw_callers, grid_of(n), dim3(RTR_BLOCK), 0, stream, static_cast<unsigned long long*>(t->buf),
                       (unsigned long long)seed, (long long)n);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    unsigned long long h[4] = {0};
    TCHK(c, hipMemcpy(h, t->buf, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = h[0], *tested = h[1], *first = h[2];
    return RTR_OK;
}

int rtr_test_draw_host(const uint32_t* s, double* out, int64_t n) {
    if (n < 0 || (n > 0 && (!s || !out))) return RTR_ERR_INVALID;
    for (int64_t k = 0; k < n; ++k) out[k] = draw_sym_join(s[k]);
    return RTR_OK;
}

int rtr_test_draw_host_range(uint64_t first, uint64_t count, uint64_t stride, int32_t threads, uint64_t* mismatches, uint64_t* tested) {
    if (!mismatches || !tested || stride == 0 || threads < 1 || threads > 256) return RTR_ERR_INVALID;
    if (first >= (1ull << 32) || count > (1ull << 32) || (count && first + (count - 1) * stride >= (1ull << 32))) return RTR_ERR_INVALID;
    std::vector<uint64_t> bad((size_t)threads, 0), done((size_t)threads, 0);
    auto work = [&](int w) {
        const uint64_t k0 = count * (uint64_t)w / (uint64_t)threads, k1 = count * (uint64_t)(w + 1) / (uint64_t)threads;
        uint64_t b = 0;
        for (uint64_t k = k0; k < k1; ++k) {
            const uint32_t v = (uint32_t)(first + k * stride);
            const double y = draw_sym_join(v), y0 = draw_sym_plain(v);
            uint64_t by, by0;
            memcpy(&by, &y, 8), memcpy(&by0, &y0, 8);
            b += by != by0;
        }
        bad[(size_t)w] = b, done[(size_t)w] = k1 - k0;
    };
    std::vector<std::thread> pool;
    for (int w = 1; w < threads; ++w) pool.emplace_back(work, w);
    work(0);
    for (auto& th : pool) th.join();
    *mismatches = 0, *tested = 0;
    for (int w = 0; w < threads; ++w) *mismatches += bad[(size_t)w], *tested += done[(size_t)w];
    return RTR_OK;
}

int rtr_test_scene_consts(rtr_context* c, uint64_t* table, uint64_t* again, int64_t cap, int32_t* n_lights) {
    static_assert(sizeof(SceneConsts) == 32 && sizeof(LightConsts) == 40, "4 + 5 words per light");
    rtr_debug_view v;
    TestState* t;
    int rc = begin(c, nullptr, 0, 0, v, t);
    if (rc) return rc;
    if (!n_lights || cap < 0 || (cap > 0 && (!table || !again))) return fail(c, RTR_ERR_INVALID, "bad array");
    *n_lights = v.ds.n_lights;
    const size_t bytes = scene_consts_bytes(v.ds.n_lights);
    if ((size_t)cap * 8 < bytes) return cap == 0 ? RTR_OK : fail(c, RTR_ERR_INVALID, "table buffer too small");
    if (!v.ds.consts) return fail(c, RTR_ERR_DEVICE, "the uploaded scene has no table of constants");
    TCHK(c, hipSetDevice(v.device));
    if ((rc = ensure(c, *t, bytes))) return rc;
    TCHK(c, hipMemsetAsync(t->buf, 0, bytes, v.stream));
    hipLaunchKernelGGL(k_test_scene_consts, dim3(1), dim3(RTR_BLOCK), 0, v.stream, v.ds, static_cast<SceneConsts*>(t->buf));
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(v.stream));
    TCHK(c, hipMemcpy(again, t->buf, bytes, hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(table, v.ds.consts, bytes, hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* k_temporal_blend and k_temporal_store of the product on caller-given planes: the planes they touch in the test buffer,
 * the grids of denoise_run (rtr_image.hip) */
int rtr_test_temporal_planes(rtr_context* c, int32_t width, int32_t height, int32_t image_width, int32_t image_height, int32_t x0,
                             int32_t y0, const rtr_camera* cam, const rtr_camera* prev, int have, const rtr_temporal_params* tp,
                             const double* h_color, const double* h_q, const int32_t* h_count, const double* h_feat,
                             const double* h_hist_in, double* h_c, double* h_var, double* h_hist_out) {
    if (!c) return RTR_ERR_INVALID;
    if (!cam || !prev || !tp || !h_color || !h_q || !h_count || !h_feat || !h_hist_in || !h_c || !h_var || !h_hist_out)
        return fail(c, RTR_ERR_INVALID, "null argument");
    if (width < 1 || height < 1 || image_width < 2 || image_height < 2 || x0 < 0 || y0 < 0 || width > image_width - x0 ||
        height > image_height - y0 || (int64_t)image_width * image_height > ((int64_t)1 << 24))
        return fail(c, RTR_ERR_INVALID, "region outside the image, or image size out of range");
    if (!(tp->alpha_min > 0.0 && tp->alpha_min <= 1.0) || !(tp->tau_z > 0.0) || !(tp->tau_n > 0.0) ||
        !(tp->min_weight > 0.0 && tp->min_weight < 1.0))
        return fail(c, RTR_ERR_INVALID, "temporal parameter out of range");
    const size_t np = (size_t)width * height;
    for (size_t p = 0; p < np; ++p)
        if (h_count[p] < 0) return fail(c, RTR_ERR_INVALID, "negative sample count");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    /* doubles: m 3, q 1, feat 7, c[0] 3, v[0] 1, a 3, nrm 3, z 1, hist_in 10, hist_out 10, mom 3; then n (int) */
    const size_t n_doubles = (22 + 2 * RTR_HIST + 3) * np;
    if ((rc = ensure(c, *t, n_doubles * sizeof(double) + np * sizeof(int)))) return rc;
    double* d = static_cast<double*>(t->buf);
    DenoiseK D{};
    D.w = width, D.h = height;
    D.m = d, d += 3 * np;
    D.q = d, d += np;
    D.feat = d, d += RTR_FEAT * np;
    D.c[0] = d, d += 3 * np;
    D.v[0] = d, d += np;
    D.a = d, d += 3 * np;
    D.nrm = d, d += 3 * np;
    D.z = d, d += np;
    TemporalK T{};
    T.cam = *cam, T.prev = *prev;
    T.W = image_width, T.H = image_height, T.x0 = x0, T.y0 = y0;
    T.have = have ? 1 : 0;
    T.alpha_min = tp->alpha_min, T.tau_z = tp->tau_z, T.tau_n = tp->tau_n, T.min_weight = tp->min_weight;
    double* hist_in = d;
    T.hist_in = hist_in, d += RTR_HIST * np;
    T.hist_out = d, d += RTR_HIST * np;
    T.mom = d, d += 3 * np;
    D.n = reinterpret_cast<int*>(d);
    TCHK(c, hipMemcpy(D.m, h_color, 3 * np * sizeof(double), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(D.q, h_q, np * sizeof(double), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(D.n, h_count, np * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(D.feat, h_feat, RTR_FEAT * np * sizeof(double), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(hist_in, h_hist_in, RTR_HIST * np * sizeof(double), hipMemcpyHostToDevice));
    const dim3 grid1((unsigned)((np + RTR_BLOCK - 1) / RTR_BLOCK)), grid2((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
    hipLaunchKernelGGL(k_temporal_blend, grid2, dim3(RTR_BLOCK), 0, stream, D, T);
    hipLaunchKernelGGL(k_temporal_store, grid1, dim3(RTR_BLOCK), 0, stream, D, T);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    std::vector<double> cc(3 * np), vv(np);
    TCHK(c, hipMemcpy(cc.data(), D.c[0], 3 * np * sizeof(double), hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(vv.data(), D.v[0], np * sizeof(double), hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(h_hist_out, T.hist_out, RTR_HIST * np * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < np; ++p) {
        if (h_count[p] == 0) continue;
        for (int k = 0; k < 3; ++k) h_c[3 * p + k] = cc[p + k * np];
        h_var[p] = vv[p];
    }
    return RTR_OK;
}

int rtr_test_accum_load(rtr_context* c, rtr_accum* acc, const double* sum, const double* q, const int32_t* count, int64_t n) {
    return rtr_debug_accum_load(c, acc, sum, q, count, n);
}

/* k_accum_plan of the product on caller-given counts, errors and targets: the launch of accum_pass_plan (rtr_accum.hip) */
int rtr_test_accum_plan(rtr_context* c, int64_t n, int32_t mode, int32_t spp, int32_t spp_min, int32_t spp_max, double threshold,
                        const int32_t* count, const double* err, int32_t* tile_s1, int32_t* active, int32_t* n_active) {
    if (!c) return RTR_ERR_INVALID;
    if (!count || !err || !tile_s1 || !active || !n_active) return fail(c, RTR_ERR_INVALID, "null argument");
    if (n < 1 || n > ((int64_t)1 << 24)) return fail(c, RTR_ERR_INVALID, "need 1 <= n <= 2^24 tiles");
    if (mode < 0 || mode > 2) return fail(c, RTR_ERR_INVALID, "unknown plan mode");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    const size_t m = (size_t)n;
    if ((rc = ensure(c, *t, m * sizeof(double) + (3 * m + 1) * sizeof(int)))) return rc;
    double* d_err = static_cast<double*>(t->buf);
    int* d_count = reinterpret_cast<int*>(d_err + m);
    int* d_s1 = d_count + m;
    int* d_active = d_s1 + m;
    int* d_nactive = d_active + m;
    std::vector<int> minus(m + 1, -1); /* the slots of the list the kernel does not write stay -1 */
    TCHK(c, hipMemcpy(d_err, err, m * sizeof(double), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_count, count, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_s1, tile_s1, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_active, minus.data(), (m + 1) * sizeof(int), hipMemcpyHostToDevice));
    AccumPlanK K{};
    K.n_tiles = (int)n, K.mode = mode;
    K.count = d_count, K.err = d_err, K.tile_s1 = d_s1, K.active = d_active, K.n_active = d_nactive;
    K.spp = spp, K.spp_min = spp_min, K.spp_max = spp_max, K.threshold = threshold;
    hipLaunchKernelGGL(k_accum_plan, dim3(1), dim3(1024), 0, stream, K);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    TCHK(c, hipMemcpy(tile_s1, d_s1, m * sizeof(int), hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(active, d_active, m * sizeof(int), hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(n_active, d_nactive, sizeof(int), hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* k_accum_commit of the product over caller-given pass results: the launch of accum_pass_commit (rtr_accum.hip) */
int rtr_test_accum_commit(rtr_context* c, int64_t n, const int32_t* active, int32_t n_active, const int32_t* done,
                          const int32_t* tile_s1, const double* partial, const double* q_part, double* sum, double* q, int32_t* count) {
    if (!c) return RTR_ERR_INVALID;
    if (!active || !done || !tile_s1 || !partial || !sum || !count) return fail(c, RTR_ERR_INVALID, "null argument");
    if ((q == nullptr) != (q_part == nullptr)) return fail(c, RTR_ERR_INVALID, "q and q_part go together");
    if (n < 1 || n > ((int64_t)1 << 20)) return fail(c, RTR_ERR_INVALID, "need 1 <= n <= 2^20 tiles");
    if (n_active < 0 || n_active > n) return fail(c, RTR_ERR_INVALID, "need 0 <= n_active <= n");
    for (int64_t k = 0; k < n; ++k)
        if (active[k] < 0 || active[k] >= n) return fail(c, RTR_ERR_INVALID, "active slot out of range");
    hipStream_t stream;
    int n_cus;
    TestState* t;
    int rc = bare(c, stream, n_cus, t);
    if (rc) return rc;
    const size_t m = (size_t)n, ns = m * 3 * RTR_BLOCK, nq = m * RTR_BLOCK;
    if ((rc = ensure(c, *t, (2 * ns + 2 * nq) * sizeof(double) + (4 * m + 1) * sizeof(int)))) return rc;
    double* d_partial = static_cast<double*>(t->buf);
    double* d_qpart = d_partial + ns;
    double* d_sum = d_qpart + nq;
    double* d_q = d_sum + ns;
    int* d_active = reinterpret_cast<int*>(d_q + nq);
    int* d_done = d_active + m;
    int* d_s1 = d_done + m;
    int* d_count = d_s1 + m;
    int* d_nactive = d_count + m;
    TCHK(c, hipMemcpy(d_partial, partial, ns * sizeof(double), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_sum, sum, ns * sizeof(double), hipMemcpyHostToDevice));
    if (q) {
        TCHK(c, hipMemcpy(d_qpart, q_part, nq * sizeof(double), hipMemcpyHostToDevice));
        TCHK(c, hipMemcpy(d_q, q, nq * sizeof(double), hipMemcpyHostToDevice));
    }
    TCHK(c, hipMemcpy(d_active, active, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_done, done, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_s1, tile_s1, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_count, count, m * sizeof(int), hipMemcpyHostToDevice));
    TCHK(c, hipMemcpy(d_nactive, &n_active, sizeof(int), hipMemcpyHostToDevice));
    RenderK P{};
    P.n_tiles = (int)n, P.chunks = 1;
    P.partial = d_partial, P.q_part = q ? d_qpart : nullptr;
    P.done = d_done, P.tile_s1 = d_s1, P.active = d_active, P.n_active = d_nactive;
    hipLaunchKernelGGL(k_accum_commit, dim3((unsigned)n), dim3(RTR_BLOCK), 0, stream, P, d_sum, q ? d_q : nullptr, d_count);
    TCHK(c, hipGetLastError());
    TCHK(c, hipStreamSynchronize(stream));
    TCHK(c, hipMemcpy(sum, d_sum, ns * sizeof(double), hipMemcpyDeviceToHost));
    if (q) TCHK(c, hipMemcpy(q, d_q, nq * sizeof(double), hipMemcpyDeviceToHost));
    TCHK(c, hipMemcpy(count, d_count, m * sizeof(int), hipMemcpyDeviceToHost));
    return RTR_OK;
}

} /* extern "C" */
