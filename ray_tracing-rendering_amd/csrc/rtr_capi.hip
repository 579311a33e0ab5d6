/*
 * rtr_capi.hip -- the core of the C ABI (include/rtr_hip.h): context life cycle, scene validation and the copy of the
 * lowered scene (rt_lower.h: lower_scene) to the device, the render entries and render_core behind them, chunk planning,
 * statistics / cancel / synchronize, the camera, Integrator::Li of single samples (k_li), and the rtr_debug_* seam of the
 * test library.  Which kernel a call runs is rt_select.h's decision; the accumulator, image, query and gather entries
 * live in rtr_accum.hip, rtr_image.hip, rtr_query.hip and rtr_gather.hip and share the context through rt_context.h.
 */
#include "rt_context.h"
#include "rt_render_kernels.h"
#include "rt_validate.h"

#include <cstdio>
#include <cstring>

using namespace rtr;

static thread_local std::string g_create_error;

namespace rtr {

int fail(rtr_context* c, int code, const std::string& msg) {
    if (c)
        c->err = msg;
    else
        g_create_error = msg;
    return code;
}

int ensure(rtr_context* c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return RTR_OK;
    if (b.p) {
        HIPCHK(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, RTR_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    b.cap = bytes;
    return RTR_OK;
}

/* ensure() for a buffer that work queued without blocking may still read or write (b_denoise, an accumulator's d_feat:
 * the rtr_accum_*_device calls): the stream is waited for only when the buffer has to be replaced by a larger one */
int ensure_behind_queue(rtr_context* c, DevBuf& b, size_t bytes) {
    if (b.p && b.cap < std::max(bytes, (size_t)16)) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ensure(c, b, bytes);
}

int upload(rtr_context* c, DevBuf& b, const void* src, size_t bytes) {
    int rc = ensure(c, b, bytes);
    if (rc) return rc;
    if (bytes) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return RTR_OK;
}
/* rtr_upload_scene: one array to the device and its address into the DScene member that names it */
template <typename T>
int put(rtr_context* c, DevBuf& b, const T* src, size_t n, const T*& member) {
    const int rc = upload(c, b, src, sizeof(T) * n);
    member = static_cast<const T*>(b.p);
    return rc;
}
template <typename T>
int put(rtr_context* c, DevBuf& b, const std::vector<T>& src, const T*& member) {
    return put(c, b, src.data(), src.size(), member);
}

int params_check(rtr_context* c, const rtr_render_params* p) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null params");
    if (image_too_small(*p)) return fail(c, RTR_ERR_INVALID, "image smaller than 2x2");
    /* tile indices are int32 and the tile list is materialised: 2^26 tiles = 131 072 x 131 072 pixels, more
     * than a framebuffer in 288 GB of HBM holds */
    if (((int64_t)p->image_width + 15) / 16 * (((int64_t)p->image_height + 15) / 16) > ((int64_t)1 << 26))
        return fail(c, RTR_ERR_INVALID, "image larger than 2^26 tiles");
    if (region_outside(*p)) return fail(c, RTR_ERR_INVALID, "region outside the image or empty");
    if (p->spp < 1 || p->max_depth < 1 || p->rr_start_depth < 0)
        return fail(c, RTR_ERR_INVALID, "spp/max_depth/rr_start_depth out of range");
    if (p->integrator < RTR_INTEGRATOR_PATH || p->integrator > RTR_INTEGRATOR_MIS)
        return fail(c, RTR_ERR_UNSUPPORTED, "integrator id not supported (0 path, 1 RR, 2 PBR, 3 NEE, 4 MIS)");
    if (p->tile_stride > 1 && (p->tile_first < 0 || p->tile_first >= p->tile_stride))
        return fail(c, RTR_ERR_INVALID, "tile_first must be in [0, tile_stride)");
    if (p->spp_chunks < 0 || p->spp_chunks > p->spp) return fail(c, RTR_ERR_INVALID, "spp_chunks must be in [0, spp]");
    if (p->flags & ~(RTR_FLAG_REFERENCE_ORDER | RTR_FLAG_WF_PERSISTENT | RTR_FLAG_SORTED_SHADING | RTR_FLAG_SPLIT_CASTS | RTR_FLAG_STATIC_GRID)) return fail(c, RTR_ERR_INVALID, "unknown flag bits");
    if (p->pipeline < RTR_PIPELINE_AUTO || p->pipeline > RTR_PIPELINE_WAVEFRONT)
        return fail(c, RTR_ERR_INVALID, "unknown pipeline");
    return RTR_OK;
}

/* tiles this call owns, in the reference's dispatch order (renderer.h:40-62) */
std::vector<int> owned_tiles(const rtr_render_params& p, int& tiles_x, int& tiles_y) {
    tiles_x = (p.image_width + 15) / 16;
    tiles_y = (p.image_height + 15) / 16;
    const int stride = p.tile_stride > 1 ? p.tile_stride : 1;
    const int first = p.tile_stride > 1 ? p.tile_first : 0;
    std::vector<int> out;
    for (int t = first; t < tiles_x * tiles_y; t += stride) {
        int ty = (tiles_y - 1) - t / tiles_x, tx = t % tiles_x;
        int xs = tx * 16, ys = ty * 16;
        if (xs + 16 <= p.x0 || xs >= p.x1 || ys + 16 <= p.y0 || ys >= p.y1) continue;
        out.push_back(t);
    }
    return out;
}

int no_per_ray_kernel(rtr_context* c, int trav) {
    return fail(c, RTR_ERR_UNSUPPORTED, "no per-ray kernel for traversal " + std::to_string(trav));
}

int finish_stats(rtr_context* c) {
    if (!c->stats_pending) {
        if (c->in_flight) { /* a call that failed after its first stream-ordered step: wait for what it queued */
            c->in_flight = false;
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        return RTR_OK;
    }
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    unsigned long long h[RT_STATS_WORDS] = {0};
    HIPCHK(c, hipMemcpy(h, c->b_stats.p, sizeof h, hipMemcpyDeviceToHost));
    if (getenv("RTR_REGION_PROFILE")) { /* a -DRTR_REGION_PROFILE build filled these (rt_device.h: RT_REGION) */
        static const char* names[RG_N] = {"other / loop", "closest: instance setup", "closest: rect runs", "closest: sphere runs",
                                          "closest: generic scan", "closest: tree inner nodes", "closest: tree leaves",
                                          "closest: hit record (fast_finish)", "shadow: instance setup", "shadow: rect runs",
                                          "shadow: sphere runs", "shadow: generic scan", "shadow: tree inner nodes",
                                          "shadow: tree leaves", "media steps", "mat_prepare", "shade_a (emission, light sample)",
                                          "shade_b (BSDF sample, roulette)", "miss", "end of sample + regeneration",
                                          "shade_rr / shade_path", "park path state", "sorted shading: barrier waits",
                                          "sorted shading: tickets + exchange / queue: job switch", "pair cast: instance setup",
                                          "pair cast: rect runs", "pair cast: sphere runs", "sample end: cancel poll",
                                          "sample end: begin_sample (camera ray)", "sample end: settle into the pixel sum",
                                          "cast counters", "random_in_unit_sphere rejection loop",
                                          "shade_a: emitter MIS weight (compute_light_pdf)", "camera_sample: image-size divisions",
                                          "shading: lane-varying 1 / x and n / d", "shading: lane-varying sqrt",
                                          "pair cast: recast through the single casts"};
        double total = 0;
        for (int k = 0; k < RG_N; ++k) total += (double)h[RT_PROF_BASE + k];
        std::fprintf(stderr, "[region profile] %.4g wave cycles in all, %llu samples\n", total, h[0]);
        for (int k = 0; k < RG_N; ++k)
            if (h[RT_PROF_BASE + RT_PROF_REGIONS + k])
                std::fprintf(stderr, "[region profile] %-48s %6.2f %%  %12llu visits  %8.1f cycles/visit\n", names[k],
                             100.0 * (double)h[RT_PROF_BASE + k] / total, h[RT_PROF_BASE + RT_PROF_REGIONS + k],
                             (double)h[RT_PROF_BASE + k] / (double)h[RT_PROF_BASE + RT_PROF_REGIONS + k]);
    }
#ifdef RTR_PHASE_CLOCKS
    std::fprintf(stderr, "[phase clocks] closest %.3e  shade %.3e  shadow %.3e  other %.3e (wave cycles)\n", (double)h[3],
                 (double)h[4], (double)h[5], (double)h[6]);
#endif
    c->stats.samples = h[0];
    c->stats.closest_segments = h[1];
    c->stats.shadow_segments = h[2];
    c->stats.device_ms = ms;
    if (h[7]) c->stats.cancelled = 1; /* workgroups that saw the cancel before their last sample */
    c->stats_pending = false;
    c->in_flight = false;
    return RTR_OK;
}

int nothing_to_render(rtr_context* c) {
    if (int rc = finish_stats(c)) return rc;
    c->stats = rtr_render_stats{};
    return RTR_OK;
}

/* one call into the integrator group's unit: prepares the kernel of L (MegaLaunch::prepare) or launches it */
static int run_mega(rtr_context* c, MegaLaunch& L) {
    switch (L.variant.integ) {
    case RTR_INTEGRATOR_MIS: return rtr_mega_launch_mis(L, c->err);
    case RTR_INTEGRATOR_RR:
    case RTR_INTEGRATOR_PATH: return rtr_mega_launch_rr_path(L, c->err);
    default: return rtr_mega_launch_pbr_nee(L, c->err);
    }
}
/* The kernel of L prepared for P (whose chunk count decides L.queue with the variant): the one LDS check, attribute and
 * occupancy query of a render.  Auto chunking needs the occupancy, and so does the grid of a queue launch. */
static int prepare_mega(rtr_context* c, MegaLaunch& L, const RenderK& P, int flags, bool auto_chunks) {
    L.queue = mega_queue(L.variant, P, flags);
    L.prepare = true, L.occupancy = auto_chunks || L.queue;
    const int rc = run_mega(c, L);
    L.prepare = false;
    return rc;
}

/* spp_chunks = 0: the library's choice for this scene, pipeline and number of owned tiles.  L: the plan of a megakernel
 * render (null: wavefront), left prepared for the kernel a render in one chunk runs */
static int auto_chunking(rtr_context* c, RenderK P, MegaLaunch* L, int pipeline, int spp, int flags, int* chunks, int* guided) {
    int per_cu = 4;
    P.chunks = 1;
    if (L) {
        if (int rc = prepare_mega(c, *L, P, flags, true)) return rc;
        per_cu = L->per_cu;
    }
    choose_chunks(pipeline, (double)c->n_cus * (per_cu > 0 ? per_cu : 1), P.n_tiles, spp, chunks, guided);
    return RTR_OK;
}

/* the render call proper; tile_done != nullptr: packed output (see ResolveK).
 * acc != nullptr: a pass of that accumulator (p->spp_chunks = 1): its tile list, its counts as start samples and its
 * sums (and moments) as start values; `plan` (mode, targets, refinement bounds) says how k_accum_plan sets each tile's
 * end sample and the active list before the megakernel, k_accum_errors runs first for a refinement, and the commit
 * kernel takes the place of k_resolve */
int render_core(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, unsigned char* tile_done, int blocking,
                rtr_accum* acc, const AccumPlanK* plan) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call (ours or the host framework's) is not this call's */
    int rc = RTR_OK;

    RenderK P{};
    P.W = p->image_width, P.H = p->image_height;
    P.x0 = p->x0, P.y0 = p->y0, P.x1 = p->x1, P.y1 = p->y1;
    P.spp = p->spp, P.max_depth = p->max_depth, P.rr_start = p->rr_start_depth;
    P.seed = p->seed;
    P.integrator = p->integrator;
    std::vector<int> tiles;
    if (acc)
        P.tiles_x = acc->tiles_x, P.tiles_y = acc->tiles_y;
    else
        tiles = owned_tiles(*p, P.tiles_x, P.tiles_y);
    P.n_tiles = (int)(acc ? acc->tiles.size() : tiles.size());
    if (P.n_tiles == 0) { /* nothing to do: this call's statistics are all zero (an earlier render's are dropped) */
        if ((rc = nothing_to_render(c))) return rc;
        c->last_kernel = rtr_debug_kernel{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
        return RTR_OK;
    }

    int pipeline = p->pipeline;
    if (pipeline == RTR_PIPELINE_AUTO) pipeline = RTR_PIPELINE_MEGAKERNEL;
    const bool mega = pipeline == RTR_PIPELINE_MEGAKERNEL;
    const int trav = pick_trav(c->facts, c->info, p->flags);
    /* which kernels, decided once (rt_select.h) */
    MegaLaunch L{};
    WavefrontPlan wf{};
    if (mega)
        L = mega_plan(c->facts, c->info, p->integrator, trav, p->flags, acc ? (acc->moments ? 2 : 1) : 0, c->n_cus);
    else if ((rc = wavefront_plan(c->facts, c->info, trav, p->flags, c->ds.n_lights > 0, c->n_cus, wf, c->err)))
        return rc;
    int chunks = p->spp_chunks, guided[3] = {0, 0, 0};
    if (chunks == 0 && (rc = auto_chunking(c, P, mega ? &L : nullptr, pipeline, p->spp, p->flags, &chunks, guided))) return rc;
    P.n_big = guided[0], P.big_spp = guided[1], P.small_spp = guided[2];
    P.chunks = chunks;

    /* A render that was queued without blocking may still be running.  Everything below is ordered behind
     * it on the stream, so the host only has to wait where it would touch memory that render still reads:
     * another tile list, larger workspace buffers, the wavefront pool.  Back-to-back renders of the same
     * shape (bench.py's steps) then queue up without a bubble between them; the statistics of a render nobody
     * asked for are dropped. */
    const size_t partial_bytes = (size_t)P.n_tiles * chunks * 3 * RTR_BLOCK * sizeof(double);
    const size_t done_bytes = ((size_t)P.n_tiles * chunks + 1) * sizeof(int); /* + the block counter of a queue render */
    const bool same_tiles = acc || tiles == c->last_tiles; /* (an accumulator's tile list is its own) */
    if ((c->stats_pending || c->in_flight) && (!same_tiles || partial_bytes > c->b_partial.cap || done_bytes > c->b_done.cap ||
                                               pipeline == RTR_PIPELINE_WAVEFRONT)) {
        if ((rc = finish_stats(c))) return rc;
    }
    /* everything that can fail comes before the first stream-ordered side effect, so an error return leaves
     * a render that is still in flight (and its pending statistics) alone */
    if (!same_tiles) {
        c->last_tiles.clear();
        if ((rc = upload(c, c->b_tiles, tiles.data(), tiles.size() * sizeof(int)))) return rc;
        c->last_tiles = tiles;
    }
    if ((rc = ensure(c, c->b_partial, partial_bytes))) return rc;
    if ((rc = ensure(c, c->b_done, done_bytes))) return rc;
    P.tile_ids = static_cast<const int*>(acc ? acc->d_tiles.p : c->b_tiles.p);
    if (acc) {
        P.tile_s0 = static_cast<const int*>(acc->d_count.p);
        P.acc_in = static_cast<const double*>(acc->d_sum.p);
        P.tile_s1 = static_cast<const int*>(acc->d_s1.p);
        P.active = static_cast<const int*>(acc->d_active.p);
        P.n_active = static_cast<const int*>(acc->d_nactive.p);
        if (acc->moments) {
            P.q_in = static_cast<const double*>(acc->d_q.p);
            P.q_part = static_cast<double*>(acc->d_qpart.p);
        }
    }
    P.stats = static_cast<unsigned long long*>(c->b_stats.p);
    P.cancel = static_cast<const uint32_t*>(c->b_cancel.p);
    P.partial = static_cast<double*>(c->b_partial.p);
    P.done = static_cast<int*>(c->b_done.p);
    /* the chunking has prepared the kernel -- unless the chunk count was given, or one so large came out of it that the
     * 2^31 blocks of mega_queue move the launch off the queue */
    if (mega && !(p->spp_chunks == 0 && L.queue == mega_queue(L.variant, P, p->flags)) && (rc = prepare_mega(c, L, P, p->flags, false)))
        return rc;

    const uint32_t id = c->render_seq.fetch_add(1) + 1; /* rtr_cancel() from now on covers this render */
    P.render_id = id;
    c->stats_pending = false; /* an unfinished earlier render's statistics are dropped here */
    c->in_flight = true;      /* ... but what it queued, and what this call queues from here on, is still tracked: an error
                                 return below leaves it set, and the next call (or rtr_get_stats) waits before it touches
                                 the tile list, the workspace or the wavefront pool */
    c->stats = rtr_render_stats{};
    c->stats.spp_chunks = chunks;
    c->last_kernel = rtr_debug_kernel{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
    c->pending_id = id;
    HIPCHK(c, hipMemsetAsync(c->b_stats.p, 0, RT_STATS_WORDS * sizeof(unsigned long long), c->stream));
    if (c->camera_dirty) { /* rtr_set_camera: behind every render queued with the old camera, in front of this one */
        hipLaunchKernelGGL(k_camera_store, dim3(1), dim3(64), 0, c->stream, static_cast<DScene*>(c->sb.dscene.p), c->ds.camera);
        HIPCHK(c, hipGetLastError());
        c->camera_dirty = false;
    }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (!mega) {
        int launches = 0;
        LaunchedKernel launched{};
        if (wf.machine) c->stats.flags_in_effect |= RTR_FLAG_WF_PERSISTENT;
        rc = wavefront_render(c->pool, static_cast<const DScene*>(c->sb.dscene.p), wf, P, p->integrator, d_rgb, row_stride,
                              tile_done, c->stream, &c->cancelled_upto, &launches, &launched, c->err);
        c->last_kernel = rtr_debug_kernel{pipeline, p->integrator, launched.trav, launched.ms, launched.sorted, launched.phases,
                                          wf.lean, wf.quadlit, wf.sort, wf.media, wf.machine};
        if (rc && rc != RTR_ERR_CANCELLED) return rc;
        if (rc == RTR_ERR_CANCELLED) c->stats.cancelled = 1;
        c->stats.kernel_launches = launches;
    } else {
        int launches = 2;
        if (acc) { /* the pass's plan, on the device: no host round trip between a refinement's decision and its pass */
            accum_pass_plan(acc, plan, P.n_tiles, c->stream, &launches);
            HIPCHK(c, hipGetLastError());
        }
        if (L.queue) /* the jobs count themselves in the completion words, and the waves pull blocks through the counter behind them */
            HIPCHK(c, hipMemsetAsync(c->b_done.p, 0, done_bytes, c->stream));
        L.stream = c->stream, L.dsc = static_cast<const DScene*>(c->sb.dscene.p), L.P = P;
        c->stats.flags_in_effect |= L.flags_in_effect;
        if ((rc = run_mega(c, L))) return rc;
        const MegaVariant& v = L.variant;
        c->last_kernel = rtr_debug_kernel{pipeline, p->integrator, v.trav, v.ms, v.sorted, 0, 0, 0, 0, 0, 0, L.accum, v.pair, L.queue};
        if (acc) {
            accum_pass_commit(acc, P, c->stream);
        } else {
            ResolveK R{P, d_rgb, (long long)row_stride, tile_done, L.queue ? RTR_BLOCK : 0};
            rtr_launch_resolve(R, c->stream);
        }
        HIPCHK(c, hipGetLastError());
        c->stats.kernel_launches = launches;
    }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->stats.pipeline = pipeline;
    c->stats_pending = true;
    if (blocking || c->stats.cancelled) { /* the host-driven wavefront loop has already waited */
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = finish_stats(c))) return rc;
        if (c->stats.cancelled) return fail(c, RTR_ERR_CANCELLED, "render cancelled");
    }
    return RTR_OK;
}

} // namespace rtr

void rtr_launch_resolve(const ResolveK& R, hipStream_t stream) {
    hipLaunchKernelGGL(k_resolve, dim3((unsigned)R.r.n_tiles), dim3(RTR_BLOCK), 0, stream, R);
}

extern "C" {

uint32_t rtr_abi_version(void) { return RTR_ABI_VERSION; }

int rtr_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return RTR_ERR_DEVICE;
    return n;
}

uint32_t rtr_sample_seed(uint32_t seed, int32_t image_width, int32_t i, int32_t j, int32_t s) {
    return rtr_sample_seed_inline(seed, image_width, i, j, s);
}

int rtr_validate_scene(const rtr_scene_desc* scene, rtr_scene_info* info, char* msg, size_t msg_cap) {
    Validator v;
    v.s = scene;
    int rc = v.run(info);
    if (msg && msg_cap) {
        std::snprintf(msg, msg_cap, "%s", v.msg.c_str());
    }
    if (rc == RTR_OK && info) rtc::compile_validated(scene, *info);
    return rc;
}

int rtr_create(int device_ordinal, rtr_context** out_ctx) {
    if (!out_ctx) return fail(nullptr, RTR_ERR_INVALID, "null out_ctx");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, RTR_ERR_DEVICE,
                    std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "count is 0"));
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, RTR_ERR_INVALID, "device ordinal out of range");
    rtr_context* c = new rtr_context();
    c->device = device_ordinal;
#define CREATE_CHK(expr)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            g_create_error = std::string(#expr) + ": " + hipGetErrorString(e_);              \
            delete c;                                                                        \
            return RTR_ERR_DEVICE;                                                           \
        }                                                                                    \
    } while (0)
    CREATE_CHK(hipSetDevice(device_ordinal));
    {
        hipDeviceProp_t prop;
        CREATE_CHK(hipGetDeviceProperties(&prop, device_ordinal));
        c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    CREATE_CHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    CREATE_CHK(hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    CREATE_CHK(hipEventCreate(&c->ev0));
    CREATE_CHK(hipEventCreate(&c->ev1));
#undef CREATE_CHK
    c->stream = c->own_stream;
    int rc = ensure(c, c->b_stats, RT_STATS_WORDS * sizeof(unsigned long long));
    if (!rc) rc = ensure(c, c->b_cancel, sizeof(uint32_t));
    if (!rc && hipMemset(c->b_cancel.p, 0, sizeof(uint32_t)) != hipSuccess) rc = RTR_ERR_DEVICE;
    if (!rc) rc = display_create(c);
    if (rc) {
        g_create_error = c->err;
        rtr_destroy(c);
        return rc;
    }
    *out_ctx = c;
    return RTR_OK;
}

void rtr_destroy(rtr_context* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (rtr_accum* a : c->accums) free_accum(a);
    c->accums.clear();
    for (rtr_history* h : c->histories) free_history(h);
    c->histories.clear();
    for (DevBuf& b : c->sb)
        if (b.p) hipFree(b.p);
    DevBuf* bufs[] = {&c->b_tiles, &c->b_partial, &c->b_done, &c->b_stats, &c->b_cancel, &c->b_test, &c->b_stage, &c->b_denoise,
                      &c->b_batch, &c->b_display, &c->b_display_io};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    c->pool.release();
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    if (c->side_stream) hipStreamDestroy(c->side_stream);
    delete c;
}

int rtr_set_stream(rtr_context* c, void* hip_stream) {
    if (!c) return RTR_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return RTR_OK;
}

/* the scene's table of shading constants (rt_device.h: SceneConsts): one workgroup, a lane per light */
__global__ void __launch_bounds__(RTR_BLOCK) k_scene_consts(const rtr_light* __restrict__ lights, const int n_lights,
                                                            SceneConsts* __restrict__ out) {
    for (int k = threadIdx.x; k < (n_lights > 1 ? n_lights : 1); k += RTR_BLOCK) scene_consts_fill(lights, n_lights, out, k);
}

int rtr_upload_scene(rtr_context* c, const rtr_scene_desc* s) {
    if (!c) return RTR_ERR_INVALID;
    Validator v;
    v.s = s;
    rtr_scene_info info{};
    int rc = v.run(&info);
    if (rc) return fail(c, rc, "scene rejected: " + v.msg);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->has_scene = false;
    ++c->scene_gen;
    const LoweredScene L = lower_scene(s, info);
    const CompiledScene& cs = L.cs;
    SceneBufs& b = c->sb;
    DScene& d = c->ds = L.ds; /* the members that are no pointers; one line per array below */
    if ((rc = put(c, b.nodes, cs.dev_nodes, d.nodes))) return rc;
    if ((rc = put(c, b.kids, s->list_children, s->n_list_children, d.list_children))) return rc;
    if ((rc = put(c, b.mats, s->materials, s->n_materials, d.materials))) return rc;
    if ((rc = put(c, b.tex, s->textures, s->n_textures, d.textures))) return rc;
    if ((rc = put(c, b.perlin, s->perlin, s->n_perlin, d.perlin))) return rc;
    if ((rc = put(c, b.images, s->images, s->n_images, d.images))) return rc;
    if ((rc = put(c, b.imgbytes, s->image_bytes, s->n_image_bytes, d.image_bytes))) return rc;
    if ((rc = put(c, b.lights, s->lights, s->n_lights, d.lights))) return rc;
    if ((rc = put(c, b.finst, cs.inst, d.finst))) return rc;
    if ((rc = put(c, b.fxf, cs.xf, d.fxf))) return rc;
    if ((rc = put(c, b.fref, cs.ref, d.fref))) return rc;
    if ((rc = put(c, b.fexit, cs.exits, d.fexit))) return rc;
    if ((rc = put(c, b.fbvh, cs.bvh, d.fbvh))) return rc;
    if ((rc = put(c, b.fsub, cs.subs, d.fsub))) return rc;
    if ((rc = put(c, b.fscan, cs.scan, d.fscan))) return rc;
    if ((rc = put(c, b.fguard, cs.guards, d.fguard))) return rc;
    if ((rc = put(c, b.fstep, L.steps, d.fstep))) return rc;
    if ((rc = put(c, b.fvisit, L.visits, d.fvisit))) return rc;
    if ((rc = put(c, b.fprim, L.prims, d.fprim))) return rc;
    if ((rc = put(c, b.fleaf, L.leaves, d.fleaf))) return rc;
    if ((rc = put(c, b.fmat, L.mats, d.fmat))) return rc;
    if ((rc = put(c, b.ffin, L.finish, d.ffin))) return rc;
    if (L.finish.empty()) d.ffin = nullptr; /* (an earlier scene's buffer may still be there: null means "no records") */
    /* the lights are on the device (blocking copies): their table is made there, and is there when this call returns.
     * Nothing else changes lights, so nothing else makes it */
    if ((rc = ensure(c, b.sconsts, scene_consts_bytes(s->n_lights)))) return rc;
    d.consts = static_cast<const SceneConsts*>(b.sconsts.p);
    hipLaunchKernelGGL(k_scene_consts, dim3(1), dim3(RTR_BLOCK), 0, c->stream, d.lights, (int)s->n_lights,
                       static_cast<SceneConsts*>(b.sconsts.p));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = upload(c, b.dscene, &d, sizeof(DScene)))) return rc;
    c->info = info;
    c->facts = L.facts;
    c->camera_dirty = false;
    c->has_scene = true;
    return RTR_OK;
}

int rtr_render_device(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_render before rtr_upload_scene");
    if (int prc = params_check(c, p)) return prc;
    if (!d_rgb || row_stride < (int64_t)(p->x1 - p->x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    return render_core(c, p, d_rgb, row_stride, nullptr, blocking);
}

int rtr_render_host(rtr_context* c, const rtr_render_params* p, double* h_rgb, int64_t row_stride) {
    if (!c) return RTR_ERR_INVALID;
    if (int prc = params_check(c, p)) return prc;
    if (!h_rgb || row_stride < (int64_t)(p->x1 - p->x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    HIPCHK(c, hipSetDevice(c->device));
    const int w = p->x1 - p->x0, h = p->y1 - p->y0;
    const size_t bytes = (size_t)w * h * 3 * sizeof(double);
    /* staging framebuffer kept across calls (a progressive host render calls once per band); a render
     * still queued on the stream may be writing it */
    if (bytes > c->b_stage.cap) HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = ensure(c, c->b_stage, bytes);
    if (rc) return rc;
    void* d = c->b_stage.p;
    /* pixels of tiles this call does not own (or does not finish: cancel) keep the caller's values */
    hipError_t ce = hipMemcpy2DAsync(d, (size_t)w * 3 * sizeof(double), h_rgb, (size_t)row_stride * 3 * sizeof(double),
                                     (size_t)w * 3 * sizeof(double), h, hipMemcpyHostToDevice, c->stream);
    rc = ce == hipSuccess ? rtr_render_device(c, p, static_cast<double*>(d), w, 1)
                          : fail(c, RTR_ERR_DEVICE, hipGetErrorString(ce));
    if (rc == RTR_OK || rc == RTR_ERR_CANCELLED) {
        hipError_t e2 = hipMemcpy2D(h_rgb, (size_t)row_stride * 3 * sizeof(double), d, (size_t)w * 3 * sizeof(double),
                                    (size_t)w * 3 * sizeof(double), h, hipMemcpyDeviceToHost);
        if (e2 != hipSuccess) rc = fail(c, RTR_ERR_DEVICE, hipGetErrorString(e2));
    }
    return rc;
}

int rtr_render_tiles_host(rtr_context* c, const rtr_render_params* p, const double** tiles, const int32_t** tile_ids,
                          const uint8_t** tile_done, int64_t* n_tiles) {
    if (!c) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_render before rtr_upload_scene");
    if (int prc = params_check(c, p)) return prc;
    if (!tiles || !tile_ids || !tile_done || !n_tiles) return fail(c, RTR_ERR_INVALID, "null output pointer");
    HIPCHK(c, hipSetDevice(c->device));
    int tx, ty;
    const std::vector<int> owned = owned_tiles(*p, tx, ty);
    const size_t n = owned.size();
    /* [pixels: n x 768 doubles][done: n bytes, padded][ids: n int32] -- on the device and, pinned, on the host */
    const size_t px_bytes = n * 768 * sizeof(double), done_bytes = (n + 15) & ~(size_t)15, id_bytes = n * sizeof(int32_t);
    const size_t total = px_bytes + done_bytes + id_bytes + 16;
    if (total > c->b_stage.cap || total > c->h_stage_cap) HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = ensure(c, c->b_stage, total);
    if (rc) return rc;
    if (total > c->h_stage_cap) {
        if (c->h_stage) HIPCHK(c, hipHostFree(c->h_stage));
        c->h_stage = nullptr, c->h_stage_cap = 0;
        if (hipHostMalloc(&c->h_stage, total, hipHostMallocDefault) != hipSuccess)
            return fail(c, RTR_ERR_NOMEM, "hipHostMalloc of the tile staging buffer");
        c->h_stage_cap = total;
    }
    char* d = static_cast<char*>(c->b_stage.p);
    char* h = static_cast<char*>(c->h_stage);
    *n_tiles = (int64_t)n;
    *tiles = reinterpret_cast<const double*>(h);
    *tile_done = reinterpret_cast<const uint8_t*>(h + px_bytes);
    *tile_ids = reinterpret_cast<const int32_t*>(h + px_bytes + done_bytes);
    if (n == 0) return RTR_OK;
    std::memcpy(h + px_bytes + done_bytes, owned.data(), id_bytes);
    HIPCHK(c, hipMemsetAsync(d + px_bytes, 0, done_bytes, c->stream));
    rc = render_core(c, p, reinterpret_cast<double*>(d), -1, reinterpret_cast<unsigned char*>(d + px_bytes), 0);
    if (rc && rc != RTR_ERR_CANCELLED) return rc;
    /* one D2H of the owned tiles and their flags into pinned memory */
    HIPCHK(c, hipMemcpyAsync(h, d, px_bytes + done_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int frc = finish_stats(c)) return frc;
    if (c->stats.cancelled) return fail(c, RTR_ERR_CANCELLED, "render cancelled");
    return RTR_OK;
}

int rtr_plan_chunks(rtr_context* c, const rtr_render_params* p) {
    if (!c) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_plan_chunks before rtr_upload_scene");
    if (int prc = params_check(c, p)) return prc;
    if (p->spp_chunks > 0) return p->spp_chunks;
    HIPCHK(c, hipSetDevice(c->device));
    RenderK P{};
    rtr_render_params q = *p;
    P.n_tiles = (int)owned_tiles(q, P.tiles_x, P.tiles_y).size();
    if (P.n_tiles == 0) return 1;
    const int pipeline = p->pipeline == RTR_PIPELINE_AUTO ? RTR_PIPELINE_MEGAKERNEL : p->pipeline;
    const bool mega = pipeline == RTR_PIPELINE_MEGAKERNEL;
    MegaLaunch L{};
    if (mega) L = mega_plan(c->facts, c->info, p->integrator, pick_trav(c->facts, c->info, p->flags), p->flags, 0, c->n_cus);
    int chunks = 1, guided[3];
    if (int rc = auto_chunking(c, P, mega ? &L : nullptr, pipeline, p->spp, p->flags, &chunks, guided)) return rc;
    return chunks;
}

int rtr_synchronize(rtr_context* c) {
    if (!c) return RTR_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
}

int rtr_cancel(rtr_context* c) {
    if (!c) return RTR_ERR_INVALID;
    std::lock_guard<std::mutex> lk(c->cancel_mu);
    /* static: the copy may still read the word after this function has returned an error */
    static thread_local uint32_t upto;
    upto = c->render_seq.load();
    if (upto == 0 || upto == c->cancelled_upto.load()) return RTR_OK; /* nothing issued since the last cancel */
    c->cancelled_upto.store(upto);
    hipSetDevice(c->device);
    hipError_t e = hipMemcpyAsync(c->b_cancel.p, &upto, sizeof(uint32_t), hipMemcpyHostToDevice, c->side_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->side_stream);
    return e == hipSuccess ? RTR_OK : RTR_ERR_DEVICE;
}

int rtr_get_stats(rtr_context* c, rtr_render_stats* out) {
    if (!c || !out) return RTR_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = finish_stats(c);
    if (rc) return rc;
    *out = c->stats;
    return RTR_OK;
}

const char* rtr_last_error(const rtr_context* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

/* ---- per-ray entry: Integrator::Li of camera samples or caller-given rays ------------------------------------ */
static int li_run(rtr_context* c, const rtr_render_params* p, const int32_t* ijs, const rtr_li_ray* rays, LiOut* host_out,
                  int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_li_* before rtr_upload_scene");
    if (int prc = params_check(c, p)) return prc;
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t in_bytes = rays ? (size_t)n * sizeof(rtr_li_ray) : (size_t)n * 3 * sizeof(int32_t);
    const size_t in_pad = (in_bytes + 15) & ~(size_t)15;
    int rc = ensure(c, c->b_test, in_pad + (size_t)n * sizeof(LiOut));
    if (rc) return rc;
    char* base = static_cast<char*>(c->b_test.p);
    HIPCHK(c, hipMemcpy(base, rays ? (const void*)rays : (const void*)ijs, in_bytes, hipMemcpyHostToDevice));
    RenderK P{};
    P.W = p->image_width, P.H = p->image_height;
    P.spp = p->spp, P.max_depth = p->max_depth, P.rr_start = p->rr_start_depth;
    P.seed = p->seed;
    const int32_t* d_ijs = rays ? nullptr : reinterpret_cast<const int32_t*>(base);
    const rtr_li_ray* d_rays = rays ? reinterpret_cast<const rtr_li_ray*>(base) : nullptr;
    LiOut* d_out = reinterpret_cast<LiOut*>(base + in_pad);
    const int per_ray = per_ray_trav(c->facts, c->info, p->flags, false), trav = li_trav(p->integrator, per_ray);
    const size_t lds = stack_bytes(c->facts, c->info, per_ray);
    const dim3 grid((unsigned)((n + RTR_BLOCK - 1) / RTR_BLOCK));
    const bool found = dispatch_li(p->integrator, trav, [&](auto integ, auto t) {
        constexpr int I = decltype(integ)::value, T = decltype(t)::value;
        if ((rc = set_lds(c, k_li<I, T>, lds))) return;
        hipLaunchKernelGGL((k_li<I, T>), grid, dim3(RTR_BLOCK), lds, c->stream, c->ds, P, d_ijs, d_rays, d_out, (long long)n);
    });
    if (!found) return no_per_ray_kernel(c, trav);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host_out, d_out, (size_t)n * sizeof(LiOut), hipMemcpyDeviceToHost));
    return RTR_OK;
}

int rtr_li_samples(rtr_context* c, const rtr_render_params* p, const int32_t* ijs, double* L, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (n < 0 || (n > 0 && (!ijs || !L))) return fail(c, RTR_ERR_INVALID, "bad sample / radiance arrays");
    if (int prc = params_check(c, p)) return prc;
    for (int64_t k = 0; k < n; ++k)
        if (ijs[3 * k] < 0 || ijs[3 * k] >= p->image_width || ijs[3 * k + 1] < 0 || ijs[3 * k + 1] >= p->image_height ||
            ijs[3 * k + 2] < 0)
            return fail(c, RTR_ERR_INVALID, "sample outside the image");
    std::vector<LiOut> out((size_t)n);
    int rc = li_run(c, p, ijs, nullptr, out.data(), n);
    if (rc) return rc;
    for (int64_t k = 0; k < n; ++k)
        for (int q = 0; q < 3; ++q) L[3 * k + q] = out[(size_t)k].L[q];
    return RTR_OK;
}

int rtr_li_rays(rtr_context* c, const rtr_render_params* p, const rtr_li_ray* rays, double* L, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (n < 0 || (n > 0 && (!rays || !L))) return fail(c, RTR_ERR_INVALID, "bad ray / radiance arrays");
    for (int64_t k = 0; k < n; ++k)
        if (rays[k].rng_state == 0) return fail(c, RTR_ERR_INVALID, "a xorshift32 state must not be 0 (rtweekend.h:24-34)");
    std::vector<LiOut> out((size_t)n);
    int rc = li_run(c, p, nullptr, rays, out.data(), n);
    if (rc) return rc;
    for (int64_t k = 0; k < n; ++k)
        for (int q = 0; q < 3; ++q) L[3 * k + q] = out[(size_t)k].L[q];
    return RTR_OK;
}

int rtr_set_camera(rtr_context* c, const rtr_camera* cam) {
    if (!c) return RTR_ERR_INVALID;
    if (!cam) return fail(c, RTR_ERR_INVALID, "null camera");
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_set_camera before rtr_upload_scene");
    static_assert(sizeof(rtr_camera) == 24 * sizeof(double), "rtr_camera is 24 doubles");
    double v[24];
    std::memcpy(v, cam, sizeof v);
    for (double x : v)
        if (!std::isfinite(x)) return fail(c, RTR_ERR_INVALID, "non-finite camera member");
    /* what rtr_upload_scene derived from the old camera: the boxes of moving spheres cover the ray times [t_lo, t_hi],
     * and DScene::shared_div asked for |time| <= 2^60 */
    for (double t : {cam->time0, cam->time1})
        if (t < c->facts.t_lo || t > c->facts.t_hi)
            return fail(c, RTR_ERR_UNSUPPORTED, "camera time " + std::to_string(t) + " outside the range [" + std::to_string(c->facts.t_lo) +
                                                    ", " + std::to_string(c->facts.t_hi) + "] the scene was compiled for: upload the scene "
                                                    "with this camera (rtr_upload_scene)");
    if ((std::fabs(cam->time0) <= 0x1p60 && std::fabs(cam->time1) <= 0x1p60) != c->facts.camera_times_small)
        return fail(c, RTR_ERR_UNSUPPORTED, "camera times cross the 2^60 bound of the shared divisions: upload the scene with "
                                            "this camera (rtr_upload_scene)");
    c->ds.camera = *cam;
    c->camera_dirty = true;
    ++c->camera_gen;
    return RTR_OK;
}

int rtr_get_camera(rtr_context* c, rtr_camera* out) {
    if (!c) return RTR_ERR_INVALID;
    if (!out) return fail(c, RTR_ERR_INVALID, "null out");
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_get_camera before rtr_upload_scene");
    *out = c->ds.camera;
    return RTR_OK;
}

/* ---- the seam librtr_hip_test.so reaches the context through (csrc/rt_debug.h; not part of include/) ------------- */
int rtr_debug_view_get(rtr_context* c, int flags, rtr_debug_view* v, size_t size) {
    if (!c || !v || size != sizeof(rtr_debug_view)) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_test_* before rtr_upload_scene");
    v->ds = c->ds;
    v->stream = c->stream;
    v->device = c->device;
    v->n_cus = c->n_cus;
    v->n_materials = c->facts.n_materials;
    v->trav = per_ray_trav(c->facts, c->info, flags, true); /* the unit kernels walk what the megakernel walks */
    v->stack_bytes = stack_bytes(c->facts, c->info, v->trav);
    /* mega_variant's choice for MIS / RR where that is a flat kernel */
    const int mega = mega_variant(c->facts, RTR_INTEGRATOR_MIS, pick_trav(c->facts, c->info, flags), flags, nullptr).trav;
    v->flat_trav = mega == RT_TRAV_FLAT || mega == RT_TRAV_FLAT_GUARD ? mega : -1;
    v->lean_ok = c->facts.lean_materials;
    v->quadlit_ok = c->facts.quad_lights_only && !c->facts.needs_uv;
    return RTR_OK;
}
int rtr_debug_scene_plan(const rtr_scene_desc* s, int integrator, int flags, rtr_debug_plan* out, size_t size, int32_t* ref_flags,
                         int64_t cap, void* finish, int64_t finish_cap) {
    if (!out || size != sizeof(rtr_debug_plan) || cap < 0 || (cap > 0 && !ref_flags)) return RTR_ERR_INVALID;
    if (finish_cap < 0 || (finish_cap > 0 && !finish)) return RTR_ERR_INVALID;
    Validator v;
    v.s = s;
    rtr_scene_info info{};
    if (int rc = v.run(&info)) return rc;
    const LoweredScene L = lower_scene(s, info);
    const SceneFacts& f = L.facts;
    int ties = 0, guards = 0;
    for (size_t k = 0; k < L.prims.size(); ++k) {
        ties += (L.prims[k].reserved & RT_TIE_FLAG) != 0, guards += (L.prims[k].reserved & RT_GUARD_FLAG) != 0;
        if ((int64_t)k < cap) ref_flags[k] = L.prims[k].reserved;
    }
    const int trav = pick_trav(f, info, flags);
    const MegaVariant m = mega_variant(f, integrator, trav, flags, nullptr);
    *out = rtr_debug_plan{info.fast_ok, info.has_media, f.flat_scene, f.flat_guarded, f.lean_materials, f.quad_lights_only,
                          f.uv_order_dependent, f.machine_ok, f.guarded_program, f.top_tree, f.needs_uv, f.n_material_types,
                          L.ds.shared_div, L.ds.pair_cast, (int32_t)L.steps.size(), (int32_t)L.visits.size(),
                          (int32_t)L.prims.size(), f.fast_stack_words, info.stack_words + f.walk_extra_words, ties, guards,
                          trav, m.trav, m.ms, m.sorted, m.pair, (int32_t)L.finish.size()};
    if (finish_cap > 0 && !L.finish.empty())
        std::memcpy(finish, L.finish.data(), sizeof(FFin) * (size_t)std::min<int64_t>(finish_cap, (int64_t)L.finish.size()));
    return RTR_OK;
}
int rtr_debug_frame_shapes(const rtr_scene_desc* s, int32_t* shapes, int64_t cap, int32_t* n_inst) {
    if (!n_inst || cap < 0 || (cap > 0 && !shapes)) return RTR_ERR_INVALID;
    Validator v;
    v.s = s;
    rtr_scene_info info{};
    if (int rc = v.run(&info)) return rc;
    const LoweredScene L = lower_scene(s, info);
    *n_inst = L.ds.n_finst;
    for (int k = 0; k < L.ds.n_finst && k < cap; ++k) shapes[k] = L.cs.inst[(size_t)k].shape;
    return RTR_OK;
}
int rtr_debug_last_kernel(rtr_context* c, rtr_debug_kernel* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_kernel)) return RTR_ERR_INVALID;
    *out = c->last_kernel;
    return RTR_OK;
}
int rtr_debug_last_batch(rtr_context* c, int family, rtr_debug_batch* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_batch) || family < 0 || family >= RTR_DEBUG_FAMILIES) return RTR_ERR_INVALID;
    *out = c->last_batch[family];
    return RTR_OK;
}
int64_t rtr_debug_last_launches(rtr_context* c) { return c ? c->last_launches : -1; }
int rtr_debug_li(rtr_context* c, const rtr_render_params* p, const int32_t* ijs, rtr_debug_li_out* out, int64_t n) {
    static_assert(sizeof(rtr_debug_li_out) == sizeof(LiOut), "one layout");
    if (n < 0 || (n > 0 && (!ijs || !out))) return RTR_ERR_INVALID;
    return li_run(c, p, ijs, nullptr, reinterpret_cast<LiOut*>(out), n);
}
void rtr_debug_set_error(rtr_context* c, const char* msg) {
    if (c) c->err = msg ? msg : "";
}

} /* extern "C" */
