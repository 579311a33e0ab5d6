/*
 * rt_context.h -- the private context of librtr_hip.so, declared once: what is behind the opaque rtr_context, rtr_accum
 * and rtr_history of include/rtr_hip.h, and the helpers that more than one translation unit of the library needs.
 * Each helper is defined in exactly one unit (named below); all sit in namespace rtr.  Nothing outside csrc/ includes
 * this header, and librtr_hip_test.so reaches a context through rt_debug.h only.
 */
#pragma once

#include "rt_debug.h"
#include "rt_select.h"

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

struct AccumPlanK; /* rt_accum_kernels.h */

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
/* the device arrays of the uploaded scene, one per pointer of DScene, and the DScene itself.  DevBufs only: rtr_destroy
 * frees them as an array, so a new one needs its declaration here and its line in rtr_upload_scene, nothing else */
struct SceneBufs {
    DevBuf nodes, kids, mats, tex, perlin, images, imgbytes, lights;
    DevBuf finst, fxf, fref, fexit, fbvh, fsub, fscan, fguard, fstep, fvisit, fprim, fleaf, fmat, ffin, sconsts, dscene;
    DevBuf* begin() { return &nodes; }
    DevBuf* end() { return begin() + sizeof(SceneBufs) / sizeof(DevBuf); }
};
static_assert(sizeof(SceneBufs) == 24 * sizeof(DevBuf), "SceneBufs holds DevBufs only");

struct rtr_context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr; /* cancel flag writes */
    std::string err;
    /* scene */
    bool has_scene = false;
    rtr_scene_info info{};
    DScene ds{};
    SceneFacts facts; /* what lower_scene found out about it */
    SceneBufs sb;
    /* per-render workspace */
    DevBuf b_tiles, b_partial, b_done, b_stats, b_cancel, b_test, b_stage;
    DevBuf b_denoise; /* rtr_accum_denoise / rtr_denoise_host: the planes of DenoiseK */
    /* the host entries of every unit that includes rt_batch.h: what stays on the device for the whole call at the head (a
     * grid, centres, an environment), then one slice of inputs and its results (staged_slices of rt_batch.h; rtr_preview
     * lays its frame out there itself).  One buffer serves them all: each returns only behind its last slice's wait, and
     * the device entries never touch it */
    DevBuf b_batch;
    DevBuf b_display;    /* rtr_display_*: the sRGB thresholds (uploaded by rtr_create), the histogram, the DisplayRec */
    DevBuf b_display_io; /* rtr_display_host / _histogram: the image and its outputs (nothing else uses it) */
    std::vector<int> last_tiles; /* what b_tiles holds */
    WavefrontPool pool;
    void* h_stage = nullptr; /* pinned: rtr_render_tiles_host */
    size_t h_stage_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool stats_pending = false;
    bool in_flight = false; /* stream-ordered work of a render call is queued whose statistics are not pending (an error return) */
    rtr_render_stats stats{};
    rtr_debug_kernel last_kernel{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0}; /* rtr_debug_last_kernel */
    rtr_debug_batch last_batch[RTR_DEBUG_FAMILIES] = {{-1, -1, 0, 0}, {-1, -1, 0, 0}, {-1, -1, 0, 0}, {-1, -1, 0, 0}}; /* rtr_debug_last_batch */
    long long last_launches = 0; /* launches of the last launch_records call (rt_batch.h): rtr_debug_last_launches */
    /* Cancel.  Renders are numbered; rtr_cancel() covers every render issued so far: it stores the newest
     * id in `cancelled_upto` and in the device word the kernels poll.  A render issued afterwards carries a
     * larger id, so nothing has to be reset between renders and a cancel that arrives while a render waits
     * in the stream behind another one is not lost. */
    std::atomic<uint32_t> render_seq{0};
    std::atomic<uint32_t> cancelled_upto{0};
    uint32_t pending_id = 0; /* id of the render whose statistics are pending */
    std::mutex cancel_mu;
    int n_cus = 256; /* hipDeviceProp.multiProcessorCount */
    uint64_t scene_gen = 0; /* rtr_upload_scene calls that reached the device: an accumulator belongs to one scene */
    std::vector<rtr_accum*> accums; /* live accumulators (rtr_destroy frees what is left) */
    /* rtr_set_camera: ds.camera is the current camera; the DScene on the device (sb.dscene: the megakernel and the
     * wavefront stages read it through a pointer) takes it, in stream order, when the next render is issued */
    uint64_t camera_gen = 0;   /* rtr_set_camera calls that succeeded: an accumulator's samples belong to one camera */
    bool camera_dirty = false; /* sb.dscene still holds an older camera */
    std::vector<rtr_history*> histories; /* live histories (rtr_destroy frees what is left) */
};

/* rtr_accum_*: one running sum per owned pixel and a sample count per owned tile, on the device */
struct rtr_accum {
    rtr_context* ctx = nullptr;
    rtr_render_params params{}; /* spp / spp_chunks normalised to 1 */
    uint64_t scene_gen = 0;
    uint64_t camera_gen = 0; /* the context's at creation or at the last rtr_accum_reset */
    std::vector<int> tiles; /* owned tiles, dispatch order; slot k = tiles[k] */
    int tiles_x = 0, tiles_y = 0;
    bool moments = false; /* RTR_ACCUM_MOMENTS: d_q / d_qpart exist and the passes run k_mega<..., ACC = 2> */
    DevBuf d_tiles, d_sum, d_count; /* [n] int, [n][3][RTR_BLOCK] double, [n] int */
    DevBuf d_q, d_qpart; /* [n][RTR_BLOCK] double: committed second moments, and the pass's (committed by k_accum_commit) */
    DevBuf d_s1, d_active, d_nactive, d_err; /* plan of a pass (k_accum_plan): [n] targets, [n] active slots, 1 int; [n] errors */
    mutable std::vector<int> h_counts; /* host copy of d_count ... */
    mutable bool counts_stale = false; /* ... unless a pass was queued since it was read */
    DevBuf d_out; /* rtr_accum_resolve staging: [n][RTR_BLOCK][3] doubles, then [n][RTR_BLOCK][3] bytes */
    DevBuf d_feat; /* rtr_accum_features: [n][RTR_FEAT][RTR_BLOCK] doubles of feat_k samples (0: none yet) */
    int feat_k = 0;
    void* h_out = nullptr; /* pinned, same layout */
    size_t h_out_cap = 0;
};

/* rtr_history_*: the last frame of rtr_accum_denoise_temporal */
struct rtr_history {
    rtr_context* ctx = nullptr;
    int W = 0, H = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    DevBuf d_planes[2]; /* [np][RTR_HIST] each; `cur` is the set the next frame reads */
    DevBuf d_mom;       /* [3][np]: TemporalK::mom */
    int cur = 0;
    bool have = false;  /* false: cleared */
    rtr_camera cam{};   /* the camera d_planes[cur] was seen from */
};

namespace rtr {

/* ---- rtr_capi.hip ---- */
int fail(rtr_context* c, int code, const std::string& msg); /* c->err (null: the error of rtr_create) = msg; returns code */
int ensure(rtr_context* c, DevBuf& b, size_t bytes);
int ensure_behind_queue(rtr_context* c, DevBuf& b, size_t bytes);
int upload(rtr_context* c, DevBuf& b, const void* src, size_t bytes);
int params_check(rtr_context* c, const rtr_render_params* p);
/* the image-size and region predicates of params_check, which rtr_history_create shares */
inline bool image_too_small(const rtr_render_params& p) { return p.image_width < 2 || p.image_height < 2; }
inline bool region_outside(const rtr_render_params& p) {
    return p.x0 < 0 || p.y0 < 0 || p.x1 > p.image_width || p.y1 > p.image_height || p.x0 >= p.x1 || p.y0 >= p.y1;
}
std::vector<int> owned_tiles(const rtr_render_params& p, int& tiles_x, int& tiles_y);
int no_per_ray_kernel(rtr_context* c, int trav);
int finish_stats(rtr_context* c);
int nothing_to_render(rtr_context* c); /* finish_stats, then this call's statistics: all zero */
/* the render call proper; acc != nullptr: a pass of that accumulator, planned on the device from `plan` */
int render_core(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, unsigned char* tile_done, int blocking,
                rtr_accum* acc = nullptr, const AccumPlanK* plan = nullptr);

/* ---- rtr_accum.hip ---- */
int refresh_counts(rtr_context* c, const rtr_accum* a);
int accum_render_check(rtr_context* c, const rtr_accum* a);
AccumResolveK accum_view(const rtr_accum* a);
int accum_features(rtr_context* c, rtr_accum* a, int K);
void free_accum(rtr_accum* a);
/* render_core's accumulator pass: k_accum_errors (a refinement) and k_accum_plan in front of the megakernel, k_accum_commit
 * behind it; `launches` counts the kernels */
void accum_pass_plan(rtr_accum* acc, const AccumPlanK* plan, int n_tiles, hipStream_t stream, int* launches);
void accum_pass_commit(rtr_accum* acc, const RenderK& P, hipStream_t stream);

/* ---- rtr_image.hip ---- */
int display_create(rtr_context* c); /* rtr_create: c->b_display with the sRGB thresholds in it */
void free_history(rtr_history* h);

template <typename K>
int set_lds(rtr_context* c, K kernel, size_t bytes) {
    return kernel_lds(kernel, bytes, 0, c->err);
}

} // namespace rtr

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return rtr::fail(ctx, RTR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)
