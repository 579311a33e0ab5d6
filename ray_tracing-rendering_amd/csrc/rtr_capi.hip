/*
 * rtr_capi.hip -- implementation of the C ABI (include/rtr_hip.h) on top of the HIP
 * kernels of rt_kernels.h.  Host side only: scene validation, the copy of the lowered scene
 * (rt_lower.h: lower_scene) to the device, the kernel-variant decisions (pick_trav, mega_variant),
 * launch geometry, workspace, cancel, statistics.  Built by hipcc for gfx950 into librtr_hip.so.
 */
#define RTR_TU_CAPI
#include "rt_lower.h"
#include "rt_kernels.h"
#include "rt_launch.h"
#include "rt_machine.h"
#include "rt_debug.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

thread_local std::string g_create_error;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
/* the device arrays of the uploaded scene, one per pointer of DScene, and the DScene itself.  DevBufs only: rtr_destroy
 * frees them as an array, so a new one needs its declaration here and its line in rtr_upload_scene, nothing else */
struct SceneBufs {
    DevBuf nodes, kids, mats, tex, perlin, images, imgbytes, lights;
    DevBuf finst, fxf, fref, fexit, fbvh, fsub, fscan, fguard, fstep, fvisit, fprim, fleaf, fmat, ffin, dscene;
    DevBuf* begin() { return &nodes; }
    DevBuf* end() { return begin() + sizeof(SceneBufs) / sizeof(DevBuf); }
};
static_assert(sizeof(SceneBufs) == 23 * sizeof(DevBuf), "SceneBufs holds DevBufs only");

} // namespace

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
    DevBuf b_query; /* rtr_query_closest / rtr_query_occluded: one slice of rays and its results (nothing else uses it) */
    DevBuf b_gather; /* rtr_gather_occlusion / rtr_gather_radiance: one slice of points and its results (nothing else uses it) */
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
    LaunchedGather last_gather{};                                       /* rtr_debug_last_gather */
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

namespace {

int fail(rtr_context* c, int code, const std::string& msg) {
    if (c)
        c->err = msg;
    else
        g_create_error = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(ctx, RTR_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

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

/* rtr_display_srgb_thresholds: S[b] = the inverse sRGB transfer of b / 255.0, computed once on the host.  This table, not
 * a pow on the device, defines RTR_ENCODE_SRGB. */
const double* display_srgb_table() {
    static const struct Table {
        double s[256];
        Table() {
            s[0] = 0.0;
            for (int b = 1; b < 256; ++b) {
                const double v = b / 255.0;
                s[b] = v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4);
            }
        }
    } table;
    return table.s;
}
/* c->b_display: thresholds, histogram, record */
constexpr size_t kDisplayHistOff = 256 * sizeof(double), kDisplayRecOff = kDisplayHistOff + RTR_DISPLAY_BINS * sizeof(unsigned);
constexpr size_t kDisplayBytes = kDisplayRecOff + sizeof(DisplayRec);

/* ---- host-only scene validation + traversal stack analysis -------------------------------- */
struct Validator {
    const rtr_scene_desc* s;
    std::string msg;
    std::vector<int> state;  /* 0 new, 1 on DFS stack, 2 done */
    std::vector<int> need;   /* stack words used below a node (see traverse()) */
    std::vector<int> depth;
    std::vector<char> media; /* subtree contains a constant_medium */
    int code = RTR_OK;

    bool bad(int c, const std::string& m) {
        if (code == RTR_OK) {
            code = c;
            msg = m;
        }
        return false;
    }
    bool node_ix(int i) const { return i >= 0 && i < s->n_nodes; }

    bool texture_ok(int ix, int guard) {
        if (ix < 0 || ix >= s->n_textures) return bad(RTR_ERR_INVALID, "texture index out of range");
        if (guard > 7) return bad(RTR_ERR_UNSUPPORTED, "checker textures nested deeper than 8");
        const rtr_texture& t = s->textures[ix];
        switch (t.type) {
        case RTR_TEX_SOLID: return true;
        case RTR_TEX_CHECKER: return texture_ok(t.a, guard + 1) && texture_ok(t.b, guard + 1);
        case RTR_TEX_NOISE:
            if (t.a < 0 || t.a >= s->n_perlin) return bad(RTR_ERR_INVALID, "perlin table index out of range");
            return true;
        case RTR_TEX_IMAGE:
            if (t.a >= s->n_images) return bad(RTR_ERR_INVALID, "image index out of range");
            if (t.a >= 0) {
                const rtr_image& im = s->images[t.a];
                /* width * height * 3 of two positive int32 fits a uint64; the offset is compared first so
                 * the sum cannot wrap */
                if (im.width <= 0 || im.height <= 0 || im.offset > s->n_image_bytes ||
                    (uint64_t)im.width * (uint64_t)im.height * 3 > s->n_image_bytes - im.offset)
                    return bad(RTR_ERR_INVALID, "image texels out of range");
            }
            return true;
        default: return bad(RTR_ERR_UNSUPPORTED, "unknown texture type");
        }
    }

    bool material_ok(int ix) {
        if (ix < 0 || ix >= s->n_materials) return bad(RTR_ERR_INVALID, "material index out of range");
        const rtr_material& m = s->materials[ix];
        switch (m.type) {
        case RTR_MAT_LAMBERTIAN:
        case RTR_MAT_DIFFUSE_LIGHT:
        case RTR_MAT_ISOTROPIC: return texture_ok(m.tex[0], 0);
        case RTR_MAT_METAL:
        case RTR_MAT_DIELECTRIC: return true;
        case RTR_MAT_PBR:
            if (!texture_ok(m.tex[0], 0) || !texture_ok(m.tex[1], 0) || !texture_ok(m.tex[2], 0)) return false;
            return m.tex[3] < 0 || texture_ok(m.tex[3], 0);
        default: return bad(RTR_ERR_UNSUPPORTED, "unknown material type");
        }
    }

    /* children of a node by position (no per-visit copies: a hittable_list can hold a million of them) */
    int child_count(const rtr_node& n) const {
        switch (n.type) {
        case RTR_NODE_BVH: return 2;
        case RTR_NODE_LIST: return n.b;
        case RTR_NODE_TRANSLATE:
        case RTR_NODE_ROTATE_Y:
        case RTR_NODE_FLIP_FACE:
        case RTR_NODE_MEDIUM: return 1;
        default: return 0;
        }
    }
    int child_at(const rtr_node& n, int k) const {
        if (n.type == RTR_NODE_BVH) return k == 0 ? n.a : n.b;
        if (n.type == RTR_NODE_LIST) return s->list_children[n.a + k];
        return n.a;
    }

    /* iterative post-order DFS over the hittable DAG */
    bool walk(int root) {
        struct Frame {
            int node, next;
        };
        std::vector<Frame> stk;
        stk.push_back({root, 0});
        state[root] = 1;
        while (!stk.empty()) {
            Frame& f = stk.back();
            const rtr_node& n = s->nodes[f.node];
            if (f.next == 0) { /* first visit: check the record itself */
                int n_geom = 0; /* leading f[] entries the scene compiler builds boxes from: must be finite */
                switch (n.type) {
                case RTR_NODE_BVH: /* its box is only ever compared with a ray: any value is safe */
                case RTR_NODE_FLIP_FACE: break;
                case RTR_NODE_TRANSLATE: n_geom = 3; break;
                case RTR_NODE_ROTATE_Y: n_geom = 2; break;
                case RTR_NODE_LIST:
                    if (n.a < 0 || n.b < 0 || (int64_t)n.a + n.b > s->n_list_children)
                        return bad(RTR_ERR_INVALID, "hittable_list children out of range");
                    break;
                case RTR_NODE_MEDIUM:
                    if (!material_ok(n.b)) return false;
                    break;
                case RTR_NODE_SPHERE: n_geom = 4; break;
                case RTR_NODE_MOVING_SPHERE: n_geom = 9; break;
                case RTR_NODE_XY_RECT:
                case RTR_NODE_XZ_RECT:
                case RTR_NODE_YZ_RECT: n_geom = 5; break;
                default: return bad(RTR_ERR_UNSUPPORTED, "unknown hittable node type");
                }
                if (n.type >= RTR_NODE_SPHERE && !material_ok(n.a)) return false;
                for (int k = 0; k < n_geom; ++k)
                    if (!std::isfinite(n.f[k])) return bad(RTR_ERR_INVALID, "non-finite primitive or transform parameter");
            }
            const int m = child_count(n);
            if (f.next < m) {
                int k = child_at(n, f.next++);
                if (!node_ix(k)) return bad(RTR_ERR_INVALID, "hittable child index out of range");
                if (state[k] == 1) return bad(RTR_ERR_INVALID, "hittable graph has a cycle");
                if (state[k] == 0) {
                    state[k] = 1;
                    stk.push_back({k, 0});
                }
                continue;
            }
            /* children done: stack words, depth, media */
            const int me = f.node;
            int u = 0, d = 0;
            char md = 0;
            for (int k = 0; k < m; ++k) {
                const int ck = child_at(n, k);
                d = std::max(d, depth[ck]);
                md |= media[ck];
            }
            switch (n.type) {
            case RTR_NODE_BVH: u = std::max(2, std::max(1 + need[n.a], need[n.b])); break;
            case RTR_NODE_LIST:
                if (m > RT_LIST_BULK) { /* continuation (2 words) + the child being walked */
                    u = 3;
                    for (int k = 0; k < m; ++k) u = std::max(u, 2 + need[child_at(n, k)]);
                } else {
                    u = m;
                    for (int k = 0; k < m; ++k) u = std::max(u, (m - 1 - k) + need[child_at(n, k)]);
                }
                break;
            case RTR_NODE_TRANSLATE: u = RT_FRAME_TRANSLATE + std::max(1, need[n.a]); break;
            case RTR_NODE_ROTATE_Y: u = RT_FRAME_ROTATE + std::max(1, need[n.a]); break;
            case RTR_NODE_FLIP_FACE: u = RT_FRAME_FLIP + std::max(1, need[n.a]); break;
            case RTR_NODE_MEDIUM:
                if (md) return bad(RTR_ERR_UNSUPPORTED, "constant_medium nested inside a medium boundary");
                u = std::max(1, need[n.a]);
                md = 1;
                break;
            default: break;
            }
            need[me] = u;
            depth[me] = d + 1;
            media[me] = md;
            state[me] = 2;
            stk.pop_back();
        }
        return true;
    }

    int run(rtr_scene_info* info) {
        if (!s) return (bad(RTR_ERR_INVALID, "null scene"), code);
        if (s->abi_version != RTR_ABI_VERSION) return (bad(RTR_ERR_INVALID, "ABI version mismatch"), code);
        if (s->n_nodes >= RT_LIST_MARK) return (bad(RTR_ERR_INVALID, "more than 2^30 nodes"), code);
    if (s->n_nodes <= 0 || s->n_list_children < 0 || s->n_materials < 0 || s->n_textures < 0 ||
            s->n_perlin < 0 || s->n_images < 0 || s->n_lights < 0)
            return (bad(RTR_ERR_INVALID, "negative or empty counts"), code);
        if (!node_ix(s->root)) return (bad(RTR_ERR_INVALID, "root out of range"), code);
        if (!s->nodes || (s->n_list_children && !s->list_children) || (s->n_materials && !s->materials) ||
            (s->n_textures && !s->textures) || (s->n_perlin && !s->perlin) || (s->n_images && !s->images) ||
            (s->n_image_bytes && !s->image_bytes) || (s->n_lights && !s->lights))
            return (bad(RTR_ERR_INVALID, "null array with non-zero count"), code);
        for (int k = 0; k < s->n_lights; ++k) {
            const rtr_light& l = s->lights[k];
            if (l.type < 0 || l.type >= RTR_LIGHT_TYPE_COUNT)
                return (bad(RTR_ERR_UNSUPPORTED, "unknown light type (QuadLight, PointLight, SpotLight, DirectionalLight, EnvironmentLight are on the device)"), code);
            if (l.type == RTR_LIGHT_ENV_MAP) { /* texels and sampling tables live in image_bytes */
                const double w = l.f[0], h = l.f[1], to = l.f[3], tb = l.f[4];
                if (!(w >= 1 && h >= 1 && w <= 65536 && h <= 65536) || w != (double)(int)w || h != (double)(int)h)
                    return (bad(RTR_ERR_INVALID, "environment map size out of range"), code);
                const double nb = (double)s->n_image_bytes;
                const double texel_bytes = w * h * 3 * 4, table_bytes = (h * (2 * w + 2) + (2 * h + 2)) * 8;
                if (!(to >= 0 && tb >= 0) || to != (double)(uint64_t)to || tb != (double)(uint64_t)tb ||
                    (uint64_t)to % 4 || (uint64_t)tb % 8 || to + texel_bytes > nb || tb + table_bytes > nb)
                    return (bad(RTR_ERR_INVALID, "environment map texels / tables out of range or misaligned"), code);
            }
        }
        /* every record is checked, also those the graph under `root` does not reach: upload and the
         * scene-wide facts (material classes, texture classes) loop over whole arrays */
        for (int k = 0; k < s->n_textures; ++k)
            if (!texture_ok(k, 0)) return code;
        for (int k = 0; k < s->n_materials; ++k)
            if (!material_ok(k)) return code;
        /* materials/perlin.h:35 indexes ranvec[perm_x ^ perm_y ^ perm_z]: the device does the same, unchecked */
        for (int k = 0; k < s->n_perlin; ++k)
            for (int i = 0; i < 256; ++i)
                if ((unsigned)s->perlin[k].perm_x[i] > 255u || (unsigned)s->perlin[k].perm_y[i] > 255u ||
                    (unsigned)s->perlin[k].perm_z[i] > 255u)
                    return (bad(RTR_ERR_INVALID, "perlin permutation entry out of range"), code);
        for (int k = 0; k < s->n_nodes; ++k) {
            const rtr_node& n = s->nodes[k];
            if (n.type < 0 || n.type >= RTR_NODE_TYPE_COUNT)
                return (bad(RTR_ERR_UNSUPPORTED, "unknown hittable node type"), code);
            if (n.type >= RTR_NODE_SPHERE && (n.a < 0 || n.a >= s->n_materials))
                return (bad(RTR_ERR_INVALID, "material index out of range"), code);
            if (n.type == RTR_NODE_MEDIUM && (n.b < 0 || n.b >= s->n_materials))
                return (bad(RTR_ERR_INVALID, "material index out of range"), code);
        }
        state.assign(s->n_nodes, 0);
        need.assign(s->n_nodes, 0);
        depth.assign(s->n_nodes, 0);
        media.assign(s->n_nodes, 0);
        if (!walk(s->root)) return code;
        if (info) {
            info->stack_words = std::max(1, need[s->root]);
            info->has_media = media[s->root];
            int inverted = 0;
            for (int k = 0; k < s->n_nodes; ++k)
                if (state[k] == 2 && ((s->nodes[k].type == RTR_NODE_SPHERE && s->nodes[k].f[3] < 0) ||
                                      (s->nodes[k].type == RTR_NODE_MOVING_SPHERE && s->nodes[k].f[8] < 0)))
                    ++inverted;
            info->inverted_boxes = inverted;
            info->graph_depth = depth[s->root];
            int uv = 0;
            for (int k = 0; k < s->n_textures; ++k)
                if (s->textures[k].type == RTR_TEX_IMAGE && s->textures[k].a >= 0) uv = 1;
            info->needs_uv = uv;
        }
        return RTR_OK;
    }
};

int params_check(rtr_context* c, const rtr_render_params* p) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null params");
    if (p->image_width < 2 || p->image_height < 2) return fail(c, RTR_ERR_INVALID, "image smaller than 2x2");
    /* tile indices are int32 and the tile list is materialised: 2^26 tiles = 131 072 x 131 072 pixels, more
     * than a framebuffer in 288 GB of HBM holds */
    if (((int64_t)p->image_width + 15) / 16 * (((int64_t)p->image_height + 15) / 16) > ((int64_t)1 << 26))
        return fail(c, RTR_ERR_INVALID, "image larger than 2^26 tiles");
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->image_width || p->y1 > p->image_height || p->x0 >= p->x1 ||
        p->y0 >= p->y1)
        return fail(c, RTR_ERR_INVALID, "region outside the image or empty");
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

/* which traversal a call uses: the compiled scene unless it does not exist or the caller asks
 * for the reference's visiting order */
int pick_trav(const SceneFacts& f, const rtr_scene_info& info, int flags) {
    if (info.has_media || (info.inverted_boxes && !info.fast_ok)) /* (hollow spheres as guarded references: compiled) */
        return info.program_steps > 0 && !(flags & RTR_FLAG_REFERENCE_ORDER) ? RT_TRAV_PROGRAM : RT_TRAV_MEDIA;
    if (!info.fast_ok || f.uv_order_dependent || (flags & RTR_FLAG_REFERENCE_ORDER))
        return RT_TRAV_EXACT;
    return f.flat_scene ? RT_TRAV_FLAT : RT_TRAV_FAST;
}
size_t stack_bytes(const SceneFacts& f, const rtr_scene_info& info, int trav) {
    const bool compiled = trav == RT_TRAV_FAST || trav == RT_TRAV_FLAT || rt_is_program(trav) || trav == RT_TRAV_TOP || trav == RT_TRAV_FLAT_GUARD;
    const int words = compiled ? f.fast_stack_words : info.stack_words + f.walk_extra_words;
    return (size_t)words * RTR_BLOCK * sizeof(int);
}
/* The RT_TRAV_* template value a per-ray kernel (k_li, k_features, k_query_*, the unit kernels of the test library)
 * takes for a call with `flags`: flat scenes take RT_TRAV_FAST (same hits, one kernel for both), a program the general
 * program kernel, and with `top` a sub-scene 0 with a top tree RT_TRAV_TOP, like the megakernel. */
int per_ray_trav(const SceneFacts& f, const rtr_scene_info& info, int flags, bool top) {
    int trav = pick_trav(f, info, flags);
    if (trav == RT_TRAV_FLAT) trav = RT_TRAV_FAST;
    if (top && trav == RT_TRAV_FAST && f.top_tree) trav = RT_TRAV_TOP;
    return trav == RT_TRAV_PROGRAM ? RT_TRAV_PROGRAM_EXT : trav;
}
/* the traversals k_li and k_features are instantiated for; the queries and the unit kernels also walk a top tree */
using PerRayTravs = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>;
using PerRayTravsTop = TravSet<RT_TRAV_FAST, RT_TRAV_TOP, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>;
int no_per_ray_kernel(rtr_context* c, int trav) {
    return fail(c, RTR_ERR_UNSUPPORTED, "no per-ray kernel for traversal " + std::to_string(trav));
}

template <typename K>
int set_lds(rtr_context* c, K kernel, size_t bytes) {
    return kernel_lds(kernel, bytes, 0, c->err);
}

/* THE place that decides which k_mega instantiation a render runs: from what lower_scene found out about the scene,
 * the integrator, the traversal pick_trav() chose and the render flags.  `flags_in_effect` (may be null) receives the
 * flags that changed the choice. */
MegaVariant mega_variant(const SceneFacts& f, int integ, int trav, int flags, int* flags_in_effect) {
    MegaVariant v{integ, trav, RT_MS_FULL, false, false};
    /* MIS and RR have flat, lean and guarded kernels; the others the generic material set on the
     * general compiled-scene kernel, one program kernel -- the general one --, and the media kernel, which also serves
     * the reference-order traversal of scenes without media */
    const bool n1 = integ != RTR_INTEGRATOR_MIS && integ != RTR_INTEGRATOR_RR;
    if (v.trav == RT_TRAV_FLAT && n1) v.trav = RT_TRAV_FAST;
    if (v.trav == RT_TRAV_FAST && f.top_tree) v.trav = RT_TRAV_TOP; /* many instances: the per-lane walk (FSub) */
    if (v.trav == RT_TRAV_FAST && f.flat_guarded && !n1) v.trav = RT_TRAV_FLAT_GUARD;
    if (v.trav == RT_TRAV_PROGRAM && (f.guarded_program || n1)) v.trav = RT_TRAV_PROGRAM_EXT;
    if (n1) {
        if (v.trav == RT_TRAV_EXACT) v.trav = RT_TRAV_MEDIA;
        return v;
    }
    const int t = v.trav;
    const bool lean = f.lean_materials && (t == RT_TRAV_FLAT || t == RT_TRAV_FAST || t == RT_TRAV_TOP || t == RT_TRAV_EXACT);
    /* "every material, QuadLights only": a kernel of the MIS integrator (RR has no light code) on the compiled scene */
    const bool quadlit = f.quad_lights_only && !f.needs_uv && integ == RTR_INTEGRATOR_MIS && t != RT_TRAV_MEDIA && t != RT_TRAV_EXACT;
    v.ms = lean ? RT_MS_LEAN : (quadlit ? RT_MS_QUADLIT : RT_MS_FULL);
    /* (the sorted variant packs the material index into 16 bits) */
    v.sorted = (flags & RTR_FLAG_SORTED_SHADING) && f.n_materials <= 65535 && mega_sortable(integ, t, v.ms);
    const bool pairable = mega_pairable(integ, t) && !v.sorted && f.pair_cast;
    v.pair = pairable && !(flags & RTR_FLAG_SPLIT_CASTS);
    if (flags_in_effect && v.sorted) *flags_in_effect |= RTR_FLAG_SORTED_SHADING;
    if (flags_in_effect && pairable && !v.pair) *flags_in_effect |= RTR_FLAG_SPLIT_CASTS;
    return v;
}

/* Whether a render of variant `v` runs the job-queue twin of its pair-cast kernel (rt_kernels.h: k_mega_queue): one-shot
 * renders only; the pixel is packed into 16 + 16 bits and block ids are int32, beyond that the static grid stays. */
bool mega_queue(const MegaVariant& v, const RenderK& P, int flags) {
    return v.pair && P.tile_s0 == nullptr && !(flags & RTR_FLAG_STATIC_GRID) && P.W <= 65535 && P.H <= 65535 &&
           (long long)P.n_tiles * P.chunks * 4 < (1ll << 31);
}

/* `dry`: only what can fail without touching the stream (the LDS size check / attribute, the occupancy query) */
int launch_mega(rtr_context* c, const RenderK& P, int integrator, int trav_in, bool dry, int* blocks_per_cu, int flags,
                int* flags_in_effect = nullptr, LaunchedKernel* launched = nullptr) {
    MegaLaunch L{};
    const MegaVariant& v = L.variant = mega_variant(c->facts, integrator, trav_in, flags, flags_in_effect);
    L.stack_words = (int)(stack_bytes(c->facts, c->info, v.trav) / (RTR_BLOCK * sizeof(int)));
    L.dsc = static_cast<const DScene*>(c->sb.dscene.p);
    /* (the reference-order walk of PBR / NEE runs the media kernel with the parked words of the traversal that was
     * asked for, as it always has: workgroups per CU decide the chunking of a render, and that its rounding) */
    const int park = v.sorted ? SK_WORDS : park_words(integrator, trav_in == RT_TRAV_EXACT ? RT_TRAV_EXACT : v.trav);
    L.lds = stack_bytes(c->facts, c->info, v.trav) + (size_t)park * RTR_BLOCK * sizeof(double);
    L.accum = P.tile_s0 == nullptr ? 0 : (P.q_in ? 2 : 1);
    L.stream = c->stream;
    L.P = P;
    L.dry = dry;
    L.blocks_per_cu = blocks_per_cu;
    L.queue = mega_queue(v, P, flags);
    L.n_cus = c->n_cus;
    /* (RTR_QUEUE_WORKGROUPS = n caps the persistent grid: with 1, four waves eat every block of a small image) */
    if (const char* g = getenv("RTR_QUEUE_WORKGROUPS")) L.grid_cap = std::atoi(g);
    if (flags_in_effect && v.pair && L.accum == 0 && (flags & RTR_FLAG_STATIC_GRID)) *flags_in_effect |= RTR_FLAG_STATIC_GRID;
    int rc;
    switch (integrator) {
    case RTR_INTEGRATOR_MIS: rc = rtr_mega_launch_mis(L, c->err); break;
    case RTR_INTEGRATOR_RR:
    case RTR_INTEGRATOR_PATH: rc = rtr_mega_launch_rr_path(L, c->err); break;
    default: rc = rtr_mega_launch_pbr_nee(L, c->err); break;
    }
    if (rc == RTR_OK && !dry && launched)
        launched->trav = v.trav, launched->ms = v.ms, launched->sorted = v.sorted, launched->pair = v.pair, launched->queue = L.queue;
    return rc;
}

/* auto chunking.  A workgroup renders one tile for one chunk of the samples.  More chunks = more, shorter
 * workgroups: the resident slots drain more evenly at the end of the launch, but every workgroup pays its
 * start-up once.  Model fitted to sweeps on scenes 21 / 23 / 9 (4-8 chunks beat 1-2 by 3-10 %, 32 lose
 * 10 %): efficiency = R / (R + 0.75) * s / (s + 2) with R = rounds over the resident slots and s = samples
 * per pixel and chunk; the best power of two is taken.  It picks 8 for C2 on one GPU and 16 for the 313
 * tiles one of 8 ranks owns. */
int auto_chunks(int pipeline, double resident_slots, int n_tiles, int spp) {
    int chunks = 1;
    if (pipeline == RTR_PIPELINE_WAVEFRONT) { /* one pool slot per pixel and chunk: keep the pool small */
        while ((long long)n_tiles * chunks < 8192 && chunks * 2 * 8 <= spp && chunks < 64) chunks *= 2;
        return chunks; /* about 2 M slots (0.5 GB of path state) where the image allows it */
    }
    double best = 0;
    for (int cand = 1; cand <= 64 && cand <= spp; cand *= 2) {
        const double rounds = (double)n_tiles * cand / resident_slots, s_per = (double)spp / cand;
        const double eff = rounds / (rounds + 0.75) * s_per / (s_per + 2.0);
        if (eff > best) best = eff, chunks = cand;
    }
    return chunks;
}


/* spp_chunks = 0: the library's choice for this scene, pipeline and number of owned tiles */
int choose_chunks(rtr_context* c, RenderK P, int integrator, int pipeline, int trav, int spp, int flags, int* chunks, int* guided) {
    /* workgroups of this kernel variant the chip holds at once (registers / LDS decide: 2-5 per CU) */
    int per_cu = 4;
    P.chunks = 1;
    if (pipeline == RTR_PIPELINE_MEGAKERNEL)
        if (int rc = launch_mega(c, P, integrator, trav, true, &per_cu, flags)) return rc;
    const double resident = (double)c->n_cus * (per_cu > 0 ? per_cu : 1);
    *chunks = auto_chunks(pipeline, resident, P.n_tiles, spp);
    /* Guided chunks.  With equal chunks a launch ends with part of the chip waiting for the last full-size
     * workgroups -- a tenth of the time of a rank's eighth of C2 (313 tiles: 4.9 rounds over the resident slots).
     * Instead three quarters of the chunks carry 90 % of a pixel's samples and run first; the rest is cut into thirds
     * of that size and drains the launch.  Measured on one GPU, scene 21 800x800 spp 400, share of 1 / 2 / 4 / 8
     * ranks: 75.2 / 38.6 / 20.3 / 10.9 ms with equal chunks, 74.5 / 37.9 / 19.8 / 10.2 ms guided (100 / 98 / 94 / 91 %
     * of the ideal share).  Not worth it once the launch has tens of rounds anyway. */
    guided[0] = guided[1] = guided[2] = 0;
    const double rounds = (double)P.n_tiles * *chunks / resident;
    if (pipeline == RTR_PIPELINE_MEGAKERNEL && *chunks >= 4 && rounds < 30.0 && spp >= 8 * *chunks) {
        /* (RTR_GUIDED = "big-share,small-divisor,big-chunk-eighths" overrides the split for tools/shard_sweep.py) */
        double share = 0.90;
        int div = 3, eighths = 6;
        if (const char* g = getenv("RTR_GUIDED")) std::sscanf(g, "%lf,%d,%d", &share, &div, &eighths);
        const int n_big = std::max(1, *chunks * eighths / 8);
        const int big = (int)((share * spp + n_big - 1) / n_big);
        const int rem = spp - n_big * big;
        const int small = std::max(1, big / std::max(1, div));
        if (rem > 0) {
            const int n_small = (rem + small - 1) / small;
            guided[0] = n_big, guided[1] = big, guided[2] = small;
            *chunks = n_big + n_small;
        }
    }
    return RTR_OK;
}

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
                                          "cast counters", "random_in_unit_sphere rejection loop"};
        double total = 0;
        for (int k = 0; k < RG_N; ++k) total += (double)h[RT_PROF_BASE + k];
        std::fprintf(stderr, "[region profile] %.4g wave cycles in all, %llu samples\n", total, h[0]);
        for (int k = 0; k < RG_N; ++k)
            if (h[RT_PROF_BASE + RT_PROF_REGIONS + k])
                std::fprintf(stderr, "[region profile] %-36s %6.2f %%  %12llu visits  %8.1f cycles/visit\n", names[k],
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

} // namespace

static void free_accum(rtr_accum* a) {
    DevBuf* bufs[] = {&a->d_tiles, &a->d_sum, &a->d_count, &a->d_out, &a->d_q, &a->d_qpart, &a->d_s1, &a->d_active, &a->d_nactive, &a->d_err,
                      &a->d_feat};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    if (a->h_out) hipHostFree(a->h_out);
    delete a;
}

static void free_history(rtr_history* h) {
    for (DevBuf* b : {&h->d_planes[0], &h->d_planes[1], &h->d_mom})
        if (b->p) hipFree(b->p);
    delete h;
}

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
    if (!rc) rc = ensure(c, c->b_display, kDisplayBytes);
    if (!rc && hipMemcpy(c->b_display.p, display_srgb_table(), 256 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        rc = RTR_ERR_DEVICE;
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
                      &c->b_query, &c->b_gather, &c->b_display, &c->b_display_io};
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
    if ((rc = upload(c, b.dscene, &d, sizeof(DScene)))) return rc;
    c->info = info;
    c->facts = L.facts;
    c->camera_dirty = false;
    c->has_scene = true;
    return RTR_OK;
}

/* the render call proper; tile_done != nullptr: packed output (see ResolveK) */
static int render_core(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, unsigned char* tile_done,
                       int blocking, rtr_accum* acc = nullptr, const AccumPlanK* plan = nullptr);

int rtr_render_device(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_render before rtr_upload_scene");
    if (int prc = params_check(c, p)) return prc;
    if (!d_rgb || row_stride < (int64_t)(p->x1 - p->x0)) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    return render_core(c, p, d_rgb, row_stride, nullptr, blocking);
}

/* acc != nullptr: a pass of that accumulator (p->spp_chunks = 1): its tile list, its counts as start samples and its
 * sums (and moments) as start values; `plan` (mode, targets, refinement bounds) says how k_accum_plan sets each tile's
 * end sample and the active list before the megakernel, k_accum_errors runs first for a refinement, and the commit
 * kernel takes the place of k_resolve */
static int render_core(rtr_context* c, const rtr_render_params* p, double* d_rgb, int64_t row_stride, unsigned char* tile_done,
                       int blocking, rtr_accum* acc, const AccumPlanK* plan) {
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
        if ((rc = finish_stats(c))) return rc;
        c->stats = rtr_render_stats{};
        c->last_kernel = rtr_debug_kernel{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
        return RTR_OK;
    }

    int pipeline = p->pipeline;
    if (pipeline == RTR_PIPELINE_AUTO) pipeline = RTR_PIPELINE_MEGAKERNEL;
    const int trav = pick_trav(c->facts, c->info, p->flags);
    if (pipeline == RTR_PIPELINE_WAVEFRONT && (!c->facts.machine_ok || (trav != RT_TRAV_FLAT && trav != RT_TRAV_FAST && trav != RT_TRAV_PROGRAM)))
        return fail(c, RTR_ERR_UNSUPPORTED, "the wavefront pipeline runs the compiled traversals only: this graph (or "
                                            "RTR_FLAG_REFERENCE_ORDER) needs the reference-order walk of the megakernel");
    if (pipeline == RTR_PIPELINE_WAVEFRONT && (p->flags & RTR_FLAG_WF_PERSISTENT) && c->facts.guarded_program)
        return fail(c, RTR_ERR_UNSUPPORTED, "RTR_FLAG_WF_PERSISTENT: the traversal machine does not run step programs with "
                                            "guarded primitives (hollow spheres under bvh_nodes) or media under transforms; "
                                            "the lockstep stages do");
    int chunks = p->spp_chunks, guided[3] = {0, 0, 0};
    if (chunks == 0 && (rc = choose_chunks(c, P, p->integrator, pipeline, trav, p->spp, p->flags, &chunks, guided))) return rc;
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
    if (pipeline == RTR_PIPELINE_MEGAKERNEL && (rc = launch_mega(c, P, p->integrator, trav, true, nullptr, p->flags))) return rc;
    const bool queue = pipeline == RTR_PIPELINE_MEGAKERNEL && mega_queue(mega_variant(c->facts, p->integrator, trav, p->flags, nullptr), P, p->flags);

    const uint32_t id = c->render_seq.fetch_add(1) + 1; /* rtr_cancel() from now on covers this render */
    P.render_id = id;
    c->stats_pending = false; /* an unfinished earlier render's statistics are dropped here */
    c->in_flight = true;      /* ... but what it queued, and what this call queues from here on, is still tracked: an error
                                 return below leaves it set, and the next call (or rtr_get_stats) waits before it touches
                                 the tile list, the workspace or the wavefront pool */
    c->stats = rtr_render_stats{};
    c->stats.spp_chunks = chunks;
    c->last_kernel = rtr_debug_kernel{-1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
    LaunchedKernel launched{};
    c->pending_id = id;
    HIPCHK(c, hipMemsetAsync(c->b_stats.p, 0, RT_STATS_WORDS * sizeof(unsigned long long), c->stream));
    if (c->camera_dirty) { /* rtr_set_camera: behind every render queued with the old camera, in front of this one */
        hipLaunchKernelGGL(k_camera_store, dim3(1), dim3(64), 0, c->stream, static_cast<DScene*>(c->sb.dscene.p), c->ds.camera);
        HIPCHK(c, hipGetLastError());
        c->camera_dirty = false;
    }
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (pipeline == RTR_PIPELINE_WAVEFRONT) {
        int launches = 0;
        WavefrontPlan plan{};
        plan.has_lights = c->ds.n_lights > 0;
        plan.media = trav == RT_TRAV_PROGRAM;
        plan.lean = c->facts.lean_materials && !plan.media;
        plan.quadlit = c->facts.quad_lights_only && !c->info.needs_uv;
        plan.sort = !plan.lean && c->facts.n_material_types > 1;
        plan.n_cus = c->n_cus;
        plan.lds = stack_bytes(c->facts, c->info, trav);
        plan.trav = trav;
        plan.machine = (p->flags & RTR_FLAG_WF_PERSISTENT) != 0;
        if (plan.machine) c->stats.flags_in_effect |= RTR_FLAG_WF_PERSISTENT;
        rc = wavefront_render(c->pool, static_cast<const DScene*>(c->sb.dscene.p), plan, P, p->integrator, d_rgb, row_stride,
                              tile_done, c->stream, &c->cancelled_upto, &launches, &launched, c->err);
        c->last_kernel = rtr_debug_kernel{pipeline, p->integrator, launched.trav, launched.ms, launched.sorted, launched.phases,
                                          plan.lean, plan.quadlit, plan.sort, plan.media, plan.machine};
        if (rc && rc != RTR_ERR_CANCELLED) return rc;
        if (rc == RTR_ERR_CANCELLED) c->stats.cancelled = 1;
        c->stats.kernel_launches = launches;
    } else {
        int launches = 2;
        if (acc) { /* the pass's plan, on the device: no host round trip between a refinement's decision and its pass */
            acc->counts_stale = true;
            AccumPlanK K = *plan;
            K.n_tiles = P.n_tiles;
            K.count = static_cast<const int*>(acc->d_count.p);
            K.err = static_cast<const double*>(acc->d_err.p);
            K.tile_s1 = static_cast<int*>(acc->d_s1.p);
            K.active = static_cast<int*>(acc->d_active.p);
            K.n_active = static_cast<int*>(acc->d_nactive.p);
            if (K.mode == 2) {
                hipLaunchKernelGGL(k_accum_errors, dim3((unsigned)P.n_tiles), dim3(RTR_BLOCK), 0, c->stream, accum_view(acc),
                                   static_cast<const double*>(acc->d_q.p), static_cast<double*>(acc->d_err.p));
                ++launches;
            }
            hipLaunchKernelGGL(k_accum_plan, dim3(1), dim3(1024), 0, c->stream, K);
            ++launches;
            HIPCHK(c, hipGetLastError());
        }
        if (queue) /* the jobs count themselves in the completion words, and the waves pull blocks through the counter behind them */
            HIPCHK(c, hipMemsetAsync(c->b_done.p, 0, done_bytes, c->stream));
        if ((rc = launch_mega(c, P, p->integrator, trav, false, nullptr, p->flags, &c->stats.flags_in_effect, &launched))) return rc;
        c->last_kernel = rtr_debug_kernel{pipeline, p->integrator, launched.trav, launched.ms, launched.sorted, 0, 0, 0, 0, 0, 0,
                                          acc ? (acc->moments ? 2 : 1) : 0, launched.pair, launched.queue};
        if (acc) {
            hipLaunchKernelGGL(k_accum_commit, dim3((unsigned)P.n_tiles), dim3(RTR_BLOCK), 0, c->stream, P,
                               static_cast<double*>(acc->d_sum.p), static_cast<double*>(acc->moments ? acc->d_q.p : nullptr),
                               static_cast<int*>(acc->d_count.p));
        } else {
            ResolveK R{P, d_rgb, (long long)row_stride, tile_done, queue ? RTR_BLOCK : 0};
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
    int chunks = 1, guided[3];
    if (int rc = choose_chunks(c, P, p->integrator, pipeline, pick_trav(c->facts, c->info, p->flags), p->spp, p->flags, &chunks, guided)) return rc;
    return chunks;
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
    if (!rc && n) {
        hipError_t e = hipMemsetAsync(a->d_sum.p, 0, n * 3 * RTR_BLOCK * sizeof(double), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(a->d_count.p, 0, n * sizeof(int), c->stream);
        if (e == hipSuccess && a->moments) e = hipMemsetAsync(a->d_q.p, 0, n * RTR_BLOCK * sizeof(double), c->stream);
        if (e != hipSuccess) rc = fail(c, RTR_ERR_DEVICE, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
    }
    if (rc) {
        free_accum(a);
        return rc;
    }
    c->accums.push_back(a);
    *out = a;
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
    if (!behind) { /* every tile is there: nothing to do, and the statistics of this call are all zero */
        if (int rc = finish_stats(c)) return rc;
        c->stats = rtr_render_stats{};
        return RTR_OK;
    }
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
    if (!behind) {
        if (int rc = finish_stats(c)) return rc;
        c->stats = rtr_render_stats{};
        return RTR_OK;
    }
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

} // extern "C"

/* ---- first-hit features and the a-trous denoiser ------------------------------------------------------------------ */
namespace {

/* the defaults of rtr_denoise_defaults: the sweep of INTEGRATION.md section 4, "Denoising" */
constexpr rtr_denoise_params kDenoiseDefaults = {4, 8, 16.0, 0.2, 0.3, 1.0, {0.0, 0.0, 0.0, 0.0}};

int denoise_check(rtr_context* c, const rtr_denoise_params* p) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null denoise params");
    if (p->iterations < 0 || p->iterations > 10) return fail(c, RTR_ERR_INVALID, "iterations must be in 0..10");
    if (p->feature_spp < 1) return fail(c, RTR_ERR_INVALID, "feature_spp must be >= 1");
    for (double s : {p->sigma_l, p->sigma_n, p->sigma_a, p->sigma_z})
        if (!(s > 0.0) || !std::isfinite(s)) return fail(c, RTR_ERR_INVALID, "the sigmas must be finite and > 0");
    for (double r : p->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    return RTR_OK;
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
    if (!dispatch_trav(PerRayTravs{}, trav, [&](auto t) {
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

/* the planes of a w x h region in c->b_denoise */
int denoise_planes(rtr_context* c, int w, int h, const rtr_denoise_params* prm, DenoiseK& D) {
    const size_t np = (size_t)w * h;
    /* doubles: m 3, q 1, feat 7, c 3 + 3, v 1 + 1, a 3, nrm 3, z 1, out 3; then n (int) and rgb8 (3 bytes) */
    const size_t n_doubles = 29 * np;
    if (int rc = ensure_behind_queue(c, c->b_denoise, n_doubles * sizeof(double) + np * sizeof(int) + 3 * np)) return rc;
    double* d = static_cast<double*>(c->b_denoise.p);
    D = DenoiseK{};
    D.w = w, D.h = h, D.iterations = prm->iterations;
    D.sl2 = prm->sigma_l * prm->sigma_l, D.sn2 = prm->sigma_n * prm->sigma_n;
    D.sa2 = prm->sigma_a * prm->sigma_a, D.sz2 = prm->sigma_z * prm->sigma_z;
    D.m = d, d += 3 * np;
    D.q = d, d += np;
    D.feat = d, d += RTR_FEAT * np;
    D.c[0] = d, d += 3 * np;
    D.c[1] = d, d += 3 * np;
    D.v[0] = d, d += np;
    D.v[1] = d, d += np;
    D.a = d, d += 3 * np;
    D.nrm = d, d += 3 * np;
    D.z = d, d += np;
    D.out = d, d += 3 * np;
    D.n = reinterpret_cast<int*>(d);
    D.rgb8 = reinterpret_cast<unsigned char*>(D.n + np);
    return RTR_OK;
}

/* where a denoise call's outputs go: HOST buffers (the library's planes, a copy, a wait and a per-pixel loop on the CPU)
 * or, with `device`, the caller's DEVICE buffers, written by k_denoise_out itself with nothing after it on the host */
struct DenoiseOut {
    double* linear;
    int64_t row_stride;
    uint8_t* rgb8;
    bool device;
    int blocking; /* device only */
};

/* prep, the passes and the output on the filled input planes; then the valid pixels into the caller's buffers (linear:
 * row r at linear + r * row_stride * 3; 8-bit: rows of w pixels, the top row first).  With `T` the temporal blend and
 * the history write-back take the place of the prep (rtr_accum_denoise_temporal). */
int denoise_run(rtr_context* c, DenoiseK D, const DenoiseOut& O, const TemporalK* T = nullptr) {
    double* const h_linear = O.linear;
    uint8_t* const h_rgb8 = O.rgb8;
    const size_t np = (size_t)D.w * D.h;
    const dim3 grid1((unsigned)((np + RTR_BLOCK - 1) / RTR_BLOCK)), grid2((unsigned)((D.w + 15) / 16), (unsigned)((D.h + 15) / 16));
    if (!h_linear) D.out = nullptr;
    if (!h_rgb8) D.rgb8 = nullptr;
    const int64_t row_stride = O.device ? O.row_stride : D.w; /* of D.out: the host forms read the library's plane */
    if (O.device) D.out = O.linear, D.rgb8 = O.rgb8;
    if (T) {
        hipLaunchKernelGGL(k_temporal_blend, grid2, dim3(RTR_BLOCK), 0, c->stream, D, *T);
        hipLaunchKernelGGL(k_temporal_store, grid1, dim3(RTR_BLOCK), 0, c->stream, D, *T);
    } else {
        hipLaunchKernelGGL(k_denoise_prep, grid1, dim3(RTR_BLOCK), 0, c->stream, D);
    }
    int src = 0;
    /* steps 1 and 2 from LDS unless RTR_DENOISE_LDS=0 (A/B measurement: INTEGRATION.md section 4, "Denoising") */
    const char* lds_env = getenv("RTR_DENOISE_LDS");
    const bool lds = !(lds_env && lds_env[0] == '0');
    for (int k = 0; k < D.iterations; ++k, src ^= 1) {
        if (lds && k == 0)
            hipLaunchKernelGGL(k_denoise_pass_lds<1>, grid2, dim3(RTR_BLOCK), 0, c->stream, D, src);
        else if (lds && k == 1)
            hipLaunchKernelGGL(k_denoise_pass_lds<2>, grid2, dim3(RTR_BLOCK), 0, c->stream, D, src);
        else
            hipLaunchKernelGGL(k_denoise_pass, grid2, dim3(RTR_BLOCK), 0, c->stream, D, 1 << k, src);
    }
    hipLaunchKernelGGL(k_denoise_out, grid1, dim3(RTR_BLOCK), 0, c->stream, D, src, (long long)row_stride);
    HIPCHK(c, hipGetLastError());
    if (O.device) { /* D.n decided on the device which pixels were written */
        if (O.blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
        return RTR_OK;
    }
    std::vector<int> n(np);
    std::vector<double> lin(h_linear ? 3 * np : 0);
    std::vector<unsigned char> rgb(h_rgb8 ? 3 * np : 0);
    HIPCHK(c, hipMemcpyAsync(n.data(), D.n, np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (h_linear) HIPCHK(c, hipMemcpyAsync(lin.data(), D.out, 3 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_rgb8) HIPCHK(c, hipMemcpyAsync(rgb.data(), D.rgb8, 3 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int y = 0; y < D.h; ++y)
        for (int x = 0; x < D.w; ++x) {
            const size_t p = (size_t)y * D.w + x;
            if (n[p] == 0) continue;
            if (h_linear) std::memcpy(h_linear + ((size_t)y * (size_t)O.row_stride + x) * 3, &lin[3 * p], 3 * sizeof(double));
            if (h_rgb8) {
                const size_t o = ((size_t)(D.h - 1 - y) * D.w + x) * 3;
                h_rgb8[o] = rgb[o], h_rgb8[o + 1] = rgb[o + 1], h_rgb8[o + 2] = rgb[o + 2];
            }
        }
    return RTR_OK;
}

/* the defaults of rtr_temporal_defaults ("Camera updates and temporal reprojection") */
constexpr rtr_temporal_params kTemporalDefaults = {0.05, 0.1, 0.25, 0.25, {0.0, 0.0, 0.0, 0.0}};

int temporal_check(rtr_context* c, const rtr_temporal_params* t) {
    if (!t) return fail(c, RTR_ERR_INVALID, "null temporal params");
    if (!(t->alpha_min > 0.0 && t->alpha_min <= 1.0)) return fail(c, RTR_ERR_INVALID, "alpha_min must be in (0, 1]");
    if (!(t->tau_z > 0.0) || !std::isfinite(t->tau_z) || !(t->tau_n > 0.0) || !std::isfinite(t->tau_n))
        return fail(c, RTR_ERR_INVALID, "tau_z and tau_n must be finite and > 0");
    if (!(t->min_weight > 0.0 && t->min_weight < 1.0)) return fail(c, RTR_ERR_INVALID, "min_weight must be in (0, 1)");
    for (double r : t->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    return RTR_OK;
}

int history_check(rtr_context* c, const rtr_history* h) {
    if (!h) return fail(c, RTR_ERR_INVALID, "null history");
    if (h->ctx != c) return fail(c, RTR_ERR_INVALID, "the history belongs to another context");
    return RTR_OK;
}

/* rtr_accum_denoise, and with `hist` rtr_accum_denoise_temporal: ONE list of checks, all before any device work; then
 * features, gather and the filter, with the temporal stage in the prep's place */
int accum_denoise(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, rtr_history* hist, const rtr_temporal_params* tp,
                  const DenoiseOut& O) {
    double* const h_linear = O.linear;
    uint8_t* const h_rgb8 = O.rgb8;
    const int64_t row_stride = O.row_stride;
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (int rc = denoise_check(c, prm)) return rc;
    if (hist)
        if (int rc = temporal_check(c, tp)) return rc;
    if (!a->moments) return fail(c, RTR_ERR_INVALID, "the accumulator keeps no moments (RTR_ACCUM_MOMENTS)");
    const rtr_render_params& p = a->params;
    const int w = p.x1 - p.x0, h = p.y1 - p.y0;
    if (!h_linear && !h_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    if (h_linear && row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad output stride");
    if (O.device && reinterpret_cast<uintptr_t>(h_linear) % sizeof(double))
        return fail(c, RTR_ERR_INVALID, "d_linear is not 8-byte aligned");
    if (p.tile_stride > 1)
        return fail(c, RTR_ERR_UNSUPPORTED, hist ? "a tile-sharded accumulator: temporal denoising is single-context"
                                                 : "a tile-sharded accumulator: gather the shards and call rtr_denoise_host");
    if (hist) {
        if (int rc = history_check(c, hist)) return rc;
        if (hist->W != p.image_width || hist->H != p.image_height || hist->x0 != p.x0 || hist->y0 != p.y0 || hist->x1 != p.x1 ||
            hist->y1 != p.y1)
            return fail(c, RTR_ERR_INVALID, "the history was created for another image size or region");
    }
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (O.device)
        (void)hipGetLastError();
    else if (int rc = refresh_counts(c, a)) /* (the device forms leave the counts where they are: k_denoise_gather reads them) */
        return rc;
    if (int rc = accum_features(c, a, prm->feature_spp)) return rc;
    DenoiseK D;
    if (int rc = denoise_planes(c, w, h, prm, D)) return rc;
    hipLaunchKernelGGL(k_denoise_gather, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, accum_view(a),
                       static_cast<const double*>(a->d_q.p), static_cast<const double*>(a->d_feat.p), D);
    HIPCHK(c, hipGetLastError());
    if (!hist) return denoise_run(c, D, O);
    TemporalK T{};
    T.cam = c->ds.camera, T.prev = hist->cam;
    T.W = p.image_width, T.H = p.image_height, T.x0 = p.x0, T.y0 = p.y0;
    T.have = hist->have ? 1 : 0;
    T.alpha_min = tp->alpha_min, T.tau_z = tp->tau_z, T.tau_n = tp->tau_n, T.min_weight = tp->min_weight;
    T.hist_in = static_cast<const double*>(hist->d_planes[hist->cur].p);
    T.hist_out = static_cast<double*>(hist->d_planes[hist->cur ^ 1].p);
    T.mom = static_cast<double*>(hist->d_mom.p);
    if (int rc = denoise_run(c, D, O, &T)) return rc;
    hist->cur ^= 1, hist->have = true, hist->cam = c->ds.camera; /* the write-back counts once the frame has finished */
    return RTR_OK;
}

} // namespace

extern "C" {

void rtr_denoise_defaults(rtr_denoise_params* p) {
    if (p) *p = kDenoiseDefaults;
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

int rtr_accum_denoise(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, double* h_linear, int64_t row_stride,
                      uint8_t* h_rgb8) {
    return accum_denoise(c, a, prm, nullptr, nullptr, DenoiseOut{h_linear, row_stride, h_rgb8, false, 1});
}

int rtr_accum_denoise_device(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, double* d_linear, int64_t row_stride,
                             uint8_t* d_rgb8, int blocking) {
    return accum_denoise(c, a, prm, nullptr, nullptr, DenoiseOut{d_linear, row_stride, d_rgb8, true, blocking});
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

int rtr_denoise_host(rtr_context* c, const rtr_denoise_params* prm, int32_t width, int32_t height, const double* h_color,
                     const double* h_q, const int32_t* h_count, const double* h_feat, double* h_linear, uint8_t* h_rgb8) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = denoise_check(c, prm)) return rc;
    if (width < 1 || height < 1 || (int64_t)width * height > ((int64_t)1 << 28))
        return fail(c, RTR_ERR_INVALID, "region size out of range");
    if (!h_color || !h_q || !h_count || !h_feat) return fail(c, RTR_ERR_INVALID, "null input plane");
    if (!h_linear && !h_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    const size_t np = (size_t)width * height;
    for (size_t p = 0; p < np; ++p)
        if (h_count[p] < 0) return fail(c, RTR_ERR_INVALID, "negative sample count");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DenoiseK D;
    if (int rc = denoise_planes(c, width, height, prm, D)) return rc;
    HIPCHK(c, hipMemcpy(D.m, h_color, 3 * np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.q, h_q, np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.n, h_count, np * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.feat, h_feat, RTR_FEAT * np * sizeof(double), hipMemcpyHostToDevice));
    return denoise_run(c, D, DenoiseOut{h_linear, width, h_rgb8, false, 1});
}

void rtr_accum_destroy(rtr_accum* a) {
    if (!a) return;
    rtr_context* c = a->ctx;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream); /* a pass may still use the buffers */
    for (size_t k = 0; k < c->accums.size(); ++k)
        if (c->accums[k] == a) {
            c->accums.erase(c->accums.begin() + (long)k);
            break;
        }
    free_accum(a);
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
    int trav = per_ray_trav(c->facts, c->info, p->flags, false);
    const size_t lds = stack_bytes(c->facts, c->info, trav);
    const dim3 grid((unsigned)((n + RTR_BLOCK - 1) / RTR_BLOCK));
    /* integrators 0 / 2 / 3: the media kernel also serves the reference-order traversal */
    const bool n1 = p->integrator != RTR_INTEGRATOR_MIS && p->integrator != RTR_INTEGRATOR_RR;
    if (n1 && trav == RT_TRAV_EXACT) trav = RT_TRAV_MEDIA;
    auto launch = [&](auto integ, auto travs) {
        constexpr int I = decltype(integ)::value;
        return dispatch_trav(travs, trav, [&](auto t) {
            constexpr int T = decltype(t)::value;
            if ((rc = set_lds(c, k_li<I, T>, lds))) return;
            hipLaunchKernelGGL((k_li<I, T>), grid, dim3(RTR_BLOCK), lds, c->stream, c->ds, P, d_ijs, d_rays, d_out, (long long)n);
        });
    };
    using TravsN1 = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA>;
    bool found;
    switch (p->integrator) {
    case RTR_INTEGRATOR_MIS: found = launch(std::integral_constant<int, RTR_INTEGRATOR_MIS>{}, PerRayTravs{}); break;
    case RTR_INTEGRATOR_RR: found = launch(std::integral_constant<int, RTR_INTEGRATOR_RR>{}, PerRayTravs{}); break;
    case RTR_INTEGRATOR_PATH: found = launch(std::integral_constant<int, RTR_INTEGRATOR_PATH>{}, TravsN1{}); break;
    case RTR_INTEGRATOR_PBR: found = launch(std::integral_constant<int, RTR_INTEGRATOR_PBR>{}, TravsN1{}); break;
    default: found = launch(std::integral_constant<int, RTR_INTEGRATOR_NEE>{}, TravsN1{}); break;
    }
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
    /* mega_variant's choice for MIS / RR: a flat scene keeps RT_TRAV_FLAT, a guarded one takes its kernel unless a top tree does */
    const int picked = pick_trav(c->facts, c->info, flags);
    v->flat_trav = picked == RT_TRAV_FLAT ? RT_TRAV_FLAT
                   : (picked == RT_TRAV_FAST && c->facts.flat_guarded && !c->facts.top_tree ? RT_TRAV_FLAT_GUARD : -1);
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
int rtr_debug_last_gather(rtr_context* c, rtr_debug_gather* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_gather)) return RTR_ERR_INVALID;
    *out = rtr_debug_gather{c->last_gather.integ, c->last_gather.trav, c->last_gather.broadcast, c->last_gather.lg};
    return RTR_OK;
}
int rtr_debug_last_kernel(rtr_context* c, rtr_debug_kernel* out, size_t size) {
    if (!c || !out || size != sizeof(rtr_debug_kernel)) return RTR_ERR_INVALID;
    *out = c->last_kernel;
    return RTR_OK;
}
int rtr_debug_li(rtr_context* c, const rtr_render_params* p, const int32_t* ijs, rtr_debug_li_out* out, int64_t n) {
    static_assert(sizeof(rtr_debug_li_out) == sizeof(LiOut), "one layout");
    if (n < 0 || (n > 0 && (!ijs || !out))) return RTR_ERR_INVALID;
    return li_run(c, p, ijs, nullptr, reinterpret_cast<LiOut*>(out), n);
}
void rtr_debug_set_error(rtr_context* c, const char* msg) {
    if (c) c->err = msg ? msg : "";
}

} /* extern "C" */

/* ---- ray queries: hittable::hit of the scene root for caller-given rays ----------------------------------------- */
namespace {

constexpr int64_t kQuerySlice = (int64_t)1 << 22; /* rays per slice of the host entries */

/* what every query entry checks before any device work */
int query_check(rtr_context* c, const void* rays, const void* out, int64_t n, int32_t flags) {
    if (!c) return RTR_ERR_INVALID;
    if (flags & ~RTR_FLAG_REFERENCE_ORDER) return fail(c, RTR_ERR_INVALID, "rtr_query_*: unknown flag bits");
    if (n < 0 || (n > 0 && (!rays || !out))) return fail(c, RTR_ERR_INVALID, "rtr_query_*: negative n or NULL array");
    if (!c->has_scene) return fail(c, RTR_ERR_NO_SCENE, "rtr_query_* before rtr_upload_scene");
    return RTR_OK;
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
    if (!dispatch_trav(PerRayTravsTop{}, trav, [&](auto t) { staged ? launch(t, std::true_type{}) : launch(t, std::false_type{}); }))
        return no_per_ray_kernel(c, trav);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return RTR_OK;
}

/* the host entries: slices of at most kQuerySlice rays through c->b_query, everything stream-ordered on the context
 * stream (behind a render that is still running; its workspace, statistics and events are not touched) */
int query_host(rtr_context* c, const rtr_ray* rays, rtr_ray_hit* hits, uint8_t* occ, uint32_t* rng_out, int64_t n, int flags) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError(); /* a launch error of an earlier call is not this call's */
    const int64_t slice = std::min(n, kQuerySlice);
    const size_t in_bytes = (size_t)slice * sizeof(rtr_ray);
    const size_t out_bytes = hits ? (size_t)slice * sizeof(rtr_ray_hit) : (size_t)slice * sizeof(uint32_t);
    const size_t occ_bytes = hits ? 0 : (((size_t)slice + 15) & ~(size_t)15);
    if (int rc = ensure(c, c->b_query, in_bytes + out_bytes + occ_bytes)) return rc;
    char* base = static_cast<char*>(c->b_query.p);
    rtr_ray* d_rays = reinterpret_cast<rtr_ray*>(base);
    rtr_ray_hit* d_hits = hits ? reinterpret_cast<rtr_ray_hit*>(base + in_bytes) : nullptr;
    uint32_t* d_rng = hits ? nullptr : reinterpret_cast<uint32_t*>(base + in_bytes);
    uint8_t* d_occ = hits ? nullptr : reinterpret_cast<uint8_t*>(base + in_bytes + out_bytes);
    for (int64_t k0 = 0; k0 < n; k0 += slice) {
        const int64_t m = std::min(slice, n - k0);
        HIPCHK(c, hipMemcpyAsync(d_rays, rays + k0, (size_t)m * sizeof(rtr_ray), hipMemcpyHostToDevice, c->stream));
        if (int rc = query_launch(c, d_rays, d_hits, d_occ, d_rng, m, flags)) return rc;
        if (hits) {
            HIPCHK(c, hipMemcpyAsync(hits + k0, d_hits, (size_t)m * sizeof(rtr_ray_hit), hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPCHK(c, hipMemcpyAsync(occ + k0, d_occ, (size_t)m, hipMemcpyDeviceToHost, c->stream));
            if (rng_out) HIPCHK(c, hipMemcpyAsync(rng_out + k0, d_rng, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* the next slice reuses the buffer */
    }
    return RTR_OK;
}

int query_device(rtr_context* c, const rtr_ray* d_rays, rtr_ray_hit* d_hits, uint8_t* d_occ, uint32_t* d_rng, int64_t n, int flags,
                 int blocking) {
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    if (int rc = query_launch(c, d_rays, d_hits, d_occ, d_rng, n, flags)) return rc;
    if (blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTR_OK;
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

/* ---- hemisphere gathers: occlusion and radiance over the hemisphere at caller-given points (kernels: rtr_gather.hip) -- */
namespace {

constexpr int64_t kGatherSlice = (int64_t)1 << 20; /* points per slice of the host entries */

/* what every gather entry checks before any device work; `radiance`: rp is checked too (a NULL one is invalid) */
int gather_check(rtr_context* c, const rtr_render_params* rp, bool radiance, const rtr_gather_params* gp, const void* pts,
                 const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = rtr_gather_params_check(gp, c->err)) return rc;
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

/* launches over device arrays on the context stream */
int gather_launch(rtr_context* c, const rtr_render_params* rp, const rtr_gather_params* gp, uint32_t point_base,
                  const rtr_gather_point* d_pts, rtr_gather_out* d_out, int64_t n) {
    GatherLaunch L;
    L.ds = c->ds;
    L.integ = rp ? rp->integrator : -1;
    L.trav = per_ray_trav(c->facts, c->info, rp ? rp->flags : gp->flags, !rp);
    L.lds = stack_bytes(c->facts, c->info, L.trav);
    L.broadcast = gather_broadcast();
    L.stream = c->stream;
    if (!rp && !(gp->t_min >= 0x1p-100)) L.ds.shared_div = 0; /* the plain divisions, as k_query_* per wave */
    L.K = GatherK{d_pts, d_out, (long long)n, gp->samples, gather_lg(gp->samples), gp->seed, point_base, gp->time, gp->t_min,
                  gp->t_max, rp ? rp->max_depth : 0, rp ? rp->rr_start_depth : 0};
    return rtr_gather_launch(L, &c->last_gather, c->err);
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

} /* extern "C" */

/* ---- camera updates, accumulator reset, temporal reprojection (include/rtr_hip.h) --------------------------------- */
extern "C" {

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

int rtr_accum_reset(rtr_context* c, rtr_accum* a, uint32_t seed) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_check(c, a)) return rc;
    if (!c->has_scene || a->scene_gen != c->scene_gen)
        return fail(c, RTR_ERR_INVALID, "the scene changed since the accumulator was created (rtr_upload_scene)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* its queued passes */
    const size_t n = a->tiles.size();
    if (n) { /* what rtr_accum_create_ex leaves */
        HIPCHK(c, hipMemsetAsync(a->d_sum.p, 0, n * 3 * RTR_BLOCK * sizeof(double), c->stream));
        HIPCHK(c, hipMemsetAsync(a->d_count.p, 0, n * sizeof(int), c->stream));
        if (a->moments) HIPCHK(c, hipMemsetAsync(a->d_q.p, 0, n * RTR_BLOCK * sizeof(double), c->stream));
    }
    a->h_counts.assign(n, 0);
    a->counts_stale = false;
    a->feat_k = 0;
    a->params.seed = seed;
    a->camera_gen = c->camera_gen;
    return RTR_OK;
}

void rtr_temporal_defaults(rtr_temporal_params* p) {
    if (p) *p = kTemporalDefaults;
}

int rtr_history_create(rtr_context* c, const rtr_render_params* p, rtr_history** out) {
    if (!c) return RTR_ERR_INVALID;
    if (!out) return fail(c, RTR_ERR_INVALID, "null out");
    *out = nullptr;
    if (!p) return fail(c, RTR_ERR_INVALID, "null params");
    if (p->image_width < 2 || p->image_height < 2) return fail(c, RTR_ERR_INVALID, "image smaller than 2x2");
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->image_width || p->y1 > p->image_height || p->x0 >= p->x1 || p->y0 >= p->y1)
        return fail(c, RTR_ERR_INVALID, "region outside the image or empty");
    HIPCHK(c, hipSetDevice(c->device));
    rtr_history* h = new rtr_history();
    h->ctx = c;
    h->W = p->image_width, h->H = p->image_height;
    h->x0 = p->x0, h->y0 = p->y0, h->x1 = p->x1, h->y1 = p->y1;
    const size_t np = (size_t)(p->x1 - p->x0) * (size_t)(p->y1 - p->y0), bytes = np * RTR_HIST * sizeof(double);
    int rc = ensure(c, h->d_planes[0], bytes);
    if (!rc) rc = ensure(c, h->d_planes[1], bytes);
    if (!rc) rc = ensure(c, h->d_mom, np * 3 * sizeof(double));
    for (int k = 0; k < 2 && !rc; ++k)
        if (hipMemsetAsync(h->d_planes[k].p, 0, bytes, c->stream) != hipSuccess) rc = fail(c, RTR_ERR_DEVICE, "hipMemsetAsync of a history");
    if (rc) {
        free_history(h);
        return rc;
    }
    c->histories.push_back(h);
    *out = h;
    return RTR_OK;
}

int rtr_history_clear(rtr_context* c, rtr_history* h) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = history_check(c, h)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)(h->x1 - h->x0) * (size_t)(h->y1 - h->y0) * RTR_HIST * sizeof(double);
    for (DevBuf& b : h->d_planes) HIPCHK(c, hipMemsetAsync(b.p, 0, bytes, c->stream));
    h->have = false;
    h->cur = 0;
    h->cam = rtr_camera{};
    return RTR_OK;
}

void rtr_history_destroy(rtr_history* h) {
    if (!h) return;
    rtr_context* c = h->ctx;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream); /* a frame may still use the planes */
    for (size_t k = 0; k < c->histories.size(); ++k)
        if (c->histories[k] == h) {
            c->histories.erase(c->histories.begin() + (long)k);
            break;
        }
    free_history(h);
}

int rtr_history_planes(rtr_context* c, rtr_history* h, double* h_planes, int64_t row_stride) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = history_check(c, h)) return rc;
    const int w = h->x1 - h->x0, ht = h->y1 - h->y0;
    if (!h_planes || row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t row = (size_t)w * RTR_HIST * sizeof(double);
    HIPCHK(c, hipMemcpy2D(h_planes, (size_t)row_stride * RTR_HIST * sizeof(double), h->d_planes[h->cur].p, row, row, (size_t)ht,
                          hipMemcpyDeviceToHost));
    return RTR_OK;
}

int rtr_accum_denoise_temporal(rtr_context* c, rtr_accum* a, rtr_history* hist, const rtr_denoise_params* prm,
                               const rtr_temporal_params* tp, double* h_linear, int64_t row_stride, uint8_t* h_rgb8) {
    if (!c) return RTR_ERR_INVALID;
    if (!hist) return fail(c, RTR_ERR_INVALID, "null history");
    return accum_denoise(c, a, prm, hist, tp, DenoiseOut{h_linear, row_stride, h_rgb8, false, 1});
}

int rtr_accum_denoise_temporal_device(rtr_context* c, rtr_accum* a, rtr_history* hist, const rtr_denoise_params* prm,
                                      const rtr_temporal_params* tp, double* d_linear, int64_t row_stride, uint8_t* d_rgb8,
                                      int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (!hist) return fail(c, RTR_ERR_INVALID, "null history");
    return accum_denoise(c, a, prm, hist, tp, DenoiseOut{d_linear, row_stride, d_rgb8, true, blocking});
}

} /* extern "C" */

/* ---- the display transform: metered exposure, tone curve, 8-bit encoding ------------------------------------------- */
namespace {

/* the defaults of rtr_display_defaults: conventional values (median metering, 18 % grey key), not tuned ones */
constexpr rtr_display_params kDisplayDefaults = {0, 500, RTR_TONE_CLAMP, RTR_ENCODE_GAMMA2, 1.0, 0.18, 4.0, {0.0, 0.0, 0.0, 0.0, 0.0}};

int display_size_check(rtr_context* c, int32_t w, int32_t h, const void* linear, int64_t row_stride) {
    if (w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 28)) return fail(c, RTR_ERR_INVALID, "image size out of range");
    if (!linear || row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad input buffer / stride");
    return RTR_OK;
}

int display_check(rtr_context* c, const rtr_display_params* p, int32_t w, int32_t h, const void* linear, int64_t row_stride,
                  const void* rgb8, const void* mapped) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null display params");
    if (p->auto_exposure != 0 && p->auto_exposure != 1) return fail(c, RTR_ERR_INVALID, "auto_exposure must be 0 or 1");
    if (p->meter_permille < 1 || p->meter_permille > 1000) return fail(c, RTR_ERR_INVALID, "meter_permille must be in 1..1000");
    if (p->tone_curve < RTR_TONE_CLAMP || p->tone_curve > RTR_TONE_ACES) return fail(c, RTR_ERR_INVALID, "unknown tone curve");
    if (p->encoding != RTR_ENCODE_GAMMA2 && p->encoding != RTR_ENCODE_SRGB) return fail(c, RTR_ERR_INVALID, "unknown encoding");
    for (double v : {p->exposure, p->key, p->white})
        if (!(v > 0.0) || !std::isfinite(v)) return fail(c, RTR_ERR_INVALID, "exposure, key and white must be finite and > 0");
    for (double r : p->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    if (int rc = display_size_check(c, w, h, linear, row_stride)) return rc;
    if (!rgb8 && !mapped) return fail(c, RTR_ERR_INVALID, "no output buffer");
    return RTR_OK;
}

DisplayK display_view(rtr_context* c, const rtr_display_params* p, int w, int h, const double* d_linear, int64_t row_stride) {
    char* base = static_cast<char*>(c->b_display.p);
    DisplayK D{};
    D.w = w, D.h = h, D.row_stride = row_stride, D.in = d_linear;
    D.srgb = reinterpret_cast<const double*>(base);
    D.hist = reinterpret_cast<unsigned*>(base + kDisplayHistOff);
    D.rec = reinterpret_cast<DisplayRec*>(base + kDisplayRecOff);
    if (p) {
        D.auto_exposure = p->auto_exposure, D.permille = p->meter_permille, D.curve = p->tone_curve, D.encoding = p->encoding;
        D.exposure = p->exposure, D.key = p->key, D.white = p->white;
    }
    return D;
}

/* the histogram of D.in into D.hist, on the stream: the grid follows the region (RTR_DISPLAY_TRIPS pixels per lane) */
int display_meter(rtr_context* c, const DisplayK& D) {
    HIPCHK(c, hipMemsetAsync(D.hist, 0, RTR_DISPLAY_BINS * sizeof(unsigned), c->stream));
    const size_t np = (size_t)D.w * D.h, per_group = (size_t)RTR_BLOCK * RTR_DISPLAY_TRIPS;
    hipLaunchKernelGGL(k_display_meter, dim3((unsigned)((np + per_group - 1) / per_group)), dim3(RTR_BLOCK), 0, c->stream, D);
    return RTR_OK;
}

/* meter (with auto exposure only), scale, apply: all on the stream, no host wait */
int display_run(rtr_context* c, const DisplayK& D) {
    if (D.auto_exposure)
        if (int rc = display_meter(c, D)) return rc;
    hipLaunchKernelGGL(k_display_scale, dim3(1), dim3(64), 0, c->stream, D);
    const size_t np = (size_t)D.w * D.h;
    hipLaunchKernelGGL(k_display_apply, dim3((unsigned)((np + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), 0, c->stream, D);
    HIPCHK(c, hipGetLastError());
    return RTR_OK;
}

/* after the stream has been waited for */
int display_result(rtr_context* c, const DisplayK& D, rtr_display_result* out) {
    static_assert(sizeof(DisplayRec) == sizeof(rtr_display_result), "one layout");
    if (out) HIPCHK(c, hipMemcpy(out, D.rec, sizeof(DisplayRec), hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* the image of a host entry in c->b_display_io: [h][w][3] doubles in, [h][w][3] doubles mapped, [h][w][3] bytes */
int display_upload(rtr_context* c, int w, int h, const double* h_linear, int64_t row_stride, double*& d_in) {
    const size_t np = (size_t)w * h, row = (size_t)w * 3 * sizeof(double);
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = ensure(c, c->b_display_io, np * (6 * sizeof(double) + 3))) return rc;
    d_in = static_cast<double*>(c->b_display_io.p);
    HIPCHK(c, hipMemcpy2D(d_in, row, h_linear, (size_t)row_stride * 3 * sizeof(double), row, (size_t)h, hipMemcpyHostToDevice));
    return RTR_OK;
}

} // namespace

extern "C" {

void rtr_display_defaults(rtr_display_params* p) {
    if (p) *p = kDisplayDefaults;
}

void rtr_display_srgb_thresholds(double out[256]) {
    if (out) std::memcpy(out, display_srgb_table(), 256 * sizeof(double));
}

int rtr_display_histogram(rtr_context* c, int32_t width, int32_t height, const double* h_linear, int64_t row_stride,
                          uint32_t h_hist[512], int64_t* n_metered) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_size_check(c, width, height, h_linear, row_stride)) return rc;
    if (!h_hist) return fail(c, RTR_ERR_INVALID, "no output buffer");
    double* d_in = nullptr;
    if (int rc = display_upload(c, width, height, h_linear, row_stride, d_in)) return rc;
    const DisplayK D = display_view(c, nullptr, width, height, d_in, width);
    if (int rc = display_meter(c, D)) return rc;
    HIPCHK(c, hipGetLastError());
    uint32_t hist[RTR_DISPLAY_BINS];
    HIPCHK(c, hipMemcpyAsync(hist, D.hist, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t n = 0;
    for (int m = 0; m < RTR_DISPLAY_BINS; ++m) h_hist[m] = hist[m], n += hist[m];
    if (n_metered) *n_metered = n;
    return RTR_OK;
}

int rtr_display_host(rtr_context* c, const rtr_display_params* p, int32_t width, int32_t height, const double* h_linear,
                     int64_t row_stride, uint8_t* h_rgb8, double* h_mapped, rtr_display_result* result) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_check(c, p, width, height, h_linear, row_stride, h_rgb8, h_mapped)) return rc;
    double* d_in = nullptr;
    if (int rc = display_upload(c, width, height, h_linear, row_stride, d_in)) return rc;
    const size_t np = (size_t)width * height;
    DisplayK D = display_view(c, p, width, height, d_in, width);
    if (h_mapped) D.mapped = d_in + 3 * np;
    if (h_rgb8) D.rgb8 = reinterpret_cast<unsigned char*>(d_in + 6 * np);
    if (int rc = display_run(c, D)) return rc;
    if (h_mapped) HIPCHK(c, hipMemcpyAsync(h_mapped, D.mapped, 3 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_rgb8) HIPCHK(c, hipMemcpyAsync(h_rgb8, D.rgb8, 3 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return display_result(c, D, result);
}

int rtr_display_device(rtr_context* c, const rtr_display_params* p, int32_t width, int32_t height, const double* d_linear,
                       int64_t row_stride, uint8_t* d_rgb8, double* d_mapped, rtr_display_result* h_result, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_check(c, p, width, height, d_linear, row_stride, d_rgb8, d_mapped)) return rc;
    if (h_result && !blocking) return fail(c, RTR_ERR_INVALID, "a result needs a blocking call");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    DisplayK D = display_view(c, p, width, height, d_linear, row_stride);
    D.mapped = d_mapped, D.rgb8 = d_rgb8;
    if (int rc = display_run(c, D)) return rc;
    if (!blocking) return RTR_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return display_result(c, D, h_result);
}

} /* extern "C" */
