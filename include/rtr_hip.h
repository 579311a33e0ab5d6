/*
 * rtr_hip.h -- C ABI of the MI355X (gfx950) path tracer.
 *
 * This is the drop-in boundary for ONE hot path of JiGuang283/Ray_Tracing-Rendering:
 * the tile-threaded integrator loop behind
 *     void Renderer::render(shared_ptr<hittable> world, shared_ptr<camera> cam,
 *                           const color& background, RenderBuffer& target,
 *                           const std::vector<shared_ptr<Light>>& lights)
 * (reference src/renderer/renderer.h:30-102).  The reference has no C plugin ABI;
 * the entry points below are what an FFI for that call would bind.  Plain
 * pointers and sizes only: no C++ types, no torch types.
 *
 * Data model: the caller flattens the (immutable) scene graph into the POD
 * arrays of `rtr_scene_desc`, uploads it once, then asks for linear mean
 * radiance of a pixel region.  The host applies the reference's gamma-2 /
 * clamp store (renderer.h:126-140) itself.
 *
 * All scene quantities are IEEE double, like the reference (core/vec3.h:88).
 * All functions return RTR_OK (0) or a negative rtr_status; the text of the
 * last failure of a context is available from rtr_last_error().  No exception
 * crosses this boundary.
 */
#ifndef RTR_HIP_H
#define RTR_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTR_ABI_VERSION 4 /* 2: rtr_render_stats grew spp_chunks / cancelled; 3: ... flags_in_effect; 4: the accumulator
                             entry points rtr_accum_* (no struct changed) */

/* ------------------------------------------------------------------------- */
/* status codes                                                              */
typedef enum rtr_status {
    RTR_OK = 0,
    RTR_ERR_INVALID = -1,     /* bad argument / malformed scene            */
    RTR_ERR_UNSUPPORTED = -2, /* scene uses a node/material the device lacks */
    RTR_ERR_DEVICE = -3,      /* HIP runtime error                           */
    RTR_ERR_NO_SCENE = -4,    /* render before upload                        */
    RTR_ERR_CANCELLED = -5,   /* rtr_cancel() observed (partial image)       */
    RTR_ERR_NOMEM = -6
} rtr_status;

/* ------------------------------------------------------------------------- */
/* flattened scene graph                                                     */

/* hittable nodes: one record per object of the reference's hittable graph
 * (geometry/hittable.h:25-32).  Indices refer to rtr_scene_desc.nodes.
 * The graph may be a DAG (bvh_node with left == right, bvh.h:68-69; a sphere
 * that is both a world object and a medium boundary, scenes.cpp:255-258). */
typedef enum rtr_node_type {
    RTR_NODE_BVH = 0,           /* bvh_node        geometry/bvh.h:12-31        a=left b=right f[0..5]=box min,max */
    RTR_NODE_LIST = 1,          /* hittable_list   geometry/hittable_list.h    a=first (into list_children) b=count */
    RTR_NODE_TRANSLATE = 2,     /* translate       geometry/hittable.h:34-73   a=child f[0..2]=offset */
    RTR_NODE_ROTATE_Y = 3,      /* rotate_y        geometry/hittable.h:75-156  a=child f[0]=sin f[1]=cos */
    RTR_NODE_FLIP_FACE = 4,     /* flip_face       geometry/hittable.h:158-179 a=child */
    RTR_NODE_MEDIUM = 5,        /* constant_medium geometry/constant_medium.h  a=boundary b=phase material f[0]=neg_inv_density */
    RTR_NODE_SPHERE = 6,        /* sphere          geometry/sphere.h           a=material f[0..2]=center f[3]=radius */
    RTR_NODE_MOVING_SPHERE = 7, /* moving_sphere   geometry/moving_sphere.h    a=material f[0..2]=c0 f[3..5]=c1 f[6]=t0 f[7]=t1 f[8]=radius */
    RTR_NODE_XY_RECT = 8,       /* xy_rect         geometry/aarect.h:10-32     a=material f[0]=x0 f[1]=x1 f[2]=y0 f[3]=y1 f[4]=k */
    RTR_NODE_XZ_RECT = 9,       /* xz_rect         geometry/aarect.h:34-54     a=material f[0]=x0 f[1]=x1 f[2]=z0 f[3]=z1 f[4]=k */
    RTR_NODE_YZ_RECT = 10,      /* yz_rect         geometry/aarect.h:56-76     a=material f[0]=y0 f[1]=y1 f[2]=z0 f[3]=z1 f[4]=k */
    RTR_NODE_TYPE_COUNT = 11
} rtr_node_type;

typedef struct rtr_node {
    int32_t type; /* rtr_node_type */
    int32_t a;
    int32_t b;
    int32_t reserved;
    double f[10];
} rtr_node; /* 96 bytes */

/* materials (materials/material.h:72-439, geometry/constant_medium.h:12-29) */
typedef enum rtr_material_type {
    RTR_MAT_LAMBERTIAN = 0,    /* tex[0]=albedo */
    RTR_MAT_METAL = 1,         /* f[0..2]=albedo f[3]=fuzz (already clamped <=1) */
    RTR_MAT_DIELECTRIC = 2,    /* f[0]=ir */
    RTR_MAT_DIFFUSE_LIGHT = 3, /* tex[0]=emit */
    RTR_MAT_PBR = 4,           /* tex[0]=albedo tex[1]=roughness tex[2]=metallic tex[3]=normal_map or -1 */
    RTR_MAT_ISOTROPIC = 5,     /* tex[0]=albedo */
    RTR_MAT_TYPE_COUNT = 6
} rtr_material_type;

typedef struct rtr_material {
    int32_t type;
    int32_t tex[4];
    int32_t reserved[3];
    double f[4];
} rtr_material; /* 64 bytes */

/* textures (materials/texture.h:11-162) */
typedef enum rtr_texture_type {
    RTR_TEX_SOLID = 0,   /* f[0..2]=color */
    RTR_TEX_CHECKER = 1, /* a=even texture b=odd texture */
    RTR_TEX_NOISE = 2,   /* a=perlin table index f[0]=scale */
    RTR_TEX_IMAGE = 3,   /* a=image index, or -1 = file missing (cyan fallback, texture.h:116-118) */
    RTR_TEX_TYPE_COUNT = 4
} rtr_texture_type;

typedef struct rtr_texture {
    int32_t type;
    int32_t a;
    int32_t b;
    int32_t reserved;
    double f[4];
} rtr_texture; /* 48 bytes */

/* perlin noise tables (materials/perlin.h:10-19,57-60) */
typedef struct rtr_perlin {
    double ranvec[256][3];
    int32_t perm_x[256];
    int32_t perm_y[256];
    int32_t perm_z[256];
} rtr_perlin; /* 9216 bytes */

/* 8-bit RGB images for image_texture (materials/texture.h:96-107); image_bytes also holds the
 * float texels and sampling tables of RTR_LIGHT_ENV_MAP lights */
typedef struct rtr_image {
    int32_t width;
    int32_t height;
    uint64_t offset; /* byte offset of texel (0,0) in rtr_scene_desc.image_bytes, rows of 3*width bytes */
} rtr_image;

/* lights (lighting/light.h:15-47) */
typedef enum rtr_light_type {
    RTR_LIGHT_QUAD = 0,        /* QuadLight lighting/quad_light.h:9-92: f[0..2]=Q f[3..5]=u f[6..8]=v f[9..11]=intensity f[12..14]=normal f[15]=area */
    RTR_LIGHT_POINT = 1,       /* PointLight lighting/point_light.h:6-37: f[0..2]=position f[3..5]=intensity */
    RTR_LIGHT_SPOT = 2,        /* SpotLight lighting/spot_light.h:6-41: f[0..2]=position f[3..5]=unit direction f[6..8]=intensity f[9]=cos_cutoff */
    RTR_LIGHT_DIRECTIONAL = 3, /* DirectionalLight lighting/directional_light.h:7-31: f[0..2]=unit direction f[3..5]=radiance */
    RTR_LIGHT_ENV_UNIFORM = 4, /* EnvironmentLight whose map file is missing (lighting/environmental_light.h:126-131,
                                  187-192,251-252,293-294): uniform white sky, sampled with random_unit_vector() */
    RTR_LIGHT_ENV_MAP = 5,     /* EnvironmentLight with its HDR map (lighting/environmental_light.h:120-374):
                                  f[0]=width f[1]=height f[2]=is_light_probe (square map = angular probe, :137-140)
                                  f[3]=byte offset in rtr_scene_desc.image_bytes of the float32 RGB texels as stbi_loadf
                                       returns them (row 0 first, 3*width floats per row; multiple of 4)
                                  f[4]=byte offset (multiple of 8) of the float64 sampling tables of Distribution2D
                                       (:60-117): per map row v {func[width], cdf[width+1], func_int}, then the
                                       marginal {func[height], cdf[height+1], func_int} */
    RTR_LIGHT_TYPE_COUNT = 6
} rtr_light_type;

typedef struct rtr_light {
    int32_t type;
    int32_t reserved;
    double f[16];
} rtr_light; /* 136 bytes */

/* thin-lens camera, the private state of renderer/camera.h:43-50 */
typedef struct rtr_camera {
    double origin[3];
    double lower_left_corner[3];
    double horizontal[3];
    double vertical[3];
    double u[3];
    double v[3];
    double w[3];
    double lens_radius;
    double time0;
    double time1;
} rtr_camera; /* 192 bytes */

typedef struct rtr_scene_desc {
    uint32_t abi_version; /* RTR_ABI_VERSION */
    int32_t root;         /* node index of `world` */
    int32_t n_nodes;
    int32_t n_list_children;
    int32_t n_materials;
    int32_t n_textures;
    int32_t n_perlin;
    int32_t n_images;
    int32_t n_lights;
    int32_t reserved;
    uint64_t n_image_bytes;
    const rtr_node* nodes;
    const int32_t* list_children; /* node indices, hittable_list order */
    const rtr_material* materials;
    const rtr_texture* textures;
    const rtr_perlin* perlin;
    const rtr_image* images;
    const uint8_t* image_bytes;
    const rtr_light* lights;
    rtr_camera camera;
    double background[3];
} rtr_scene_desc;

/* ------------------------------------------------------------------------- */
/* render request                                                            */

/* integrator ids follow the reference CLI (main.cpp:52,78-100) */
#define RTR_INTEGRATOR_PATH 0 /* PathIntegrator        renderer/path_integrator.h:22-44 (summed front to back on the device) */
#define RTR_INTEGRATOR_RR 1   /* RRPathInterator       renderer/rr_path_integrator.h:21-59  */
#define RTR_INTEGRATOR_PBR 2  /* PBRPathIntegrator     renderer/pbr_path_integrator.h:21-73 */
#define RTR_INTEGRATOR_NEE 3  /* DirectLightIntegrator renderer/direct_light_integrator.h:25-142 */
#define RTR_INTEGRATOR_MIS 4  /* MISPathIntegrator     renderer/mis_path_integrator.h:25-150 */

/* device pipeline selection */
#define RTR_PIPELINE_AUTO 0       /* the megakernel (the faster one on every measured scene: DESIGN.md 4.4) */
#define RTR_PIPELINE_MEGAKERNEL 1 /* one lane per pixel, in-register bounce loop     */
#define RTR_PIPELINE_WAVEFRONT 2  /* SoA path pool in HBM, extend/shade/connect stages over live-block lists; all five
                                     integrators; compiled traversals only (RTR_ERR_UNSUPPORTED for graphs that need the
                                     reference-order walk -- e.g. a list holding a medium under a transform -- or with
                                     RTR_FLAG_REFERENCE_ORDER; hollow spheres and a medium straight under transforms are
                                     compiled) */

typedef struct rtr_render_params {
    int32_t image_width;  /* W of the full image (pixel (i,j), j=0 is the bottom row, renderer.h:69-74) */
    int32_t image_height; /* H */
    int32_t x0, y0;       /* region [x0,x1) x [y0,y1) to render                        */
    int32_t x1, y1;
    int32_t spp;          /* Renderer::set_samples (renderer.h:104)                    */
    int32_t max_depth;    /* Integrator::set_max_depth, reference uses 50 (main.cpp:102) */
    int32_t rr_start_depth; /* 3 (mis_path_integrator.h:237)                           */
    int32_t integrator;   /* RTR_INTEGRATOR_*                                          */
    uint32_t seed;        /* render seed; per-sample xorshift32 state = rtr_sample_seed() */
    int32_t pipeline;     /* RTR_PIPELINE_*                                            */
    /* tile sharding (renderer.h:40-62): the image is cut in 16x16 tiles, numbered in
     * the reference's dispatch order; this call renders the tiles with
     * index % tile_stride == tile_first that intersect the region.  tile_stride <= 1
     * renders every tile. */
    int32_t tile_first;
    int32_t tile_stride;
    /* The spp samples of a pixel may be summed as `spp_chunks` consecutive partial sums that
     * are then added in order (more parallelism on small images).  1 = one running sum in
     * sample order, exactly like renderer.h:72-79; 0 = let the library choose.  The library's choice depends on
     * the GPU, on the scene's kernel variant and on how many tiles the call owns, so with 0 the same image rendered
     * as ONE call, or tile-sharded over N contexts, or on another device agrees within 1e-13 relative (another
     * summation order) but not bit for bit; with 1, or any explicit count, every pixel is the same bits under every
     * sharding (tests: test_sharded_render_equals_unsharded). */
    int32_t spp_chunks;
    int32_t flags; /* RTR_FLAG_* */
} rtr_render_params;

/* Visit the hittable graph in the reference's own order (bvh_node left-then-right, lists in
 * order) instead of the compiled scene.  Always on for scenes with constant_medium, whose RNG
 * draws depend on that order; elsewhere both give the same image and this flag is a
 * cross-check. */
#define RTR_FLAG_REFERENCE_ORDER 1
/* Wavefront pipeline only: run the two ray-casting stages as PERSISTENT THREADS on the resumable traversal machine
 * (every lane takes the next ray of its wave's blocks as soon as its own is finished) instead of lockstep waves.
 * Same image bit for bit; measured slower on MI355X for every BASELINE scene, kept selectable. */
#define RTR_FLAG_WF_PERSISTENT 2
/* Megakernel only: once per bounce the 256 lanes of a workgroup exchange their hits through LDS so that every wave
 * shades hits of ONE material type (the reference's virtual scatter() call, material.h:31-60, is what diverges).
 * Exists for the MIS integrator on flat scenes lit by quad lights only (scene 23's kernel); ignored elsewhere.
 * Same image bit for bit; measured slower on MI355X (4.06 against 6.62 Gsamples/s on scene 23), kept
 * selectable. */
#define RTR_FLAG_SORTED_SHADING 4
/* Megakernel only: cast a bounce's shadow ray and the next closest-hit ray one after the other instead of in one pass over
 * the instances.  The pair cast is what the MIS integrator runs on lit flat scenes of at most four instances made of
 * rectangles, boxes and spheres (scenes 21 and 23); this flag asks for the split casts there, and is reported in
 * flags_in_effect where it changed the kernel.  Same image and segment counts bit for bit. */
#define RTR_FLAG_SPLIT_CASTS 8
/* Megakernel only: one workgroup per (tile, chunk of samples), every lane on one pixel until the slowest pixel of its wave
 * has finished the chunk.  A one-shot render with the pair cast otherwise runs a persistent grid whose lanes pull (pixel,
 * chunk) jobs from a launch-wide queue as they finish (images up to 65 535 x 65 535; accumulator passes keep the static
 * grid).  The jobs are the static grid's partial sums, summed in the same order and added in the same order: same image
 * and counts bit for bit, so this flag is the A/B switch of tests and measurements; reported in flags_in_effect where it
 * changed the kernel.  The environment variable RTR_QUEUE_WORKGROUPS=n, read at every launch, caps the persistent grid
 * at n workgroups (a test hook, like RTR_GUIDED for the guided chunk split). */
#define RTR_FLAG_STATIC_GRID 16

typedef struct rtr_render_stats {
    uint64_t samples;          /* camera samples finished                               */
    uint64_t closest_segments; /* closest-hit traversals (hot loop 3)       */
    uint64_t shadow_segments;  /* shadow-ray traversals                                 */
    double device_ms;          /* HIP-event time of the render kernels of the last call */
    int32_t kernel_launches;
    int32_t pipeline;          /* pipeline that actually ran                            */
    int32_t spp_chunks;        /* partial sums per pixel that were used (params.spp_chunks, or the library's choice for 0) */
    int32_t cancelled;         /* 1: rtr_cancel() stopped this render before its last sample */
    int32_t flags_in_effect;   /* the RTR_FLAG_* bits of params.flags that selected another kernel than 0 would have */
    int32_t reserved;
} rtr_render_stats;

typedef struct rtr_context rtr_context;

/* ------------------------------------------------------------------------- */
/* entry points                                                              */

/* ABI version of the loaded library. */
uint32_t rtr_abi_version(void);

/* Number of HIP devices visible, or a negative status. */
int rtr_device_count(void);

/* Create / destroy a context bound to one GPU.  Replaces the construction of
 * `Renderer` (renderer.h:22-24).  One context is driven by one host thread. */
int rtr_create(int device_ordinal, rtr_context** out_ctx);
void rtr_destroy(rtr_context* ctx);

/* Launch the render kernels on an existing HIP stream (hipStream_t as void*;
 * NULL = the context's own stream).  Lets a host framework time the kernels
 * with its own events. */
int rtr_set_stream(rtr_context* ctx, void* hip_stream);

/* Validate + upload an immutable flattened scene.  Replaces the `world`, `cam`,
 * `background`, `lights` arguments of Renderer::render (renderer.h:30-32).
 * Every record of every array is checked, reachable from `root` or not: indices and
 * types in range, no cycle, image texels and environment tables inside image_bytes,
 * perlin permutation entries in 0..255, and finite parameters for the primitives and
 * transforms the graph reaches (RTR_ERR_INVALID / RTR_ERR_UNSUPPORTED with a message
 * in rtr_last_error; nothing is uploaded then).  These checks are what keeps the host
 * and the kernels inside the arrays they were given: a scene file is untrusted input. */
int rtr_upload_scene(rtr_context* ctx, const rtr_scene_desc* scene);

/* Render the region into a DEVICE buffer of doubles, 3 per pixel:
 * d_rgb[((j - y0) * row_stride + (i - x0)) * 3 + c] = linear mean radiance
 * (sum over samples * (1/spp)); pixels of tiles this call does not own are
 * left untouched.  Asynchronous on the context stream unless `blocking`; further
 * non-blocking calls queue behind it (the host waits only if the new call needs
 * another tile list or larger buffers than the one still running). */
int rtr_render_device(rtr_context* ctx, const rtr_render_params* params,
                      double* d_rgb, int64_t row_stride, int blocking);

/* Same, into a HOST buffer (blocking; includes the D2H copy). */
int rtr_render_host(rtr_context* ctx, const rtr_render_params* params,
                    double* h_rgb, int64_t row_stride);

/* Like rtr_render_host, but only what the call OWNS crosses PCIe: the tiles with index % tile_stride == tile_first that
 * intersect the region, packed.  On return *n_tiles tiles were rendered; tile k is the reference's tile (*tile_ids)[k]
 * (dispatch numbering, renderer.h:61-62) and occupies (*tiles)[k * 768 ...]: 16 rows of 16 pixels of 3 doubles, lowest
 * row first, linear mean radiance (pixels of a border tile outside the image or region are undefined);
 * (*tile_done)[k] = 1 when the tile was finished, 0 when a cancel came first (the reference's workers leave such a
 * tile untouched, renderer.h:52-59).  The three arrays live in pinned host memory owned by the context and stay valid
 * until its next render call.  Blocking.  This is what one worker of an N-GPU renderer calls: nothing is uploaded,
 * one D2H copy of n_tiles x 6 KiB. */
int rtr_render_tiles_host(rtr_context* ctx, const rtr_render_params* params, const double** tiles, const int32_t** tile_ids,
                          const uint8_t** tile_done, int64_t* n_tiles);

/* The number of partial sums per pixel the library would use for `params` (params->spp_chunks, or its own
 * choice for 0: depends on the scene's kernel variant, the pipeline and the number of owned tiles).  Returns
 * the count (>= 1) or a negative status.  Lets a caller render a crop with the summation of a full-size render. */
int rtr_plan_chunks(rtr_context* ctx, const rtr_render_params* params);

/* Per-ray entry: `Integrator::Li(r, world, background, lights)` (renderer/integrator.h:12-19) for `n` camera
 * samples of the uploaded scene, one GPU lane each.  Sample k is (pixel i = ijs[3k], j = ijs[3k+1], sample index
 * s = ijs[3k+2]) of the image params describe: its ray is camera::get_ray under rtr_sample_seed(seed, W, i, j, s)
 * exactly as in a render, and L[3k..3k+2] receives its radiance (not divided by spp).  params->integrator,
 * max_depth, rr_start_depth and flags apply; region, tiles, chunks and pipeline do not.  Host arrays; blocking. */
int rtr_li_samples(rtr_context* ctx, const rtr_render_params* params, const int32_t* ijs, double* L, int64_t n);

/* The same for ARBITRARY rays (Integrator::Li takes any `ray`: renderer/integrator.h:12-19): ray k starts at
 * origin with direction (not normalised by the library, like the reference's), time, and the xorshift32 state
 * (core/rtweekend.h:24-34; must not be 0) the reference's thread-local generator would hold when Li is entered --
 * for a camera ray that is the state after camera::get_ray.  L[3k..3k+2] receives the radiance. */
typedef struct rtr_li_ray {
    double origin[3], direction[3], time;
    uint32_t rng_state, pad;
} rtr_li_ray;
int rtr_li_rays(rtr_context* ctx, const rtr_render_params* params, const rtr_li_ray* rays, double* L, int64_t n);

/* Wait for everything queued on the context stream. */
int rtr_synchronize(rtr_context* ctx);

/* Thread-safe cooperative cancel (Renderer::cancel, renderer.h:113-115).  Covers every render
 * issued on the context so far, running or still queued behind another one; a render issued
 * afterwards is not affected.  A covered render stops at its next poll (every 8th sample of a
 * pixel / every wavefront batch) and reports RTR_ERR_CANCELLED: from the blocking call itself,
 * otherwise as rtr_render_stats.cancelled.  Output buffer after a cancel: like the reference's
 * workers (renderer.h:52-59), tiles whose samples all finished hold their final values and every
 * other tile keeps what the caller's buffer held before the call (megakernel: per 16x16 tile;
 * wavefront: no tile is written).  A cancel that arrives after the last sample has no effect. */
int rtr_cancel(rtr_context* ctx);

/* Statistics of the LAST render call (blocks until it has finished).  The
 * statistics of earlier queued calls that were never asked for are dropped. */
int rtr_get_stats(rtr_context* ctx, rtr_render_stats* out);

/* Text of the last error on this context ("" if none).  ctx may be NULL for
 * errors of rtr_create. */
const char* rtr_last_error(const rtr_context* ctx);

/* Per-sample RNG seed shared by the oracle and the device: the
 * xorshift32 state (core/rtweekend.h:24-34) used for sample `s` of pixel
 * (i, j) under render seed `seed`; never 0. */
uint32_t rtr_sample_seed(uint32_t seed, int32_t image_width, int32_t i, int32_t j, int32_t s);

/* Facts rtr_upload_scene() derives from a scene, and the host-only check it runs before touching the GPU. */
typedef struct rtr_scene_info {
    int32_t stack_words; /* LDS traversal-stack words per lane the reference-order traversal needs */
    int32_t has_media;   /* constant_medium present: RNG is consumed inside traversal */
    int32_t needs_uv;    /* some texture reads (u,v) */
    int32_t graph_depth; /* longest root-to-leaf chain of hittables */
    int32_t fast_ok;     /* a compiled scene exists (no media): the order-free traversal is the default */
    int32_t fast_instances, fast_refs, fast_stack_words;
    int32_t compiled_subtrees; /* media scenes: media-free subtrees compiled inside the reference-order walk */
    int32_t program_steps;     /* media scenes: steps of the ray-cast program (0: media not directly under the root list) */
    int32_t inverted_boxes;    /* spheres with a negative radius (hollow glass): sphere::bounding_box (sphere.h:62-66)
                                  then has min > max, the bvh_node boxes built from it do not enclose the sphere,
                                  and which rays still reach it depends on the reference's visiting order */
    int32_t top_trees;         /* compiled sub-scenes whose many transformed instances sit in a box tree of their own
                                  (walked per lane by the megakernel) instead of being scanned one after the other */
} rtr_scene_info;

/* ------------------------------------------------------------------------- */
/* progressive accumulation (megakernel pipeline)                            */

/* A device-resident accumulator: per owned pixel ONE running FP64 sum in sample order and, per owned tile, the number
 * of samples it holds.  Passes continue the sums: a sample's generator state depends on (seed, W, i, j, s) only, so
 * after any sequence of passes that ends at target T the resolved image is the bits of rtr_render_host with spp = T
 * and spp_chunks = 1 (it differs from the spp_chunks = 0 default by summation order only, within 1e-13 relative), and
 * the statistics summed over the passes are the one-shot render's.  The accumulator owns its sums, counts and tile
 * list: one-shot renders on the same context between its passes do not disturb it. */
typedef struct rtr_accum rtr_accum;

/* Bind an accumulator to the context's current scene and to region, image size, tile sharding (tile_first /
 * tile_stride), seed, integrator, max_depth, rr_start_depth, pipeline and flags of *params (params->spp and
 * params->spp_chunks are ignored).  Every owned tile starts at 0 samples.  RTR_ERR_UNSUPPORTED for
 * RTR_PIPELINE_WAVEFRONT; RTR_ERR_NO_SCENE before rtr_upload_scene.  rtr_destroy() frees the accumulators left on
 * the context. */
int rtr_accum_create(rtr_context* ctx, const rtr_render_params* params, rtr_accum** out);

/* One pass: every owned tile continues from its own sample count to spp_target (samples [count, spp_target)); tiles
 * already there do no work, a target equal to every count is a no-op, a target below some count is RTR_ERR_INVALID.
 * Asynchronous on the context stream unless `blocking`, like rtr_render_device; rtr_get_stats reports the pass.
 * rtr_cancel() stops it with RTR_ERR_CANCELLED, atomically per tile: a tile then holds either its old sums and count
 * or the new ones, and the same call again finishes the tiles that are still behind.  RTR_ERR_INVALID after the
 * context's scene was uploaded again, or with a handle of another context. */
int rtr_accum_render(rtr_context* ctx, rtr_accum* acc, int32_t spp_target, int blocking);

/* The mean of the samples so far, (1.0 / count) * sum as in a render, into HOST buffers (blocking); either may be NULL:
 *   h_linear  linear radiance, 3 doubles per pixel, h_linear[((j - y0) * row_stride + (i - x0)) * 3 + c]
 *   h_rgb8    the bytes RenderBuffer::save_to_png writes for the region (renderer.h:126-140, render_buffer.h:35-55):
 *             uchar(clamp(sqrt(c), 0, 1) * 255), rows of (x1 - x0) pixels, the TOP row of the region (j = y1 - 1) first
 * Pixels of tiles the accumulator does not own or that hold no sample yet keep the caller's values, so the
 * accumulators of a tile-sharded render can resolve into one buffer.  Only the owned tiles cross PCIe, packed. */
int rtr_accum_resolve(rtr_context* ctx, rtr_accum* acc, double* h_linear, int64_t row_stride, uint8_t* h_rgb8);

/* The owned tiles (reference dispatch numbering, renderer.h:61-62) and the samples each holds: the first
 * min(cap, *n_tiles) entries go to tile_ids / counts (either may be NULL), *n_tiles receives the number of owned
 * tiles.  Blocking. */
int rtr_accum_tiles(rtr_context* ctx, const rtr_accum* acc, int32_t* tile_ids, int32_t* counts, int64_t cap,
                    int64_t* n_tiles);

/* Free an accumulator (waits for its queued work).  NULL is ignored. */
void rtr_accum_destroy(rtr_accum* acc);

/* ---- adaptive sampling: per-tile targets, second moments, noise estimates (megakernel pipeline) ----
 *
 * rtr_accum_create_ex with RTR_ACCUM_MOMENTS: the accumulator also keeps, per owned pixel and in sample order,
 * Q = sum over samples of y_s * y_s, y_s = 0.2126 * L.x + 0.7152 * L.y + 0.0722 * L.z (left to right) of the sample's
 * radiance L.  Its passes run a third megakernel twin (k_mega<..., ACC = 2>); the sums stay the bits of a plain
 * accumulator.  A cancel leaves a tile's sums, moments and count all old or all new.
 *
 * The error of a pixel of a tile holding n samples, with m = (1.0 / n) * sum per channel and y_m its luminance:
 *   var = max(0, (1.0 / n) * Q - y_m * y_m) / (n - 1),   err = sqrt(var) / (2 * sqrt(max(y_m, 1e-4)))
 * -- the standard error of the gamma-2 value RenderBuffer stores (renderer.h:126-140), so 1/255 is one 8-bit step.  A
 * tile's error is the largest of its pixels inside the region, +inf below 2 samples.  Only + - * / sqrt max are used:
 * the values are reproducible bit for bit on the host. */
#define RTR_ACCUM_MOMENTS 1u /* accum_flags of rtr_accum_create_ex */

/* rtr_accum_create with flags: 0 or RTR_ACCUM_MOMENTS (rtr_accum_create(ctx, p, out) = rtr_accum_create_ex(ctx, p, 0, out)).
 * RTR_ERR_INVALID for an unknown flag, RTR_ERR_UNSUPPORTED for RTR_PIPELINE_WAVEFRONT. */
int rtr_accum_create_ex(rtr_context* ctx, const rtr_render_params* params, uint32_t accum_flags, rtr_accum** out);

/* One pass with a target per owned tile: targets[k] for the k-th tile of rtr_accum_tiles; every tile continues from its
 * count to its target (a tile already there does no work; all there: a no-op).  Each tile is one workgroup and the
 * tiles with most samples to go are dispatched first; a tile holding T samples is the bits of a render with spp = T and
 * spp_chunks = 1, whatever the passes were.  RTR_ERR_INVALID if n is not the number of owned tiles or a target is below
 * its tile's count.  Asynchronous unless `blocking`; cancel as rtr_accum_render. */
int rtr_accum_render_tiles(rtr_context* ctx, rtr_accum* acc, const int32_t* targets, int64_t n, int blocking);

/* The raw second moments Q, one double per pixel into a HOST buffer, h_q[(j - y0) * row_stride + (i - x0)]; pixels of
 * tiles not owned or without samples keep the caller's values.  Blocking.  RTR_ERR_INVALID without RTR_ACCUM_MOMENTS. */
int rtr_accum_moments(rtr_context* ctx, rtr_accum* acc, double* h_q, int64_t row_stride);

/* The error of every owned tile (above) in the order of rtr_accum_tiles: the first min(cap, *n_tiles) go to tile_err
 * (may be NULL), *n_tiles receives the number of owned tiles.  Blocking.  RTR_ERR_INVALID without RTR_ACCUM_MOMENTS. */
int rtr_accum_errors(rtr_context* ctx, rtr_accum* acc, double* tile_err, int64_t cap, int64_t* n_tiles);

/* One refinement pass, decided on the device with no host round trip: per owned tile holding n samples with error e
 *   n < spp_min                        -> target spp_min
 *   e > threshold and n < spp_max      -> target min(spp_max, 2 * n)
 *   otherwise                          -> the tile stops (no work)
 * then the pass as rtr_accum_render_tiles.  Decisions are tile-local, so a tile-sharded render (one context and
 * accumulator per shard) reaches the counts and bits of an unsharded one.  Blocking: *n_active (may be NULL) receives
 * the number of tiles the pass refined, 0 = the render is done; not blocking: -1.  RTR_ERR_INVALID without
 * RTR_ACCUM_MOMENTS, for threshold <= 0 or NaN, spp_min < 1 or spp_max < spp_min (before any device work).  Cancel as
 * rtr_accum_render: the same call again redoes the tiles that were interrupted. */
int rtr_accum_refine(rtr_context* ctx, rtr_accum* acc, double threshold, int32_t spp_min, int32_t spp_max, int blocking,
                     int32_t* n_active);

/* ---- first-hit feature buffers and an a-trous denoiser (megakernel pipeline) ----
 *
 * Features.  For samples s = 0 .. K-1 of pixel (i, j) the camera ray sample s of a render builds is cast to its closest
 * hit with the traversal of the accumulator's renders (RTR_FLAG_REFERENCE_ORDER included); a medium draws from the
 * sample's own generator state after the camera ray.  Per sample, 7 doubles:
 *   surface hit   albedo: lambertian / isotropic / PBR the value of tex[0] at the hit, metal f[0..2], dielectric and
 *                 diffuse_light (1, 1, 1); normal: the hit record's (no normal map); depth: t * sqrt(d.x*d.x + d.y*d.y +
 *                 d.z*d.z), d the unnormalised ray direction
 *   medium event  (the hit's material is isotropic) albedo as above, normal (0, 0, 0), depth as above
 *   miss          albedo (1, 1, 1), normal (0, 0, 0), depth 0
 * A pixel's feature is (1.0 / K) * (the sum over s in sample order).  It depends on (seed, W, i, j, K) and the scene only.
 *
 * Filter: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with the variance-guided luminance weight of
 * SVGF's spatial part (Schied et al. 2017), FP64, only + - * / sqrt and compares (a numpy restatement gives the same
 * bits).  Per valid pixel p of the region (n the tile's count, m = (1.0 / n) * sum, lum(c) = 0.2126 * c.x + 0.7152 *
 * c.y + 0.0722 * c.z left to right, a / nn / z the features):
 *   var_p = max(0, (1.0 / n) * Q - lum(m)^2) / (n - 1) / n, or 1e30 when n < 2; var_p /= max(lum(a), 1e-3)^2
 *   c_p   = m / a per channel where a > 1e-3, else m
 * Pass k = 0 .. iterations-1, step = 2^k, reading buffer k % 2 and writing the other:
 *   g_p = sum of k3[dx] * k3[dy] * var_q / sum of k3[dx] * k3[dy] over the valid q = p + (dx, dy), dy (outer) and dx in
 *         -1..1, k3 = {1/4, 1/2, 1/4}
 *   taps q = p + step * (dx, dy), dy (outer) and dx in -2..2, valid ones only; h = {1, 4, 6, 4, 1} / 16;
 *   w = h[dx] * h[dy] * w_l * w_n * w_a * w_z (left to right) with, l = lum(c),
 *     w_l = 1 / (1 + (l_p - l_q)^2 / (sigma_l^2 * g_p + 1e-10))
 *     w_n = 1 / (1 + |nn_p - nn_q|^2 / sigma_n^2),  w_a = 1 / (1 + |a_p - a_q|^2 / sigma_a^2)
 *     w_z = 1 / (1 + (z_p - z_q)^2 / (sigma_z^2 * step^2 * max(z_p, 1e-3)^2))
 *   c'_p = sum of w * c_q / sum of w,  var'_p = sum of w * w * var_q / (sum of w)^2   (sums in tap order)
 * Output: c_p * a_p per channel where a_p > 1e-3, else c_p; iterations = 0 gives m itself (the bits of
 * rtr_accum_resolve).  A pixel is valid if its tile holds a sample; pixels outside the region are never taps. */
typedef struct rtr_denoise_params {
    int32_t iterations;  /* 0..10 */
    int32_t feature_spp; /* K >= 1: camera samples averaged per pixel feature */
    double sigma_l, sigma_n, sigma_a, sigma_z; /* > 0, finite */
    double reserved[4];  /* must be 0 */
} rtr_denoise_params;

/* The defaults (measured on scenes 21, 22 and 23: INTEGRATION.md section 4, "Denoising"). */
void rtr_denoise_defaults(rtr_denoise_params* p);

/* The features of every pixel of the owned tiles inside the region into a HOST buffer, 7 doubles per pixel:
 * h_feat[((j - y0) * row_stride + (i - x0)) * 7 + c], c = albedo 0..2, normal 3..5, depth 6; other pixels keep the
 * caller's values.  With or without RTR_ACCUM_MOMENTS; the accumulator keeps the features of the last K it computed
 * until it is destroyed.  Blocking.  RTR_ERR_INVALID for K < 1, a re-uploaded scene or a handle of another context. */
int rtr_accum_features(rtr_context* ctx, rtr_accum* acc, int32_t feature_spp, double* h_feat, int64_t row_stride);

/* The denoised image of the accumulator's samples so far (features of params->feature_spp samples, computed unless
 * cached), in the layouts of rtr_accum_resolve; either output may be NULL, not both.  Pixels of tiles holding no sample
 * keep the caller's values.  Sums, moments, counts and tile list are not modified.  Blocking.  RTR_ERR_INVALID without
 * RTR_ACCUM_MOMENTS, for bad params (NULL params too), a re-uploaded scene or a handle of another context, before any
 * device work; RTR_ERR_UNSUPPORTED if the accumulator does not own every tile of its region (tile_stride > 1). */
int rtr_accum_denoise(rtr_context* ctx, rtr_accum* acc, const rtr_denoise_params* params, double* h_linear,
                      int64_t row_stride, uint8_t* h_rgb8);

/* The same filter over row-major HOST planes of a width x height region (pixel p = row * width + col, row 0 = the lowest
 * row y0): h_color the linear mean (3 doubles per pixel), h_q the second moments, h_count the sample count of the
 * pixel's tile (0: not a tap, its outputs keep the caller's values), h_feat the features (7 per pixel).  h_linear gets
 * 3 doubles per pixel in the same layout, h_rgb8 the 8-bit store with the TOP row first; either may be NULL, not both.
 * The shards of a tile-sharded render gathered with rtr_accum_resolve / _moments / _tiles / _features give the bits of
 * the unsharded rtr_accum_denoise.  Needs no scene.  Blocking.  RTR_ERR_INVALID for bad params or sizes. */
int rtr_denoise_host(rtr_context* ctx, const rtr_denoise_params* params, int32_t width, int32_t height,
                     const double* h_color, const double* h_q, const int32_t* h_count, const double* h_feat,
                     double* h_linear, uint8_t* h_rgb8);

/* ---- ray queries: closest hit and occlusion of caller-given rays on the uploaded scene ----
 * rtr_query_closest is `world->hit(ray, t_min, t_max, rec)` (geometry/hittable.h:25-32) on the scene's root for each of
 * `n` rays, one GPU lane each; rtr_query_occluded is the boolean of the same call, taken through the any-hit forms the
 * integrators' shadow rays use.  The traversal is the one a render of the scene with `flags` walks (compiled scene, top
 * tree, step program of a scene with media, or the reference-order walk), so t, p, n, front_face and material are the
 * reference's bits wherever a render's are.  (u, v) are always computed, whether or not a texture of the scene reads
 * them.  In a scene with media the draws inside constant_medium::hit happen in both calls: occluded[k] and rng_out[k]
 * equal hits[k].hit and hits[k].rng_out of the closest query on the same ray.
 *
 * flags: 0 or RTR_FLAG_REFERENCE_ORDER (as in a render); any other bit is RTR_ERR_INVALID.  n == 0 is RTR_OK without a
 * launch; n < 0 or a NULL array (rng_out may be NULL) is RTR_ERR_INVALID; a call before rtr_upload_scene is
 * RTR_ERR_NO_SCENE -- all before any device work.
 *
 * A ray is BAD if origin, direction, time or t_min is not finite, t_max is NaN (+-inf are fine), or rng_state is 0 in
 * a scene with media.  The host entries reject the whole batch with RTR_ERR_INVALID, name the first bad index in
 * rtr_last_error and leave the outputs untouched; the device entries cannot see the data: there the kernel writes a
 * miss (occluded = 0, rng_out = rng_state) for such a ray without casting it.  Any finite t_min is allowed, 0 and
 * negative values included: a wave holding a ray with t_min < 2^-100 takes the plain IEEE divisions instead of the
 * shared reciprocals, so the results are the reference's bits there too.
 *
 * The host entries take host arrays and block; they copy through a staging buffer of the context that only grows, in
 * slices of at most 2^22 rays, so n is bounded by the caller's memory only.  The device entries take device pointers
 * (8-byte aligned; in and out must not overlap), run on the context stream behind whatever is queued there -- renders
 * and accumulator passes included -- and return at once unless `blocking`.  Neither touches anything a queued render
 * or accumulator pass uses, nor the statistics of rtr_get_stats.  rtr_cancel does not apply to queries. */
typedef struct rtr_ray {            /* 80 bytes */
    double origin[3], direction[3]; /* direction is not normalised by the library, like the reference's ray */
    double time, t_min, t_max;      /* t_max may be +inf */
    uint32_t rng_state, pad;        /* xorshift32 state when hit() is entered; read only where the scene has media */
} rtr_ray;

typedef struct rtr_ray_hit {        /* 88 bytes */
    double t, p[3], n[3], u, v;     /* u, v are NaN where the reference leaves them unset; all 0 on a miss */
    int32_t hit, front_face, material; /* material = -1 on a miss */
    uint32_t rng_out;               /* generator state after the call (= rng_state without media) */
} rtr_ray_hit;

int rtr_query_closest(rtr_context* ctx, const rtr_ray* rays, rtr_ray_hit* hits, int64_t n, int32_t flags);
int rtr_query_occluded(rtr_context* ctx, const rtr_ray* rays, uint8_t* occluded, uint32_t* rng_out, int64_t n,
                       int32_t flags);
int rtr_query_closest_device(rtr_context* ctx, const rtr_ray* d_rays, rtr_ray_hit* d_hits, int64_t n, int32_t flags,
                             int blocking);
int rtr_query_occluded_device(rtr_context* ctx, const rtr_ray* d_rays, uint8_t* d_occluded, uint32_t* d_rng_out,
                              int64_t n, int32_t flags, int blocking);

/* ---- camera updates: a new camera for the uploaded scene without another upload ----
 * rtr_set_camera replaces the camera of the uploaded scene for every call issued afterwards (one-shot renders of both
 * pipelines, rtr_li_samples, accumulator passes, features): the image is the bits of rtr_upload_scene of the same scene
 * with that camera.  The call itself does no device work and does not wait: work already queued keeps the camera it was
 * issued with, and the next render carries the new one to the device in stream order.  Nothing rtr_upload_scene derives
 * from a scene depends on the camera but the range of ray times its boxes of moving spheres were built for.
 * RTR_ERR_NO_SCENE before an upload; RTR_ERR_INVALID for NULL or a non-finite member; RTR_ERR_UNSUPPORTED (with a
 * message) when time0 or time1 lies outside [min(0, time0, time1), max(0, time0, time1)] of the uploaded camera, or
 * crosses the 2^60 bound of the shared divisions: such a camera needs an upload.
 *
 * The context counts camera updates.  An accumulator remembers the count of its creation or last reset; with a stale
 * one rtr_accum_render, _render_tiles, _refine, _features, _denoise and _denoise_temporal return RTR_ERR_INVALID before
 * any device work (its samples belong to the old camera: rtr_accum_resolve, _moments, _tiles and _errors still return
 * them).  rtr_accum_reset waits for the accumulator's queued work, sets every owned tile to 0 samples, drops the cached
 * features, binds the accumulator to the current camera and replaces its seed: afterwards it is indistinguishable from
 * one created now with that seed.  After rtr_upload_scene it stays RTR_ERR_INVALID, reset included. */
int rtr_set_camera(rtr_context* ctx, const rtr_camera* cam);
int rtr_get_camera(rtr_context* ctx, rtr_camera* out);
int rtr_accum_reset(rtr_context* ctx, rtr_accum* acc, uint32_t seed);

/* ---- temporal reprojection: the other half of SVGF (Schied et al. 2017) in front of the a-trous filter ----
 * A history keeps, per pixel of its region, 10 doubles of the last frame -- c[3] demodulated colour, mu1, mu2 raw
 * luminance moments, n effective sample count (0: no history), z, nn[3] -- in two plane sets (a frame reads one and
 * writes the other), and the camera they were seen from.
 *
 * rtr_accum_denoise_temporal is rtr_accum_denoise with the history blended in before the filter.  Per valid pixel
 * (i, j) (full-image coordinates) with m, Q, n, a, nn, z, lum, la = max(lum(a), 1e-3) and c_p of the filter definition
 * above, mu1_cur = lum(m), mu2_cur = (1.0 / n) * Q, n_cur = double(n); cam the context's camera, prev the history's;
 * vector operations per component, sums left to right, compares in binary64:
 *   su = (i + 0.5) / (W - 1), sv = (j + 0.5) / (H - 1);  d = llc + su * hor + sv * ver - origin
 *   len = sqrt(d.x*d.x + d.y*d.y + d.z*d.z);  P = origin + (z / len) * d      (no history when z <= 0 or it is cleared)
 *   q = P - prev.origin, e = prev.llc - prev.origin, zc = -(q . prev.w) (no history unless zc > 0), F = -(e . prev.w)
 *   k = F / zc;  s = (k * (q . prev.u) - e . prev.u) / (prev.hor . prev.u);  t likewise with prev.v and prev.ver
 *   x = s * (W - 1) - 0.5, y = t * (H - 1) - 0.5;  x0 = floor(x), fx = x - x0, y likewise;  z_exp = sqrt(q . q)
 * Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with weights (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy; a tap
 * is accepted when it lies inside the region, its history n > 0, |z_exp - z_tap| <= tau_z * max(z_exp, 1e-3) and
 * |nn_p - nn_tap|^2 <= tau_n.  sw = the sum of the accepted weights in tap order; no history unless sw >= min_weight;
 * else each history value is (sum of w * value) / sw in tap order, for c, mu1, mu2 and n.
 *   with history:  alpha = max(n_cur / (n_cur + n_h), alpha_min);  c' = alpha * c_p + (1 - alpha) * c_h, mu1' and mu2'
 *                  likewise;  n' = n_cur / alpha
 *   without:       c', mu1', mu2', n' are the current values
 *   var' = max(0, mu2' - mu1' * mu1') / (n' - 1) / n', or 1e30 when n' < 2;  var' /= la * la
 * The a-trous passes and the output stage then run unchanged on (c', var', a, nn, z), and the history takes c', mu1',
 * mu2', n', z, nn per pixel (n = 0 where the pixel is invalid) and the current camera -- on every successful call.  The
 * first frame on a cleared history is therefore the bits of rtr_accum_denoise. */
typedef struct rtr_history rtr_history;
typedef struct rtr_temporal_params {
    double alpha_min;   /* (0, 1]: lower bound of the current frame's blend weight */
    double tau_z;       /* > 0: relative depth tolerance of a history tap */
    double tau_n;       /* > 0: largest |n_p - n_q|^2 of a history tap */
    double min_weight;  /* (0, 1): smallest sum of accepted bilinear weights */
    double reserved[4]; /* must be 0 */
} rtr_temporal_params;

/* The defaults ("Camera updates and temporal reprojection"). */
void rtr_temporal_defaults(rtr_temporal_params* p);

/* A cleared history for the image size and region of *p (nothing else of *p is read).  rtr_destroy() frees the
 * histories left on the context. */
int rtr_history_create(rtr_context* ctx, const rtr_render_params* p, rtr_history** out);
/* Forget everything (waits for queued work): the next frame has no history. */
int rtr_history_clear(rtr_context* ctx, rtr_history* hist);
void rtr_history_destroy(rtr_history* hist);
/* The plane set the next frame will read, into a HOST buffer: h_planes[((j - y0) * row_stride + (i - x0)) * 10 + k],
 * k = c 0..2, mu1 3, mu2 4, n 5, z 6, nn 7..9.  Blocking. */
int rtr_history_planes(rtr_context* ctx, rtr_history* hist, double* h_planes, int64_t row_stride);

/* rtr_accum_denoise with the temporal stage above; outputs as there (either may be NULL, not both).  Every check of
 * rtr_accum_denoise, the ranges of rtr_temporal_params, and a history of the same context, image size and region
 * (RTR_ERR_INVALID) -- all before any device work: after an error the history and the accumulator are unchanged. */
int rtr_accum_denoise_temporal(rtr_context* ctx, rtr_accum* acc, rtr_history* hist, const rtr_denoise_params* params,
                               const rtr_temporal_params* temporal, double* h_linear, int64_t row_stride,
                               uint8_t* h_rgb8);

/* ---- device outputs for accumulators: resolve, features, denoise and temporal frames without a host round trip ----
 * The four calls below are rtr_accum_resolve, _features, _denoise and _denoise_temporal with DEVICE pointers for the
 * outputs: the same layouts and, per pixel written, the same bits.
 *   d_linear  d_linear[((j - y0) * row_stride + (i - x0)) * 3 + c], 8-byte aligned
 *   d_rgb8    rows of (x1 - x0) pixels, the TOP row of the region first: the layout rtr_display_device writes too
 *   d_feat    d_feat[((j - y0) * row_stride + (i - x0)) * 7 + c], 8-byte aligned
 * Which pixels are written is decided ON THE DEVICE, when the kernels execute: a pixel whose tile holds no sample then
 * (never rendered, reset, left behind by a cancelled pass or by rtr_accum_render_tiles with a target of 0) keeps the
 * caller's bytes in both outputs, and so does, for resolve and features, a pixel of a tile the accumulator does not own
 * (features are written for every owned tile, like rtr_accum_features).  The host does not read the sample counts: the
 * calls neither wait for the passes queued before nor refresh the copy rtr_accum_tiles returns.
 *
 * Stream order: the work goes on the context stream (rtr_set_stream included) behind whatever is queued there -- a
 * non-blocking rtr_accum_render of the same accumulator included -- and the call returns at once unless `blocking`;
 * rtr_display_device on d_linear may follow with no host wait in between.  Once the workspace has reached its size, a
 * call makes no allocation, no copy to the host and no wait; the host waits for the stream only when the call has to
 * replace the filter's planes (a larger region than any denoise call of the context before) or the accumulator's feature
 * planes by larger ones while queued work may still use the old ones.  The temporal form takes the context's camera and
 * the history's by value at the call and advances the history (plane set, camera) when it returns RTR_OK: queued frames
 * see the history in call order.  rtr_history_planes, rtr_history_clear, rtr_accum_reset and rtr_accum_destroy wait for
 * queued work as before.  rtr_cancel does not apply to these calls, and they leave the statistics of rtr_get_stats alone.
 *
 * Checks, all before any device work (outputs and history untouched): every check of the host form of the same name
 * (rtr_accum_resolve_device and rtr_accum_features_device accept tile-sharded accumulators, so the shards of one image
 * held on one device compose into one buffer; the two denoise forms return RTR_ERR_UNSUPPORTED for them); a NULL
 * d_linear together with a NULL d_rgb8, or a NULL d_feat; row_stride below the region's width (where d_linear or d_feat
 * is given); a d_linear or d_feat that is not 8-byte aligned -- RTR_ERR_INVALID.  The outputs must not overlap each
 * other or any buffer of the library, and must hold the region at the given stride; neither is checked. */
int rtr_accum_resolve_device(rtr_context* ctx, rtr_accum* acc, double* d_linear, int64_t row_stride, uint8_t* d_rgb8,
                             int blocking);
int rtr_accum_features_device(rtr_context* ctx, rtr_accum* acc, int32_t feature_spp, double* d_feat, int64_t row_stride,
                              int blocking);
int rtr_accum_denoise_device(rtr_context* ctx, rtr_accum* acc, const rtr_denoise_params* params, double* d_linear,
                             int64_t row_stride, uint8_t* d_rgb8, int blocking);
int rtr_accum_denoise_temporal_device(rtr_context* ctx, rtr_accum* acc, rtr_history* hist,
                                      const rtr_denoise_params* params, const rtr_temporal_params* temporal,
                                      double* d_linear, int64_t row_stride, uint8_t* d_rgb8, int blocking);

/* ---- display transform: metered exposure, tone curve, 8-bit encoding ----
 * The last stage in front of a viewer, separate from every output path above (those keep the reference's store).  The
 * input is linear radiance, 3 doubles per pixel, row 0 the LOWEST row, `row_stride` pixels from one row to the next: the
 * layout rtr_denoise_host and rtr_accum_resolve write.  Only + - * / sqrt, compares and integer bit operations are used,
 * so a numpy restatement gives the same bits.  With the defaults the bytes are the reference's store for every finite
 * input.  bits(v) is the 64-bit pattern of the double v.
 *
 * Metering (auto_exposure = 1 and rtr_display_histogram), exact:
 *   y = 0.2126 * c.x + 0.7152 * c.y + 0.0722 * c.z, left to right
 *   a pixel is metered if c.x, c.y and c.z are all finite and y >= 2^-20
 *   its bin: 511 if y >= 2^12, else (bits(y) >> 48) - 0x3EB0 -- 512 bins, 16 per octave (the exponent and the top four
 *            mantissa bits; no log); the lower edge of bin m is the double with bits (uint64)(m + 0x3EB0) << 48
 *   n_metered = the number of metered pixels; T = (n_metered * meter_permille + 999) / 1000 in 64-bit integers
 *   m = the first bin whose cumulative count reaches T; metered = edge(m); scale = (exposure * key) / metered
 *   with n_metered = 0: scale = exposure, metered = 0
 * With auto_exposure = 0 nothing is metered: scale = exposure, metered = 0, n_metered = 0.
 *
 * Mapping, per channel c of a pixel:
 *   x = (c is finite and c > 0) ? min(scale * c, 1e30) : 0
 *   u = the tone curve of x (below), t = u > 0 ? min(u, 1) : 0   (compares only; a NaN becomes 0)
 *   byte = the code of the encoding (below); the optional FP64 output holds t
 *
 * RTR_ENCODE_SRGB is defined by the table S of rtr_display_srgb_thresholds, not by a pow on the device: S[0] = 0 and, for
 * b = 1..255 with v = b / 255.0, S[b] = v / 12.92 if v <= 0.04045, else pow((v + 0.055) / 1.055, 2.4), computed once on
 * the host.  The code of t is the number of b in 1..255 with S[b] <= t (each byte's range starts at its own inverse
 * transfer: truncation, like the gamma-2 store). */
#define RTR_TONE_CLAMP    0   /* u = x: with exposure 1 and gamma-2 encoding, the reference's store */
#define RTR_TONE_REINHARD 1   /* u = x * (1.0 + x / (white * white)) / (1.0 + x), left to right */
#define RTR_TONE_ACES     2   /* u = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)   (Narkowicz fit) */
#define RTR_ENCODE_GAMMA2 0   /* uchar(sqrt(t) * 255), the reference's */
#define RTR_ENCODE_SRGB   1   /* the number of b in 1..255 with S[b] <= t */

typedef struct rtr_display_params {
    int32_t auto_exposure;   /* 0: scale = exposure; 1: scale = exposure * key / metered */
    int32_t meter_permille;  /* 1..1000: which quantile of the metered pixels is `metered` */
    int32_t tone_curve, encoding;
    double exposure;         /* finite, > 0 */
    double key;              /* finite, > 0 */
    double white;            /* finite, > 0 (Reinhard only) */
    double reserved[5];      /* must be 0 */
} rtr_display_params;        /* 80 bytes */

typedef struct rtr_display_result {
    double scale, metered;
    int64_t n_metered, reserved;
} rtr_display_result;        /* 32 bytes */

/* The defaults: auto_exposure 0, meter_permille 500 (the median), RTR_TONE_CLAMP, RTR_ENCODE_GAMMA2, exposure 1,
 * key 0.18 (middle grey), white 4.  Conventional values, not tuned ones. */
void rtr_display_defaults(rtr_display_params* p);

/* The 256 thresholds S the library encodes RTR_ENCODE_SRGB with (S[0] = 0, strictly increasing, S[255] = 1). */
void rtr_display_srgb_thresholds(double out[256]);

/* The metering pass alone over a HOST image: the 512 counts and (unless NULL) their sum.  Needs no scene.  Blocking.
 * RTR_ERR_INVALID for a NULL buffer, a size outside 1 .. 2^28 pixels or row_stride < width, before any device work. */
int rtr_display_histogram(rtr_context* ctx, int32_t width, int32_t height, const double* h_linear, int64_t row_stride,
                          uint32_t h_hist[512], int64_t* n_metered);

/* The transform over a HOST image.  h_rgb8 gets rows of `width` pixels, the TOP row first, like every other 8-bit output
 * here; h_mapped gets t in the input's layout with row_stride = width.  Either may be NULL, not both; `result` may be
 * NULL.  Needs no scene.  Blocking.  RTR_ERR_INVALID -- before any device work, outputs untouched -- for NULL params, an
 * unknown curve or encoding, auto_exposure outside 0..1, meter_permille outside 1..1000, exposure, key or white not
 * finite or <= 0, non-zero reserved, a size outside 1 .. 2^28 pixels, row_stride < width or a NULL input. */
int rtr_display_host(rtr_context* ctx, const rtr_display_params* params, int32_t width, int32_t height,
                     const double* h_linear, int64_t row_stride, uint8_t* h_rgb8, double* h_mapped,
                     rtr_display_result* result);

/* The same with DEVICE pointers, on the context stream behind whatever is queued there: it follows a non-blocking
 * rtr_render_device into the same buffer with no host wait in between, and the scale never visits the host.  Returns at
 * once unless `blocking`; h_result must be NULL unless `blocking`.  The histogram, the scale record and the thresholds
 * live in a buffer of the context nothing else uses: a queued render or accumulator pass is not disturbed. */
int rtr_display_device(rtr_context* ctx, const rtr_display_params* params, int32_t width, int32_t height,
                       const double* d_linear, int64_t row_stride, uint8_t* d_rgb8, double* d_mapped,
                       rtr_display_result* h_result, int blocking);

/* ---- hemisphere gathers: ambient occlusion and mean radiance at caller-given surface points ----
 * For each of `n` points (position p, normal n) the library makes N = params->samples rays over the hemisphere about n in
 * registers, casts them with the traversal a render walks and reduces them to one 32-byte record: nothing per ray ever
 * visits memory.  Every output bit is defined here; only + - * / sqrt and compares are used on the way to a ray, so a
 * host, numpy and the device give the same bits (rtr_gather_ray is the host form).
 *
 * RAY s (0 <= s < N) of point k (k = its index in the call + params->point_base, taken modulo 2^32):
 *   state = rtr_sample_seed_inline(seed, 1, 0, (int32_t)k, s)                  (rtr_seed.h)
 *   w  = unit(n)                               unit(v) = (1 / sqrt(v.x*v.x + v.y*v.y + v.z*v.z)) * v   (core/vec3.h:208-224)
 *   u  = random_unit_vector(state)             the rejection loop of core/vec3.h:226-237: draws z, y, x, each
 *                                              -1 + state' * 2^-31 after one xorshift32 step (13, 17, 5), until
 *                                              x*x + y*y + z*z < 1; then unit
 *   sd = w + u;  if every |component| of sd is < 1e-8 (near_zero, core/vec3.h:81-85): sd = w
 *   d  = unit(sd)
 * The ray is (origin p, direction d, time, [t_min, t_max]) with the state left after the draws: the direction of the
 * reference's lambertian scatter, cosine-distributed about n and of unit length, so t_max is a distance.
 *
 * REDUCTION (part of the contract: v is FP64).  G = min(64, bit_ceil(N)).  Lane l (0 <= l < G) takes the samples
 * s = l, l + G, l + 2G, ... < N in increasing order into a = +0.0; a = a + x_s, per component.  Then for
 * off = G/2, ..., 1: a[l] = a[l] + a[l xor off], all lanes at once.  Then v = (1.0 / N) * a[0].  Counts the same way.
 *
 * rtr_gather_occlusion: a sample is BLOCKED when the any-hit cast of the integrators' shadow rays finds something in
 * [t_min, t_max] -- rtr_query_occluded of that ray, draws inside media included.  x_s = d for an unblocked sample; a
 * blocked one adds nothing.  count = unblocked samples, v = the unnormalised bent normal, count / N = ambient occlusion.
 * rtr_gather_radiance: x_s = Integrator::Li of that ray with that state under render->integrator, max_depth,
 * rr_start_depth and flags -- what rtr_li_rays returns for it (t_min and t_max do not apply).  count = N; v = the mean
 * radiance over cosine-distributed directions: irradiance is pi * v.
 *
 * A point is BAD if a component of p or n is not finite or sqrt(n.n) as computed above is not in (0, +inf).  The host
 * entries reject the whole batch with RTR_ERR_INVALID, name the first bad index in rtr_last_error and leave the outputs
 * untouched; the device entries cannot see the data: there the kernel writes {0, 0, 0, count 0, valid 0} for such a
 * point without casting, and every other point gets valid = 1 and its value.
 *
 * params: 1 <= samples <= 2^20; flags 0 or RTR_FLAG_REFERENCE_ORDER; time and t_min finite (any finite t_min, 0 and
 * negative included: below 2^-100 the launch takes the plain IEEE divisions); t_max not NaN; reserved 0.  Anything else,
 * n < 0 or a NULL array is RTR_ERR_INVALID; a call before rtr_upload_scene is RTR_ERR_NO_SCENE -- all before any device
 * work.  n == 0 is RTR_OK without a launch.
 *
 * The host entries take host arrays and block; they go through a buffer of the context nothing else uses, in slices of
 * at most 2^20 points, and advance point_base per slice.  The device entries take device pointers (8-byte aligned; in and
 * out must not overlap), run on the context stream behind whatever is queued there and return at once unless `blocking`.
 * Neither touches anything a queued render or accumulator pass uses, nor the statistics of rtr_get_stats; rtr_cancel
 * does not apply.  Points can be sharded over contexts: shard j passes point_base = its first point's index. */
typedef struct rtr_gather_point {   /* 48 bytes */
    double p[3], n[3];              /* n need not be normalised */
} rtr_gather_point;

typedef struct rtr_gather_params {  /* 56 bytes */
    int32_t samples;
    uint32_t seed, point_base;
    int32_t flags;
    double time, t_min, t_max;
    double reserved[2];
} rtr_gather_params;

typedef struct rtr_gather_out {     /* 32 bytes */
    double v[3];
    int32_t count, valid;
} rtr_gather_out;

/* samples 64, seed 0, point_base 0, flags 0, time 0, t_min 0.001, t_max +inf */
void rtr_gather_defaults(rtr_gather_params* p);

int rtr_gather_occlusion(rtr_context* ctx, const rtr_gather_params* params, const rtr_gather_point* points,
                         rtr_gather_out* out, int64_t n);
int rtr_gather_radiance(rtr_context* ctx, const rtr_render_params* render, const rtr_gather_params* params,
                        const rtr_gather_point* points, rtr_gather_out* out, int64_t n);
int rtr_gather_occlusion_device(rtr_context* ctx, const rtr_gather_params* params, const rtr_gather_point* d_points,
                                rtr_gather_out* d_out, int64_t n, int blocking);
int rtr_gather_radiance_device(rtr_context* ctx, const rtr_render_params* render, const rtr_gather_params* params,
                               const rtr_gather_point* d_points, rtr_gather_out* d_out, int64_t n, int blocking);

/* Host-only, needs no context: ray s of the point at `index_in_call` (the definition above; `point` is that point's
 * record, not an array).  RTR_ERR_INVALID for a bad point, bad params, a negative index or s outside [0, samples). */
int rtr_gather_ray(const rtr_gather_params* params, const rtr_gather_point* point, int64_t index_in_call, int32_t s,
                   rtr_ray* out);

/* ---- light probes: second-order spherical harmonics of visibility and radiance at points in space, and their use ----
 * A probe is a point p in free space, without a normal.  For each of `n` probes the library makes N = params->samples rays
 * over the whole sphere in registers, casts them, projects every sample onto nine real spherical harmonics and reduces
 * them inside the wave to one record: directional lighting for objects that move through a baked scene.  rtr_gather_params
 * is the parameter block, and everything the gathers' contract above says of it holds here.  Every output bit is defined
 * here; only + - * / sqrt and compares are used, in the order written.
 *
 * RAY s (0 <= s < N) of probe k (k = its index in the call + params->point_base, taken modulo 2^32):
 *   state = rtr_sample_seed_inline(seed, 1, 0, (int32_t)k, s)
 *   u = random_unit_vector(state)       the rejection loop of the gathers: draws z, y, x until x*x + y*y + z*z < 1
 *   d = unit(u) = (1 / sqrt(x*x + y*y + z*z)) * (x, y, z)
 * There is no normal and no near_zero step: d is uniform on the sphere and of unit length, so t_max is a distance.  The
 * ray is (origin p, direction d, time, [t_min, t_max]) with the state left after the draws (rtr_probe_ray is the host form).
 *
 * BASIS: nine functions of d = (x, y, z), in this order and with these literals (rtr_sh_basis is the host form, the same
 * function the kernels call):
 *   K0 = 0.28209479177387814  K1 = 0.4886025119029199  K2 = 1.0925484305920792  K3 = 0.31539156525252005
 *   K4 = 0.5462742152960396
 *   Y0 = K0          Y1 = K1*y        Y2 = K1*z                       Y3 = K1*x       Y4 = K2*(x*y)
 *   Y5 = K2*(y*z)    Y6 = K3*(3.0*(z*z) - 1.0)                        Y7 = K2*(x*z)   Y8 = K4*(x*x - y*y)
 *
 * REDUCTION: the gathers', word for word, for every component independently: G = min(64, bit_ceil(N)); lane l adds its
 * samples l, l + G, ... in increasing order into +0.0; then for off = G/2, ..., 1: a[l] = a[l] + a[l xor off]; then
 * c = (1.0 / N) * a[0].  Counts the same way.
 *
 * rtr_probe_visibility: an unblocked sample adds Y_i(d) to component i, a blocked one adds nothing.  BLOCKED is the
 * gathers' meaning: the any-hit cast of the shadow rays finds something in [t_min, t_max] (rtr_query_occluded of that ray,
 * draws inside media included).  count = the unblocked samples.
 * rtr_probe_radiance: sample s adds Y_i(d) * L[ch] to c[i][ch], L = what rtr_li_rays returns for that ray and state under
 * render->integrator, max_depth, rr_start_depth and flags (t_min and t_max do not apply).  count = N.  c is the mean over
 * uniform directions: the estimate of the SH coefficients of the radiance field is 4 pi * c (rtr_sh_irradiance applies it).
 *
 * A probe is BAD if a component of p is not finite.  The host entries reject the whole batch with RTR_ERR_INVALID, name
 * the first bad index in rtr_last_error and leave the outputs untouched; the device entries write an all-zero record
 * (valid 0) for such a probe without casting, and every other probe gets valid = 1.
 *
 * Parameter checks, n == 0, RTR_ERR_NO_SCENE, the slices of 2^20 points that advance point_base, the 2^-100 rule of t_min,
 * stream order (device pointers 8-byte aligned, `blocking`), and what a call leaves alone -- renders, accumulators,
 * statistics -- are the gathers'.  The host entries go through a buffer of the context nothing else uses. */
typedef struct rtr_probe_point {    /* 24 bytes */
    double p[3];
} rtr_probe_point;

typedef struct rtr_probe_vis {      /* 80 bytes */
    double c[9];
    int32_t count, valid;
} rtr_probe_vis;

typedef struct rtr_probe_sh {       /* 224 bytes */
    double c[9][3];                 /* [basis function][r, g, b] */
    int32_t count, valid;
} rtr_probe_sh;

int rtr_probe_visibility(rtr_context* ctx, const rtr_gather_params* params, const rtr_probe_point* points,
                         rtr_probe_vis* out, int64_t n);
int rtr_probe_radiance(rtr_context* ctx, const rtr_render_params* render, const rtr_gather_params* params,
                       const rtr_probe_point* points, rtr_probe_sh* out, int64_t n);
int rtr_probe_visibility_device(rtr_context* ctx, const rtr_gather_params* params, const rtr_probe_point* d_points,
                                rtr_probe_vis* d_out, int64_t n, int blocking);
int rtr_probe_radiance_device(rtr_context* ctx, const rtr_render_params* render, const rtr_gather_params* params,
                              const rtr_probe_point* d_points, rtr_probe_sh* d_out, int64_t n, int blocking);

/* Host-only, needs no context: ray s of the probe at `index_in_call`, like rtr_gather_ray.  RTR_ERR_INVALID for a bad
 * probe, bad params, a negative index or s outside [0, samples). */
int rtr_probe_ray(const rtr_gather_params* params, const rtr_probe_point* point, int64_t index_in_call, int32_t s,
                  rtr_ray* out);

/* Host-only: the nine basis functions at d (taken as given: the kernels pass unit vectors). */
void rtr_sh_basis(const double d[3], double y[9]);

/* Host-only: irradiance E[ch] at a surface with normal n lit by the radiance whose probe record holds c.
 *   w = unit(n), y = basis(w)
 *   per channel: e = +0.0; for i = 0..8 in order: e = e + (A[i] * y[i]) * c[i][ch]; E[ch] = 12.566370614359172 * e
 *   A = {3.141592653589793, 2.0943951023931953 x3, 0.7853981633974483 x5}: the clamped-cosine factors pi, 2 pi / 3, pi / 4
 * RTR_ERR_INVALID for a NULL pointer or a bad normal (the gathers' rule: a component not finite, or sqrt(n.n) not in (0, inf)). */
int rtr_sh_irradiance(const double c[9][3], const double n[3], double E[3]);

/* GRID LOOKUP: probes on a regular grid -> irradiance at query points (p, n), trilinear in the coefficients.
 * Probe (ix, iy, iz) of the grid has index ix + dims[0] * (iy + dims[1] * iz) in the rtr_probe_sh array and stands at
 * origin + (ix, iy, iz) * spacing.  origin finite; spacing finite and > 0; dims >= 1 with a product <= 2^24; pad 0.
 * Per axis a:
 *   f = (p[a] - origin[a]) / spacing[a];  f = min(max(f, 0.0), (double)(dims[a] - 1))     (a query outside is clamped)
 *   i0 = (int)f;  if i0 > dims[a] - 2: i0 = max(dims[a] - 2, 0)
 *   t = f - (double)i0, and t = 0 when dims[a] == 1;  w0 = 1.0 - t, w1 = t
 * The corners are visited with dz outermost, then dy, then dx, each in {0, 1}, every index clipped to dims - 1:
 *   w = (wx * wy) * wz;  the corner is USED if w > 0 and its probe has valid != 0
 *   a used corner: wsum = wsum + w and acc[i][ch] = acc[i][ch] + w * probe.c[i][ch]
 * No used corner: {0, 0, 0, count 0, valid 0}.  Otherwise c = (1.0 / wsum) * acc, v = rtr_sh_irradiance(c, n),
 * count = the used corners, valid 1.  A BAD query is a bad gather point: the host entry rejects the batch and names the
 * index, the device entry writes valid 0 for it without reading a probe.  Neither entry needs a scene; n == 0 is RTR_OK. */
typedef struct rtr_probe_grid {     /* 64 bytes */
    double origin[3], spacing[3];
    int32_t dims[3], pad;
} rtr_probe_grid;

int rtr_probe_lookup(rtr_context* ctx, const rtr_probe_grid* grid, const rtr_probe_sh* probes,
                     const rtr_gather_point* queries, rtr_gather_out* out, int64_t n);
int rtr_probe_lookup_device(rtr_context* ctx, const rtr_probe_grid* grid, const rtr_probe_sh* d_probes,
                            const rtr_gather_point* d_queries, rtr_gather_out* d_out, int64_t n, int blocking);
/* Host-only, needs no context: the lookup of one query over HOST probes, the same function the kernel calls.
 * RTR_ERR_INVALID for a bad grid, a bad query or a NULL pointer. */
int rtr_probe_lookup_one(const rtr_probe_grid* grid, const rtr_probe_sh* probes, const rtr_gather_point* query,
                         rtr_gather_out* out);

/* ---- probe distance maps: how far a probe sees in each direction, and a grid lookup that weighs probes by it ----
 * The grid lookup above blends the eight probes around a query by distance alone, so a query next to a wall takes light
 * from the probe behind it.  A distance map records per probe the mean and the mean square of the distance to the nearest
 * surface over an octahedral map of directions; rtr_probe_lookup_visible weighs every corner by the chance that the query
 * is no farther from the probe than what the probe sees that way (the Chebyshev test of Majercik et al., "Dynamic Diffuse
 * Global Illumination with Ray-Traced Irradiance Fields", JCGT 2019).  Every output bit is defined here: only + - * / sqrt,
 * |x| and compares are used, in the order written, without contraction; x*x + y*y + z*z is (x*x + y*y) + z*z;
 * unit(w) = (1 / sqrt(w.x*w.x + w.y*w.y + w.z*w.z)) * w is the gathers';  sg(t) = (t >= 0) ? 1.0 : -1.0.
 *
 * OCTAHEDRAL MAP: T x T texels, row b, column a, 1 <= T <= 64, over the square (u, v) in [-1, 1]^2.
 *   DECODE (u, v) -> d:   z = (1.0 - |u|) - |v|
 *                         z >= 0: x = u, y = v;   else: x = (1.0 - |v|) * sg(u), y = (1.0 - |u|) * sg(v)
 *                         d = unit(x, y, z)                                           (rtr_octa_decode is the host form)
 *   ENCODE d -> (ox, oy): s = (|x| + |y|) + |z|, which must be > 0; d need not be unit
 *                         ox = x / s, oy = y / s
 *                         z < 0: (ox, oy) = ((1.0 - |oy|) * sg(ox), (1.0 - |ox|) * sg(oy)), both from the old values
 *                                                                                     (rtr_octa_encode is the host form)
 *
 * rtr_probe_depth: for each of `n` probes (rtr_probe_point) a T x T map of rtr_probe_depth_texel records, laid out
 * [probe][row b][column a], T = params->map_size, each texel reduced from N = params->samples rays.
 * RAY s (0 <= s < N) of texel e = b * T + a of probe k (k = its index in the call + params->point_base, modulo 2^32):
 *   state = rtr_sample_seed_inline(seed, T * T, e, (int32_t)k, s)                    (rtr_seed.h)
 *   jitter = 1: the captures' two draws, ju first, then jv.  jitter = 0: ju = jv = 0.5 and nothing is drawn.
 *   u = (2.0 * (a + ju)) / T - 1.0;  v = (2.0 * (b + jv)) / T - 1.0                   (a, b and T converted to double)
 *   d = DECODE(u, v)
 * The ray is (origin p, direction d, time, [t_min, t_max]) with the state left after the draws (rtr_probe_depth_ray is the
 * host form).  (hit, t, front_face) = what rtr_query_closest returns for that ray and state, draws inside media included;
 * d is a unit vector, so t is a distance.  x_s = hit ? t : t_max.  A sample adds x_s to `mean` and x_s * x_s to `mean2`;
 * a hit adds 1 to `hits`; a hit with front_face == 0 adds 1 to `back` (the probe looks at the inside of a surface;
 * front_face is the reference's, which translate and rotate_y set again from the normal that already faces the ray: a hit
 * under a transform always counts as a front face).
 * REDUCTION: the gathers', word for word, over the two sums and the two counts: G = min(64, bit_ceil(N)); lane l adds its
 * samples l, l + G, ... in increasing order into +0.0 / 0; then for off = G/2, ..., 1: a[l] = a[l] + a[l xor off]; then
 * mean = (1.0 / N) * a[0], mean2 likewise.  The counts are not scaled.
 *
 * params: 1 <= map_size <= 64; samples as the captures' (1 .. 2^20); jitter 0 or 1; pad 0; time finite; t_min finite (any
 * finite value: below 2^-100 the launch takes the plain IEEE divisions, the gathers' rule); t_max finite and > t_min --
 * it has NO default: it is the distance of a miss and bounds what a map can tell apart, so the caller sets it (a grid
 * wants somewhat more than its cell diagonal).  Everything else is the captures' contract: a probe is BAD if a component
 * of p is not finite; the host entry rejects the whole batch with RTR_ERR_INVALID, names the first bad index in
 * rtr_last_error and leaves the outputs untouched; the device entry writes all-zero records (valid 0) for every texel of
 * such a probe without casting, and every other texel gets valid = 1.  Bad params, n < 0 or a NULL array is
 * RTR_ERR_INVALID, a call before rtr_upload_scene RTR_ERR_NO_SCENE, in this order: context, params, n / NULL, scene -- all
 * before any device work.  n == 0 is RTR_OK without a launch.  The host entry stages the probes once in the buffer of the
 * gathers' host entries and brings the records back in slices of at most 2^20 texels; the device entry takes device
 * pointers (8-byte aligned; in and out must not overlap), runs on the context stream behind whatever is queued there and
 * returns at once unless `blocking`.  Neither touches anything a queued render or accumulator pass uses, nor the
 * statistics of rtr_get_stats; rtr_cancel does not apply.  Probes can be sharded over contexts: shard j passes
 * point_base = its first probe's index. */
typedef struct rtr_probe_depth_texel { /* 32 bytes */
    double mean, mean2;             /* of x_s and of x_s * x_s over the texel's samples */
    int32_t hits, back, valid, pad; /* pad is written 0 */
} rtr_probe_depth_texel;

typedef struct rtr_probe_depth_params { /* 48 bytes */
    int32_t map_size, samples;
    uint32_t seed, point_base;
    int32_t jitter, pad;            /* pad must be 0 */
    double time, t_min, t_max;
} rtr_probe_depth_params;

/* map_size 16, samples 8, seed 0, point_base 0, jitter 1, time 0, t_min 0.001, t_max 0: t_max must be set by the caller */
void rtr_probe_depth_defaults(rtr_probe_depth_params* p);

int rtr_probe_depth(rtr_context* ctx, const rtr_probe_depth_params* params, const rtr_probe_point* points,
                    rtr_probe_depth_texel* out, int64_t n);
int rtr_probe_depth_device(rtr_context* ctx, const rtr_probe_depth_params* params, const rtr_probe_point* d_points,
                           rtr_probe_depth_texel* d_out, int64_t n, int blocking);

/* Host-only, needs no context: ray s of texel (a, b) of the probe at `index_in_call` (the definition above; `point` is
 * that probe's record, not an array).  RTR_ERR_INVALID for a bad probe, bad params, a negative index, a or b outside
 * [0, T) or s outside [0, samples). */
int rtr_probe_depth_ray(const rtr_probe_depth_params* params, const rtr_probe_point* point, int64_t index_in_call, int32_t a,
                        int32_t b, int32_t s, rtr_ray* out);

/* Host-only: ENCODE and DECODE as defined above, the same functions the kernels call; the arguments are taken as given. */
void rtr_octa_encode(const double d[3], double uv[2]);
void rtr_octa_decode(const double uv[2], double d[3]);

/* VISIBLE GRID LOOKUP: rtr_probe_lookup with two more inputs, the distance maps of the grid's probes (`depth`:
 * [probe][b][a], probe indexed like the rtr_probe_sh array, T = params->map_size) and the parameter block below.  The grid
 * rule is rtr_probe_lookup's, and in addition probes * T * T <= 2^24; the query tests are rtr_probe_lookup's.
 *   w = unit(n);  pb = p + normal_bias * w                      (the point the visibility is tested at, lifted off the surface)
 *   axis weights and corner indices from the unbiased p, exactly as above; corners with dz outermost, then dy, then dx
 * A corner with probe position P[a] = origin[a] + (double)i[a] * spacing[a] (i: the clipped index) and
 * tri = (wx * wy) * wz is a CANDIDATE if tri > 0 and its rtr_probe_sh has valid != 0.  For a candidate:
 *   wrap weight:  e = P - p;  el2 = e.e;  cosn = (el2 > 0) ? (e.w) / sqrt(el2) : 0.0;  h = (cosn + 1.0) * 0.5;
 *                 wb = h * h + 0.2                               (a probe behind the surface still counts a little)
 *   visibility:   dv = pb - P;  r2 = dv.dv;  !(r2 > 0): c = 1.0.  Otherwise r = sqrt(r2) and (m1, m2, ok) = FETCH(dv) in
 *                 that probe's map;  !ok or r <= m1: c = 1.0.  Otherwise var = |m2 - m1 * m1|, dd = r - m1,
 *                 den = var + dd * dd,  c = (den > 0) ? var / den : 0.0,  then c = (c * c) * c
 *   weight:       wv = wb * c;  if !(wv >= 0x1p-20): wv = 0x1p-20;  wgt = tri * wv
 *   wsum = wsum + wgt;  acc[i][ch] = acc[i][ch] + wgt * probe.c[i][ch]
 * (a.b of two vectors is (a.x*b.x + a.y*b.y) + a.z*b.z.)  The ending is rtr_probe_lookup's: no candidate gives
 * {0, 0, 0, count 0, valid 0}; otherwise c = (1.0 / wsum) * acc, v = rtr_sh_irradiance(c, n), count = the candidates, valid 1.
 * FETCH(d):  (ox, oy) = ENCODE(d).  Per axis, with c = ox for the columns and c = oy for the rows:
 *     g = ((c + 1.0) * T) * 0.5 - 0.5;  i0 = (g < 0) ? -1 : (int)g;  t = g - (double)i0;  w0 = 1.0 - t, w1 = t
 *   There is no clamp: the indices -1 and T fold over the map's edge, where the octahedral square continues in itself.
 *   The four taps are visited with db outermost, then da, w = wa[da] * wb[db]; a tap is USED if w > 0.  Its index
 *   (ia, ib) = (i0a + da, i0b + db) is folded in this order:
 *     if ia < 0: (ia, ib) = (0, T-1-ib);   else if ia > T-1: (ia, ib) = (T-1, T-1-ib)
 *     then if ib < 0: (ib, ia) = (0, T-1-ia);   else if ib > T-1: (ib, ia) = (T-1, T-1-ia)
 *   m1 = m1 + w * mean, m2 = m2 + w * mean2, both from +0.0;  ok is false if a used tap has valid == 0.
 * 0.2, the cube and the floor 2^-20 are the published constants; here they are definitions.  The floor keeps a query that
 * no corner "can see" normalised, so it never comes out black.  params: 1 <= map_size <= 64; pad 0; normal_bias finite
 * and >= 0; reserved 0.  Checks in this order: context, grid, params, n / NULL; the host entry then rejects a batch with a
 * bad query and names the index; the device entry writes valid 0 for it without reading a probe.  No scene is needed;
 * n == 0 is RTR_OK.  The host entry stages the rtr_probe_sh records and the maps once and the queries in slices of 2^20;
 * the device entry is stream-ordered like the gathers' (8-byte aligned pointers, `blocking`). */
typedef struct rtr_probe_visible_params { /* 32 bytes */
    int32_t map_size, pad;          /* pad must be 0 */
    double normal_bias;             /* finite, >= 0 */
    double reserved[2];             /* 0 */
} rtr_probe_visible_params;

int rtr_probe_lookup_visible(rtr_context* ctx, const rtr_probe_grid* grid, const rtr_probe_sh* probes,
                             const rtr_probe_depth_texel* depth, const rtr_probe_visible_params* params,
                             const rtr_gather_point* queries, rtr_gather_out* out, int64_t n);
int rtr_probe_lookup_visible_device(rtr_context* ctx, const rtr_probe_grid* grid, const rtr_probe_sh* d_probes,
                                    const rtr_probe_depth_texel* d_depth, const rtr_probe_visible_params* params,
                                    const rtr_gather_point* d_queries, rtr_gather_out* d_out, int64_t n, int blocking);
/* Host-only, needs no context: the lookup of one query over HOST records, the same function the kernel calls.
 * RTR_ERR_INVALID for a bad grid, bad params, a bad query or a NULL pointer. */
int rtr_probe_lookup_visible_one(const rtr_probe_grid* grid, const rtr_probe_sh* probes, const rtr_probe_depth_texel* depth,
                                 const rtr_probe_visible_params* params, const rtr_gather_point* query, rtr_gather_out* out);

/* ---- environment captures: cube maps of radiance about points in space, their lookup, and Radiance .hdr output ----
 * Gathers and probes reduce what arrives at a point to one normal or to nine coefficients.  A capture keeps the directions:
 * for each of `n` centres (rtr_probe_point) six faces of S x S texels, each texel the mean of Integrator::Li over
 * N = params->samples rays through it, made in registers and reduced inside the wave like a gather.  The texel record is
 * rtr_gather_out (v = mean radiance, count = N, valid); the records are laid out [centre][face f][row b][column a], so a
 * call writes n * 6 * S * S of them.  Texels are indexed in 64 bits; 1 <= S <= 4096 (6 S^2 and a centre's texel index fit
 * an int32).  Every output bit is defined here; only + - * / sqrt and compares are used on the way to a ray, in the order
 * written, so a host, numpy and the device give the same bits (rtr_capture_ray is the host form).
 *
 * RAY s (0 <= s < N) of texel e = (f * S + b) * S + a of centre k (k = its index in the call + params->point_base, taken
 * modulo 2^32):
 *   state = rtr_sample_seed_inline(seed, 6 * S * S, e, (int32_t)k, s)            (rtr_seed.h)
 *   jitter = 1: two draws of the reference's random_double (core/rtweekend.h:24-34), each one xorshift32 step (13, 17, 5)
 *               and then state * 2^-32: ju first, then jv.  jitter = 0: ju = jv = 0.5 and nothing is drawn.
 *   u = (2.0 * (a + ju)) / S - 1.0;  v = (2.0 * (b + jv)) / S - 1.0               (a, b and S converted to double)
 *   d0 by face:  0 (+x): ( 1, -v, -u)    1 (-x): (-1, -v,  u)    2 (+y): ( u,  1,  v)
 *                3 (-y): ( u, -1, -v)    4 (+z): ( u, -v,  1)    5 (-z): (-u, -v, -1)
 *   d = unit(d0)                    unit(w) = (1 / sqrt(w.x*w.x + w.y*w.y + w.z*w.z)) * w, the gathers'
 * The ray is (origin = the centre, direction d, time) and the state left after the draws enters Li: x_s = what rtr_li_rays
 * returns for that ray and state under render->integrator, max_depth, rr_start_depth and flags, exactly as for
 * rtr_gather_radiance.  Face f looks down its axis with u to the right and v downwards as seen from the centre (the usual
 * cube-map table): row 0 is the top row of a face.
 *
 * REDUCTION: the gathers', word for word: G = min(64, bit_ceil(N)); lane l adds its samples l, l + G, ... in increasing
 * order into +0.0; then for off = G/2, ..., 1: a[l] = a[l] + a[l xor off]; then v = (1.0 / N) * a[0].  count = N.
 *
 * A centre is BAD if a component of p is not finite.  The host entry rejects the whole batch with RTR_ERR_INVALID, names
 * the first bad index in rtr_last_error and leaves the outputs untouched; the device entry writes an all-zero record
 * (valid 0) for every texel of such a centre without casting, and every other texel gets valid = 1.
 *
 * params: face_size and samples as above; jitter 0 or 1; time finite; reserved 0.  Anything else, a NULL render, n < 0 or
 * a NULL array is RTR_ERR_INVALID; a call before rtr_upload_scene is RTR_ERR_NO_SCENE -- all before any device work, in
 * the gathers' order.  n == 0 is RTR_OK without a launch.  The host entry takes host arrays and blocks; it stages the
 * centres once in the buffer of the gathers' host entries and brings the records back in slices of at most 2^20 texels.
 * The device entry takes device pointers (8-byte aligned; in and out must not overlap), runs on the context stream behind
 * whatever is queued there and returns at once unless `blocking`.  Neither touches anything a queued render or accumulator
 * pass uses, nor the statistics of rtr_get_stats; rtr_cancel does not apply.  Centres can be sharded over contexts: shard
 * j passes point_base = its first centre's index. */
typedef struct rtr_capture_params { /* 48 bytes */
    int32_t face_size, samples;
    uint32_t seed, point_base;
    int32_t jitter, pad;            /* pad must be 0 */
    double time;
    double reserved[2];
} rtr_capture_params;

/* face_size 32, samples 16, seed 0, point_base 0, jitter 1, time 0 */
void rtr_capture_defaults(rtr_capture_params* p);

int rtr_capture_cube(rtr_context* ctx, const rtr_render_params* render, const rtr_capture_params* params,
                     const rtr_probe_point* centres, rtr_gather_out* out, int64_t n);
int rtr_capture_cube_device(rtr_context* ctx, const rtr_render_params* render, const rtr_capture_params* params,
                            const rtr_probe_point* d_centres, rtr_gather_out* d_out, int64_t n, int blocking);

/* Host-only, needs no context: ray s of texel (a, b) of face `face` of the centre at `index_in_call` (the definition
 * above; `point` is that centre's record, not an array).  out->t_min = 0.001 and out->t_max = +inf, the defaults of the
 * queries: Li does not read them.  RTR_ERR_INVALID for a bad centre, bad params, a negative index, a face outside 0..5,
 * a or b outside [0, S) or s outside [0, samples). */
int rtr_capture_ray(const rtr_capture_params* params, const rtr_probe_point* point, int64_t index_in_call, int32_t face,
                    int32_t a, int32_t b, int32_t s, rtr_ray* out);

/* CUBE LOOKUP: the radiance of ONE capture (`texels`: its 6 S^2 records, 1 <= face_size <= 4096) along caller-given
 * directions; an rtr_probe_point holds a direction (x, y, z) here, which need not be normalised.
 *   major axis: the one of largest |component|; on a tie x wins over y and y over z.  m = that |component|.
 *   face and (u, v), the inverse of the table above, one division each:
 *     x major: x > 0: face 0, u = -z / m   else face 1, u =  z / m;   v = -y / m
 *     y major: y > 0: face 2, v =  z / m   else face 3, v = -z / m;   u =  x / m
 *     z major: z > 0: face 4, u =  x / m   else face 5, u = -x / m;   v = -y / m
 *   per axis, with c = u for the columns and c = v for the rows:
 *     g = ((c + 1.0) * S) * 0.5 - 0.5;  g = min(max(g, 0.0), (double)(S - 1))      (clamped to the face)
 *     i0 = (int)g;  if i0 > S - 2: i0 = max(S - 2, 0);   t = g - (double)i0, and t = 0 when S == 1;  w0 = 1.0 - t, w1 = t
 *   the four texels are visited with the row offset db outermost, then the column offset da, each in {0, 1}, indices
 *   clipped to S - 1:  w = wa[da] * wb[db];  a texel is USED if w > 0;  acc = +0.0;  acc[ch] = acc[ch] + w * texel.v[ch]
 * The filter is bilinear inside the face only: there is NO filtering across faces, a direction near a cube edge reads
 * the clamped texels of its own face.  Result: v = acc, count = the texels used, valid 1.  {0, 0, 0, count 0, valid 0}
 * when a component of the direction is not finite, sqrt(x*x + y*y + z*z) is not in (0, +inf), or a used texel has
 * valid == 0 -- the entries reject nothing per direction.  face_size outside 1 .. 4096, n < 0 or a NULL array is
 * RTR_ERR_INVALID; n == 0 is RTR_OK; no scene is needed.  The host entry stages the texels once and the directions in
 * slices of 2^20; the device entry is stream-ordered like the gathers' (8-byte aligned pointers, `blocking`). */
int rtr_cube_lookup(rtr_context* ctx, int32_t face_size, const rtr_gather_out* texels, const rtr_probe_point* directions,
                    rtr_gather_out* out, int64_t n);
int rtr_cube_lookup_device(rtr_context* ctx, int32_t face_size, const rtr_gather_out* d_texels,
                           const rtr_probe_point* d_directions, rtr_gather_out* d_out, int64_t n, int blocking);
/* Host-only, needs no context: the lookup of one direction over HOST texels, the same function the kernel calls. */
int rtr_cube_lookup_one(int32_t face_size, const rtr_gather_out* texels, const rtr_probe_point* direction,
                        rtr_gather_out* out);

/* Host-only (uses libm): the direction of the centre of texel (i, j) of a W x H equirectangular map under the
 * reference's mapping (lighting/environmental_light.h:225-232): u = (i + 0.5) / W, v = (j + 0.5) / H,
 * phi = 2 pi u - pi, theta = pi v, d = (sin(theta) * cos(phi), cos(theta), -sin(theta) * sin(phi)).  Row 0 is the top.
 * RTR_ERR_INVALID for W or H < 1, a texel outside the map or a NULL d. */
int rtr_latlong_direction(int32_t W, int32_t H, int32_t i, int32_t j, double d[3]);

/* Host-only: out_rgb[(j * W + i) * 3 + ch] = rtr_cube_lookup_one(face_size, texels, rtr_latlong_direction(W, H, i, j)).v[ch],
 * and nothing else (an invalid lookup gives 0).  RTR_ERR_INVALID for a bad size or a NULL pointer. */
int rtr_cube_to_latlong(int32_t face_size, const rtr_gather_out* texels, int32_t W, int32_t H, double* out_rgb);

/* Host-only: writes H rows (row 0 first: the top) of W texels, 3 doubles each, as a Radiance picture with flat
 * scanlines: the header "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y H +X W\n", then 4 bytes per texel.  A negative or NaN
 * channel counts as 0; m = the largest channel.  m < 1e-32: four zero bytes.  Otherwise (f, e) = frexp(m),
 * scale = (f * 256.0) / m, each of the three bytes is (int)(c * scale), at most 255, and the fourth is e + 128 (m above
 * 2^127 is stored as four bytes 255: the format ends there).  A reader's texel is byte * 2^(e - 136): never above the
 * input, and below it by less than 2^(e - 136).  (Inherent to flat files: readers take a file of 8 <= W < 32768 whose
 * very first texel is the bytes 2, 2, b < 128 for run-length encoded.)  RTR_ERR_INVALID for W or H < 1 or a NULL pointer,
 * RTR_ERR_DEVICE when the file cannot be written. */
int rtr_write_rgbe(const char* path, int32_t W, int32_t H, const double* rgb);

/* ---- filtered cube maps: a GGX-filtered level made on the device from a capture, and a seam-aware lookup that blends two
 * levels by roughness ----
 * A glossy object needs the capture convolved with its specular lobe at several roughnesses.  rtr_cube_filter makes one
 * such level: every texel of an output cube of face size face_out is a DEFINED SUM over all 6 face_in^2 texels of the
 * source cube (brute force, no Monte-Carlo prefilter: no noise, no sin / cos, a definition independent of the
 * implementation).  Only + - * / sqrt and compares, no fused multiply-add: every product is rounded before its add, so a
 * host (rtr_cube_filter_one), numpy and the device give the same bits.  Records are rtr_gather_out, cubes are laid out
 * [cube][face][row][column] as the captures': texels holds n_cubes * 6 face_in^2 records, out n_cubes * 6 face_out^2.
 *
 * FILTER: output texel (f, b, a) of cube k.
 *   R = its unit centre direction: the capture's RAY above with jitter 0 (ju = jv = 0.5) at S = face_out: d0 by the face
 *       table, R = unit(d0).
 *   Source texel j (0 <= j < 6 face_in^2, the record order [face][row][column]): d0 the same way at S = face_in,
 *       r2 = d0.x*d0.x + d0.y*d0.y + d0.z*d0.z,  L = unit(d0) = (1 / sqrt(r2)) * d0,
 *       dw = 1.0 / (r2 * sqrt(r2))                  (its solid angle; the common factor 4 / S^2 cancels)
 *   c = (R.x*L.x + R.y*L.y) + R.z*L.z               texel j is USED iff c > cos_cut
 *   h2 = (1.0 + c) * 0.5                            ((n.h)^2 for n = v = R)
 *   den = h2 * (alpha*alpha - 1.0) + 1.0
 *   w = (c * dw) / (den * den)                      (GGX D times n.l times dw; the numerator alpha^2 and the pi of D cancel
 *                                                    in the normalisation and are left out)
 * REDUCTION: the gathers' with G = 64 fixed.  Lane l visits j = l, l + 64, ... in increasing order and for each USED texel
 * does acc[ch] = acc[ch] + w * v[ch] (ch = 0, 1, 2) and wsum = wsum + w, all from +0.0, counts the texel and remembers
 * whether it had valid == 0.  Then for off = 32, 16, ..., 1: x[l] = x[l] + x[l xor off] on the four sums and the count.
 * Result: v = (1.0 / wsum) * acc, count = the texels used, valid 1.  The all-zero record (valid 0) is written when count
 * is 0, when a USED texel is invalid, or when wsum is not in (0, +inf).  Skipping texels that are not USED, or whole
 * blocks of them, changes no bit: an implementation may cull.
 *
 * params: 1 <= face_in, face_out <= 512; 2^-20 <= alpha <= 1 (alpha = roughness^2, the reference's a,
 * materials/material.h:399); 0 <= cos_cut < 1 written with a clear sign bit (-0.0 is rejected: one spelling per filter);
 * pad 0.  Bad params, n_cubes < 0 or a NULL array is RTR_ERR_INVALID, before any device work, context first as for the
 * captures; n_cubes == 0 is RTR_OK without a launch; no scene is needed.  The host entry takes host arrays and blocks: it
 * stages the source cubes once at the head of the buffer of the gathers' host entries and brings the records back in
 * slices of at most 2^20.  The device entry takes device pointers (8-byte aligned; texels and out must not overlap: both
 * RTR_ERR_INVALID before any launch), runs on the context stream behind whatever is queued there -- a
 * rtr_capture_cube_device, say -- needs no scratch memory and returns at once unless `blocking`.  A call is split into
 * launches over output texels so that no launch exceeds a fixed number of (output, source) pairs; the environment variable
 * RTR_FILTER_PAIRS=n, read at every call, lowers that cap (a test hook: the bits do not depend on it). */
typedef struct rtr_cube_filter_params { /* 32 bytes */
    int32_t face_in, face_out;
    double alpha;
    double cos_cut;
    int32_t pad[2];                 /* must be 0 */
} rtr_cube_filter_params;

/* face_in 32, face_out 16, alpha 0.25, cos_cut 0.0 */
void rtr_cube_filter_defaults(rtr_cube_filter_params* p);

int rtr_cube_filter(rtr_context* ctx, const rtr_cube_filter_params* params, const rtr_gather_out* texels,
                    rtr_gather_out* out, int64_t n_cubes);
int rtr_cube_filter_device(rtr_context* ctx, const rtr_cube_filter_params* params, const rtr_gather_out* d_texels,
                           rtr_gather_out* d_out, int64_t n_cubes, int blocking);
/* Host-only, needs no context: output texel (a, b) of face `face` from the 6 face_in^2 HOST records of one cube, the
 * arithmetic the kernel runs in the lane order above.  RTR_ERR_INVALID for bad params, a NULL pointer, a face outside
 * 0..5 or a, b outside [0, face_out). */
int rtr_cube_filter_one(const rtr_cube_filter_params* params, const rtr_gather_out* cube_texels, int32_t face, int32_t a,
                        int32_t b, rtr_gather_out* out);

/* A CHAIN is a set of 1 <= n_levels <= 13 cubes of one environment in one array of `n_records` records: level i has face
 * size levels[i].face_size (1 .. 4096), starts at record levels[i].offset and was filtered with levels[i].alpha.  The
 * alphas are finite and strictly increasing, offsets are >= 0, every level lies inside n_records, pads are 0: anything
 * else is RTR_ERR_INVALID in every entry below.
 *
 * PLAN (host only): the usual chain for a capture of face size S (1 .. 4096): level i has face_size = max(S >> i, 1),
 * offset = the records of the levels before it, alpha = r * r with r = (double)i / (n_levels - 1) (r = 0 for one level):
 * level 0 has alpha 0 and is the capture itself, level i > 0 is rtr_cube_filter of level 0 with that alpha (the caller
 * runs it: face_out > 512 is outside the filter).  *n_records = the records of all levels.  levels may be NULL to ask for
 * n_records alone. */
typedef struct rtr_cube_level {     /* 24 bytes */
    int32_t face_size, pad;
    int64_t offset;                 /* in records */
    double alpha;
} rtr_cube_level;
typedef struct rtr_cube_query {     /* 32 bytes */
    double d[3];                    /* direction, need not be normalised */
    double alpha;                   /* roughness^2 */
} rtr_cube_query;
int rtr_cube_chain_plan(int32_t face_size, int32_t n_levels, rtr_cube_level* levels, int64_t* n_records);

/* CHAIN LOOKUP of one query:
 *   a = min(max(q.alpha, alpha_0), alpha_last)
 *   i = the largest level with alpha_i <= a, capped at n_levels - 2 when there are two or more levels
 *   t = (a - alpha_i) / (alpha_{i+1} - alpha_i);  with one level t = 0
 *   t == 0: the result is X_i, and level i + 1 is not read.  Otherwise v = (1.0 - t) * X_i.v + t * X_{i+1}.v per channel,
 *   count = X_i.count + X_{i+1}.count, valid 1 -- and the zero record if either X is invalid.
 * A non-finite q.alpha, or a direction rtr_cube_lookup would reject, gives the zero record.
 *
 * X = the SEAM-AWARE LOOKUP of q.d in one level (S = its face size, its 6 S^2 records):
 *   face and (u, v) exactly as rtr_cube_lookup.
 *   per axis (c = u: columns, c = v: rows): g = ((c + 1.0) * S) * 0.5 - 0.5, NOT clamped;  i0 = floor(g), -1 .. S - 1;
 *     t = g - (double)i0;  w0 = 1.0 - t, w1 = t
 *   taps as there: db outermost, then da, each in {0, 1}: ia = i0a + da, ib = i0b + db, w = wa[da] * wb[db], USED iff w > 0,
 *     acc[ch] = acc[ch] + w * texel.v[ch] from +0.0
 *   a tap inside [0, S)^2 reads texel (ib, ia) of its own face.  Any other tap: u' = (2.0 * (ia + 0.5)) / S - 1.0 and v'
 *     likewise from ib; d0 = the face table at (u', v'), un-normalised; the major-axis rule of rtr_cube_lookup applied to d0
 *     gives (f'', u'', v''); the tap reads texel min(max((int)(((c'' + 1.0) * S) * 0.5), 0), S - 1) per axis of face f''.
 *     A corner tap, outside on both axes, resolves by the tie rule: x over y over z.
 *   v = acc, count = the taps used, valid 1; the zero record if a used texel has valid == 0.
 * This holds for S = 1 too, where it blends the six texels.  The filter is continuous across cube edges: a tap beyond an
 * edge lands on the neighbouring face's edge texel, and that texel's outward tap comes back.  It is NOT a true three-face
 * filter at the corners, where the fourth tap is one of the three texels that meet there.  rtr_cube_lookup itself stays
 * unfiltered across faces and keeps its bits.
 *
 * n < 0 or a NULL array is RTR_ERR_INVALID, n == 0 is RTR_OK, no scene is needed.  The host entry stages the n_records
 * texels once and the queries in slices of 2^20; the device entry (levels is a HOST array, copied at the call) is
 * stream-ordered like the gathers' (8-byte aligned pointers, `blocking`). */
int rtr_cube_chain_lookup(rtr_context* ctx, const rtr_cube_level* levels, int32_t n_levels, const rtr_gather_out* texels,
                          int64_t n_records, const rtr_cube_query* queries, rtr_gather_out* out, int64_t n);
int rtr_cube_chain_lookup_device(rtr_context* ctx, const rtr_cube_level* levels, int32_t n_levels,
                                 const rtr_gather_out* d_texels, int64_t n_records, const rtr_cube_query* d_queries,
                                 rtr_gather_out* d_out, int64_t n, int blocking);
/* Host-only, needs no context: one query over HOST records, the same function the kernel calls.  RTR_ERR_INVALID for a bad
 * chain (checked against the level ends: there is no n_records here) or a NULL pointer. */
int rtr_cube_chain_lookup_one(const rtr_cube_level* levels, int32_t n_levels, const rtr_gather_out* texels,
                              const rtr_cube_query* query, rtr_gather_out* out);

/* ---- image-based shading: the environment BRDF table of the split-sum approximation, and one fused call that turns a
 * probe grid, a filtered cube chain and that table into the radiance a PBRMaterial surface sends to a viewer ----
 * rtr_probe_lookup(_visible) gives an irradiance E, rtr_cube_chain_lookup a prefiltered radiance X.  The third factor of
 * the split sum is the directional albedo of the specular lobe, int f_spec cos dw ~ F0 * a + b, tabulated over
 * (mu = n.v, roughness) for the reference's D, G, F and its + 0.0001 (materials/material.h:372-432).  Everything below
 * is FP64 with + - * / sqrt and compares only, no libm and no fused multiply-add: every product is rounded before its
 * add, so a host (the _one forms), numpy and the device give the same bits.
 *
 * TABLE: n_rough x n_mu records {a, b}, row = roughness: record r * n_mu + c is ENTRY (r, c).
 *   rough = (r + 0.5) / n_rough,  mu = (c + 0.5) / n_mu,  alpha = rough * rough,  a2 = alpha * alpha,
 *   k = alpha * 0.5                                 (GeometrySchlickGGX, whose k is roughness^2 / 2),   omk = 1.0 - k
 *   Vx = sqrt(1.0 - mu * mu),  Vz = mu,  g1v = mu / (mu * omk + k)
 * A defined quadrature with M = `nodes` over the half vector, in the coordinates in which GGX importance sampling is
 * uniform (D cancels; the sharp lobe of a low roughness needs no fine grid), the azimuth through the rational
 * parametrisation of the circle (no sin / cos).  NODE j, 0 <= j < 2 M^2:
 *   sx = +1.0 for j < M^2, else -1.0;  jj = j mod M^2;  s = (jj / M + 0.5) / M  (integer jj / M),  t = (jj mod M + 0.5) / M
 *   den = a2 + (1.0 - a2) * (s * s),  c2 = (s * s) / den,  Hz = sqrt(c2),  sh = sqrt(max(1.0 - c2, 0.0))
 *   q = 1.0 + t * t,  Hx = sh * (sx * ((1.0 - t * t) / q)),  wphi = 1.0 / q
 *   vh = Vx * Hx + Vz * Hz,  nl = (2.0 * vh) * Hz - Vz       (Vy = 0: Hy never enters)
 *   every node:  W = W + wphi * s.     The node is USED iff nl > 0 and vh > 0; a USED node also does
 *   g = g1v * (nl / (nl * omk + k))
 *   e = (((g * nl) * (4.0 * vh)) * sqrt(den)) / ((4.0 * mu) * nl + 0.0001)
 *   x = 1.0 - vh,  fc = ((x * x) * (x * x)) * x
 *   A = A + wphi * (e * (1.0 - fc)),  B = B + wphi * (e * fc)
 * REDUCTION: the gathers' with G = 64 fixed.  Lane l visits j = l, l + 64, ... in increasing order, W, A, B from +0.0; then
 * for off = 32, 16, ..., 1: x[l] = x[l] + x[l xor off] on the three sums.  a = (1.0 / W) * A, b = (1.0 / W) * B.
 *
 * params: 1 <= n_mu, n_rough, nodes <= 256; pad and reserved 0.  Bad params or a NULL pointer is RTR_ERR_INVALID before
 * any device work, context first; no scene is needed.  The host entry blocks and brings the records back through the
 * buffer of the gathers' host entries; the device entry takes a device pointer (8-byte aligned), runs on the context
 * stream behind whatever is queued there, needs no scratch memory and returns at once unless `blocking`.  A call is split
 * into launches over runs of entries so that no launch exceeds a fixed number of nodes; the environment variable
 * RTR_TABLE_NODES=n, read at every call, lowers that cap (a test hook: the bits do not depend on it). */
typedef struct rtr_brdf_params {    /* 32 bytes */
    int32_t n_mu, n_rough;
    int32_t nodes;                  /* M */
    int32_t pad;                    /* must be 0 */
    double reserved[2];             /* must be 0 */
} rtr_brdf_params;
typedef struct rtr_brdf_entry {     /* 16 bytes */
    double a, b;
} rtr_brdf_entry;

int rtr_brdf_table(rtr_context* ctx, const rtr_brdf_params* params, rtr_brdf_entry* out);
int rtr_brdf_table_device(rtr_context* ctx, const rtr_brdf_params* params, rtr_brdf_entry* d_out, int blocking);
/* Host-only, needs no context: ENTRY (r, c), the arithmetic the kernel runs in the lane order above.  RTR_ERR_INVALID for
 * bad params, a NULL pointer, r outside [0, n_rough) or c outside [0, n_mu). */
int rtr_brdf_entry_one(const rtr_brdf_params* params, int32_t r, int32_t c, rtr_brdf_entry* out);
/* FETCH (host only, the function the shader calls): bilinear in the table at (mu, rough), texel centres at (i + 0.5) / n.
 *   per axis (x = mu with n = n_mu: columns; x = rough with n = n_rough: rows): g = x * n - 0.5,
 *     f = min(max(g, 0), n - 1),  i0 = (int)f capped at max(n - 2, 0),  t = f - (double)i0 (t = 0 for n == 1),
 *     w0 = 1.0 - t, w1 = t: the per-axis rule of rtr_probe_lookup
 *   taps: dr outermost, then dc, each in {0, 1}: entry (min(i0r + dr, n_rough - 1), min(i0c + dc, n_mu - 1)),
 *     w = wc[dc] * wr[dr], read iff w > 0:  a = a + w * entry.a, b = b + w * entry.b from +0.0
 * RTR_ERR_INVALID for n_mu or n_rough outside 1 .. 256, a NULL pointer or a non-finite mu or rough. */
int rtr_brdf_fetch_one(int32_t n_mu, int32_t n_rough, const rtr_brdf_entry* table, double mu, double rough,
                       rtr_brdf_entry* out);

/* SHADE: the radiance of one surface point towards its viewer under an ENVIRONMENT: a probe grid (with its distance maps
 * and the parameters of rtr_probe_lookup_visible, or both NULL for the plain rtr_probe_lookup), a cube chain and a table.
 * `parts` selects the terms: RTR_SHADE_DIFFUSE | RTR_SHADE_SPECULAR, at least one.  The arrays of a part that is not
 * selected (grid, probes, depth, visible / levels, chain) may be NULL and are not read; the table serves both.  The struct
 * is a HOST struct, copied at the call with the grid, the visible params and the levels it points to; probes, depth, chain
 * and table are host arrays for the host entry and rtr_shade_ibl_one, device arrays for the device entry.
 *
 * A query is BAD when one of its 14 fields is not finite or when n or v has a length outside (0, inf) (the gathers' rule).
 *   N = (1 / |n|) * n,  Vd = (1 / |v|) * v   with |x| = sqrt(x.x*x.x + x.y*x.y + x.z*x.z)
 *   mu = (N.x*Vd.x + N.y*Vd.y) + N.z*Vd.z,  muc = max(mu, 0.0)
 *   rough = min(max(roughness, 0.01), 1.0)          (material.h:368),   alpha = rough * rough
 *   DIFFUSE:  Erec = rtr_probe_lookup(_visible) of the query (p, n)
 *   SPECULAR: R = (2.0 * mu) * N - Vd per component,  Xrec = rtr_cube_chain_lookup of (R, alpha)
 *   (a, b) = FETCH at (muc, rough)
 *   per channel: F0 = (1.0 - metallic) * 0.04 + metallic * base                  (material.h:375)
 *     kS = F0 * a + b,  kD = (1.0 - kS) * (1.0 - metallic)
 *     diffuse = ((kD * base) * Erec.v) / pi,  specular = Xrec.v * kS              (pi = 3.1415926535897932385)
 *     v = diffuse + specular with both parts, else the selected term alone
 *   valid = 1 and count = the sum of the selected parts' counts when every selected part's record is valid; the all-zero
 *   record otherwise (the chain is not read when the diffuse record is invalid).
 *
 * Entries: env, its table (1 <= n_mu, n_rough <= 256) and the arrays of the selected parts are checked with the rules of
 * the lookups they name (grid, visible params, chain against n_records); parts outside 1 .. 3, depth without visible or
 * visible without depth, n < 0 or a NULL array is RTR_ERR_INVALID, before any device work, context first; n == 0 is
 * RTR_OK; no scene is needed.  The host entry rejects a batch with a BAD query, naming its index, with `out` untouched; it
 * stages the records once at the head of the buffer of the gathers' host entries and the queries in slices of 2^20.  The
 * device entry (8-byte aligned pointers; out must not overlap the queries or any array read: RTR_ERR_INVALID) writes the
 * all-zero record for a BAD query without reading a record, runs on the context stream behind whatever is queued there --
 * rtr_cube_filter_device, rtr_probe_radiance_device and rtr_brdf_table_device, say -- and returns at once unless
 * `blocking`. */
#define RTR_SHADE_DIFFUSE 1
#define RTR_SHADE_SPECULAR 2
typedef struct rtr_shade_env {      /* 80 bytes */
    int32_t parts;                  /* RTR_SHADE_* */
    int32_t n_levels;
    const rtr_probe_grid* grid;     /* host */
    const rtr_probe_sh* probes;     /* dims[0] * dims[1] * dims[2] records */
    const rtr_probe_depth_texel* depth;         /* probes * map_size^2 records, or NULL */
    const rtr_probe_visible_params* visible;    /* host; NULL with depth NULL: the plain lookup */
    const rtr_cube_level* levels;   /* host, n_levels of them */
    const rtr_gather_out* chain;    /* n_records records */
    int64_t n_records;
    const rtr_brdf_entry* table;    /* n_rough * n_mu records */
    int32_t n_mu, n_rough;
} rtr_shade_env;
typedef struct rtr_shade_query {    /* 112 bytes */
    double p[3];                    /* position */
    double n[3];                    /* surface normal, need not be normalised */
    double v[3];                    /* towards the viewer, need not be normalised */
    double base[3];                 /* base colour */
    double roughness, metallic;
} rtr_shade_query;

int rtr_shade_ibl(rtr_context* ctx, const rtr_shade_env* env, const rtr_shade_query* queries, rtr_gather_out* out, int64_t n);
int rtr_shade_ibl_device(rtr_context* ctx, const rtr_shade_env* env, const rtr_shade_query* d_queries, rtr_gather_out* d_out,
                         int64_t n, int blocking);
/* Host-only, needs no context: one query over HOST arrays, the same function the kernel calls.  RTR_ERR_INVALID for a bad
 * environment, a NULL pointer or a BAD query. */
int rtr_shade_ibl_one(const rtr_shade_env* env, const rtr_shade_query* query, rtr_gather_out* out);

/* ---- baked previews: a frame of the uploaded scene shaded from a probe grid, a cube chain and a table ----
 * One launch per frame: every pixel casts k * k camera rays to their closest hit, turns each hit into an rtr_shade_query by
 * its material and adds rtr_shade_ibl of it; rays and queries never visit memory.  What an interactive viewer of a baked
 * scene shows while the path tracer converges.  FP64 throughout with + - * / sqrt and compares only, no fused
 * multiply-add, plain IEEE divisions for everything stated here (the casts inside use whatever a render of the scene uses):
 * a host, numpy and the device give the same bits.
 *
 * RAY: sample s (0 <= s < k * k) of pixel (i, j) of a W x H image, with a = s % k and b = s / k (b is the outer loop):
 *   u = (i + (a + 0.5) / k) / (W - 1),   v = (j + (b + 0.5) / k) / (H - 1)            (i, j, a, b, k, W - 1, H - 1 as doubles)
 *   origin = the camera's origin,  d = ((lower_left_corner + u * horizontal) + v * vertical) - origin per component
 *   (renderer/camera.h:32-40 without the lens offset),  time = time0,  t_min from the params,  t_max = +inf.
 * No lens offset and no draw: the picture is that of a pinhole at the lens centre.  For k = 1 these are the pixel-centre
 * rays of rtr_cli --pick.
 *
 * SAMPLE: the ray is cast to its closest hit with the traversal a render with `flags` walks (rtr_query_closest of it).
 *   miss:  kind = MISS, material = -1; direct = what Integrator::Li of RTR_INTEGRATOR_MIS returns for a camera ray that
 *     leaves the scene (rtr_li_rays of it): the sum of the environment lights' Le, or else the background.
 *   a diffuse_light:  kind = EMITTER; direct = the value of tex[0] at the hit on a front face, (0, 0, 0) on a back face.
 *   any other material:  kind = SURFACE;  q.p = the hit's p,  q.n = the hit record's normal (no normal map is applied, as
 *     for the feature buffers),  q.v = (-d.x, -d.y, -d.z), and by material
 *       lambertian   base = tex[0] at the hit   roughness = 1.0              metallic = 0.0
 *       metal        base = f[0..2]             roughness = f[3] (fuzz)      metallic = 1.0
 *       dielectric   base = (1, 1, 1)           roughness = 0.0              metallic = 1.0
 *       PBR          base = tex[0] at the hit   roughness = tex[1] at the hit (as it is: the shader clamps it)
 *                                               metallic = tex[2] at the hit
 *     A dielectric is a mirror of the environment: there is no refraction in a preview, a stated limit.
 *   Members not named are 0: q of a MISS or EMITTER sample, direct of a SURFACE sample.
 *
 * PIXEL: s = 0 .. k * k - 1 in order, acc from +0.0 per channel.  A MISS or EMITTER sample adds `direct`; a SURFACE sample
 * adds rtr_shade_ibl_one(env, q).v when that record is valid and nothing otherwise (a point outside the grid, invalid
 * probes or texels, a BAD query such as a zero normal).  linear = (1.0 / (k * k)) * acc per channel, like the resolve of a
 * render; lit = the number of samples that added something (every MISS and EMITTER sample, every valid SURFACE sample).
 *
 * Layouts: rtr_preview_samples writes record ((j - y0) * (x1 - x0) + (i - x0)) * k * k + s.  The frame entries write
 * linear[((j - y0) * row_stride + (i - x0)) * 3 + c] -- the layout of rtr_accum_resolve_device, so rtr_display_device may
 * follow with no host wait -- and, unless lit is NULL, lit[(j - y0) * row_stride + (i - x0)]; only region pixels are written.
 *
 * Checks, all before any device work and with the outputs untouched, context first: RTR_ERR_INVALID for a NULL pointer, W
 * or H below 2, an empty region or one outside the image, grid outside 1 .. 8, a flag bit other than
 * RTR_FLAG_REFERENCE_ORDER, a t_min that is not finite or below 2^-100, non-zero reserved; RTR_ERR_NO_SCENE before an
 * upload; RTR_ERR_UNSUPPORTED for a scene with media (isotropic materials: their free paths need the path's generator).
 * The frame entries check env with the rules of rtr_shade_ibl, and row_stride below the region's width is
 * RTR_ERR_INVALID.  The device entries want linear, the samples and the environment's arrays 8-byte aligned and lit 4-byte
 * aligned, and no output may overlap an array of the environment or the other output: RTR_ERR_INVALID.
 * The entries use the context's current camera (rtr_set_camera applies); rtr_cancel and rtr_get_stats do not apply.
 * rtr_preview takes the environment's arrays as HOST arrays, staged like those of rtr_shade_ibl, and blocks;
 * rtr_preview_device takes them as DEVICE arrays, runs on the context stream behind whatever is queued there -- the bakes
 * included -- and returns at once unless `blocking`.  The samples entries need no environment. */
typedef struct rtr_preview_params {   /* 64 bytes */
    int32_t image_width, image_height;  /* W, H >= 2 */
    int32_t x0, y0, x1, y1;             /* region, as in rtr_render_params */
    int32_t grid;                       /* k in 1 .. 8: k * k rays per pixel */
    int32_t flags;                      /* 0 or RTR_FLAG_REFERENCE_ORDER */
    double t_min;                       /* finite, >= 2^-100; default 0.001 */
    double reserved[3];                 /* must be 0 */
} rtr_preview_params;
#define RTR_PREVIEW_MISS 0
#define RTR_PREVIEW_EMITTER 1
#define RTR_PREVIEW_SURFACE 2
typedef struct rtr_preview_sample {   /* 144 bytes */
    rtr_shade_query q;                  /* all 0 unless kind == RTR_PREVIEW_SURFACE */
    double direct[3];                   /* the value of a MISS / EMITTER sample, else 0 */
    int32_t kind, material;             /* RTR_PREVIEW_*; material = -1 on a miss */
} rtr_preview_sample;

/* grid 1, t_min 0.001, everything else 0: the caller sets the image size and the region */
void rtr_preview_defaults(rtr_preview_params* params);
/* Host-only, needs no context: RAY of sample s of pixel (i, j), the function the kernel calls; rng_state is 1.
 * RTR_ERR_INVALID for a NULL pointer, bad params, a pixel outside the image or s outside [0, k * k). */
int rtr_preview_ray(const rtr_camera* camera, const rtr_preview_params* params, int32_t i, int32_t j, int32_t s, rtr_ray* out);
/* the G-buffer, for callers who shade themselves */
int rtr_preview_samples(rtr_context* ctx, const rtr_preview_params* params, rtr_preview_sample* out);
int rtr_preview_samples_device(rtr_context* ctx, const rtr_preview_params* params, rtr_preview_sample* d_out, int blocking);
int rtr_preview(rtr_context* ctx, const rtr_preview_params* params, const rtr_shade_env* env, double* h_linear,
                int64_t row_stride, int32_t* h_lit);
int rtr_preview_device(rtr_context* ctx, const rtr_preview_params* params, const rtr_shade_env* env, double* d_linear,
                       int64_t row_stride, int32_t* d_lit, int blocking);

/* ---- capture sets: several captures of one scene, each with the box it was taken in, read with parallax correction ----
 * rtr_shade_ibl reads its one chain along R as if the environment were infinitely far away, which is right only at the
 * capture's centre.  A CAPTURE SET holds 1 <= C <= 16 captures.  Capture k has a VOLUME: the point `centre` it was taken
 * from, the PROXY box its reflections are projected onto (the room), the REACH box of points it serves and the width `fade`
 * of the band inside the reach box over which its weight rises from 0 to 1.  A lookup at a point p along d intersects the
 * ray (p, d) with the proxy box of every capture that reaches p, reads that capture towards the intersection as seen from
 * its centre (box projection), and blends the captures by their weights.  Everything below is FP64 with + - * / and
 * compares only, no fused multiply-add (every product is rounded before its add), plain IEEE divisions; min(a, b) is b when
 * b < a and a otherwise.  A host (the _one forms), numpy and the device give the same bits.
 *
 * Rules of a set, RTR_ERR_INVALID in every entry below, before any device work, context first: n_captures in 1 .. 16;
 * fallback -1 or in 0 .. n_captures - 1; volumes not NULL; every number of every volume finite; per axis
 * proxy_lo < centre < proxy_hi strictly and proxy_lo <= reach_lo <= reach_hi <= proxy_hi; fade >= 0 with a clear sign bit
 * (-0.0 is rejected: one spelling per set, like cos_cut).  The struct and its volumes are HOST data, copied at the call;
 * the cap of 16 lets the set travel as a kernel argument.
 *
 * LAYOUT: `levels`, `n_levels` and `n_records` describe the chain of ONE capture, exactly as for rtr_cube_chain_lookup, and
 * every capture of a set has that plan.  The set's array holds C * n_records records level-major: cube k of level i
 * (S_i = its face size) starts at record levels[i].offset * C + k * 6 * S_i^2.  Level i of all captures is therefore
 * contiguous in the [cube][face][row][column] order that rtr_capture_cube(_device) with n = C and
 * rtr_cube_filter(_device) with n_cubes = C write: a set is baked in place with one capture call, and one filter call per
 * further level, and no copy.  With C = 1 it is the chain layout.
 *
 * SET LOOKUP of one query (p, d, alpha).  The query is BAD when one of its seven numbers is not finite or when
 * sqrt((d.x*d.x + d.y*d.y) + d.z*d.z) is not in (0, inf); a BAD query gives the zero record; pad is not read.
 * For k = 0 .. C - 1 in order, from acc = +0.0 per channel, wsum = +0.0, count = 0, used = 0:
 *   m = p[0] - reach_lo[0];  m = min(m, reach_hi[0] - p[0]);  then for a = 1, 2:  m = min(m, p[a] - reach_lo[a]),
 *     m = min(m, reach_hi[a] - p[a])
 *   m < 0: capture k does not reach p.
 *   w = 1.0 when fade == 0, else min(m / fade, 1.0).   Not w > 0: capture k does not reach p (a point on the face of a
 *     faded reach box is outside, on the face of an unfaded one inside).
 *   box projection: t = +inf;  for a = 0, 1, 2:  d[a] > 0: ta = (proxy_hi[a] - p[a]) / d[a];  d[a] < 0:
 *     ta = (proxy_lo[a] - p[a]) / d[a];  a zero component of either sign takes no part;  t = min(t, ta)
 *     x[a] = p[a] + t * d[a],   dk[a] = x[a] - centre[a]
 *   Xk = the CHAIN LOOKUP of (dk, alpha) in cube k (rtr_cube_chain_lookup's function over the level starts above).
 *     Xk invalid: the whole result is the zero record.
 *   acc[ch] = acc[ch] + w * Xk.v[ch];  wsum = wsum + w;  count += Xk.count;  used += 1
 * Then  used > 0: v = (1.0 / wsum) * acc per channel, that count, valid 1.
 *       used == 0 and fallback >= 0: the CHAIN LOOKUP of (d, alpha) in cube `fallback`, its record as it is -- no projection,
 *         no weight: the "sky" capture, and rtr_cube_chain_lookup / rtr_shade_ibl as a special case.
 *       used == 0 and fallback < 0: the zero record.
 * A lane whose point no capture reaches reads no record but the fallback's.  Stated limit: the lobe is not widened with
 * the distance to the proxy; alpha is used as given.
 *
 * rtr_capture_set_lookup: set, levels (against n_records) and n < 0 / NULL arrays as above; n == 0 is RTR_OK; no scene is
 * needed.  The host entry stages the C * n_records records once at the head of the buffer of the gathers' host entries and
 * the queries in slices of 2^20 (RTR_SET_SLICE=n, read at every call, lowers that: a test hook, the bits do not depend on
 * it); the device entry is stream-ordered behind the bakes (8-byte aligned pointers, out must not overlap an input,
 * `blocking`).  rtr_capture_set_lookup_one is host only, the function the kernel calls; RTR_ERR_INVALID for a bad set or
 * chain (checked against the level ends) or a NULL pointer, RTR_OK and the zero record for a BAD query.
 *
 * rtr_shade_ibl_set(_device, _one) is rtr_shade_ibl word for word, except that the SPECULAR record is the SET LOOKUP of
 * (q.p, R, alpha): env->chain is the set's array, env->levels / n_levels / n_records describe one capture, and the size and
 * overlap rules use C * n_records.  rtr_preview_set(_device) is rtr_preview with that shader.  `set` is not checked, and
 * may be NULL, when SPECULAR is not selected. */
typedef struct rtr_capture_volume {   /* 128 bytes */
    double centre[3];                 /* where the capture was taken */
    double proxy_lo[3], proxy_hi[3];  /* the box reflections are projected onto (the room) */
    double reach_lo[3], reach_hi[3];  /* the box of points this capture serves */
    double fade;                      /* width of the band inside `reach` over which the weight rises from 0 to 1 */
} rtr_capture_volume;
typedef struct rtr_capture_set {      /* host struct, copied at the call */
    int32_t n_captures, fallback;     /* 1 .. 16;  -1 or 0 .. n_captures - 1 */
    const rtr_capture_volume* volumes;/* host */
} rtr_capture_set;
typedef struct rtr_capture_query {    /* 64 bytes */
    double p[3], d[3], alpha, pad;    /* d need not be normalised; alpha = roughness^2; pad 0 */
} rtr_capture_query;

int rtr_capture_set_lookup(rtr_context* ctx, const rtr_capture_set* set, const rtr_cube_level* levels, int32_t n_levels,
                           const rtr_gather_out* records, int64_t n_records, const rtr_capture_query* queries,
                           rtr_gather_out* out, int64_t n);
int rtr_capture_set_lookup_device(rtr_context* ctx, const rtr_capture_set* set, const rtr_cube_level* levels, int32_t n_levels,
                                  const rtr_gather_out* d_records, int64_t n_records, const rtr_capture_query* d_queries,
                                  rtr_gather_out* d_out, int64_t n, int blocking);
int rtr_capture_set_lookup_one(const rtr_capture_set* set, const rtr_cube_level* levels, int32_t n_levels,
                               const rtr_gather_out* records, const rtr_capture_query* query, rtr_gather_out* out);
int rtr_shade_ibl_set(rtr_context* ctx, const rtr_shade_env* env, const rtr_capture_set* set, const rtr_shade_query* queries,
                      rtr_gather_out* out, int64_t n);
int rtr_shade_ibl_set_device(rtr_context* ctx, const rtr_shade_env* env, const rtr_capture_set* set,
                             const rtr_shade_query* d_queries, rtr_gather_out* d_out, int64_t n, int blocking);
int rtr_shade_ibl_set_one(const rtr_shade_env* env, const rtr_capture_set* set, const rtr_shade_query* query, rtr_gather_out* out);
int rtr_preview_set(rtr_context* ctx, const rtr_preview_params* params, const rtr_shade_env* env, const rtr_capture_set* set,
                    double* h_linear, int64_t row_stride, int32_t* h_lit);
int rtr_preview_set_device(rtr_context* ctx, const rtr_preview_params* params, const rtr_shade_env* env,
                           const rtr_capture_set* set, double* d_linear, int64_t row_stride, int32_t* d_lit, int blocking);

/* Host-only: the checks rtr_upload_scene() runs before touching the GPU.  Returns RTR_OK,
 * RTR_ERR_INVALID or RTR_ERR_UNSUPPORTED; `msg` (may be NULL) receives the reason. */
int rtr_validate_scene(const rtr_scene_desc* scene, rtr_scene_info* info, char* msg, size_t msg_cap);


#ifdef __cplusplus
}
#endif
#endif /* RTR_HIP_H */
