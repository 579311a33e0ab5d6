/*
 * rt_debug.h -- the seam between librtr_hip.so and librtr_hip_test.so (NOT part of include/: a renderer integration
 * never sees it).  The test library runs its own unit kernels over the device functions of rt_device.h; what it needs
 * from a context is where the uploaded scene lives and which stream and traversal a call would use.  One entry needs no
 * context: rtr_debug_scene_plan, the host-only answer to "which kernel will this scene get, and why".
 */
#pragma once

#include "rt_device.h"
#include "rtr_hip.h"

struct rtr_debug_view {
    DScene ds;          /* device pointers of the uploaded scene */
    hipStream_t stream; /* the context's stream */
    int device, n_cus, n_materials;
    int trav;           /* RT_TRAV_* template value of the per-ray kernels for a call with `flags` (per_ray_trav, rt_select.h) */
    size_t stack_bytes; /* LDS traversal stack per workgroup of that traversal */
    int flat_trav;      /* RT_TRAV_FLAT / RT_TRAV_FLAT_GUARD where the megakernel of such a call runs a flat kernel, else -1 */
    int lean_ok, quadlit_ok; /* mega_variant's predicates for RT_MS_LEAN / RT_MS_QUADLIT kernels (rt_select.h):
                                SceneFacts::lean_materials; quad_lights_only and no texture that reads (u,v) */
};
/* the kernels the last render call launched, recorded on the host when they are enqueued (no device work) */
struct rtr_debug_kernel {
    int pipeline;   /* RTR_PIPELINE_MEGAKERNEL / RTR_PIPELINE_WAVEFRONT; -1: no render has launched anything yet */
    int integrator; /* RTR_INTEGRATOR_* */
    int trav;       /* megakernel: RT_TRAV_* template value of k_mega (RT_TRAV_FLAT_GUARD, RT_TRAV_PROGRAM_EXT included);
                       wavefront: WavefrontPlan::trav (RT_TRAV_FLAT / RT_TRAV_FAST / RT_TRAV_PROGRAM) */
    int ms;         /* RT_MS_* of k_mega / of the wf_shade stage */
    int sorted;     /* k_mega's sorted instantiation / wf_shade<..., true> */
    int shade_phases; /* wavefront: bit PH set for every wf_shade<I, PH, ...> launched; 0 for the megakernel */
    int lean, quadlit, sort, media, machine; /* wavefront: the WavefrontPlan fields; 0 for the megakernel */
    int accum;      /* megakernel: the ACC template value of k_mega (0 one-shot, 1 accumulator pass, 2 with moments) */
    int pair;       /* megakernel: k_mega's pair-cast instantiation (PAIR = true) */
    int queue;      /* megakernel: k_mega_queue<integrator, trav, ms>, the job-queue twin of the pair-cast kernel, ran instead */
};
/* the kernel the last call of a batch family launched (of its last slice), recorded on the host when it is enqueued: one
 * record per family.  A family without a member leaves it as it starts */
enum { RTR_DEBUG_GATHER, RTR_DEBUG_PROBE, RTR_DEBUG_CAPTURE, RTR_DEBUG_PROBE_DEPTH, RTR_DEBUG_FAMILIES };
struct rtr_debug_batch {
    int integ;     /* k_gather_li / k_probe_li / k_capture_li<integ, trav>; -1: k_gather_any, k_probe_any, k_probe_depth */
    int trav;      /* RT_TRAV_* template value, after the EXACT -> MEDIA substitution of li_trav; -1: no such call yet */
    int broadcast; /* gathers: k_gather_any<T, true> */
    int lg;        /* log2 of the lanes that share a record (gather_lg of the samples) */
};
struct rtr_debug_li_out { /* per camera sample: what rtr_li_samples drops */
    double L[3];
    uint32_t rng_exit;
    int32_t n_closest, n_shadow, pad;
};
/* what lowering (rt_lower.h) and the variant decisions of rt_select.h make of a scene, without a device; the layout of
 * rtr_scene_plan (include/rtr_hip_test.h), which documents the members */
struct rtr_debug_plan {
    int32_t fast_ok, has_media, flat_scene, flat_guarded, lean_materials, quad_lights_only, uv_order_dependent, machine_ok;
    int32_t guarded_program, top_tree, needs_uv, n_material_types, shared_div, pair_cast;
    int32_t n_steps, n_visits, n_refs, fast_stack_words, walk_stack_words, n_tie_refs, n_guard_refs;
    int32_t pick_trav, mega_trav, mega_ms, mega_sorted, mega_pair;
    int32_t n_finish;
};
extern "C" {
/* validator + lower_scene + pick_trav + mega_variant for `integrator` and render `flags`; ref_flags[0 .. min(cap, n_refs))
 * receives rtr_node::reserved of every reference record, finish[0 .. min(finish_cap, n_finish)) the finish records
 * (struct FFin, 96 bytes each).  Returns the validator's status. */
int rtr_debug_scene_plan(const rtr_scene_desc* scene, int integrator, int flags, rtr_debug_plan* out, size_t size_of_out,
                         int32_t* ref_flags, int64_t cap, void* finish, int64_t finish_cap);
/* FInst::shape (RT_SHAPE_*) of the first min(cap, *n_inst) instances of sub-scene 0 after lower_scene; host only */
int rtr_debug_frame_shapes(const rtr_scene_desc* scene, int32_t* shapes, int64_t cap, int32_t* n_inst);
int rtr_debug_view_get(rtr_context* ctx, int flags, rtr_debug_view* view, size_t size_of_view);
int rtr_debug_last_kernel(rtr_context* ctx, rtr_debug_kernel* out, size_t size_of_out);
int rtr_debug_last_batch(rtr_context* ctx, int family, rtr_debug_batch* out, size_t size_of_out); /* family: RTR_DEBUG_* */
/* the kernel launches the context's last pass through the chunked launcher made (launch_records of rt_batch.h): 1 unless the
 * call held more records than the cap, which RTR_LAUNCH_RECORDS lowers; 0: none yet; -1: a NULL context */
int64_t rtr_debug_last_launches(rtr_context* ctx);
int rtr_debug_li(rtr_context* ctx, const rtr_render_params* params, const int32_t* ijs, rtr_debug_li_out* out, int64_t n);
void rtr_debug_set_error(rtr_context* ctx, const char* msg); /* rtr_last_error() of a failing rtr_test_* call */
/* Synthetic state into an accumulator, so that the product's own k_accum_errors / _plan / _commit / _resolve(_scatter) run on
 * sums, moments and counts no render produces: sum [n][3][RTR_BLOCK] and q [n][RTR_BLOCK] doubles in the tile layout of
 * d_sum / d_q (every lane of a tile, those outside the region included), count [n] ints >= 0, n the number of owned
 * tiles; q exactly when the accumulator keeps moments.  Waits for the context's stream, copies the arrays and sets the
 * host copy of the counts; no kernel.  RTR_ERR_INVALID, before any device work, for a NULL array, a wrong n, a negative
 * count or a q that does not match the moments flag. */
int rtr_debug_accum_load(rtr_context* ctx, rtr_accum* acc, const double* sum, const double* q, const int32_t* count, int64_t n);
}
