/*
 * rt_debug.h -- the seam between librtr_hip.so and librtr_hip_test.so (NOT part of include/: a renderer integration
 * never sees it).  The test library runs its own unit kernels over the device functions of rt_device.h; what it needs
 * from a context is where the uploaded scene lives and which stream and traversal a call would use.
 */
#pragma once

#include "rt_device.h"
#include "rtr_hip.h"

struct rtr_debug_view {
    DScene ds;          /* device pointers of the uploaded scene */
    hipStream_t stream; /* the context's stream */
    int device, n_cus, n_materials;
    int trav;           /* RT_TRAV_* template value of the per-ray kernels for a call with `flags` (per_ray_trav, rtr_capi.hip) */
    size_t stack_bytes; /* LDS traversal stack per workgroup of that traversal */
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
};
struct rtr_debug_li_out { /* per camera sample: what rtr_li_samples drops */
    double L[3];
    uint32_t rng_exit;
    int32_t n_closest, n_shadow, pad;
};
extern "C" {
int rtr_debug_view_get(rtr_context* ctx, int flags, rtr_debug_view* view, size_t size_of_view);
int rtr_debug_last_kernel(rtr_context* ctx, rtr_debug_kernel* out, size_t size_of_out);
int rtr_debug_li(rtr_context* ctx, const rtr_render_params* params, const int32_t* ijs, rtr_debug_li_out* out, int64_t n);
void rtr_debug_set_error(rtr_context* ctx, const char* msg); /* rtr_last_error() of a failing rtr_test_* call */
}
