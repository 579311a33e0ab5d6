/*
 * rt_launch.h -- host-side seams between the translation units of librtr_hip.so that launch for one another.  The
 * units are compiled in parallel: rtr_capi.hip (context, scene upload, renders, k_li), rtr_accum.hip, rtr_image.hip,
 * rtr_query.hip, rtr_gather.hip and rtr_probe.hip (one subject of include/rtr_hip.h each, with its kernels), rtr_mega.hip three times
 * (one integrator group each: RTR_MEGA_GROUP 0 = MIS, 1 = RR + path, 2 = PBR + NEE) and rtr_wavefront.hip (stage
 * kernels + their host driver).
 *
 * Which k_mega instantiation a render runs is decided once, by mega_plan() of rt_select.h; the MegaVariant travels in
 * MegaLaunch to the group's unit, which looks it up in its explicit list of instantiations.  kernel_lds() is the one
 * LDS-limit check of every launcher, and dispatch_trav() the one place a runtime RT_TRAV_* becomes a template argument
 * of the per-ray kernels.
 */
#pragma once

#include "rt_render.h"

#include <atomic>
#include <string>
#include <utility>

/* which stage instantiations a wavefront render actually ran, recorded on the host (rtr_debug_last_kernel; a megakernel
 * render records its MegaLaunch) */
struct LaunchedKernel {
    int trav = -1;   /* WavefrontPlan::trav */
    int ms = -1;     /* RT_MS_* of the wf_shade stage */
    int sorted = 0;  /* wf_shade<..., true> */
    int phases = 0;  /* bit PH set for every wf_shade<I, PH, ...> launched */
};

/* the k_mega<integ, trav, ms, sorted, ACC, pair> a render runs (ACC follows from the call: MegaLaunch::accum; a one-shot
 * render of a pair variant runs k_mega_queue<integ, trav, ms> instead unless RTR_FLAG_STATIC_GRID is set: MegaLaunch::queue) */
struct MegaVariant {
    int integ, trav, ms; /* RTR_INTEGRATOR_*, RT_TRAV_* template value, RT_MS_* */
    bool sorted, pair;   /* the sorted instantiation (RTR_FLAG_SORTED_SHADING) / the pair-cast twin of a flat MIS kernel */
};

/* one megakernel launch: the plan of rt_select.h (mega_plan), then the call's own part */
struct MegaLaunch {
    MegaVariant variant;
    int accum;          /* 0, or an accumulator pass: the k_mega<..., ACC = 1> twin of the variant, 2 with moments */
    size_t lds;         /* traversal stack + parked path state, bytes per workgroup */
    int stack_words;
    int n_cus, grid_cap;
    int flags_in_effect; /* the render flags that changed the choice */
    /* the job-queue twin of a pair-cast variant (rt_kernels.h: k_mega_queue; accum = 0 only): a persistent grid of the
     * workgroups the chip holds -- per_cu x n_cus, at most one per (tile, chunk), at most grid_cap if that is > 0 --
     * whose waves pull blocks of jobs through the counter behind the completion words, P.done[n_tiles * chunks];
     * the caller zeroes the words and the counter on the stream before the launch */
    bool queue;
    /* A kernel is PREPARED once per render, without touching the stream: its LDS checked and the attribute raised, and
     * with `occupancy` -- auto chunking and the queue's grid need it -- per_cu, the resident workgroups per CU, queried.
     * The launch proper (prepare = false) checks and queries nothing: per_cu travels here. */
    bool prepare, occupancy;
    int per_cu;
    hipStream_t stream;
    const DScene* dsc;
    RenderK P;
};
/* return an rtr_status; `err` receives the text of a failure */
int rtr_mega_launch_mis(MegaLaunch& L, std::string& err);
int rtr_mega_launch_rr_path(MegaLaunch& L, std::string& err);
int rtr_mega_launch_pbr_nee(MegaLaunch& L, std::string& err);

void rtr_launch_resolve(const ResolveK& R, hipStream_t stream);

/* The per-lane traversal stack lives in LDS: a graph that needs more than the CU has (e.g. the reference-order walk
 * of a hittable_list with thousands of direct children) cannot run that way.  `static_bytes`: the kernel's own static
 * LDS, which counts against the same 160 KiB.  Raises the kernel's dynamic limit where the launch needs it. */
template <typename K>
int kernel_lds(K kernel, size_t dynamic_bytes, size_t static_bytes, std::string& err) {
    if (dynamic_bytes + static_bytes > 160 * 1024) {
        err = "this traversal of the scene needs a deeper stack than 160 KiB of LDS holds";
        return RTR_ERR_UNSUPPORTED;
    }
    if (dynamic_bytes <= 64 * 1024) return RTR_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)dynamic_bytes);
    if (e == hipSuccess) return RTR_OK;
    err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e);
    return RTR_ERR_DEVICE;
}

/* Runtime traversal -> template argument: calls f(std::integral_constant<int, T>{}) for the T among Ts that equals
 * `trav`; false, and no call, when none does.  Ts is the set of instantiations the caller's kernel has. */
template <int... Ts>
using TravSet = std::integer_sequence<int, Ts...>;
template <int... Ts, typename F>
bool dispatch_trav(TravSet<Ts...>, int trav, F&& f) {
    return ((trav == Ts && (f(std::integral_constant<int, Ts>{}), true)) || ...);
}

struct WavefrontPool {
    void* slab = nullptr;
    size_t slab_bytes = 0;
    uint32_t* h_live = nullptr; /* pinned + mapped: live blocks after the newest compaction */
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release();
};
struct WavefrontPlan {
    bool has_lights, lean, quadlit, sort, media;
    bool machine; /* casting stages as persistent threads on the traversal machine instead of lockstep waves */
    int trav;     /* RT_TRAV_FLAT / RT_TRAV_FAST / RT_TRAV_PROGRAM */
    int n_cus;
    size_t lds; /* traversal stack of the extend / connect stages */
};
int wavefront_render(WavefrontPool& pool, const DScene* sc, const WavefrontPlan& plan, const RenderK& P, int integrator,
                     double* d_rgb, int64_t row_stride, unsigned char* tile_done, hipStream_t stream,
                     std::atomic<uint32_t>* cancelled_upto,
                     int* launches, LaunchedKernel* launched, std::string& err);
