/*
 * rt_select.h -- from what is known about a scene and a call to the kernel that runs: THE place of every rule that
 * turns (SceneFacts, rtr_scene_info, integrator, flags) into a traversal, a k_mega instantiation, a k_li-shaped kernel,
 * a wavefront plan or a chunk count.  Host side, no HIP call, nothing else: a sibling of rt_lower.h, which finds the
 * facts out.  The units that launch (rtr_capi.hip, rtr_accum.hip, rtr_query.hip, rtr_gather.hip, rtr_probe.hip) ask here.
 */
#pragma once

#include "rt_kernels.h" /* park_words, mega_sortable, mega_pairable: what the instantiations are made of */
#include "rt_launch.h"
#include "rt_lower.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

/* which traversal a call uses: the compiled scene unless it does not exist or the caller asks
 * for the reference's visiting order */
inline int pick_trav(const SceneFacts& f, const rtr_scene_info& info, int flags) {
    if (info.has_media || (info.inverted_boxes && !info.fast_ok)) /* (hollow spheres as guarded references: compiled) */
        return info.program_steps > 0 && !(flags & RTR_FLAG_REFERENCE_ORDER) ? RT_TRAV_PROGRAM : RT_TRAV_MEDIA;
    if (!info.fast_ok || f.uv_order_dependent || (flags & RTR_FLAG_REFERENCE_ORDER))
        return RT_TRAV_EXACT;
    return f.flat_scene ? RT_TRAV_FLAT : RT_TRAV_FAST;
}
inline size_t stack_bytes(const SceneFacts& f, const rtr_scene_info& info, int trav) {
    const bool compiled = trav == RT_TRAV_FAST || trav == RT_TRAV_FLAT || rt_is_program(trav) || trav == RT_TRAV_TOP || trav == RT_TRAV_FLAT_GUARD;
    const int words = compiled ? f.fast_stack_words : info.stack_words + f.walk_extra_words;
    return (size_t)words * RTR_BLOCK * sizeof(int);
}
/* The RT_TRAV_* template value a per-ray kernel (k_li, k_features, k_query_*, k_gather_*, the unit kernels of the test
 * library) takes for a call with `flags`: flat scenes take RT_TRAV_FAST (same hits, one kernel for both), a program the
 * general program kernel, and with `top` a sub-scene 0 with a top tree RT_TRAV_TOP, like the megakernel. */
inline int per_ray_trav(const SceneFacts& f, const rtr_scene_info& info, int flags, bool top) {
    int trav = pick_trav(f, info, flags);
    if (trav == RT_TRAV_FLAT) trav = RT_TRAV_FAST;
    if (top && trav == RT_TRAV_FAST && f.top_tree) trav = RT_TRAV_TOP;
    return trav == RT_TRAV_PROGRAM ? RT_TRAV_PROGRAM_EXT : trav;
}

/* ---- the k_li family: k_li, k_gather_li and k_probe_li<INTEG, TRAV> ----
 * The traversals the per-ray kernels are instantiated for: TravsLi those of k_features and of the k_li-shaped kernels of
 * MIS and RR, TravsN1 those of path, PBR and NEE (the media kernel also serves the reference-order walk),
 * TravsTop those of the kernels that also walk a top tree (k_query_*, k_gather_any, k_probe_any). */
using TravsLi = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>;
using TravsN1 = TravSet<RT_TRAV_FAST, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA>;
using TravsTop = TravSet<RT_TRAV_FAST, RT_TRAV_TOP, RT_TRAV_PROGRAM_EXT, RT_TRAV_MEDIA, RT_TRAV_EXACT>;
constexpr bool integ_n1(int integ) { return integ != RTR_INTEGRATOR_MIS && integ != RTR_INTEGRATOR_RR; }
/* the traversal a k_li-shaped kernel of `integ` takes for per_ray_trav(..., top = false) */
inline int li_trav(int integ, int per_ray) { return integ_n1(integ) && per_ray == RT_TRAV_EXACT ? RT_TRAV_MEDIA : per_ray; }
/* Runtime (integrator, li_trav) -> template arguments: calls f(integral_constant<int, I>{}, integral_constant<int, T>{})
 * for the instantiation that exists; false, and no call, when none does (dispatch_trav, with the integrator in front) */
template <typename F>
bool dispatch_li(int integ, int trav, F&& f) {
    auto with = [&](auto i, auto travs) { return dispatch_trav(travs, trav, [&](auto t) { f(i, t); }); };
    switch (integ) {
    case RTR_INTEGRATOR_MIS: return with(std::integral_constant<int, RTR_INTEGRATOR_MIS>{}, TravsLi{});
    case RTR_INTEGRATOR_RR: return with(std::integral_constant<int, RTR_INTEGRATOR_RR>{}, TravsLi{});
    case RTR_INTEGRATOR_PATH: return with(std::integral_constant<int, RTR_INTEGRATOR_PATH>{}, TravsN1{});
    case RTR_INTEGRATOR_PBR: return with(std::integral_constant<int, RTR_INTEGRATOR_PBR>{}, TravsN1{});
    default: return with(std::integral_constant<int, RTR_INTEGRATOR_NEE>{}, TravsN1{});
    }
}

/* ---- the megakernel ----
 * Which k_mega instantiation a render runs: from what lower_scene found out about the scene, the integrator, the
 * traversal pick_trav() chose and the render flags.  `flags_in_effect` (may be null) receives the flags that changed
 * the choice. */
inline MegaVariant mega_variant(const SceneFacts& f, int integ, int trav, int flags, int* flags_in_effect) {
    MegaVariant v{integ, trav, RT_MS_FULL, false, false};
    /* MIS and RR have flat, lean and guarded kernels; the others the generic material set on the
     * general compiled-scene kernel, one program kernel -- the general one --, and the media kernel, which also serves
     * the reference-order traversal of scenes without media */
    const bool n1 = integ_n1(integ);
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
inline bool mega_queue(const MegaVariant& v, const RenderK& P, int flags) {
    return v.pair && P.tile_s0 == nullptr && !(flags & RTR_FLAG_STATIC_GRID) && P.W <= 65535 && P.H <= 65535 &&
           (long long)P.n_tiles * P.chunks * 4 < (1ll << 31);
}

/* What of a MegaLaunch follows from the scene, the integrator, the traversal pick_trav() chose, the flags and the kind
 * of call (`accum`: MegaLaunch::accum): the variant, its stack and LDS, the persistent grid's bounds, the flags in
 * effect.  The call's own part (P, queue, stream, dsc) is the caller's. */
inline MegaLaunch mega_plan(const SceneFacts& f, const rtr_scene_info& info, int integ, int trav_in, int flags, int accum, int n_cus) {
    MegaLaunch L{};
    const MegaVariant& v = L.variant = mega_variant(f, integ, trav_in, flags, &L.flags_in_effect);
    L.stack_words = (int)(stack_bytes(f, info, v.trav) / (RTR_BLOCK * sizeof(int)));
    /* (the reference-order walk of PBR / NEE runs the media kernel with the parked words of the traversal that was
     * asked for, as it always has: workgroups per CU decide the chunking of a render, and that its rounding) */
    const int park = v.sorted ? SK_WORDS : park_words(integ, trav_in == RT_TRAV_EXACT ? RT_TRAV_EXACT : v.trav);
    L.lds = stack_bytes(f, info, v.trav) + (size_t)park * RTR_BLOCK * sizeof(double);
    L.accum = accum;
    L.n_cus = n_cus;
    /* (RTR_QUEUE_WORKGROUPS = n caps the persistent grid: with 1, four waves eat every block of a small image) */
    if (const char* g = getenv("RTR_QUEUE_WORKGROUPS")) L.grid_cap = std::atoi(g);
    if (v.pair && accum == 0 && (flags & RTR_FLAG_STATIC_GRID)) L.flags_in_effect |= RTR_FLAG_STATIC_GRID;
    return L;
}

/* ---- the wavefront pipeline: its plan, or why this call cannot run on it (RTR_ERR_UNSUPPORTED, the reason in `err`) ---- */
inline int wavefront_plan(const SceneFacts& f, const rtr_scene_info& info, int trav, int flags, bool has_lights, int n_cus,
                          WavefrontPlan& plan, std::string& err) {
    const char* why = nullptr;
    if (!f.machine_ok || (trav != RT_TRAV_FLAT && trav != RT_TRAV_FAST && trav != RT_TRAV_PROGRAM))
        why = "the wavefront pipeline runs the compiled traversals only: this graph (or "
              "RTR_FLAG_REFERENCE_ORDER) needs the reference-order walk of the megakernel";
    else if ((flags & RTR_FLAG_WF_PERSISTENT) && f.guarded_program)
        why = "RTR_FLAG_WF_PERSISTENT: the traversal machine does not run step programs with "
              "guarded primitives (hollow spheres under bvh_nodes) or media under transforms; "
              "the lockstep stages do";
    if (why) return (err = why, RTR_ERR_UNSUPPORTED);
    plan = WavefrontPlan{};
    plan.has_lights = has_lights;
    plan.media = trav == RT_TRAV_PROGRAM;
    plan.lean = f.lean_materials && !plan.media;
    plan.quadlit = f.quad_lights_only && !info.needs_uv;
    plan.sort = !plan.lean && f.n_material_types > 1;
    plan.n_cus = n_cus;
    plan.lds = stack_bytes(f, info, trav);
    plan.trav = trav;
    plan.machine = (flags & RTR_FLAG_WF_PERSISTENT) != 0;
    return RTR_OK;
}

/* ---- chunks ----
 * auto chunking.  A workgroup renders one tile for one chunk of the samples.  More chunks = more, shorter
 * workgroups: the resident slots drain more evenly at the end of the launch, but every workgroup pays its
 * start-up once.  Model fitted to sweeps on scenes 21 / 23 / 9 (4-8 chunks beat 1-2 by 3-10 %, 32 lose
 * 10 %): efficiency = R / (R + 0.75) * s / (s + 2) with R = rounds over the resident slots and s = samples
 * per pixel and chunk; the best power of two is taken.  It picks 8 for C2 on one GPU and 16 for the 313
 * tiles one of 8 ranks owns. */
inline int auto_chunks(int pipeline, double resident_slots, int n_tiles, int spp) {
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

/* spp_chunks = 0: the library's choice for this pipeline, number of owned tiles and `resident`, the workgroups of the
 * kernel variant the chip holds at once (registers / LDS decide: 2-5 per CU) */
inline void choose_chunks(int pipeline, double resident, int n_tiles, int spp, int* chunks, int* guided) {
    *chunks = auto_chunks(pipeline, resident, n_tiles, spp);
    /* Guided chunks.  With equal chunks a launch ends with part of the chip waiting for the last full-size
     * workgroups -- a tenth of the time of a rank's eighth of C2 (313 tiles: 4.9 rounds over the resident slots).
     * Instead three quarters of the chunks carry 90 % of a pixel's samples and run first; the rest is cut into thirds
     * of that size and drains the launch.  Measured on one GPU, scene 21 800x800 spp 400, share of 1 / 2 / 4 / 8
     * ranks: 75.2 / 38.6 / 20.3 / 10.9 ms with equal chunks, 74.5 / 37.9 / 19.8 / 10.2 ms guided (100 / 98 / 94 / 91 %
     * of the ideal share).  Not worth it once the launch has tens of rounds anyway. */
    guided[0] = guided[1] = guided[2] = 0;
    const double rounds = (double)n_tiles * *chunks / resident;
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
}
