/*
 * rt_kernels.h -- the template __global__ kernels of the path tracer (gfx950).
 *
 *  k_mega      megakernel: one workgroup = one 16x16 image tile (renderer/renderer.h:40-67),
 *              one lane = one pixel.  A lane runs its samples back to back: when a path ends
 *              the lane starts its pixel's next camera sample in the same loop iteration
 *              (in-lane path regeneration), so the 64 lanes of a wave stay busy although path
 *              lengths differ (P(k=4)=0.45, long tail).  Samples of a pixel are
 *              summed in sample order like renderer.h:72-79.
 *  k_mega_queue  the pair-cast loop of k_mega on a persistent grid: a lane whose (pixel, chunk) job is over pulls the next
 *              one from a launch-wide queue instead of idling until the slowest lane of its wave is through; same
 *              partial sums, same image (what a one-shot render of a pair-cast scene runs).
 *  k_li        Integrator::Li of single camera samples or caller-given rays, one lane each (rtr_li_samples / rtr_li_rays).
 *  k_gather_any / k_gather_li   hemisphere gathers (rtr_gather_*): a group of up to 64 lanes per point makes its samples'
 *              rays in registers, casts them (any-hit / Integrator::Li) and reduces them inside the wave.
 *  k_probe_any / k_probe_li     light probes (rtr_probe_*): the gathers' mapping over the whole sphere, every sample projected
 *              onto nine spherical harmonics; 9 or 27 sums per point instead of 3.
 *  k_capture_li   environment captures (rtr_capture_cube): the gathers' mapping with a cube-map texel as the point.
 *  k_features  first-hit albedo / normal / depth of a pixel's first K camera samples (rtr_accum_features).
 *  k_query_closest / k_query_any   hittable::hit of the scene root for caller-given rays (rtr_query_*).
 * Template kernels only, instantiated by the unit that launches them.  The non-template kernels live in one header per
 * subject, each included by one unit: rt_render_kernels.h, rt_accum_kernels.h, rt_image_kernels.h.
 */
#pragma once

#include "rt_render.h"

#ifndef RTR_MEGA_WAVES
#define RTR_MEGA_WAVES 4 /* min waves per SIMD the register allocator must leave room for */
#endif
#ifndef RTR_PROGRAM_WAVES
#define RTR_PROGRAM_WAVES 3 /* media scenes are traversal-latency bound: a third wave pays for the spills it causes */
#endif

/* Waves per SIMD the register allocator must leave room for, per kernel variant (measured: scene 23
 * 4.36 -> 5.12, scene 1 1.36 -> 1.63 Gsamples/s at 3 instead of 2; the variants with the full light
 * set or the reference-order walk lose 10-30 % there to spills) */
constexpr int mega_waves(int integ, int trav, int ms) {
    if (ms == RT_MS_LEAN) return RTR_MEGA_WAVES;
    if (rt_is_program(trav)) return RTR_PROGRAM_WAVES;
    if (trav == RT_TRAV_MEDIA || trav == RT_TRAV_EXACT) return 2;
    if (ms == RT_MS_QUADLIT) return 3;
    if (integ == RTR_INTEGRATOR_RR || integ == RTR_INTEGRATOR_PATH) return 3;
    return 2;
}

/* Which pair-cast kernels recast after a failed vote (trace_pair<true>, rt_device.h) and which keep the per-frame fallback
 * inside the instance loop: the lean material set's, whose kernels are bound by the vector instructions they issue
 * (cornell_mis x1.023, c5_shard x1.025).  With the recast in the kernels of the other sets mis_spheres lost 0.9 %
 * (k_mega_queue<4,4,2>: eight more spilled SGPRs) and four of their accumulator-pass kernels spilled two to four more
 * VGPRs: they compile the fallback's text, as before (profiles/r24_recast.txt). */
constexpr bool pair_recasts(int ms) { return ms == RT_MS_LEAN; }
/* Which of them run the rect and box runs of a frame as the one hand-placed routine (pair_runs_lean, rt_device.h): the same
 * set, whose kernels are bound by instruction issue and whose scenes hold no sphere.  Every other pair-cast kernel keeps
 * pair_runs<...>, and so does every kernel of a -DRTR_PAIR_RUNS_PLAIN build. */
constexpr bool pair_runs_routine(int ms) { return ms == RT_MS_LEAN; }

/* Per-lane path state that the ray casts do not touch lives in LDS between shading steps
 * ("parked"), so it does not occupy VGPRs across the traversal loops: throughput, radiance of
 * the sample, pixel sum, previous BSDF pdf and the pending light contribution.  Word k of lane l
 * is park[k * RTR_BLOCK + l] (8-byte words: conflict-free ds_read_b64 / ds_write_b64). */
#define RT_PARK_WORDS 19
struct Park {
    double* base;
    RT_DEV V3 get3(int k) const { return mk(base[k * RTR_BLOCK], base[(k + 1) * RTR_BLOCK], base[(k + 2) * RTR_BLOCK]); }
    RT_DEV void set3(int k, V3 v) const {
        base[k * RTR_BLOCK] = v.x, base[(k + 1) * RTR_BLOCK] = v.y, base[(k + 2) * RTR_BLOCK] = v.z;
    }
    RT_DEV double get(int k) const { return base[k * RTR_BLOCK]; }
    RT_DEV void set(int k, double v) const { base[k * RTR_BLOCK] = v; }
    /* a word that holds two 32-bit integers (lo, hi): one ds_read_b64 / ds_write_b64 like every other word */
    RT_DEV void get2(int k, uint32_t& lo, uint32_t& hi) const {
        const unsigned long long w = (unsigned long long)__double_as_longlong(base[k * RTR_BLOCK]);
        lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
    }
    RT_DEV void set2(int k, uint32_t lo, uint32_t hi) const {
        base[k * RTR_BLOCK] = __longlong_as_double((long long)((unsigned long long)lo | ((unsigned long long)hi << 32)));
    }
};
/* PK_NCAST: the lane's closest-hit (lo) and shadow (hi) cast counts, two uint32 (they end in the uint32 PathCounters);
 * PK_PIXEL: the lane's pixel (i lo, j hi), which never changes during the kernel: begin_sample reads it back instead
 * of walking tile_ids and dividing by the tile geometry for every new sample */
enum { PK_THR = 0, PK_L = 3, PK_ACC = 6, PK_PDF = 9, PK_NCAST = 10, PK_PIXEL = 11, /* every variant */
       PK_CONTRIB = 12, PK_SWI = 15, PK_STMAX = 18 };                                /* deferred shadow ray only */
/* a shadow request of shade_a_mis written straight into the parked words PK_SWI, PK_STMAX, PK_CONTRIB */
struct ParkedReq {
    bool valid;
    Park pk;
    RT_DEV void put(V3 wi, Real tmax, V3 contrib) {
        valid = true;
        pk.set3(PK_SWI, wi);
        pk.set(PK_STMAX, tmax);
        pk.set3(PK_CONTRIB, contrib);
    }
};
/* words a variant parks: the deferred shadow request exists only where the shadow ray is cast after the
 * BSDF sample (MIS-type integrators on scenes without media); fewer words = more workgroups per CU where
 * LDS, not registers, is the limit (the lean RR kernel: 92 VGPRs) */
constexpr int park_words(int integ, int trav) {
    return (integ == RTR_INTEGRATOR_RR || integ == RTR_INTEGRATOR_PATH || rt_is_program(trav) || trav == RT_TRAV_MEDIA)
               ? 12
               : RT_PARK_WORDS;
}

/* ---- material-sorted shading inside the workgroup ---------------------------------------------------------------
 * The variant for "every material, QuadLights, flat compiled scene" (scene 23's kernel) regroups the 256 paths of the
 * tile by the material class of their hit before it shades them.  Without it a wave runs the code of every class
 * that one of its lanes hit, one after the other, with the lanes whose ray left the scene idle all the while (half of
 * them on scene 23).  Per bounce: the lane that OWNS a path casts its ray, adds the emission term (it needs the ray
 * that hit the emitter) and takes a ticket in its class (one LDS atomic per wave and class); after a barrier every lane
 * knows the class totals, classes are laid out in wave-aligned ranges where 256 slots allow it, the owner writes
 * (hit point, normal, incoming direction, generator state, material) into its slot; after a second barrier lane i
 * SHADES slot i -- light sample, BSDF sample, roulette: waves past the last item skip shading altogether -- and writes
 * throughput / pdf / pending light contribution straight into the owner's parked words and the new direction into the
 * slot; after a third barrier the owner takes them back.  A path's generator state travels with it and every sum is
 * formed by the same operands in the same order, so the image is the unsorted kernel's bit for bit
 * (test_sorted_shading_equals_unsorted).  MEASURED ON SCENE 23: 4 063 against 6 617 Msamples/s unsorted -- the three
 * barriers cost 16 % of the wave cycles, tickets and exchange 7 %, the owner's emission pass and the second material
 * fetch another 6 %, and with four classes in four wave-aligned ranges every wave still shades (one class each):
 * profiles/r03_sorted_regions.txt.  It is therefore NOT what RTR_PIPELINE_AUTO runs; RTR_FLAG_SORTED_SHADING asks
 * for it. */
/* which (integrator, traversal, material set) has a sorted instantiation: RTR_FLAG_SORTED_SHADING selects it */
constexpr bool mega_sortable(int integ, int trav, int ms) {
    return integ == RTR_INTEGRATOR_MIS && trav == RT_TRAV_FLAT && ms == RT_MS_QUADLIT;
}
/* which (integrator, traversal) has a pair-cast instantiation (k_mega's PAIR branch, trace_pair): what a DScene::pair_cast
 * scene runs unless RTR_FLAG_SPLIT_CASTS asks for the split casts */
constexpr bool mega_pairable(int integ, int trav) { return integ == RTR_INTEGRATOR_MIS && trav == RT_TRAV_FLAT; }
/* parked words of the sorted variant (the pixel sum lives in the partial-sum buffer itself) + the exchange slot */
enum { SK_THR = 0, SK_L = 3, SK_PDF = 6, SK_NCLOSEST = 7, SK_NSHADOW = 8, SK_CONTRIB = 9, SK_SWI = 12, SK_STMAX = 15, SK_X = 16,
       SK_WORDS = 26 };
enum { SX_P = 0, SX_N = 3, SX_RD = 6, SX_PACK = 9 }; /* slot words: hit point, normal, direction (in: incoming, out: next), packed */
RT_DEV int material_class(int type) { /* what shades alike */
    return type == RTR_MAT_LAMBERTIAN ? 0 : (type == RTR_MAT_PBR ? 1 : ((type == RTR_MAT_DIELECTRIC || type == RTR_MAT_METAL) ? 2 : 3));
}

/* the sum a pixel's samples are added to: 0, or for an accumulator pass what the accumulator holds (RenderK::acc_in) */
template <int ACC>
RT_DEV V3 acc_start(const RenderK& P, int slot) {
    if (!ACC) return mk(0, 0, 0);
    const double* a = P.acc_in + (size_t)slot * 3 * RTR_BLOCK + threadIdx.x;
    return mk(a[0], a[RTR_BLOCK], a[2 * RTR_BLOCK]);
}

/* cycles per phase of the lockstep loops, summed per wave into RenderK::stats[3..6] (builds with -DRTR_PHASE_CLOCKS) */
#ifdef RTR_PHASE_CLOCKS
struct PhaseClocks {
    long long closest = 0, shade = 0, shadow = 0, other = 0, t = wall_clock64();
    RT_DEV void flush(const RenderK& P) const {
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&P.stats[3], (unsigned long long)closest);
            atomicAdd(&P.stats[4], (unsigned long long)shade);
            atomicAdd(&P.stats[5], (unsigned long long)shadow);
            atomicAdd(&P.stats[6], (unsigned long long)other);
        }
    }
};
#define RTR_CLK(phase) do { const long long now_ = wall_clock64(); clk.phase += now_ - clk.t; clk.t = now_; } while (0)
#else
struct PhaseClocks {
    RT_DEV void flush(const RenderK&) const {}
};
#define RTR_CLK(phase) do { } while (0)
#endif

/* rtr_cancel() in the lockstep loops: the wave polls the cancel word once every RT_POLL_EVERY loop iterations, every
 * lane in the same iteration (one request for the wave), and reads it before it looks at it: the pair loop issues the
 * load when the iteration's pair cast is over and takes it after shading, so nobody waits for the round trip (the split
 * loop issues it after its shadow cast: no register of the poll lives across a cast).  `it` counts the wave's
 * iterations.  A set word stops every lane of the wave within RT_POLL_EVERY iterations of its arrival: an
 * iteration is one bounce and a sample has at least one, so that is never later than the 8 samples of the slowest
 * lane that a per-lane poll keyed on the sample index allowed, and a render cancelled before its launch stops in its
 * first iteration.  A lane that stops in mid-sample has s < s_end: its workgroup counts as interrupted and the tile
 * stays untouched, as before.  The word is 0 where no poll was made, and render ids start at 1. */
#define RT_POLL_EVERY 8
RT_DEV uint32_t cancel_poll_issue(const RenderK& P, uint32_t it) {
    uint32_t word = 0;
    if ((it & (RT_POLL_EVERY - 1)) == 0) word = __hip_atomic_load(P.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return word;
}
RT_DEV bool cancel_poll_take(const RenderK& P, uint32_t word) { return word >= P.render_id; }

/* renderer.h:73-75 under the per-sample seed: the camera ray of sample s of the lane's pixel and the parked words of a
 * new path.  K_* : the variant's parked words (PK_* / SK_*); K_L < 0: the loop clears the radiance word itself (the
 * pair cast, step (3)); K_PIX >= 0: the word that holds the lane's pixel (PK_PIXEL), else it is worked out again */
template <int K_THR, int K_L, int K_PDF, int K_PIX = -1, bool JOIN = false>
RT_DEV void begin_sample(const DScene& sc, const RenderK& P, const Park& pk, int slot, int s, uint32_t& rng, PathState& ps) {
    int pi, pj;
    if (K_PIX >= 0) {
        uint32_t ui, uj;
        pk.get2(K_PIX, ui, uj);
        pi = (int)ui, pj = (int)uj;
    } else {
        bool in_region;
        tile_pixel(P, slot, threadIdx.x, pi, pj, in_region); /* recomputed: not worth two live registers */
    }
    camera_sample<JOIN>(sc, P, pi, pj, s, rng, ps.ro, ps.rd, ps.tm);
    ps.depth = 0, ps.specular_bounce = false;
    pk.set3(K_THR, mk(1.0, 1.0, 1.0));
    if (K_L >= 0) pk.set3(K_L, mk(0.0, 0.0, 0.0));
    pk.set(K_PDF, 0.0);
}

/* ACC: 0 = a one-shot render; 1 = an accumulator pass (rtr_accum_*) -- a kernel of its own, so that the registers of
 * the one-shot kernels do not pay for its pointers: workgroup b renders the active tile slot RenderK::active[b] from
 * its sample count RenderK::tile_s0 to RenderK::tile_s1 with the sums RenderK::acc_in; 2 = a pass of an accumulator
 * with moments, which also continues Q = sum of y_s * y_s (y_s = luminance of sample s) in a register, in sample
 * order, and leaves it in RenderK::q_part */
template <int INTEG, int TRAV, int MS, bool SORT = false, int ACC = 0, bool PAIR = false>
__global__ void __launch_bounds__(RTR_BLOCK, mega_waves(INTEG, TRAV, MS))
    k_mega(const DScene* __restrict__ scp, const RenderK P, const int stack_words) {
    static_assert(!SORT || mega_sortable(INTEG, TRAV, MS), "no sorted variant of this kernel");
    static_assert(!PAIR || (mega_pairable(INTEG, TRAV) && !SORT), "no pair-cast variant of this kernel");
    extern __shared__ int lds_stack[];
    const DScene& sc = *scp;
    const Stack st{lds_stack + threadIdx.x};
    const Park pk{reinterpret_cast<double*>(lds_stack + stack_words * RTR_BLOCK) + threadIdx.x};
#ifdef RTR_REGION_PROFILE
    if (threadIdx.x < 4 * 2 * RT_PROF_REGIONS + 8) rt_prof_lds[threadIdx.x] = 0;
    if (threadIdx.x + 256 < 4 * 2 * RT_PROF_REGIONS + 8) rt_prof_lds[threadIdx.x + 256] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) rt_prof_lds[4 * 2 * RT_PROF_REGIONS + (threadIdx.x >> 6) * 2] = __builtin_readcyclecounter();
#endif
    int slot, chunk;
    if (ACC) { /* the launch covers every owned tile; the active ones come first, most pending samples first */
        if ((int)blockIdx.x >= *P.n_active) return; /* workgroup-uniform */
        slot = P.active[blockIdx.x], chunk = 0;
    } else {
        mega_work(P, blockIdx.x, slot, chunk);
    }
    const int cell = slot * P.chunks + chunk; /* partial sum / completion word of this (tile, chunk) */
    int i, j;
    bool active;
    tile_pixel(P, slot, threadIdx.x, i, j, active);
    /* samples [s, s_end) of this pixel belong to this chunk */
    int s, s_end_;
    if (ACC) /* the tile's earlier samples are in P.acc_in */
        s = P.tile_s0[slot], s_end_ = P.tile_s1[slot];
    else
        chunk_range(P, chunk, s, s_end_);
    const int s_end = s_end_;
    if (!SORT) pk.set3(PK_ACC, acc_start<ACC>(P, slot));
    double q = ACC == 2 ? P.q_in[(size_t)slot * RTR_BLOCK + threadIdx.x] : 0.0; /* (dead unless ACC == 2) */
    PathCounters cnt;
    cnt.closest = 0, cnt.shadow = 0;
    uint32_t n_samples = 0;
    PathState ps;
    uint32_t rng = 1;
    bool fresh = true;
    bool done = !active || s >= s_end;
    if (SORT) {
        /* the class counters live in the traversal-stack words, which a flat scan never touches: one static word more
         * would round the workgroup's LDS up to the next 512 bytes and cost the third workgroup per CU */
        int* const s_cnt = lds_stack;
        const double* const xin = pk.base - threadIdx.x + SK_X * RTR_BLOCK; /* slot q, word k: xin[k * RTR_BLOCK + q] */
        double* const xw = const_cast<double*>(xin);
        double* const accp = P.partial + (size_t)cell * 3 * RTR_BLOCK + threadIdx.x; /* this lane's pixel sum */
        {
            const V3 a0 = acc_start<ACC>(P, slot);
            accp[0] = a0.x, accp[RTR_BLOCK] = a0.y, accp[2 * RTR_BLOCK] = a0.z;
        }
        if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
        pk.set(SK_NCLOSEST, 0.0);
        pk.set(SK_NSHADOW, 0.0);
        if (!done) begin_sample<SK_THR, SK_L, SK_PDF, -1, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
        __syncthreads();
        for (;;) {
            bool pending = false, ended = false, shade_me = false;
            int cls = 0, ticket = 0;
            Hit rec;
            rec.u = 0, rec.v = 0, rec.mat = 0, rec.front = false;
            RT_REGION(RG_OTHER);
            if (!done) {
                pk.set(SK_NCLOSEST, pk.get(SK_NCLOSEST) + 1.0);
                const bool hit_any = cast_closest<TRAV, false>(sc, ps.ro, ps.rd, ps.tm, rec, rng, st);
                if (!hit_any) {
                    RT_REGION(RG_MISS);
                    pk.set3(SK_L, add(pk.get3(SK_L), miss_radiance<INTEG, MS>(sc, pk.get3(SK_THR), ps.ro, ps.rd, ps.depth,
                                                                          ps.specular_bounce, pk.get(SK_PDF))));
                    ended = true;
                } else { /* the emission term of mis_path_integrator.h:72-94 needs the ray that hit: it stays with the owner */
                    ps.thr = pk.get3(SK_THR);
                    ps.L = mk(0.0, 0.0, 0.0);
                    ps.prev_bsdf_pdf = pk.get(SK_PDF);
                    const MatCtx mc = mat_prepare<MS>(sc, rec);
                    ShadowReq none;
                    shade_a_mis<MS, INTEG, 1>(sc, ps, rec, mc, mk(0, 0, 0), rng, none);
                    if (ps.L.x != 0.0 || ps.L.y != 0.0 || ps.L.z != 0.0) pk.set3(SK_L, add(pk.get3(SK_L), ps.L));
                    shade_me = true;
                    cls = material_class(mc.type);
                }
            }
            /* tickets: one LDS atomic per wave and class, ranks inside the wave by counting lanes below */
            RT_REGION(RG_EXCHANGE);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long m = __ballot(shade_me && cls == k);
                if (m) { /* wave-uniform */
                    int base = 0;
                    if ((int)__lane_id() == __builtin_ctzll(m)) base = atomicAdd(&s_cnt[k], __builtin_popcountll(m));
                    base = __shfl(base, __builtin_ctzll(m), 64);
                    if (shade_me && cls == k) ticket = base + (int)__builtin_popcountll(m & ((1ull << __lane_id()) - 1ull));
                }
            }
            RT_REGION(RG_BARRIER);
            if (!__syncthreads_or(!done)) break; /* barrier 1: every ticket is taken; nothing left to do = leave together */
            RT_REGION(RG_EXCHANGE);
            const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], c3 = s_cnt[3];
            int b0 = 0, b1 = (c0 + 63) & ~63, b2 = b1 + ((c1 + 63) & ~63), b3 = b2 + ((c2 + 63) & ~63);
            if (b3 + c3 > RTR_BLOCK) b1 = c0, b2 = c0 + c1, b3 = c0 + c1 + c2; /* no room for wave-aligned classes: packed */
            const int pos = (cls == 0 ? b0 : (cls == 1 ? b1 : (cls == 2 ? b2 : b3))) + ticket;
            if (shade_me) {
                xw[(SX_P + 0) * RTR_BLOCK + pos] = rec.p.x, xw[(SX_P + 1) * RTR_BLOCK + pos] = rec.p.y, xw[(SX_P + 2) * RTR_BLOCK + pos] = rec.p.z;
                xw[(SX_N + 0) * RTR_BLOCK + pos] = rec.n.x, xw[(SX_N + 1) * RTR_BLOCK + pos] = rec.n.y, xw[(SX_N + 2) * RTR_BLOCK + pos] = rec.n.z;
                xw[(SX_RD + 0) * RTR_BLOCK + pos] = ps.rd.x, xw[(SX_RD + 1) * RTR_BLOCK + pos] = ps.rd.y, xw[(SX_RD + 2) * RTR_BLOCK + pos] = ps.rd.z;
                const unsigned long long pack = (unsigned long long)rng | ((unsigned long long)(rec.mat & 0xffff) << 32) |
                                                ((unsigned long long)threadIdx.x << 48) | ((unsigned long long)(rec.front ? 1 : 0) << 56) |
                                                ((unsigned long long)(ps.depth >= P.rr_start ? 1 : 0) << 57);
                xw[SX_PACK * RTR_BLOCK + pos] = __longlong_as_double((long long)pack);
            }
            RT_REGION(RG_BARRIER);
            __syncthreads(); /* barrier 2: the slots are filled */
            RT_REGION(RG_EXCHANGE);
            if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0; /* everyone has read the totals; the next tickets come after barrier 3 */
            {
                const int q = threadIdx.x;
                const bool mine = (q >= b0 && q < b0 + c0) || (q >= b1 && q < b1 + c1) || (q >= b2 && q < b2 + c2) || (q >= b3 && q < b3 + c3);
                if (mine) { /* shade slot q: mis_path_integrator.h:96-146 */
                    const unsigned long long pack = (unsigned long long)__double_as_longlong(xin[SX_PACK * RTR_BLOCK + q]);
                    Hit h;
                    h.u = 0, h.v = 0, h.t = 0;
                    h.p = mk(xin[(SX_P + 0) * RTR_BLOCK + q], xin[(SX_P + 1) * RTR_BLOCK + q], xin[(SX_P + 2) * RTR_BLOCK + q]);
                    h.n = mk(xin[(SX_N + 0) * RTR_BLOCK + q], xin[(SX_N + 1) * RTR_BLOCK + q], xin[(SX_N + 2) * RTR_BLOCK + q]);
                    h.mat = (int)((pack >> 32) & 0xffff);
                    h.front = ((pack >> 56) & 1) != 0;
                    const int owner = (int)((pack >> 48) & 0xff);
                    const Park po{pk.base - threadIdx.x + owner}; /* the owner's parked words */
                    PathState sh;
                    sh.rd = mk(xin[(SX_RD + 0) * RTR_BLOCK + q], xin[(SX_RD + 1) * RTR_BLOCK + q], xin[(SX_RD + 2) * RTR_BLOCK + q]);
                    sh.ro = h.p, sh.tm = 0;
                    sh.thr = po.get3(SK_THR);
                    sh.L = mk(0.0, 0.0, 0.0);
                    sh.prev_bsdf_pdf = 0.0;
                    sh.depth = ((pack >> 57) & 1) ? P.rr_start : P.rr_start - 1; /* only `depth >= rr_start` is read */
                    sh.specular_bounce = false;
                    uint32_t r2 = (uint32_t)pack;
                    const V3 wo = neg(unit(sh.rd));
                    ShadowReq rq;
                    const MatCtx mc = mat_prepare<MS>(sc, h);
                    shade_a_mis<MS, INTEG, 2>(sc, sh, h, mc, wo, r2, rq);
                    if (rq.valid) {
                        po.set3(SK_SWI, rq.wi);
                        po.set(SK_STMAX, rq.tmax);
                        po.set3(SK_CONTRIB, rq.contrib);
                    }
                    const bool go = shade_b_mis<MS, INTEG>(sc, sh, h, mc, wo, r2, P.rr_start);
                    po.set3(SK_THR, sh.thr);
                    po.set(SK_PDF, sh.prev_bsdf_pdf);
                    xw[(SX_RD + 0) * RTR_BLOCK + q] = sh.rd.x, xw[(SX_RD + 1) * RTR_BLOCK + q] = sh.rd.y, xw[(SX_RD + 2) * RTR_BLOCK + q] = sh.rd.z;
                    const unsigned long long back = (unsigned long long)r2 | ((unsigned long long)(go ? 1 : 0) << 32) |
                                                    ((unsigned long long)(sh.specular_bounce ? 1 : 0) << 33) |
                                                    ((unsigned long long)(rq.valid ? 1 : 0) << 34);
                    xw[SX_PACK * RTR_BLOCK + q] = __longlong_as_double((long long)back);
                }
            }
            RT_REGION(RG_BARRIER);
            __syncthreads(); /* barrier 3: results are back */
            RT_REGION(RG_PARK);
            if (shade_me) {
                const unsigned long long back = (unsigned long long)__double_as_longlong(xin[SX_PACK * RTR_BLOCK + pos]);
                rng = (uint32_t)back;
                ps.ro = mk(xin[(SX_P + 0) * RTR_BLOCK + pos], xin[(SX_P + 1) * RTR_BLOCK + pos], xin[(SX_P + 2) * RTR_BLOCK + pos]);
                ps.rd = mk(xin[(SX_RD + 0) * RTR_BLOCK + pos], xin[(SX_RD + 1) * RTR_BLOCK + pos], xin[(SX_RD + 2) * RTR_BLOCK + pos]);
                ps.specular_bounce = ((back >> 33) & 1) != 0;
                pending = ((back >> 34) & 1) != 0;
                const bool go = ((back >> 32) & 1) != 0;
                ended = !go || ++ps.depth >= P.max_depth;
            }
            RT_REGION(RG_OTHER);
            if (pending) { /* mis_path_integrator.h:210-213, origin = the hit point = ps.ro */
                pk.set(SK_NSHADOW, pk.get(SK_NSHADOW) + 1.0);
                if (!cast_shadow<TRAV>(sc, ps.ro, pk.get3(SK_SWI), pk.get(SK_STMAX), rng, st))
                    pk.set3(SK_L, add(pk.get3(SK_L), pk.get3(SK_CONTRIB)));
            }
            RT_REGION(RG_REGEN);
            if (ended) {
                const V3 L = pk.get3(SK_L);
                accp[0] += L.x, accp[RTR_BLOCK] += L.y, accp[2 * RTR_BLOCK] += L.z; /* renderer.h:77-78 */
                if (ACC == 2) {
                    const double y = luminance(L);
                    q += y * y;
                }
                ++n_samples;
                ++s;
                done = s >= s_end || ((s & 7) == 0 && render_cancelled(P));
                if (!done) begin_sample<SK_THR, SK_L, SK_PDF, -1, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
            }
        }
        cnt.closest = (uint32_t)pk.get(SK_NCLOSEST);
        cnt.shadow = (uint32_t)pk.get(SK_NSHADOW);
    } else if (TRAV == RT_TRAV_MEDIA) {
        /* media draw random numbers inside both ray casts: keep the reference's statement order */
        V3 acc = acc_start<ACC>(P, slot);
        while (!done) {
            if (fresh) { /* renderer.h:73-75 under the per-sample seed */
                if ((s & 7) == 0 && render_cancelled(P)) break;
                V3 ro, rd;
                Real tm;
                camera_sample<RT_DRAW_MS(MS)>(sc, P, i, j, s, rng, ro, rd, tm);
                path_begin(ps, ro, rd, tm);
                fresh = false;
            }
            if (!bounce<INTEG, TRAV>(sc, ps, rng, st, P.max_depth, P.rr_start, cnt)) {
                acc = add(acc, ps.L); /* renderer.h:77-78 */
                if (ACC == 2) {
                    const double y = luminance(ps.L);
                    q += y * y;
                }
                ++n_samples;
                ++s;
                fresh = true;
                done = s >= s_end;
            }
        }
        pk.set3(PK_ACC, acc);
    } else if (PAIR) {
        /* The MIS kernel of a DScene::pair_cast scene: the shadow ray of bounce k and the closest-hit ray of bounce k + 1
         * are both known once the BSDF sample of bounce k is drawn, and neither cast draws a random number (no media), so
         * one trace_pair per iteration casts both.  An iteration: (1) the pair cast of the parked shadow request (B) and
         * the lane's ray (A); (2) the light sample of B reaches L; (3) a sample that ended in the previous iteration --
         * its L complete now -- is added to the pixel sum; (4) A's hit is shaded (emission, light sample, BSDF sample) or
         * its miss term added; (5) the new shadow request is parked; (6) an ended sample's lane starts the next one.  The
         * terms reach L in the reference's order (the light sample of bounce k, then the emission or miss term of bounce
         * k + 1), samples reach the pixel sum in sample order, and a lane whose sample ended keeps that sample's L in
         * PK_L, and the origin of its shadow ray in `so`, while it casts the new sample's camera ray. */
        pk.set2(PK_NCAST, 0u, 0u);
        pk.set2(PK_PIXEL, (uint32_t)i, (uint32_t)j);
        pk.set3(PK_L, mk(0.0, 0.0, 0.0));
        if (!done) begin_sample<PK_THR, -1, PK_PDF, PK_PIXEL, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
        uint32_t it = 0; /* iterations of the wave: wave-uniform */
        bool pending = false; /* a shadow request is parked: PK_SWI, PK_STMAX, PK_CONTRIB, origin `so` */
        bool settle = false;  /* the sample in PK_L has ended: add it to the pixel sum once its shadow ray is resolved */
        V3 so = mk(0.0, 0.0, 0.0);
        PhaseClocks clk; /* closest = the pair casts, shadow = resolving them + settling ended samples */
        while (!done || settle) {
            RTR_CLK(other);
            RT_REGION(RG_OTHER);
            const bool cast_a = !done;
            Real a_tmax = RT_INF, b_tmax = 0.0;
            int a_ref, a_inst, b_ref;
            V3 swi = mk(1.0, 1.0, 1.0);
            RT_REGION(RG_COUNT);
            { /* both counters in one pass over their word, every lane alike (the wave-scalar form miscounts) */
                uint32_t n_closest, n_shadow;
                pk.get2(PK_NCAST, n_closest, n_shadow);
                pk.set2(PK_NCAST, n_closest + (cast_a ? 1u : 0u), n_shadow + (pending ? 1u : 0u));
            }
            RT_REGION(RG_OTHER);
            if (!cast_a) { /* (the lane's path state is dead: the dummy ray in place, no copies live across the cast) */
                ps.ro = mk(0.0, 0.0, 0.0), ps.rd = mk(1.0, 1.0, 1.0), ps.tm = 0.0;
                a_tmax = 0.0;
            }
            if (pending) {
                swi = pk.get3(PK_SWI);
                b_tmax = pk.get(PK_STMAX);
            } else {
                so = mk(0.0, 0.0, 0.0);
            }
            if (!trace_pair<pair_recasts(MS), pair_runs_routine(MS)>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, so, swi, b_tmax, b_ref, st)) {
                /* a vote failed (cold): the two single casts, both t_max from where they came (a request that is not
                 * pending is the dummy already: nothing stale to replace) */
                a_tmax = cast_a ? RT_INF : 0.0;
                b_tmax = pending ? pk.get(PK_STMAX) : 0.0;
                pair_recast(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, so, swi, b_tmax, b_ref, st);
            }
            RTR_CLK(closest);
            RT_REGION(RG_POLL);
            const uint32_t cancel_word = cancel_poll_issue(P, it++);
            RT_REGION(RG_SETTLE);
            /* steps (2) and (3) in one pass over PK_L: the light sample of B, then the ended sample into the pixel sum */
            const bool lit = pending && b_ref < 0;
            if (lit || settle) {
                V3 L = pk.get3(PK_L);
                if (lit) L = add(L, pk.get3(PK_CONTRIB)); /* mis_path_integrator.h:210-213 */
                if (settle) {
                    pk.set3(PK_ACC, add(pk.get3(PK_ACC), L)); /* renderer.h:77-78 */
                    if (ACC == 2) {
                        const double y = luminance(L);
                        q += y * y;
                    }
                    L = mk(0.0, 0.0, 0.0);
                    settle = false;
                }
                pk.set3(PK_L, L);
            }
            pending = false;
            RTR_CLK(shadow);
            if (cast_a) {
                bool ended;
                if (a_ref < 0) {
                    RT_REGION(RG_MISS);
                    pk.set3(PK_L, add(pk.get3(PK_L), miss_radiance<INTEG, MS>(sc, pk.get3(PK_THR), ps.ro, ps.rd, ps.depth,
                                                                          ps.specular_bounce, pk.get(PK_PDF))));
                    ended = true;
                } else {
                    Hit rec;
                    rec.u = 0, rec.v = 0;
                    if (MS == RT_MS_FULL && sc.needs_uv) /* (cast_closest's hit record) */
                        fast_finish<true, true>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, rec);
                    else
                        fast_finish<false, true>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, rec);
                    ps.thr = pk.get3(PK_THR);
                    ps.L = mk(0.0, 0.0, 0.0); /* see the split loop below: L + e is the reference's L += e */
                    ps.prev_bsdf_pdf = pk.get(PK_PDF);
                    const V3 wo = neg(unit(ps.rd));
                    ParkedReq rq{false, pk}; /* parked until the next pair cast */
                    const MatCtx mc = mat_prepare<MS>(sc, rec);
                    shade_a_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, rq);
                    pending = rq.valid;
                    const bool go = shade_b_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, P.rr_start);
                    RT_REGION(RG_PARK);
                    ps.ro = rec.p; /* next ray origin and shadow ray origin */
                    so = rec.p;
                    pk.set3(PK_THR, ps.thr);
                    if (ps.L.x != 0.0 || ps.L.y != 0.0 || ps.L.z != 0.0) pk.set3(PK_L, add(pk.get3(PK_L), ps.L));
                    pk.set(PK_PDF, ps.prev_bsdf_pdf);
                    ended = !go || ++ps.depth >= P.max_depth;
                }
                RTR_CLK(shade);
                RT_REGION(RG_REGEN);
                if (ended) {
                    settle = true;
                    ++n_samples;
                    ++s;
                    done = s >= s_end;
                    RT_REGION(RG_BEGIN);
                    if (!done) begin_sample<PK_THR, -1, PK_PDF, PK_PIXEL, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
                }
            }
            RT_REGION(RG_POLL);
            if (cancel_poll_take(P, cancel_word)) done = true; /* (an ended sample still settles: the loop's condition) */
        }
        pk.get2(PK_NCAST, cnt.closest, cnt.shadow);
        clk.flush(P);
    } else {
        /* Without media the shadow ray draws nothing, so it can be cast AFTER the BSDF sample of
         * the same bounce, when the hit record is dead.  Every live lane runs the same phases in
         * every iteration (closest hit, shade, shadow ray, end-of-sample + regeneration), so a wave
         * stays in lockstep although path lengths differ; the sums still see their terms in the
         * reference's order (emission, then the light sample of the same bounce). */
        /* cast counters live in LDS as well */
        pk.set2(PK_NCAST, 0u, 0u);
        pk.set2(PK_PIXEL, (uint32_t)i, (uint32_t)j);
        if (!done) begin_sample<PK_THR, PK_L, PK_PDF, PK_PIXEL, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
        PhaseClocks clk;
        uint32_t it = 0; /* iterations of the wave: wave-uniform */
        while (!done) {
            bool pending = false, ended = false;
            bool shadowed = false; /* a shadow ray was cast inside the shading (program traversals) */
            RTR_CLK(other);
            RT_REGION(RG_OTHER);
            {
                Hit rec;
                rec.u = 0, rec.v = 0;
                const bool hit_any = cast_closest<TRAV, MS == RT_MS_FULL>(sc, ps.ro, ps.rd, ps.tm, rec, rng, st);
                RTR_CLK(closest);
                if (!hit_any) {
                    RT_REGION(RG_MISS);
                    pk.set3(PK_L, add(pk.get3(PK_L), miss_radiance<INTEG, MS>(sc, pk.get3(PK_THR), ps.ro, ps.rd, ps.depth,
                                                                          ps.specular_bounce, pk.get(PK_PDF))));
                    ended = true;
                } else {
                    ps.thr = pk.get3(PK_THR);
                    /* shading adds at most ONE term (the emission) to L before the light sample is
                     * resolved, so it can start from zero and be added to the parked sum afterwards:
                     * L + e is the same rounding as the reference's L += e */
                    ps.L = mk(0.0, 0.0, 0.0);
                    ps.prev_bsdf_pdf = pk.get(PK_PDF);
                    bool go;
                    if (INTEG == RTR_INTEGRATOR_RR) {
                        go = shade_rr<MS>(sc, ps, rec, rng, P.rr_start);
                    } else if (INTEG == RTR_INTEGRATOR_PATH) {
                        go = shade_path<MS>(sc, ps, rec, rng);
                    } else {
                        const V3 wo = neg(unit(ps.rd));
                        ShadowReq rq;
                        MatCtx mc = mat_prepare<MS>(sc, rec);
                        shade_a_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, rq);
                        if (rt_is_program(TRAV)) {
                            /* media draw inside the shadow cast: it keeps its place between the light
                             * sample and the BSDF sample (mis_path_integrator.h:96-106) */
                            if (ps.L.x != 0.0 || ps.L.y != 0.0 || ps.L.z != 0.0) {
                                pk.set3(PK_L, add(pk.get3(PK_L), ps.L));
                                ps.L = mk(0.0, 0.0, 0.0);
                            }
                            if (rq.valid) {
                                shadowed = true;
                                if (!cast_shadow<TRAV>(sc, rec.p, rq.wi, rq.tmax, rng, st))
                                    pk.set3(PK_L, add(pk.get3(PK_L), rq.contrib));
                                mc = mat_prepare<MS>(sc, rec); /* cheaper than keeping it in registers across the cast */
                            }
                        } else if (rq.valid) { /* parked until the shadow ray is cast */
                            pending = true;
                            pk.set3(PK_SWI, rq.wi);
                            pk.set(PK_STMAX, rq.tmax);
                            pk.set3(PK_CONTRIB, rq.contrib);
                        }
                        go = shade_b_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, P.rr_start);
                    }
                    RT_REGION(RG_PARK);
                    ps.ro = rec.p; /* next ray origin and shadow ray origin */
                    pk.set3(PK_THR, ps.thr);
                    if (ps.L.x != 0.0 || ps.L.y != 0.0 || ps.L.z != 0.0) pk.set3(PK_L, add(pk.get3(PK_L), ps.L));
                    pk.set(PK_PDF, ps.prev_bsdf_pdf);
                    ended = !go || ++ps.depth >= P.max_depth;
                }
            }
            RTR_CLK(shade);
            RT_REGION(RG_OTHER);
            if (pending) { /* mis_path_integrator.h:210-213, origin = the hit point = ps.ro */
                if (!cast_shadow<TRAV>(sc, ps.ro, pk.get3(PK_SWI), pk.get(PK_STMAX), rng, st))
                    pk.set3(PK_L, add(pk.get3(PK_L), pk.get3(PK_CONTRIB)));
            }
            RTR_CLK(shadow);
            RT_REGION(RG_POLL);
            const uint32_t cancel_word = cancel_poll_issue(P, it++); /* (no register of it lives across a cast) */
            RT_REGION(RG_REGEN);
            if (ended) {
                pk.set3(PK_ACC, add(pk.get3(PK_ACC), pk.get3(PK_L))); /* renderer.h:77-78 */
                if (ACC == 2) {
                    const double y = luminance(pk.get3(PK_L));
                    q += y * y;
                }
                ++n_samples;
                ++s;
                done = s >= s_end;
                RT_REGION(RG_BEGIN);
                if (!done) begin_sample<PK_THR, PK_L, PK_PDF, PK_PIXEL, RT_DRAW_MS(MS)>(sc, P, pk, slot, s, rng, ps);
            }
            RT_REGION(RG_COUNT);
            { /* one closest-hit cast per iteration of a live lane, and its shadow ray if it cast one */
                uint32_t n_closest, n_shadow;
                pk.get2(PK_NCAST, n_closest, n_shadow);
                pk.set2(PK_NCAST, n_closest + 1u, n_shadow + ((pending || shadowed) ? 1u : 0u));
            }
            RT_REGION(RG_POLL);
            if (cancel_poll_take(P, cancel_word)) done = true; /* rtr_cancel(): cancel_poll_issue */
        }
        pk.get2(PK_NCAST, cnt.closest, cnt.shadow);
        clk.flush(P);
    }
#ifdef RTR_REGION_PROFILE
    RT_REGION(RG_OTHER);
    __syncthreads();
    if (threadIdx.x < 2 * RT_PROF_REGIONS) {
        unsigned long long v = 0;
        for (int w = 0; w < 4; ++w) v += rt_prof_lds[w * 2 * RT_PROF_REGIONS + threadIdx.x];
        if (v) atomicAdd(&P.stats[RT_PROF_BASE + threadIdx.x], v);
    }
#endif
    if (!SORT) { /* (the sorted variant summed into the buffer itself) */
        const V3 acc = pk.get3(PK_ACC);
        double* out = P.partial + (size_t)cell * 3 * RTR_BLOCK + threadIdx.x;
        out[0] = acc.x;
        out[RTR_BLOCK] = acc.y;
        out[2 * RTR_BLOCK] = acc.z;
    }
    if (ACC == 2) P.q_part[(size_t)cell * RTR_BLOCK + threadIdx.x] = q;
    unsigned long long a = wave_sum(n_samples), b = wave_sum(cnt.closest), c = wave_sum(cnt.shadow);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&P.stats[0], a);
        atomicAdd(&P.stats[1], b);
        atomicAdd(&P.stats[2], c);
    }
    /* a cancelled render leaves unfinished tiles untouched, like the reference's workers
     * (renderer.h:52-59): k_resolve stores a tile only when all its chunks ran to the end */
    const int interrupted = __syncthreads_or(active && s < s_end);
    if (threadIdx.x == 0) {
        P.done[cell] = !interrupted;
        if (interrupted) atomicAdd(&P.stats[7], 1ull);
    }
}


/* ---- k_mega_queue: the pair-cast loop of k_mega<..., ACC = 0, PAIR = true> over a launch-wide job queue ----------------
 * k_mega's pair loop runs until the slowest of a wave's 64 pixels has finished its chunk of samples; the other lanes cast
 * dummy rays meanwhile (a quarter more iterations than rays on the headline).  Here the launch is a persistent grid, and
 * a lane whose job -- one pixel of one (tile, chunk) cell, rt_render.h: queue_block -- is over takes the next one: of
 * the wave's current block, or of the block the wave fetches with ONE atomic add on the launch-wide counter `q_counter`
 * (block ids >= n_blocks: the queue has run out, and the wave never asks again).  No spin loop, no barrier: the four
 * waves of a workgroup never meet after they have started, and no wave waits for another.
 *
 * No sum changes.  A job has the cell, the sample range and the sample order of the static kernel, one lane sums it
 * from start to end in PK_ACC and stores it where the static kernel stores it, so the image is that kernel's bit for
 * bit in every chunk mode; only which lane of which wave computes a cell differs.
 *
 * Job switch, with the loop's own states: (1) the job's last sample ends: the lane is `done` and stops casting ray A;
 * (2) in the next iteration the sample settles into PK_ACC; (3) later in that iteration the lane stores PK_ACC to its
 * cell and adds 1 to the cell's completion word RenderK::done (k_resolve takes a cell whose word is RTR_BLOCK), clears
 * PK_ACC, takes the next job and begins its first sample: one idle iteration per job.  A pixel outside the region, or
 * an empty sample range, is a null job: it counts as finished when it is taken.  A lane that finds no job is done for
 * good, and the loop ends as k_mega's does.
 *
 * State: the pixel (16 bits each) and the job's s_end share PK_PIXEL (queue_pack), read at a sample's end, where the
 * camera ray needs the pixel anyway; the lane's cell lives in its traversal-stack word of LDS, which a flat scan never
 * touches (-1: no job); the wave's block, its cursor and its sample count are wave-uniform and live in an LDS slot of the
 * wave (QueueSlot), and the job switch reads the launch's arguments where it needs them (queue_args).  Nothing of the
 * queue is live across the pair cast.
 *
 * rtr_cancel(): the wave polls as k_mega does.  A wave that takes the cancel drops its jobs -- no lane of it stores or
 * counts again, so their cells stay incomplete and their tiles untouched -- and adds 1 to stats[7]: here that word
 * counts interrupted WAVES (inside the loop a wave always holds a job that is not stored yet). */
struct QueueWave {
    int block; /* the block the wave takes jobs from; -1: the queue has run out */
    int next;  /* jobs of it that are taken */
    unsigned long long samples; /* samples of the jobs the wave's lanes have taken (wave-uniform: a lane has no register
                                   to count its own in); a cancel takes back what its dropped jobs had left */
};
/* Nothing of the queue is live across the pair cast, where every scalar register that is held is one that the scans
 * spill (a spilled scalar is a v_writelane and every reload a v_readlane: vector instructions of a kernel the vector
 * pipe binds).  The wave's QueueWave lives in LDS, one slot per wave of the workgroup, and is read and written only by
 * the job switch and the cancel path.  Every lane that is there stores the same value and a lane reads after its own
 * store (a lane that has left the loop never comes back), so no lane depends on another's store; the accesses are
 * volatile so that none of them is kept in a register across an iteration. */
__shared__ int rt_queue_waves[(RTR_BLOCK / 64) * 4]; /* [wave]: block, next, samples lo, samples hi (k_mega_queue only) */
struct QueueSlot {
    /* (through an LDS pointer: a volatile access through a generic one stays a flat access with a 64-bit address) */
    RT_DEV static volatile __attribute__((address_space(3))) int& w(int k) {
        return ((volatile __attribute__((address_space(3))) int*)rt_queue_waves)[(threadIdx.x >> 6) * 4 + k];
    }
    RT_DEV static int uni(int v) { return __builtin_amdgcn_readfirstlane(v); } /* every lane read the same word */
    RT_DEV static QueueWave get() {
        QueueWave q;
        q.block = uni(w(0)), q.next = uni(w(1));
        q.samples = get_samples();
        return q;
    }
    RT_DEV static unsigned long long get_samples() {
        return (unsigned long long)(uint32_t)uni(w(2)) | ((unsigned long long)(uint32_t)uni(w(3)) << 32);
    }
    RT_DEV static void set_samples(unsigned long long n) { w(2) = (int)(uint32_t)n, w(3) = (int)(uint32_t)(n >> 32); }
    RT_DEV static void set(const QueueWave& q) {
        w(0) = q.block, w(1) = q.next;
        set_samples(q.samples);
    }
};
/* The image's divisors for camera_sample (CameraDiv), made in the prologue and kept the same way: (W - 1), its refined
 * reciprocal, (H - 1), its refined reciprocal.  Every lane of the workgroup stores the same four words before its first
 * sample and reads them back where a sample begins, so they cost no register across the cast and no division there. */
__shared__ double rt_queue_camera[4];
struct QueueCamera {
    RT_DEV static volatile __attribute__((address_space(3))) double& w(int k) {
        return ((volatile __attribute__((address_space(3))) double*)rt_queue_camera)[k];
    }
    RT_DEV static void set(const CameraDiv& c) { w(0) = c.w.d, w(1) = c.w.r, w(2) = c.h.d, w(3) = c.h.r; }
    RT_DEV static CameraDiv get(int W, int H) {
        CameraDiv c;
        c.w.d = w(0), c.w.r = w(1), c.h.d = w(2), c.h.r = w(3);
        c.w.safe = c.h.safe = (W != 1) & (H != 1);
        return c;
    }
};
/* The launch's arguments for the same two places, read from the kernel-argument segment where they are used: the
 * arguments a kernel names are loaded at its entry and would be held, or spilled, through every cast.  The layout is
 * k_mega_queue's parameter list, each argument at its natural alignment; the pointer passes through an empty asm so
 * that the loads stay behind it. */
struct QueueArgs {
    const DScene* scp;
    RenderK P;
    int stack_words;
    uint32_t* q_counter;
    int n_blocks;
};
RT_DEV QueueArgs queue_args() {
    unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return ld_const(reinterpret_cast<const QueueArgs*>(p), 0);
}
/* P for the camera sample inside the loop: W and H behind an empty asm, so that (W - 1) and (H - 1) are converted where a
 * sample begins (two instructions) and not carried as doubles through every cast, where the lean kernel spills them */
RT_DEV RenderK queue_image_size(const RenderK& P) {
    RenderK B = P;
    asm volatile("" : "+s"(B.W), "+s"(B.H));
    return B;
}
/* Lanes with `need` take consecutive jobs, by their rank among those lanes, until each has a job with samples or the
 * queue has run out; the wave-uniform loop fetches a block whenever the current one has none left.  true: the lane has a
 * job (PK_PIXEL and *my_cell are set, `s` is its first sample); a lane in need that gets none has *my_cell = -1. */
RT_DEV bool queue_take(const RenderK& P, uint32_t* __restrict__ q_counter, const int n_blocks, const QueueSlot slot, bool need,
                       const Park& pk, int* my_cell, int& s) {
    bool got = false;
    QueueWave qw = slot.get();
    unsigned long long m = __ballot(need);
    while (m) { /* wave-uniform */
        if (qw.block >= 0 && qw.next == RT_QUEUE_JOBS) {
            const int first = __builtin_ctzll(m);
            uint32_t b = 0;
            if ((int)__lane_id() == first) b = atomicAdd(q_counter, 1u);
            b = (uint32_t)__builtin_amdgcn_readlane((int)b, first);
            qw.block = b < (uint32_t)n_blocks ? (int)b : -1;
            qw.next = 0;
        }
        if (qw.block < 0) {
            if (need) *my_cell = -1;
            break;
        }
        const QueueBlock qb = queue_block(P, qw.block);
        const int tile = P.tile_ids[qb.slot];
        const int tile_y = (P.tiles_y - 1) - tile / P.tiles_x; /* tile_pixel */
        const int tile_x = tile % P.tiles_x;
        const int cell = qb.slot * P.chunks + qb.chunk;
        const int k = qw.next + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        bool now = false;
        if (need && k < RT_QUEUE_JOBS) {
            const int i = tile_x * 16 + (k & 15), j = tile_y * 16 + qb.quarter * 4 + (k >> 4);
            if (i >= P.x0 && i < P.x1 && j >= P.y0 && j < P.y1 && qb.s0 < qb.s1) {
                uint32_t lo, hi;
                queue_pack(i, j, qb.s1, lo, hi);
                pk.set2(PK_PIXEL, lo, hi);
                *my_cell = cell;
                s = qb.s0;
                got = now = true, need = false;
            } else {
                atomicAdd(&P.done[cell], 1); /* a null job */
            }
        }
        qw.samples += (unsigned long long)__builtin_popcountll(__ballot(now)) * (unsigned long long)(qb.s1 - qb.s0);
        const int taken = qw.next + (int)__builtin_popcountll(m);
        qw.next = taken < RT_QUEUE_JOBS ? taken : RT_QUEUE_JOBS;
        m = __ballot(need);
    }
    slot.set(qw);
    return got;
}

/* After a recast (pair_recast) of a kernel whose request B stays resident in PK_SWI / `so` while it is dead: the request is
 * dead after its cast, and gets the prologue's direction and a zero origin, which pass every vote */
RT_DEV void pair_retire(const Park& pk, V3& so) {
    pk.set3(PK_SWI, mk(1.0, 1.0, 1.0));
    so = mk(0.0, 0.0, 0.0);
}

template <int INTEG, int TRAV, int MS>
__global__ void __launch_bounds__(RTR_BLOCK, mega_waves(INTEG, TRAV, MS))
    k_mega_queue(const DScene* __restrict__ scp, const RenderK P, const int stack_words, uint32_t* __restrict__ /* q_counter */,
                 const int /* n_blocks */) { /* (the queue's own arguments: queue_args(), where they are used) */
    static_assert(mega_pairable(INTEG, TRAV), "no pair-cast variant of this kernel");
    extern __shared__ int lds_stack[];
    const DScene& sc = *scp;
    const Stack st{lds_stack + threadIdx.x};
    const Park pk{reinterpret_cast<double*>(lds_stack + stack_words * RTR_BLOCK) + threadIdx.x};
    int* const my_cell = lds_stack + threadIdx.x; /* the lane's cell, in its stack word */
    const QueueSlot slot; /* the wave's QueueWave, in LDS */
#ifdef RTR_REGION_PROFILE
    if (threadIdx.x < 4 * 2 * RT_PROF_REGIONS + 8) rt_prof_lds[threadIdx.x] = 0;
    if (threadIdx.x + 256 < 4 * 2 * RT_PROF_REGIONS + 8) rt_prof_lds[threadIdx.x + 256] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) rt_prof_lds[4 * 2 * RT_PROF_REGIONS + (threadIdx.x >> 6) * 2] = __builtin_readcyclecounter();
#endif
    PathCounters cnt;
    cnt.closest = 0, cnt.shadow = 0;
    PathState ps;
    uint32_t rng = 1;
    int s = 0;
    slot.set(QueueWave{0, RT_QUEUE_JOBS, 0ull});
    pk.set3(PK_ACC, mk(0.0, 0.0, 0.0));
    pk.set2(PK_NCAST, 0u, 0u);
    pk.set3(PK_L, mk(0.0, 0.0, 0.0));
    /* ray B's request is always in PK_SWI / PK_STMAX, dead (t_max = 0: no record accepts it) or parked by the shading */
    pk.set3(PK_SWI, mk(1.0, 1.0, 1.0));
    pk.set(PK_STMAX, 0.0);
    *my_cell = -1;
    QueueCamera::set(camera_div_make(P.W, P.H));
    bool done;
    {
        const QueueArgs Q = queue_args();
        done = !queue_take(Q.P, Q.q_counter, Q.n_blocks, slot, true, pk, my_cell, s);
    }
    if (!done) {
        uint32_t lo, hi;
        int i, j, s_end;
        pk.get2(PK_PIXEL, lo, hi);
        queue_unpack(lo, hi, i, j, s_end);
        camera_sample<RT_DRAW_MS(MS)>(sc, QueueCamera::get(P.W, P.H), P.seed, P.W, i, j, s, rng, ps.ro, ps.rd, ps.tm); /* begin_sample */
        ps.depth = 0, ps.specular_bounce = false;
        pk.set3(PK_THR, mk(1.0, 1.0, 1.0));
        pk.set(PK_PDF, 0.0);
    }
    uint32_t it = 0; /* iterations of the wave: wave-uniform */
    bool pending = false; /* k_mega's pair loop: a shadow request is parked */
    bool settle = false;  /* the sample in PK_L has ended */
    V3 so = mk(0.0, 0.0, 0.0);
    PhaseClocks clk;
    while (!done || settle) {
        RTR_CLK(other);
        RT_REGION(RG_OTHER);
        const bool cast_a = !done;
        Real a_tmax = RT_INF;
        int a_ref, a_inst, b_ref;
        RT_REGION(RG_COUNT);
        { /* (two ds_add_u32 with a 0 / 1 operand in its place save four instructions and no time: profiles/r17_loopstate.txt) */
            uint32_t n_closest, n_shadow;
            pk.get2(PK_NCAST, n_closest, n_shadow);
            pk.set2(PK_NCAST, n_closest + (cast_a ? 1u : 0u), n_shadow + (pending ? 1u : 0u));
        }
        RT_REGION(RG_OTHER);
        /* the dummy A of a lane that waits for its job switch is installed here and not where `done` becomes true: held
         * from there, its seven words would have to survive the other lanes' shading, which has no registers for them */
        if (!cast_a) {
            ps.ro = mk(0.0, 0.0, 0.0), ps.rd = mk(1.0, 1.0, 1.0), ps.tm = 0.0;
            a_tmax = 0.0;
        }
        /* B is what the parked words hold, read by every lane alike.  A dead request keeps the direction of the lane's
         * last one, and `so` its origin: with t_max = 0 no record of the fast or the plain scans accepts it (t_min is
         * 0.001), and a b_ref it did set would not count, because `lit` asks for `pending`.  A direction or origin that
         * failed rcp_safe or the origin verdict sent its cast to the recast below, which replaces it (pair_retire): what
         * stays resident has passed every vote once. */
        const V3 swi = pk.get3(PK_SWI);
        Real b_tmax = pk.get(PK_STMAX);
        if (!trace_pair<pair_recasts(MS), pair_runs_routine(MS)>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, so, swi, b_tmax, b_ref, st)) {
            /* a vote failed (cold): both rays again through the single casts, their t_max from where they came (the
             * request is not yet marked dead).  After this cast the resident request is dead in every lane, and takes
             * the prologue's direction and a zero origin: a stale direction or origin that failed its verdict would fail
             * it again in every later iteration and pin the wave to this block. */
            a_tmax = cast_a ? RT_INF : 0.0;
            b_tmax = pk.get(PK_STMAX);
            pair_recast(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, so, swi, b_tmax, b_ref, st);
            pair_retire(pk, so);
        }
        RTR_CLK(closest);
        RT_REGION(RG_POLL);
        const uint32_t cancel_word = cancel_poll_issue(P, it++);
        RT_REGION(RG_SETTLE);
        const bool lit = pending && b_ref < 0;
        if (lit || settle) {
            V3 L = pk.get3(PK_L);
            if (lit) L = add(L, pk.get3(PK_CONTRIB)); /* mis_path_integrator.h:210-213 */
            if (settle) {
                pk.set3(PK_ACC, add(pk.get3(PK_ACC), L)); /* renderer.h:77-78 */
                L = mk(0.0, 0.0, 0.0);
                settle = false;
            }
            pk.set3(PK_L, L);
        }
        pending = false;
        { /* the request is cast: the resident one is dead until the shading parks the next (the zero is made here: hoisted
           * out of the loop it is one more pair of registers that the lean kernel spills) */
            Real dead = 0.0;
            asm volatile("" : "+v"(dead));
            pk.set(PK_STMAX, dead);
        }
        RTR_CLK(shadow);
        bool begin = false; /* the lane starts sample s at the end of this iteration */
        if (cast_a) {
            bool ended;
            if (a_ref < 0) {
                RT_REGION(RG_MISS);
                pk.set3(PK_L, add(pk.get3(PK_L), miss_radiance<INTEG, MS>(sc, pk.get3(PK_THR), ps.ro, ps.rd, ps.depth,
                                                                      ps.specular_bounce, pk.get(PK_PDF))));
                ended = true;
            } else {
                Hit rec;
                rec.u = 0, rec.v = 0;
                if (MS == RT_MS_FULL && sc.needs_uv) /* (cast_closest's hit record) */
                    fast_finish<true, true>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, rec);
                else
                    fast_finish<false, true>(sc, ps.ro, ps.rd, ps.tm, a_tmax, a_ref, a_inst, rec);
                ps.thr = pk.get3(PK_THR);
                ps.L = mk(0.0, 0.0, 0.0);
                ps.prev_bsdf_pdf = pk.get(PK_PDF);
                const V3 wo = neg(unit(ps.rd));
                ParkedReq rq{false, pk}; /* parked until the next pair cast */
                const MatCtx mc = mat_prepare<MS>(sc, rec);
                shade_a_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, rq);
                pending = rq.valid;
                const bool go = shade_b_mis<MS, INTEG>(sc, ps, rec, mc, wo, rng, P.rr_start);
                RT_REGION(RG_PARK);
                ps.ro = rec.p; /* next ray origin and shadow ray origin */
                so = rec.p;
                pk.set3(PK_THR, ps.thr);
                if (ps.L.x != 0.0 || ps.L.y != 0.0 || ps.L.z != 0.0) pk.set3(PK_L, add(pk.get3(PK_L), ps.L));
                pk.set(PK_PDF, ps.prev_bsdf_pdf);
                ended = !go || ++ps.depth >= P.max_depth;
            }
            RTR_CLK(shade);
            RT_REGION(RG_REGEN);
            if (ended) {
                settle = true;
                ++s;
                begin = true; /* (unless the job is over: the pixel's word says, below) */
            }
        }
        /* a lane that was not casting has settled its job's last sample in this iteration: the job switch, step (3) */
        const bool job_end = !cast_a && *my_cell >= 0;
        if (__ballot(job_end)) { /* wave-uniform */
            RT_REGION(RG_EXCHANGE);
            const QueueArgs Q = queue_args();
            if (job_end) {
                uint32_t lo, hi;
                pk.get2(PK_PIXEL, lo, hi);
                const V3 acc = pk.get3(PK_ACC);
                const int cell = *my_cell;
                double* out = Q.P.partial + (size_t)cell * 3 * RTR_BLOCK + ((lo >> 12) & 0xf0u) + (lo & 0xfu); /* tile_pixel's tid */
                out[0] = acc.x;
                out[RTR_BLOCK] = acc.y;
                out[2 * RTR_BLOCK] = acc.z;
                atomicAdd(&Q.P.done[cell], 1);
                pk.set3(PK_ACC, mk(0.0, 0.0, 0.0));
            }
            if (queue_take(Q.P, Q.q_counter, Q.n_blocks, slot, job_end, pk, my_cell, s)) done = false, begin = true;
        }
        if (begin) {
            uint32_t lo, hi;
            int i, j, s_end;
            pk.get2(PK_PIXEL, lo, hi);
            queue_unpack(lo, hi, i, j, s_end);
            done = s >= s_end;
            if (!done) {
                RT_REGION(RG_BEGIN);
                const RenderK B = queue_image_size(P);
                camera_sample<RT_DRAW_MS(MS)>(sc, QueueCamera::get(B.W, B.H), B.seed, B.W, i, j, s, rng, ps.ro, ps.rd, ps.tm); /* begin_sample */
                ps.depth = 0, ps.specular_bounce = false;
                pk.set3(PK_THR, mk(1.0, 1.0, 1.0));
                pk.set(PK_PDF, 0.0);
            }
        }
        RT_REGION(RG_POLL);
        if (__any(cancel_poll_take(P, cancel_word))) { /* wave-uniform: every lane polled the same word */
            const unsigned long long here = __ballot(1);
            if ((int)__lane_id() == __builtin_ctzll(here)) atomicAdd(&queue_args().P.stats[7], 1ull);
            int left = 0; /* samples of the lane's job that have not ended */
            if (*my_cell >= 0) {
                uint32_t lo, hi;
                pk.get2(PK_PIXEL, lo, hi);
                left = (int)hi - s;
            }
            unsigned long long dropped = 0;
            for (unsigned long long m = __ballot(left > 0); m; m &= m - 1) /* wave-uniform */
                dropped += (unsigned long long)__builtin_amdgcn_readlane(left, __builtin_ctzll(m));
            slot.set_samples(slot.get_samples() - dropped);
            *my_cell = -1; /* the wave's jobs are dropped (an ended sample still settles: the loop's condition) */
            done = true;
        }
    }
    pk.get2(PK_NCAST, cnt.closest, cnt.shadow);
    clk.flush(P);
#ifdef RTR_REGION_PROFILE
    RT_REGION(RG_OTHER);
    __syncthreads();
    if (threadIdx.x < 2 * RT_PROF_REGIONS) {
        unsigned long long v = 0;
        for (int w = 0; w < 4; ++w) v += rt_prof_lds[w * 2 * RT_PROF_REGIONS + threadIdx.x];
        if (v) atomicAdd(&P.stats[RT_PROF_BASE + threadIdx.x], v);
    }
#endif
    unsigned long long b = wave_sum(cnt.closest), c = wave_sum(cnt.shadow);
    const unsigned long long taken = slot.get_samples();
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&P.stats[0], taken);
        atomicAdd(&P.stats[1], b);
        atomicAdd(&P.stats[2], c);
    }
}

/* rtr_li_samples / rtr_li_rays: Integrator::Li (renderer/integrator.h:12-19) of n camera samples of the image P
 * describes, or of n caller-given rays; one lane each.  `in` per item: camera sample = (i, j, s) as three int32 in
 * the first 12 bytes; ray = rtr_li_ray.  `out` per item: radiance (3 doubles), rng state at exit, closest / shadow
 * segment counts. */
struct LiOut {
    double L[3];
    uint32_t rng_exit;
    int32_t n_closest, n_shadow, pad;
};
template <int INTEG, int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_li(const DScene sc, const RenderK P, const int32_t* __restrict__ ijs,
                                                   const rtr_li_ray* __restrict__ rays, LiOut* __restrict__ out, long long n) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    uint32_t rng;
    V3 ro, rd;
    Real tm;
    if (rays) {
        const rtr_li_ray r = rays[k];
        ro = ld3(r.origin), rd = ld3(r.direction), tm = r.time, rng = r.rng_state;
    } else {
        const int i = ijs[3 * k], j = ijs[3 * k + 1], s = ijs[3 * k + 2];
        camera_sample(sc, P, i, j, s, rng, ro, rd, tm);
    }
    PathState ps;
    path_begin(ps, ro, rd, tm);
    PathCounters cnt;
    cnt.closest = 0, cnt.shadow = 0;
    while (bounce<INTEG, TRAV>(sc, ps, rng, st, P.max_depth, P.rr_start, cnt)) {
    }
    LiOut o;
    o.L[0] = ps.L.x, o.L[1] = ps.L.y, o.L[2] = ps.L.z;
    o.rng_exit = rng, o.n_closest = (int)cnt.closest, o.n_shadow = (int)cnt.shadow, o.pad = 0;
    out[k] = o;
}

/* rtr_accum_features: first-hit feature buffers, one workgroup per owned tile and one lane per pixel.  Samples s = 0 .. K-1
 * of pixel (i, j) build the camera ray of k_li (the ray sample s of a render builds) and cast it to its closest hit with
 * the render's traversal; the generator goes on from its state after get_ray, so a medium's free path is the path's own.
 * Per sample: albedo (3), normal (3), depth (1) -- include/rtr_hip.h -- summed in sample order and scaled by 1.0 / K
 * like k_resolve.  feat: [n_tiles][7][RTR_BLOCK]. */
#define RTR_FEAT 7
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_features(const DScene sc, const RenderK P, int K, double* __restrict__ feat) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    int i, j;
    bool active;
    tile_pixel(P, blockIdx.x, threadIdx.x, i, j, active);
    if (!active) return;
    double acc[RTR_FEAT];
    for (int s = 0; s < K; ++s) {
        uint32_t rng;
        V3 ro, rd;
        Real tm;
        camera_sample(sc, P, i, j, s, rng, ro, rd, tm);
        Hit rec;
        rec.u = 0, rec.v = 0;
        double f[RTR_FEAT] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0}; /* a miss */
        if (cast_closest<TRAV>(sc, ro, rd, tm, rec, rng, st)) {
            const FMat m = ld_const(sc.fmat, rec.mat);
            V3 a = mk(1.0, 1.0, 1.0);
            if (m.type == RTR_MAT_LAMBERTIAN || m.type == RTR_MAT_ISOTROPIC || m.type == RTR_MAT_PBR)
                a = tex_value(sc, m.tex[0], rec.u, rec.v, rec.p);
            else if (m.type == RTR_MAT_METAL)
                a = mk(m.f[0], m.f[1], m.f[2]);
            f[0] = a.x, f[1] = a.y, f[2] = a.z;
            if (m.type != RTR_MAT_ISOTROPIC) /* the phase material of a medium event: no normal */
                f[3] = rec.n.x, f[4] = rec.n.y, f[5] = rec.n.z;
            f[6] = rec.t * __builtin_sqrt(rd.x * rd.x + rd.y * rd.y + rd.z * rd.z);
        }
        for (int c = 0; c < RTR_FEAT; ++c) acc[c] = s == 0 ? f[c] : acc[c] + f[c];
    }
    const double scale = 1.0 / K;
    double* o = feat + (size_t)blockIdx.x * RTR_FEAT * RTR_BLOCK + threadIdx.x;
    for (int c = 0; c < RTR_FEAT; ++c) o[c * RTR_BLOCK] = scale * acc[c];
}

/* rtr_query_closest / rtr_query_occluded: hittable::hit of the scene root (geometry/hittable.h:25-32) for n caller-given
 * rays, one lane each, with the traversal a render of the scene walks.  The DScene arrives with needs_uv set: the hit
 * record's (u, v) are computed whether or not a texture reads them.
 * A bad ray (rtr_ray_bad: include/rtr_hip.h) is answered with a miss before any traversal code.  The shared-reciprocal
 * divisions hold for t_min >= 2^-100 (div_shared); a wave that holds a ray below that clears its copy of
 * DScene::shared_div, which makes RayDiv::fast false in every frame of its casts: the plain divisions, wave-uniform,
 * like the other operands RayDiv::fast votes on.
 * STAGED: the workgroup moves its RTR_BLOCK contiguous records with coalesced 8-byte loads and stores through dynamic
 * LDS behind the traversal stack (word `stage_word` of it) instead of every lane moving its own 80 / 88 bytes. */
#define RTR_QUERY_STAGE_BYTES (RTR_BLOCK * sizeof(rtr_ray_hit)) /* the larger of the two records */
#ifndef RTR_QUERY_STAGED_DEFAULT
#define RTR_QUERY_STAGED_DEFAULT 0 /* which form the library launches (RTR_QUERY_STAGED=0/1 overrides it: DESIGN.md 4.6) */
#endif
__host__ __device__ inline bool rtr_ray_bad(const rtr_ray& r, bool media) {
    bool ok = __builtin_isfinite(r.time) && __builtin_isfinite(r.t_min) && !(r.t_max != r.t_max);
    for (int a = 0; a < 3; ++a) ok = ok && __builtin_isfinite(r.origin[a]) && __builtin_isfinite(r.direction[a]);
    return !ok || (media && r.rng_state == 0);
}
/* this lane's ray; false past the end of the batch */
template <bool STAGED>
RT_DEV bool query_fetch(const rtr_ray* __restrict__ rays, long long n, double* stage, rtr_ray& r) {
    constexpr int W = (int)(sizeof(rtr_ray) / sizeof(double));
    const long long base = (long long)blockIdx.x * RTR_BLOCK;
    const bool live = base + threadIdx.x < n;
    if (STAGED) {
        const long long left = n - base;
        const int words = (int)(left < RTR_BLOCK ? left : RTR_BLOCK) * W;
        const double* src = reinterpret_cast<const double*>(rays + base);
        for (int w = threadIdx.x; w < words; w += RTR_BLOCK) stage[w] = src[w];
        __syncthreads();
        double v[W];
        for (int k = 0; k < W; ++k) v[k] = live ? stage[threadIdx.x * W + k] : 0.0;
        __builtin_memcpy(&r, v, sizeof r);
        __syncthreads(); /* the results go through the same words */
    } else if (live) {
        r = rays[base + threadIdx.x];
    }
    return live;
}
template <bool STAGED>
RT_DEV void query_store(rtr_ray_hit* __restrict__ hits, long long n, double* stage, bool live, const rtr_ray_hit& h) {
    constexpr int W = (int)(sizeof(rtr_ray_hit) / sizeof(double));
    const long long base = (long long)blockIdx.x * RTR_BLOCK;
    if (STAGED) {
        double v[W];
        __builtin_memcpy(v, &h, sizeof h);
        if (live)
            for (int k = 0; k < W; ++k) stage[threadIdx.x * W + k] = v[k];
        __syncthreads();
        const long long left = n - base;
        const int words = (int)(left < RTR_BLOCK ? left : RTR_BLOCK) * W;
        double* dst = reinterpret_cast<double*>(hits + base);
        for (int w = threadIdx.x; w < words; w += RTR_BLOCK) dst[w] = stage[w];
    } else if (live) {
        hits[base + threadIdx.x] = h;
    }
}
template <int TRAV, bool STAGED>
__global__ void __launch_bounds__(RTR_BLOCK) k_query_closest(DScene sc, const rtr_ray* __restrict__ rays,
                                                              rtr_ray_hit* __restrict__ hits, long long n, int media, int stage_word) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    double* stage = reinterpret_cast<double*>(lds_stack + stage_word);
    rtr_ray r;
    const bool live = query_fetch<STAGED>(rays, n, stage, r);
    if (!STAGED && !live) return;
    rtr_ray_hit h;
    h.t = 0, h.u = 0, h.v = 0;
    for (int a = 0; a < 3; ++a) h.p[a] = 0, h.n[a] = 0;
    h.hit = 0, h.front_face = 0, h.material = -1, h.rng_out = r.rng_state;
    const bool cast = live && !rtr_ray_bad(r, media != 0);
    if (__any(cast && !(r.t_min >= 0x1p-100))) sc.shared_div = 0;
    if (cast) {
        uint32_t rng = r.rng_state;
        Hit rec;
        rec.u = rec.v = __builtin_nan("");
        rec.mat = -1;
        rec.t = 0, rec.p = mk(0, 0, 0), rec.n = mk(0, 0, 0), rec.front = false;
        if (cast_closest<TRAV>(sc, ld3(r.origin), ld3(r.direction), r.time, rec, rng, st, r.t_min, r.t_max)) {
            h.hit = 1, h.front_face = (int)rec.front, h.material = rec.mat;
            h.t = rec.t, h.u = rec.u, h.v = rec.v;
            h.p[0] = rec.p.x, h.p[1] = rec.p.y, h.p[2] = rec.p.z;
            h.n[0] = rec.n.x, h.n[1] = rec.n.y, h.n[2] = rec.n.z;
        }
        h.rng_out = rng;
    }
    query_store<STAGED>(hits, n, stage, live, h);
}
template <int TRAV, bool STAGED>
__global__ void __launch_bounds__(RTR_BLOCK) k_query_any(DScene sc, const rtr_ray* __restrict__ rays, uint8_t* __restrict__ occluded,
                                                          uint32_t* __restrict__ rng_out, long long n, int media, int stage_word) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    double* stage = reinterpret_cast<double*>(lds_stack + stage_word);
    rtr_ray r;
    if (!query_fetch<STAGED>(rays, n, stage, r)) return; /* (no barrier follows) */
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    uint32_t rng = r.rng_state;
    bool blocked = false;
    const bool cast = !rtr_ray_bad(r, media != 0);
    if (__any(cast && !(r.t_min >= 0x1p-100))) sc.shared_div = 0;
    if (cast) {
        blocked = cast_shadow<TRAV>(sc, ld3(r.origin), ld3(r.direction), r.t_max, rng, st, r.time, r.t_min);
    }
    occluded[k] = blocked ? 1 : 0;
    if (rng_out) rng_out[k] = rng;
}

/* rtr_gather_occlusion / rtr_gather_radiance: N hemisphere samples per point, made in registers, cast, and reduced inside
 * the wave (include/rtr_hip.h has the contract: ray, reduction order, bad points).  Global lane g = block * RTR_BLOCK +
 * thread serves point g / G as lane g % G of its group (G = 1 << K.lg <= 64, so a group never leaves its wave and a wave
 * holds 64 / G points).  A lane takes the samples l, l + G, ... in order; the casts run under divergent EXEC like the
 * queries'.  The butterfly does not: lanes without a sample, of a bad point or of a point past the end carry +0.0 / 0 and
 * reach every __shfl_xor; only a wave whose first point is past the end returns.  Lane 0 of a group stores the record.
 * BCAST: lane 0 of the group loads the point and the group reads it from that lane, instead of every lane loading the
 * same 48 bytes (tools/time_gather.py measures both: DESIGN.md 4.8). */
#ifndef RTR_GATHER_BROADCAST_DEFAULT
#define RTR_GATHER_BROADCAST_DEFAULT 0 /* which form the library launches (RTR_GATHER_BROADCAST=0/1 overrides it) */
#endif
/* The lane-to-record map of every kernel that gives a record a group of G = 1 << lg lanes (the gathers, the probes, the
 * captures, the distance maps): this launch serves the records [k0, n), global lane g record k = k0 + g / G as lane
 * l = g % G.  false: the whole wave is past the end and returns.  A lane whose k >= n is not live: it stays, and carries
 * +0.0 / 0 through the butterfly.  The gathers and probes number their records from 0: k0 is the constant 0 there.
 * `live`, k < n, is a line of each caller: as a reference parameter of this function it makes the compiler associate the
 * lane predicates the other way round, and the kernels' code differs (profiles/r27_kres.txt). */
RT_DEV bool group_begin(long long k0, long long n, int lg, long long& k, int& l) {
    const long long g = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k0 + ((g & ~63ll) >> lg) >= n) return false;
    k = k0 + (g >> lg), l = (int)(g & ((1 << lg) - 1));
    return true;
}
struct GatherLane {
    long long k; /* point of this lane's group */
    int l;       /* lane in the group */
    bool cast;   /* the point exists and is not bad */
    V3 p, w;
};
template <bool BCAST>
RT_DEV bool gather_begin(const GatherK& K, GatherLane& L) {
    if (!group_begin(0, K.n, K.lg, L.k, L.l)) return false;
    const bool live = L.k < K.n;
    rtr_gather_point q;
    for (int a = 0; a < 3; ++a) q.p[a] = 0.0, q.n[a] = 0.0;
    if (BCAST) {
        if (live && L.l == 0) q = K.pts[L.k];
        const int src = (int)(threadIdx.x & 63) - L.l;
        for (int a = 0; a < 3; ++a) q.p[a] = __shfl(q.p[a], src, 64), q.n[a] = __shfl(q.n[a], src, 64);
    } else if (live) {
        q = K.pts[L.k];
    }
    double nlen;
    L.cast = !gather_point_bad(q, nlen) && live;
    L.p = ld3(q.p);
    L.w = scl(1 / nlen, ld3(q.n));
    return true;
}
RT_DEV uint32_t gather_ray(const GatherK& K, const GatherLane& L, int s, V3& d) {
    uint32_t rng = rtr_sample_seed_inline(K.seed, 1, 0, (int32_t)((uint32_t)L.k + K.point_base), s);
    gather_direction(L.w.x, L.w.y, L.w.z, rng, d.x, d.y, d.z);
    return rng;
}
/* (K, L: GatherK and GatherLane, or the capture's CaptureK and CaptureLane, which have the members this reads) */
template <typename KT, typename LT>
RT_DEV void gather_end(const KT& K, const LT& L, V3 a, int count) {
    for (int off = (1 << K.lg) >> 1; off > 0; off >>= 1) {
        a.x = a.x + __shfl_xor(a.x, off, 64), a.y = a.y + __shfl_xor(a.y, off, 64), a.z = a.z + __shfl_xor(a.z, off, 64);
        count = count + __shfl_xor(count, off, 64);
    }
    if (L.l != 0 || L.k >= K.n) return;
    rtr_gather_out o;
    const double scale = 1.0 / K.samples;
    o.v[0] = L.cast ? scale * a.x : 0.0, o.v[1] = L.cast ? scale * a.y : 0.0, o.v[2] = L.cast ? scale * a.z : 0.0;
    o.count = L.cast ? count : 0, o.valid = L.cast ? 1 : 0;
    K.out[L.k] = o;
}
template <int TRAV, bool BCAST>
__global__ void __launch_bounds__(RTR_BLOCK) k_gather_any(const DScene sc, const GatherK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    GatherLane L;
    if (!gather_begin<BCAST>(K, L)) return;
    V3 a = mk(0.0, 0.0, 0.0);
    int count = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            V3 d;
            uint32_t rng = gather_ray(K, L, s, d);
            if (!cast_shadow<TRAV>(sc, L.p, d, K.t_max, rng, st, K.time, K.t_min)) a = add(a, d), ++count;
        }
    gather_end(K, L, a, count);
}
template <int INTEG, int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_gather_li(const DScene sc, const GatherK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    GatherLane L;
    if (!gather_begin<false>(K, L)) return;
    V3 a = mk(0.0, 0.0, 0.0);
    int count = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            V3 d;
            uint32_t rng = gather_ray(K, L, s, d);
            PathState ps;
            path_begin(ps, L.p, d, K.time);
            PathCounters cnt;
            cnt.closest = 0, cnt.shadow = 0;
            while (bounce<INTEG, TRAV>(sc, ps, rng, st, K.max_depth, K.rr_start, cnt)) {
            }
            a = add(a, ps.L), ++count;
        }
    gather_end(K, L, a, count);
}

/* rtr_probe_visibility / rtr_probe_radiance: N sphere samples per probe, projected onto the nine SH functions of
 * sh_basis and reduced like a gather (include/rtr_hip.h has the contract).  The mapping is the gathers': global lane g
 * serves point g / G as lane g % G, lanes without a sample, of a bad point or of a point past the end carry +0.0 / 0
 * through every __shfl_xor, lane 0 of a group stores the record.  A probe has no normal and the records differ, so the
 * kernels have a begin and an end of their own and leave gather_begin / gather_end as they are.
 * k_probe_li keeps its 27 sums per lane in LDS behind the traversal stack (RTR_PROBE_LDS_SUMS): word i of
 * lane l is sums[i * RTR_BLOCK + l], each lane touches only its own words, so no barrier is needed; the butterfly reads
 * them back into registers behind the sample loop. */
#ifndef RTR_PROBE_LDS_SUMS
#define RTR_PROBE_LDS_SUMS 1 /* 0: the sums of k_probe_li stay in registers across the bounce loop */
#endif
constexpr size_t probe_sum_bytes() { return RTR_PROBE_LDS_SUMS ? (size_t)27 * sizeof(double) * RTR_BLOCK : 0; }
struct ProbeLane {
    long long k; /* point of this lane's group */
    int l;       /* lane in the group */
    bool cast;   /* the point exists and is not bad */
    V3 p;
};
RT_DEV bool probe_begin(const ProbeK& K, ProbeLane& L) {
    if (!group_begin(0, K.n, K.lg, L.k, L.l)) return false;
    const bool live = L.k < K.n;
    rtr_probe_point q;
    for (int a = 0; a < 3; ++a) q.p[a] = 0.0;
    if (live) q = K.pts[L.k];
    L.cast = !probe_point_bad(q) && live;
    L.p = ld3(q.p);
    return true;
}
RT_DEV uint32_t probe_ray(const ProbeK& K, const ProbeLane& L, int s, V3& d) {
    uint32_t rng = rtr_sample_seed_inline(K.seed, 1, 0, (int32_t)((uint32_t)L.k + K.point_base), s);
    probe_direction(rng, d.x, d.y, d.z);
    return rng;
}
/* the butterfly over C sums and the count; afterwards lane 0 of a group holds the totals */
template <int C>
RT_DEV void probe_reduce(const ProbeK& K, double (&a)[C], int& count) {
    for (int off = (1 << K.lg) >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < C; ++i) a[i] = a[i] + __shfl_xor(a[i], off, 64);
        count = count + __shfl_xor(count, off, 64);
    }
}
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_probe_any(const DScene sc, const ProbeK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    ProbeLane L;
    if (!probe_begin(K, L)) return;
    double a[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = 0.0;
    int count = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            V3 d;
            uint32_t rng = probe_ray(K, L, s, d);
            if (!cast_shadow<TRAV>(sc, L.p, d, K.t_max, rng, st, K.time, K.t_min)) {
                double Y[9];
                sh_basis(d.x, d.y, d.z, Y);
#pragma unroll
                for (int i = 0; i < 9; ++i) a[i] = a[i] + Y[i];
                ++count;
            }
        }
    probe_reduce(K, a, count);
    if (L.l != 0 || L.k >= K.n) return;
    rtr_probe_vis o;
    const double scale = 1.0 / K.samples;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.c[i] = L.cast ? scale * a[i] : 0.0;
    o.count = L.cast ? count : 0, o.valid = L.cast ? 1 : 0;
    static_cast<rtr_probe_vis*>(K.out)[L.k] = o;
}
template <int INTEG, int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_probe_li(const DScene sc, const ProbeK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    ProbeLane L;
    if (!probe_begin(K, L)) return;
    double a[27];
#if RTR_PROBE_LDS_SUMS
    double* sums = reinterpret_cast<double*>(lds_stack + K.sum_word) + threadIdx.x;
#pragma unroll
    for (int i = 0; i < 27; ++i) sums[i * RTR_BLOCK] = 0.0;
#else
#pragma unroll
    for (int i = 0; i < 27; ++i) a[i] = 0.0;
#endif
    int count = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            V3 d;
            uint32_t rng = probe_ray(K, L, s, d);
            PathState ps;
            path_begin(ps, L.p, d, K.time);
            PathCounters cnt;
            cnt.closest = 0, cnt.shadow = 0;
            while (bounce<INTEG, TRAV>(sc, ps, rng, st, K.max_depth, K.rr_start, cnt)) {
            }
            double Y[9];
            sh_basis(d.x, d.y, d.z, Y);
#pragma unroll
            for (int i = 0; i < 9; ++i) {
#if RTR_PROBE_LDS_SUMS
                sums[(3 * i) * RTR_BLOCK] = sums[(3 * i) * RTR_BLOCK] + Y[i] * ps.L.x;
                sums[(3 * i + 1) * RTR_BLOCK] = sums[(3 * i + 1) * RTR_BLOCK] + Y[i] * ps.L.y;
                sums[(3 * i + 2) * RTR_BLOCK] = sums[(3 * i + 2) * RTR_BLOCK] + Y[i] * ps.L.z;
#else
                a[3 * i] = a[3 * i] + Y[i] * ps.L.x, a[3 * i + 1] = a[3 * i + 1] + Y[i] * ps.L.y, a[3 * i + 2] = a[3 * i + 2] + Y[i] * ps.L.z;
#endif
            }
            ++count;
        }
#if RTR_PROBE_LDS_SUMS
#pragma unroll
    for (int i = 0; i < 27; ++i) a[i] = sums[i * RTR_BLOCK];
#endif
    probe_reduce(K, a, count);
    if (L.l != 0 || L.k >= K.n) return;
    rtr_probe_sh o;
    const double scale = 1.0 / K.samples;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        for (int ch = 0; ch < 3; ++ch) o.c[i][ch] = L.cast ? scale * a[3 * i + ch] : 0.0;
    o.count = L.cast ? count : 0, o.valid = L.cast ? 1 : 0;
    static_cast<rtr_probe_sh*>(K.out)[L.k] = o;
}

/* rtr_capture_cube: a cube map of mean radiance about each centre, N rays through every texel (include/rtr_hip.h has the
 * contract).  A texel is a "point" of the gathers' mapping: global lane g serves record K.k0 + g / G of K.out as lane g % G,
 * a group never leaves its wave, lanes without a sample, of a bad centre or past the end carry +0.0 / 0 through every
 * __shfl_xor, lane 0 of a group stores the record: gather_end as it is.  Begin and ray are the capture's own: the texel
 * number of the call (K.first + record) gives the centre (texel / 6 S^2) and (face, row, column), capture_direction of
 * rt_render.h the direction. */
struct CaptureLane {
    long long k; /* record of K.out of this lane's group */
    int l;       /* lane in the group */
    bool cast;   /* the texel exists and its centre is not bad */
    V3 p;
    int e, f, a, b;   /* texel of the centre's capture: e = (f * S + b) * S + a */
    uint32_t centre;  /* the centre's number under the seed: its index in the call + point_base */
};
RT_DEV bool capture_begin(const CaptureK& K, CaptureLane& L) {
    if (!group_begin(K.k0, K.n, K.lg, L.k, L.l)) return false;
    const bool live = L.k < K.n;
    const long long texel = K.first + (live ? L.k : K.k0);
    const long long c = texel / K.F;
    L.e = (int)(texel - c * K.F);
    L.f = L.e / K.SS;
    const int r = L.e - L.f * K.SS;
    L.b = r / K.S, L.a = r - L.b * K.S;
    L.centre = (uint32_t)c + K.point_base;
    rtr_probe_point q;
    for (int i = 0; i < 3; ++i) q.p[i] = 0.0;
    if (live) q = K.pts[c];
    L.cast = !probe_point_bad(q) && live;
    L.p = ld3(q.p);
    return true;
}
RT_DEV uint32_t capture_ray(const CaptureK& K, const CaptureLane& L, int s, V3& d) {
    uint32_t rng = rtr_sample_seed_inline(K.seed, K.F, L.e, (int32_t)L.centre, s);
    capture_direction(K.S, L.f, L.a, L.b, K.jitter, rng, d.x, d.y, d.z);
    return rng;
}
template <int INTEG, int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_capture_li(const DScene sc, const CaptureK K) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    CaptureLane L;
    if (!capture_begin(K, L)) return;
    V3 a = mk(0.0, 0.0, 0.0);
    int count = 0;
    if (L.cast)
        for (int s = L.l; s < K.samples; s += 1 << K.lg) {
            V3 d;
            uint32_t rng = capture_ray(K, L, s, d);
            PathState ps;
            path_begin(ps, L.p, d, K.time);
            PathCounters cnt;
            cnt.closest = 0, cnt.shadow = 0;
            while (bounce<INTEG, TRAV>(sc, ps, rng, st, K.max_depth, K.rr_start, cnt)) {
            }
            a = add(a, ps.L), ++count;
        }
    gather_end(K, L, a, count);
}
