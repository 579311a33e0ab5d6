/*
 * rtr_hip_test.h -- entry points of librtr_hip_test.so, a SEPARATE library next to librtr_hip.so (it links against
 * it): device unit kernels that run the product's own device functions (csrc/rt_device.h) over golden-vector records
 * (include/rtr_testrec.h), one lane per record, plus counter-calibration and instruction-level checks, a unit
 * entry that runs the temporal kernels of the denoiser over caller-given planes (rtr_test_temporal_planes), three that
 * hold the accumulator kernels to synthetic tile state (rtr_test_accum_load / _plan / _commit), and a host-only entry
 * that says what lowering makes of a scene and which kernel it would get (rtr_test_scene_plan).  They
 * exist so tests can compare the HIP path with the oracle below the whole-image level; none of this code is in the
 * product library, and a renderer integration only needs rtr_hip.h.
 */
#ifndef RTR_HIP_TEST_H
#define RTR_HIP_TEST_H

#include "rtr_hip.h"
#include "rtr_testrec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* In-place on HOST arrays of records: inputs are read, outputs overwritten. */
int rtr_test_hits(rtr_context* ctx, rtr_hit_record* recs, int64_t n);
int rtr_test_materials(rtr_context* ctx, rtr_mat_record* recs, int64_t n);
int rtr_test_lights(rtr_context* ctx, rtr_light_record* recs, int64_t n);
int rtr_test_li(rtr_context* ctx, const rtr_render_params* params, rtr_li_record* recs, int64_t n);
/* rtr_test_materials runs mat_prepare, mat_sample, mat_eval, mat_pdf and mat_emitted, and then the fused mat_eval_pdf the MIS
 * kernels call for the light sample, on (wo, wi_in): the record's `pad` gets bit 0 where its f differs from mat_eval in any
 * bit and bit 1 where its pdf differs from mat_pdf (a NaN equals a NaN), so 0 means the fused form is the separate ones.
 * rtr_test_scatter: mat_prepare + the legacy mat_scatter of integrators 0 and 1 with r_in.direction() = wo (not normalised)
 * in the same record: sample_ok the return value, s_wi the scattered direction, s_f the attenuation, rng_out the state
 * after the call; every other output is zero. */
int rtr_test_scatter(rtr_context* ctx, rtr_mat_record* recs, int64_t n);
/* The same kernels instantiated for material set ms (RT_MS_LEAN 0, RT_MS_FULL 1, RT_MS_QUADLIT 2 of csrc/rt_device.h) as the
 * render kernels are: mat_prepare<ms>, mat_sample<ms>, ..., light_sample<ms>, light_pdf<ms>.  RTR_ERR_UNSUPPORTED, the records
 * untouched, where the uploaded scene is not of that class by the predicates of mega_variant (rtr_scene_plan::lean_materials;
 * quad_lights_only and no texture that reads (u, v)).  The entries without _ms are ms = RT_MS_FULL. */
int rtr_test_materials_ms(rtr_context* ctx, rtr_mat_record* recs, int64_t n, int32_t ms);
int rtr_test_scatter_ms(rtr_context* ctx, rtr_mat_record* recs, int64_t n, int32_t ms);
int rtr_test_lights_ms(rtr_context* ctx, rtr_light_record* recs, int64_t n, int32_t ms);
/* pow5 of csrc/rt_device.h (the device's pow(x, 5.0): x^5 in double-double arithmetic) over a host array, on the device and
 * as a host build of the same function (no context, no GPU).  Both are the same fused multiply-adds without contraction. */
int rtr_test_pow5(rtr_context* ctx, const double* x, double* out, int64_t n);
int rtr_test_pow5_host(const double* x, double* out, int64_t n);
/* rtr_test_hits through the closest-hit cast of the FLAT kernels (cast_closest<RT_TRAV_FLAT> or, in a scene with guarded
 * references, <RT_TRAV_FLAT_GUARD>), which the megakernel runs on flat scenes and no query or per-ray kernel does: the flat
 * scan, then the hit record from the scene's finish records (rtr_finish_record) where it has them.  with_uv: compute
 * (u, v) as a scene with image textures would.  *used_finish (may be NULL): whether the uploaded scene has finish
 * records.  RTR_ERR_UNSUPPORTED where no flat kernel runs the scene (or rtr_test_reference_order is on). */
int rtr_test_flat_hits(rtr_context* ctx, rtr_hit_record* recs, int64_t n, int with_uv, int32_t* used_finish);

/* Which kernel instantiation the context's last render call launched, recorded on the host as it was enqueued.
 * Megakernel: k_mega<integrator, trav, ms, sorted, accum, pair> (accum: 0 one-shot, 1 accumulator pass, 2 accumulator pass
 * with moments), or with queue set k_mega_queue<integrator, trav, ms>; wavefront: the plan (lean / quadlit / sort / media / machine /
 * trav) and wf_shade<integrator, PH, ms, sorted> for every PH bit of shade_phases.  trav and ms are the RT_TRAV_* and
 * RT_MS_* values of csrc/rt_device.h.  pipeline = -1: no render of this context has launched anything yet. */
typedef struct rtr_kernel_record {
    int32_t pipeline, integrator, trav, ms, sorted, shade_phases;
    int32_t lean, quadlit, sort, media, machine;
    int32_t accum;
    int32_t pair, queue; /* megakernel: the pair-cast instantiation k_mega<..., accum, true> / its job-queue twin
                            k_mega_queue<integrator, trav, ms> ran in its place (one-shot renders only) */
} rtr_kernel_record;
/* size_of_out must be sizeof(rtr_kernel_record) */
int rtr_test_last_kernel(rtr_context* ctx, rtr_kernel_record* out, size_t size_of_out);

/* Which gather kernel the context's last rtr_gather_* call launched (of its last slice), recorded on the host as it was
 * enqueued: k_gather_li<integ, trav> of a radiance gather, or with integ = -1 k_gather_any<trav, broadcast> of an occlusion
 * gather.  trav is the RT_TRAV_* template value, after the substitution of the media kernel for the reference-order walk
 * of integrators 0, 2 and 3; lg is log2 of the lanes that share a point.  trav = -1: no gather has launched anything yet. */
typedef struct rtr_gather_record {
    int32_t integ, trav, broadcast, lg;
} rtr_gather_record;
/* size_of_out must be sizeof(rtr_gather_record) */
int rtr_test_last_gather(rtr_context* ctx, rtr_gather_record* out, size_t size_of_out);

/* The same for the light probes: k_probe_li<integ, trav> of the last rtr_probe_radiance call, or with integ = -1
 * k_probe_any<trav> of the last rtr_probe_visibility call; trav = -1: no probe call has launched anything yet. */
typedef struct rtr_probe_record {
    int32_t integ, trav, lg;
} rtr_probe_record;
/* size_of_out must be sizeof(rtr_probe_record) */
int rtr_test_last_probe(rtr_context* ctx, rtr_probe_record* out, size_t size_of_out);

/* And for the environment captures: k_capture_li<integ, trav> of the last rtr_capture_cube call; trav = -1: none yet. */
typedef struct rtr_capture_record {
    int32_t integ, trav, lg;
} rtr_capture_record;
/* size_of_out must be sizeof(rtr_capture_record) */
int rtr_test_last_capture(rtr_context* ctx, rtr_capture_record* out, size_t size_of_out);

/* And for the probe distance maps: k_probe_depth<trav> of the last rtr_probe_depth call; trav = -1: none yet. */
typedef struct rtr_probe_depth_record {
    int32_t trav, lg;
} rtr_probe_depth_record;
/* size_of_out must be sizeof(rtr_probe_depth_record) */
int rtr_test_last_probe_depth(rtr_context* ctx, rtr_probe_depth_record* out, size_t size_of_out);

/* What the library makes of a scene before anything reaches a device: the validator, the host-only lowering
 * (csrc/rt_lower.h: lower_scene) and the two decisions every launch hangs on -- pick_trav and, for `integrator` and the
 * render `flags`, mega_variant (csrc/rt_select.h).  Needs no context and no GPU.  RT_TRAV_*, RT_MS_*, RT_TIE_FLAG and
 * RT_GUARD_FLAG are those of csrc/rt_device.h. */
typedef struct rtr_scene_plan {
    int32_t fast_ok, has_media;                /* rtr_scene_info */
    int32_t flat_scene, flat_guarded;          /* no box tree, no tie-capable reference; without / with guarded references */
    int32_t lean_materials, quad_lights_only;  /* the material and light class of the kernels */
    int32_t uv_order_dependent;                /* a moving_sphere carries a material that reads (u,v) */
    int32_t machine_ok, guarded_program;       /* the traversal machine has a program / one it does not run */
    int32_t top_tree, needs_uv, n_material_types;
    int32_t shared_div, pair_cast;             /* DScene members of the same names */
    int32_t n_steps, n_visits, n_refs;         /* step program (the default one-step program included), visits, references */
    int32_t fast_stack_words, walk_stack_words; /* LDS stack words per lane: compiled traversals / reference-order walk */
    int32_t n_tie_refs, n_guard_refs;          /* references that carry RT_TIE_FLAG / RT_GUARD_FLAG */
    int32_t pick_trav;                         /* RT_TRAV_* pick_trav chooses for `flags` */
    int32_t mega_trav, mega_ms, mega_sorted, mega_pair; /* the MegaVariant: k_mega<integrator, trav, ms, sorted, ., pair> */
    int32_t n_finish;                          /* finish records: n_refs, or 0 for a scene that gets none */
} rtr_scene_plan;
/* The finish record of a reference (csrc/rt_device.h: struct FFin): what the flat kernels fetch to build the hit record
 * of a hit on it.  A scene gets them when it is flat (flat_scene or flat_guarded), every transform chain of its instances
 * has at most two ops, and no reference is a moving sphere or sits under more than 31 wrappers.
 * The reference's hit record is: the primitive's own hit() tail on the ray taken through level 0, then level 1; then the
 * epilogue of level 1 and of level 0 (translate::hit / rotate_y::hit after the child's hit); then front ^= flip. */
typedef struct rtr_finish_record {
    int32_t kind;    /* 0, 1, 2: rectangle with its normal along x, y, z (yz_rect, xz_rect, xy_rect); 3: sphere */
    int32_t material;
    int32_t levels;  /* bits 0-1: transforms above the primitive (0..2); bit 2: level 0, the OUTERMOST, is a rotate_y (else a
                        translate); bit 3: level 1 is a rotate_y */
    int32_t flip;    /* parity of the flip_face wrappers outside the outermost transform (of all of them without a level):
                        those inside are overwritten by the set_face_normal of the level above them */
    double op[2][3]; /* per level: the translate's offset, or the rotate_y's sin, cos, 0; zero where absent */
    double g[4];     /* sphere: centre, radius; rectangle: a0 a1 b0 b1 */
} rtr_finish_record; /* 96 bytes */
/* ref_flags (may be NULL when cap is 0) receives the `reserved` word of the first min(cap, n_refs) reference records:
 * visiting order | RT_TIE_FLAG | RT_GUARD_FLAG; finish (may be NULL when finish_cap is 0) the first min(finish_cap,
 * n_finish) finish records, in reference order.  Returns RTR_OK or the validator's status for a scene it rejects. */
int rtr_test_scene_plan(const rtr_scene_desc* scene, int32_t integrator, int32_t flags, rtr_scene_plan* out,
                        int32_t* ref_flags, int64_t cap, rtr_finish_record* finish, int64_t finish_cap);

/* The frame shape lowering gives every instance of the scene's sub-scene 0 (csrc/rt_device.h: FInst::shape), which the
 * pair cast switches on: 0 none, 1 T, 2 R, 3 T.R (translate outermost), 4 R.T, 5 other (more than two ops, or two of a
 * kind).  shapes receives the first min(cap, *n_instances) of them.  Needs no context and no GPU. */
int rtr_test_pair_frames(const rtr_scene_desc* scene, int32_t* shapes, int64_t cap, int32_t* n_instances);
/* Host build of the pair cast's frame block (csrc/rt_device.h: pair_frame) on one ray pair per record, for a frame of
 * `shape` (0..4) with the operands ops[0..2] of the outer op and ops[3..5] of the inner one (translate: offset; rotate_y:
 * sin, cos, 0; unused ones are ignored).  same_frame: pair_frame's origins and directions equal, in every bit, the ray
 * taken down op by op as translate::hit / rotate_y::hit do (restated in the test library), d.y untouched.  fo, fd: what
 * pair_frame made of ray A.  Needs no context and no GPU. */
typedef struct rtr_pair_frame_record {
    double ao[3], ad[3], bo[3], bd[3]; /* in */
    double fo[3], fd[3];               /* out */
    int32_t same_frame, pad;           /* out */
} rtr_pair_frame_record;
int rtr_test_pair_frame_host(int32_t shape, const double* ops, rtr_pair_frame_record* recs, int64_t n);
/* trace_pair of the MIS pair-cast kernels on one ray pair per lane -- A: closest hit in [0.001, a_tmax], B: any hit in
 * [0.001, b_tmax] -- next to the two single casts of the flat kernels for the same lanes, trace_fast<false> for A and
 * trace_fast<true> for B.  Lanes of one wave share the wave-level votes of the pair cast, as in a render.
 * RTR_ERR_UNSUPPORTED unless the uploaded scene is a pair-cast scene (rtr_scene_plan::pair_cast). */
typedef struct rtr_pair_record {
    double ao[3], ad[3], a_tmax, bo[3], bd[3], b_tmax; /* in */
    double a_t, s_a_t;                                  /* out: t of A's hit (a_tmax without one), pair / single */
    int32_t a_ref, a_inst, b_hit;                       /* out, pair cast: A's reference and instance (-1: none), B hit */
    int32_t s_a_ref, s_a_inst, s_b_hit;                 /* out, single casts */
    int32_t recasts, pad;                               /* out: casts of the lane's wave that failed a vote of the pair
                                                           path and were cast again through the single casts */
} rtr_pair_record; /* 160 bytes */
int rtr_test_pair_cast(rtr_context* ctx, rtr_pair_record* recs, int64_t n);
/* The same with the choice between the product's two texts of the pair cast: recast != 0 (what rtr_test_pair_cast runs):
 * the lean material set's kernels' -- the pair path alone, and both rays again through the single casts where a vote
 * fails --; recast == 0: the per-frame fallback of every other pair-cast kernel (`recasts` stays 0). */
int rtr_test_pair_cast_text(rtr_context* ctx, rtr_pair_record* recs, int64_t n, int32_t recast);
/* The resident shadow request of the job-queue kernel (k_mega_queue) over `casts` >= 1 pair casts of every lane, with that
 * kernel's own steps around trace_pair: ray B of the record is parked as the request of the first cast and is dead (t_max
 * 0, direction and origin left where they are) in every later one; ray A is cast every time.  The pair-cast columns are
 * those of the first cast, `recasts` counts over all of them.  Errors as rtr_test_pair_cast. */
int rtr_test_pair_resident(rtr_context* ctx, rtr_pair_record* recs, int64_t n, int32_t casts);

/* Host builds of the job queue's own device functions (csrc/rt_render.h: queue_block, queue_pack / queue_unpack), which
 * k_mega_queue -- the persistent-grid twin of the pair-cast kernels -- decodes block ids and keeps its per-lane job with.
 * rtr_test_queue_blocks_host: blocks 0 .. n-1 of a launch over n_tiles owned tiles with `chunks` partial sums of `spp`
 * samples (n_big, big_spp, small_spp: the guided split, all 0 for equal chunks); ref_s0 / ref_s1 are chunk_range of the
 * decoded chunk.  rtr_test_queue_pack_host: packs (i, j, s_end) into the two halves of the parked word and unpacks them
 * again into out[0..2].  Neither needs a context or a GPU. */
typedef struct rtr_queue_block_record {
    int32_t slot, quarter, chunk, s0, s1, ref_s0, ref_s1, pad;
} rtr_queue_block_record;
int rtr_test_queue_blocks_host(int32_t n_tiles, int32_t spp, int32_t chunks, int32_t n_big, int32_t big_spp, int32_t small_spp,
                               rtr_queue_block_record* recs, int64_t n);
int rtr_test_queue_pack_host(int32_t i, int32_t j, int32_t s_end, uint32_t* lo, uint32_t* hi, int32_t* out);

/* Make rtr_test_hits (which takes no render params) use the reference-order traversal. */
int rtr_test_reference_order(rtr_context* ctx, int on);

/* Counter calibration for profiles/: stream `n_doubles` doubles through the access shape of the wavefront
 * stages (one 8-byte word per lane, consecutive lanes consecutive words: out[i] = in[i] + 1), `repeat` times.
 * The launch reads and writes exactly n_doubles * 8 bytes each per repetition, which is what rocprofv3's
 * FETCH_SIZE / WRITE_SIZE of the same run are compared with (MI355X_MICROARCH.md, HBM: widths other than
 * 16 bytes per lane are uncalibrated).  Returns RTR_OK or a negative status. */
int rtr_test_stream8(rtr_context* ctx, int64_t n_doubles, int repeat);

/* The samplers take sin and cos of phi = 2 pi r for r = s * 2^-32, s any state of the 32-bit generator
 * (vec3.h:261-269, material.h:268-275); the device evaluates both with ONE sincos().  This walks ALL 2^32 values of
 * s and counts those where sincos(phi) and the pair sin(phi), cos(phi) differ in any bit: *mismatches must be 0.
 * *tested: the values of s the kernel compared, 2^32 when it walked them all. */
int rtr_test_sincos_exhaustive(rtr_context* ctx, uint64_t* mismatches, uint64_t* tested);

/* Measured issue costs for bench.py's `valu_slot_utilisation`: shader cycles a wave spends per instruction of one class
 * while four waves share each SIMD (so a pipe-bound class reads four times its pipe cost), classes in this order:
 * v_fma_f64, v_add_f64, v_mul_f64, v_rcp_f64, v_rsq_f64, v_cmp_lt_f64, v_cndmask_b32, v_mov_b32, v_fma_f32, s_and_b64,
 * v_div_scale_f64, v_div_fixup_f64, {v_cmp_lt_f64 + dependent s_and_b64}, v_cndmask_b32 with a scalar-pair mask, v_min_f32,
 * {v_cmp_lt_f32 + v_cndmask_b32}, v_cndmask_b32 into four destinations, {v_cmp_lt_f64 + v_cndmask_b32}.  Fills
 * cycles_per_inst[0 .. n) (n <= 18). */
int rtr_test_issue_rates(rtr_context* ctx, double* cycles_per_inst, int n);

/* The primitive tests divide many numerators by the same ray-direction component through a shared refined reciprocal
 * (rt_device.h: div_shared) instead of the compiler's eleven-instruction division.  This compares the two on 2^32
 * operand pairs from the range the short form is used in; *mismatches (quotients that differ in any bit) must be 0.
 * *tested: the pairs the kernel compared, 2^32 when every pair drawn was in that range. */
int rtr_test_shared_division(rtr_context* ctx, uint64_t* mismatches, uint64_t* tested);

/* Shading and the sample start divide by numbers that are the same for a whole scene or launch -- an edge of a quad light,
 * pi, the image size -- through a reciprocal made once (rt_device.h: udiv).  rtr_test_udiv runs udiv beside the
 * compiler's n / d for every one of the n numerators against every one of the m divisors, the divisor's record made on
 * the device as the kernels make theirs.  *mismatches
 * (quotients that differ in any bit, a NaN equal to a NaN) must be 0; *tested = n * m.  Needs no scene. */
int rtr_test_udiv(rtr_context* ctx, const double* numerators, int64_t n, const double* divisors, int32_t m,
                  uint64_t* mismatches, uint64_t* tested);
/* Shading takes 1.0 / d and sqrt(x) of a lane's own numbers through short forms when every lane of the wave holds an
 * operand in the ordinary range, and through the compiler's expansion otherwise (rt_device.h: rcp_lane; sqrt_lane and
 * sqrt_rcp_lane).  Each entry runs one kernel over 2^26 operands made from a counter -- random mantissas under every
 * exponent of the accepted window, and in every fourth wave one lane with a value of rtr_test_lane_specials -- beside the
 * compiler's result.  *mismatches (operands with a result that differs in any bit, NaN payloads included) must be 0;
 * *tested = 2^26; *short_sets: how many operands sat in a wave that voted for the short form; first[0 .. 4): a mismatching
 * operand, 0, its result and the expected result as bits, zeros when there is none.  Needs no scene. */
int rtr_test_rcp_lane(rtr_context* ctx, uint64_t* mismatches, uint64_t* tested, uint64_t* short_sets, uint64_t* first);
int rtr_test_sqrt_lane(rtr_context* ctx, uint64_t* mismatches, uint64_t* tested, uint64_t* short_sets, uint64_t* first);
/* The edge values of those kernels as bits: every window bound, the smallest normal number and 2^1023 with their
 * neighbours, zero, denormals, infinity, NaNs, the largest finite number and 1, each with both signs.  Fills out[0 .. min(cap,
 * count)) and returns the count.  No GPU needed. */
int rtr_test_lane_specials(uint64_t* out, int64_t cap);
/* The host build of the short forms' arithmetic, the vote replaced by a flag per element: op 0: 1.0 / a, 1: sqrt(a).
 * took_short[k] = the element was inside the window and went through the short form; the seeds of the host build are the
 * correctly rounded reciprocal and reciprocal square root with their low coarse_bits bits cleared (0 .. 40; 29 is the
 * accuracy the ISA manual gives v_rcp_f64 and v_rsq_f64).  Not thread-safe.  No GPU needed. */
int rtr_test_lane_host(int32_t op, int32_t coarse_bits, const double* a, double* out, int32_t* took_short, int64_t n);

/* A random draw in (-1, 1) is the generator's 32-bit state s as the double -1 + s * 2^-31; the lean kernels make it with
 * one addition from a double whose low word is s (rt_device.h: draw_sym_join).  rtr_test_draw_forms walks ALL 2^32 states
 * on the device and counts those where the joined form and the plain text differ in any bit: *mismatches must be 0,
 * *tested 2^32; *first: such a state + 1, or 0.  Needs no scene. */
int rtr_test_draw_forms(rtr_context* ctx, uint64_t* mismatches, uint64_t* tested, uint64_t* first);
/* The functions that draw -- random_in_unit_sphere, random_in_unit_disk, random_cosine_direction, rng_range(0.25, 7.5),
 * rng_int(0, 6), one after the other -- from n states seeded by `seed`, one per lane, with the joined form and in the
 * plain text (a second instantiation in this library).  *mismatches: lanes where an output bit or the
 * state after a call differs, must be 0; *tested = n; *first: such a lane's starting state, or 0.  Needs no scene. */
int rtr_test_draw_callers(rtr_context* ctx, uint64_t seed, int64_t n, uint64_t* mismatches, uint64_t* tested, uint64_t* first);
/* The host build of the joined form: out[k] = draw_sym_join(s[k]).  No GPU needed. */
int rtr_test_draw_host(const uint32_t* s, double* out, int64_t n);
/* The host build of the joined form beside the plain text on the states first, first + stride, ... (count of them, all
 * below 2^32), split over `threads` threads: *mismatches = states where it differs in any bit, *tested = count.
 * first 0, count 2^32, stride 1 is every state.  No GPU needed. */
int rtr_test_draw_host_range(uint64_t first, uint64_t count, uint64_t stride, int32_t threads, uint64_t* mismatches, uint64_t* tested);

/* The uploaded scene's table of shading constants (rt_device.h: SceneConsts, made on the device by rtr_upload_scene) as
 * 8-byte words -- 1 / n_lights, 0, pi, rcp_refined(pi); then per light len2(U), its refined reciprocal, len2(V), its refined
 * reciprocal, the `safe` flag in the low half of a word -- into `table`, and a second evaluation of the same expressions
 * by a kernel of the test library into `again`: 4 + 5 * n_lights words each (cap: the words each array holds; 0 only
 * asks for *n_lights). */
int rtr_test_scene_consts(rtr_context* ctx, uint64_t* table, uint64_t* again, int64_t cap, int32_t* n_lights);

/* The temporal stage of rtr_accum_denoise_temporal alone, over HOST planes: the product's k_temporal_blend and
 * k_temporal_store, launched with the grids of a frame, on a width x height region at (x0, y0) of an image_width x
 * image_height image.  h_color, h_q, h_count and h_feat are the planes of rtr_denoise_host, h_hist_in the last frame's
 * history in the layout of rtr_history_planes (10 doubles per pixel, rows of `width` pixels; read only when `have`), cam
 * the current camera and prev the one the history was seen from.  h_c gets the blended demodulated colour c' (3 doubles
 * per pixel), h_var the variance var' that enters the first a-trous pass, h_hist_out the history the frame writes.
 * Pixels with count 0 keep the caller's h_c and h_var values and have an all-zero history.  Needs no scene.  Blocking.
 * RTR_ERR_INVALID for a NULL pointer, a region outside the image, a negative count or parameters out of range. */
int rtr_test_temporal_planes(rtr_context* ctx, int32_t width, int32_t height, int32_t image_width, int32_t image_height,
                             int32_t x0, int32_t y0, const rtr_camera* cam, const rtr_camera* prev, int have,
                             const rtr_temporal_params* tp, const double* h_color, const double* h_q,
                             const int32_t* h_count, const double* h_feat, const double* h_hist_in,
                             double* h_c, double* h_var, double* h_hist_out);

/* ---- the accumulator kernels (csrc/rt_accum_kernels.h) on synthetic tile state ----
 *
 * rtr_test_accum_load puts caller-given state into an accumulator of the product, so that its own binaries --
 * k_accum_errors behind rtr_accum_errors, k_accum_resolve and the host scatter loops behind rtr_accum_resolve / _moments,
 * k_accum_resolve_scatter behind rtr_accum_resolve_device, and k_accum_plan / k_accum_commit inside rtr_accum_refine -- run
 * on sums, moments and counts no render produces:
 *   sum    [n][3][256] doubles: per owned tile (order of rtr_accum_tiles) the three channel planes, lane = 16 * row + column
 *          of the tile, row 0 its lowest; EVERY lane is given, those outside the region included
 *   q      [n][256] doubles, same lanes; required exactly when the accumulator keeps moments (else NULL)
 *   count  [n] ints >= 0
 *   n      the number of owned tiles
 * Waits for the context's stream, copies, and sets the library's host copy of the counts; runs no kernel.  The state is
 * what the next rtr_accum_* call sees; a pass continues the loaded sums.  RTR_ERR_INVALID, before any device work, for a
 * NULL array, a wrong n, a negative count, or a q that does not match the moments flag. */
int rtr_test_accum_load(rtr_context* ctx, rtr_accum* acc, const double* sum, const double* q, const int32_t* count, int64_t n);

/* k_accum_plan alone, launched as a pass launches it (one workgroup of 1024 threads), over HOST arrays of n tiles:
 * count[n], err[n] (read in mode 2 only) and tile_s1[n] (in: the targets of mode 0; out: the targets of every mode).
 * mode 0: targets as given; 1: max(count, spp); 2: the refinement rule of rtr_accum_refine with spp_min, spp_max and
 * threshold.  active[n] receives the list of the slots with target > count -- its first *n_active entries, the most
 * pending samples first by floor(log2(target - count)), any order inside such a bucket; the entry fills the list with -1
 * before the launch, so the entries from *n_active on read -1.  Nothing is rendered: counts and targets may be as large
 * as INT32_MAX.  Needs no scene.  Blocking.  RTR_ERR_INVALID for a NULL pointer, n < 1 or an unknown mode. */
int rtr_test_accum_plan(rtr_context* ctx, int64_t n, int32_t mode, int32_t spp, int32_t spp_min, int32_t spp_max,
                        double threshold, const int32_t* count, const double* err, int32_t* tile_s1, int32_t* active,
                        int32_t* n_active);

/* k_accum_commit alone, one workgroup per tile as behind a pass, over HOST arrays of n tiles: workgroup b < n_active takes
 * the slot active[b] and, where done[slot] is nonzero, copies partial[slot] ([n][3][256]) into sum, q_part[slot] ([n][256])
 * into q and tile_s1[slot] into count[slot]; every other slot of sum, q and count keeps every byte.  q and q_part are both
 * NULL (an accumulator without moments) or both given.  Needs no scene.  Blocking.  RTR_ERR_INVALID for a NULL pointer,
 * n < 1, n_active outside [0, n] or an entry of active[0 .. n) outside [0, n). */
int rtr_test_accum_commit(rtr_context* ctx, int64_t n, const int32_t* active, int32_t n_active, const int32_t* done,
                          const int32_t* tile_s1, const double* partial, const double* q_part, double* sum, double* q,
                          int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* RTR_HIP_TEST_H */
