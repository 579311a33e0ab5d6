/*
 * rt_test_kernels.h -- device unit kernels of librtr_hip_test.so (include/rtr_hip_test.h): the library's own device
 * functions (rt_device.h) over golden-vector records, one lane per record, plus counter-calibration and
 * instruction-level checks.  Test infrastructure: nothing of this is linked into librtr_hip.so.
 */
#pragma once

#include "rt_kernels.h"
#include "rtr_hip_test.h" /* rtr_pair_record */
#include "rtr_testrec.h"

/* ---- device unit kernels over golden-vector records ---------------------------------------- */
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_hits(const DScene sc, rtr_hit_record* recs, long long n) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_hit_record r = recs[k];
    uint32_t rng = r.rng_in;
    Hit rec;
    rec.u = rec.v = __builtin_nan("");
    rec.mat = -1;
    rec.t = 0, rec.p = mk(0, 0, 0), rec.n = mk(0, 0, 0), rec.front = false;
    Real tmax = r.t_max;
    bool h;
    if (TRAV == RT_TRAV_FAST || TRAV == RT_TRAV_TOP) {
        int ref, inst;
        h = trace_fast<false, true, false, TRAV == RT_TRAV_TOP>(sc, sub_scene0(sc), ld3(r.o), ld3(r.d), r.time, r.t_min, tmax, ref, inst, st, 0);
        if (h) fast_finish<true>(sc, ld3(r.o), ld3(r.d), r.time, tmax, ref, inst, rec);
    } else if (rt_is_program(TRAV)) {
        h = cast_closest<TRAV>(sc, ld3(r.o), ld3(r.d), r.time, rec, rng, st, r.t_min, tmax);
    } else {
        h = traverse<true, TRAV == RT_TRAV_MEDIA>(sc, sc.root, ld3(r.o), ld3(r.d), r.time, r.t_min, tmax, rec, rng, st, 0);
    }
    r.rng_out = rng;
    r.hit = h;
    r.front_face = h ? (int)rec.front : 0;
    r.material = h ? rec.mat : -1;
    r.pad = 0;
    r.t = h ? rec.t : 0;
    r.p[0] = h ? rec.p.x : 0, r.p[1] = h ? rec.p.y : 0, r.p[2] = h ? rec.p.z : 0;
    r.n[0] = h ? rec.n.x : 0, r.n[1] = h ? rec.n.y : 0, r.n[2] = h ? rec.n.z : 0;
    r.u = h ? rec.u : 0, r.v = h ? rec.v : 0;
    recs[k] = r;
}

/* the closest-hit cast of the flat kernels, cast_closest<RT_TRAV_FLAT / RT_TRAV_FLAT_GUARD>: the flat scan and the hit record
 * from the scene's finish records (fast_finish_flat), or from FInst + fprim where it has none */
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_flat_hits(const DScene sc, rtr_hit_record* recs, long long n) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_hit_record r = recs[k];
    uint32_t rng = r.rng_in;
    Hit rec;
    rec.u = rec.v = __builtin_nan("");
    rec.mat = -1;
    rec.t = 0, rec.p = mk(0, 0, 0), rec.n = mk(0, 0, 0), rec.front = false;
    const bool h = cast_closest<TRAV>(sc, ld3(r.o), ld3(r.d), r.time, rec, rng, st, r.t_min, r.t_max);
    r.rng_out = rng;
    r.hit = h;
    r.front_face = h ? (int)rec.front : 0;
    r.material = h ? rec.mat : -1;
    r.pad = 0;
    r.t = h ? rec.t : 0;
    r.p[0] = h ? rec.p.x : 0, r.p[1] = h ? rec.p.y : 0, r.p[2] = h ? rec.p.z : 0;
    r.n[0] = h ? rec.n.x : 0, r.n[1] = h ? rec.n.y : 0, r.n[2] = h ? rec.n.z : 0;
    r.u = h ? rec.u : 0, r.v = h ? rec.v : 0;
    recs[k] = r;
}

/* trace_pair on one ray pair per lane, and the single casts of the flat kernels (cast_closest / cast_any<RT_TRAV_FLAT>'s
 * trace_fast instantiations) for the same lanes.  RECAST: which of the product's two texts runs -- true: the lean kernels'
 * (trace_pair_recast + pair_recast), false: the per-frame fallback of every other pair-cast kernel (trace_pair_frames) */
template <bool RECAST>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_pair(const DScene sc, rtr_pair_record* recs, long long n) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_pair_record r = recs[k];
    Real a_t = r.a_tmax, b_t = r.b_tmax;
    int a_ref, a_inst, b_ref;
    r.recasts = 0, r.pad = 0;
    if (!trace_pair<RECAST>(sc, ld3(r.ao), ld3(r.ad), 0.0, a_t, a_ref, a_inst, ld3(r.bo), ld3(r.bd), b_t, b_ref, st)) {
        a_t = r.a_tmax, b_t = r.b_tmax;
        pair_recast(sc, ld3(r.ao), ld3(r.ad), 0.0, a_t, a_ref, a_inst, ld3(r.bo), ld3(r.bd), b_t, b_ref, st);
        r.recasts = 1;
    }
    Real s_t = r.a_tmax, sb_t = r.b_tmax;
    int s_ref, s_inst, sb_ref, sb_inst;
    trace_fast<false, false, false, false, false>(sc, sub_scene0(sc), ld3(r.ao), ld3(r.ad), 0.0, 0.001, s_t, s_ref, s_inst, st, 0);
    trace_fast<true, false, true, false, false>(sc, sub_scene0(sc), ld3(r.bo), ld3(r.bd), 0.0, 0.001, sb_t, sb_ref, sb_inst, st, 0);
    r.a_t = a_t, r.s_a_t = s_t;
    r.a_ref = a_ref, r.a_inst = a_inst, r.b_hit = b_ref >= 0;
    r.s_a_ref = s_ref, r.s_a_inst = s_inst, r.s_b_hit = sb_ref >= 0;
    recs[k] = r;
}

/* rtr_test_pair_resident: k_mega_queue's steps around its pair cast, `casts` times (wave-uniform) -- the request read from
 * its parked words and `so`, the cast, the recast with pair_retire where a vote failed, the request marked dead */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_pair_resident(const DScene sc, rtr_pair_record* recs, long long n,
                                                                  const int stack_words, const int casts) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const Park pk{reinterpret_cast<double*>(lds_stack + stack_words * RTR_BLOCK) + threadIdx.x};
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_pair_record r = recs[k];
    const V3 ao = ld3(r.ao), ad = ld3(r.ad);
    V3 so = ld3(r.bo);
    pk.set3(PK_SWI, ld3(r.bd));
    pk.set(PK_STMAX, r.b_tmax);
    r.recasts = 0, r.pad = 0;
    for (int c = 0; c < casts; ++c) {
        Real a_t = r.a_tmax;
        int a_ref, a_inst, b_ref;
        const V3 swi = pk.get3(PK_SWI);
        Real b_t = pk.get(PK_STMAX);
        if (!trace_pair(sc, ao, ad, 0.0, a_t, a_ref, a_inst, so, swi, b_t, b_ref, st)) {
            a_t = r.a_tmax;
            b_t = pk.get(PK_STMAX);
            pair_recast(sc, ao, ad, 0.0, a_t, a_ref, a_inst, so, swi, b_t, b_ref, st);
            pair_retire(pk, so);
            ++r.recasts;
        }
        pk.set(PK_STMAX, 0.0);
        if (c == 0) {
            r.a_t = a_t;
            r.a_ref = a_ref, r.a_inst = a_inst, r.b_hit = b_ref >= 0;
        }
    }
    Real s_t = r.a_tmax, sb_t = r.b_tmax;
    int s_ref, s_inst, sb_ref, sb_inst;
    trace_fast<false, false, false, false, false>(sc, sub_scene0(sc), ao, ad, 0.0, 0.001, s_t, s_ref, s_inst, st, 0);
    trace_fast<true, false, true, false, false>(sc, sub_scene0(sc), ld3(r.bo), ld3(r.bd), 0.0, 0.001, sb_t, sb_ref, sb_inst, st, 0);
    r.s_a_t = s_t;
    r.s_a_ref = s_ref, r.s_a_inst = s_inst, r.s_b_hit = sb_ref >= 0;
    recs[k] = r;
}

/* equal in every bit, a NaN equal to a NaN of any payload */
RT_DEV bool same_bits(Real a, Real b) { return (a != a && b != b) || __double_as_longlong(a) == __double_as_longlong(b); }

/* mat_prepare + mat_sample / mat_eval / mat_pdf / mat_emitted of the MS instantiation, and the fused mat_eval_pdf the MIS
 * kernels call for the light sample: pad bit 0 = its f differs from mat_eval, bit 1 = its pdf differs from mat_pdf */
template <int MS>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_materials(const DScene sc, rtr_mat_record* recs, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_mat_record r = recs[k];
    Hit rec;
    rec.p = ld3(r.p), rec.n = ld3(r.n);
    rec.u = r.u, rec.v = r.v, rec.t = 1.0;
    rec.front = r.front_face != 0;
    rec.mat = r.material;
    const V3 wo = ld3(r.wo), wi = ld3(r.wi_in);
    uint32_t rng = r.rng_in;
    BSDFSample bs;
    bs.wi = mk(0, 0, 0), bs.f = mk(0, 0, 0), bs.pdf = 0, bs.is_specular = false, bs.is_transmission = false;
    const MatCtx mc = mat_prepare<MS>(sc, rec);
    const UDiv pi = scene_pi(sc);
    const bool ok = mat_sample<MS>(mc, rec, wo, bs, rng, pi);
    r.rng_out = rng;
    r.sample_ok = ok, r.is_specular = bs.is_specular;
    r.is_transmission = bs.is_transmission;
    r.s_wi[0] = bs.wi.x, r.s_wi[1] = bs.wi.y, r.s_wi[2] = bs.wi.z;
    r.s_f[0] = bs.f.x, r.s_f[1] = bs.f.y, r.s_f[2] = bs.f.z;
    r.s_pdf = bs.pdf;
    const V3 e = mat_eval<MS>(mc, wo, wi);
    r.eval[0] = e.x, r.eval[1] = e.y, r.eval[2] = e.z;
    r.pdf = mat_pdf<MS>(mc, rec, wo, wi, pi);
    const V3 em = mat_emitted(mc, rec);
    r.emitted[0] = em.x, r.emitted[1] = em.y, r.emitted[2] = em.z;
    V3 f2;
    Real pdf2;
    mat_eval_pdf<MS>(mc, rec, wo, wi, f2, pdf2, pi);
    r.pad = (same_bits(f2.x, e.x) && same_bits(f2.y, e.y) && same_bits(f2.z, e.z) ? 0 : 1) | (same_bits(pdf2, r.pdf) ? 0 : 2);
    recs[k] = r;
}

/* mat_prepare + the legacy mat_scatter with rd = wo: sample_ok the return value, s_wi the new direction, s_f the attenuation */
template <int MS>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_scatter(const DScene sc, rtr_mat_record* recs, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_mat_record r = recs[k];
    Hit rec;
    rec.p = ld3(r.p), rec.n = ld3(r.n);
    rec.u = r.u, rec.v = r.v, rec.t = 1.0;
    rec.front = r.front_face != 0;
    rec.mat = r.material;
    uint32_t rng = r.rng_in;
    V3 attenuation = mk(0, 0, 0), dir = mk(0, 0, 0);
    const MatCtx mc = mat_prepare<MS>(sc, rec);
    const bool ok = mat_scatter<MS>(mc, ld3(r.wo), rec, attenuation, dir, rng);
    r.rng_out = rng;
    r.sample_ok = ok, r.is_specular = 0, r.is_transmission = 0, r.pad = 0;
    r.s_wi[0] = dir.x, r.s_wi[1] = dir.y, r.s_wi[2] = dir.z;
    r.s_f[0] = attenuation.x, r.s_f[1] = attenuation.y, r.s_f[2] = attenuation.z;
    r.s_pdf = 0, r.pdf = 0;
    r.eval[0] = r.eval[1] = r.eval[2] = 0;
    r.emitted[0] = r.emitted[1] = r.emitted[2] = 0;
    recs[k] = r;
}

template <int MS>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_lights(const DScene sc, rtr_light_record* recs, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    rtr_light_record r = recs[k];
    const rtr_light l = ld_const(sc.lights, r.light);
    uint32_t rng = 0x2545F491u; /* the uniform environment light draws its direction itself */
    LightSample s = light_sample<MS>(l, ld3(r.p), r.u[0], r.u[1], rng, sc.image_bytes);
    r.Li[0] = s.Li.x, r.Li[1] = s.Li.y, r.Li[2] = s.Li.z;
    r.wi[0] = s.wi.x, r.wi[1] = s.wi.y, r.wi[2] = s.wi.z;
    r.pdf = s.pdf, r.dist = s.dist, r.is_delta = s.is_delta, r.pad2 = 0;
    r.pdf_dir = light_pdf<MS>(l, scene_light_consts(sc, r.light), ld3(r.p), ld3(r.dir), RT_LANE_MS(MS) ? len<true>(ld3(r.dir)) : 0.0, sc.image_bytes);
    recs[k] = r;
}

/* rtr_test_udiv: udiv() beside the compiler's n / d, every numerator against every divisor; the divisor's record is
 * made as the kernels make theirs (udiv_make).  out[0] += quotients that differ in any bit (a NaN equals a NaN), out[1] += pairs compared */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_udiv(const double* __restrict__ num, long long n, const double* __restrict__ div,
                                                         int m, unsigned long long* out) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    unsigned long long bad = 0, tested = 0;
    if (k < n) {
        const double x = num[k];
        for (int j = 0; j < m; ++j) { /* wave-uniform divisor: `safe` is a scalar branch, as in the renders */
            const double d = as_const(div)[j];
            const UDiv u = udiv_make(d);
            const double ref = x / d;
            bad += !same_bits(udiv(x, u), ref);
            if (__builtin_fabs(x) <= 0x1p200) bad += !same_bits(udiv<true>(x, u), ref);
            ++tested;
        }
    }
    bad = wave_sum(bad);
    tested = wave_sum(tested);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
}

/* rtr_test_rcp_lane / rtr_test_sqrt_lane: the wave-voted short forms of rt_device.h beside the compiler's 1.0 / d and
 * __builtin_sqrt(x), bit for bit (NaN payloads too).
 * The edge values every wave class gets: each window bound of the short forms (and 2^-300, 2^200), the smallest normal
 * number and the exponent of the largest, each with the value one ulp below and above it; zero, denormals, infinity, NaNs
 * (quiet, with a payload, signalling), the largest finite number and 1 -- all of them with both signs. */
#define RT_LANE_SPECIALS 68
RT_HD unsigned long long lane_special(unsigned k) {
    const unsigned long long sign = (unsigned long long)(k & 1) << 63;
    k >>= 1;
    if (k < 24) {
        const int e[8] = {-1022, -767, -300, -200, -100, 100, 200, 1023};
        return sign | ((((unsigned long long)(1023 + e[k / 3])) << 52) + (k % 3) - 1);
    }
    const unsigned long long other[10] = {0ull, 1ull, 0x0008000000000000ull, 1ull << 44, 0x7ff0000000000000ull, 0x7ff8000000000000ull,
                                          0x7ff8000000001234ull, 0x7ff0000000000001ull, 0x7fefffffffffffffull, 0x3ff0000000000000ull};
    return sign | other[(k - 24) % 10];
}
RT_DEV unsigned long long lane_mix(unsigned long long z) { /* splitmix64's finaliser */
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* OP 0: rcp_lane in its two windows (either sign; positive divisors only, the callers'), 1: sqrt_lane and sqrt_rcp_lane.
 * Operand set g of gridDim.x * RTR_BLOCK * per_thread comes from the counter alone: a random mantissa (OP 0: and sign) under
 * every exponent of the accepted window in turn, lane after lane, so a wave of such sets votes for the short form.  Every
 * fourth wave gets one edge value: in lane (w / 4) % 64, value (w / 256) % 68, so every value meets every lane position,
 * and waves that vote for the plain form carry 63 lanes in range through it.
 * out[0] += sets with a result that differs, out[1] += sets compared, out[2]: a mismatch was recorded in out[3..6] =
 * operand, 0, result, expected (bits), out[7] += sets whose wave had every lane inside the form's widest window. */
template <int OP>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_lane(unsigned long long* out, unsigned per_thread) {
    const unsigned long long threads = (unsigned long long)gridDim.x * RTR_BLOCK, tid = (unsigned long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    unsigned long long bad = 0, tested = 0, in_short = 0;
    for (unsigned it = 0; it < per_thread; ++it) {
        const unsigned long long g = (unsigned long long)it * threads + tid, w = g >> 6;
        const unsigned long long h = lane_mix(g);
        const int e = OP == 1 ? -767 + (int)(g % 1791) : -100 + (int)(g % 200);
        Real a = __longlong_as_double((long long)((h & (OP == 1 ? 0x000FFFFFFFFFFFFFull : 0x800FFFFFFFFFFFFFull)) |
                                                  ((unsigned long long)(1023 + e) << 52)));
        if ((w & 3) == 3 && (g & 63) == ((w >> 2) & 63)) a = __longlong_as_double((long long)lane_special((unsigned)(w >> 8) % RT_LANE_SPECIALS));
        Real got, want;
        bool differs = false, all_in;
        auto check = [&](Real g_, Real w_) {
            if (!differs && __double_as_longlong(g_) != __double_as_longlong(w_)) differs = true, got = g_, want = w_;
        };
        if (OP == 0) {
            all_in = __all(lane_window<-100, 100>(a));
            check(rcp_lane(a), 1.0 / a);
            check(rcp_lane<1>(a), 1.0 / a);
            check(rcp_lane<1>(__builtin_fabs(a)), 1.0 / __builtin_fabs(a));
        } else {
            all_in = __all(RT_SQRT_WINDOW(a));
            const Real s = __builtin_sqrt(a);
            check(sqrt_lane(a), s);
            Real root;
            const Real r = sqrt_rcp_lane(a, root);
            check(root, s);
            check(r, 1.0 / s);
        }
        if (differs && atomicCAS(out + 2, 0ull, 1ull) == 0ull) {
            out[3] = (unsigned long long)__double_as_longlong(a), out[4] = 0;
            out[5] = (unsigned long long)__double_as_longlong(got), out[6] = (unsigned long long)__double_as_longlong(want);
        }
        bad += differs, in_short += all_in, ++tested;
    }
    bad = wave_sum(bad), tested = wave_sum(tested), in_short = wave_sum(in_short);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
    if ((threadIdx.x & 63) == 0 && in_short) atomicAdd(out + 7, in_short);
}

/* rtr_test_scene_consts: a second evaluation of the scene table (scene_consts_fill) into the test buffer */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_scene_consts(const DScene sc, SceneConsts* out) {
    for (int k = threadIdx.x; k < (sc.n_lights > 1 ? sc.n_lights : 1); k += RTR_BLOCK)
        scene_consts_fill(sc.lights, sc.n_lights, out, k);
}

/* rtr_test_pow5: pow5 of rt_device.h, one value per lane */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_pow5(const double* __restrict__ x, double* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k < n) out[k] = pow5(x[k]);
}

/* rtr_test_stream8: 8 bytes per lane in, 8 bytes per lane out */
/* out[0] += angles whose sincos differs from sin, cos; out[1] += angles tested */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_sincos(unsigned long long* out) {
    unsigned long long bad = 0, tested = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * RTR_BLOCK;
    for (unsigned long long s = (unsigned long long)blockIdx.x * RTR_BLOCK + threadIdx.x; s < (1ull << 32); s += stride) {
        const Real phi = 2.0 * RT_PI * ((uint32_t)s * 2.3283064365386963e-10); /* as random_cosine_direction / pbr_sample */
        Real s2, c2;
        sincos(phi, &s2, &c2);
        const Real s1 = sin(phi), c1 = cos(phi);
        bad += (__double_as_longlong(s1) != __double_as_longlong(s2)) | (__double_as_longlong(c1) != __double_as_longlong(c2));
        ++tested;
    }
    bad = wave_sum(bad);
    tested = wave_sum(tested);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
}

/* rtr_test_draw_forms: the joined form of a draw in (-1, 1) (rt_device.h: draw_sym_join, with its own high word and with
 * the one from rng_hi(), as the rejection loops hold it) beside the plain text, for all 2^32 states.
 * out[0] += states where it differs in any bit; out[1] += states tested; out[2]: one such state + 1 */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_draw_forms(unsigned long long* out) {
    unsigned long long bad = 0, tested = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * RTR_BLOCK;
    const uint32_t hi = rng_hi();
    for (unsigned long long k = (unsigned long long)blockIdx.x * RTR_BLOCK + threadIdx.x; k < (1ull << 32); k += stride) {
        const uint32_t s = (uint32_t)k;
        const bool differs = (__double_as_longlong(draw_sym_join(s)) != __double_as_longlong(draw_sym_plain(s))) |
                             (__double_as_longlong(draw_sym_join(s, hi)) != __double_as_longlong(draw_sym_plain(s)));
        if (differs) out[2] = k + 1;
        bad += differs;
        ++tested;
    }
    bad = wave_sum(bad);
    tested = wave_sum(tested);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
}

/* rtr_test_draw_callers: the functions that draw, with the joined form (JOIN) and in the plain text (this library's second
 * instantiation), lane by lane from the same seeded state: random_in_unit_sphere, random_in_unit_disk,
 * random_cosine_direction, rng_range(0.25, 7.5), rng_int(0, 6), in that order, the state carried from call to call (the
 * last three draw through rng_next, which has one form).
 * out[0] += lanes with an output bit or an exit state that differs; out[1] += lanes tested; out[2]: one such lane's seed
 * state */
#define RT_DRAW_WORDS 11
template <bool JOIN>
RT_DEV void draw_callers(uint32_t& s, long long* w, uint32_t* exits) {
    V3 p = random_in_unit_sphere<JOIN>(s);
    w[0] = __double_as_longlong(p.x), w[1] = __double_as_longlong(p.y), w[2] = __double_as_longlong(p.z), exits[0] = s;
    p = random_in_unit_disk<JOIN>(s);
    w[3] = __double_as_longlong(p.x), w[4] = __double_as_longlong(p.y), w[5] = __double_as_longlong(p.z), exits[1] = s;
    p = random_cosine_direction(s);
    w[6] = __double_as_longlong(p.x), w[7] = __double_as_longlong(p.y), w[8] = __double_as_longlong(p.z), exits[2] = s;
    w[9] = __double_as_longlong(rng_range(s, 0.25, 7.5)), exits[3] = s;
    w[10] = rng_int(s, 0, 6), exits[4] = s;
}
__global__ void __launch_bounds__(RTR_BLOCK) k_test_draw_callers(unsigned long long* out, unsigned long long seed, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    unsigned long long bad = 0, tested = 0;
    if (k < n) {
        uint32_t s0 = (uint32_t)lane_mix(seed + (unsigned long long)k);
        if (s0 == 0) s0 = 0x2545F491u; /* xorshift32 has no state 0 */
        uint32_t a = s0, b = s0, ea[5], eb[5];
        long long wa[RT_DRAW_WORDS], wb[RT_DRAW_WORDS];
        draw_callers<true>(a, wa, ea);
        draw_callers<false>(b, wb, eb);
        bool differs = false;
        for (int j = 0; j < RT_DRAW_WORDS; ++j) differs |= wa[j] != wb[j];
        for (int j = 0; j < 5; ++j) differs |= ea[j] != eb[j];
        if (differs) out[2] = s0;
        bad = differs, tested = 1;
    }
    bad = wave_sum(bad), tested = wave_sum(tested);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
}

/* rtr_test_shared_division: div_shared() against the compiler's n / d on 2^32 operand pairs.  Three quarters of them
 * take both operands from the whole range the short form is used in (|d| in [2^-100, 2^100), |n| in [2^-300, 2^200),
 * random mantissas and signs); the rest are shaped like the rectangle test's (k - o) / d: a difference of two
 * coordinates below 1000 over a direction component in (-1, 1), small values of both included.  Quotients of
 * numerators below 2^-300 are only required to stay below 2^-200 (see div_shared). */
/* out[0] += quotients that differ; out[1] += operand pairs tested */
__global__ void __launch_bounds__(RTR_BLOCK) k_test_shared_div(unsigned long long* out, unsigned per_thread) {
    unsigned long long x = 0x9E3779B97F4A7C15ull * ((unsigned long long)blockIdx.x * RTR_BLOCK + threadIdx.x + 1);
    auto next = [&]() {
        x ^= x >> 12, x ^= x << 25, x ^= x >> 27;
        return x * 0x2545F4914F6CDD1Dull;
    };
    auto make = [&](int emin, int espan) { /* +-1.m * 2^e, e in [emin, emin + espan) */
        const unsigned long long u = next();
        const int e = emin + (int)((u >> 52) % (unsigned)espan);
        const double m = __longlong_as_double((u & 0x800FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
        return ldexp(m, e);
    };
    unsigned long long bad = 0, tested = 0;
    for (unsigned k = 0; k < per_thread; ++k) {
        double n, d;
        if (k & 3) {
            d = make(-100, 200), n = make(-300, 500);
        } else {
            const double o = (double)(long long)(next() >> 11) * 0x1p-53 * 2000.0 - 1000.0;
            const double p = (k & 4) ? o + make(-60, 60) : (double)(long long)(next() >> 11) * 0x1p-53 * 2000.0 - 1000.0;
            n = p - o;
            d = (k & 8) ? make(-40, 40) : (double)(long long)(next() >> 11) * 0x1p-52 - 1.0;
        }
        if (!rcp_safe(d)) continue;
        const double r = rcp_refined(d);
        const double t = div_shared<true>(n, d, r, false), ref = n / d;
        if (__builtin_fabs(n) >= 0x1p-300)
            bad += __double_as_longlong(t) != __double_as_longlong(ref);
        else
            bad += !(__builtin_fabs(t) < 0x1p-200) || !(__builtin_fabs(ref) < 0x1p-200);
        const double g = div_shared<true>(n, d, r, true); /* guarded: every numerator */
        bad += __double_as_longlong(g) != __double_as_longlong(ref);
        ++tested;
    }
    bad = wave_sum(bad);
    tested = wave_sum(tested);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(out, bad);
    if ((threadIdx.x & 63) == 0 && tested) atomicAdd(out + 1, tested);
}

/* rtr_test_issue_rates: shader cycles per wave-instruction, one instruction class per launch.  Every wave runs
 * `iters` trips of 32 independent instructions of the class between two s_memtime reads; with four waves on each SIMD
 * (grid = 4 workgroups per CU) the quotient cycles x 1 / (32 iters) of a wave is four times the SIMD's cost per
 * instruction when the class is bound by its pipe, and the single-wave issue cost when it is not.  out[0] += cycles of
 * every wave, out[1] += waves. */
#define RT_REP32(S) S S S S S S S S S S S S S S S S S S S S S S S S S S S S S S S S
template <int KIND>
__global__ void __launch_bounds__(RTR_BLOCK) k_test_issue_rate(unsigned long long* out, int iters, double seed) {
    double a = seed + threadIdx.x, b = seed * 0.5, c = 1.0 / (seed + 3.0), d = seed;
    float fa = (float)a, fb = (float)b, fc = (float)c;
    int ia = threadIdx.x, ib = 3, ic = 0;
    unsigned long long m = 0;
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; ++i) {
        if (KIND == 0) asm volatile(RT_REP32("v_fma_f64 %0, %1, %2, %1\n") : "+v"(d) : "v"(b), "v"(c));
        if (KIND == 1) asm volatile(RT_REP32("v_add_f64 %0, %1, %2\n") : "+v"(d) : "v"(b), "v"(c));
        if (KIND == 2) asm volatile(RT_REP32("v_mul_f64 %0, %1, %2\n") : "+v"(d) : "v"(b), "v"(c));
        if (KIND == 3) asm volatile(RT_REP32("v_rcp_f64 %0, %1\n") : "+v"(d) : "v"(b));
        if (KIND == 4) asm volatile(RT_REP32("v_rsq_f64 %0, %1\n") : "+v"(d) : "v"(b));
        if (KIND == 5) asm volatile(RT_REP32("v_cmp_lt_f64 %0, %1, %2\n") : "=s"(m) : "v"(b), "v"(c));
        if (KIND == 6) asm volatile(RT_REP32("v_cndmask_b32 %0, %1, %2, vcc\n") : "=v"(ic) : "v"(ib), "v"(ia) : "vcc");
        if (KIND == 7) asm volatile(RT_REP32("v_mov_b32 %0, %1\n") : "+v"(ia) : "v"(ib));
        if (KIND == 8) asm volatile(RT_REP32("v_fma_f32 %0, %1, %2, %1\n") : "+v"(fa) : "v"(fb), "v"(fc));
        if (KIND == 9) asm volatile(RT_REP32("s_and_b64 %0, %0, exec\n") : "+s"(m) : : "scc");
        if (KIND == 10) asm volatile(RT_REP32("v_div_scale_f64 %0, vcc, %1, %2, %1\n") : "+v"(d) : "v"(b), "v"(c) : "vcc");
        if (KIND == 11) asm volatile(RT_REP32("v_div_fixup_f64 %0, %1, %2, %1\n") : "+v"(d) : "v"(b), "v"(c));
        if (KIND == 13) asm volatile(RT_REP32("v_cndmask_b32_e64 %0, %1, %2, %3\n") : "=v"(ic) : "v"(ib), "v"(ia), "s"(m));
        if (KIND == 14) asm volatile(RT_REP32("v_min_f32 %0, %1, %2\n") : "=v"(fa) : "v"(fb), "v"(fc));
        if (KIND == 15) asm volatile(RT_REP32("v_cmp_lt_f32 vcc, %1, %2\nv_cndmask_b32 %0, %1, %2, vcc\n") : "=v"(fa) : "v"(fb), "v"(fc) : "vcc");
        if (KIND == 16) { int i0, i1, i2, i3; asm volatile(RT_REP32("v_cndmask_b32 %0, %4, %5, vcc\nv_cndmask_b32 %1, %4, %5, vcc\nv_cndmask_b32 %2, %4, %5, vcc\nv_cndmask_b32 %3, %4, %5, vcc\n") : "=v"(i0), "=v"(i1), "=v"(i2), "=v"(i3) : "v"(ib), "v"(ia) : "vcc"); ic = i0 + i1 + i2 + i3; }
        if (KIND == 17) asm volatile(RT_REP32("v_cmp_lt_f64 vcc, %1, %2\nv_cndmask_b32 %0, %3, %4, vcc\n") : "=v"(ic) : "v"(b), "v"(c), "v"(ib), "v"(ia) : "vcc");
        if (KIND == 12) /* the rectangle test's mix: one compare into a scalar pair and the scalar AND that uses it */
            asm volatile(RT_REP32("v_cmp_lt_f64 %0, %1, %2\ns_and_b64 %0, %0, exec\n") : "=s"(m) : "v"(b), "v"(c) : "scc");
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    if (d == 12345.678 || fa == 1.5f || ia == -77 || ic == -78 || m == 0x1234567ull) out[2] = 1; /* keep the results alive */
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], t1 - t0);
        atomicAdd(&out[1], 1ull);
    }
}

__global__ void __launch_bounds__(RTR_BLOCK) k_stream8(const double* __restrict__ in, double* __restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * RTR_BLOCK)
        out[i] = in[i] + 1.0;
}
