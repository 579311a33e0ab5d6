/*
 * rtr_cube.hip -- filtered cube maps (include/rtr_hip.h: rtr_cube_filter*, rtr_cube_chain_*): the parameter and chain checks,
 * the split of a filter call into launches of bounded work, the two kernels of rt_cube.h and their launches, the entries,
 * and the host-only pieces that need no context (rtr_cube_filter_defaults, rtr_cube_filter_one, rtr_cube_chain_plan,
 * rtr_cube_chain_lookup_one), and the lookup of a capture set (rtr_capture_set_lookup*: the set's rules and arithmetic are
 * rt_render.h's, the kernel rt_cube.h's).  The entries' common checks, the staging of the host entries, the body of the device
 * entries, the chunked launcher of the chain lookup and the cap hook are rt_batch.h's, shared with the other batch units.
 */
#include "rt_batch.h"
#include "rt_cube.h"

using namespace rtr;

namespace {

constexpr int64_t kCubeSlice = (int64_t)1 << 20; /* output records (queries of a lookup) per slice of the host entries */
/* (output, source) pairs per launch at most (RTR_FILTER_PAIRS, a test hook, lowers it): DESIGN.md 4.11 has the measured
 * time of a launch of this size */
constexpr long long kFilterPairs = 1ll << 35;
#ifndef RTR_FILTER_WIDE
#define RTR_FILTER_WIDE 4 /* output texels per wave of the wide kernel; the narrow one has 1 (experiments: -DRTR_FILTER_WIDE=n) */
#endif
constexpr int kFilterWide = RTR_FILTER_WIDE;

long long face_records(int S) { return 6ll * S * S; }

/* what both filter entries check before any device work: context, params, n / NULL; no scene is needed */
int filter_check(rtr_context* c, const rtr_cube_filter_params* fp, const void* texels, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = cube_filter_params_why(fp)) return fail(c, RTR_ERR_INVALID, std::string("rtr_cube_filter: ") + why);
    return batch_check(c, "rtr_cube_filter", n, texels && out);
}

/* the output records [o0, o1) of the call (numbered cube * Fout + e) into d_out, whose record 0 is o0.  No launch holds
 * more than that many pairs: whole cubes side by side while they fit, else one cube's texels in runs.  A launch
 * with few workgroups takes the kernel with one output texel per wave, which spreads it over four times as many */
int filter_launch(rtr_context* c, const rtr_cube_filter_params* fp, const rtr_gather_out* d_texels, rtr_gather_out* d_out,
                  long long o0, long long o1) {
    FilterK K{};
    K.texels = d_texels, K.out = d_out, K.out_first = o0;
    K.Sin = fp->face_in, K.SSin = K.Sin * K.Sin, K.Fin = 6 * K.SSin;
    K.Sout = fp->face_out, K.SSout = K.Sout * K.Sout, K.Fout = 6 * K.SSout;
    K.a2m1 = fp->alpha * fp->alpha - 1.0, K.cos_cut = fp->cos_cut;
    const long long per_launch = std::max(1ll, env_cap("RTR_FILTER_PAIRS", kFilterPairs) / K.Fin); /* output texels */
    for (long long o = o0; o < o1;) {
        const long long cube = o / K.Fout;
        const int e = (int)(o - cube * K.Fout);
        long long cubes = 1;
        K.cube0 = cube, K.e0 = e;
        if (e == 0 && o1 - o >= K.Fout && per_launch >= K.Fout) {
            cubes = std::min(std::min((o1 - o) / K.Fout, per_launch / K.Fout), 65535ll);
            K.e1 = K.Fout;
        } else {
            K.e1 = (int)std::min<long long>(K.Fout, e + std::min(per_launch, o1 - o));
        }
        const int texels = K.e1 - K.e0, per_wg = kFilterWide * (RTR_BLOCK / 64);
        const bool wide = (long long)((texels + per_wg - 1) / per_wg) * cubes >= 1024;
        if (wide)
            hipLaunchKernelGGL(k_cube_filter<kFilterWide>, dim3((unsigned)((texels + per_wg - 1) / per_wg), (unsigned)cubes),
                               dim3(RTR_BLOCK), 0, c->stream, K);
        else
            hipLaunchKernelGGL(k_cube_filter<1>, dim3((unsigned)((texels + RTR_BLOCK / 64 - 1) / (RTR_BLOCK / 64)), (unsigned)cubes),
                               dim3(RTR_BLOCK), 0, c->stream, K);
        o += cubes * (long long)texels;
    }
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("cube filter launch: ") + hipGetErrorString(err));
}

/* what both chain lookups check before any device work: context, chain, n / NULL; no scene is needed */
int chain_check(rtr_context* c, const rtr_cube_level* lv, int32_t n_levels, const void* texels, int64_t n_records, const void* q,
                const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (n_records < 0) return fail(c, RTR_ERR_INVALID, "rtr_cube_chain_lookup: negative n_records");
    if (const char* why = cube_chain_why(lv, n_levels, n_records))
        return fail(c, RTR_ERR_INVALID, std::string("rtr_cube_chain_lookup: ") + why);
    return batch_check(c, "rtr_cube_chain_lookup", n, texels && q && out);
}
int chain_launch(rtr_context* c, const rtr_cube_level* lv, int n_levels, const rtr_gather_out* d_texels, const rtr_cube_query* d_q,
                 rtr_gather_out* d_out, int64_t n) {
    ChainK C{};
    for (int i = 0; i < n_levels; ++i) C.lv[i] = lv[i];
    C.n = n_levels;
    return launch_records(c, "rtr_cube_chain_lookup", k_cube_chain_lookup, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(C, d_texels, d_q + k0, d_out + k0, m); });
}

/* what both set lookups check before any device work: context, set, the chain of one capture, n / NULL; no scene is needed */
int set_check(rtr_context* c, const rtr_capture_set* set, const rtr_cube_level* lv, int32_t n_levels, const void* texels,
              int64_t n_records, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = capture_set_why(set)) return fail(c, RTR_ERR_INVALID, std::string("rtr_capture_set_lookup: ") + why);
    if (n_records < 0) return fail(c, RTR_ERR_INVALID, "rtr_capture_set_lookup: negative n_records");
    if (const char* why = cube_chain_why(lv, n_levels, n_records))
        return fail(c, RTR_ERR_INVALID, std::string("rtr_capture_set_lookup: ") + why);
    return batch_check(c, "rtr_capture_set_lookup", n, texels && q && out);
}
int set_launch(rtr_context* c, const rtr_capture_set* set, const rtr_cube_level* lv, int n_levels, const rtr_gather_out* d_texels,
               const rtr_capture_query* d_q, rtr_gather_out* d_out, int64_t n) {
    ChainK C{};
    for (int i = 0; i < n_levels; ++i) C.lv[i] = lv[i];
    C.n = n_levels;
    const SetK S = set_k(set);
    return launch_records(c, "rtr_capture_set_lookup", k_capture_set_lookup, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(S, C, d_texels, d_q + k0, d_out + k0, m); });
}

} // namespace

extern "C" {

int rtr_capture_set_lookup_one(const rtr_capture_set* set, const rtr_cube_level* lv, int32_t n_levels, const rtr_gather_out* texels,
                               const rtr_capture_query* q, rtr_gather_out* out) {
    if (capture_set_why(set) || cube_chain_why(lv, n_levels, -1) || !texels || !q || !out) return RTR_ERR_INVALID;
    *out = capture_set_lookup_one(set_k(set), lv, n_levels, texels, q->p, q->d, q->alpha);
    return RTR_OK;
}

int rtr_capture_set_lookup(rtr_context* c, const rtr_capture_set* set, const rtr_cube_level* lv, int32_t n_levels,
                           const rtr_gather_out* texels, int64_t n_records, const rtr_capture_query* q, rtr_gather_out* out, int64_t n) {
    if (int rc = set_check(c, set, lv, n_levels, texels, n_records, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    /* the records of all captures stay at the head of the staging buffer for all slices: the first one brings them.
     * RTR_SET_SLICE, a test hook, lowers the slice */
    const size_t set_bytes = (size_t)set->n_captures * (size_t)n_records * sizeof(rtr_gather_out);
    const StagedIO io{set_bytes, sizeof(rtr_capture_query), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, env_cap("RTR_SET_SLICE", kCubeSlice), io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, texels, set_bytes, hipMemcpyHostToDevice, c->stream));
        return set_launch(c, set, lv, n_levels, static_cast<const rtr_gather_out*>(s.head), static_cast<const rtr_capture_query*>(s.in),
                          static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_capture_set_lookup_device(rtr_context* c, const rtr_capture_set* set, const rtr_cube_level* lv, int32_t n_levels,
                                  const rtr_gather_out* d_texels, int64_t n_records, const rtr_capture_query* d_q,
                                  rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = set_check(c, set, lv, n_levels, d_texels, n_records, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    const uintptr_t u0 = (uintptr_t)d_out;
    const size_t un = (size_t)n * sizeof(rtr_gather_out);
    const size_t set_bytes = (size_t)set->n_captures * (size_t)n_records * sizeof(rtr_gather_out);
    const auto meets = [&](uintptr_t b0, size_t bn) { return u0 < b0 + bn && b0 < u0 + un; };
    if (meets((uintptr_t)d_texels, set_bytes) || meets((uintptr_t)d_q, (size_t)n * sizeof(rtr_capture_query)))
        return fail(c, RTR_ERR_INVALID, "rtr_capture_set_lookup_device: out overlaps an input");
    return device_entry(c, "rtr_capture_set_lookup_device", (uintptr_t)d_texels | (uintptr_t)d_q | u0, blocking,
                        [&] { return set_launch(c, set, lv, n_levels, d_texels, d_q, d_out, n); });
}


void rtr_cube_filter_defaults(rtr_cube_filter_params* p) {
    if (!p) return;
    *p = rtr_cube_filter_params{};
    p->face_in = 32, p->face_out = 16, p->alpha = 0.25, p->cos_cut = 0.0;
}

int rtr_cube_filter_one(const rtr_cube_filter_params* fp, const rtr_gather_out* texels, int32_t face, int32_t a, int32_t b,
                        rtr_gather_out* out) {
    if (cube_filter_params_why(fp) || !texels || !out) return RTR_ERR_INVALID;
    if (face < 0 || face > 5 || a < 0 || a >= fp->face_out || b < 0 || b >= fp->face_out) return RTR_ERR_INVALID;
    const int Sin = fp->face_in, Fin = 6 * Sin * Sin;
    const double a2m1 = fp->alpha * fp->alpha - 1.0;
    double rx, ry, rz, dw;
    cube_texel_centre(fp->face_out, face, a, b, rx, ry, rz, dw);
    FilterAcc lanes[64];
    for (int l = 0; l < 64; ++l) filter_acc_zero(lanes[l]);
    for (int j = 0; j < Fin; ++j) { /* lane j % 64 meets its texels in increasing order */
        const int f = j / (Sin * Sin), r = j - f * Sin * Sin, jb = r / Sin;
        double lx, ly, lz;
        cube_texel_centre(Sin, f, r - jb * Sin, jb, lx, ly, lz, dw);
        const double c = (rx * lx + ry * ly) + rz * lz;
        if (c > fp->cos_cut)
            filter_add(lanes[j & 63], filter_weight(c, dw, a2m1), texels[j].v[0], texels[j].v[1], texels[j].v[2], texels[j].valid);
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) { /* lane l of the xor tree; the lanes above it are not read again */
            FilterAcc& s = lanes[l];
            const FilterAcc& o = lanes[l ^ off];
            for (int ch = 0; ch < 3; ++ch) s.v[ch] = s.v[ch] + o.v[ch];
            s.wsum = s.wsum + o.wsum, s.count += o.count, s.bad += o.bad;
        }
    *out = filter_result(lanes[0]);
    return RTR_OK;
}

int rtr_cube_filter(rtr_context* c, const rtr_cube_filter_params* fp, const rtr_gather_out* texels, rtr_gather_out* out,
                    int64_t n) {
    if (int rc = filter_check(c, fp, texels, out, n)) return rc;
    if (n == 0) return RTR_OK;
    /* the source cubes stay at the head of the staging buffer for all slices: the first one brings them */
    static_assert(sizeof(rtr_gather_out) % 16 == 0, "StagedIO::head_bytes");
    const size_t src_bytes = (size_t)n * face_records(fp->face_in) * sizeof(rtr_gather_out);
    const StagedIO io{src_bytes, 0, nullptr, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n * face_records(fp->face_out), kCubeSlice, io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, texels, src_bytes, hipMemcpyHostToDevice, c->stream));
        return filter_launch(c, fp, static_cast<const rtr_gather_out*>(s.head), static_cast<rtr_gather_out*>(s.out[0]), s.k0,
                             s.k0 + s.m);
    });
}

int rtr_cube_filter_device(rtr_context* c, const rtr_cube_filter_params* fp, const rtr_gather_out* d_texels,
                           rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = filter_check(c, fp, d_texels, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    const uintptr_t t0 = (uintptr_t)d_texels, t1 = t0 + (size_t)n * face_records(fp->face_in) * sizeof(rtr_gather_out);
    const uintptr_t u0 = (uintptr_t)d_out, u1 = u0 + (size_t)n * face_records(fp->face_out) * sizeof(rtr_gather_out);
    if (t0 < u1 && u0 < t1) return fail(c, RTR_ERR_INVALID, "rtr_cube_filter_device: texels and out overlap");
    return device_entry(c, "rtr_cube_filter_device", t0 | u0, blocking,
                        [&] { return filter_launch(c, fp, d_texels, d_out, 0, n * face_records(fp->face_out)); });
}

int rtr_cube_chain_plan(int32_t S, int32_t n_levels, rtr_cube_level* levels, int64_t* n_records) {
    if (S < 1 || S > RTR_CAPTURE_MAX_FACE || n_levels < 1 || n_levels > RTR_CHAIN_MAX_LEVELS || !n_records) return RTR_ERR_INVALID;
    int64_t at = 0;
    for (int i = 0; i < n_levels; ++i) {
        const int s = (S >> i) > 1 ? S >> i : 1;
        if (levels) {
            const double r = n_levels > 1 ? (double)i / (n_levels - 1) : 0.0;
            levels[i] = rtr_cube_level{s, 0, at, r * r};
        }
        at += face_records(s);
    }
    *n_records = at;
    return RTR_OK;
}

int rtr_cube_chain_lookup_one(const rtr_cube_level* lv, int32_t n_levels, const rtr_gather_out* texels, const rtr_cube_query* q,
                              rtr_gather_out* out) {
    if (cube_chain_why(lv, n_levels, -1) || !texels || !q || !out) return RTR_ERR_INVALID;
    *out = cube_chain_lookup_one(lv, n_levels, texels, *q, 1, 0);
    return RTR_OK;
}

int rtr_cube_chain_lookup(rtr_context* c, const rtr_cube_level* lv, int32_t n_levels, const rtr_gather_out* texels,
                          int64_t n_records, const rtr_cube_query* q, rtr_gather_out* out, int64_t n) {
    if (int rc = chain_check(c, lv, n_levels, texels, n_records, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    /* the chain's records stay at the head of the staging buffer for all slices: the first one brings them */
    const size_t chain_bytes = (size_t)n_records * sizeof(rtr_gather_out);
    const StagedIO io{chain_bytes, sizeof(rtr_cube_query), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kCubeSlice, io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, texels, chain_bytes, hipMemcpyHostToDevice, c->stream));
        return chain_launch(c, lv, n_levels, static_cast<const rtr_gather_out*>(s.head), static_cast<const rtr_cube_query*>(s.in),
                            static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_cube_chain_lookup_device(rtr_context* c, const rtr_cube_level* lv, int32_t n_levels, const rtr_gather_out* d_texels,
                                 int64_t n_records, const rtr_cube_query* d_q, rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = chain_check(c, lv, n_levels, d_texels, n_records, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_cube_chain_lookup_device", (uintptr_t)d_texels | (uintptr_t)d_q | (uintptr_t)d_out, blocking,
                        [&] { return chain_launch(c, lv, n_levels, d_texels, d_q, d_out, n); });
}

} /* extern "C" */
