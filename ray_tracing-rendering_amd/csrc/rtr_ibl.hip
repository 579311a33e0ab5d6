/*
 * rtr_ibl.hip -- image-based shading (include/rtr_hip.h: rtr_brdf_*, rtr_shade_ibl*): the parameter and environment checks,
 * the split of a table call into launches of bounded work, the two kernels of rt_ibl_kernels.h and their launches, the entries, and
 * the host-only pieces that need no context (rtr_brdf_entry_one, rtr_brdf_fetch_one, rtr_shade_ibl_one), and the set forms
 * of the shader (rtr_shade_ibl_set*: the same entries with a capture set behind the environment).  The entries'
 * common checks, the staging of the host entries, the body of the device entries, the chunked launcher of the shader and
 * the cap hook are rt_batch.h's, shared with the other batch units; the staging of an environment is rt_ibl.h's.
 */
#include "rt_batch.h"
#include "rt_ibl_kernels.h"

using namespace rtr;

namespace {

constexpr int64_t kShadeSlice = (int64_t)1 << 20; /* queries (table entries) per slice of the host entries */
constexpr long long kTableNodes = 1ll << 31;      /* nodes per launch at most (RTR_TABLE_NODES, a test hook, lowers it) */

/* what both table entries check before any device work: context, params, NULL; no scene is needed */
int table_check(rtr_context* c, const rtr_brdf_params* bp, const void* out) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = brdf_params_why(bp)) return fail(c, RTR_ERR_INVALID, std::string("rtr_brdf_table: ") + why);
    return batch_check(c, "rtr_brdf_table", 1, out != nullptr);
}

/* the entries [e0, e1) of the table (numbered r * n_mu + c) into d_out, whose record 0 is e0.  No launch holds more than
 * that many nodes: whole rows one above the other while they fit, else one row's columns in runs */
int table_launch(rtr_context* c, const rtr_brdf_params* bp, rtr_brdf_entry* d_out, long long e0, long long e1) {
    TableK K{};
    K.out = d_out, K.out_first = e0;
    K.n_mu = bp->n_mu, K.n_rough = bp->n_rough, K.M = bp->nodes;
    const long long per_launch = std::max(1ll, env_cap("RTR_TABLE_NODES", kTableNodes) / (2ll * K.M * K.M)); /* entries */
    for (long long e = e0; e < e1;) {
        const int r = (int)(e / K.n_mu), col = (int)(e - (long long)r * K.n_mu);
        long long rows = 1;
        K.row0 = r, K.c0 = col;
        if (col == 0 && e1 - e >= K.n_mu && per_launch >= K.n_mu) {
            rows = std::min((e1 - e) / K.n_mu, per_launch / K.n_mu);
            K.c1 = K.n_mu;
        } else {
            K.c1 = (int)std::min<long long>(K.n_mu, col + std::min(per_launch, e1 - e));
        }
        const int cols = K.c1 - K.c0, per_wg = RTR_BLOCK / 64;
        hipLaunchKernelGGL(k_brdf_table, dim3((unsigned)((cols + per_wg - 1) / per_wg), (unsigned)rows), dim3(RTR_BLOCK), 0, c->stream, K);
        e += rows * (long long)cols;
    }
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? RTR_OK : fail(c, RTR_ERR_DEVICE, std::string("brdf table launch: ") + hipGetErrorString(err));
}

/* what both shader entries check before any device work: context, environment, n / NULL; no scene is needed */
int shade_check(rtr_context* c, const rtr_shade_env* env, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = env_why(env)) return fail(c, RTR_ERR_INVALID, std::string("rtr_shade_ibl: ") + why);
    return batch_check(c, "rtr_shade_ibl", n, q && out);
}
int shade_launch(rtr_context* c, const ShadeK& K, const rtr_shade_query* d_q, rtr_gather_out* d_out, int64_t n) {
    return launch_records(c, "rtr_shade_ibl", k_shade_ibl, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(K, d_q + k0, d_out + k0, m); });
}

/* the set forms: the same checks with the set's rules behind the environment's; without SPECULAR the set is not looked at */
int shade_set_check(rtr_context* c, const rtr_shade_env* env, const rtr_capture_set* set, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = env_set_why(env, set)) return fail(c, RTR_ERR_INVALID, std::string("rtr_shade_ibl_set: ") + why);
    return batch_check(c, "rtr_shade_ibl_set", n, q && out);
}
int shade_set_launch(rtr_context* c, const ShadeK& K, const SetK& S, const rtr_shade_query* d_q, rtr_gather_out* d_out, int64_t n) {
    return launch_records(c, "rtr_shade_ibl_set", k_shade_ibl_set, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(K, S, d_q + k0, d_out + k0, m); });
}

} // namespace

extern "C" {

int rtr_shade_ibl_set_one(const rtr_shade_env* env, const rtr_capture_set* set, const rtr_shade_query* q, rtr_gather_out* out) {
    double nlen, vlen;
    if (env_set_why(env, set) || !q || !out || shade_query_bad(*q, nlen, vlen)) return RTR_ERR_INVALID;
    const SetK S = env_set_k(env, set);
    *out = shade_ibl_one<true>(shade_k(env, env->probes, env->depth, env->chain, env->table), *q, nlen, vlen, &S);
    return RTR_OK;
}

int rtr_shade_ibl_set(rtr_context* c, const rtr_shade_env* env, const rtr_capture_set* set, const rtr_shade_query* q,
                      rtr_gather_out* out, int64_t n) {
    if (int rc = shade_set_check(c, env, set, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_shade_ibl_set", "query", "a non-finite field, or a normal or view vector whose length is not in (0, inf)",
                               n, [&](int64_t k) {
                                   double nlen, vlen;
                                   return shade_query_bad(q[k], nlen, vlen);
                               }))
        return rc;
    /* as rtr_shade_ibl: the arrays at the head of the staging buffer, the set's chains among them; the set itself travels as
     * a kernel argument.  RTR_SET_SLICE, a test hook, lowers the slice */
    const EnvBytes b = env_bytes(env, env_cubes(env, set));
    const SetK S = env_set_k(env, set);
    const StagedIO io{b.total(), sizeof(rtr_shade_query), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, env_cap("RTR_SET_SLICE", kShadeSlice), io, [&](const Slice& s) {
        ShadeK K;
        HIPCHK(c, env_stage(env, b, static_cast<char*>(s.head), s.k0 == 0, c->stream, K));
        return shade_set_launch(c, K, S, static_cast<const rtr_shade_query*>(s.in), static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_shade_ibl_set_device(rtr_context* c, const rtr_shade_env* env, const rtr_capture_set* set, const rtr_shade_query* d_q,
                             rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = shade_set_check(c, env, set, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    const EnvBytes b = env_bytes(env, env_cubes(env, set));
    const uintptr_t u0 = (uintptr_t)d_out;
    const size_t un = (size_t)n * sizeof(rtr_gather_out);
    uintptr_t bits = u0 | (uintptr_t)d_q;
    if (spans_overlap(u0, un, (uintptr_t)d_q, (size_t)n * sizeof(rtr_shade_query)) || env_overlaps(env, b, u0, un, bits))
        return fail(c, RTR_ERR_INVALID, "rtr_shade_ibl_set_device: out overlaps an input");
    const SetK S = env_set_k(env, set);
    return device_entry(c, "rtr_shade_ibl_set_device", bits, blocking, [&] {
        return shade_set_launch(c, shade_k(env, env->probes, env->depth, env->chain, env->table), S, d_q, d_out, n);
    });
}

int rtr_brdf_entry_one(const rtr_brdf_params* bp, int32_t r, int32_t c, rtr_brdf_entry* out) {
    if (brdf_params_why(bp) || !out || r < 0 || r >= bp->n_rough || c < 0 || c >= bp->n_mu) return RTR_ERR_INVALID;
    const int M = bp->nodes, MM = M * M;
    const BrdfRow R = brdf_row(r, bp->n_rough);
    const BrdfCol C = brdf_col(c, bp->n_mu, R);
    double W[64], A[64], B[64];
    for (int l = 0; l < 64; ++l) W[l] = A[l] = B[l] = 0.0;
    for (int j = 0; j < 2 * MM; ++j) { /* lane j % 64 meets its nodes in increasing order */
        const int jj = j < MM ? j : j - MM;
        const BrdfS S = brdf_s(jj / M, M, R);
        const BrdfT T = brdf_t(jj % M, M);
        W[j & 63] = W[j & 63] + T.wphi * S.s;
        brdf_node(R, C, S, T, j < MM ? 1.0 : -1.0, A[j & 63], B[j & 63]);
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) /* lane l of the xor tree; the lanes above it are not read again */
            W[l] = W[l] + W[l ^ off], A[l] = A[l] + A[l ^ off], B[l] = B[l] + B[l ^ off];
    *out = brdf_result(W[0], A[0], B[0]);
    return RTR_OK;
}

int rtr_brdf_fetch_one(int32_t n_mu, int32_t n_rough, const rtr_brdf_entry* table, double mu, double rough, rtr_brdf_entry* out) {
    if (n_mu < 1 || n_mu > RTR_BRDF_MAX || n_rough < 1 || n_rough > RTR_BRDF_MAX || !table || !out) return RTR_ERR_INVALID;
    if (!__builtin_isfinite(mu) || !__builtin_isfinite(rough)) return RTR_ERR_INVALID;
    *out = brdf_fetch(n_mu, n_rough, table, mu, rough);
    return RTR_OK;
}

int rtr_brdf_table(rtr_context* c, const rtr_brdf_params* bp, rtr_brdf_entry* out) {
    if (int rc = table_check(c, bp, out)) return rc;
    const StagedIO io{0, 0, nullptr, {sizeof(rtr_brdf_entry), 0}, {out, nullptr}};
    return staged_slices(c, (int64_t)bp->n_mu * bp->n_rough, kShadeSlice, io, [&](const Slice& s) {
        return table_launch(c, bp, static_cast<rtr_brdf_entry*>(s.out[0]), s.k0, s.k0 + s.m);
    });
}

int rtr_brdf_table_device(rtr_context* c, const rtr_brdf_params* bp, rtr_brdf_entry* d_out, int blocking) {
    if (int rc = table_check(c, bp, d_out)) return rc;
    return device_entry(c, "rtr_brdf_table_device", (uintptr_t)d_out, blocking,
                        [&] { return table_launch(c, bp, d_out, 0, (long long)bp->n_mu * bp->n_rough); });
}

int rtr_shade_ibl_one(const rtr_shade_env* env, const rtr_shade_query* q, rtr_gather_out* out) {
    double nlen, vlen;
    if (env_why(env) || !q || !out || shade_query_bad(*q, nlen, vlen)) return RTR_ERR_INVALID;
    *out = shade_ibl_one(shade_k(env, env->probes, env->depth, env->chain, env->table), *q, nlen, vlen);
    return RTR_OK;
}

int rtr_shade_ibl(rtr_context* c, const rtr_shade_env* env, const rtr_shade_query* q, rtr_gather_out* out, int64_t n) {
    if (int rc = shade_check(c, env, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_shade_ibl", "query", "a non-finite field, or a normal or view vector whose length is not in (0, inf)",
                               n, [&](int64_t k) {
                                   double nlen, vlen;
                                   return shade_query_bad(q[k], nlen, vlen);
                               }))
        return rc;
    /* the environment's arrays stay at the head of the staging buffer for all slices: the first slice brings them */
    const EnvBytes b = env_bytes(env);
    const StagedIO io{b.total(), sizeof(rtr_shade_query), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kShadeSlice, io, [&](const Slice& s) {
        ShadeK K;
        HIPCHK(c, env_stage(env, b, static_cast<char*>(s.head), s.k0 == 0, c->stream, K));
        return shade_launch(c, K, static_cast<const rtr_shade_query*>(s.in), static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_shade_ibl_device(rtr_context* c, const rtr_shade_env* env, const rtr_shade_query* d_q, rtr_gather_out* d_out, int64_t n,
                         int blocking) {
    if (int rc = shade_check(c, env, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    const EnvBytes b = env_bytes(env);
    const uintptr_t u0 = (uintptr_t)d_out;
    const size_t un = (size_t)n * sizeof(rtr_gather_out);
    uintptr_t bits = u0 | (uintptr_t)d_q;
    if (spans_overlap(u0, un, (uintptr_t)d_q, (size_t)n * sizeof(rtr_shade_query)) || env_overlaps(env, b, u0, un, bits))
        return fail(c, RTR_ERR_INVALID, "rtr_shade_ibl_device: out overlaps an input");
    return device_entry(c, "rtr_shade_ibl_device", bits, blocking,
                        [&] { return shade_launch(c, shade_k(env, env->probes, env->depth, env->chain, env->table), d_q, d_out, n); });
}

} /* extern "C" */
