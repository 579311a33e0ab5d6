/*
 * rtr_capture.hip -- environment captures (include/rtr_hip.h: rtr_capture_*, rtr_cube_*, rtr_latlong_direction,
 * rtr_write_rgbe): the centre check, the kernel choice among the 17 k_capture_li held here (the k_li family rule of
 * rt_select.h, like the gathers'), k_cube_lookup and its launch, the entries, and the host-only pieces that need no context
 * (rtr_capture_defaults, rtr_capture_ray, rtr_cube_lookup_one, rtr_latlong_direction, rtr_cube_to_latlong,
 * rtr_write_rgbe).  The entries' common checks, the staging of the host entries, the body of the device entries, the
 * chunked launcher and the single-ray entry are rt_batch.h's, shared with the other batch units.
 */
#include "rt_batch.h"

#include <cmath>
#include <cstdio>

using namespace rtr;

/* rtr_cube_lookup: one lane per direction, four records of 32 bytes each, straight-line (cube_lookup_one of rt_render.h) */
__global__ void __launch_bounds__(RTR_BLOCK) k_cube_lookup(const int S, const rtr_gather_out* __restrict__ texels,
                                                            const rtr_probe_point* __restrict__ dirs,
                                                            rtr_gather_out* __restrict__ out, long long n) {
    const long long k = (long long)blockIdx.x * RTR_BLOCK + threadIdx.x;
    if (k >= n) return;
    out[k] = cube_lookup_one(S, texels, dirs[k]);
}

namespace {

constexpr int64_t kCaptureSlice = (int64_t)1 << 20; /* texels (directions of a lookup) per slice of the host entries */

/* what both capture entries check before any device work, in the gathers' order: context, capture params, n / NULL,
 * render params, scene */
int capture_check(rtr_context* c, const rtr_render_params* rp, const rtr_capture_params* cp, const void* pts, const void* out,
                  int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (const char* why = capture_params_why(cp)) return fail(c, RTR_ERR_INVALID, std::string("rtr_capture_cube: ") + why);
    if (int rc = batch_check(c, "rtr_capture_cube", n, pts && out)) return rc;
    if (int rc = params_check(c, rp)) return rc;
    return scene_check(c, "rtr_capture_cube");
}

long long face_texels(int S) { return 6ll * S * S; }

/* launches over the device array of the call's centres on the context stream: the records [0, m) of d_out, which are
 * the texels first .. first + m of the call */
int capture_launch(rtr_context* c, const rtr_render_params* rp, const rtr_capture_params* cp, const rtr_probe_point* d_pts,
                   rtr_gather_out* d_out, long long first, long long m) {
    const int per_ray = per_ray_trav(c->facts, c->info, rp->flags, false);
    const int trav = li_trav(rp->integrator, per_ray);
    const size_t lds = stack_bytes(c->facts, c->info, per_ray);
    CaptureK K{};
    K.pts = d_pts, K.out = d_out, K.first = first, K.k0 = 0, K.n = m;
    K.S = cp->face_size, K.SS = K.S * K.S, K.F = 6 * K.SS;
    K.samples = cp->samples, K.lg = gather_lg(cp->samples), K.seed = cp->seed, K.point_base = cp->point_base;
    K.jitter = cp->jitter, K.time = cp->time, K.max_depth = rp->max_depth, K.rr_start = rp->rr_start_depth;
    int rc = RTR_OK;
    const bool found = dispatch_li(rp->integrator, trav, [&](auto i, auto t) {
        rc = launch_records(c, "rtr_capture_cube", k_capture_li<decltype(i)::value, decltype(t)::value>, lds, K.n, K.lg, texel_args(c->ds, K));
    });
    if (!found) return fail(c, RTR_ERR_UNSUPPORTED, "no capture kernel for traversal " + std::to_string(trav));
    if (rc == RTR_OK) c->last_batch[RTR_DEBUG_CAPTURE] = rtr_debug_batch{rp->integrator, trav, 0, K.lg};
    return rc;
}

/* what both lookup entries check before any device work: context, face size, n / NULL; no scene is needed */
int lookup_check(rtr_context* c, int32_t S, const void* texels, const void* q, const void* out, int64_t n) {
    if (!c) return RTR_ERR_INVALID;
    if (S < 1 || S > RTR_CAPTURE_MAX_FACE) return fail(c, RTR_ERR_INVALID, "rtr_cube_lookup: face_size outside 1 .. 4096");
    return batch_check(c, "rtr_cube_lookup", n, texels && q && out);
}
int lookup_launch(rtr_context* c, int S, const rtr_gather_out* d_texels, const rtr_probe_point* d_q, rtr_gather_out* d_out,
                  int64_t n) {
    return launch_records(c, "rtr_cube_lookup", k_cube_lookup, 0, n, 0,
                          [&](long long k0, long long m) { return std::make_tuple(S, d_texels, d_q + k0, d_out + k0, m); });
}

/* the four bytes of one texel of rtr_write_rgbe */
void rgbe_texel(const double* rgb, unsigned char* q) {
    double c[3], m = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        c[ch] = rgb[ch] > 0.0 ? rgb[ch] : 0.0; /* negative, NaN: 0 */
        m = c[ch] > m ? c[ch] : m;
    }
    if (m < 1e-32) {
        q[0] = q[1] = q[2] = q[3] = 0;
    } else if (!(m < 0x1p127)) {
        q[0] = q[1] = q[2] = q[3] = 255;
    } else {
        int e;
        const double f = std::frexp(m, &e);
        const double scale = (f * 256.0) / m;
        for (int ch = 0; ch < 3; ++ch) {
            const int b = (int)(c[ch] * scale);
            q[ch] = (unsigned char)(b < 255 ? b : 255);
        }
        q[3] = (unsigned char)(e + 128);
    }
}

} // namespace

extern "C" {

int rtr_capture_cube(rtr_context* c, const rtr_render_params* rp, const rtr_capture_params* cp, const rtr_probe_point* pts,
                     rtr_gather_out* out, int64_t n) {
    if (int rc = capture_check(c, rp, cp, pts, out, n)) return rc;
    if (n == 0) return RTR_OK;
    if (int rc = records_check(c, "rtr_capture_cube", "centre", kPositionRule, n, [&](int64_t k) { return probe_point_bad(pts[k]); }))
        return rc;
    return staged_texels(c, pts, n, face_texels(cp->face_size), sizeof(rtr_gather_out), out, kCaptureSlice,
                         [&](const rtr_probe_point* d_pts, void* d_out, long long first, long long m) {
                             return capture_launch(c, rp, cp, d_pts, static_cast<rtr_gather_out*>(d_out), first, m);
                         });
}

int rtr_capture_cube_device(rtr_context* c, const rtr_render_params* rp, const rtr_capture_params* cp,
                            const rtr_probe_point* d_pts, rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = capture_check(c, rp, cp, d_pts, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_capture_cube_device", (uintptr_t)d_pts | (uintptr_t)d_out, blocking,
                        [&] { return capture_launch(c, rp, cp, d_pts, d_out, 0, n * face_texels(cp->face_size)); });
}

void rtr_capture_defaults(rtr_capture_params* p) {
    if (!p) return;
    *p = rtr_capture_params{};
    p->face_size = 32, p->samples = 16, p->jitter = 1;
}

int rtr_capture_ray(const rtr_capture_params* cp, const rtr_probe_point* point, int64_t index_in_call, int32_t face, int32_t a,
                    int32_t b, int32_t s, rtr_ray* out) {
    if (capture_params_why(cp)) return RTR_ERR_INVALID;
    const int S = cp->face_size;
    if (face < 0 || face > 5 || a < 0 || a >= S || b < 0 || b >= S) return RTR_ERR_INVALID;
    const RaySeed seed{cp->seed, cp->point_base, 6 * S * S, (face * S + b) * S + a, cp->samples, cp->time, 0.001, __builtin_huge_val()};
    return sample_ray(seed, point ? point->p : nullptr, index_in_call, s, out, [&](uint32_t& rng, double* d) {
        if (probe_point_bad(*point)) return false;
        capture_direction(S, face, a, b, cp->jitter, rng, d[0], d[1], d[2]);
        return true;
    });
}

int rtr_cube_lookup_one(int32_t S, const rtr_gather_out* texels, const rtr_probe_point* q, rtr_gather_out* out) {
    if (S < 1 || S > RTR_CAPTURE_MAX_FACE || !texels || !q || !out) return RTR_ERR_INVALID;
    *out = cube_lookup_one(S, texels, *q);
    return RTR_OK;
}

int rtr_cube_lookup(rtr_context* c, int32_t S, const rtr_gather_out* texels, const rtr_probe_point* q, rtr_gather_out* out,
                    int64_t n) {
    if (int rc = lookup_check(c, S, texels, q, out, n)) return rc;
    if (n == 0) return RTR_OK;
    /* the capture stays at the head of the staging buffer for all slices: the first one brings it */
    static_assert(sizeof(rtr_gather_out) % 16 == 0, "StagedIO::head_bytes");
    const size_t cube_bytes = (size_t)face_texels(S) * sizeof(rtr_gather_out);
    const StagedIO io{cube_bytes, sizeof(rtr_probe_point), q, {sizeof(rtr_gather_out), 0}, {out, nullptr}};
    return staged_slices(c, n, kCaptureSlice, io, [&](const Slice& s) {
        if (s.k0 == 0) HIPCHK(c, hipMemcpyAsync(s.head, texels, cube_bytes, hipMemcpyHostToDevice, c->stream));
        return lookup_launch(c, S, static_cast<const rtr_gather_out*>(s.head), static_cast<const rtr_probe_point*>(s.in),
                             static_cast<rtr_gather_out*>(s.out[0]), s.m);
    });
}

int rtr_cube_lookup_device(rtr_context* c, int32_t S, const rtr_gather_out* d_texels, const rtr_probe_point* d_q,
                           rtr_gather_out* d_out, int64_t n, int blocking) {
    if (int rc = lookup_check(c, S, d_texels, d_q, d_out, n)) return rc;
    if (n == 0) return RTR_OK;
    return device_entry(c, "rtr_cube_lookup_device", (uintptr_t)d_texels | (uintptr_t)d_q | (uintptr_t)d_out, blocking,
                        [&] { return lookup_launch(c, S, d_texels, d_q, d_out, n); });
}

int rtr_latlong_direction(int32_t W, int32_t H, int32_t i, int32_t j, double d[3]) {
    if (W < 1 || H < 1 || i < 0 || i >= W || j < 0 || j >= H || !d) return RTR_ERR_INVALID;
    const double pi = 3.141592653589793;
    const double u = (i + 0.5) / W, v = (j + 0.5) / H;
    const double phi = 2.0 * pi * u - pi, theta = pi * v;
    d[0] = std::sin(theta) * std::cos(phi), d[1] = std::cos(theta), d[2] = -std::sin(theta) * std::sin(phi);
    return RTR_OK;
}

int rtr_cube_to_latlong(int32_t S, const rtr_gather_out* texels, int32_t W, int32_t H, double* out_rgb) {
    if (S < 1 || S > RTR_CAPTURE_MAX_FACE || !texels || W < 1 || H < 1 || !out_rgb) return RTR_ERR_INVALID;
    for (int32_t j = 0; j < H; ++j)
        for (int32_t i = 0; i < W; ++i) {
            rtr_probe_point q;
            rtr_latlong_direction(W, H, i, j, q.p);
            const rtr_gather_out o = cube_lookup_one(S, texels, q);
            for (int ch = 0; ch < 3; ++ch) out_rgb[((size_t)j * W + i) * 3 + ch] = o.v[ch];
        }
    return RTR_OK;
}

int rtr_write_rgbe(const char* path, int32_t W, int32_t H, const double* rgb) {
    if (!path || W < 1 || H < 1 || !rgb) return RTR_ERR_INVALID;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return RTR_ERR_DEVICE;
    std::vector<unsigned char> row((size_t)W * 4);
    bool ok = std::fprintf(f, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n", (int)H, (int)W) > 0;
    for (int32_t j = 0; j < H && ok; ++j) {
        for (int32_t i = 0; i < W; ++i) rgbe_texel(rgb + ((size_t)j * W + i) * 3, &row[(size_t)i * 4]);
        ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    ok = (std::fclose(f) == 0) && ok;
    return ok ? RTR_OK : RTR_ERR_DEVICE;
}

} /* extern "C" */
