/*
 * rtr_image.hip -- what happens to an image after its samples (include/rtr_hip.h): the a-trous denoiser on an
 * accumulator or on host planes, the histories and the temporal reprojection in front of it, and the display transform.
 * Holds the kernels of rt_image_kernels.h.
 */
#include "rt_context.h"
#include "rt_image_kernels.h"

#include <cstring>

using namespace rtr;

/* ---- the a-trous denoiser ----------------------------------------------------------------------------------------- */
namespace {

/* the defaults of rtr_denoise_defaults: the sweep of INTEGRATION.md section 4, "Denoising" */
constexpr rtr_denoise_params kDenoiseDefaults = {4, 8, 16.0, 0.2, 0.3, 1.0, {0.0, 0.0, 0.0, 0.0}};

int denoise_check(rtr_context* c, const rtr_denoise_params* p) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null denoise params");
    if (p->iterations < 0 || p->iterations > 10) return fail(c, RTR_ERR_INVALID, "iterations must be in 0..10");
    if (p->feature_spp < 1) return fail(c, RTR_ERR_INVALID, "feature_spp must be >= 1");
    for (double s : {p->sigma_l, p->sigma_n, p->sigma_a, p->sigma_z})
        if (!(s > 0.0) || !std::isfinite(s)) return fail(c, RTR_ERR_INVALID, "the sigmas must be finite and > 0");
    for (double r : p->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    return RTR_OK;
}

/* the planes of a w x h region in c->b_denoise */
int denoise_planes(rtr_context* c, int w, int h, const rtr_denoise_params* prm, DenoiseK& D) {
    const size_t np = (size_t)w * h;
    /* doubles: m 3, q 1, feat 7, c 3 + 3, v 1 + 1, a 3, nrm 3, z 1, out 3; then n (int) and rgb8 (3 bytes) */
    const size_t n_doubles = 29 * np;
    if (int rc = ensure_behind_queue(c, c->b_denoise, n_doubles * sizeof(double) + np * sizeof(int) + 3 * np)) return rc;
    double* d = static_cast<double*>(c->b_denoise.p);
    D = DenoiseK{};
    D.w = w, D.h = h, D.iterations = prm->iterations;
    D.sl2 = prm->sigma_l * prm->sigma_l, D.sn2 = prm->sigma_n * prm->sigma_n;
    D.sa2 = prm->sigma_a * prm->sigma_a, D.sz2 = prm->sigma_z * prm->sigma_z;
    D.m = d, d += 3 * np;
    D.q = d, d += np;
    D.feat = d, d += RTR_FEAT * np;
    D.c[0] = d, d += 3 * np;
    D.c[1] = d, d += 3 * np;
    D.v[0] = d, d += np;
    D.v[1] = d, d += np;
    D.a = d, d += 3 * np;
    D.nrm = d, d += 3 * np;
    D.z = d, d += np;
    D.out = d, d += 3 * np;
    D.n = reinterpret_cast<int*>(d);
    D.rgb8 = reinterpret_cast<unsigned char*>(D.n + np);
    return RTR_OK;
}

/* where a denoise call's outputs go: HOST buffers (the library's planes, a copy, a wait and a per-pixel loop on the CPU)
 * or, with `device`, the caller's DEVICE buffers, written by k_denoise_out itself with nothing after it on the host */
struct DenoiseOut {
    double* linear;
    int64_t row_stride;
    uint8_t* rgb8;
    bool device;
    int blocking; /* device only */
};

/* prep, the passes and the output on the filled input planes; then the valid pixels into the caller's buffers (linear:
 * row r at linear + r * row_stride * 3; 8-bit: rows of w pixels, the top row first).  With `T` the temporal blend and
 * the history write-back take the place of the prep (rtr_accum_denoise_temporal). */
int denoise_run(rtr_context* c, DenoiseK D, const DenoiseOut& O, const TemporalK* T = nullptr) {
    double* const h_linear = O.linear;
    uint8_t* const h_rgb8 = O.rgb8;
    const size_t np = (size_t)D.w * D.h;
    const dim3 grid1((unsigned)((np + RTR_BLOCK - 1) / RTR_BLOCK)), grid2((unsigned)((D.w + 15) / 16), (unsigned)((D.h + 15) / 16));
    if (!h_linear) D.out = nullptr;
    if (!h_rgb8) D.rgb8 = nullptr;
    const int64_t row_stride = O.device ? O.row_stride : D.w; /* of D.out: the host forms read the library's plane */
    if (O.device) D.out = O.linear, D.rgb8 = O.rgb8;
    if (T) {
        hipLaunchKernelGGL(k_temporal_blend, grid2, dim3(RTR_BLOCK), 0, c->stream, D, *T);
        hipLaunchKernelGGL(k_temporal_store, grid1, dim3(RTR_BLOCK), 0, c->stream, D, *T);
    } else {
        hipLaunchKernelGGL(k_denoise_prep, grid1, dim3(RTR_BLOCK), 0, c->stream, D);
    }
    int src = 0;
    /* steps 1 and 2 from LDS unless RTR_DENOISE_LDS=0 (A/B measurement: INTEGRATION.md section 4, "Denoising") */
    const char* lds_env = getenv("RTR_DENOISE_LDS");
    const bool lds = !(lds_env && lds_env[0] == '0');
    for (int k = 0; k < D.iterations; ++k, src ^= 1) {
        if (lds && k == 0)
            hipLaunchKernelGGL(k_denoise_pass_lds<1>, grid2, dim3(RTR_BLOCK), 0, c->stream, D, src);
        else if (lds && k == 1)
            hipLaunchKernelGGL(k_denoise_pass_lds<2>, grid2, dim3(RTR_BLOCK), 0, c->stream, D, src);
        else
            hipLaunchKernelGGL(k_denoise_pass, grid2, dim3(RTR_BLOCK), 0, c->stream, D, 1 << k, src);
    }
    hipLaunchKernelGGL(k_denoise_out, grid1, dim3(RTR_BLOCK), 0, c->stream, D, src, (long long)row_stride);
    HIPCHK(c, hipGetLastError());
    if (O.device) { /* D.n decided on the device which pixels were written */
        if (O.blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
        return RTR_OK;
    }
    std::vector<int> n(np);
    std::vector<double> lin(h_linear ? 3 * np : 0);
    std::vector<unsigned char> rgb(h_rgb8 ? 3 * np : 0);
    HIPCHK(c, hipMemcpyAsync(n.data(), D.n, np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (h_linear) HIPCHK(c, hipMemcpyAsync(lin.data(), D.out, 3 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_rgb8) HIPCHK(c, hipMemcpyAsync(rgb.data(), D.rgb8, 3 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int y = 0; y < D.h; ++y)
        for (int x = 0; x < D.w; ++x) {
            const size_t p = (size_t)y * D.w + x;
            if (n[p] == 0) continue;
            if (h_linear) std::memcpy(h_linear + ((size_t)y * (size_t)O.row_stride + x) * 3, &lin[3 * p], 3 * sizeof(double));
            if (h_rgb8) {
                const size_t o = ((size_t)(D.h - 1 - y) * D.w + x) * 3;
                h_rgb8[o] = rgb[o], h_rgb8[o + 1] = rgb[o + 1], h_rgb8[o + 2] = rgb[o + 2];
            }
        }
    return RTR_OK;
}

/* the defaults of rtr_temporal_defaults ("Camera updates and temporal reprojection") */
constexpr rtr_temporal_params kTemporalDefaults = {0.05, 0.1, 0.25, 0.25, {0.0, 0.0, 0.0, 0.0}};

int temporal_check(rtr_context* c, const rtr_temporal_params* t) {
    if (!t) return fail(c, RTR_ERR_INVALID, "null temporal params");
    if (!(t->alpha_min > 0.0 && t->alpha_min <= 1.0)) return fail(c, RTR_ERR_INVALID, "alpha_min must be in (0, 1]");
    if (!(t->tau_z > 0.0) || !std::isfinite(t->tau_z) || !(t->tau_n > 0.0) || !std::isfinite(t->tau_n))
        return fail(c, RTR_ERR_INVALID, "tau_z and tau_n must be finite and > 0");
    if (!(t->min_weight > 0.0 && t->min_weight < 1.0)) return fail(c, RTR_ERR_INVALID, "min_weight must be in (0, 1)");
    for (double r : t->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    return RTR_OK;
}

int history_check(rtr_context* c, const rtr_history* h) {
    if (!h) return fail(c, RTR_ERR_INVALID, "null history");
    if (h->ctx != c) return fail(c, RTR_ERR_INVALID, "the history belongs to another context");
    return RTR_OK;
}

/* rtr_accum_denoise, and with `hist` rtr_accum_denoise_temporal: ONE list of checks, all before any device work; then
 * features, gather and the filter, with the temporal stage in the prep's place */
int accum_denoise(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, rtr_history* hist, const rtr_temporal_params* tp,
                  const DenoiseOut& O) {
    double* const h_linear = O.linear;
    uint8_t* const h_rgb8 = O.rgb8;
    const int64_t row_stride = O.row_stride;
    if (!c) return RTR_ERR_INVALID;
    if (int rc = accum_render_check(c, a)) return rc;
    if (int rc = denoise_check(c, prm)) return rc;
    if (hist)
        if (int rc = temporal_check(c, tp)) return rc;
    if (!a->moments) return fail(c, RTR_ERR_INVALID, "the accumulator keeps no moments (RTR_ACCUM_MOMENTS)");
    const rtr_render_params& p = a->params;
    const int w = p.x1 - p.x0, h = p.y1 - p.y0;
    if (!h_linear && !h_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    if (h_linear && row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad output stride");
    if (O.device && reinterpret_cast<uintptr_t>(h_linear) % sizeof(double))
        return fail(c, RTR_ERR_INVALID, "d_linear is not 8-byte aligned");
    if (p.tile_stride > 1)
        return fail(c, RTR_ERR_UNSUPPORTED, hist ? "a tile-sharded accumulator: temporal denoising is single-context"
                                                 : "a tile-sharded accumulator: gather the shards and call rtr_denoise_host");
    if (hist) {
        if (int rc = history_check(c, hist)) return rc;
        if (hist->W != p.image_width || hist->H != p.image_height || hist->x0 != p.x0 || hist->y0 != p.y0 || hist->x1 != p.x1 ||
            hist->y1 != p.y1)
            return fail(c, RTR_ERR_INVALID, "the history was created for another image size or region");
    }
    const size_t n = a->tiles.size();
    if (n == 0) return RTR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (O.device)
        (void)hipGetLastError();
    else if (int rc = refresh_counts(c, a)) /* (the device forms leave the counts where they are: k_denoise_gather reads them) */
        return rc;
    if (int rc = accum_features(c, a, prm->feature_spp)) return rc;
    DenoiseK D;
    if (int rc = denoise_planes(c, w, h, prm, D)) return rc;
    hipLaunchKernelGGL(k_denoise_gather, dim3((unsigned)n), dim3(RTR_BLOCK), 0, c->stream, accum_view(a),
                       static_cast<const double*>(a->d_q.p), static_cast<const double*>(a->d_feat.p), D);
    HIPCHK(c, hipGetLastError());
    if (!hist) return denoise_run(c, D, O);
    TemporalK T{};
    T.cam = c->ds.camera, T.prev = hist->cam;
    T.W = p.image_width, T.H = p.image_height, T.x0 = p.x0, T.y0 = p.y0;
    T.have = hist->have ? 1 : 0;
    T.alpha_min = tp->alpha_min, T.tau_z = tp->tau_z, T.tau_n = tp->tau_n, T.min_weight = tp->min_weight;
    T.hist_in = static_cast<const double*>(hist->d_planes[hist->cur].p);
    T.hist_out = static_cast<double*>(hist->d_planes[hist->cur ^ 1].p);
    T.mom = static_cast<double*>(hist->d_mom.p);
    if (int rc = denoise_run(c, D, O, &T)) return rc;
    hist->cur ^= 1, hist->have = true, hist->cam = c->ds.camera; /* the write-back counts once the frame has finished */
    return RTR_OK;
}

} // namespace

void rtr::free_history(rtr_history* h) {
    for (DevBuf* b : {&h->d_planes[0], &h->d_planes[1], &h->d_mom})
        if (b->p) hipFree(b->p);
    delete h;
}

extern "C" {

void rtr_denoise_defaults(rtr_denoise_params* p) {
    if (p) *p = kDenoiseDefaults;
}

int rtr_accum_denoise(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, double* h_linear, int64_t row_stride,
                      uint8_t* h_rgb8) {
    return accum_denoise(c, a, prm, nullptr, nullptr, DenoiseOut{h_linear, row_stride, h_rgb8, false, 1});
}

int rtr_accum_denoise_device(rtr_context* c, rtr_accum* a, const rtr_denoise_params* prm, double* d_linear, int64_t row_stride,
                             uint8_t* d_rgb8, int blocking) {
    return accum_denoise(c, a, prm, nullptr, nullptr, DenoiseOut{d_linear, row_stride, d_rgb8, true, blocking});
}

int rtr_denoise_host(rtr_context* c, const rtr_denoise_params* prm, int32_t width, int32_t height, const double* h_color,
                     const double* h_q, const int32_t* h_count, const double* h_feat, double* h_linear, uint8_t* h_rgb8) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = denoise_check(c, prm)) return rc;
    if (width < 1 || height < 1 || (int64_t)width * height > ((int64_t)1 << 28))
        return fail(c, RTR_ERR_INVALID, "region size out of range");
    if (!h_color || !h_q || !h_count || !h_feat) return fail(c, RTR_ERR_INVALID, "null input plane");
    if (!h_linear && !h_rgb8) return fail(c, RTR_ERR_INVALID, "no output buffer");
    const size_t np = (size_t)width * height;
    for (size_t p = 0; p < np; ++p)
        if (h_count[p] < 0) return fail(c, RTR_ERR_INVALID, "negative sample count");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DenoiseK D;
    if (int rc = denoise_planes(c, width, height, prm, D)) return rc;
    HIPCHK(c, hipMemcpy(D.m, h_color, 3 * np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.q, h_q, np * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.n, h_count, np * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(D.feat, h_feat, RTR_FEAT * np * sizeof(double), hipMemcpyHostToDevice));
    return denoise_run(c, D, DenoiseOut{h_linear, width, h_rgb8, false, 1});
}

void rtr_temporal_defaults(rtr_temporal_params* p) {
    if (p) *p = kTemporalDefaults;
}

int rtr_history_create(rtr_context* c, const rtr_render_params* p, rtr_history** out) {
    if (!c) return RTR_ERR_INVALID;
    if (!out) return fail(c, RTR_ERR_INVALID, "null out");
    *out = nullptr;
    if (!p) return fail(c, RTR_ERR_INVALID, "null params");
    if (image_too_small(*p)) return fail(c, RTR_ERR_INVALID, "image smaller than 2x2");
    if (region_outside(*p)) return fail(c, RTR_ERR_INVALID, "region outside the image or empty");
    HIPCHK(c, hipSetDevice(c->device));
    rtr_history* h = new rtr_history();
    h->ctx = c;
    h->W = p->image_width, h->H = p->image_height;
    h->x0 = p->x0, h->y0 = p->y0, h->x1 = p->x1, h->y1 = p->y1;
    const size_t np = (size_t)(p->x1 - p->x0) * (size_t)(p->y1 - p->y0), bytes = np * RTR_HIST * sizeof(double);
    int rc = ensure(c, h->d_planes[0], bytes);
    if (!rc) rc = ensure(c, h->d_planes[1], bytes);
    if (!rc) rc = ensure(c, h->d_mom, np * 3 * sizeof(double));
    for (int k = 0; k < 2 && !rc; ++k)
        if (hipMemsetAsync(h->d_planes[k].p, 0, bytes, c->stream) != hipSuccess) rc = fail(c, RTR_ERR_DEVICE, "hipMemsetAsync of a history");
    if (rc) {
        free_history(h);
        return rc;
    }
    c->histories.push_back(h);
    *out = h;
    return RTR_OK;
}

int rtr_history_clear(rtr_context* c, rtr_history* h) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = history_check(c, h)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)(h->x1 - h->x0) * (size_t)(h->y1 - h->y0) * RTR_HIST * sizeof(double);
    for (DevBuf& b : h->d_planes) HIPCHK(c, hipMemsetAsync(b.p, 0, bytes, c->stream));
    h->have = false;
    h->cur = 0;
    h->cam = rtr_camera{};
    return RTR_OK;
}

void rtr_history_destroy(rtr_history* h) {
    if (!h) return;
    rtr_context* c = h->ctx;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream); /* a frame may still use the planes */
    c->histories.erase(std::remove(c->histories.begin(), c->histories.end(), h), c->histories.end());
    free_history(h);
}

int rtr_history_planes(rtr_context* c, rtr_history* h, double* h_planes, int64_t row_stride) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = history_check(c, h)) return rc;
    const int w = h->x1 - h->x0, ht = h->y1 - h->y0;
    if (!h_planes || row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad output buffer / stride");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t row = (size_t)w * RTR_HIST * sizeof(double);
    HIPCHK(c, hipMemcpy2D(h_planes, (size_t)row_stride * RTR_HIST * sizeof(double), h->d_planes[h->cur].p, row, row, (size_t)ht,
                          hipMemcpyDeviceToHost));
    return RTR_OK;
}

int rtr_accum_denoise_temporal(rtr_context* c, rtr_accum* a, rtr_history* hist, const rtr_denoise_params* prm,
                               const rtr_temporal_params* tp, double* h_linear, int64_t row_stride, uint8_t* h_rgb8) {
    if (!c) return RTR_ERR_INVALID;
    if (!hist) return fail(c, RTR_ERR_INVALID, "null history");
    return accum_denoise(c, a, prm, hist, tp, DenoiseOut{h_linear, row_stride, h_rgb8, false, 1});
}

int rtr_accum_denoise_temporal_device(rtr_context* c, rtr_accum* a, rtr_history* hist, const rtr_denoise_params* prm,
                                      const rtr_temporal_params* tp, double* d_linear, int64_t row_stride, uint8_t* d_rgb8,
                                      int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (!hist) return fail(c, RTR_ERR_INVALID, "null history");
    return accum_denoise(c, a, prm, hist, tp, DenoiseOut{d_linear, row_stride, d_rgb8, true, blocking});
}

} /* extern "C" */

/* ---- the display transform: metered exposure, tone curve, 8-bit encoding ------------------------------------------- */
namespace {

/* rtr_display_srgb_thresholds: S[b] = the inverse sRGB transfer of b / 255.0, computed once on the host.  This table, not
 * a pow on the device, defines RTR_ENCODE_SRGB. */
const double* display_srgb_table() {
    static const struct Table {
        double s[256];
        Table() {
            s[0] = 0.0;
            for (int b = 1; b < 256; ++b) {
                const double v = b / 255.0;
                s[b] = v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4);
            }
        }
    } table;
    return table.s;
}
/* c->b_display: thresholds, histogram, record */
constexpr size_t kDisplayHistOff = 256 * sizeof(double), kDisplayRecOff = kDisplayHistOff + RTR_DISPLAY_BINS * sizeof(unsigned);
constexpr size_t kDisplayBytes = kDisplayRecOff + sizeof(DisplayRec);

/* the defaults of rtr_display_defaults: conventional values (median metering, 18 % grey key), not tuned ones */
constexpr rtr_display_params kDisplayDefaults = {0, 500, RTR_TONE_CLAMP, RTR_ENCODE_GAMMA2, 1.0, 0.18, 4.0, {0.0, 0.0, 0.0, 0.0, 0.0}};

int display_size_check(rtr_context* c, int32_t w, int32_t h, const void* linear, int64_t row_stride) {
    if (w < 1 || h < 1 || (int64_t)w * h > ((int64_t)1 << 28)) return fail(c, RTR_ERR_INVALID, "image size out of range");
    if (!linear || row_stride < (int64_t)w) return fail(c, RTR_ERR_INVALID, "bad input buffer / stride");
    return RTR_OK;
}

int display_check(rtr_context* c, const rtr_display_params* p, int32_t w, int32_t h, const void* linear, int64_t row_stride,
                  const void* rgb8, const void* mapped) {
    if (!p) return fail(c, RTR_ERR_INVALID, "null display params");
    if (p->auto_exposure != 0 && p->auto_exposure != 1) return fail(c, RTR_ERR_INVALID, "auto_exposure must be 0 or 1");
    if (p->meter_permille < 1 || p->meter_permille > 1000) return fail(c, RTR_ERR_INVALID, "meter_permille must be in 1..1000");
    if (p->tone_curve < RTR_TONE_CLAMP || p->tone_curve > RTR_TONE_ACES) return fail(c, RTR_ERR_INVALID, "unknown tone curve");
    if (p->encoding != RTR_ENCODE_GAMMA2 && p->encoding != RTR_ENCODE_SRGB) return fail(c, RTR_ERR_INVALID, "unknown encoding");
    for (double v : {p->exposure, p->key, p->white})
        if (!(v > 0.0) || !std::isfinite(v)) return fail(c, RTR_ERR_INVALID, "exposure, key and white must be finite and > 0");
    for (double r : p->reserved)
        if (r != 0.0) return fail(c, RTR_ERR_INVALID, "reserved fields must be 0");
    if (int rc = display_size_check(c, w, h, linear, row_stride)) return rc;
    if (!rgb8 && !mapped) return fail(c, RTR_ERR_INVALID, "no output buffer");
    return RTR_OK;
}

DisplayK display_view(rtr_context* c, const rtr_display_params* p, int w, int h, const double* d_linear, int64_t row_stride) {
    char* base = static_cast<char*>(c->b_display.p);
    DisplayK D{};
    D.w = w, D.h = h, D.row_stride = row_stride, D.in = d_linear;
    D.srgb = reinterpret_cast<const double*>(base);
    D.hist = reinterpret_cast<unsigned*>(base + kDisplayHistOff);
    D.rec = reinterpret_cast<DisplayRec*>(base + kDisplayRecOff);
    if (p) {
        D.auto_exposure = p->auto_exposure, D.permille = p->meter_permille, D.curve = p->tone_curve, D.encoding = p->encoding;
        D.exposure = p->exposure, D.key = p->key, D.white = p->white;
    }
    return D;
}

/* the histogram of D.in into D.hist, on the stream: the grid follows the region (RTR_DISPLAY_TRIPS pixels per lane) */
int display_meter(rtr_context* c, const DisplayK& D) {
    HIPCHK(c, hipMemsetAsync(D.hist, 0, RTR_DISPLAY_BINS * sizeof(unsigned), c->stream));
    const size_t np = (size_t)D.w * D.h, per_group = (size_t)RTR_BLOCK * RTR_DISPLAY_TRIPS;
    hipLaunchKernelGGL(k_display_meter, dim3((unsigned)((np + per_group - 1) / per_group)), dim3(RTR_BLOCK), 0, c->stream, D);
    return RTR_OK;
}

/* meter (with auto exposure only), scale, apply: all on the stream, no host wait */
int display_run(rtr_context* c, const DisplayK& D) {
    if (D.auto_exposure)
        if (int rc = display_meter(c, D)) return rc;
    hipLaunchKernelGGL(k_display_scale, dim3(1), dim3(64), 0, c->stream, D);
    const size_t np = (size_t)D.w * D.h;
    hipLaunchKernelGGL(k_display_apply, dim3((unsigned)((np + RTR_BLOCK - 1) / RTR_BLOCK)), dim3(RTR_BLOCK), 0, c->stream, D);
    HIPCHK(c, hipGetLastError());
    return RTR_OK;
}

/* after the stream has been waited for */
int display_result(rtr_context* c, const DisplayK& D, rtr_display_result* out) {
    static_assert(sizeof(DisplayRec) == sizeof(rtr_display_result), "one layout");
    if (out) HIPCHK(c, hipMemcpy(out, D.rec, sizeof(DisplayRec), hipMemcpyDeviceToHost));
    return RTR_OK;
}

/* the image of a host entry in c->b_display_io: [h][w][3] doubles in, [h][w][3] doubles mapped, [h][w][3] bytes */
int display_upload(rtr_context* c, int w, int h, const double* h_linear, int64_t row_stride, double*& d_in) {
    const size_t np = (size_t)w * h, row = (size_t)w * 3 * sizeof(double);
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = ensure(c, c->b_display_io, np * (6 * sizeof(double) + 3))) return rc;
    d_in = static_cast<double*>(c->b_display_io.p);
    HIPCHK(c, hipMemcpy2D(d_in, row, h_linear, (size_t)row_stride * 3 * sizeof(double), row, (size_t)h, hipMemcpyHostToDevice));
    return RTR_OK;
}

} // namespace

int rtr::display_create(rtr_context* c) {
    if (int rc = ensure(c, c->b_display, kDisplayBytes)) return rc;
    return hipMemcpy(c->b_display.p, display_srgb_table(), 256 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? RTR_OK : RTR_ERR_DEVICE;
}

extern "C" {

void rtr_display_defaults(rtr_display_params* p) {
    if (p) *p = kDisplayDefaults;
}

void rtr_display_srgb_thresholds(double out[256]) {
    if (out) std::memcpy(out, display_srgb_table(), 256 * sizeof(double));
}

int rtr_display_histogram(rtr_context* c, int32_t width, int32_t height, const double* h_linear, int64_t row_stride,
                          uint32_t h_hist[512], int64_t* n_metered) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_size_check(c, width, height, h_linear, row_stride)) return rc;
    if (!h_hist) return fail(c, RTR_ERR_INVALID, "no output buffer");
    double* d_in = nullptr;
    if (int rc = display_upload(c, width, height, h_linear, row_stride, d_in)) return rc;
    const DisplayK D = display_view(c, nullptr, width, height, d_in, width);
    if (int rc = display_meter(c, D)) return rc;
    HIPCHK(c, hipGetLastError());
    uint32_t hist[RTR_DISPLAY_BINS];
    HIPCHK(c, hipMemcpyAsync(hist, D.hist, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t n = 0;
    for (int m = 0; m < RTR_DISPLAY_BINS; ++m) h_hist[m] = hist[m], n += hist[m];
    if (n_metered) *n_metered = n;
    return RTR_OK;
}

int rtr_display_host(rtr_context* c, const rtr_display_params* p, int32_t width, int32_t height, const double* h_linear,
                     int64_t row_stride, uint8_t* h_rgb8, double* h_mapped, rtr_display_result* result) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_check(c, p, width, height, h_linear, row_stride, h_rgb8, h_mapped)) return rc;
    double* d_in = nullptr;
    if (int rc = display_upload(c, width, height, h_linear, row_stride, d_in)) return rc;
    const size_t np = (size_t)width * height;
    DisplayK D = display_view(c, p, width, height, d_in, width);
    if (h_mapped) D.mapped = d_in + 3 * np;
    if (h_rgb8) D.rgb8 = reinterpret_cast<unsigned char*>(d_in + 6 * np);
    if (int rc = display_run(c, D)) return rc;
    if (h_mapped) HIPCHK(c, hipMemcpyAsync(h_mapped, D.mapped, 3 * np * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_rgb8) HIPCHK(c, hipMemcpyAsync(h_rgb8, D.rgb8, 3 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return display_result(c, D, result);
}

int rtr_display_device(rtr_context* c, const rtr_display_params* p, int32_t width, int32_t height, const double* d_linear,
                       int64_t row_stride, uint8_t* d_rgb8, double* d_mapped, rtr_display_result* h_result, int blocking) {
    if (!c) return RTR_ERR_INVALID;
    if (int rc = display_check(c, p, width, height, d_linear, row_stride, d_rgb8, d_mapped)) return rc;
    if (h_result && !blocking) return fail(c, RTR_ERR_INVALID, "a result needs a blocking call");
    HIPCHK(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    DisplayK D = display_view(c, p, width, height, d_linear, row_stride);
    D.mapped = d_mapped, D.rgb8 = d_rgb8;
    if (int rc = display_run(c, D)) return rc;
    if (!blocking) return RTR_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return display_result(c, D, h_result);
}

} /* extern "C" */
