/*
 * rtr_cli.cpp -- headless driver in the shape of the reference's main.cpp:49-153 without the
 * SDL window: scene id and integrator id as the first two arguments (main.cpp:54-59), plus the
 * overrides the BASELINE configurations need (--width --spp --seed --out).  It is the
 * reference-side usage of the host layer: select_scene -> camera -> Renderer::render -> file.
 *
 *   rtr_cli <scene 7|9|21|22|23> <integrator 0..4> [--width W] [--spp N] [--seed S] [--bands N] [--out img.ppm|img.png]
 *           [--devices 0,1,...|all] [--repeat N]   one context + host thread per listed GPU (an ordinal may repeat)
 *           [--passes 1,4,16,...]   progressive: Renderer::render_progressive through these increasing sample counts (the
 *                                   last one replaces --spp; the image is the one --spp gives), time per pass
 *           [--adaptive THRESH [--spp-min N]]   adaptive: Renderer::render_adaptive with error threshold THRESH (a number
 *                                   or a fraction such as 1/255), spp_min N (default min(16, spp_max)) and --spp as spp_max;
 *                                   time, tiles refined and samples per pass, and the total samples against W*H*spp_max
 *           [--denoise [ITER]]   with --passes, --adaptive or a plain --spp (then one accumulator pass): the image after the
 *                                   last pass is denoised (include/rtr_hip.h: rtr_accum_denoise, the library's defaults;
 *                                   ITER in 0..10 replaces their iteration count); prints the denoise time
 *           [--turntable N [--temporal]]   N frames of a camera orbiting `lookat` about the world y axis (frame k at angle
 *                                   2 pi k / N), ONE upload: per frame rtr_set_camera, rtr_accum_reset with seed + k, the passes
 *                                   of --passes (or one to --spp), and with --denoise the filter -- with --temporal (implies
 *                                   --denoise) the temporal form over one history.  Every frame stays on the device: the
 *                                   passes, rtr_accum_resolve_device / _denoise_device / _denoise_temporal_device and, with the
 *                                   display options below, rtr_display_device are queued on the context stream, and only the
 *                                   frame's bytes come back.  Frames go to out_000.ppm ... (from --out out.ppm); first device
 *                                   of --devices only; time per frame
 *           [--pick i,j]   nothing is rendered: the closest hit of pixel (i, j)'s centre ray -- u = (i + 0.5) / (W - 1),
 *                                   v = (j + 0.5) / (H - 1), no lens offset, time0 -- through Renderer::closest_hits, as one line
 *                                   `hit front_face material t p n` with the doubles as %.17g
 *           [--ao N [--ao-distance D]]   nothing is path-traced: the pixel-centre ray of every pixel (the ray of --pick) goes
 *                                   through Renderer::closest_hits, then Renderer::ambient_occlusion casts N hemisphere rays
 *                                   of length D (default: unbounded) at every hit's (p, n); a pixel is count / N grey, 1.0
 *                                   where the centre ray misses, stored like a render.  Not with --pick, --adaptive, --turntable
 *           [--capture x,y,z --capture-out file.hdr [--face S] [--capture-spp N] [--latlong W,H] [--capture-levels L]]   nothing is path-traced per
 *                                   pixel: Renderer::capture_cube makes a cube map of 6 x S x S texels (default 32), N
 *                                   (default 16) jittered rays each, of what surrounds the point under the integrator
 *                                   and --seed, and Renderer::save_environment writes it as a W x H (default 4S x 2S)
 *                                   equirectangular Radiance .hdr file, the map an EnvironmentLight reads.  With
 *                                   --capture-levels L (1..13) Renderer::prefilter_cube makes the chain of L GGX-filtered
 *                                   levels (S <= 512 for L > 1) and every level is written at W x H: file.hdr is level 0,
 *                                   file.L<i>.hdr level i
 *           [--probes NX,NY,NZ --probe-box x0,y0,z0,x1,y1,z1 [--probe-samples N]]   nothing is path-traced per pixel: a grid of
 *                                   NX x NY x NZ light probes whose first and last stand on the box corners (an axis with one
 *                                   probe: at the lower corner) goes through Renderer::light_probes with N (default 64) sphere
 *                                   samples each under the integrator and --seed; one line per probe, x fastest: `valid count`
 *                                   and the 27 coefficients c[i][channel] as %.17g.  Not with --pick, --ao, --adaptive, --turntable
 *           [--probe-depth T [--probe-depth-samples N] --probe-depth-out FILE]   with --probes: the probes' octahedral distance
 *                                   maps of T x T texels (1..64) go through Renderer::probe_depth with N (default 8) rays per
 *                                   texel under --seed, misses at 1.5 x the length of the grid's spacing; FILE receives the raw
 *                                   rtr_probe_depth_texel records, [probe][row][column].  What is printed does not change
 *           [--brdf-table NMU,NROUGH [--brdf-nodes M] --brdf-out FILE]   the environment BRDF table of the split sum
 *                                   (Renderer::brdf_table: NMU x NROUGH entries, 1..256 each, M = 1..256 quadrature nodes per
 *                                   axis, default 128); FILE receives little-endian doubles [n_rough][n_mu][2] = (a, b).
 *                                   Needs no scene and renders nothing; excludes every other mode
 *           [--preview K]           the baked preview (Renderer::render_preview: K x K rays per pixel, 1..8) instead of a path
 *                                   traced image.  Goes together with --probes NX,NY,NZ --probe-box ... [--probe-depth T],
 *                                   --capture x,y,z --capture-levels L (L >= 1) and --brdf-table NMU,NROUGH: the three parts are
 *                                   baked as those options say (nothing of them is printed or written: --capture-out,
 *                                   --probe-depth-out and --brdf-out are not needed), the frame is shaded from them and stored
 *                                   to --out like a render.  A missing part is an error.  Not with --pick, --ao, --adaptive,
 *                                   --turntable
 *           [--capture-set FILE [--capture-fallback K]]   with --preview, in the place of --capture x,y,z: a capture set
 *                                   (include/rtr_hip.h: CAPTURE SETS).  FILE is text, one volume per line: sixteen numbers in
 *                                   struct order (centre, proxy_lo, proxy_hi, reach_lo, reach_hi: three each; fade), separated
 *                                   by blanks or commas; `#` starts a comment; 1..16 volumes.  Renderer::capture_set bakes one
 *                                   capture per volume with --face, --capture-spp and --capture-levels, and the frame's
 *                                   reflections are box-projected and blended (rtr_preview_set).  K (default -1: none) is the
 *                                   capture read where no volume reaches.  A malformed file or a set that breaks a rule is
 *                                   refused before anything touches the device
 *           [--tonemap clamp|reinhard|aces] [--auto-exposure] [--exposure X] [--key X] [--white X] [--srgb]
 *                                   any of these: the file holds the bytes of the display transform (include/rtr_hip.h:
 *                                   rtr_display_host through Renderer::display; with --turntable rtr_display_device on
 *                                   every frame) of the finished image instead of the reference's store; prints the scale
 *                                   used (not per --turntable frame: nothing waits for it).  Not with --pick
 */
#include "rtr_renderer.h"

/* --turntable owns the frame's device buffers (the library takes raw device pointers).  The six HIP runtime calls it
 * needs, declared here: hip/hip_runtime_api.h declares a global `texture` template, which the reference's class `texture`
 * (texture.h) cannot share a translation unit with.  hipError_t is an int-sized enum, hipSuccess is 0. */
extern "C" {
int hipSetDevice(int device);
int hipMalloc(void** ptr, size_t bytes);
int hipFree(void* ptr);
int hipMemset(void* dst, int value, size_t bytes);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
int hipDeviceSynchronize(void);
}
static const int hipSuccess = 0, hipMemcpyDeviceToHost = 2;

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

/* --turntable: the device form of the frame loop of INTEGRATION.md section 4 on the C ABI itself: per frame everything is
 * queued, then one wait and one copy of the bytes.  `dp`: the display transform takes the place of the reference's store.
 * Returns the exit status. */
static int turntable(const SceneConfig& config, int device, int frames, int integrator_id, unsigned seed, std::vector<int> passes,
                     const rtr_denoise_params* dn, bool temporal, const rtr_display_params* dp, const std::string& out) {
    const int W = config.image_width, H = static_cast<int>(W / config.aspect_ratio);
    auto camera_of = [&](int k) {
        const double a = 2.0 * 3.14159265358979323846 * k / frames, ca = std::cos(a), sa = std::sin(a);
        const vec3 d = config.lookfrom - config.lookat;
        const point3 from = config.lookat + vec3(ca * d[0] + sa * d[2], d[1], -sa * d[0] + ca * d[2]);
        return camera(from, config.lookat, config.vup, config.vfov, config.aspect_ratio, config.aperture, config.focus_dist, 0.0, 1.0);
    };
    rtr_context* ctx = nullptr;
    if (rtr_create(device, &ctx) != RTR_OK) {
        std::cerr << "rtr_create: " << rtr_last_error(nullptr) << "\n";
        return 1;
    }
    double* d_lin = nullptr; /* [H][W][3] linear radiance, only in front of the display transform */
    uint8_t* d_rgb = nullptr; /* [H][W][3] the frame's bytes, top row first */
    auto fail = [&](const char* what) {
        std::cerr << what << ": " << rtr_last_error(ctx) << "\n";
        rtr_destroy(ctx); /* frees the accumulator and the history (and waits for queued work) */
        (void)hipFree(d_lin);
        (void)hipFree(d_rgb);
        return 1;
    };
    rtr_scene_storage st;
    std::string err;
    if (!rtr::flatten(*config.world, config.lights, camera_of(0), config.background, st, err)) {
        std::cerr << "flatten: " << err << "\n";
        rtr_destroy(ctx);
        return 1;
    }
    rtr_scene_desc d = st.desc();
    if (rtr_upload_scene(ctx, &d) != RTR_OK) return fail("rtr_upload_scene");
    rtr_render_params p{};
    p.image_width = W, p.image_height = H, p.x1 = W, p.y1 = H;
    p.spp = 1, p.max_depth = 50, p.rr_start_depth = 3, p.integrator = integrator_id, p.seed = seed, p.spp_chunks = 1;
    rtr_accum* acc = nullptr;
    rtr_history* hist = nullptr;
    if (rtr_accum_create_ex(ctx, &p, dn ? RTR_ACCUM_MOMENTS : 0u, &acc) != RTR_OK) return fail("rtr_accum_create_ex");
    if (temporal && rtr_history_create(ctx, &p, &hist) != RTR_OK) return fail("rtr_history_create");
    rtr_temporal_params tp{};
    rtr_temporal_defaults(&tp);
    std::vector<unsigned char> rgb((size_t)W * H * 3);
    if (hipSetDevice(device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_rgb), rgb.size()) != hipSuccess ||
        hipMemset(d_rgb, 0, rgb.size()) != hipSuccess ||
        (dp && (hipMalloc(reinterpret_cast<void**>(&d_lin), rgb.size() * sizeof(double)) != hipSuccess ||
                hipMemset(d_lin, 0, rgb.size() * sizeof(double)) != hipSuccess)) ||
        hipDeviceSynchronize() != hipSuccess) /* the fills are not on the context's stream */
        return fail("device buffers of a frame (the HIP runtime, not the library)");
    const size_t dot = out.rfind('.');
    const std::string stem = dot == std::string::npos ? out : out.substr(0, dot);
    for (int k = 0; k < frames; ++k) {
        const auto t0 = std::chrono::high_resolution_clock::now();
        const rtr_camera cam = camera_of(k).rtr_flatten();
        if (rtr_set_camera(ctx, &cam) != RTR_OK) return fail("rtr_set_camera");
        if (rtr_accum_reset(ctx, acc, seed + (unsigned)k) != RTR_OK) return fail("rtr_accum_reset");
        for (int target : passes)
            if (rtr_accum_render(ctx, acc, target, 0) != RTR_OK) return fail("rtr_accum_render");
        uint8_t* const store = dp ? nullptr : d_rgb; /* the reference's store, unless the display transform follows */
        const int rc = temporal ? rtr_accum_denoise_temporal_device(ctx, acc, hist, dn, &tp, d_lin, W, store, 0)
                       : dn     ? rtr_accum_denoise_device(ctx, acc, dn, d_lin, W, store, 0)
                                : rtr_accum_resolve_device(ctx, acc, d_lin, W, store, 0);
        if (rc != RTR_OK) return fail("frame output");
        if (dp && rtr_display_device(ctx, dp, W, H, d_lin, W, d_rgb, nullptr, nullptr, 0) != RTR_OK) return fail("rtr_display_device");
        if (rtr_synchronize(ctx) != RTR_OK) return fail("rtr_synchronize");
        if (hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost) != hipSuccess) return fail("copy of the frame's bytes");
        const double ms = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count() * 1e3;
        std::cout << "frame " << k << ": " << ms << " ms\n";
        if (!out.empty()) {
            char name[32];
            std::snprintf(name, sizeof name, "_%03d.ppm", k);
            FILE* f = std::fopen((stem + name).c_str(), "wb");
            if (!f) return fail("cannot write a frame");
            std::fprintf(f, "P6\n%d %d\n255\n", W, H);
            const bool ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
            if (std::fclose(f) != 0 || !ok) return fail("cannot write a frame");
        }
    }
    std::cout << "turntable: " << frames << " frames, scene uploads: 1\n";
    rtr_destroy(ctx);
    (void)hipFree(d_lin);
    (void)hipFree(d_rgb);
    return 0;
}

/* a finite number > 0 and nothing else */
static bool parse_positive(const char* s, double& out) {
    char* end = nullptr;
    const double v = std::strtod(s, &end);
    if (end == s || *end != '\0' || !(v > 0.0) || !std::isfinite(v)) return false;
    out = v;
    return true;
}

/* "0.004" or "1/255"; false unless the whole string is such a number */
static bool parse_threshold(const char* s, double& out) {
    char* end = nullptr;
    double v = std::strtod(s, &end);
    if (end == s) return false;
    if (*end == '/') {
        const char* d = end + 1;
        const double den = std::strtod(d, &end);
        if (end == d || den == 0.0) return false;
        v /= den;
    }
    out = v;
    return *end == '\0';
}

int main(int argc, char** argv) {
    int scene_id = 21, integrator_id = 4, width = 0, spp = 0, bands = 0, repeat = 1, spp_min = 0;
    bool adaptive = false, denoise = false, pick = false, temporal = false, display = false;
    rtr_display_params dp{};
    rtr_display_defaults(&dp);
    int turntable_frames = 0;
    int pick_i = 0, pick_j = 0;
    int denoise_iter = -1, ao_samples = 0;
    double threshold = 0.0, ao_distance = 0.0; /* 0: unbounded */
    int probe_dims[3] = {0, 0, 0}, probe_samples = 64;
    double probe_box[6];
    bool probes = false, probe_boxed = false, probe_sampled = false;
    int probe_depth = 0, probe_depth_samples = 8;
    bool probe_depth_set = false, probe_depth_sampled = false;
    std::string probe_depth_out;
    int brdf_dims[2] = {0, 0}, brdf_nodes = 128;
    bool brdf = false, brdf_noded = false;
    std::string brdf_out;
    double capture_at[3] = {0, 0, 0};
    int capture_face = 32, capture_spp = 16, latlong[2] = {0, 0}, capture_levels = 0;
    bool capture = false, capture_face_set = false, capture_spp_set = false, latlong_set = false;
    std::string capture_out;
    int preview = 0; /* --preview K */
    std::vector<rtr_capture_volume> set_volumes; /* --capture-set FILE */
    bool capture_set = false, capture_fallback_set = false;
    int capture_fallback = -1;
    std::vector<int> devices{0}, passes;
    unsigned seed = 1;
    std::string out;
    int pos = 0;
    for (int k = 1; k < argc; ++k) {
        if (!std::strcmp(argv[k], "--width") && k + 1 < argc) width = std::atoi(argv[++k]);
        else if (!std::strcmp(argv[k], "--spp") && k + 1 < argc) spp = std::atoi(argv[++k]);
        else if (!std::strcmp(argv[k], "--seed") && k + 1 < argc) seed = (unsigned)std::strtoul(argv[++k], nullptr, 0);
        else if (!std::strcmp(argv[k], "--out") && k + 1 < argc) out = argv[++k];
        else if (!std::strcmp(argv[k], "--bands") && k + 1 < argc) bands = std::atoi(argv[++k]);
        else if (!std::strcmp(argv[k], "--repeat") && k + 1 < argc) repeat = std::atoi(argv[++k]);
        else if (!std::strcmp(argv[k], "--adaptive") && k + 1 < argc) {
            adaptive = true;
            if (!parse_threshold(argv[++k], threshold) || !(threshold > 0.0) || !std::isfinite(threshold)) {
                std::cerr << "--adaptive: the threshold must be a finite number > 0, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--denoise")) {
            denoise = true;
            if (k + 1 < argc && std::strncmp(argv[k + 1], "--", 2) != 0) {
                char* end = nullptr;
                const long v = std::strtol(argv[++k], &end, 10);
                if (end == argv[k] || *end != '\0' || v < 0 || v > 10) {
                    std::cerr << "--denoise: ITER must be an integer in 0..10, not " << argv[k] << "\n";
                    return 2;
                }
                denoise_iter = (int)v;
            }
        }
        else if (!std::strcmp(argv[k], "--temporal")) temporal = true;
        else if (!std::strcmp(argv[k], "--tonemap") && k + 1 < argc) {
            const char* v = argv[++k];
            display = true;
            if (!std::strcmp(v, "clamp")) dp.tone_curve = RTR_TONE_CLAMP;
            else if (!std::strcmp(v, "reinhard")) dp.tone_curve = RTR_TONE_REINHARD;
            else if (!std::strcmp(v, "aces")) dp.tone_curve = RTR_TONE_ACES;
            else {
                std::cerr << "--tonemap takes clamp, reinhard or aces, not " << v << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--auto-exposure")) display = true, dp.auto_exposure = 1;
        else if (!std::strcmp(argv[k], "--srgb")) display = true, dp.encoding = RTR_ENCODE_SRGB;
        else if ((!std::strcmp(argv[k], "--exposure") || !std::strcmp(argv[k], "--key") || !std::strcmp(argv[k], "--white")) && k + 1 < argc) {
            double& field = argv[k][2] == 'e' ? dp.exposure : argv[k][2] == 'k' ? dp.key : dp.white;
            display = true;
            if (!parse_positive(argv[k + 1], field)) {
                std::cerr << argv[k] << " takes a finite number > 0, not " << argv[k + 1] << "\n";
                return 2;
            }
            ++k;
        }
        else if (!std::strcmp(argv[k], "--turntable") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > 999) {
                std::cerr << "--turntable: N must be an integer in 1..999, not " << argv[k] << "\n";
                return 2;
            }
            turntable_frames = (int)v;
        }
        else if (!std::strcmp(argv[k], "--pick") && k + 1 < argc) {
            pick = std::sscanf(argv[++k], "%d,%d", &pick_i, &pick_j) == 2;
            if (!pick) {
                std::cerr << "--pick takes a pixel as i,j, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--ao") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > (1 << 20)) {
                std::cerr << "--ao: N must be an integer in 1..1048576, not " << argv[k] << "\n";
                return 2;
            }
            ao_samples = (int)v;
        }
        else if (!std::strcmp(argv[k], "--ao-distance") && k + 1 < argc) {
            if (!parse_positive(argv[k + 1], ao_distance)) {
                std::cerr << "--ao-distance takes a finite number > 0, not " << argv[k + 1] << "\n";
                return 2;
            }
            ++k;
        }
        else if (!std::strcmp(argv[k], "--probes") && k + 1 < argc) {
            char tail = 0;
            probes = std::sscanf(argv[++k], "%d,%d,%d%c", &probe_dims[0], &probe_dims[1], &probe_dims[2], &tail) == 3;
            if (!probes || probe_dims[0] < 1 || probe_dims[1] < 1 || probe_dims[2] < 1 ||
                (long long)probe_dims[0] * probe_dims[1] * probe_dims[2] > (1ll << 24)) {
                std::cerr << "--probes takes NX,NY,NZ, each >= 1 with a product <= 16777216, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--capture") && k + 1 < argc) {
            char tail;
            capture = std::sscanf(argv[++k], "%lf,%lf,%lf%c", &capture_at[0], &capture_at[1], &capture_at[2], &tail) == 3;
            for (int a = 0; a < 3; ++a) capture = capture && std::isfinite(capture_at[a]);
            if (!capture) {
                std::cerr << "--capture takes three finite numbers x,y,z, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if ((!std::strcmp(argv[k], "--face") || !std::strcmp(argv[k], "--capture-spp")) && k + 1 < argc) {
            const bool face = !std::strcmp(argv[k], "--face");
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (!end || *end || v < 1 || v > (face ? 4096 : 1 << 20)) {
                std::cerr << argv[k - 1] << ": an integer in 1.." << (face ? 4096 : 1 << 20) << ", not " << argv[k] << "\n";
                return 2;
            }
            if (face) capture_face = (int)v, capture_face_set = true;
            else capture_spp = (int)v, capture_spp_set = true;
        }
        else if (!std::strcmp(argv[k], "--capture-out") && k + 1 < argc) capture_out = argv[++k];
        else if (!std::strcmp(argv[k], "--brdf-table") && k + 1 < argc) {
            char tail;
            brdf = std::sscanf(argv[++k], "%d,%d%c", &brdf_dims[0], &brdf_dims[1], &tail) == 2 && brdf_dims[0] >= 1 &&
                   brdf_dims[1] >= 1 && brdf_dims[0] <= 256 && brdf_dims[1] <= 256;
            if (!brdf) {
                std::cerr << "--brdf-table takes NMU,NROUGH, each in 1..256, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--brdf-nodes") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > 256) {
                std::cerr << "--brdf-nodes takes an integer in 1..256, not " << argv[k] << "\n";
                return 2;
            }
            brdf_nodes = (int)v, brdf_noded = true;
        }
        else if (!std::strcmp(argv[k], "--brdf-out") && k + 1 < argc) brdf_out = argv[++k];
        else if (!std::strcmp(argv[k], "--preview") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > 8) {
                std::cerr << "--preview takes the rays per pixel axis K, an integer in 1..8, not " << argv[k] << "\n";
                return 2;
            }
            preview = (int)v;
        }
        else if (!std::strcmp(argv[k], "--capture-set") && k + 1 < argc) {
            std::ifstream f(argv[++k]);
            if (!f) {
                std::cerr << "--capture-set: cannot read " << argv[k] << "\n";
                return 2;
            }
            std::string line;
            for (int no = 1; std::getline(f, line); ++no) {
                line = line.substr(0, line.find('#'));
                for (char& ch : line)
                    if (ch == ',') ch = ' ';
                std::istringstream in(line);
                double v[17];
                int got = 0;
                std::string word;
                bool ok = true;
                while (in >> word) {
                    char* end = nullptr;
                    const double x = std::strtod(word.c_str(), &end);
                    if (end == word.c_str() || *end != '\0' || got == 17) ok = false;
                    else v[got++] = x;
                    if (!ok) break;
                }
                if (ok && got == 0) continue; /* blank or comment */
                if (!ok || got != 16) {
                    std::cerr << "--capture-set: " << argv[k] << " line " << no << ": sixteen numbers expected (centre, proxy_lo, "
                              << "proxy_hi, reach_lo, reach_hi, fade)\n";
                    return 2;
                }
                rtr_capture_volume vol;
                std::memcpy(&vol, v, sizeof vol);
                set_volumes.push_back(vol);
            }
            if (set_volumes.empty() || set_volumes.size() > 16) {
                std::cerr << "--capture-set: " << argv[k] << " holds " << set_volumes.size() << " volumes, 1..16 expected\n";
                return 2;
            }
            capture_set = true;
        }
        else if (!std::strcmp(argv[k], "--capture-fallback") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < -1 || v > 15) {
                std::cerr << "--capture-fallback: an integer in -1..15, not " << argv[k] << "\n";
                return 2;
            }
            capture_fallback = (int)v, capture_fallback_set = true;
        }
        else if (!std::strcmp(argv[k], "--capture-levels") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (!end || *end || v < 1 || v > 13) {
                std::cerr << "--capture-levels: an integer in 1..13, not " << argv[k] << "\n";
                return 2;
            }
            capture_levels = (int)v;
        }
        else if (!std::strcmp(argv[k], "--latlong") && k + 1 < argc) {
            char tail;
            latlong_set = std::sscanf(argv[++k], "%d,%d%c", &latlong[0], &latlong[1], &tail) == 2 && latlong[0] >= 1 &&
                          latlong[1] >= 1 && latlong[0] <= 65536 && latlong[1] <= 65536;
            if (!latlong_set) {
                std::cerr << "--latlong takes W,H, each in 1..65536, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--probe-box") && k + 1 < argc) {
            char tail = 0;
            double* b = probe_box;
            probe_boxed = std::sscanf(argv[++k], "%lf,%lf,%lf,%lf,%lf,%lf%c", b, b + 1, b + 2, b + 3, b + 4, b + 5, &tail) == 6;
            for (int a = 0; a < 6; ++a) probe_boxed = probe_boxed && std::isfinite(b[a]);
            if (!probe_boxed) {
                std::cerr << "--probe-box takes six finite numbers x0,y0,z0,x1,y1,z1, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--probe-samples") && k + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > (1 << 20)) {
                std::cerr << "--probe-samples: N must be an integer in 1..1048576, not " << argv[k] << "\n";
                return 2;
            }
            probe_samples = (int)v, probe_sampled = true;
        }
        else if ((!std::strcmp(argv[k], "--probe-depth") || !std::strcmp(argv[k], "--probe-depth-samples")) && k + 1 < argc) {
            const bool size = !std::strcmp(argv[k], "--probe-depth");
            const long most = size ? 64 : (1 << 20);
            char* end = nullptr;
            const long v = std::strtol(argv[++k], &end, 10);
            if (end == argv[k] || *end != '\0' || v < 1 || v > most) {
                std::cerr << argv[k - 1] << " takes an integer in 1.." << most << ", not " << argv[k] << "\n";
                return 2;
            }
            if (size) probe_depth = (int)v, probe_depth_set = true;
            else probe_depth_samples = (int)v, probe_depth_sampled = true;
        }
        else if (!std::strcmp(argv[k], "--probe-depth-out") && k + 1 < argc) probe_depth_out = argv[++k];
        else if (!std::strcmp(argv[k], "--spp-min") && k + 1 < argc) {
            spp_min = std::atoi(argv[++k]);
            if (spp_min < 1) {
                std::cerr << "--spp-min must be >= 1, not " << argv[k] << "\n";
                return 2;
            }
        }
        else if (!std::strcmp(argv[k], "--passes") && k + 1 < argc) {
            const std::string v = argv[++k];
            for (size_t a = 0; a < v.size();) {
                size_t b = v.find(',', a);
                if (b == std::string::npos) b = v.size();
                passes.push_back(std::atoi(v.substr(a, b - a).c_str()));
                a = b + 1;
            }
        }
        else if (!std::strcmp(argv[k], "--devices") && k + 1 < argc) {
            const std::string v = argv[++k];
            devices.clear();
            if (v == "all") devices = Renderer::all_devices();
            else
                for (size_t a = 0; a < v.size();) {
                    size_t b = v.find(',', a);
                    if (b == std::string::npos) b = v.size();
                    devices.push_back(std::atoi(v.substr(a, b - a).c_str()));
                    a = b + 1;
                }
        }
        else if (pos == 0) scene_id = std::atoi(argv[k]), ++pos;
        else if (pos == 1) integrator_id = std::atoi(argv[k]), ++pos;
    }
    if (spp_min && !adaptive) {
        std::cerr << "--spp-min goes with --adaptive\n";
        return 2;
    }
    if (adaptive && !passes.empty()) {
        std::cerr << "--adaptive and --passes exclude each other\n";
        return 2;
    }
    if (adaptive && spp_min && spp > 0 && spp < spp_min) {
        std::cerr << "--adaptive: --spp (the maximum) must be >= --spp-min\n";
        return 2;
    }
    if (temporal && !turntable_frames) {
        std::cerr << "--temporal goes with --turntable\n";
        return 2;
    }
    if (turntable_frames && (adaptive || repeat != 1 || pick)) {
        std::cerr << "--turntable excludes --adaptive, --repeat and --pick\n";
        return 2;
    }
    if (ao_distance > 0.0 && !ao_samples) {
        std::cerr << "--ao-distance goes with --ao\n";
        return 2;
    }
    if (ao_samples && (pick || adaptive || turntable_frames)) {
        std::cerr << "--ao excludes --pick, --adaptive and --turntable\n";
        return 2;
    }
    if ((probe_boxed || probe_sampled) && !probes) {
        std::cerr << "--probe-box and --probe-samples go with --probes\n";
        return 2;
    }
    if (probes && !probe_boxed) {
        std::cerr << "--probes needs --probe-box\n";
        return 2;
    }
    if ((probe_depth_set || probe_depth_sampled || !probe_depth_out.empty()) && !probes) {
        std::cerr << "--probe-depth, --probe-depth-samples and --probe-depth-out go with --probes\n";
        return 2;
    }
    if (preview) { /* the three parts of the bake go together here, and nothing of them is written */
        const char* missing = !probes ? "--probes NX,NY,NZ --probe-box x0,y0,z0,x1,y1,z1 (the probe grid)"
                              : !(capture || capture_set) || capture_levels < 1
                                  ? "--capture x,y,z (or --capture-set FILE) --capture-levels L (the cube chain)"
                              : !brdf ? "--brdf-table NMU,NROUGH (the table)" : nullptr;
        if (missing) {
            std::cerr << "--preview needs " << missing << "\n";
            return 2;
        }
        if (pick || ao_samples || adaptive || turntable_frames) {
            std::cerr << "--preview excludes --pick, --ao, --adaptive and --turntable\n";
            return 2;
        }
        if (out.empty()) {
            std::cerr << "--preview needs --out FILE\n";
            return 2;
        }
    }
    if (!preview && (probe_depth_set != !probe_depth_out.empty() || (probe_depth_sampled && !probe_depth_set))) {
        std::cerr << "--probe-depth T and --probe-depth-out FILE go together; --probe-depth-samples goes with them\n";
        return 2;
    }
    if (probes && (pick || ao_samples || adaptive || turntable_frames)) {
        std::cerr << "--probes excludes --pick, --ao, --adaptive and --turntable\n";
        return 2;
    }
    if (probes)
        for (int a = 0; a < 3; ++a)
            if (probe_dims[a] > 1 && !(probe_box[3 + a] > probe_box[a])) {
                std::cerr << "--probe-box: the upper corner must lie above the lower one on every axis with more than one probe\n";
                return 2;
            }
    if (capture_fallback_set && !capture_set) {
        std::cerr << "--capture-fallback goes with --capture-set\n";
        return 2;
    }
    if (capture_set) {
        if (!preview || capture || !capture_out.empty() || latlong_set) {
            std::cerr << "--capture-set goes with --preview and takes the place of --capture; --capture-out and --latlong do not apply\n";
            return 2;
        }
        /* the rules of a set (include/rtr_hip.h), asked of the library's host-only lookup over a chain of one texel per face */
        const rtr_capture_set set{(int32_t)set_volumes.size(), capture_fallback, set_volumes.data()};
        const rtr_cube_level one{1, 0, 0, 0.0};
        const std::vector<rtr_gather_out> texels(6 * set_volumes.size());
        const rtr_capture_query q{{0, 0, 0}, {0, 0, 1}, 0.0, 0.0};
        rtr_gather_out o;
        if (rtr_capture_set_lookup_one(&set, &one, 1, texels.data(), &q, &o) != RTR_OK) {
            std::cerr << "--capture-set: not a capture set: every number finite, proxy_lo < centre < proxy_hi, proxy_lo <= reach_lo <= "
                      << "reach_hi <= proxy_hi, fade >= 0, --capture-fallback below the number of volumes\n";
            return 2;
        }
    }
    if ((capture_face_set || capture_spp_set || !capture_out.empty() || latlong_set || capture_levels) && !capture && !capture_set) {
        std::cerr << "--face, --capture-spp, --capture-out, --latlong and --capture-levels go with --capture\n";
        return 2;
    }
    if (capture_levels > 1 && capture_face > 512) {
        std::cerr << "--capture-levels above 1 needs --face of at most 512\n";
        return 2;
    }
    if (capture && capture_out.empty() && !preview) {
        std::cerr << "--capture needs --capture-out file.hdr\n";
        return 2;
    }
    if (capture && ((probes && !preview) || pick || ao_samples || adaptive || turntable_frames)) {
        std::cerr << "--capture excludes --probes, --pick, --ao, --adaptive and --turntable\n";
        return 2;
    }
    if (capture && !latlong_set) latlong[0] = 4 * capture_face, latlong[1] = 2 * capture_face;
    if ((!preview && brdf != !brdf_out.empty()) || (brdf_noded && !brdf)) {
        std::cerr << "--brdf-table NMU,NROUGH and --brdf-out FILE go together; --brdf-nodes goes with them\n";
        return 2;
    }
    if (brdf && !preview && (capture || probes || pick || ao_samples || adaptive || turntable_frames)) {
        std::cerr << "--brdf-table excludes --capture, --probes, --pick, --ao, --adaptive and --turntable\n";
        return 2;
    }
    if (display && pick) {
        std::cerr << "the display options exclude --pick\n";
        return 2;
    }
    if (temporal) denoise = true;
    if (denoise && repeat != 1) {
        std::cerr << "--denoise takes one render (--repeat 1)\n";
        return 2;
    }
    rtr_denoise_params dn{};
    rtr_denoise_defaults(&dn);
    if (denoise_iter >= 0) dn.iterations = denoise_iter;
    rtr::rng_state() = 12345u; /* scene-construction seed */
    SceneConfig config;
    try {
        config = select_scene(scene_id);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 2;
    }
    if (width > 0) config.image_width = width;
    if (spp > 0) config.samples_per_pixel = spp;
    if (!passes.empty()) config.samples_per_pixel = passes.back();
    if (adaptive && spp_min > config.samples_per_pixel) {
        std::cerr << "--adaptive: the scene's " << config.samples_per_pixel << " spp (the maximum) is below --spp-min\n";
        return 2;
    }
    if (adaptive && !spp_min) spp_min = std::min(16, config.samples_per_pixel);
    if (turntable_frames) {
        for (size_t k = 0; k < passes.size(); ++k)
            if (passes[k] < 1 || (k && passes[k] <= passes[k - 1])) {
                std::cerr << "--passes: increasing sample counts >= 1\n";
                return 2;
            }
        if (passes.empty()) passes.push_back(config.samples_per_pixel);
        return turntable(config, devices.empty() ? 0 : devices[0], turntable_frames, integrator_id < 0 || integrator_id > 4 ? 4 : integrator_id,
                         seed, passes, denoise ? &dn : nullptr, temporal, display ? &dp : nullptr, out);
    }
    auto cam = make_shared<camera>(config.lookfrom, config.lookat, config.vup, config.vfov, config.aspect_ratio,
                                   config.aperture, config.focus_dist, 0.0, 1.0); /* main.cpp:63-66 */
    const int W = config.image_width, H = static_cast<int>(W / config.aspect_ratio);
    RenderBuffer buffer(W, H);
    Renderer renderer(devices);
    if (brdf && !preview) {
        const std::vector<rtr_brdf_entry> table = renderer.brdf_table(brdf_dims[0], brdf_dims[1], brdf_nodes);
        if (table.size() != (size_t)brdf_dims[0] * brdf_dims[1]) {
            std::cerr << "brdf table failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::FILE* f = std::fopen(brdf_out.c_str(), "wb");
        const bool ok = f && std::fwrite(table.data(), sizeof(rtr_brdf_entry), table.size(), f) == table.size();
        if (!(f && std::fclose(f) == 0 && ok)) {
            std::cerr << "cannot write " << brdf_out << "\n";
            return 1;
        }
        std::cout << "brdf table: " << brdf_dims[1] << " x " << brdf_dims[0] << " entries, " << brdf_nodes << " nodes per axis -> "
                  << brdf_out << "\n";
        return 0;
    }
    if (pick) {
        if (pick_i < 0 || pick_i >= W || pick_j < 0 || pick_j >= H) {
            std::cerr << "--pick: pixel outside the " << W << " x " << H << " image\n";
            return 2;
        }
        if (renderer.upload_scene(config.world, cam, config.background, config.lights) != RTR_OK) {
            std::cerr << "upload failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        const double u = (pick_i + 0.5) / (W - 1), v = (pick_j + 0.5) / (H - 1);
        const ray r(cam->origin, cam->lower_left_corner + u * cam->horizontal + v * cam->vertical - cam->origin, cam->time0);
        const std::vector<rtr_ray_hit> hits = renderer.closest_hits({r});
        if (hits.size() != 1) {
            std::cerr << "query failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        const rtr_ray_hit& h = hits[0];
        std::printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", h.hit, h.front_face, h.material, h.t, h.p[0], h.p[1],
                    h.p[2], h.n[0], h.n[1], h.n[2]);
        return 0;
    }
    if (ao_samples) {
        if (renderer.upload_scene(config.world, cam, config.background, config.lights) != RTR_OK) {
            std::cerr << "upload failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::vector<ray> centres;
        centres.reserve((size_t)W * H);
        for (int j = 0; j < H; ++j)
            for (int i = 0; i < W; ++i) {
                const double u = (i + 0.5) / (W - 1), v = (j + 0.5) / (H - 1);
                centres.emplace_back(cam->origin, cam->lower_left_corner + u * cam->horizontal + v * cam->vertical - cam->origin, cam->time0);
            }
        const std::vector<rtr_ray_hit> hits = renderer.closest_hits(centres);
        if (hits.size() != centres.size()) {
            std::cerr << "query failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::vector<point3> points;
        std::vector<vec3> normals;
        for (const rtr_ray_hit& h : hits)
            if (h.hit) points.emplace_back(h.p[0], h.p[1], h.p[2]), normals.emplace_back(h.n[0], h.n[1], h.n[2]);
        const std::vector<rtr_gather_out> ao = renderer.ambient_occlusion(points, normals, ao_samples, ao_distance > 0.0 ? ao_distance : infinity);
        if (ao.size() != points.size()) {
            std::cerr << "ambient occlusion failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::vector<double> lin((size_t)W * H * 3);
        size_t next = 0;
        for (size_t k = 0; k < hits.size(); ++k) {
            const double g = hits[k].hit ? (double)ao[next++].count / ao_samples : 1.0;
            lin[3 * k] = lin[3 * k + 1] = lin[3 * k + 2] = g;
        }
        buffer.store_linear_rows(lin.data(), 0, H, W);
        std::cout << "ambient occlusion: " << points.size() << " points x " << ao_samples << " samples\n";
        const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
        if (!out.empty() && !(png ? buffer.save_to_png(out) : buffer.save_to_ppm(out))) {
            std::cerr << "Failed to save image to " << out << "\n";
            return 1;
        }
        return 0;
    }
    renderer.set_samples(config.samples_per_pixel);
    switch (integrator_id) { /* main.cpp:80-100 */
    case 0: renderer.set_integrator(make_shared<PathIntegrator>()); break;
    case 1: renderer.set_integrator(make_shared<RRPathInterator>()); break;
    case 2: renderer.set_integrator(make_shared<PBRPathIntegrator>()); break;
    case 3: renderer.set_integrator(make_shared<DirectLightIntegrator>()); break;
    default: renderer.set_integrator(make_shared<MISPathIntegrator>()); break;
    }
    renderer.set_max_depth(50); /* main.cpp:102 */
    renderer.set_seed(seed);
    renderer.set_progress_bands(bands);
    if (preview) {
        if (renderer.upload_scene(config.world, cam, config.background, config.lights) != RTR_OK) {
            std::cerr << "upload failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        const auto failed = [&](const char* what) {
            std::cerr << what << " failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        };
        /* the grid of --probes: probe (ix, iy, iz) at the lower corner + (ix, iy, iz) * spacing */
        rtr_probe_grid grid{};
        for (int a = 0; a < 3; ++a) {
            grid.origin[a] = probe_box[a], grid.dims[a] = probe_dims[a];
            grid.spacing[a] = probe_dims[a] > 1 ? (probe_box[3 + a] - probe_box[a]) / (double)(probe_dims[a] - 1) : 1.0;
        }
        std::vector<point3> points;
        for (int iz = 0; iz < probe_dims[2]; ++iz)
            for (int iy = 0; iy < probe_dims[1]; ++iy)
                for (int ix = 0; ix < probe_dims[0]; ++ix)
                    points.emplace_back(grid.origin[0] + (double)ix * grid.spacing[0], grid.origin[1] + (double)iy * grid.spacing[1],
                                        grid.origin[2] + (double)iz * grid.spacing[2]);
        const std::vector<rtr_probe_sh> sh = renderer.light_probes(points, probe_samples, seed);
        if (sh.size() != points.size()) return failed("light probes");
        const double* sp = grid.spacing;
        std::vector<rtr_probe_depth_texel> maps;
        rtr_probe_visible_params vp{};
        if (probe_depth_set) {
            const double reach = 1.5 * std::sqrt((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]);
            maps = renderer.probe_depth(points, probe_depth, reach, probe_depth_samples, seed);
            if (maps.size() != points.size() * (size_t)probe_depth * probe_depth) return failed("probe depth");
            vp.map_size = probe_depth, vp.normal_bias = 0.25 * std::min(sp[0], std::min(sp[1], sp[2]));
        }
        std::vector<rtr_cube_level> plan;
        std::vector<rtr_gather_out> chain;
        if (capture_set) {
            chain = renderer.capture_set(set_volumes, capture_face, capture_spp, capture_levels, plan, seed);
            if (chain.empty()) return failed("capture set");
        } else {
            const std::vector<rtr_gather_out> cube =
                renderer.capture_cube({point3(capture_at[0], capture_at[1], capture_at[2])}, capture_face, capture_spp, seed);
            if (cube.empty()) return failed("capture");
            chain = renderer.prefilter_cube(cube, capture_face, capture_levels, plan);
            if (chain.empty()) return failed("prefilter");
        }
        const std::vector<rtr_brdf_entry> table = renderer.brdf_table(brdf_dims[0], brdf_dims[1], brdf_nodes);
        if (table.size() != (size_t)brdf_dims[0] * brdf_dims[1]) return failed("brdf table");
        rtr_shade_env env{};
        env.parts = RTR_SHADE_DIFFUSE | RTR_SHADE_SPECULAR;
        env.grid = &grid, env.probes = sh.data();
        if (probe_depth_set) env.depth = maps.data(), env.visible = &vp;
        env.levels = plan.data(), env.n_levels = (int32_t)plan.size(), env.chain = chain.data();
        env.n_records = (int64_t)(chain.size() / (capture_set ? set_volumes.size() : 1)); /* of one capture */
        env.table = table.data(), env.n_mu = brdf_dims[0], env.n_rough = brdf_dims[1];
        const rtr_capture_set set{(int32_t)set_volumes.size(), capture_fallback, set_volumes.data()};
        if ((capture_set ? renderer.render_preview(env, set, buffer, preview) : renderer.render_preview(env, buffer, preview)) != RTR_OK)
            return failed("preview");
        if (capture_set) std::cout << "capture set: " << set_volumes.size() << " volumes, fallback " << capture_fallback << "\n";
        std::cout << "preview: " << W << " x " << H << " pixels x " << preview * preview << " rays, " << points.size() << " probes, "
                  << capture_levels << " cube levels of face " << capture_face << ", table " << brdf_dims[1] << " x " << brdf_dims[0] << "\n";
        std::vector<unsigned char> shown;
        if (display && renderer.display(buffer, dp, shown) != RTR_OK) return failed("display");
        const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0;
        const std::vector<unsigned char>* bytes = display ? &shown : nullptr;
        if (!(png ? buffer.save_to_png(out, bytes) : buffer.save_to_ppm(out, bytes))) {
            std::cerr << "Failed to save image to " << out << "\n";
            return 1;
        }
        return 0;
    }
    if (capture) {
        if (renderer.upload_scene(config.world, cam, config.background, config.lights) != RTR_OK) {
            std::cerr << "upload failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        const std::vector<rtr_gather_out> cube =
            renderer.capture_cube({point3(capture_at[0], capture_at[1], capture_at[2])}, capture_face, capture_spp, seed);
        if (cube.empty() || !renderer.save_environment(capture_out, cube, capture_face, latlong[0], latlong[1])) {
            std::cerr << "capture failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::cout << "capture: 6 x " << capture_face << " x " << capture_face << " texels x " << capture_spp << " samples -> "
                  << capture_out << " (" << latlong[0] << " x " << latlong[1] << ")\n";
        if (capture_levels > 1) { /* level 0 is written above; the filtered levels go beside it */
            std::vector<rtr_cube_level> plan;
            const std::vector<rtr_gather_out> chain = renderer.prefilter_cube(cube, capture_face, capture_levels, plan);
            const size_t dot = capture_out.rfind(".hdr");
            const std::string stem = dot != std::string::npos && dot + 4 == capture_out.size() ? capture_out.substr(0, dot) : capture_out;
            for (int i = 1; i < capture_levels && !chain.empty(); ++i) {
                const size_t recs = 6 * (size_t)plan[i].face_size * plan[i].face_size;
                const std::vector<rtr_gather_out> level(chain.begin() + plan[i].offset, chain.begin() + plan[i].offset + recs);
                const std::string path = stem + ".L" + std::to_string(i) + ".hdr";
                if (!renderer.save_environment(path, level, plan[i].face_size, latlong[0], latlong[1])) {
                    std::cerr << "cannot write " << path << " (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
                    return 1;
                }
                std::cout << "level " << i << ": face " << plan[i].face_size << ", alpha " << plan[i].alpha << " -> " << path << "\n";
            }
            if (chain.empty()) {
                std::cerr << "prefilter failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
                return 1;
            }
        }
        return 0;
    }
    if (probes) {
        if (renderer.upload_scene(config.world, cam, config.background, config.lights) != RTR_OK) {
            std::cerr << "upload failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::vector<point3> points;
        for (int iz = 0; iz < probe_dims[2]; ++iz)
            for (int iy = 0; iy < probe_dims[1]; ++iy)
                for (int ix = 0; ix < probe_dims[0]; ++ix) {
                    const int idx[3] = {ix, iy, iz};
                    double p[3];
                    for (int a = 0; a < 3; ++a) {
                        const double sp = probe_dims[a] > 1 ? (probe_box[3 + a] - probe_box[a]) / (double)(probe_dims[a] - 1) : 1.0;
                        p[a] = probe_box[a] + (double)idx[a] * sp;
                    }
                    points.emplace_back(p[0], p[1], p[2]);
                }
        const std::vector<rtr_probe_sh> sh = renderer.light_probes(points, probe_samples, seed);
        if (sh.size() != points.size()) {
            std::cerr << "light probes failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        if (probe_depth_set) {
            double sp[3];
            for (int a = 0; a < 3; ++a)
                sp[a] = probe_dims[a] > 1 ? (probe_box[3 + a] - probe_box[a]) / (double)(probe_dims[a] - 1) : 1.0;
            const double reach = 1.5 * std::sqrt((sp[0] * sp[0] + sp[1] * sp[1]) + sp[2] * sp[2]);
            const std::vector<rtr_probe_depth_texel> maps = renderer.probe_depth(points, probe_depth, reach, probe_depth_samples, seed);
            if (maps.size() != points.size() * (size_t)probe_depth * probe_depth) {
                std::cerr << "probe depth failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
                return 1;
            }
            std::FILE* f = std::fopen(probe_depth_out.c_str(), "wb");
            const bool ok = f && std::fwrite(maps.data(), sizeof(rtr_probe_depth_texel), maps.size(), f) == maps.size();
            if (!(f && std::fclose(f) == 0 && ok)) {
                std::cerr << "cannot write " << probe_depth_out << "\n";
                return 1;
            }
        }
        for (const rtr_probe_sh& r : sh) {
            std::printf("%d %d", r.valid, r.count);
            for (int i = 0; i < 9; ++i)
                for (int ch = 0; ch < 3; ++ch) std::printf(" %.17g", r.c[i][ch]);
            std::printf("\n");
        }
        return 0;
    }
    for (int r = 0; r < repeat; ++r) { /* a second call finds the flattened scene on the GPUs */
        if (adaptive) {
            auto t = std::chrono::high_resolution_clock::now();
            long long total = 0;
            renderer.render_adaptive(config.world, cam, config.background, buffer, config.lights, threshold, spp_min,
                                     config.samples_per_pixel, [&](int pass, int active, long long samples) {
                const auto now = std::chrono::high_resolution_clock::now();
                std::cout << "adaptive pass " << pass << ": " << std::chrono::duration<double>(now - t).count() * 1e3
                          << " ms, " << active << " tiles refined, " << samples << " samples\n";
                t = now;
                total = samples;
            }, denoise ? &dn : nullptr);
            const double uniform = (double)W * H * config.samples_per_pixel;
            std::cout << "adaptive total: " << total << " samples of " << (long long)uniform << " (W*H*spp_max), "
                      << 100.0 * (double)total / uniform << " %\n";
        } else if (passes.empty() && !denoise) {
            renderer.render(config.world, cam, config.background, buffer, config.lights);
        } else {
            if (passes.empty()) passes.push_back(config.samples_per_pixel); /* --denoise: one accumulator pass */
            auto t = std::chrono::high_resolution_clock::now();
            renderer.render_progressive(config.world, cam, config.background, buffer, config.lights, passes, [&](int target) {
                const auto now = std::chrono::high_resolution_clock::now();
                std::cout << "pass to " << target << " spp: " << std::chrono::duration<double>(now - t).count() * 1e3 << " ms\n";
                t = now;
            }, denoise ? &dn : nullptr);
        }
        if (renderer.last_status() != RTR_OK) return 1;
        if (denoise)
            std::cout << "denoise: " << renderer.last_denoise_seconds() * 1e3 << " ms (" << dn.iterations << " iterations, features of "
                      << dn.feature_spp << " spp)\n";
    }
    std::cout << "contexts: " << renderer.device_contexts() << "  scene uploads: " << renderer.scene_uploads() << "\n";
    std::cout << "Msamples/s: " << (double)W * H * config.samples_per_pixel / renderer.last_seconds() * 1e-6
              << " (includes flatten, upload and D2H)\n";
    std::vector<unsigned char> shown;
    if (display) {
        rtr_display_result res{};
        if (renderer.display(buffer, dp, shown, &res) != RTR_OK) {
            std::cerr << "display failed (" << renderer.last_status() << "): " << renderer.last_error() << "\n";
            return 1;
        }
        std::printf("display: scale %.17g (metered %.17g over %lld pixels)\n", res.scale, res.metered, (long long)res.n_metered);
    }
    const std::vector<unsigned char>* bytes = display ? &shown : nullptr;
    const bool png = out.size() > 4 && out.compare(out.size() - 4, 4, ".png") == 0; /* main.cpp:138-151 writes a PNG */
    if (!out.empty() && !(png ? buffer.save_to_png(out, bytes) : buffer.save_to_ppm(out, bytes))) {
        std::cerr << "Failed to save image to " << out << "\n";
        return 1;
    }
    return 0;
}
