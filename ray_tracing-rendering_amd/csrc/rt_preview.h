/*
 * rt_preview.h -- baked previews (include/rtr_hip.h: rtr_preview_*): the parameter rule, the ray of a sample, written once
 * for host (rtr_preview_ray) and device, and the kernel that makes a frame in one launch: cast, material mapping,
 * shade_ibl_one of rt_ibl.h.  Instantiated and launched by rtr_preview.hip.
 */
#pragma once

#include "rt_ibl.h"

inline const char* preview_params_why(const rtr_preview_params* p) {
    if (!p) return "null preview params";
    if (p->image_width < 2 || p->image_height < 2) return "image_width and image_height must be >= 2";
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->image_width || p->y1 > p->image_height || p->x0 >= p->x1 || p->y0 >= p->y1)
        return "empty region, or one outside the image";
    if (p->grid < 1 || p->grid > 8) return "grid outside 1 .. 8";
    if (p->flags & ~RTR_FLAG_REFERENCE_ORDER) return "unknown flag bits";
    if (!(__builtin_isfinite(p->t_min) && p->t_min >= 0x1p-100)) return "t_min must be finite and >= 2^-100";
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return "reserved must be 0";
    return nullptr;
}

/* RAY: sample s of pixel (i, j) of a W x H image under a k x k grid; d in the operation order of camera_get_ray without
 * its lens offset */
RT_HD void preview_ray(const rtr_camera& c, int W, int H, int k, int i, int j, int s, double* o, double* d) {
    const int a = s % k, b = s / k;
    const double u = (i + (a + 0.5) / k) / (W - 1);
    const double v = (j + (b + 0.5) / k) / (H - 1);
    for (int x = 0; x < 3; ++x) {
        o[x] = c.origin[x];
        d[x] = ((c.lower_left_corner[x] + u * c.horizontal[x]) + v * c.vertical[x]) - c.origin[x];
    }
}

struct PreviewK {
    int W, H;
    int x0, y0, x1, y1; /* the pixels this launch serves */
    int k;              /* grid */
    double t_min;
    rtr_preview_sample* samples; /* SAMPLES: record 0 is sample 0 of pixel (x0, y0); rows of x1 - x0 pixels */
    double* linear;              /* !SAMPLES: pixel (x0, y0) at linear[0], rows row_stride pixels apart */
    int32_t* lit;                /* the same layout, or null */
    long long row_stride;
};

/* SAMPLE: the ray cast to its closest hit and the hit turned into a record */
template <int TRAV>
RT_DEV rtr_preview_sample preview_sample(const DScene& sc, const PreviewK& P, int i, int j, int s, const Stack st) {
    rtr_preview_sample r;
    for (int a = 0; a < 3; ++a) r.q.p[a] = r.q.n[a] = r.q.v[a] = r.q.base[a] = 0.0, r.direct[a] = 0.0;
    r.q.roughness = 0.0, r.q.metallic = 0.0;
    r.kind = RTR_PREVIEW_MISS, r.material = -1;
    double o[3], d[3];
    preview_ray(sc.camera, P.W, P.H, P.k, i, j, s, o, d);
    const V3 ro = ld3(o), rd = ld3(d);
    uint32_t rng = 1;
    Hit rec;
    rec.u = 0, rec.v = 0;
    if (!cast_closest<TRAV>(sc, ro, rd, sc.camera.time0, rec, rng, st, P.t_min, RT_INF)) {
        /* Integrator::Li of RTR_INTEGRATOR_MIS for a camera ray that leaves the scene, as bounce() adds it */
        const V3 L = add(mk(0, 0, 0), miss_radiance<RTR_INTEGRATOR_MIS>(sc, mk(1, 1, 1), ro, rd, 0, false, 0.0));
        r.direct[0] = L.x, r.direct[1] = L.y, r.direct[2] = L.z;
        return r;
    }
    const FMat m = ld_const(sc.fmat, rec.mat);
    r.material = rec.mat;
    if (m.type == RTR_MAT_DIFFUSE_LIGHT) { /* mat_emitted: the front face only */
        r.kind = RTR_PREVIEW_EMITTER;
        if (rec.front) {
            const V3 e = tex_value(sc, m.tex[0], rec.u, rec.v, rec.p);
            r.direct[0] = e.x, r.direct[1] = e.y, r.direct[2] = e.z;
        }
        return r;
    }
    r.kind = RTR_PREVIEW_SURFACE;
    r.q.p[0] = rec.p.x, r.q.p[1] = rec.p.y, r.q.p[2] = rec.p.z;
    r.q.n[0] = rec.n.x, r.q.n[1] = rec.n.y, r.q.n[2] = rec.n.z;
    r.q.v[0] = -rd.x, r.q.v[1] = -rd.y, r.q.v[2] = -rd.z;
    V3 base = mk(1.0, 1.0, 1.0);
    double rough = 0.0, metal = 1.0; /* dielectric: a mirror of the environment */
    if (m.type == RTR_MAT_METAL) {
        base = mk(m.f[0], m.f[1], m.f[2]), rough = m.f[3];
    } else if (m.type == RTR_MAT_PBR) {
        base = tex_value(sc, m.tex[0], rec.u, rec.v, rec.p);
        rough = tex_scalar(sc, m.tex[1], rec.u, rec.v, rec.p); /* as it is: the shader clamps it */
        metal = tex_scalar(sc, m.tex[2], rec.u, rec.v, rec.p);
    } else if (m.type != RTR_MAT_DIELECTRIC) { /* lambertian (isotropic: the entries refuse scenes with media) */
        base = tex_value(sc, m.tex[0], rec.u, rec.v, rec.p);
        rough = 1.0, metal = 0.0;
    }
    r.q.base[0] = base.x, r.q.base[1] = base.y, r.q.base[2] = base.z;
    r.q.roughness = rough, r.q.metallic = metal;
    return r;
}

/* rtr_preview / rtr_preview_samples: one workgroup per 16 x 16 pixel block of the region (blockIdx.x, blockIdx.y count
 * blocks from its lower left corner), one lane per pixel, the traversal stack in LDS as for k_features.  The phases of a
 * sample follow each other in the lane -- cast, material mapping, shade_ibl_one -- so the rays and the queries stay in
 * registers and the register cost is that of the widest phase.  SAMPLES: the records go out instead of being shaded (E is
 * not read). */
/* The kernels are held to two waves per SIMD, 256 registers.  Left to itself (-DRTR_PREVIEW_WAVES=1) the compiler takes 256
 * VGPRs and 74 - 88 AGPRs for the frame form, one wave, and is 1.3 - 1.4 x slower on scenes 21 and 23 than with the 70 - 84
 * VGPRs of the shading phase spilled to scratch; the samples form needs 216 - 242 VGPRs and no scratch either way, but
 * takes 255 without the cap (profiles/r26_kres.txt, r26_preview.txt) */
#ifndef RTR_PREVIEW_WAVES
#define RTR_PREVIEW_WAVES 2
#endif
/* the lane's pixel, the body of every kernel below.  SET: the shader reads the capture set *S (rtr_preview_set) */
template <int TRAV, bool SAMPLES, bool SET>
RT_DEV void preview_pixel(const DScene& sc, const PreviewK& P, const ShadeK& E, const SetK* S) {
    extern __shared__ int lds_stack[];
    const Stack st{lds_stack + threadIdx.x};
    const int i = P.x0 + (int)blockIdx.x * 16 + (int)(threadIdx.x & 15);
    const int j = P.y0 + (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (i >= P.x1 || j >= P.y1) return;
    const int kk = P.k * P.k;
    const long long pixel = (long long)(j - P.y0) * (SAMPLES ? P.x1 - P.x0 : P.row_stride) + (i - P.x0);
    double acc[3] = {0.0, 0.0, 0.0};
    int lit = 0;
    for (int s = 0; s < kk; ++s) {
        const rtr_preview_sample r = preview_sample<TRAV>(sc, P, i, j, s, st);
        if (SAMPLES) {
            P.samples[pixel * kk + s] = r;
            continue;
        }
        if (r.kind != RTR_PREVIEW_SURFACE) {
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + r.direct[c];
            ++lit;
            continue;
        }
        double nlen, vlen;
        if (shade_query_bad(r.q, nlen, vlen)) continue;
        const rtr_gather_out o = shade_ibl_one<SET>(E, r.q, nlen, vlen, S);
        if (!o.valid) continue;
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + o.v[c];
        ++lit;
    }
    if (SAMPLES) return;
    const double scale = 1.0 / kk;
    for (int c = 0; c < 3; ++c) P.linear[pixel * 3 + c] = scale * acc[c];
    if (P.lit) P.lit[pixel] = lit;
}
template <int TRAV, bool SAMPLES>
__global__ void __launch_bounds__(RTR_BLOCK) __attribute__((amdgpu_waves_per_eu(RTR_PREVIEW_WAVES))) k_preview(const DScene sc, const PreviewK P, const ShadeK E) {
    preview_pixel<TRAV, SAMPLES, false>(sc, P, E, nullptr);
}
/* rtr_preview_set: the frame form with the capture set as a fourth argument */
template <int TRAV>
__global__ void __launch_bounds__(RTR_BLOCK) __attribute__((amdgpu_waves_per_eu(RTR_PREVIEW_WAVES))) k_preview_set(const DScene sc, const PreviewK P, const ShadeK E, const SetK S) {
    preview_pixel<TRAV, false, true>(sc, P, E, &S);
}
