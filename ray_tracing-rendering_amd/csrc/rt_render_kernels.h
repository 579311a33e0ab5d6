/*
 * rt_render_kernels.h -- the non-template kernels of a render call; rtr_capi.hip includes them, and no other unit.
 *  k_resolve       adds the per-chunk partial sums of a pixel in chunk order, scales by 1/spp (renderer.h:131) and stores
 *                  linear mean radiance (the wavefront driver reaches it through rtr_launch_resolve).
 *  k_camera_store  rtr_set_camera: the new camera into the DScene on the device, in stream order.
 */
#pragma once

#include "rt_render.h"

__global__ void __launch_bounds__(RTR_BLOCK) k_resolve(const ResolveK R) {
    const RenderK& P = R.r;
    int i, j;
    bool active;
    tile_pixel(P, blockIdx.x, threadIdx.x, i, j, active);
    for (int c = 0; c < P.chunks; ++c) { /* wave-uniform: scalar loads */
        const int d = P.done[blockIdx.x * P.chunks + c];
        if (R.done_full ? d != R.done_full : !d) return;
    }
    const bool packed = R.row_stride < 0;
    if (packed && threadIdx.x == 0) R.tile_done[blockIdx.x] = 1;
    if (!active) return;
    const double* in = P.partial + (size_t)blockIdx.x * P.chunks * 3 * RTR_BLOCK + threadIdx.x;
    double r = 0, g = 0, b = 0;
    for (int c = 0; c < P.chunks; ++c) {
        if (c == 0) {
            r = in[0], g = in[RTR_BLOCK], b = in[2 * RTR_BLOCK];
        } else {
            r += in[0], g += in[RTR_BLOCK], b += in[2 * RTR_BLOCK];
        }
        in += 3 * RTR_BLOCK;
    }
    const double scale = 1.0 / P.spp; /* renderer.h:131 */
    double* o = packed ? R.out + ((long long)blockIdx.x * RTR_BLOCK + threadIdx.x) * 3
                       : R.out + ((long long)(j - P.y0) * R.row_stride + (i - P.x0)) * 3;
    o[0] = scale * r;
    o[1] = scale * g;
    o[2] = scale * b;
}

/* rtr_set_camera: the camera of the DScene the megakernel and the wavefront stages read through a pointer, replaced in
 * stream order (the per-ray kernels take the DScene by value) */
__global__ void __launch_bounds__(64) k_camera_store(DScene* sc, const rtr_camera cam) {
    static_assert(sizeof(rtr_camera) == 24 * sizeof(double), "24 doubles");
    const double* src = reinterpret_cast<const double*>(&cam);
    double* dst = reinterpret_cast<double*>(&sc->camera);
    if (threadIdx.x < 24) dst[threadIdx.x] = src[threadIdx.x];
}
