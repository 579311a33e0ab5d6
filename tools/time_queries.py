#!/usr/bin/env python3
"""Rates of the ray queries (include/rtr_hip.h: rtr_query_closest_device / rtr_query_occluded_device): 2^20 closest-hit
and 2^20 occlusion queries on scenes 21 and 9, camera-coherent rays (the pixel-centre rays of a 1024 x 1024 image) and the
same rays shuffled, with the per-lane and the staged record access (RTR_QUERY_STAGED=0 / 1).  HIP events around the
device-pointer entries, one warm-up, median of 5.  For context: the megakernel's own segment rate,
(closest_segments + shadow_segments) / device_ms of one render in the same process and context.

  tools/time_queries.py [--ab-only]     --ab-only: one closest batch per form on scene 21 (for a kernel trace)
"""
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import _golden as G

A = G.A
N_SIDE = 1024
N = N_SIDE * N_SIDE


def camera_rays(sc):
    cam = sc.camera[0]
    i, j = np.meshgrid(np.arange(N_SIDE, dtype=np.float64), np.arange(N_SIDE, dtype=np.float64))
    u = ((i + 0.5) / (N_SIDE - 1)).reshape(-1, 1)
    v = ((j + 0.5) / (N_SIDE - 1)).reshape(-1, 1)
    o = np.asarray(cam["origin"], dtype=np.float64)
    d = (np.asarray(cam["lower_left_corner"]) + u * np.asarray(cam["horizontal"]) + v * np.asarray(cam["vertical"])) - o
    return G.rtr.Context.make_rays(np.broadcast_to(o, d.shape), d, times=float(cam["time0"]),
                                   rng_states=np.arange(1, N + 1, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(1))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ab_only = "--ab-only" in sys.argv
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the queries run on
    ctx.set_stream(stream.cuda_stream)
    d_hits = torch.zeros(N * A.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_occ = torch.zeros(N, dtype=torch.uint8, device="cuda")
    d_rng = torch.zeros(N, dtype=torch.int32, device="cuda")
    for sid in (21,) if ab_only else (21, 9):
        sc = G.scene(sid)
        ctx.upload(sc)
        coherent = camera_rays(sc)
        sets = {"coherent": coherent, "shuffled": coherent[np.random.default_rng(1).permutation(N)]}
        if not ab_only:
            p = A.make_params(N_SIDE, N_SIDE, 16, integrator=4 if sid == 21 else 1, seed=1, spp_chunks=0)
            fb = torch.zeros((N_SIDE, N_SIDE, 3), dtype=torch.float64, device="cuda")
            ctx.render_into(p, fb.data_ptr(), N_SIDE, blocking=True)
            ctx.render_into(p, fb.data_ptr(), N_SIDE, blocking=True)
            st = ctx.stats()
            seg = st["closest_segments"] + st["shadow_segments"]
            print("scene %02d  megakernel (integrator %d, 16 spp): %.1f Msegments/s (%d segments in %.2f ms)" %
                  (sid, p.integrator, seg / st["device_ms"] * 1e-3, seg, st["device_ms"]), flush=True)
            del fb
        for name, rays in sets.items():
            if ab_only and name != "coherent":
                continue
            d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            for staged in (0, 1):
                os.environ["RTR_QUERY_STAGED"] = str(staged)
                form = "staged" if staged else "per-lane"
                if ab_only:
                    ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), N, blocking=True)
                    continue
                ms = timed(lambda: ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), N))
                print("scene %02d  %-8s  closest   %-8s  %7.3f ms  %8.1f Mrays/s" % (sid, name, form, ms, N / ms * 1e-3), flush=True)
                ms = timed(lambda: ctx.query_occluded_into(d_rays.data_ptr(), d_occ.data_ptr(), N, rng_out_ptr=d_rng.data_ptr()))
                print("scene %02d  %-8s  occluded  %-8s  %7.3f ms  %8.1f Mrays/s" % (sid, name, form, ms, N / ms * 1e-3), flush=True)
            del d_rays
    os.environ.pop("RTR_QUERY_STAGED", None)
    ctx.close()


if __name__ == "__main__":
    main()
