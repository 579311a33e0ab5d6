#!/usr/bin/env python3
"""Times of the hemisphere gathers (include/rtr_hip.h: rtr_gather_*) against the routes they replace, on one context:
64 samples at each first hit of a 128 x 128 camera grid (at most 2^14 points, 2^20 rays) on scenes 21 and 9.

  occlusion  rtr_gather_occlusion_device (every lane loads the point / one load per group and a broadcast:
             RTR_GATHER_BROADCAST=0 / 1) against rtr_query_occluded_device over the same rays already resident on the
             device -- their generation and the host sum are not counted, which favours the query route
  radiance   rtr_gather_radiance_device against blocking rtr_li_rays over the same rays (host arrays, as the entry takes them)

HIP events on the context's stream, one warm-up, median of 5 windows; a window of the non-blocking device entries holds
20 back-to-back calls (a single call of 0.05 ms would time the launch as much as the kernel) and is reported per call."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import _gather_ref as GR
import _golden as G

A = G.A
SIDE, SAMPLES, SEED = 128, 64, 7


def timed(fn, calls=20):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return statistics.median(ms)


def first_hits(ctx, sc):
    cam = sc.camera[0]
    i, j = np.meshgrid(np.arange(SIDE, dtype=np.float64), np.arange(SIDE, dtype=np.float64))
    u, v = ((i + 0.5) / (SIDE - 1)).reshape(-1, 1), ((j + 0.5) / (SIDE - 1)).reshape(-1, 1)
    o = np.asarray(cam["origin"], dtype=np.float64)
    d = (np.asarray(cam["lower_left_corner"]) + u * np.asarray(cam["horizontal"]) + v * np.asarray(cam["vertical"])) - o
    hits = ctx.query_closest(ctx.make_rays(np.broadcast_to(o, d.shape), d, times=float(cam["time0"])))
    return hits[hits["hit"] == 1]


def main():
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    for sid, integrator in ((21, 4), (9, 1)):
        sc = G.scene(sid)
        ctx.upload(sc)
        hits = first_hits(ctx, sc)
        n = len(hits)
        pts = G.rtr.native.gather_points(hits["p"], hits["n"])
        d, state = GR.rays(hits["p"], hits["n"], SAMPLES, SEED)
        rays = ctx.make_rays(np.repeat(hits["p"], SAMPLES, axis=0), d.reshape(-1, 3), rng_states=state.reshape(-1))
        print("scene %02d  %d points (first hits of a %d x %d grid) x %d samples = %d rays" % (sid, n, SIDE, SIDE, SAMPLES, len(rays)),
              flush=True)
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
        d_out = torch.zeros(n * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        d_occ = torch.zeros(len(rays), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        q_ms = timed(lambda: ctx.query_occluded_into(d_rays.data_ptr(), d_occ.data_ptr(), len(rays)))
        blocked = d_occ.cpu().numpy().astype(bool).reshape(n, SAMPLES)
        print("scene %02d  occlusion  query route (rays resident)   %8.3f ms  %8.1f Mrays/s" % (sid, q_ms, len(rays) / q_ms * 1e-3),
              flush=True)
        for bcast in (0, 1):
            os.environ["RTR_GATHER_BROADCAST"] = str(bcast)
            ms = timed(lambda: ctx.gather_occlusion_into(d_pts.data_ptr(), d_out.data_ptr(), n, samples=SAMPLES, seed=SEED))
            got = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE)
            same = np.array_equal(got["count"], SAMPLES - blocked.sum(axis=1))
            print("scene %02d  occlusion  gather, %-22s %8.3f ms  %8.1f Mrays/s  query / gather = %.2f  counts equal: %s" %
                  (sid, "one load + broadcast" if bcast else "every lane loads", ms, len(rays) / ms * 1e-3, q_ms / ms, same), flush=True)
        os.environ.pop("RTR_GATHER_BROADCAST", None)
        prm = A.make_params(64, 64, 1, integrator=integrator)
        li = np.zeros(len(rays), dtype=A.LI_RAY_DTYPE)  # packed once: only the library's call is timed
        li["origin"], li["direction"], li["time"], li["rng_state"] = rays["origin"], rays["direction"], rays["time"], rays["rng_state"]
        radiance = np.zeros((len(rays), 3))
        li_ms = timed(lambda: ctx._chk(ctx._L.rtr_li_rays(ctx._h, C.byref(prm), li.ctypes.data, radiance.ctypes.data, len(li))), calls=1)
        ms = timed(lambda: ctx.gather_radiance_into(prm, d_pts.data_ptr(), d_out.data_ptr(), n, samples=SAMPLES, seed=SEED))
        print("scene %02d  radiance (integrator %d)  rtr_li_rays, blocking  %8.3f ms   gather %8.3f ms  li_rays / gather = %.2f" %
              (sid, integrator, li_ms, ms, li_ms / ms), flush=True)
        del d_pts, d_out, d_rays, d_occ
    ctx.close()


if __name__ == "__main__":
    main()
