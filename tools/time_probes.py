#!/usr/bin/env python3
"""Times of the light probes (include/rtr_hip.h: rtr_probe_*) against their gather twins and the route they replace, on one
context: 64 samples at each first hit of a 128 x 128 camera grid, moved DISPLACE along its normal (at most 2^14 probes,
2^20 rays), on scenes 21 and 9.

  visibility  rtr_probe_visibility_device against rtr_gather_occlusion_device at the same points (the gather casts over the
              hemisphere of the normal, the probe over the sphere: other rays, the same number of them)
  radiance    rtr_probe_radiance_device against rtr_gather_radiance_device, and against blocking rtr_li_rays over the
              probe's own rays (host arrays, as the entry takes them; the projection in numpy is not counted)
  lookup      rtr_probe_lookup_device, 10^6 queries in an 8 x 8 x 8 grid

HIP events on the context's stream, one warm-up, median of 5 windows of 20 back-to-back calls, reported per call; each
pair is timed twice in alternating order (a b b a) and both figures are printed."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import _golden as G
import _probe_ref as PR

A = G.A
SIDE, SAMPLES, SEED, DISPLACE = 128, 64, 7, 5.0


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


def pair(a, b):
    """(a, b) each timed twice in the order a b b a"""
    a0, b0, b1, a1 = timed(a), timed(b), timed(b), timed(a)
    return (a0, a1), (b0, b1)


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
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    # (scene:integrator pairs on the command line replace the two cases the committed figures come from)
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(21, 4), (9, 1)]
    for sid, integrator in cases:
        sc = G.scene(sid)
        ctx.upload(sc)
        hits = first_hits(ctx, sc)
        n = len(hits)
        where = hits["p"] + DISPLACE * hits["n"]
        print("scene %02d  %d points (first hits of a %d x %d grid, moved %g along the normal) x %d samples = %d rays" %
              (sid, n, SIDE, SIDE, DISPLACE, SAMPLES, n * SAMPLES), flush=True)
        d_gpts = dev(G.rtr.native.gather_points(where, hits["n"]))
        d_ppts = dev(G.rtr.native.probe_points(where))
        d_gout = torch.zeros(n * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_vis = torch.zeros(n * A.PROBE_VIS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_sh = torch.zeros(n * A.PROBE_SH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g, p = pair(lambda: ctx.gather_occlusion_into(d_gpts.data_ptr(), d_gout.data_ptr(), n, samples=SAMPLES, seed=SEED),
                    lambda: ctx.probe_visibility_into(d_ppts.data_ptr(), d_vis.data_ptr(), n, samples=SAMPLES, seed=SEED))
        print("scene %02d  visibility  occlusion gather %8.3f %8.3f ms   probe %8.3f %8.3f ms   probe / gather = %.2f   %s" %
              (sid, g[0], g[1], p[0], p[1], sum(p) / sum(g), ctx.last_probe()), flush=True)
        prm = A.make_params(64, 64, 1, integrator=integrator)
        g, p = pair(lambda: ctx.gather_radiance_into(prm, d_gpts.data_ptr(), d_gout.data_ptr(), n, samples=SAMPLES, seed=SEED),
                    lambda: ctx.probe_radiance_into(prm, d_ppts.data_ptr(), d_sh.data_ptr(), n, samples=SAMPLES, seed=SEED))
        print("scene %02d  radiance (integrator %d)  gather %8.3f %8.3f ms   probe %8.3f %8.3f ms   probe / gather = %.2f   %s" %
              (sid, integrator, g[0], g[1], p[0], p[1], sum(p) / sum(g), ctx.last_probe()), flush=True)
        # the route the probes replace: the probe's own rays through blocking rtr_li_rays (packed once, made on the host)
        state = np.zeros((n, SAMPLES), dtype=np.uint32)
        direction = np.zeros((n, SAMPLES, 3))
        for k0 in range(0, n, 1024):  # the rays of rtr_probe_ray, from the vectorised restatement of the tests
            m = min(1024, n - k0)
            direction[k0:k0 + m], state[k0:k0 + m] = PR.rays(m, SAMPLES, SEED, point_base=k0)
        li = np.zeros(n * SAMPLES, dtype=A.LI_RAY_DTYPE)
        li["origin"], li["direction"] = np.repeat(where, SAMPLES, axis=0), direction.reshape(-1, 3)
        li["time"], li["rng_state"] = 0.0, state.reshape(-1)
        radiance = np.zeros((len(li), 3))
        li_ms = timed(lambda: ctx._chk(ctx._L.rtr_li_rays(ctx._h, C.byref(prm), li.ctypes.data, radiance.ctypes.data, len(li))), calls=1)
        same = np.array_equal(PR.radiance(direction, radiance.reshape(n, SAMPLES, 3)).view(np.uint64),
                              d_sh.cpu().numpy().view(A.PROBE_SH_DTYPE)["c"].view(np.uint64))
        print("scene %02d  radiance (integrator %d)  rtr_li_rays, blocking %8.3f ms   li_rays / probe = %.2f   coefficients equal: %s" %
              (sid, integrator, li_ms, li_ms / (sum(p) / 2), same), flush=True)
        del d_gpts, d_ppts, d_gout, d_vis, d_sh
    # lookup: 10^6 queries in an 8 x 8 x 8 grid of random coefficients (needs no scene)
    rng = np.random.default_rng(1)
    probes = np.zeros(512, dtype=A.PROBE_SH_DTYPE)
    probes["c"], probes["valid"] = rng.standard_normal((512, 9, 3)), 1
    grid = G.rtr.native.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))
    nq = 1000000
    q = G.rtr.native.gather_points(rng.random((nq, 3)) * 7.0, rng.standard_normal((nq, 3)))
    d_probes, d_q = dev(probes), dev(q)
    d_out = torch.zeros(nq * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = timed(lambda: ctx.probe_lookup_into(grid, d_probes.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), nq))
    print("lookup  %d queries, 8 x 8 x 8 grid  %8.3f ms  %8.1f Mqueries/s" % (nq, ms, nq / ms * 1e-3), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
