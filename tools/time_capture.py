#!/usr/bin/env python3
"""Times of the environment captures (include/rtr_hip.h: rtr_capture_cube) against their gather twin and the route they
replace, on one context: 16 centres (first hits of an 8 x 8 camera grid, 16 of them evenly picked and moved DISPLACE along
their normal) x 6 faces x 32 x 32 texels x 4 samples = 393 216 rays, MIS on scene 21 and RR on scene 9.

  gather    rtr_capture_cube_device against rtr_gather_radiance_device at the same ray count: one gather point per texel,
            at the texel's centre with the texel's central direction as the normal (cosine-distributed rays about it
            instead of rays through the texel: other rays, the same number of them from the same places)
  li_rays   blocking rtr_li_rays over the capture's own rays (rtr_capture_ray; host arrays, as the entry takes them; the
            reduction in numpy is not counted)
  lookup    rtr_cube_lookup_device, 10^6 directions in one capture of S = 32

HIP events on the context's stream, one warm-up, median of 5 windows of 20 back-to-back calls, reported per call; the
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
import _capture_ref as CR
import _golden as G

A = G.A
GRID, CENTRES, FACE, SAMPLES, SEED, DISPLACE = 8, 16, 32, 4, 7, 60.0


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
    i, j = np.meshgrid(np.arange(GRID, dtype=np.float64), np.arange(GRID, dtype=np.float64))
    u, v = ((i + 0.5) / GRID).reshape(-1, 1), ((j + 0.5) / GRID).reshape(-1, 1)
    o = np.asarray(cam["origin"], dtype=np.float64)
    d = (np.asarray(cam["lower_left_corner"]) + u * np.asarray(cam["horizontal"]) + v * np.asarray(cam["vertical"])) - o
    hits = ctx.query_closest(ctx.make_rays(np.broadcast_to(o, d.shape), d, times=float(cam["time0"])))
    hits = hits[hits["hit"] == 1]
    return hits[np.linspace(0, len(hits) - 1, min(CENTRES, len(hits))).astype(int)]


def main():
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    # (scene:integrator pairs on the command line replace the two cases the committed figures come from)
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(21, 4), (9, 1)]
    texels = 6 * FACE * FACE
    for sid, integrator in cases:
        sc = G.scene(sid)
        ctx.upload(sc)
        hits = first_hits(ctx, sc)
        n = len(hits)
        centres = hits["p"] + DISPLACE * hits["n"]
        print("scene %02d  %d centres (of the first hits of a %d x %d grid, moved %g along the normal) x 6 x %d x %d texels x %d samples = %d rays" %
              (sid, n, GRID, GRID, DISPLACE, FACE, FACE, SAMPLES, n * texels * SAMPLES), flush=True)
        prm = A.make_params(64, 64, 1, integrator=integrator)
        # the gather twin: a point per texel at its centre, the normal the texel's central direction
        axis = CR.rays(1, FACE, 1, SEED, 0, 0)[0].reshape(texels, 3)
        d_gpts = dev(G.rtr.native.gather_points(np.repeat(centres, texels, axis=0), np.tile(axis, (n, 1))))
        d_cpts = dev(G.rtr.native.probe_points(centres))
        d_gout = torch.zeros(n * texels * 32, dtype=torch.uint8, device="cuda")
        d_cout = torch.zeros(n * texels * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g, c = pair(lambda: ctx.gather_radiance_into(prm, d_gpts.data_ptr(), d_gout.data_ptr(), n * texels, samples=SAMPLES, seed=SEED),
                    lambda: ctx.capture_cube_into(prm, d_cpts.data_ptr(), d_cout.data_ptr(), n, face_size=FACE, samples=SAMPLES, seed=SEED))
        print("scene %02d  radiance (integrator %d)  gather %8.3f %8.3f ms   capture %8.3f %8.3f ms   capture / gather = %.2f   %s %s" %
              (sid, integrator, g[0], g[1], c[0], c[1], sum(c) / sum(g), ctx.last_gather(), ctx.last_capture()), flush=True)
        # the route the capture replaces: its own rays through blocking rtr_li_rays (packed once, made on the host)
        direction, state = CR.rays(n, FACE, SAMPLES, SEED)
        li = np.zeros(n * texels * SAMPLES, dtype=A.LI_RAY_DTYPE)
        li["origin"], li["direction"] = np.repeat(centres, texels * SAMPLES, axis=0), direction.reshape(-1, 3)
        li["time"], li["rng_state"] = 0.0, state.reshape(-1)
        radiance = np.zeros((len(li), 3))
        li_ms = timed(lambda: ctx._chk(ctx._L.rtr_li_rays(ctx._h, C.byref(prm), li.ctypes.data, radiance.ctypes.data, len(li))), calls=1)
        got = d_cout.cpu().numpy().view(A.GATHER_OUT_DTYPE)["v"].reshape(n, 6, FACE, FACE, 3)
        same = np.array_equal(CR.reduce(radiance.reshape(n, 6, FACE, FACE, SAMPLES, 3)).view(np.uint64), got.view(np.uint64))
        print("scene %02d  radiance (integrator %d)  rtr_li_rays, blocking %8.3f ms   li_rays / capture = %.2f   texels equal: %s" %
              (sid, integrator, li_ms, li_ms / (sum(c) / 2), same), flush=True)
        if (sid, integrator) == cases[-1]:  # lookup: 10^6 directions in the first centre's capture (needs no scene)
            nq = 1000000
            q = G.rtr.native.probe_points(np.random.default_rng(1).standard_normal((nq, 3)))
            d_q = dev(q)
            d_out = torch.zeros(nq * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ms = timed(lambda: ctx.cube_lookup_into(FACE, d_cout.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), nq))
            print("lookup  %d directions, S = %d  %8.3f ms  %8.1f Mqueries/s" % (nq, FACE, ms, nq / ms * 1e-3), flush=True)
        del d_gpts, d_cpts, d_gout, d_cout
    ctx.close()


if __name__ == "__main__":
    main()
