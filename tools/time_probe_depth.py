#!/usr/bin/env python3
"""Times of the probe distance maps (include/rtr_hip.h: rtr_probe_depth*, rtr_probe_lookup_visible*) against the entries
they are made of, on one context.

  maps    rtr_probe_depth_device on scene 21: a T x T map (T = 8) of 4 samples per texel at each first hit of a 128 x 128
          camera grid, moved DISPLACE along its normal, against rtr_query_closest_device over the same rays already resident
          on the device (80 bytes in and 88 bytes out per ray, where the map kernel makes the ray in registers and keeps 32
          bytes per texel); the maps are compared with the restatement's reduction of those hits
  lookup  rtr_probe_lookup_visible_device, 10^6 queries in an 8 x 8 x 8 grid with maps of T = 16, against
          rtr_probe_lookup_device on the same grid and queries

HIP events on the context's stream, one warm-up, median of 5 windows of 20 back-to-back calls, reported per call; each
pair is timed twice in alternating order (a b b a) and both figures are printed."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import _capture_ref as CR
import _gather_ref as GR
import _golden as G
import _probe_depth_ref as DR
from time_probes import first_hits, pair

A = G.A
MAP, SAMPLES, SEED, DISPLACE, T_MAX = 8, 4, 7, 5.0, 400.0


def map_rays(points, T, N, seed, t_max, chunk=512):
    """RAY_DTYPE [n, T, T, N]: the rays of rtr_probe_depth_ray with jitter, the restatement's rule in whole-array numpy"""
    n = len(points)
    rays = np.zeros((n, T, T, N), dtype=A.RAY_DTYPE)
    b = np.arange(T, dtype=np.uint64).reshape(1, T, 1, 1)
    a = np.arange(T, dtype=np.uint64).reshape(1, 1, T, 1)
    s = np.arange(N, dtype=np.uint64).reshape(1, 1, 1, N)
    for k0 in range(0, n, chunk):
        m = min(chunk, n - k0)
        k = (np.arange(k0, k0 + m, dtype=np.uint64) & GR.M32).reshape(m, 1, 1, 1)
        state = np.broadcast_to(CR.sample_seed(seed, T * T, b * np.uint64(T) + a, k, s), (m, T, T, N)).copy()
        state = GR.xorshift(state)
        ju = state.astype(np.float64) * 2.0 ** -32
        state = GR.xorshift(state)
        jv = state.astype(np.float64) * 2.0 ** -32
        u = (2.0 * (a.astype(np.float64) + ju)) / float(T) - 1.0
        v = (2.0 * (b.astype(np.float64) + jv)) / float(T) - 1.0
        z = (1.0 - np.abs(u)) - np.abs(v)
        sg = lambda t: np.where(t >= 0, 1.0, -1.0)
        x = np.where(z >= 0, u, (1.0 - np.abs(v)) * sg(u))
        y = np.where(z >= 0, v, (1.0 - np.abs(u)) * sg(v))
        r = 1.0 / np.sqrt((x * x + y * y) + z * z)
        out = rays[k0:k0 + m]
        out["direction"] = np.stack([r * x, r * y, r * z], axis=-1)
        out["origin"] = points[k0:k0 + m, None, None, None, :]
        out["rng_state"] = state.astype(np.uint32)
    rays["t_min"], rays["t_max"] = 0.001, t_max
    return rays


def main():
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    sc = G.scene(21)
    ctx.upload(sc)
    hits = first_hits(ctx, sc)
    n = len(hits)
    where = hits["p"] + DISPLACE * hits["n"]
    n_rays = n * MAP * MAP * SAMPLES
    print("scene 21  %d probes x %d x %d texels x %d samples = %d rays, t_max %g" % (n, MAP, MAP, SAMPLES, n_rays, T_MAX), flush=True)
    rays = map_rays(where, MAP, SAMPLES, SEED, T_MAX)
    d_rays, d_pts = dev(rays.reshape(-1)), dev(G.rtr.native.probe_points(where))
    d_hits = torch.zeros(n_rays * A.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_maps = torch.zeros(n * MAP * MAP * A.PROBE_DEPTH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kw = dict(map_size=MAP, samples=SAMPLES, seed=SEED, t_max=T_MAX)
    q, m = pair(lambda: ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), n_rays),
                lambda: ctx.probe_depth_into(d_pts.data_ptr(), d_maps.data_ptr(), n, **kw))
    torch.cuda.synchronize()
    h = d_hits.cpu().numpy().view(A.RAY_HIT_DTYPE).reshape(rays.shape)
    same = DR.reduce(h["hit"], h["t"], h["front_face"], T_MAX).tobytes() == d_maps.cpu().numpy().tobytes()
    print("maps    closest-hit query %8.3f %8.3f ms   depth maps %8.3f %8.3f ms   maps / query = %.2f   %.1f Mrays/s   hit %.2f   "
          "maps equal the reduction of the hits: %s   %s" % (q[0], q[1], m[0], m[1], sum(m) / sum(q), n_rays / (sum(m) / 2) * 1e-3,
                                                          float((h["hit"] == 1).mean()), same, ctx.last_probe_depth()), flush=True)
    del d_rays, d_hits, d_maps, d_pts
    # lookup: 10^6 queries in an 8 x 8 x 8 grid of random coefficients and random maps (needs no scene)
    rng = np.random.default_rng(1)
    T = 16
    probes = np.zeros(512, dtype=A.PROBE_SH_DTYPE)
    probes["c"], probes["valid"] = rng.standard_normal((512, 9, 3)), 1
    depth = np.zeros((512, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    depth["mean"] = 0.3 + rng.random(depth.shape) * 1.2  # about half of the corners lie beyond what their probe sees
    depth["mean2"] = depth["mean"] ** 2 + rng.random(depth.shape) * 0.1
    depth["valid"] = 1
    grid = G.rtr.native.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))
    vp = G.rtr.native.probe_visible_params(T, 0.25)
    nq = 1000000
    qs = G.rtr.native.gather_points(rng.random((nq, 3)) * 7.0, rng.standard_normal((nq, 3)))
    d_probes, d_depth, d_q = dev(probes), dev(depth.reshape(-1)), dev(qs)
    d_out = torch.zeros(nq * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p, v = pair(lambda: ctx.probe_lookup_into(grid, d_probes.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), nq),
                lambda: ctx.probe_lookup_visible_into(grid, d_probes.data_ptr(), d_depth.data_ptr(), vp, d_q.data_ptr(),
                                                      d_out.data_ptr(), nq))
    print("lookup  %d queries, 8 x 8 x 8 grid, T = %d   plain %8.3f %8.3f ms   visible %8.3f %8.3f ms   visible / plain = %.2f   "
          "%.1f Mqueries/s" % (nq, T, p[0], p[1], v[0], v[1], sum(v) / sum(p), nq / (sum(v) / 2) * 1e-3), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
