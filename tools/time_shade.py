#!/usr/bin/env python3
"""Times of image-based shading (include/rtr_hip.h: rtr_brdf_table_device, rtr_shade_ibl_device) on one context.

  table   the 64 x 64 table at M = 128 (2 M^2 = 32 768 nodes per entry): nodes/s, and counted FP64 operations against the
          78.6 TFLOP/s vector peak bench.py uses.  A fused multiply-add would count as two (the build has none); an IEEE
          division counts 17 (two scales, the reciprocal, four fused steps, a product, the residual step, the select-and-
          multiply and the fix-up).  Every (node, entry) costs 12 (W 2, Hx 2, v.h 3, n.l 3, two compares); a USED one 55
          more (g 3 + a division, e 6 + a division, x 1, fc 4, A 4, B 3).  `used` is counted on the host from the
          definition.
  shade   10^6 rtr_shade_ibl_device queries (both parts) in an 8 x 8 x 8 grid with maps of T = 16, the five-level chain of
          an S = 64 capture and that table, against the two launches it fuses over the same queries:
          rtr_probe_lookup_visible_device + rtr_cube_chain_lookup_device (whose results would still have to be combined);
          the first 2000 records are compared with rtr_shade_ibl_one

HIP events on the context's stream, one warm-up, median of 5 windows of back-to-back calls, reported per call; the pair is
timed twice in alternating order (a b b a) and both figures are printed."""
import ctypes as C
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import _golden as G
from time_probes import pair, timed

A = G.A
N = G.rtr.native
PEAK = 78.6e12
N_MU = N_ROUGH = 64
NODES = 128


def used_nodes(n_mu, n_rough, M):
    """how many (node, entry) pairs of the table are USED, from the header's definition in whole-array numpy"""
    jj = np.arange(M * M)
    s, t = (jj // M + 0.5) / M, (jj % M + 0.5) / M
    cx = (1.0 - t * t) / (1.0 + t * t)
    used = 0
    for r in range(n_rough):
        rough = (r + 0.5) / n_rough
        a2 = (rough * rough) * (rough * rough)
        c2 = (s * s) / (a2 + (1.0 - a2) * (s * s))
        Hz, sh = np.sqrt(c2), np.sqrt(np.maximum(1.0 - c2, 0.0))
        for c in range(n_mu):
            mu = (c + 0.5) / n_mu
            Vx = np.sqrt(1.0 - mu * mu)
            for sx in (1.0, -1.0):
                vh = Vx * (sh * (sx * cx)) + mu * Hz
                used += int(((vh > 0) & ((2.0 * vh) * Hz - mu > 0)).sum())
    return used


def main():
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()
    entries = N_MU * N_ROUGH
    d_table = torch.zeros(entries * A.BRDF_ENTRY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = timed(lambda: ctx.brdf_table_into(d_table.data_ptr(), N_MU, N_ROUGH, NODES), calls=5)
    nodes = entries * 2 * NODES * NODES
    used = used_nodes(N_MU, N_ROUGH, NODES)
    flops = 12 * nodes + 55 * used
    table = d_table.cpu().numpy().view(A.BRDF_ENTRY_DTYPE).reshape(N_ROUGH, N_MU)
    spot = np.zeros(1, dtype=A.BRDF_ENTRY_DTYPE)
    same = True
    for r, c in ((0, 0), (17, 40), (63, 63)):
        N.lib().rtr_brdf_entry_one(C.byref(N.brdf_params(N_MU, N_ROUGH, NODES)), r, c, spot.ctypes.data)
        same = same and spot[0].tobytes() == table[r, c].tobytes()
    print("table   %d x %d entries, M = %d   %8.3f ms   %.3e nodes   %6.1f Gnodes/s   used %.3f   %5.2f TFLOP/s FP64 = %.3f of peak   "
          "three entries equal rtr_brdf_entry_one: %s" % (N_MU, N_ROUGH, NODES, ms, nodes, nodes / ms * 1e-6, used / nodes,
                                                          flops / ms * 1e-9, flops / (ms * 1e-3) / PEAK, same), flush=True)
    # shade: 10^6 queries, random coefficients, maps and texels (needs no scene)
    rng = np.random.default_rng(1)
    T, S, LEVELS, nq = 16, 64, 5, 1000000
    probes = np.zeros(512, dtype=A.PROBE_SH_DTYPE)
    probes["c"], probes["valid"] = rng.standard_normal((512, 9, 3)), 1
    depth = np.zeros((512, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    depth["mean"] = 0.3 + rng.random(depth.shape) * 1.2
    depth["mean2"] = depth["mean"] ** 2 + rng.random(depth.shape) * 0.1
    depth["valid"] = 1
    levels, n_records = N.cube_chain_plan(S, LEVELS)
    chain = np.zeros(n_records, dtype=A.GATHER_OUT_DTYPE)
    chain["v"], chain["count"], chain["valid"] = rng.random((n_records, 3)), 4, 1
    grid = N.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))
    vp = N.probe_visible_params(T, 0.25)
    p, n, v = rng.random((nq, 3)) * 7.0, rng.standard_normal((nq, 3)), rng.standard_normal((nq, 3))
    rough = rng.random(nq)
    q = N.shade_queries(p, n, v, rng.random((nq, 3)), rough, rng.random(nq))
    # the inputs of the two-launch route: the same points and normals, and the reflection vectors at alpha = rough^2
    Nn, Vv = n / np.linalg.norm(n, axis=1)[:, None], v / np.linalg.norm(v, axis=1)[:, None]
    mu = (Nn * Vv).sum(axis=1)
    r_clamped = np.clip(rough, 0.01, 1.0)
    cq = N.cube_queries(2.0 * mu[:, None] * Nn - Vv, r_clamped * r_clamped)
    d_probes, d_depth, d_chain = dev(probes), dev(depth), dev(chain)
    d_q, d_gp, d_cq = dev(q), dev(N.gather_points(p, n)), dev(cq)
    d_out, d_out2, d_out3 = (torch.zeros(nq * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(3))
    env = N.shade_env(d_table.data_ptr(), grid=grid, probes=d_probes.data_ptr(), depth=d_depth.data_ptr(), visible=vp,
                      levels=levels, chain=d_chain.data_ptr(), n_records=n_records, n_mu=N_MU, n_rough=N_ROUGH)
    torch.cuda.synchronize()

    def two():
        ctx.probe_lookup_visible_into(grid, d_probes.data_ptr(), d_depth.data_ptr(), vp, d_gp.data_ptr(), d_out3.data_ptr(), nq)
        ctx.cube_chain_lookup_into(levels, d_chain.data_ptr(), n_records, d_cq.data_ptr(), d_out2.data_ptr(), nq)

    a, b = pair(two, lambda: ctx.shade_ibl_into(env, d_q.data_ptr(), d_out.data_ptr(), nq))
    vis = timed(lambda: ctx.probe_lookup_visible_into(grid, d_probes.data_ptr(), d_depth.data_ptr(), vp, d_gp.data_ptr(),
                                                      d_out2.data_ptr(), nq))
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE)
    host = N.shade_env(table, grid=grid, probes=probes, depth=depth, visible=vp, levels=levels, chain=chain)
    same = got[:2000].tobytes() == N.shade_ibl_one(host, q[:2000]).tobytes()
    print("shade   %d queries, 8 x 8 x 8 grid, T = %d, S = %d x %d levels   two launches %8.3f %8.3f ms (visible lookup alone %.3f)   "
          "fused %8.3f %8.3f ms   fused / two = %.2f   %.1f Mqueries/s   valid %.3f   2000 records equal rtr_shade_ibl_one: %s" %
          (nq, T, S, LEVELS, a[0], a[1], vis, b[0], b[1], sum(b) / sum(a), nq / (sum(b) / 2) * 1e-3,
           float((got["valid"] == 1).mean()), same), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
