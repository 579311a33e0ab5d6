#!/usr/bin/env python3
"""Times of the baked preview (include/rtr_hip.h: rtr_preview_device) on one context, scenes 21 and 23 at 800 x 800.

  bake     a real one: an 8 x 8 x 8 probe grid over the middle half of the bounding box of the first hits, 64 samples per
           probe, distance maps of T = 16, the five-level chain of an S = 64 capture at the box's centre, a 64 x 64 table
  fused    rtr_preview_device, k = 1 and k = 2, against the two existing calls it fuses over the same rays and queries already
           resident on the device: rtr_query_closest_device + rtr_shade_ibl_device.  That pair leaves undone what the preview
           also does: making the rays, the material mapping, the values of the rays that miss or meet an emitter, and the
           reduction over a pixel's samples (its queries of samples that are no surface are all-zero records, which the shader
           answers without reading the environment).  The frame is compared with the reduction of the pair's records
  context  the same frame through a 1-spp accumulator pass + rtr_accum_resolve_device, and the relMSE of the k = 2 preview
           against the golden path-traced images at their sizes: mean over pixels and channels of (p - g)^2 / (g^2 + 0.01)

HIP events on the context's stream, one warm-up, median of 5 windows of back-to-back calls, reported per call; pairs are
timed twice in alternating order (a b b a) and both figures are printed."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import _golden as G
import _preview_ref as PR
from time_probes import pair, timed

A = G.A
N = G.rtr.native
rtr = G.rtr
SIDE = 800
GOLDEN = {21: "img_scene21_i4_128_spp32.f64", 23: "img_scene23_i4_64_spp16.f64"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def bake(ctx, sc):
    """(the IblEnvironment, its rtr_shade_env over device copies, what keeps them alive)"""
    prm = A.make_params(64, 64, 1, integrator=A.INTEGRATOR_MIS)
    s = ctx.preview_samples(N.preview_params(64, 64, 1))
    p = s["q"]["p"][s["kind"] == PR.SURFACE]
    lo, hi = p.min(axis=0), p.max(axis=0)
    grid = rtr.ProbeGrid.in_box(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), (8, 8, 8))
    grid.bake(ctx, prm, samples=64, seed=3, depth=16, classify=True)
    cube = rtr.Cubemap(ctx.capture_cube_records(prm, (0.5 * (lo + hi))[None, :], face_size=64, samples=16, seed=3)[0])
    ibl = rtr.IblEnvironment(grid, cube.prefilter(levels=5, ctx=ctx), rtr.BrdfTable.make(64, 64, 128, ctx=ctx))
    host = ibl.env()
    vis = N.probe_visible_params(16, 0.25 * float(grid.spacing.min()))
    keep = [dev(grid.coefficients), dev(grid.depth), dev(ibl.chain.records), dev(ibl.table.entries)]
    env = N.shade_env(keep[3].data_ptr(), grid=grid.grid(), probes=keep[0].data_ptr(), depth=keep[1].data_ptr(), visible=vis,
                      levels=ibl.chain.levels, chain=keep[2].data_ptr(), n_records=host.n_records, n_mu=64, n_rough=64)
    return ibl, env, keep


def rel_mse(p, g):
    return float(np.mean((p - g) ** 2 / (g ** 2 + 0.01)))


def main():
    ctx = rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    for sid in (21, 23):
        sc = G.scene(sid)
        ctx.upload(sc)
        ibl, env, keep = bake(ctx, sc)
        d_lin = torch.zeros(SIDE * SIDE * 3, dtype=torch.float64, device="cuda")
        d_lit = torch.zeros(SIDE * SIDE, dtype=torch.int32, device="cuda")
        for k in (1, 2):
            p = N.preview_params(SIDE, SIDE, k)
            n = SIDE * SIDE * k * k
            rays = PR.numpy_rays(sc.camera, SIDE, SIDE, k)
            samples = ctx.preview_samples(p)
            d_rays, d_q = dev(rays), dev(np.ascontiguousarray(samples["q"]))
            d_hits = torch.zeros(n * A.RAY_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(n * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def two():
                ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), n)
                ctx.shade_ibl_into(env, d_q.data_ptr(), d_out.data_ptr(), n)

            a, b = pair(two, lambda: ctx.preview_into(p, env, d_lin.data_ptr(), SIDE, d_lit.data_ptr()))
            cast = timed(lambda: ctx.query_closest_into(d_rays.data_ptr(), d_hits.data_ptr(), n))
            d_sam = torch.zeros(n * A.PREVIEW_SAMPLE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            g_buf = timed(lambda: ctx.preview_samples_into(p, d_sam.data_ptr()))
            torch.cuda.synchronize()
            # the frame against the reduction of the pair's records
            rec = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE).reshape(SIDE, SIDE, k * k)
            surf = samples["kind"] == PR.SURFACE
            add = np.where(surf[..., None], rec["v"], samples["direct"])
            counted = np.where(surf, rec["valid"] == 1, True)
            acc = np.zeros((SIDE, SIDE, 3))
            for s in range(k * k):
                acc = np.where(counted[:, :, s, None], acc + add[:, :, s], acc)
            want = np.float64(1.0 / (k * k)) * acc
            lin = d_lin.cpu().numpy().reshape(SIDE, SIDE, 3)
            lit = d_lit.cpu().numpy().reshape(SIDE, SIDE)
            same = lin.tobytes() == want.tobytes() and np.array_equal(lit, counted.sum(axis=2))
            hits = d_hits.cpu().numpy().view(A.RAY_HIT_DTYPE)
            print("fused   scene %d  %d x %d  k = %d  %d rays (%.3f surface, %.3f of those lit)   query + shade %8.3f %8.3f ms (query alone "
                  "%.3f)   preview %8.3f %8.3f ms   preview / pair = %.2f   samples form %.3f ms   %.1f Mrays/s   frame equals the "
                  "pair's reduction: %s   pair's hits %d" %
                  (sid, SIDE, SIDE, k, n, float(surf.mean()), float((rec["valid"][surf] == 1).mean()), a[0], a[1], cast, b[0], b[1],
                   sum(b) / sum(a), g_buf, n / (sum(b) / 2) * 1e-3, same, int(hits["hit"].sum())), flush=True)
            del d_rays, d_q, d_hits, d_out, d_sam
        # context: a 1-spp accumulator pass + resolve of the same frame
        rp = A.make_params(SIDE, SIDE, 1, integrator=A.INTEGRATOR_MIS, seed=1)
        with ctx.accumulator(rp) as acc1:
            def one_spp():
                acc1.reset(1)
                acc1.render(1, blocking=False)
                acc1.resolve_into(d_lin.data_ptr(), SIDE)
            spp1 = timed(one_spp)
        gold, info = G.image(GOLDEN[sid])
        side, rows = info["width"], info["height"]
        pv = ibl.render(ctx, N.preview_params(side, rows, 2))
        print("context scene %d  1-spp accumulator pass + resolve at %d x %d: %8.3f ms   relMSE of the k = 2 preview against %s "
              "(%d x %d): %.4f" % (sid, SIDE, SIDE, spp1, GOLDEN[sid], side, rows, rel_mse(pv, gold)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
