#!/usr/bin/env python3
"""Times of the capture sets (include/rtr_hip.h: rtr_shade_ibl_set_device, rtr_preview_set_device) on one context, each
against the plain entry it extends, timed in the same call.

  shade    10^6 rtr_shade_ibl_set_device queries against rtr_shade_ibl_device over the same queries, in the setup of
           tools/time_shade.py (8 x 8 x 8 grid, maps of T = 16, five levels of S = 64, a 64 x 64 table; random records, no
           scene).  Sets: C = 1 whose volume reaches nothing (fallback 0: the plain shader's arithmetic), C = 1 that reaches
           every query, C = 4 and C = 16 slabs along x of which two reach a typical query.  The first 2000 records are
           compared with rtr_shade_ibl_set_one
  preview  rtr_preview_set_device against rtr_preview_device at 800 x 800, k = 1 and 2, scenes 21 and 23: the bake of
           tools/time_preview.py, and beside it a set of 2 x 2 x 2 captures at the quarter points of the bounding box of the
           first hits, proxy = that box, reach = the capture's octant grown by a quarter of its size on every side, fade = that
           quarter; same face size, samples and levels.  The relMSE of the k = 2 frame against the golden path-traced
           images, single capture and set

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
from time_preview import GOLDEN, SIDE, bake, dev, rel_mse

A = G.A
N = G.rtr.native
rtr = G.rtr


def volume(centre, proxy_lo, proxy_hi, reach_lo, reach_hi, fade):
    v = np.zeros((), dtype=A.CAPTURE_VOLUME_DTYPE)
    v["centre"], v["proxy_lo"], v["proxy_hi"], v["reach_lo"], v["reach_hi"], v["fade"] = centre, proxy_lo, proxy_hi, reach_lo, reach_hi, fade
    return v


def slabs(C, lo=-1.0, hi=8.0):
    """C volumes over [lo, hi]^3, slabs along x that overlap by half: two reach a point that is not in an end slab's outer half"""
    w = (hi - lo) / (C + 1)
    out = []
    for k in range(C):
        cx = lo + (k + 1) * w
        out.append(volume((cx, 3.5, 3.5), (lo,) * 3, (hi,) * 3, (cx - w, lo, lo), (cx + w, hi, hi), 0.5 * w))
    return np.array(out)


def shade(ctx):
    rng = np.random.default_rng(1)
    T, S, LEVELS, nq, NT = 16, 64, 5, 1000000, 64
    probes = np.zeros(512, dtype=A.PROBE_SH_DTYPE)
    probes["c"], probes["valid"] = rng.standard_normal((512, 9, 3)), 1
    depth = np.zeros((512, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    depth["mean"] = 0.3 + rng.random(depth.shape) * 1.2
    depth["mean2"] = depth["mean"] ** 2 + rng.random(depth.shape) * 0.1
    depth["valid"] = 1
    levels, n_records = N.cube_chain_plan(S, LEVELS)
    table = np.zeros((NT, NT), dtype=A.BRDF_ENTRY_DTYPE)
    table["a"], table["b"] = rng.random((NT, NT)), rng.random((NT, NT)) * 0.1
    grid = N.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (8, 8, 8))
    vp = N.probe_visible_params(T, 0.25)
    p, n, v = rng.random((nq, 3)) * 7.0, rng.standard_normal((nq, 3)), rng.standard_normal((nq, 3))
    q = N.shade_queries(p, n, v, rng.random((nq, 3)), rng.random(nq), rng.random(nq))
    d_probes, d_depth, d_table, d_q = dev(probes), dev(depth), dev(table), dev(q)
    d_out, d_out2 = (torch.zeros(nq * A.GATHER_OUT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
    far = volume((100.0,) * 3, (90.0,) * 3, (110.0,) * 3, (95.0,) * 3, (105.0,) * 3, 0.0)
    whole = volume((3.5,) * 3, (-1.0,) * 3, (8.0,) * 3, (-1.0,) * 3, (8.0,) * 3, 0.0)
    for name, vols, fallback in (("C = 1, reaches nothing, fallback 0", np.array([far]), 0), ("C = 1, reaches every query", np.array([whole]), -1),
                                 ("C = 4 slabs", slabs(4), -1), ("C = 16 slabs", slabs(16), -1)):
        C_ = len(vols)
        cset = N.capture_set(vols, fallback)
        rec = np.zeros(C_ * n_records, dtype=A.GATHER_OUT_DTYPE)
        rec["v"], rec["count"], rec["valid"] = rng.random((C_ * n_records, 3)), 4, 1
        d_rec = dev(rec)
        kw = dict(grid=grid, probes=d_probes.data_ptr(), depth=d_depth.data_ptr(), visible=vp, levels=levels, n_mu=NT, n_rough=NT)
        env_set = N.shade_env(d_table.data_ptr(), chain=d_rec.data_ptr(), n_records=n_records, **kw)
        env_one = N.shade_env(d_table.data_ptr(), chain=d_rec.data_ptr(), n_records=n_records, **kw)  # the plain shader over the same bytes, read as one chain
        torch.cuda.synchronize()
        a, b = pair(lambda: ctx.shade_ibl_into(env_one, d_q.data_ptr(), d_out2.data_ptr(), nq),
                    lambda: ctx.shade_ibl_into(env_set, d_q.data_ptr(), d_out.data_ptr(), nq, captures=cset))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(A.GATHER_OUT_DTYPE)
        host = N.shade_env(table, grid=grid, probes=probes, depth=depth, visible=vp, levels=levels, chain=rec, n_records=n_records)
        same = got[:2000].tobytes() == N.shade_ibl_set_one(host, cset, q[:2000]).tobytes()
        reach = np.zeros(nq, dtype=np.int32)
        for vol in vols:
            reach += ((p >= vol["reach_lo"]) & (p <= vol["reach_hi"])).all(axis=1)
        print("shade   %-36s %d queries   plain %8.3f %8.3f ms   set %8.3f %8.3f ms   set - plain = %+.3f ms   set / plain = %.2f   "
              "captures reaching a query: mean %.2f   valid %.3f   2000 records equal rtr_shade_ibl_set_one: %s" %
              (name, nq, a[0], a[1], b[0], b[1], (sum(b) - sum(a)) / 2, sum(b) / sum(a), float(reach.mean()),
               float((got["valid"] == 1).mean()), same), flush=True)
        del d_rec


def octants(lo, hi):
    """2 x 2 x 2 volumes at the quarter points of the box [lo, hi]"""
    half = 0.5 * (hi - lo)
    grow = 0.25 * half
    out = []
    for iz in (0, 1):
        for iy in (0, 1):
            for ix in (0, 1):
                o = lo + half * np.array([ix, iy, iz])
                out.append(volume(o + 0.5 * half, lo, hi, np.maximum(o - grow, lo), np.minimum(o + half + grow, hi), float(grow.min())))
    return np.array(out)


def preview(ctx):
    for sid in (21, 23):
        sc = G.scene(sid)
        ctx.upload(sc)
        ibl, env, keep = bake(ctx, sc)
        prm = A.make_params(64, 64, 1, integrator=A.INTEGRATOR_MIS)
        s = ctx.preview_samples(N.preview_params(64, 64, 1))
        pts = s["q"]["p"][s["kind"] == PR.SURFACE]
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        pad = 1e-6 * (hi - lo)  # the hits themselves lie on the box: keep them inside every rule
        vols = octants(lo - pad, hi + pad)
        cs = rtr.CaptureSet.bake(ctx, prm, vols, face_size=64, samples=16, levels=5, fallback=-1, seed=3)
        d_set = dev(cs.records)
        host = ibl.env()
        env_set = N.shade_env(keep[3].data_ptr(), grid=ibl.grid.grid(), probes=keep[0].data_ptr(), depth=keep[1].data_ptr(),
                              visible=N.probe_visible_params(16, 0.25 * float(ibl.grid.spacing.min())), levels=cs.levels,
                              chain=d_set.data_ptr(), n_records=cs.n_records, n_mu=64, n_rough=64)
        d_lin = torch.zeros(SIDE * SIDE * 3, dtype=torch.float64, device="cuda")
        d_lit = torch.zeros(SIDE * SIDE, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for k in (1, 2):
            p = N.preview_params(SIDE, SIDE, k)
            a, b = pair(lambda: ctx.preview_into(p, env, d_lin.data_ptr(), SIDE, d_lit.data_ptr()),
                        lambda: ctx.preview_into(p, env_set, d_lin.data_ptr(), SIDE, d_lit.data_ptr(), captures=cs.set()))
            print("preview scene %d  %d x %d  k = %d   rtr_preview_device %8.3f %8.3f ms   rtr_preview_set_device (C = %d) %8.3f %8.3f ms   "
                  "set / plain = %.2f" % (sid, SIDE, SIDE, k, a[0], a[1], len(vols), b[0], b[1], sum(b) / sum(a)), flush=True)
        gold, info = G.image(GOLDEN[sid])
        pp = N.preview_params(info["width"], info["height"], 2)
        one = ibl.render(ctx, pp)
        many = rtr.IblEnvironment(ibl.grid, cs, ibl.table).render(ctx, pp)
        print("buys    scene %d  relMSE of the k = 2 preview against %s (%d x %d): single capture %.4f, set of %d captures %.4f   "
              "box %s .. %s" % (sid, GOLDEN[sid], info["width"], info["height"], rel_mse(one, gold), len(vols), rel_mse(many, gold),
                                np.round(lo, 3).tolist(), np.round(hi, 3).tolist()), flush=True)
        del d_set, keep


def main():
    ctx = rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    shade(ctx)
    preview(ctx)
    ctx.close()


if __name__ == "__main__":
    main()
