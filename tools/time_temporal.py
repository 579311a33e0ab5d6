#!/usr/bin/env python3
"""Cost and gain of the temporal stage (include/rtr_hip.h: rtr_set_camera / rtr_accum_reset / rtr_accum_denoise_temporal).

  1. Accumulator.denoise against Accumulator.denoise_temporal on C2 -- scene 21, 800 x 800, 4 spp in the accumulator,
     features cached -- one warm-up, median of 5.  Both calls block, so the HIP events around them time the WHOLE call
     (kernels, the 15 MB D2H copy, the stream wait and the host scatter), not the device time of a stage: what the
     temporal stage costs is the DIFFERENCE of the two lines (two more kernels; the copies are the same).
  2. Wall time of one rtr_set_camera + rtr_accum_reset against one rtr_upload_scene, scenes 21 and 24, median of 5.
  3. Static camera, 8 frames of 4 spp under 8 seeds, 128 x 128, scenes 21 / 22 / 23: relative MSE against a 1024-spp render
     of frame 8 with the history over frame 8 alone, for a sweep of alpha_min.
  4. A walking camera (the walk of tests/test_temporal.py, 6 frames), same scenes: relative MSE of the last frame against a
     1024-spp render from its camera, temporal over spatial, for a sweep of tau_z, tau_n and min_weight.

  tools/time_temporal.py [--quick]     --quick: parts 1 and 2 only
"""
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import _golden as G
import _temporal_ref as T

A = G.A
rtr = G.rtr
SPP = 4


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


def wall(fn):
    fn()
    s = []
    for _ in range(5):
        t = time.perf_counter()
        fn()
        s.append((time.perf_counter() - t) * 1e3)
    return statistics.median(s)


def relmse(x, r):
    return float(np.mean((x - r) ** 2 / (r * r + 1e-2)))


def walk(sc, n):
    cam = T.camera_dict(sc.camera)
    step = 0.04 * np.sqrt(cam["horizontal"] @ cam["horizontal"])
    return [T.moved_camera(cam, translate=k * (step * cam["u"] + 0.37 * step * cam["v"]), yaw_deg=3.0 * k) for k in range(n)]


def sequence(ctx, p, cams, tp):
    """relMSE ratio temporal / spatial of the last frame (the reference: 1024 spp from the last camera)"""
    with ctx.accumulator(p, moments=True) as acc, ctx.history(p) as hist:
        for k, cam in enumerate(cams):
            ctx.set_camera(cam)
            acc.reset(1 + k)
            acc.render(SPP)
            temporal = acc.denoise_temporal(hist, temporal=tp)
        alone = acc.denoise()
    return temporal, alone


def main():
    quick = "--quick" in sys.argv
    ctx = rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library works on
    ctx.set_stream(stream.cuda_stream)
    sc = G.scene(21)
    ctx.upload(sc)
    p = A.make_params(800, 800, 1, seed=1)
    with ctx.accumulator(p, moments=True) as acc, ctx.history(p) as hist:
        acc.render(SPP)
        out = np.zeros((800, 800, 3))
        plain = timed(lambda: acc.denoise(out=out))
        temporal = timed(lambda: acc.denoise_temporal(hist, out=out))
        print("C2 (scene 21, 800 x 800), whole blocking call (kernels + D2H + host scatter): denoise %.3f ms, "
              "denoise_temporal %.3f ms; the temporal stage adds %.3f ms (%.1f %%)" %
              (plain, temporal, temporal - plain, 100.0 * (temporal - plain) / plain), flush=True)
    for sid in (21, 24):
        sc = G.scene(sid)
        ctx.upload(sc)
        cam2 = T.camera_record(walk(sc, 2)[1])
        with ctx.accumulator(A.make_params(800, 800, 1, seed=1), moments=True) as acc:
            def update():
                ctx.set_camera(cam2)
                acc.reset(2)
            t_set = wall(update)
        t_up = wall(lambda: ctx.upload(sc))
        print("scene %02d: rtr_set_camera + rtr_accum_reset %.3f ms, rtr_upload_scene %.3f ms (%.0f x)" %
              (sid, t_set, t_up, t_up / t_set), flush=True)
    if quick:
        ctx.close()
        return
    S = 128
    for sid in (21, 22, 23):
        sc = G.scene(sid)
        ctx.upload(sc)
        p = A.make_params(S, S, 1, seed=1)
        ref = ctx.render(A.make_params(S, S, 1024, seed=11))
        for alpha_min in (0.02, 0.05, 0.1, 0.2, 0.5):
            t, s = sequence(ctx, p, [sc.camera] * 8, rtr.native.temporal_defaults(alpha_min=alpha_min))
            print("scene %02d static  alpha_min %.2f: relMSE temporal %.4g spatial %.4g ratio %.3f" %
                  (sid, alpha_min, relmse(t, ref), relmse(s, ref), relmse(t, ref) / relmse(s, ref)), flush=True)
        cams = walk(sc, 6)
        ctx.set_camera(cams[-1])
        ref = ctx.render(A.make_params(S, S, 1024, seed=11))
        d = rtr.native.temporal_defaults()
        combos = [dict()] + [dict(tau_z=v) for v in (0.02, 0.05, 0.3)] + [dict(tau_n=v) for v in (0.05, 1.0)] + \
                 [dict(min_weight=v) for v in (0.05, 0.6)] + [dict(alpha_min=v) for v in (0.1, 0.2)]
        for kw in combos:
            t, s = sequence(ctx, p, cams, rtr.native.temporal_defaults(**kw))
            print("scene %02d walking %-18s: relMSE temporal %.4g spatial %.4g ratio %.3f" %
                  (sid, ", ".join("%s %.2f" % kv for kv in kw.items()) or "defaults (%.2f %.2f %.2f %.2f)" %
                   (d.alpha_min, d.tau_z, d.tau_n, d.min_weight), relmse(t, ref), relmse(s, ref), relmse(t, ref) / relmse(s, ref)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
