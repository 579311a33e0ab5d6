#!/usr/bin/env python3
"""One viewer frame through the host forms and through the device forms of the accumulator outputs (include/rtr_hip.h).

C2 (scene 21, 800 x 800, MIS), temporal denoise with the defaults, display with auto exposure, the ACES curve and sRGB
bytes; a static camera and one that orbits by 1.5 degrees per frame; 1, 4 and 16 samples per pixel and frame.  Per frame

  (a) host chain    set_camera, reset, blocking render, rtr_accum_denoise_temporal into a host image (15 MB D2H through
                    pageable memory, a per-pixel loop on the CPU), rtr_display_host (15 MB H2D, 1.9 MB D2H)
  (b) device chain  set_camera, reset, render, rtr_accum_denoise_temporal_device, rtr_display_device all queued on one
                    stream, one copy of the 1.9 MB of bytes into pinned memory behind them, one synchronise

each with an accumulator and a history of its own on ONE context.  One warm-up frame per chain grows the workspaces; then
FRAMES frames, (a) and (b) alternating frame by frame, each timed with a host clock from before set_camera to after the
bytes are on the host (both end in a wait for the device).  Reported per configuration: the median frame time of both,
(a)'s own spread (quartiles and extremes of its repeats), the median time the host spends inside the four enqueue calls
of (b) -- reset, render, denoise_temporal_into, display_into -- and whether (b)'s median lies below (a)'s by more than
(a)'s spread.  The last frame's bytes of both chains are compared: the two chains compute the same image.

  tools/time_frame.py [--frames N]
"""
import argparse
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
S = 800


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", type=int, default=S)
    args = ap.parse_args()
    if args.frames < 20:
        ap.error("at least 20 frames per chain")
    size = args.size
    ctx = rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the copy of the bytes is queued on the stream the library works on
    ctx.set_stream(stream.cuda_stream)
    sc = G.scene(21)
    ctx.upload(sc)
    cam0 = T.camera_dict(sc.camera)
    prm, tp = rtr.native.denoise_defaults(), rtr.native.temporal_defaults()
    dsp = rtr.native.display_defaults(auto_exposure=1, tone_curve=A.TONE_ACES, encoding=A.ENCODE_SRGB)
    p = A.make_params(size, size, 1, integrator=A.INTEGRATOR_MIS, seed=1)
    d_lin = torch.zeros((size, size, 3), dtype=torch.float64, device="cuda")
    d_rgb = torch.zeros((size, size, 3), dtype=torch.uint8, device="cuda")
    h_rgb = torch.zeros((size, size, 3), dtype=torch.uint8).pin_memory()
    h_lin = np.zeros((size, size, 3))
    torch.cuda.synchronize()
    print("scene 21, %d x %d, MIS, temporal denoise (defaults), display auto exposure / ACES / sRGB; %d frames per chain "
          "after one warm-up frame, (a) and (b) alternating; ms" % (size, size, args.frames))
    print("%-7s %3s | %9s %9s %9s %9s %9s | %9s %9s | %9s | %s" % ("camera", "spp", "(a) med", "(a) q1", "(a) q3", "(a) min",
                                                                    "(a) max", "(b) med", "(b) max", "(b) enq", "(a)-(b) against (a)'s spread"))
    with ctx.accumulator(p, moments=True) as acc_a, ctx.history(p) as hist_a, \
            ctx.accumulator(p, moments=True) as acc_b, ctx.history(p) as hist_b:

        def frame_a(cam, seed, spp):
            t0 = time.perf_counter()
            ctx.set_camera(cam)
            acc_a.reset(seed)
            acc_a.render(spp)
            acc_a.denoise_temporal(hist_a, prm, tp, out=h_lin)
            rgb = ctx.display(h_lin, dsp)[0]
            return time.perf_counter() - t0, 0.0, rgb

        def frame_b(cam, seed, spp):
            t0 = time.perf_counter()
            ctx.set_camera(cam)
            e0 = time.perf_counter()
            acc_b.reset(seed)
            acc_b.render(spp, blocking=False)
            acc_b.denoise_temporal_into(hist_b, d_lin.data_ptr(), size, None, prm, tp)
            ctx.display_into(d_lin.data_ptr(), size, size, size, d_rgb.data_ptr(), dsp)
            e1 = time.perf_counter()
            h_rgb.copy_(d_rgb, non_blocking=True)
            stream.synchronize()
            return time.perf_counter() - t0, e1 - e0, h_rgb.numpy()

        for name, yaw in (("static", 0.0), ("orbit", 1.5)):
            for spp in (1, 4, 16):
                hist_a.clear()
                hist_b.clear()
                ta, tb, enq = [], [], []
                same = True
                for k in range(args.frames + 1):  # frame 0 is the warm-up
                    cam = T.moved_camera(cam0, yaw_deg=yaw * k)
                    a, _, rgb_a = frame_a(cam, 100 + k, spp)
                    b, e, rgb_b = frame_b(cam, 100 + k, spp)
                    same = same and np.array_equal(rgb_a, rgb_b)
                    if k:
                        ta.append(1e3 * a), tb.append(1e3 * b), enq.append(1e3 * e)
                q1, med_a, q3 = statistics.quantiles(ta, n=4)
                med_b, gain = statistics.median(tb), statistics.median(ta) - statistics.median(tb)
                verdict = "%.3f: %s the quartile range %.3f, %s the full range %.3f" % (
                    gain, "above" if gain > q3 - q1 else "NOT above", q3 - q1,
                    "above" if gain > max(ta) - min(ta) else "NOT above", max(ta) - min(ta))
                print("%-7s %3d | %9.3f %9.3f %9.3f %9.3f %9.3f | %9.3f %9.3f | %9.3f | %s%s" % (
                    name, spp, med_a, q1, q3, min(ta), max(ta), med_b, max(tb), statistics.median(enq), verdict,
                    "" if same else "  BYTES DIFFER"), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
