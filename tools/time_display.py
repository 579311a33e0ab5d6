#!/usr/bin/env python3
"""Cost of the display transform (include/rtr_hip.h: rtr_display_device) next to the denoiser it follows.

  1. rtr_display_device on an 800 x 800 device image (scene 21 rendered at 4 spp, so the luminances are a real frame's),
     bytes only, for each tone curve x encoding with auto exposure off (k_display_scale + k_display_apply) and on (the
     histogram memset + k_display_meter in front).  Non-blocking calls on the library's stream between two HIP events:
     one warm-up window, then ROUNDS windows of CALLS calls per configuration, the configurations interleaved; per-call
     time = window / CALLS; median and minimum over the windows.  No copy and no host wait is inside a window.
  2. Accumulator.denoise on C2 (scene 21, 800 x 800, 4 spp, features cached) in the same process: the WHOLE blocking
     call (kernels, the 15 MB D2H copy, the stream wait, the host scatter), as tools/time_temporal.py times it.
  3. Context.display, the blocking host entry (15 MB up, 1.9 MB down), for scale.

  tools/time_display.py
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
rtr = G.rtr
S, SPP, CALLS, ROUNDS = 800, 4, 50, 7
CURVES = (("clamp", A.TONE_CLAMP), ("reinhard", A.TONE_REINHARD), ("aces", A.TONE_ACES))
ENCODINGS = (("gamma2", A.ENCODE_GAMMA2), ("srgb", A.ENCODE_SRGB))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ctx = rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events are recorded on the stream the library works on
    ctx.set_stream(stream.cuda_stream)
    ctx.upload(G.scene(21))
    fb = torch.zeros((S, S, 3), dtype=torch.float64, device="cuda")
    rgb = torch.zeros((S, S, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.render_into(A.make_params(S, S, SPP, seed=1), fb.data_ptr(), S, blocking=True)
    configs = []
    for auto in (0, 1):
        for cname, curve in CURVES:
            for ename, enc in ENCODINGS:
                prm = rtr.native.display_defaults(auto_exposure=auto, tone_curve=curve, encoding=enc)
                configs.append(("auto %d %-8s %-6s" % (auto, cname, ename),
                                lambda prm=prm: ctx.display_into(fb.data_ptr(), S, S, S, rgb.data_ptr(), prm)))
    times = {name: [] for name, _ in configs}
    for name, fn in configs:  # warm-up: every configuration once
        window(fn, CALLS)
    for _ in range(ROUNDS):
        for name, fn in configs:
            times[name].append(window(fn, CALLS))
    print("rtr_display_device, %d x %d device image, bytes only, %d windows of %d calls (ms per call):" % (S, S, ROUNDS, CALLS))
    for name, _ in configs:
        print("  %s  median %.4f  min %.4f" % (name, statistics.median(times[name]), min(times[name])), flush=True)
    res = ctx.display_into(fb.data_ptr(), S, S, S, rgb.data_ptr(),
                           rtr.native.display_defaults(auto_exposure=1, tone_curve=A.TONE_ACES, encoding=A.ENCODE_SRGB), blocking=True)
    print("  (auto exposure metered %d of %d pixels: scale %.6g)" % (res["n_metered"], S * S, res["scale"]))
    with ctx.accumulator(A.make_params(S, S, 1, seed=1), moments=True) as acc:
        acc.render(SPP)
        out = np.zeros((S, S, 3))
        acc.denoise(out=out)
        t = [window(lambda: acc.denoise(out=out), 1) for _ in range(ROUNDS)]
        print("Accumulator.denoise on C2, whole blocking call (kernels + D2H + host scatter): median %.3f ms  min %.3f ms" %
              (statistics.median(t), min(t)), flush=True)
        prm = rtr.native.display_defaults(auto_exposure=1, tone_curve=A.TONE_ACES, encoding=A.ENCODE_SRGB)
        ctx.display(out, prm)
        t = [window(lambda: ctx.display(out, prm), 1) for _ in range(ROUNDS)]
        print("Context.display (host entry: 15 MB H2D, kernels, 1.9 MB D2H): median %.3f ms  min %.3f ms" %
              (statistics.median(t), min(t)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
