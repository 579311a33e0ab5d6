#!/usr/bin/env python3
"""Times of the filtered cube maps (include/rtr_hip.h: rtr_cube_filter_device, rtr_cube_chain_lookup_device) on one
context, from synthetic texels: the five-level chain of rtr_cube_chain_plan at S = 64, 128 and 256 -- four filters of
level 0, face sizes S/2 .. S/16, alphas (i/4)^2, cos_cut 0 --, then 10^6 chain lookups in the S = 64 chain, and beside
them the host route the filter replaces: rtr_cube_filter_one looped on the CPU over the same S = 64 chain.

  pairs      (output texel, source texel) pairs of the four filters: 6 S^2 x the output texels
  used       the pairs with c > cos_cut, summed from the records' counts: only these reach the weight and the sums
  FP64       counted operations, a fused multiply-add as two: 6 per pair (the dot product and the compare), 27 more per
             used pair (h2 2, den 2, den^2 1, c dw 1, the division's short form 14 = rcp + 6 fma + 1 mul, the four sums
             7), against the 78.6 TFLOP/s vector peak bench.py uses

HIP events on the context's stream, one warm-up, median of 5 windows of back-to-back calls, reported per call."""
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

A = G.A
N = G.rtr.native
PEAK = 78.6e12
LEVELS = 5


def timed(fn, calls):
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
    return statistics.median(ms), min(ms), max(ms)


def synthetic(S):
    rng = np.random.default_rng(S)
    t = np.zeros(6 * S * S, dtype=A.GATHER_OUT_DTYPE)
    t["v"] = rng.uniform(0.0, 4.0, (len(t), 3))
    t["count"], t["valid"] = 16, 1
    return t


def main():
    ctx = G.rtr.Context(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)  # the events of timed() are recorded on the stream the library runs on
    ctx.set_stream(stream.cuda_stream)
    sizes = [int(a) for a in sys.argv[1:]] or [64, 128, 256]
    chain64 = None
    for S in sizes:
        plan, n_records = N.cube_chain_plan(S, LEVELS)
        rec = np.zeros(n_records, dtype=A.GATHER_OUT_DTYPE)
        rec[:6 * S * S] = synthetic(S)
        d_chain = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        base = d_chain.data_ptr()
        params = [N.cube_filter_defaults(face_in=S, face_out=lv.face_size, alpha=lv.alpha) for lv in list(plan)[1:]]

        def chain():
            for lv, fp in zip(list(plan)[1:], params):
                ctx.cube_filter_into(base, base + lv.offset * 32, 1, fp)

        ms, lo, hi = timed(chain, calls=max(1, (128 // S) ** 2))
        got = d_chain.cpu().numpy().view(A.GATHER_OUT_DTYPE)
        outputs = n_records - 6 * S * S
        pairs = 6 * S * S * outputs
        used = int(got["count"][6 * S * S:].astype(np.int64).sum())
        flops = 6 * pairs + 27 * used
        print("chain S = %3d  %d levels  %8.3f ms (%.3f .. %.3f)  %.3e pairs  %6.1f Gpairs/s  used %.3f  %5.2f TFLOP/s FP64 = %.3f of peak" %
              (S, LEVELS, ms, lo, hi, pairs, pairs / ms * 1e-6, used / pairs, flops / ms * 1e-9, flops / (ms * 1e-3) / PEAK), flush=True)
        # the largest call of the chain: level 1 alone
        l1, _, _ = timed(lambda: ctx.cube_filter_into(base, base + plan[1].offset * 32, 1, params[0]), calls=max(1, (128 // S) ** 2))
        print("chain S = %3d  level 1 alone (%d -> %d)  %8.3f ms  %.3e pairs" % (S, S, plan[1].face_size, l1, 6 * S * S * 6 * plan[1].face_size ** 2),
              flush=True)
        if S == 64:
            chain64 = (plan, n_records, got.copy(), d_chain)
    if chain64 is not None:
        plan, n_records, rec, d_chain = chain64
        nq = 1000000
        rng = np.random.default_rng(1)
        q = N.cube_queries(rng.standard_normal((nq, 3)), rng.uniform(0.0, 1.0, nq))
        d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
        d_out = torch.zeros(nq * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms, lo, hi = timed(lambda: ctx.cube_chain_lookup_into(plan, d_chain.data_ptr(), n_records, d_q.data_ptr(), d_out.data_ptr(), nq),
                           calls=20)
        print("chain lookup  %d queries, S = 64, %d levels  %8.3f ms (%.3f .. %.3f)  %8.1f Mqueries/s" % (nq, LEVELS, ms, lo, hi, nq / ms * 1e-3),
              flush=True)
        # the host route: rtr_cube_filter_one over every output texel of the same chain, one CPU thread
        t0 = time.perf_counter()
        host = [N.cube_filter_host(rec[:6 * 64 * 64], face_in=64, face_out=lv.face_size, alpha=lv.alpha) for lv in list(plan)[1:]]
        cpu_s = time.perf_counter() - t0
        same = all(np.array_equal(h.reshape(-1).view(np.uint8), rec[lv.offset:lv.offset + h.size].view(np.uint8))
                   for h, lv in zip(host, list(plan)[1:]))
        print("host route  rtr_cube_filter_one looped, S = 64 chain  %8.1f ms on one CPU thread   records equal the device's: %s" %
              (cpu_s * 1e3, same), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
