"""Cases of tests/test_job_queue.py: a render with the job queue (csrc/rt_kernels.h: k_mega_queue) next to the same render
with RTR_FLAG_STATIC_GRID in one context.  Run as a program it renders every case and prints the outcomes as one JSON
line: the tests start it as a child process with RTR_QUEUE_WORKGROUPS=1 in its environment, where the four waves of one
workgroup eat every block of the image.  Test infrastructure only."""
import json
import os
import sys

import numpy as np

FILL = -7.0  # what the caller's buffer holds before a render

# name -> (width, height, spp, make_params keywords)
CASES = {
    "auto_chunks": (96, 64, 6, dict(spp_chunks=0)),
    "one_chunk": (96, 64, 6, dict(spp_chunks=1)),
    "three_chunks": (96, 64, 6, dict(spp_chunks=3)),
    "region": (80, 64, 6, dict(spp_chunks=3, region=(5, 3, 59, 45))),  # null jobs, partly covered tiles
    "region_auto": (80, 64, 6, dict(spp_chunks=0, region=(5, 3, 59, 45))),
    "strided_tiles": (96, 64, 6, dict(spp_chunks=3, tile_first=1, tile_stride=2)),  # the tile slots run with gaps
    "ragged_chunks": (96, 64, 7, dict(spp_chunks=3)),  # sample ranges 2, 2, 3
    "one_sample": (96, 64, 1, dict(spp_chunks=1)),
    "one_sample_auto": (96, 64, 1, dict(spp_chunks=0)),
}
SCENES = (21, 23)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _counts(st):
    return [int(st["samples"]), int(st["closest_segments"]), int(st["shadow_segments"])]


def run_case(ctx, A, name):
    """outcome of one case on the scene ``ctx`` holds, as a dict of plain values"""
    W, H, spp, kw = CASES[name]
    kw = dict(integrator=4, seed=5, pipeline=A.PIPELINE_MEGAKERNEL, **kw)
    pq, ps = A.make_params(W, H, spp, **kw), A.make_params(W, H, spp, flags=A.FLAG_STATIC_GRID, **kw)
    h, w = pq.y1 - pq.y0, pq.x1 - pq.x0
    queue = ctx.render(pq, out=np.full((h, w, 3), FILL))
    sq = ctx.stats()
    static = ctx.render(ps, out=np.full((h, w, 3), FILL))
    ss = ctx.stats()
    untouched = np.all(queue == FILL, axis=2)
    return {"same_bits": bool(np.array_equal(_bits(queue), _bits(static))), "counts_queue": _counts(sq), "counts_static": _counts(ss),
            "chunks": [sq["spp_chunks"], ss["spp_chunks"]], "cancelled": [bool(sq["cancelled"]), bool(ss["cancelled"])],
            "flag_queue": bool(sq["flags_in_effect"] & A.FLAG_STATIC_GRID), "flag_static": bool(ss["flags_in_effect"] & A.FLAG_STATIC_GRID),
            "untouched_pixels": int(untouched.sum()), "rendered_min": float(queue[~untouched].min()) if (~untouched).any() else None}


def after_cancel(ctx, A):
    """two renders issued after ctx.cancel() has returned: [cancelled, samples, expected samples] each"""
    out = []
    for _ in range(2):
        ctx.cancel()
        ctx.render(A.make_params(96, 64, 6, integrator=4, seed=5, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=3))
        st = ctx.stats()
        out.append([bool(st["cancelled"]), int(st["samples"]), 96 * 64 * 6])
    return out


def check(name, r):
    """what every case must show (the tests call this on outcomes of their own process and of the child's)"""
    W, H, spp, kw = CASES[name]
    x0, y0, x1, y1 = kw.get("region", (0, 0, W, H))
    assert r["same_bits"], (name, r)
    assert r["counts_queue"] == r["counts_static"], (name, r)
    assert r["chunks"][0] == r["chunks"][1], (name, r)  # the queue does not change the library's choice of chunks
    assert r["cancelled"] == [False, False], (name, r)
    assert r["flag_static"] and not r["flag_queue"], (name, r)
    # owned tiles, clipped to the region, are rendered (radiance >= 0); every other pixel keeps the caller's fill
    stride, first = kw.get("tile_stride", 1), kw.get("tile_first", 0)
    tx, ty = (W + 15) // 16, (H + 15) // 16
    owned = 0
    for t in range(first, tx * ty, stride):
        xs, ys = (t % tx) * 16, ((ty - 1) - t // tx) * 16
        owned += max(0, min(xs + 16, x1) - max(xs, x0)) * max(0, min(ys + 16, y1) - max(ys, y0))
    assert r["counts_queue"][0] == owned * spp, (name, r, owned)
    assert r["untouched_pixels"] == (x1 - x0) * (y1 - y0) - owned, (name, r, owned)
    assert r["rendered_min"] is not None and r["rendered_min"] >= 0.0, (name, r)


if __name__ == "__main__":
    try:
        import torch  # noqa: F401  (first to load the HIP runtime, as in tests/conftest.py)
    except ImportError:
        pass
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import _golden as G

    results = {}
    ctx = G.rtr.Context(0)
    for sid in SCENES:
        ctx.upload(G.scene(sid))
        for case in CASES:
            results["%d.%s" % (sid, case)] = run_case(ctx, G.A, case)
    ctx.upload(G.scene(21))
    results["after_cancel"] = after_cancel(ctx, G.A)
    ctx.close()
    print("RESULTS " + json.dumps(results))
