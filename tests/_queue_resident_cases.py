"""Cases of tests/test_queue_resident_state.py: the smallest renders that reach the state k_mega_queue
(csrc/rt_kernels.h) keeps between iterations -- ray B's request, always resident in the parked words, the dummy ray A of
a lane that waits for its job switch, and the wave's queue state in LDS -- each rendered with the job queue and with
RTR_FLAG_STATIC_GRID in one context.  Run as a program it renders the cases of ONE_WORKGROUP and prints the outcomes as
one JSON line: the test starts it as a child process with RTR_QUEUE_WORKGROUPS=1 in its environment.  Test
infrastructure only."""
import json
import os
import sys

import numpy as np

FILL = -7.0  # what the caller's buffer holds before a render

# name -> (width, height, spp, make_params keywords)
CASES = {
    # every job is one sample long: a lane is at a job switch (dummy A, dead request) after each sample it renders.
    # (LEFT OUT: "empty_ranges", 32x32 spp 3 with spp_chunks = 4 -- sample ranges [0,0) [0,1) [1,2) [2,3).  make_params
    # takes it, but rtr_render_* rejects more chunks than samples for either kernel: "spp_chunks must be in [0, spp]".
    # No render has an empty sample range; the null jobs that exist are the pixels outside a region, the next case.)
    "one_sample_jobs": (32, 32, 3, dict(spp_chunks=3)),
    # every block of the border tiles has lanes with and without a pixel
    "region": (48, 32, 8, dict(spp_chunks=1, region=(3, 5, 45, 30))),
    # a sample ends in its first iteration, its request still parked: the next sample's camera ray is cast beside it
    "depth_one": (16, 16, 1, dict(spp_chunks=1, max_depth=1)),
}
# in a process whose persistent grid is one workgroup: four waves eat every block of the one tile and run dry at
# different iterations (one block each with one chunk, four each with four)
ONE_WORKGROUP = {
    "one_workgroup": (16, 16, 16, dict(spp_chunks=1)),
    "one_workgroup_chunks": (16, 16, 16, dict(spp_chunks=4)),
}
SCENES = ("21", "23", "flat_full")


def scene(G, name):
    """scene 21 (the lean pair kernel), scene 23 (QuadLights only) and a pair scene of the full material set"""
    if name != "flat_full":
        return G.scene(int(name))
    import _flatscenes as F
    return full_flat_scene(F)


def full_flat_scene(F):
    """tests/_flatscenes.flat_scene -- four frames, every transform chain the pair cast has a shape for -- with the
    point light of tests/_randscene.random_scene beside its QuadLight: a delta light takes a scene out of the lean and
    the QuadLights-only material sets, and nothing else about it changes"""
    sc = F.flat_scene(0, "TR")
    point = np.zeros(1, dtype=F.A.LIGHT_DTYPE)
    point["type"] = F.A.LIGHT_POINT
    point["f"][0, :6] = [3.0, 4.5, 1.0, 9.0, 8.0, 6.0]
    return F.rtr.Scene(sc.root, sc.nodes, sc.list_children, sc.materials, sc.textures, sc.perlin, sc.images, sc.image_bytes,
                       np.concatenate([sc.lights, point]), sc.camera, sc.background)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _counts(st):
    return [int(st["samples"]), int(st["closest_segments"]), int(st["shadow_segments"])]


def run_case(ctx, A, spec):
    """outcome of one case on the scene ``ctx`` holds, as a dict of plain values"""
    W, H, spp, kw = spec
    kw = dict(integrator=4, seed=11, pipeline=A.PIPELINE_MEGAKERNEL, **kw)
    pq, ps = A.make_params(W, H, spp, **kw), A.make_params(W, H, spp, flags=A.FLAG_STATIC_GRID, **kw)
    h, w = pq.y1 - pq.y0, pq.x1 - pq.x0
    queue = ctx.render(pq, out=np.full((h, w, 3), FILL))
    sq = ctx.stats()
    static = ctx.render(ps, out=np.full((h, w, 3), FILL))
    ss = ctx.stats()
    return {"same_bytes": bool(queue.tobytes() == static.tobytes()), "counts_queue": _counts(sq), "counts_static": _counts(ss),
            "cancelled": [bool(sq["cancelled"]), bool(ss["cancelled"])],
            "flag_queue": bool(sq["flags_in_effect"] & A.FLAG_STATIC_GRID), "flag_static": bool(ss["flags_in_effect"] & A.FLAG_STATIC_GRID),
            "filled": int(np.any(queue == FILL, axis=2).sum()), "min": float(queue.min())}


def check(spec, r):
    W, H, spp, kw = spec
    x0, y0, x1, y1 = kw.get("region", (0, 0, W, H))
    assert r["same_bytes"], r
    assert r["counts_queue"] == r["counts_static"], r
    assert r["cancelled"] == [False, False], r
    assert r["flag_static"] and not r["flag_queue"], r  # the first render ran the queue, the second the static grid
    assert r["counts_queue"][0] == (x1 - x0) * (y1 - y0) * spp, r
    assert r["filled"] == 0 and r["min"] >= 0.0, r  # every pixel of the region was rendered


if __name__ == "__main__":
    try:
        import torch  # noqa: F401  (first to load the HIP runtime, as in tests/conftest.py)
    except ImportError:
        pass
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import _golden as G

    results = {}
    ctx = G.rtr.Context(0)
    for name in SCENES:
        ctx.upload(scene(G, name))
        for case, spec in ONE_WORKGROUP.items():
            results["%s.%s" % (name, case)] = run_case(ctx, G.A, spec)
    ctx.close()
    print("RESULTS " + json.dumps(results))
