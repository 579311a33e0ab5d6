"""The job queue of the pair-cast megakernel (csrc/rt_kernels.h: k_mega_queue): a one-shot render of a pair-cast scene
runs a persistent grid whose lanes pull (pixel, chunk) jobs from a launch-wide queue; RTR_FLAG_STATIC_GRID selects the
one-workgroup-per-(tile, chunk) kernel it replaces.  A job is a cell of the static kernel's partial sums, summed in the
same order, so both must give the same image bit for bit and the same sample and segment counts, in every chunk mode.
The cases (tests/_job_queue_cases.py) run in this process with the full grid and once more in a child process with
RTR_QUEUE_WORKGROUPS=1, where one workgroup eats every block: a wave's several blocks, and the refill across block
boundaries, at a shape that takes a second."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _golden as G
import _job_queue_cases as Q

A = G.A
rtr = G.rtr
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_workgroup():
    """outcomes of every case in a fresh process whose persistent grid is capped at one workgroup"""
    env = dict(os.environ, RTR_QUEUE_WORKGROUPS="1")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [Q.__file__]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULTS ")]
    assert len(line) == 1, r.stdout.decode()[-2000:]
    return json.loads(line[0][len("RESULTS "):])


@pytest.mark.parametrize("case", list(Q.CASES))
@pytest.mark.parametrize("sid", Q.SCENES)
def test_queue_equals_static_grid(ctx, sid, case):
    assert "RTR_QUEUE_WORKGROUPS" not in os.environ
    ctx.upload(G.scene(sid))
    Q.check(case, Q.run_case(ctx, A, case))


@pytest.mark.parametrize("case", list(Q.CASES))
@pytest.mark.parametrize("sid", Q.SCENES)
def test_queue_equals_static_grid_with_one_workgroup(one_workgroup, sid, case):
    Q.check(case, one_workgroup["%d.%s" % (sid, case)])


@pytest.mark.parametrize("sid", Q.SCENES)
def test_pixels_outside_the_region_keep_the_fill(ctx, sid):
    """The region case into a device buffer of the whole image: only the region's pixels are written, with the bits of
    the static grid."""
    import torch
    ctx.upload(G.scene(sid))
    W, H, spp, kw = Q.CASES["region"]
    x0, y0, x1, y1 = kw["region"]
    got = {}
    for flags in (0, A.FLAG_STATIC_GRID):
        fb = torch.full((H, W, 3), Q.FILL, dtype=torch.float64, device="cuda")
        p = A.make_params(W, H, spp, integrator=4, seed=5, pipeline=A.PIPELINE_MEGAKERNEL, flags=flags, **kw)
        ctx.render_into(p, fb.data_ptr() + (y0 * W + x0) * 3 * 8, W, blocking=True)
        got[flags] = fb.cpu().numpy()
    img = got[0]
    inside = np.zeros((H, W), dtype=bool)
    inside[y0:y1, x0:x1] = True
    assert np.all(img[~inside] == Q.FILL)
    assert np.all(img[inside] >= 0.0)
    assert np.array_equal(_bits(img), _bits(got[A.FLAG_STATIC_GRID]))


def test_queue_equals_the_oracle(ctx):
    """One running sum per pixel (spp_chunks = 1) is the reference's own order: the queue render is the oracle's image."""
    sc = G.scene(21)
    ctx.upload(sc)
    p = A.make_params(64, 64, 16, integrator=4, seed=1, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    got = ctx.render(p)
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_STATIC_GRID == 0
    want, wst = G.oracle_render(sc, p)
    assert np.array_equal(_bits(got), _bits(want))
    assert (st["samples"], st["closest_segments"], st["shadow_segments"]) == \
        (wst["samples"], wst["closest_segments"], wst["shadow_segments"])


def test_render_after_cancel_is_complete(ctx, one_workgroup):
    """A render issued after cancel() has returned runs to the end: the block counter and the completion words are reset
    per render (the cancel itself is raced against a running render in tests/test_gpu_parity.py only)."""
    ctx.upload(G.scene(21))
    for cancelled, samples, expected in Q.after_cancel(ctx, A) + one_workgroup["after_cancel"]:
        assert not cancelled and samples == expected


def test_accumulator_passes_keep_the_static_grid(ctx):
    """The queue is a one-shot kernel: an accumulator's passes run the static grid whatever the flag says, do not report
    it, and continue the one-shot image."""
    ctx.upload(G.scene(21))
    kw = dict(integrator=4, seed=3, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    ref = ctx.render(A.make_params(64, 48, 10, **kw))
    for flags in (0, A.FLAG_STATIC_GRID):
        with ctx.accumulator(A.make_params(64, 48, 10, flags=flags, **kw)) as acc:
            acc.render(4)
            acc.render(10)
            assert ctx.stats()["flags_in_effect"] & A.FLAG_STATIC_GRID == 0
            assert np.array_equal(_bits(acc.resolve()), _bits(ref)), flags
