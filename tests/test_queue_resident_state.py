"""What k_mega_queue (csrc/rt_kernels.h) keeps from one iteration to the next: ray B's request is always resident in the
parked words (dead, t_max = 0, or parked by the shading), a lane that waits for its job switch casts the dummy ray A,
and the wave's queue state -- its block, the cursor into it, the samples it has taken -- lives in LDS and is touched only
by the job switch and the cancel path.  None of it may show: a render with the queue and the same render with
RTR_FLAG_STATIC_GRID, in one context, give the same image byte for byte and the same sample and segment counts.  The
cases (tests/_queue_resident_cases.py) are the smallest shapes that reach those states, on scene 21 (the lean pair
kernel), scene 23 (QuadLights only) and a pair scene of the full material set; the one-workgroup cases run in a child
process with RTR_QUEUE_WORKGROUPS=1.  One planned case is left out by name: 32x32 spp 3 with spp_chunks = 4 (an empty
sample range), which the library rejects for the static grid as well ("spp_chunks must be in [0, spp]")."""
import json
import os
import subprocess
import sys

import pytest

import _golden as G
import _queue_resident_cases as Q

A = G.A
rtr = G.rtr
MS_OF = {"21": 0, "23": 2, "flat_full": 1}  # RT_MS_LEAN, RT_MS_QUADLIT, RT_MS_FULL


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    return {name: Q.scene(G, name) for name in Q.SCENES}


@pytest.fixture(scope="module")
def one_workgroup():
    """outcomes of the ONE_WORKGROUP cases in a fresh process whose persistent grid is capped at one workgroup"""
    env = dict(os.environ, RTR_QUEUE_WORKGROUPS="1")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [Q.__file__]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULTS ")]
    assert len(line) == 1, r.stdout.decode()[-2000:]
    return json.loads(line[0][len("RESULTS "):])


@pytest.mark.parametrize("name", Q.SCENES)
def test_scenes_run_the_three_queue_kernels(scenes, name):
    """(no GPU) each scene is a pair-cast scene of its own material set: together they run all three k_mega_queue"""
    plan = rtr.native.scene_plan(scenes[name], 4, 0)
    assert plan["mega_pair"] == 1 and plan["mega_ms"] == MS_OF[name], plan
    for spec in list(Q.CASES.values()) + list(Q.ONE_WORKGROUP.values()):  # the static grid renders every case
        W, H, spp, kw = spec
        A.make_params(W, H, spp, integrator=4, flags=A.FLAG_STATIC_GRID, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(Q.CASES))
@pytest.mark.parametrize("name", Q.SCENES)
def test_queue_equals_static_grid(ctx, scenes, name, case):
    assert "RTR_QUEUE_WORKGROUPS" not in os.environ
    ctx.upload(scenes[name])
    Q.check(Q.CASES[case], Q.run_case(ctx, A, Q.CASES[case]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(Q.ONE_WORKGROUP))
@pytest.mark.parametrize("name", Q.SCENES)
def test_queue_equals_static_grid_in_one_workgroup(one_workgroup, name, case):
    Q.check(Q.ONE_WORKGROUP[case], one_workgroup["%s.%s" % (name, case)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", Q.SCENES)
def test_the_plain_render_is_the_queue_kernel(ctx, scenes, name):
    """what the cases compare: a plain one-shot render of these scenes runs k_mega_queue of the scene's material set"""
    ctx.upload(scenes[name])
    ctx.render(A.make_params(16, 16, 1, integrator=4, seed=1, pipeline=A.PIPELINE_MEGAKERNEL))
    k = ctx.last_kernel()
    assert k["queue"] and k["pair"] and k["accum"] == 0 and k["ms"] == MS_OF[name], k
