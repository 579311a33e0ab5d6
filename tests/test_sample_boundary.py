"""The sample boundary of the lockstep megakernel loops (csrc/rt_kernels.h: k_mega's PAIR branch and the split-cast
loop): the wave-uniform cancel poll, the parked pixel word behind begin_sample, the integer cast counters and the
settling of an ended sample.  None of it may change a bit of an image or a count: everything here is pinned to the
reference's goldens, to the CPU oracle and to the split casts, at the sample counts around the poll interval and the
chunk edges, and a cancel still leaves every tile finished or untouched."""
import threading

import numpy as np
import pytest

import _golden as G

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

REL_L2_BAR = 1e-3  # BASELINE.json north_star tolerance (scene 23 calls libm: tests/test_gpu_parity.py)
STEP_LIMIT = 60.0  # seconds a cancelled render may take before the test gives up on it


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _counts(st):
    return st["samples"], st["closest_segments"], st["shadow_segments"]


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_oracle():
    """scene 21 at 40x24 (partial tiles, inactive lanes) from the oracle, once per spp"""
    sc = G.scene(21)
    out = {}
    for spp in (1, 7, 8, 9, 17):
        p = A.make_params(40, 24, spp, integrator=4, seed=11, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
        out[spp] = G.oracle_render(sc, p, threads=0)
    return out


def test_golden_image_and_counts(ctx):
    """scene 21, MIS, pair cast, 64x64 spp 16: the reference's image bit for bit, the reference's and the oracle's
    segment counts (209 392 closest segments; a wave-scalar counter once gave 165 153)"""
    img, info = G.image("img_scene21_i4_64_spp16.f64")
    sc = G.scene(21)
    ctx.upload(sc)
    p = A.make_params(info["width"], info["height"], info["spp"], integrator=4, seed=info["seed"],
                      pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    out = ctx.render(p)
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    assert np.array_equal(_bits(out), _bits(img))
    ora, ost = G.oracle_render(sc, p, threads=0)
    assert np.array_equal(_bits(out), _bits(ora))
    print("closest %d shadow %d (oracle %d %d)" % (st["closest_segments"], st["shadow_segments"],
                                                    ost["closest_segments"], ost["shadow_segments"]))
    assert info["info"]["closest_segments"] == 209392
    assert st["closest_segments"] == info["info"]["closest_segments"] == ost["closest_segments"]
    assert st["shadow_segments"] == info["info"]["shadow_segments"] == ost["shadow_segments"]
    assert st["samples"] == info["width"] * info["height"] * info["spp"]


@pytest.mark.parametrize("spp", [1, 7, 8, 9, 17])
def test_sample_counts_around_poll_and_chunk_edges(ctx, small_oracle, spp):
    """40x24, spp around the poll interval, spp_chunks 1 / guided / 3, pair and split casts: spp_chunks = 1 is the
    oracle bit for bit with its counts; pair equals split for every chunking (chunked sums are the library's own); three
    chunks of one sample is RTR_ERR_INVALID for both"""
    ctx.upload(G.scene(21))
    ora, ost = small_oracle[spp]
    for chunks in (1, 0, 3):
        got = {}
        for flags in (0, A.FLAG_SPLIT_CASTS):
            p = A.make_params(40, 24, spp, integrator=4, seed=11, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=chunks,
                              flags=flags)
            if chunks > spp:  # more partial sums than samples: the library refuses the call, whichever kernel it names
                with pytest.raises(rtr.RtrError) as e:
                    ctx.render(p)
                assert e.value.code == A.RTR_ERR_INVALID
                continue
            out = ctx.render(p)
            st = ctx.stats()
            assert bool(st["flags_in_effect"] & A.FLAG_SPLIT_CASTS) == bool(flags)
            assert not st["cancelled"]
            got[flags] = (out, _counts(st))
            assert _counts(st) == _counts(ost), (chunks, flags)
            if chunks == 1:
                assert np.array_equal(_bits(out), _bits(ora)), (chunks, flags)
        if not got:
            continue
        assert np.array_equal(_bits(got[0][0]), _bits(got[A.FLAG_SPLIT_CASTS][0])), chunks
        assert got[0][1] == got[A.FLAG_SPLIT_CASTS][1], chunks


@pytest.mark.parametrize("flags", [0, A.FLAG_SPLIT_CASTS])
def test_accumulator_twins_continue_bit_exactly(ctx, flags):
    """ACC = 1 and 2: passes of 4 + 5 samples on a 32x32 accumulator are one 9-spp render, second moments included"""
    ctx.upload(G.scene(21))
    kw = dict(integrator=4, seed=5, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)
    ref = ctx.render(A.make_params(32, 32, 9, **kw))
    with ctx.accumulator(A.make_params(32, 32, 9, **kw), moments=True) as one:
        one.render(9)
        q_ref = one.moments()
        assert np.array_equal(_bits(one.resolve()), _bits(ref))
    for moments in (False, True):
        with ctx.accumulator(A.make_params(32, 32, 9, **kw), moments=moments) as acc:
            acc.render(4)
            acc.render(9)
            assert np.array_equal(_bits(acc.resolve()), _bits(ref)), moments
            if moments:
                assert np.array_equal(_bits(acc.moments()), _bits(q_ref))


def test_quadlit_pair_variant_scene23(ctx):
    """scene 23 (spheres, every material: the QuadLights-only pair kernel), 32x32 spp 4: the split casts bit for bit
    with their counts, and the oracle within the bar its libm calls need"""
    sc = G.scene(23)
    ctx.upload(sc)
    kw = dict(integrator=4, seed=7, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1)
    p = A.make_params(32, 32, 4, **kw)
    out = ctx.render(p)
    st = ctx.stats()
    assert st["flags_in_effect"] & A.FLAG_SPLIT_CASTS == 0
    split = ctx.render(A.make_params(32, 32, 4, flags=A.FLAG_SPLIT_CASTS, **kw))
    ss = ctx.stats()
    assert ss["flags_in_effect"] & A.FLAG_SPLIT_CASTS
    assert np.array_equal(_bits(out), _bits(split))
    assert _counts(st) == _counts(ss)
    ora, ost = G.oracle_render(sc, p, threads=0)
    assert G.rel_l2(out, ora) <= REL_L2_BAR
    assert st["samples"] == ost["samples"] == 32 * 32 * 4


def _tiles(a, n):
    return a.reshape(n // 16, 16, n // 16, 16, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 16 * 16 * 3)


def _bounded(fn):
    """run one step that must not hang on a lost cancel"""
    res = {}

    def run():
        try:
            res["value"] = fn()
        except BaseException as e:  # noqa: BLE001 -- handed to the test thread
            res["error"] = e

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(STEP_LIMIT)
    assert not th.is_alive(), "the step did not end within %g s" % STEP_LIMIT
    if "error" in res:
        raise res["error"]
    return res["value"]


@pytest.mark.parametrize("flags", [0, A.FLAG_SPLIT_CASTS])
def test_cancel_leaves_tiles_finished_or_untouched(ctx, flags):
    """256x256 spp 64: a render cancelled while it still waits behind another one, and one cancelled right after its
    launch.  Complete tiles are the uncancelled render's, incomplete ones keep the caller's values, and the
    interrupted-workgroup word (stats: cancelled) says whether any tile was left out."""
    import torch
    S = 256
    ctx.upload(G.scene(21))
    p = A.make_params(S, S, 64, integrator=4, seed=1, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)
    big = A.make_params(1024, 1024, 64, integrator=4, seed=1, pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, flags=flags)

    def whole():  # through the same entry point as the cancelled renders: the same layout
        buf = torch.full((S, S, 3), -7.0, dtype=torch.float64, device="cuda")
        ctx.render_into(p, buf.data_ptr(), S, blocking=True)
        return buf.cpu().numpy()

    full = _bounded(whole)
    assert not ctx.stats()["cancelled"] and full.min() >= 0.0
    total = S * S * 64

    def check(fb, st, must_cancel):
        got = _tiles(fb.cpu().numpy(), S)
        want = _tiles(full, S)
        untouched = np.all(got == -7.0, axis=1)
        finished = np.all(_bits(got) == _bits(want), axis=1)
        print("flags %d: %d of %d tiles untouched, %d samples" % (flags, untouched.sum(), untouched.size, st["samples"]))
        assert np.all(untouched | finished), "%d tiles hold partial sums" % (~(untouched | finished)).sum()
        assert bool(st["cancelled"]) == bool(untouched.any())
        if st["cancelled"]:
            assert st["samples"] < total
        else:
            assert st["samples"] == total
        if must_cancel:
            assert untouched.all() and st["cancelled"]

    # cancelled before its launch: queued behind a longer render when the cancel is issued
    scratch = torch.empty((1024, 1024, 3), dtype=torch.float64, device="cuda")
    fb = torch.full((S, S, 3), -7.0, dtype=torch.float64, device="cuda")

    def queued():
        ctx.render_into(big, scratch.data_ptr(), 1024, blocking=False)
        ctx.render_into(p, fb.data_ptr(), S, blocking=False)
        ctx.cancel()
        return ctx.stats()  # of the second render

    check(fb, _bounded(queued), must_cancel=True)

    # cancelled right after its launch: wherever the flag lands, the outcome is one of the allowed ones
    fb = torch.full((S, S, 3), -7.0, dtype=torch.float64, device="cuda")

    def running():
        ctx.render_into(p, fb.data_ptr(), S, blocking=False)
        ctx.cancel()
        return ctx.stats()

    check(fb, _bounded(running), must_cancel=False)

    # the context stays usable and the cancel does not leak into the next render
    again = _bounded(whole)
    assert not ctx.stats()["cancelled"]
    assert np.array_equal(_bits(again), _bits(full))
