"""The temporal kernels (k_temporal_blend, k_temporal_store) on the GPU over the synthetic cases of tests/_planes.py,
through the unit entry rtr_test_temporal_planes (include/rtr_hip_test.h): regions from 1 x 1 up inside a 64 x 48 image
and flush with its corner, camera moves that put positions on pixel centres, between pixels, behind the last camera and
10^18 pixels outside its image, hand-made histories, and tap depths, normals and weights at the very edge of each
compare.  c', var' and the history written are held to the numpy restatement of tests/_temporal_ref.py bit for bit
(which tests/test_temporal_cpu.py holds to a scalar reference written from the header), for the frame of the case and for
a second frame on the history the device wrote."""
import numpy as np
import pytest

import _denoise_ref as D
import _golden as G
import _planes as P
import _temporal_ref as T

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)  # no scene: the entry needs none
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device(ctx, case, **replace):
    k = dict(case, **replace)
    h, w = k["count"].shape
    tp = rtr.native.temporal_defaults(**{name: k[name] for name in ("alpha_min", "tau_z", "tau_n", "min_weight")})
    return ctx.temporal_planes(k["color"], k["q"], k["count"], k["feat"], k["hist"], k["have"], k["cam"], k["prev"],
                               (k["W"], k["H"]), (k["x0"], k["y0"]), tp, c=np.full((h, w, 3), SENTINEL),
                               var=np.full((h, w), SENTINEL))


def _restatement(case, **replace):
    args, tp = P.blend_args(dict(case, **replace))
    return T.blend(*args, **tp)


def _same(got, want, valid):
    """(c', var', history) of the device against the restatement's: every bit of every valid pixel, the caller's values
    and an all-zero history elsewhere"""
    c, var, new = got
    assert np.array_equal(_bits(c[valid]), _bits(want[0][valid])) and np.array_equal(_bits(var[valid]), _bits(want[1][valid]))
    assert (c[~valid] == SENTINEL).all() and (var[~valid] == SENTINEL).all()
    assert np.array_equal(_bits(new), _bits(want[6])) and (new[~valid] == 0.0).all()


@pytest.mark.parametrize("name", P.TEMPORAL_CASES)
def test_frame_and_the_frame_after_it(ctx, name):
    case = P.temporal_case(name)
    valid = case["count"] > 0
    got = _device(ctx, case)
    _same(got, _restatement(case), valid)
    # a second frame under a static camera, on the history the device wrote
    again = dict(hist=got[2], prev=case["cam"])
    _same(_device(ctx, case, **again), _restatement(case, **again), valid)


@pytest.mark.parametrize("region", list(P.temporal_regions()))
def test_cleared_history_is_the_prep_of_the_filter(ctx, region):
    """have = 0: c' and var' are what k_denoise_prep computes, the history holds the current values; what the history
    buffer holds is not read (NaN there would show)"""
    case = P.temporal_case("half_pixel-" + region)
    valid = case["count"] > 0
    got = _device(ctx, case, have=False, hist=np.full(case["hist"].shape, np.nan))
    _same(got, _restatement(case, have=False), valid)
    c, var, a, nn, z, _ = D.prepare(case["color"], case["q"], case["count"], case["feat"])
    assert np.array_equal(_bits(got[0][valid]), _bits(c[valid])) and np.array_equal(_bits(got[1][valid]), _bits(var[valid]))
    new = got[2][valid]
    assert np.array_equal(_bits(new[:, 0:3]), _bits(c[valid])) and np.array_equal(new[:, 5], case["count"][valid].astype(np.float64))
    assert np.array_equal(_bits(new[:, 3]), _bits(D.lum(case["color"])[valid]))
    assert np.array_equal(_bits(new[:, 4]), _bits(((1.0 / case["count"][valid]) * case["q"][valid])))
    assert np.array_equal(_bits(new[:, 6]), _bits(z[valid])) and np.array_equal(_bits(new[:, 7:10]), _bits(nn[valid]))


@pytest.mark.parametrize("region", ["17x16_inside", "whole"])
def test_alpha_min_one_is_the_cleared_history_frame(ctx, region):
    """with a finite history and alpha_min = 1 the blend keeps nothing of it: the bits of the have = 0 call"""
    case = P.temporal_case("alpha_one-" + region)
    assert np.isfinite(case["hist"]).all() and case["alpha_min"] == 1.0
    with_history, cleared = _device(ctx, case), _device(ctx, case, have=False)
    for x, y in zip(with_history, cleared):
        assert np.array_equal(_bits(x), _bits(y))
    assert _restatement(case)[7]["has_history"].sum() > 100


def test_the_entry_checks_its_arguments(ctx):
    case = P.temporal_case("static-17x16_inside")
    for bad in (dict(x0=64 - 15), dict(y0=48 - 16), dict(x0=-1), dict(W=1), dict(alpha_min=0.0), dict(min_weight=1.0),
                dict(tau_z=0.0), dict(tau_n=float("nan")), dict(count=-case["count"])):
        with pytest.raises(rtr.RtrError) as e:
            _device(ctx, case, **bad)
        assert e.value.code == A.RTR_ERR_INVALID, bad
