"""The a-trous filter (rtr_denoise_host: k_denoise_prep, k_denoise_pass, k_denoise_pass_lds<1|2>, k_denoise_out) on the
GPU over the synthetic planes of tests/_planes.py: per-pixel holes in every arrangement, regions from 1 x 1 up, steps
larger than the image, counts, albedos and depths at the edges of every compare -- each held to the numpy restatement of
tests/_denoise_ref.py bit for bit (which tests/test_denoise_cpu.py holds to a scalar reference written from the header),
in both forms of steps 1 and 2: from LDS (the default) and from global memory (RTR_DENOISE_LDS=0)."""
import functools

import numpy as np
import pytest

import _denoise_ref as D
import _golden as G
import _planes as P

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SENTINEL, SENTINEL8 = -7.0, 0xA5
FORMS = ["lds", "global"]


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)  # no scene: rtr_denoise_host needs none
    yield c
    c.close()


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    """steps 1 and 2 through k_denoise_pass_lds (the default) or through k_denoise_pass; the library reads the variable
    on every call"""
    if request.param == "global":
        monkeypatch.setenv("RTR_DENOISE_LDS", "0")
    else:
        monkeypatch.delenv("RTR_DENOISE_LDS", raising=False)
    return request.param


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _prm(iterations=None, **sigmas):
    return rtr.native.denoise_defaults(**(sigmas if iterations is None else dict(sigmas, iterations=iterations)))


@functools.lru_cache(maxsize=None)
def _case(h, w, seed, pattern=None, iterations=None, sigma=None):
    """(planes, params, the restatement's output): computed once, shared by both forms, never written to"""
    planes = P.planes(h, w, seed, valid=None if pattern is None else P.patterns(h, w)[pattern])
    prm = _prm(iterations, **dict([sigma] if sigma else []))
    want = D.denoise(*planes, **D.denoise_params(prm))
    for x in planes + (want,):
        x.flags.writeable = False
    return planes, prm, want


def _check(ctx, planes, prm, want):
    """linear and 8-bit output of the device against ``want`` on every valid pixel; the caller's values elsewhere"""
    color, q, count, feat = planes
    h, w = count.shape
    v = count > 0
    assert np.isfinite(want[v]).all()
    got = rtr.native.denoise_host(ctx, color, q, count, feat, prm, out=np.full((h, w, 3), SENTINEL))
    assert np.array_equal(_bits(got[v]), _bits(want[v]))
    assert (got[~v] == SENTINEL).all()
    rgb = rtr.native.denoise_host(ctx, color, q, count, feat, prm, rgb8=True, out=np.full((h, w, 3), SENTINEL8, dtype=np.uint8))
    top = v[::-1]  # the 8-bit store has the top row first
    assert np.array_equal(rgb[top], D.rgb8(want)[top])
    assert (rgb[~top] == SENTINEL8).all()
    return got


@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 5, 10])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1), (2, 2), (5, 3), (15, 15), (16, 16), (17, 17), (16, 33), (33, 47)])
def test_shapes_and_iterations(ctx, form, h, w, iterations):
    """one pixel, one row, one column, sides around the 16-pixel workgroup, more than one workgroup each way; steps up
    to 512, far larger than the plane (only the centre tap is left, the LDS halo lies wholly outside the image)"""
    planes, prm, want = _case(h, w, 100 + 64 * h + w, iterations=iterations)
    if h > 1:  # a missing row flip of the 8-bit store would show: the rows differ
        assert not np.array_equal(D.rgb8(want), D.rgb8(want)[::-1])
    got = _check(ctx, planes, prm, want)
    if iterations == 0:
        v = planes[2] > 0
        assert np.array_equal(_bits(got[v]), _bits(planes[0][v]))


@pytest.mark.parametrize("iterations", [1, 2, None])
@pytest.mark.parametrize("pattern", ["checkerboard", "lone_valid", "lone_hole", "seam_15", "seam_16", "seam_17", "frame"])
def test_hole_patterns(ctx, form, pattern, iterations):
    """isolated holes and isolated valid pixels, holes along the workgroup seams: the per-pixel validity of the LDS halo
    and the n == 0 skips of the prefilter and of the taps; a hole is NaN in every plane, so reading one shows"""
    _check(ctx, *_case(40, 36, 7, pattern=pattern, iterations=iterations))


def test_translation_invariance(ctx, form):
    """a 13 x 20 patch at six places of a 64 x 48 field of NaN-filled holes: the same bits wherever it lies among the
    workgroups, and those of the patch alone"""
    patch, prm, want = _case(13, 20, 5)
    alone = rtr.native.denoise_host(ctx, *patch, prm, out=np.full((13, 20, 3), SENTINEL))
    v = patch[2] > 0
    assert np.array_equal(_bits(alone[v]), _bits(want[v]))
    for ox, oy in [(0, 0), (1, 0), (15, 15), (16, 16), (13, 29), (64 - 20, 48 - 13)]:
        field = [np.full((48, 64) + x.shape[2:], 0 if x.dtype == np.int32 else np.nan, dtype=x.dtype) for x in patch]
        for big, small in zip(field, patch):
            big[oy:oy + 13, ox:ox + 20] = small
        got = rtr.native.denoise_host(ctx, *field, prm, out=np.full((48, 64, 3), SENTINEL))
        assert np.array_equal(_bits(got[oy:oy + 13, ox:ox + 20]), _bits(alone)), (ox, oy)
        got[oy:oy + 13, ox:ox + 20] = SENTINEL
        assert (got == SENTINEL).all()


@pytest.mark.parametrize("iterations", [1, 2, 4, 10])
def test_partition_of_unity(ctx, form, iterations):
    """albedo 1 and one colour k on every valid pixel, everything else random: the weights of a pixel sum to one, so the
    output is k up to rounding -- per pass at most 25 rounded products and sums, one division and the remodulation:
    27 * 2^-53 relative per pass"""
    k = 0.7
    color, q, count, feat = (x.copy() for x in P.planes(33, 47, 11))
    v = count > 0
    color[v] = k
    feat[..., 0:3][v] = 1.0
    got = rtr.native.denoise_host(ctx, color, q, count, feat, _prm(iterations), out=np.full((33, 47, 3), SENTINEL))
    err = np.abs(got[v] - k).max() / k
    print("partition of unity, %d iterations: largest relative error %.3g (bound %.3g)" % (iterations, err, iterations * 27 * 2.0 ** -53))
    assert err <= iterations * 27 * 2.0 ** -53
    assert (got[~v] == SENTINEL).all()


@pytest.mark.parametrize("iterations", [1, 2, None])
def test_non_finite_samples(ctx, form, iterations):
    """One valid pixel with a NaN colour channel, one with +inf, in an otherwise finite 24 x 24 plane.  A pixel that taps
    a NaN sample gets a NaN luminance weight and is NaN in every channel; one that taps an inf sample gives it the weight
    0, and 0 * inf = NaN enters the sum of that channel, so a pass later its own luminance is NaN too.  A pass reaches 2 *
    step pixels per axis: after pass k nothing farther than 2 * (2^(k+1) - 1) pixels (2, 6, 14, 30) from a bad sample
    is touched, and at the default four iterations that is the whole plane.  The device's set of non-finite values must be
    the restatement's (NaN and inf masks, not payloads), every other valid value its bits."""
    color, q, count, feat = (x.copy() for x in P.planes(24, 24, 13))
    v = count > 0
    ys, xs = np.nonzero(v)
    (y0, x0), (y1, x1) = (ys[5], xs[5]), (ys[-5], xs[-5])
    color[y0, x0, 1] = np.nan
    color[y1, x1, 0] = np.inf
    prm = _prm(iterations)
    want = D.denoise(color, q, count, feat, **D.denoise_params(prm))
    got = rtr.native.denoise_host(ctx, color, q, count, feat, prm, out=np.full((24, 24, 3), SENTINEL))
    assert np.array_equal(np.isnan(got[v]), np.isnan(want[v])) and np.array_equal(np.isinf(got[v]), np.isinf(want[v]))
    fin = v[..., None] & np.isfinite(want)
    assert np.array_equal(_bits(got[fin]), _bits(want[fin]))
    assert (got[~v] == SENTINEL).all()
    reach = 2 * (2 ** (prm.iterations + 1) - 1)
    yy, xx = np.mgrid[0:24, 0:24]
    near = (np.maximum(abs(yy - y0), abs(xx - x0)) <= reach) | (np.maximum(abs(yy - y1), abs(xx - x1)) <= reach)
    assert np.isfinite(want[v & ~near]).all() and not np.isfinite(want[y0, x0]).any() and not np.isfinite(want[y1, x1]).any()
    assert (v & ~near).any() == (prm.iterations < 3) and (~np.isfinite(want[v])).sum() > 20


@pytest.mark.parametrize("value", [1e-6, 1e6])
@pytest.mark.parametrize("sigma", ["sigma_l", "sigma_n", "sigma_a", "sigma_z"])
def test_sigma_extremes(ctx, form, sigma, value):
    _check(ctx, *_case(17, 17, 4, sigma=(sigma, value)))
