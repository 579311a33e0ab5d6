"""The accumulator kernels (csrc/rt_accum_kernels.h: k_accum_errors, k_accum_plan, k_accum_commit, k_accum_resolve,
k_accum_resolve_scatter, k_accum_features_scatter) on the GPU over the synthetic tile state of tests/_accum_ref.py.

The product's own binaries run behind their public entries on state that Accumulator.load_state puts into an accumulator
(rtr_test_accum_load, include/rtr_hip_test.h): sums, moments and counts no render produces, lanes outside the region
poisoned.  k_accum_plan and k_accum_commit also run alone, through rtr_test_accum_plan and rtr_test_accum_commit.  The
image is 80 x 64 with the region (15, 3, 66, 49) -- tiles with one active column, two, one active row, thirteen, and six
whole ones -- once with all 20 tiles owned and once as the shard tile_first = 1, tile_stride = 3.

Every comparison is equality of bits or bytes with the numpy restatements (which tests/test_accum_planes_cpu.py holds to
scalar loops written from the header), NaN means included, with the one stated exception: the BYTE of a mean with
!(mean >= 0) is not defined by the reference's C++ and is compared between the device forms only (at most 16 pixels, all
in one tile)."""
import numpy as np
import pytest
import torch

import _accum_ref as R
import _golden as G

A = G.A
rtr = G.rtr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SHARD_IDS = ["all_tiles", "tiles_1_mod_3"]
HEIGHT, WIDTH = R.REGION[3] - R.REGION[1], R.REGION[2] - R.REGION[0]


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    c.upload(G.scene(21))
    yield c
    c.close()


@pytest.fixture(scope="module")
def ecase():
    return R.errors_case()


@pytest.fixture(scope="module")
def rcase():
    return R.resolve_case()


@pytest.fixture(scope="module")
def fcase():
    return R.refine_case()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _params(shard):
    return A.make_params(R.W, R.H, 1, integrator=4, seed=7, region=R.REGION, tile_first=shard[0], tile_stride=shard[1])


def _owned(acc, shard):
    ids, counts = acc.tiles()
    assert ids.tolist() == R.owned_tiles(R.W, R.H, R.REGION, *shard) and not counts.any()
    return ids.tolist()


def _planes(ids, counts, tiles, fill, flip=False):
    """tile-layout values (n, 256[, C]) as the host forms return them: the region, `fill` where nothing is written"""
    out = np.full((HEIGHT, WIDTH) + tiles.shape[2:], fill, dtype=tiles.dtype)
    return R.tiles_to_region(R.W, R.H, R.REGION, ids, counts, tiles, out, flip=flip)


def _dev(a):
    t = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()  # the library works on a stream of its own
    return t


def _same_bits(dev, host):
    got = dev.cpu().numpy()
    if host.dtype == np.float64:
        return np.array_equal(got.view(np.uint64), host.view(np.uint64))
    return np.array_equal(got, host)


# ---- k_accum_errors behind rtr_accum_errors -------------------------------------------------------------------------


@pytest.mark.parametrize("shard", R.SHARDS, ids=SHARD_IDS)
def test_errors_of_loaded_state(ctx, ecase, shard):
    with ctx.accumulator(_params(shard), moments=True) as acc:
        ids = _owned(acc, shard)
        c = R.select(ecase, ids)
        acc.load_state(c["sum"], c["q"], c["count"])
        assert np.array_equal(acc.tiles()[1], c["count"])
        got = acc.errors()
        want = R.errors(c["sum"], c["q"], c["count"], c["boxes"])
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
        for k, t in enumerate(ids):  # (what the restatement says, said again)
            if c["count"][k] < 2:
                assert got[k] == np.inf
            if t == R.ZERO_TILE:
                assert _bits(got[k]) == _bits(0.0)
        # the planes that went in come out: moments as they are, resolve the restated mean; a tile with count 0 and the
        # pixels no owned tile holds keep the caller's sentinel
        q = acc.moments(np.full((HEIGHT, WIDTH), SENTINEL))
        assert np.array_equal(_bits(q), _bits(_planes(ids, c["count"], c["q"], SENTINEL)))
        mean = R.resolve_linear(c["sum"], c["count"]).transpose(0, 2, 1)
        lin, want_lin = acc.resolve(np.full((HEIGHT, WIDTH, 3), SENTINEL)), _planes(ids, c["count"], mean, SENTINEL)
        assert np.isnan(want_lin).any() and np.array_equal(_bits(lin), _bits(want_lin))  # the NaN sums: their bits too
        kept = R.owner_image(R.W, R.H, R.REGION, [t for k, t in enumerate(ids) if c["count"][k] > 0]) < 0
        assert kept.any() and (q[kept] == SENTINEL).all() and (lin[kept] == SENTINEL).all()


# ---- k_accum_resolve, k_accum_resolve_scatter, the host scatter loops, k_accum_features_scatter ------------------------


def _sentinels(channels=3):
    """(linear or feature plane with row stride WIDTH + 3, bytes), no two neighbours alike"""
    lin = -(1.0 + np.arange(HEIGHT * (WIDTH + 3) * channels, dtype=np.float64)).reshape(HEIGHT, WIDTH + 3, channels)
    rgb = ((np.arange(HEIGHT * WIDTH * 3) * 7 + 3) % 251).astype(np.uint8).reshape(HEIGHT, WIDTH, 3)
    return lin, rgb


@pytest.mark.parametrize("shard", R.SHARDS, ids=SHARD_IDS)
def test_resolve_of_loaded_state(ctx, rcase, shard):
    with ctx.accumulator(_params(shard)) as acc:
        ids = _owned(acc, shard)
        c = R.select(rcase, ids)
        acc.load_state(c["sum"], None, c["count"])
        mean = R.resolve_linear(c["sum"], c["count"])
        byte, defined = R.resolve_rgb8(mean)
        s_lin, s_rgb = _sentinels()
        stride = s_lin.shape[1]
        want_lin = R.tiles_to_region(R.W, R.H, R.REGION, ids, c["count"], mean.transpose(0, 2, 1), s_lin[:, :WIDTH].copy())
        want_rgb = R.tiles_to_region(R.W, R.H, R.REGION, ids, c["count"], byte.transpose(0, 2, 1), s_rgb.copy(), flip=True)
        ok = R.tiles_to_region(R.W, R.H, R.REGION, ids, c["count"], defined.all(axis=1), np.ones((HEIGHT, WIDTH), dtype=bool),
                               flip=True)  # the pixels whose bytes the reference defines, top row first like the bytes
        assert (~ok).sum() == R.RESOLVE_ODD_PIXELS <= 16 and R.RESOLVE_ODD_TILE in ids
        # the host forms against the restatement
        lin = acc.resolve(np.ascontiguousarray(s_lin[:, :WIDTH]))
        rgb = acc.rgb8(s_rgb.copy())
        assert np.isnan(want_lin).sum() == 7 and np.array_equal(_bits(lin), _bits(want_lin))  # NaN and negative means too
        assert np.array_equal(rgb[ok], want_rgb[ok])
        written = R.owner_image(R.W, R.H, R.REGION, [t for k, t in enumerate(ids) if c["count"][k] > 0]) >= 0
        assert (~written).any() and np.array_equal(lin[~written], s_lin[:, :WIDTH][~written])
        assert np.array_equal(rgb[::-1][~written], s_rgb[::-1][~written])  # tiles with count 0 and tiles not owned: untouched
        # the device form against the host form: every byte of both buffers, the stride padding and the odd pixels included
        h_lin, h_rgb = s_lin.copy(), s_rgb.copy()
        ctx._chk(ctx._L.rtr_accum_resolve(ctx._h, acc._h, h_lin.ctypes.data, stride, h_rgb.ctypes.data))
        assert np.array_equal(_bits(h_lin[:, :WIDTH]), _bits(lin)) and np.array_equal(h_rgb, rgb)
        assert np.array_equal(h_lin[:, WIDTH:], s_lin[:, WIDTH:])
        d_lin, d_rgb = _dev(s_lin), _dev(s_rgb)
        acc.resolve_into(d_lin.data_ptr(), stride, d_rgb.data_ptr(), blocking=True)
        assert _same_bits(d_lin, h_lin) and _same_bits(d_rgb, h_rgb)
        d_lin, d_rgb = _dev(s_lin), _dev(s_rgb)  # without the rgb8 pointer
        acc.resolve_into(d_lin.data_ptr(), stride, None, blocking=True)
        assert _same_bits(d_lin, h_lin) and _same_bits(d_rgb, s_rgb)
        d_lin = _dev(s_lin)  # ... and the bytes alone
        acc.resolve_into(None, 0, d_rgb.data_ptr(), blocking=True)
        assert _same_bits(d_lin, s_lin) and _same_bits(d_rgb, h_rgb)
        # k_accum_features_scatter over the ragged boxes: the host form, same stride
        s_feat, _ = _sentinels(A.FEATURES)
        h_feat = s_feat.copy()
        ctx._chk(ctx._L.rtr_accum_features(ctx._h, acc._h, 1, h_feat.ctypes.data, stride))
        assert np.array_equal(_bits(h_feat[:, :WIDTH]), _bits(acc.features(1, np.ascontiguousarray(s_feat[:, :WIDTH]))))
        d_feat = _dev(s_feat)
        acc.features_into(1, d_feat.data_ptr(), stride, blocking=True)
        assert _same_bits(d_feat, h_feat) and not np.array_equal(h_feat, s_feat)
        owned = R.owner_image(R.W, R.H, R.REGION, ids) >= 0
        assert np.array_equal(h_feat[:, :WIDTH][~owned], s_feat[:, :WIDTH][~owned])


# ---- k_accum_errors, k_accum_plan and k_accum_commit inside rtr_accum_refine -------------------------------------------


@pytest.mark.parametrize("run", ["threshold_is_the_error", "threshold_just_below", "spp_min_one"])
@pytest.mark.parametrize("shard", R.SHARDS, ids=SHARD_IDS)
def test_refine_of_loaded_state(ctx, fcase, shard, run):
    with ctx.accumulator(_params(shard), moments=True) as acc:
        ids = _owned(acc, shard)
        c = R.select(fcase, ids)
        count = c["count"]
        err = R.errors(c["sum"], c["q"], count, c["boxes"])
        k = ids.index(R.REFINE_TILE)
        threshold = float(np.nextafter(err[k], 0.0)) if run == "threshold_just_below" else float(err[k])
        spp_min = 1 if run == "spp_min_one" else R.REFINE_MIN
        target, active = R.plan(count, err, count, 2, spp_min=spp_min, spp_max=R.REFINE_MAX, threshold=threshold)
        assert target[k] == (2 * count[k] if run == "threshold_just_below" else count[k])
        acc.load_state(c["sum"], c["q"], count)
        assert np.array_equal(_bits(acc.errors()), _bits(err))
        lin0, q0 = acc.resolve(np.full((HEIGHT, WIDTH, 3), SENTINEL)), acc.moments(np.full((HEIGHT, WIDTH), SENTINEL))
        n_active = acc.refine(threshold, spp_min, R.REFINE_MAX)
        got = acc.tiles()[1]
        assert np.array_equal(got, target), (run, count.tolist(), got.tolist(), n_active)
        assert n_active == len(active) == int((target > count).sum()) > 0
        pixels = R.box_mask(c["boxes"]).sum(axis=1)
        assert ctx.stats()["samples"] == int(((target.astype(np.int64) - count) * pixels).sum())
        lin1, q1 = acc.resolve(np.full((HEIGHT, WIDTH, 3), SENTINEL)), acc.moments(np.full((HEIGHT, WIDTH), SENTINEL))
        idle = np.isin(R.owner_image(R.W, R.H, R.REGION, ids), sorted(set(range(len(ids))) - active))
        assert idle.any() and np.array_equal(_bits(lin1[idle]), _bits(lin0[idle])) and np.array_equal(_bits(q1[idle]), _bits(q0[idle]))
        moved = np.isin(R.owner_image(R.W, R.H, R.REGION, ids), sorted(active))
        assert moved.any() and not np.array_equal(_bits(q1[moved]), _bits(q0[moved]))  # (the pass did render them)


# ---- k_accum_plan alone -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", R.PLAN_SIZES)
def test_plan_alone(ctx, n):
    for name, case in R.plan_cases(n).items():
        target, listed, n_active = ctx.accum_plan(**case)
        want, active = R.plan(**case)
        assert np.array_equal(target, want), name
        assert n_active == len(active), (name, n_active, len(active))
        assert sorted(listed[:n_active].tolist()) == sorted(active), name  # a permutation: no slot twice, none dropped
        assert (listed[n_active:] == -1).all(), name
        b = R.buckets(want, case["count"])[listed[:n_active]]
        assert (b >= 0).all() and (np.diff(b) <= 0).all(), name  # the most pending samples first


# ---- k_accum_commit alone -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("lists", R.COMMIT_LISTS)
@pytest.mark.parametrize("with_q", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("n", R.COMMIT_SIZES)
def test_commit_alone(ctx, n, with_q, lists):
    case = R.commit_case(n, with_q, lists)
    s, q, cnt = ctx.accum_commit(**case)
    want_s, want_q, want_cnt = R.commit(**case)
    assert np.array_equal(_bits(s), _bits(want_s)) and np.array_equal(cnt, want_cnt)
    assert (q is None and want_q is None) if not with_q else np.array_equal(_bits(q), _bits(want_q))
    if lists == "none":  # nothing listed: every byte stays
        assert np.array_equal(_bits(s), _bits(case["sum"])) and np.array_equal(cnt, case["count"])
        assert not with_q or np.array_equal(_bits(q), _bits(case["q"]))


# ---- the entries check their arguments ------------------------------------------------------------------------------


def test_the_entries_check_their_arguments(ctx, fcase):
    def invalid(fn, *args, **kw):
        with pytest.raises(rtr.RtrError) as e:
            fn(*args, **kw)
        assert e.value.code == A.RTR_ERR_INVALID, (args, kw)

    shard = R.SHARDS[1]
    with ctx.accumulator(_params(shard), moments=True) as acc, ctx.accumulator(_params(shard)) as plain:
        c = R.select(fcase, _owned(acc, shard))
        invalid(acc.load_state, c["sum"], None, c["count"])          # moments kept, no q
        invalid(plain.load_state, c["sum"], c["q"], c["count"])      # q without moments
        invalid(acc.load_state, c["sum"][1:], c["q"][1:], c["count"][1:])  # not the number of owned tiles
        invalid(acc.load_state, c["sum"], c["q"], -c["count"])       # a negative count
        assert not acc.tiles()[1].any() and not plain.tiles()[1].any()  # ... before any device work
    case = R.plan_case_mode1(7)
    invalid(ctx.accum_plan, **dict(case, mode=3))
    invalid(ctx.accum_plan, **dict(case, count=case["count"][:0], err=case["err"][:0], tile_s1=case["tile_s1"][:0]))
    case = R.commit_case(7, True, "half")
    invalid(ctx.accum_commit, **dict(case, n_active=8))
    invalid(ctx.accum_commit, **dict(case, n_active=-1))
    invalid(ctx.accum_commit, **dict(case, active=np.where(case["active"] == 3, 7, case["active"])))
    invalid(ctx.accum_commit, **dict(case, active=np.where(case["active"] == 3, -1, case["active"])))
