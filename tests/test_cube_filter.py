"""Filtered cube maps (include/rtr_hip.h: rtr_cube_filter, rtr_cube_chain_lookup and their device-pointer forms) on the
GPU, bit for bit against the numpy restatement of the contract (tests/_cube_filter_ref.py) and the host-only _one forms.
All inputs are synthetic texels but for the stream-order and command-line tests, which filter a capture of scene 21.

csrc/rtr_cube.hip launches k_cube_filter<1> (one output texel per wave) while a launch has fewer than 1024 workgroups of
the wide kernel k_cube_filter<4>, which the 5 -> 53 case reaches; the split test cuts that case so that both run in one
call."""
import os
import subprocess

import numpy as np
import pytest

import _capture_ref as CR
import _cube_filter_ref as FR
import _golden as G
from test_cube_filter_cpu import ALPHAS, CUTS, SHAPES, chain, chain_queries, texels

rtr = G.rtr
A = G.A
N = rtr.native

pytestmark = pytest.mark.gpu
REC = 32
WIDE = (5, 53)  # 16 854 output texels: 1 054 workgroups of the wide kernel, the last one partial


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _sentinel(n_records):
    import torch
    return torch.full(((n_records + 1) * REC,), 0xA5, dtype=torch.uint8, device="cuda")


def _filter_into(ctx, src, fp, n):
    """the device entry's records [n, 6, So, So]; one sentinel record behind them must stay"""
    import torch
    So = fp.face_out
    d_src, d_out = _dev(src), _sentinel(n * 6 * So * So)
    torch.cuda.synchronize()
    ctx.cube_filter_into(d_src.data_ptr(), d_out.data_ptr(), n, fp, blocking=True)
    raw = d_out.cpu().numpy()
    assert (raw[n * 6 * So * So * REC:] == 0xA5).all()  # nothing behind the batch is written
    assert _same_bits(d_src.cpu().numpy(), np.ascontiguousarray(src).reshape(-1).view(np.uint8))  # nor the input
    return raw[:n * 6 * So * So * REC].view(A.GATHER_OUT_DTYPE).reshape(n, 6, So, So)


@pytest.mark.parametrize("cos_cut", CUTS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_filter_entries_equal_the_restatement_and_the_one_form(ctx, shape, alpha, cos_cut):
    S_in, S_out = shape
    src = texels(S_in, n=3)
    fp = N.cube_filter_defaults(face_in=S_in, face_out=S_out, alpha=alpha, cos_cut=cos_cut)
    want = FR.filter_cubes(src, S_out, alpha, cos_cut)
    assert _same_bits(N.cube_filter_host(src, fp), want)
    assert _same_bits(ctx.cube_filter(src, fp), want)
    assert _same_bits(_filter_into(ctx, src, fp, 3), want)


@pytest.mark.parametrize("cos_cut", CUTS)
def test_the_wide_kernel(ctx, cos_cut):
    """5 -> 53, two cubes: enough workgroups for k_cube_filter<4>, with invalid source texels and outputs that use nothing"""
    src = texels(WIDE[0], n=2)
    src["valid"][1, 3, 2, 2] = 0
    src["v"][1, 3, 2, 2] = np.nan
    fp = N.cube_filter_defaults(face_in=WIDE[0], face_out=WIDE[1], alpha=0.0625, cos_cut=cos_cut)
    want = FR.filter_cubes(src, WIDE[1], 0.0625, cos_cut)
    assert (want["valid"][0] == 1).all() and 0 < (want["valid"][1] == 0).sum() < want[1].size
    assert _same_bits(ctx.cube_filter(src, fp), want)
    assert _same_bits(_filter_into(ctx, src, fp, 2), want)
    assert _same_bits(N.cube_filter_host(src[1:, ], fp)[0, 3, :2], want[1, 3, :2])


def test_culled_rows_and_empty_outputs(ctx):
    """1 -> 8 at cos_cut 0.9: corner outputs use nothing (count 0, valid 0); 8 -> 8 at 0.9: most rows of 64 source texels
    are skipped for an output, which changes no bit"""
    for S_in in (1, 8):
        src = texels(S_in, n=1)
        fp = N.cube_filter_defaults(face_in=S_in, face_out=8, alpha=0.5, cos_cut=0.9)
        want = FR.filter_cubes(src, 8, 0.5, 0.9)
        got = ctx.cube_filter(src, fp)
        assert _same_bits(got, want)
        if S_in == 1:
            assert (got["valid"][0, :, 0, 0] == 0).all() and (got["count"][0, :, 0, 0] == 0).all()
            assert (got["valid"][0, :, 3, 3] == 1).all()


def test_launch_split_changes_no_bit(ctx, monkeypatch):
    """RTR_FILTER_PAIRS lowers the pairs per launch.  8 -> 5, three cubes (150 outputs of 384 sources each): 70 outputs per
    launch puts boundaries inside every cube and off a multiple of 64; one cube and a bit per launch mixes whole-cube and
    partial launches; 1 pair: one output texel per launch.  5 -> 53: 16 500 outputs per launch leaves the wide kernel a run
    that ends off a multiple of its 16 texels per workgroup and the narrow kernel the rest of each cube."""
    src = texels(8, n=3)
    fp = N.cube_filter_defaults(face_in=8, face_out=5, alpha=0.0625, cos_cut=0.0)
    monkeypatch.delenv("RTR_FILTER_PAIRS", raising=False)
    whole = ctx.cube_filter(src, fp)
    assert _same_bits(whole, FR.filter_cubes(src, 5, 0.0625, 0.0))
    for pairs in (384 * 70, 384 * 190, 384 * 300, 1):
        monkeypatch.setenv("RTR_FILTER_PAIRS", str(pairs))
        assert _same_bits(ctx.cube_filter(src, fp), whole), pairs
        assert _same_bits(_filter_into(ctx, src, fp, 3), whole), pairs
    monkeypatch.delenv("RTR_FILTER_PAIRS")
    src = texels(WIDE[0], n=2)
    fp = N.cube_filter_defaults(face_in=WIDE[0], face_out=WIDE[1], alpha=0.25, cos_cut=0.0)
    whole = ctx.cube_filter(src, fp)
    monkeypatch.setenv("RTR_FILTER_PAIRS", str(150 * 16500))
    assert _same_bits(_filter_into(ctx, src, fp, 2), whole)
    monkeypatch.setenv("RTR_FILTER_PAIRS", "-5")  # not a cap: ignored
    assert _same_bits(ctx.cube_filter(src, fp), whole)


def test_filter_entries_check_their_arguments(ctx):
    import torch
    src = texels(2, n=2)
    fp = N.cube_filter_defaults(face_in=2, face_out=2, alpha=0.5)
    out = np.zeros(48, dtype=A.GATHER_OUT_DTYPE)
    d_buf = _sentinel(4 * 24)
    torch.cuda.synchronize()
    p = d_buf.data_ptr()
    L, h = ctx._L, ctx._h
    import ctypes as C
    inv = A.RTR_ERR_INVALID
    s, o = src.ctypes.data, out.ctypes.data
    assert L.rtr_cube_filter(h, C.byref(fp), None, None, 0) == A.RTR_OK  # n == 0: nothing read, no launch
    assert L.rtr_cube_filter_device(h, C.byref(fp), None, None, 0, 1) == A.RTR_OK
    for args in ((None, s, o, 2), (C.byref(fp), None, o, 2), (C.byref(fp), s, None, 2), (C.byref(fp), s, o, -1),
                 (C.byref(N.cube_filter_defaults(face_in=2, face_out=2, alpha=2.0)), s, o, 2),
                 (C.byref(N.cube_filter_defaults(face_in=2, face_out=2, cos_cut=-0.0)), s, o, 2),
                 (C.byref(N.cube_filter_defaults(face_in=513, face_out=2)), s, o, 2)):
        assert L.rtr_cube_filter(h, *args) == inv
        assert L.rtr_cube_filter_device(h, *args, 1) == inv
    assert not out.view(np.uint8).any()
    two = 2 * 24 * REC  # bytes of the two cubes
    # misaligned or overlapping device pointers: RTR_ERR_INVALID before any launch
    for t_ptr, o_ptr in ((p + 4, p + two), (p, p + two + 4), (p, p), (p, p + two - REC), (p + two - REC, p), (p + REC, p)):
        with pytest.raises(rtr.RtrError) as e:
            ctx.cube_filter_into(t_ptr, o_ptr, 2, fp, blocking=True)
        assert e.value.code == inv and ("aligned" in e.value.message or "overlap" in e.value.message)
    ctx.synchronize()
    assert (d_buf.cpu().numpy() == 0xA5).all()  # nothing ran
    ctx.cube_filter_into(p, p + two, 2, fp, blocking=True)  # side by side is fine (the input is sentinel bytes: valid != 0)
    assert (d_buf.cpu().numpy()[:two] == 0xA5).all() and (d_buf.cpu().numpy()[2 * two:] == 0xA5).all()


# ---- chain lookup ----

@pytest.mark.parametrize("n_levels", (1, 4))
@pytest.mark.parametrize("S", (1, 2, 8))
def test_chain_lookup_entries_equal_the_one_form(ctx, S, n_levels):
    import torch
    levels, rec = chain(S, n_levels)
    q = chain_queries(levels, S)
    want = N.cube_chain_lookup_host(levels, rec, q)
    assert _same_bits(want, FR.chain_lookup(levels, rec, q))
    assert _same_bits(ctx.cube_chain_lookup(levels, rec, q), want)
    d_rec, d_q, d_out = _dev(rec), _dev(q), _sentinel(len(q))
    torch.cuda.synchronize()
    ctx.cube_chain_lookup_into(levels, d_rec.data_ptr(), len(rec), d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=True)
    raw = d_out.cpu().numpy()
    assert _same_bits(raw[:len(q) * REC].view(A.GATHER_OUT_DTYPE), want)
    assert (raw[len(q) * REC:] == 0xA5).all()


def test_chain_lookup_across_a_slice(ctx):
    """The host entry sends its queries in slices of 2^20: a batch of 2^20 + 37, the CPU test's queries over and over, has
    the boundary inside it; every query's answer is that of its first copy"""
    levels, rec = chain(8, 4)
    q = chain_queries(levels, 8)
    want = N.cube_chain_lookup_host(levels, rec, q)
    n = (1 << 20) + 37
    idx = np.arange(n) % len(q)
    assert idx[(1 << 20) - 1] != len(q) - 1  # the boundary is inside a copy
    got = ctx.cube_chain_lookup(levels, rec, q[idx])
    assert _same_bits(got, want[idx])


def test_chain_entries_check_their_arguments(ctx):
    import ctypes as C
    levels, rec = chain(2, 2)
    q = N.cube_queries(np.ones((2, 3)), 0.5)
    out = np.zeros(2, dtype=A.GATHER_OUT_DTYPE)
    L, h, inv = ctx._L, ctx._h, A.RTR_ERR_INVALID
    lv = N.cube_levels(levels)
    r, qq, o = rec.ctypes.data, q.ctypes.data, out.ctypes.data
    assert L.rtr_cube_chain_lookup(h, C.byref(lv), 2, None, len(rec), None, None, 0) == A.RTR_OK
    bad_alpha = N.cube_levels([(2, 0, 0.5), (1, 24, 0.5)])
    for args in ((None, 2, r, len(rec), qq, o, 2), (C.byref(lv), 0, r, len(rec), qq, o, 2), (C.byref(lv), 14, r, len(rec), qq, o, 2),
                 (C.byref(lv), 2, None, len(rec), qq, o, 2), (C.byref(lv), 2, r, len(rec), None, o, 2),
                 (C.byref(lv), 2, r, len(rec), qq, None, 2), (C.byref(lv), 2, r, len(rec), qq, o, -1),
                 (C.byref(lv), 2, r, len(rec) - 1, qq, o, 2), (C.byref(lv), 2, r, -1, qq, o, 2),  # a level outside n_records
                 (C.byref(bad_alpha), 2, r, len(rec), qq, o, 2)):
        assert L.rtr_cube_chain_lookup(h, *args) == inv
        assert L.rtr_cube_chain_lookup_device(h, *args, 1) == inv
    assert L.rtr_cube_chain_lookup_device(h, C.byref(lv), 2, r + 4, len(rec), qq, o, 2, 1) == inv  # misaligned, before any launch
    assert not out.view(np.uint8).any()


# ---- behind a capture, and the other faces ----

CENTRE = (278.0, 400.0, 400.0)  # above the two boxes of the Cornell box of scene 21


def test_capture_filters_and_lookup_in_stream_order(ctx):
    """capture_cube_into (S = 8, 2 samples), three cube_filter_into levels and cube_chain_lookup_into queued back to back
    without a wait between them, one synchronise at the end"""
    import torch
    ctx.upload(G.scene(21))
    prm = A.make_params(64, 64, 1, integrator=4)
    levels, n_records = FR.plan(8, 4)
    q = chain_queries(levels, 8)
    d_pts = _dev(N.probe_points(np.array([CENTRE])))
    d_chain, d_q, d_out = _sentinel(n_records), _dev(q), _sentinel(len(q))
    torch.cuda.synchronize()
    base = d_chain.data_ptr()
    ctx.capture_cube_into(prm, d_pts.data_ptr(), base, 1, face_size=8, samples=2, seed=7, blocking=False)
    for S, at, alpha in levels[1:]:
        ctx.cube_filter_into(base, base + at * REC, 1, face_in=8, face_out=S, alpha=alpha, blocking=False)
    ctx.cube_chain_lookup_into(levels, base, n_records, d_q.data_ptr(), d_out.data_ptr(), len(q), blocking=False)
    ctx.synchronize()
    raw = d_chain.cpu().numpy()
    rec = raw[:n_records * REC].view(A.GATHER_OUT_DTYPE)
    assert (raw[n_records * REC:] == 0xA5).all()
    capture = ctx.capture_cube_records(prm, np.array([CENTRE]), face_size=8, samples=2, seed=7)[0]
    assert _same_bits(rec[:384].reshape(6, 8, 8), capture) and (capture["valid"] == 1).all() and (capture["v"] > 0).any()
    for S, at, alpha in levels[1:]:
        assert _same_bits(rec[at:at + 6 * S * S].reshape(6, S, S), FR.filter_cube(capture, S, alpha, 0.0)), S
    got = d_out.cpu().numpy()[:len(q) * REC].view(A.GATHER_OUT_DTYPE)
    assert _same_bits(got, N.cube_chain_lookup_host(levels, rec, q))


def test_python_faces_on_a_context(ctx):
    src = texels(8)[0]
    cube = rtr.Cubemap(src)
    on_host, on_dev = cube.prefilter(levels=4), cube.prefilter(levels=4, ctx=ctx)
    assert _same_bits(on_host.records, on_dev.records)
    d = FR.centres(3)[0]
    rough = np.linspace(0.0, 1.0, len(d))
    assert _same_bits(on_dev.lookup_records(d, rough, ctx=ctx), on_host.lookup_records(d, rough))
    assert _same_bits(on_dev.lookup(d, 0.3, ctx=ctx), on_host.lookup(d, 0.3))


def test_the_command_line_writes_the_chain(ctx, tmp_path):
    """rtr_cli --capture ... --capture-levels 3 (Renderer::prefilter_cube) writes three .hdr files whose texels are
    rtr_cube_to_latlong of the levels of the Python chain of the same capture, through the RGBE bytes"""
    cli = os.path.join(os.path.dirname(N.library_path()), "rtr_cli")
    out = str(tmp_path / "cli.hdr")
    r = subprocess.run([cli, "21", "4", "--capture", "%g,%g,%g" % CENTRE, "--face", "8", "--capture-spp", "2", "--seed", "7",
                        "--capture-levels", "3", "--capture-out", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    sc = rtr.hostscene.build_scene(21)
    ren = rtr.Renderer(context=ctx)
    ren.seed = 7
    ch = ren.capture_environment(sc, CENTRE, face_size=8, samples=2).prefilter(levels=3, ctx=ctx)
    assert [lv.face_size for lv in ch.levels] == [8, 4, 2]
    mine = ch.save_hdr(str(tmp_path / "py"), 32, 16)
    for i, path in enumerate((out, str(tmp_path / "cli.L1.hdr"), str(tmp_path / "cli.L2.hdr"))):
        data = open(path, "rb").read()
        assert data == open(mine[i], "rb").read(), i
        latlong = N.cube_to_latlong(ch.level(i).texels, 32, 16)
        assert np.array_equal(CR.rgbe_decode(data), CR.rgbe_decode(CR.rgbe_bytes(latlong))), i
        assert CR.rgbe_decode(data).max() > 0
    assert not os.path.exists(str(tmp_path / "cli.L3.hdr"))
    for args in (["--capture-levels", "3"], ["--capture", "1,2,3", "--capture-out", out, "--capture-levels", "0"],
                 ["--capture", "1,2,3", "--capture-out", out, "--capture-levels", "14"],
                 ["--capture", "1,2,3", "--capture-out", out, "--capture-levels", "2", "--face", "513"]):
        r = subprocess.run([cli, "21", "4"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2, args
