"""Probe distance maps (include/rtr_hip.h: rtr_probe_depth*, rtr_octa_*, rtr_probe_lookup_visible*) without a GPU: the
declarations and layouts, the host-only rtr_octa_decode, rtr_octa_encode, rtr_probe_depth_ray and
rtr_probe_lookup_visible_one against the restatement of the contract (tests/_probe_depth_ref.py) bit for bit, the folds of
the fetch at every edge and corner of the map, every branch of the visibility weight, every parameter rejection, and a
synthetic wall between two probes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _golden as G
import _probe_depth_ref as DR
import _probe_ref as PR
import test_probes_cpu as TP

A = G.A
rtr = G.rtr
N = rtr.native

NAMES = ("rtr_probe_depth_defaults", "rtr_probe_depth", "rtr_probe_depth_device", "rtr_probe_depth_ray", "rtr_octa_encode",
         "rtr_octa_decode", "rtr_probe_lookup_visible", "rtr_probe_lookup_visible_device", "rtr_probe_lookup_visible_one")


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_declared_exported_and_the_abi_version_stays():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", text))
    lib = N.lib()
    for name in NAMES:
        assert name in declared and name in N.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("rtr_probe_depth_texel", "rtr_probe_depth_params", "rtr_probe_visible_params"):
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    assert "rtr_test_last_probe_depth" in N.TEST_EXPORTS
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+4\b", _header())
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4


def test_struct_sizes_and_defaults(tmp_path):
    """32 / 48 / 32 bytes as a C compiler lays the header out, and the mirrors have the same fields at the same offsets"""
    import subprocess
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtr_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rtr_probe_depth_texel), sizeof(rtr_probe_depth_params),\n'
                   'sizeof(rtr_probe_visible_params), offsetof(rtr_probe_depth_texel, hits), offsetof(rtr_probe_depth_params, time),\n'
                   'offsetof(rtr_probe_depth_params, t_max), offsetof(rtr_probe_visible_params, normal_bias));\nreturn 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I" + os.path.join(G.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True).stdout.split()]
    assert got == [32, 48, 32, 16, 24, 40, 8]
    assert A.PROBE_DEPTH_DTYPE.itemsize == 32 and A.PROBE_DEPTH_DTYPE.fields["hits"][1] == 16
    assert C.sizeof(A.ProbeDepthParamsC) == 48 and A.ProbeDepthParamsC.time.offset == 24 and A.ProbeDepthParamsC.t_max.offset == 40
    assert C.sizeof(A.ProbeVisibleParamsC) == 32 and A.ProbeVisibleParamsC.normal_bias.offset == 8
    p = N.probe_depth_defaults()
    assert (p.map_size, p.samples, p.seed, p.point_base, p.jitter, p.pad) == (16, 8, 0, 0, 1, 0)
    assert (p.time, p.t_min, p.t_max) == (0.0, 0.001, 0.0)  # t_max has no default: the block as it stands is rejected
    pt = N.probe_points(np.zeros((1, 3)))
    ray = np.zeros(1, dtype=A.RAY_DTYPE)
    assert N.lib().rtr_probe_depth_ray(C.byref(p), pt.ctypes.data, 0, 0, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID


# ---- the octahedral map ----

def _square_points():
    rng = np.random.default_rng(3)
    uv = [rng.random((256, 2)) * 2.0 - 1.0]
    edge = np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0])
    uv.append(np.array([(u, v) for u in edge for v in edge]))  # corners, edges, the axes, |u| + |v| == 1 exactly (z == 0)
    return np.concatenate(uv)


def test_decode_equals_the_restatement():
    uv = _square_points()
    got = N.octa_decode(uv)
    want = np.array([DR.decode(float(u), float(v)) for u, v in uv])
    assert _same_bits(got, want)
    length = np.sqrt((got * got).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 4e-16
    on_fold = np.abs(uv[:, 0]) + np.abs(uv[:, 1]) == 1.0
    assert on_fold.sum() >= 8 and (got[on_fold, 2] == 0.0).all()  # z == 0 exactly takes the upper rule


def test_encode_equals_the_restatement_with_signed_zeros_and_z_zero():
    rng = np.random.default_rng(4)
    d = [rng.standard_normal((256, 3)) * 10.0 ** rng.integers(-3, 4, (256, 1))]
    z = (0.0, -0.0)
    d.append(np.array([(x, y, w) for x in z + (1.5, -2.0) for y in z + (0.5, -3.0) for w in z + (1.0, -1.0)
                       if (x, y, w) != (0.0, 0.0, 0.0) and abs(x) + abs(y) + abs(w) > 0]))
    d = np.concatenate(d)
    got = N.octa_encode(d)
    want = np.array([DR.encode(float(x), float(y), float(w)) for x, y, w in d])
    assert _same_bits(got, want)
    assert np.abs(got).max() <= 1.0
    # sg(-0.0) is +1: straight down lands on the corner (1, 1), whatever the signs of the zeros
    for x in z:
        for y in z:
            assert N.octa_encode(np.array([x, y, -1.0])).tolist() == [1.0, 1.0]
    # z == -0.0 is not below zero: no fold
    assert N.octa_encode(np.array([1.0, 1.0, -0.0])).tolist() == [0.5, 0.5]


@pytest.mark.parametrize("T", (1, 2, 3, 16))
def test_texel_centres_round_trip(T):
    for b in range(T):
        for a in range(T):
            u, v = (2.0 * (a + 0.5)) / T - 1.0, (2.0 * (b + 0.5)) / T - 1.0
            ox, oy = N.octa_encode(N.octa_decode(np.array([u, v])))
            assert (int(((ox + 1.0) * T) * 0.5), int(((oy + 1.0) * T) * 0.5)) == (a, b), (T, a, b, ox, oy)
            assert abs(ox - u) <= 4e-16 and abs(oy - v) <= 4e-16


@pytest.mark.parametrize("T,samples,jitter", ((1, 3, 1), (3, 5, 1), (3, 2, 0), (16, 1, 1)))
def test_ray_equals_the_restatement(T, samples, jitter):
    rng = np.random.default_rng(T)
    pts = rng.standard_normal((3, 3))
    got = N.probe_depth_rays(pts, map_size=T, samples=samples, seed=9, jitter=jitter, point_base=0xFFFFFFFE, time=0.25,
                             t_min=-1.0, t_max=7.5)
    d, st = DR.rays(3, T, samples, seed=9, point_base=0xFFFFFFFE, jitter=jitter)
    assert got.shape == (3, T, T, samples)
    assert _same_bits(got["direction"], d) and (got["rng_state"] == st).all()
    assert _same_bits(got["origin"], np.broadcast_to(pts[:, None, None, None, :], d.shape))
    assert (got["time"] == 0.25).all() and (got["t_min"] == -1.0).all() and (got["t_max"] == 7.5).all()
    if not jitter:  # nothing is drawn: the state is the seed's
        k = (np.arange(3, dtype=np.uint64) + np.uint64(0xFFFFFFFE)) & DR.M32
        e = np.arange(T * T, dtype=np.uint64).reshape(T, T)
        seed = DR.CR.sample_seed(9, T * T, e[None, :, :, None], k[:, None, None, None], np.arange(samples, dtype=np.uint64))
        assert (got["rng_state"] == seed).all()


# ---- the visible lookup ----

def _random_maps(n_probes, T, rng, lo=0.1, hi=0.6, spread=0.05):
    """maps whose texels all differ: mean in [lo, hi), mean2 = mean^2 + up to ``spread``"""
    d = np.zeros((n_probes, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    d["mean"] = lo + rng.random((n_probes, T, T)) * (hi - lo)
    d["mean2"] = d["mean"] * d["mean"] + rng.random((n_probes, T, T)) * spread
    d["hits"], d["valid"] = 8, 1
    return d


def _sh(n, rng):
    probes = np.zeros(n, dtype=A.PROBE_SH_DTYPE)
    probes["c"] = rng.standard_normal((n, 9, 3))
    probes["count"], probes["valid"] = 64, 1
    return probes


def _edge_directions(T):
    """directions within half a texel of the four edges and the four corners of the square, and the exact edges"""
    h = 0.5 / T  # a quarter texel in (u, v)
    near = (-1.0, -1.0 + h, 1.0 - h, 1.0)
    mid = (-0.3, 0.0, 0.45)
    uv = [(u, v) for u in near for v in near] + [(u, v) for u in near for v in mid] + [(u, v) for u in mid for v in near]
    return np.array([DR.decode(u, v) for u, v in uv]), np.array(uv)


def visible_cases():
    """(name, grid, (origin, spacing, dims), probes, depth [n, T, T], normal_bias, points, normals) of the cases both the
    host form and the kernel are held to"""
    cases = []
    rng = np.random.default_rng(23)
    # the grids, probes and queries of the plain lookup, with maps whose every texel differs
    for name, grid, host, probes, pts, nrm in TP.lookup_cases():
        n = len(probes)
        for T in ((3, 8) if name == "inside and clamped" else (4,)):
            cases.append(("%s, T=%d" % (name, T), grid, host, probes, _random_maps(n, T, rng, 0.2, 2.5, 0.5), 0.1, pts, nrm))
    # the folds: queries around the middle probe of a 3 x 1 x 1 grid, a quarter texel from every edge and corner of its map
    origin, spacing, dims = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 1, 1)
    grid = N.probe_grid(origin, spacing, dims)
    for T in (1, 2, 5, 8):
        d, _ = _edge_directions(T)
        r = 0.35 + 0.5 * rng.random((len(d), 1))
        pts = np.array([1.0, 0.0, 0.0]) + r * d
        nrm = rng.standard_normal((len(d), 3))
        cases.append(("folds, T=%d" % T, grid, (origin, spacing, dims), _sh(3, rng), _random_maps(3, T, rng), 0.0, pts, nrm))
    # exact branches on a 2 x 1 x 1 grid at the origin: flat maps (mean m, mean2 m * m) along +x, where FETCH is exact
    dims = (2, 1, 1)
    grid = N.probe_grid(origin, spacing, dims)
    m = 0.375
    flat = DR.flat_maps(2, 2, m)
    up = math.nextafter(m, math.inf)
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [m, 0.0, 0.0], [up, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0],
                    [0.5, 0.0, 0.0], [0.25, 0.5, 0.0], [0.25, 0.0, -0.5]])
    nrm = np.array([[0.0, 1.0, 0.0]] * 6 + [[-3.0, 0.0, 0.0], [0.0, 0.0, 2.0], [1.0, 1.0, 0.0]])
    cases.append(("r2 == 0, r <= m1 and one ulp above", grid, (origin, spacing, dims), _sh(2, rng), flat, 0.0, pts, nrm))
    r = 1e-150  # r * r is a normal number, but (r - m1)^2 underflows to 0 beside a variance of exactly 0
    tiny = DR.flat_maps(2, 2, r * (1.0 - 2.0 ** -40))
    cases.append(("den == 0", grid, (origin, spacing, dims), _sh(2, rng), tiny, 0.0, np.array([[r, 0.0, 0.0]]),
                  np.array([[0.0, 1.0, 0.0]])))
    holes = _random_maps(2, 4, rng)
    holes["valid"][0, 1:3, 2:4] = 0
    holes["mean"][0, 1:3, 2:4] = np.nan
    d = np.array([DR.decode(u, v) for u in (0.05, 0.3, 0.6, 0.9) for v in (-0.6, -0.3, 0.0, 0.3)])  # into the hole and beside it
    cases.append(("an invalid tap", grid, (origin, spacing, dims), _sh(2, rng), holes, 0.0, 0.7 * d, rng.standard_normal((len(d), 3))))
    return cases


def _reference(case, weights=None):
    name, grid, (origin, spacing, dims), probes, depth, bias, pts, nrm = case
    return DR.lookup_visible(origin, spacing, dims, probes, depth, bias, pts, nrm, weights)


CASES = visible_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_lookup_equals_the_restatement(case):
    name, grid, host, probes, depth, bias, pts, nrm = case
    got = N.probe_lookup_visible_host(grid, probes, depth, pts, nrm, normal_bias=bias)
    assert _same_bits(got, _reference(case)), name
    if name.startswith("all corners invalid"):
        assert _same_bits(got, np.zeros(len(got), dtype=A.GATHER_OUT_DTYPE))
    elif name.startswith("one invalid corner"):
        assert got["count"][0] == 7 and np.isfinite(got["v"]).all()
    else:
        assert (got["valid"] == 1).all() and np.isfinite(got["v"]).all()


def test_the_cases_reach_every_branch():
    """what the restatement says of the cases above: every rule of the visibility, the floor taken and not taken, every fold,
    a corner dropped for its SH record, axes of one probe and queries outside the box"""
    seen, floored, folds, invalid_corner = set(), set(), set(), False
    for case in CASES:
        name, grid, (origin, spacing, dims), probes, depth, bias, pts, nrm = case
        trace = []
        _reference(case, trace)
        for corners in trace:
            invalid_corner = invalid_corner or (0 < len(corners) < 8 and (probes["valid"] == 0).any())
            for pi, tri, wb, c, wv, branch, was_floored in corners:
                seen.add(branch)
                floored.add(was_floored)
        if name.startswith("folds"):
            T = depth.shape[1]
            for p in pts:
                ox, oy = DR.encode(*(p - np.array([1.0, 0.0, 0.0])))
                ia, ib = DR._axis(ox, T)[0], DR._axis(oy, T)[0]
                folds.add((ia < 0, ia + 1 > T - 1, ib < 0, ib + 1 > T - 1))
    assert seen == {"r2 == 0", "!ok", "r <= m1", "den == 0", "chebyshev"}
    assert floored == {True, False} and invalid_corner
    for low_a, high_a, low_b, high_b in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1),
                                         (0, 1, 1, 0), (0, 1, 0, 1)):
        assert (bool(low_a), bool(high_a), bool(low_b), bool(high_b)) in folds
    names = " ".join(c[0] for c in CASES)
    assert "1x1x1" in names and "a flat axis" in names and "inside and clamped" in names  # dims == 1, queries outside


def test_one_ulp_decides_between_full_weight_and_the_floor():
    case = next(c for c in CASES if c[0].startswith("r2 == 0"))
    trace = []
    _reference(case, trace)
    by_probe = [{pi: (c, branch, floored) for pi, tri, wb, c, wv, branch, floored in corners} for corners in trace]
    assert by_probe[0][0][1] == "r2 == 0" and by_probe[1][1][1] == "r2 == 0"  # at a probe, bias 0
    assert by_probe[2][0] == (1.0, "r <= m1", False)  # r == m1 exactly
    assert by_probe[3][0] == (0.0, "chebyshev", True)  # one ulp farther: no spread, so no chance, and the floor holds
    assert by_probe[4][0][1] == "r <= m1" and by_probe[5][0][1] == "chebyshev"


def test_fold_stays_inside_the_map_and_continues_the_square():
    """every tap index -1 .. T folds into the map; a direction on an edge reads the same texels from either side"""
    for T in (1, 2, 5, 8):
        for ia in range(-1, T + 1):
            for ib in range(-1, T + 1):
                fa, fb = DR.fold(ia, ib, T)
                assert 0 <= fa < T and 0 <= fb < T
                if 0 <= ia < T and 0 <= ib < T:
                    assert (fa, fb) == (ia, ib)
    # a smooth function of the direction, sampled at the texel centres: the fetch across an edge is as good as inside
    T = 16
    m = np.zeros((1, T, T), dtype=A.PROBE_DEPTH_DTYPE)
    f = lambda d: 2.0 + d[0] + 0.5 * d[1] * d[2]
    for b in range(T):
        for a in range(T):
            m["mean"][0, b, a] = f(DR.decode((2.0 * (a + 0.5)) / T - 1.0, (2.0 * (b + 0.5)) / T - 1.0))
    m["valid"] = 1
    grid = np.linspace(-1.0, 1.0, 97)
    lim = 1.0 - 1.0 / T  # beyond the outermost texel centres a tap folds
    border = np.array([DR.decode(u, v) for u in grid for v in grid if max(abs(u), abs(v)) > lim])
    inner = np.array([DR.decode(u, v) for u in grid for v in grid if max(abs(u), abs(v)) <= lim])
    err = lambda ds: max(abs(DR.fetch(m[0], d)[0] - f(d)) for d in ds)
    print("fetch error: interior %.3e, border %.3e" % (err(inner), err(border)))
    assert err(border) <= err(inner)  # the interior's worst is the diagonal kink of the octahedron; a fold adds nothing to it


def test_parameter_rejections():
    lib = N.lib()
    pt = N.probe_points(np.zeros((1, 3)))
    ray = np.zeros(1, dtype=A.RAY_DTYPE)

    def ray_rc(point=pt, index=0, a=0, b=0, s=0, **fields):
        p = N.probe_depth_defaults(t_max=2.0)
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.rtr_probe_depth_ray(C.byref(p), point.ctypes.data, index, a, b, s, ray.ctypes.data)

    assert ray_rc() == 0
    inf, nan = math.inf, math.nan
    for bad in (dict(map_size=0), dict(map_size=65), dict(samples=0), dict(samples=(1 << 20) + 1), dict(jitter=2), dict(jitter=-1),
                dict(pad=1), dict(time=inf), dict(time=nan), dict(t_min=inf), dict(t_min=nan), dict(t_min=-inf), dict(t_max=inf),
                dict(t_max=nan), dict(t_max=0.001), dict(t_max=0.0005), dict(t_min=3.0)):
        assert ray_rc(**bad) == A.RTR_ERR_INVALID, bad
    for ok in (dict(map_size=64), dict(samples=1 << 20), dict(t_min=0.0), dict(t_min=-1.0), dict(t_min=2.0 ** -200), dict(jitter=0)):
        assert ray_rc(**ok) == 0, ok
    assert ray_rc(index=-1) == ray_rc(a=16) == ray_rc(a=-1) == ray_rc(b=16) == ray_rc(s=8) == ray_rc(s=-1) == A.RTR_ERR_INVALID
    assert ray_rc(point=N.probe_points(np.array([[0.0, nan, 0.0]]))) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_depth_ray(None, pt.ctypes.data, 0, 0, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    p = N.probe_depth_defaults(t_max=2.0)
    assert lib.rtr_probe_depth_ray(C.byref(p), None, 0, 0, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_depth_ray(C.byref(p), pt.ctypes.data, 0, 0, 0, 0, None) == A.RTR_ERR_INVALID

    rng = np.random.default_rng(2)
    probes, depth = _sh(2, rng), _random_maps(2, 4, rng).reshape(-1)
    q = N.gather_points(np.array([[0.5, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)

    def one_rc(grid=None, query=q, dims=(2, 1, 1), spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), gpad=0, **fields):
        g = grid if grid is not None else N.probe_grid(origin, spacing, dims)
        g.pad = gpad
        vp = N.probe_visible_params(4, 0.1)
        for k, v in fields.items():
            if k == "reserved":
                vp.reserved[v] = 1.0
            else:
                setattr(vp, k, v)
        return lib.rtr_probe_lookup_visible_one(C.byref(g), probes.ctypes.data, depth.ctypes.data, C.byref(vp),
                                                query.ctypes.data, out.ctypes.data)

    assert one_rc() == 0 and out["valid"][0] == 1
    for bad in (dict(map_size=0), dict(map_size=65), dict(pad=1), dict(normal_bias=-0.5), dict(normal_bias=inf),
                dict(normal_bias=nan), dict(reserved=0), dict(reserved=1), dict(gpad=1), dict(dims=(0, 1, 1)),
                dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, inf, 1.0)), dict(origin=(nan, 0.0, 0.0)),
                dict(dims=(1 << 12, 1 << 12, 2)),       # the plain lookup's rule: more than 2^24 probes
                dict(dims=(1 << 10, 1 << 10, 2)),       # 2^21 probes x 4^2 texels > 2^24
                dict(query=N.gather_points(np.array([[0.5, 0.0, 0.0]]), np.array([[0.0, 0.0, 0.0]]))),
                dict(query=N.gather_points(np.array([[inf, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]])))):
        assert one_rc(**bad) == A.RTR_ERR_INVALID, bad
    assert one_rc(normal_bias=0.0) == 0
    g = N.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))
    vp = N.probe_visible_params(4, 0.1)
    args = [C.byref(g), probes.ctypes.data, depth.ctypes.data, C.byref(vp), q.ctypes.data, out.ctypes.data]
    for k in range(6):
        assert lib.rtr_probe_lookup_visible_one(*[None if i == k else a for i, a in enumerate(args)]) == A.RTR_ERR_INVALID, k
    with pytest.raises(TypeError):
        N.probe_depth_defaults(face_size=3)


# ---- a wall between two probes ----

def _wall():
    """2 x 1 x 1 probes one unit apart, probe 0 in a room of radiance 1 and probe 1 in the dark, a wall at x = 0.4"""
    origin, spacing, dims = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1)
    probes = np.zeros(2, dtype=A.PROBE_SH_DTYPE)
    probes["c"][0, 0] = PR.K0
    probes["count"], probes["valid"] = 64, 1
    x = np.linspace(0.45, 0.9, 10)
    pts = np.array([(xi, y, 0.1) for xi in x for y in (0.0, 0.2)] * 3)
    nrm = np.repeat(np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), len(pts) // 3, axis=0)
    return N.probe_grid(origin, spacing, dims), (origin, spacing, dims), probes, pts, nrm


def test_a_wall_keeps_the_lit_probe_out():
    """T = 16, the default map size.  How close behind the wall a query may stand is a matter of the map's resolution: at
    T = 8 the off-axis query 0.05 behind it reads a bilinear mean beyond its own distance and, with the wrap weight on the
    lit probe's side, takes MORE from it than the plain lookup does."""
    grid, (origin, spacing, dims), probes, pts, nrm = _wall()
    T, t_max, bias = 16, 1.5 * math.sqrt(3.0), 0.02
    depth = np.stack([DR.plane_map(T, 0, 0.4, t_max, 1e-4), DR.plane_map(T, 0, -0.6, t_max, 1e-4)])
    plain = N.probe_lookup_host(grid, probes, pts, nrm)["v"][:, 0]
    got = N.probe_lookup_visible_host(grid, probes, depth, pts, nrm, normal_bias=bias)
    trace = []
    want = DR.lookup_visible(origin, spacing, dims, probes, depth, bias, pts, nrm, trace)
    assert _same_bits(got, want)
    vis = got["v"][:, 0]
    assert (plain > 0).all() and (vis >= 0).all()
    assert (vis < plain).all()
    share = lambda corners: corners[0][1] * corners[0][4] / sum(c[1] * c[4] for c in corners)
    lit = np.array([share(c) for c in trace])
    tri = np.array([c[0][1] for c in trace])
    deep = pts[:, 0] >= 0.65  # a quarter spacing behind the wall
    print("lit probe's share: trilinear %.2f .. %.2f, visible at most %.2e (%.2e a quarter spacing behind the wall)"
          % (tri.min(), tri.max(), lit.max(), lit[deep].max()))
    assert 0.09 <= tri.min() and tri.max() <= 0.56 and lit[deep].max() < 1e-4
    assert np.allclose(vis / np.pi, lit, rtol=1e-12, atol=0)  # E = pi x the lit probe's share


def test_nothing_in_the_way_leaves_only_the_wrap_weight():
    grid, (origin, spacing, dims), probes, pts, nrm = _wall()
    T, t_max = 8, 1.5 * math.sqrt(3.0)
    depth = DR.flat_maps(2, T, t_max)
    got = N.probe_lookup_visible_host(grid, probes, depth, pts, nrm, normal_bias=0.02)
    trace = []
    want = DR.lookup_visible(origin, spacing, dims, probes, depth, 0.02, pts, nrm, trace)
    assert _same_bits(got, want)
    for corners, p, n, v in zip(trace, pts, nrm, got["v"][:, 0]):
        assert [c[3] for c in corners] == [1.0, 1.0] and [c[5] for c in corners] == ["r <= m1"] * 2
        w = n / math.sqrt(n @ n)
        wb = [((((P - p) @ w) / math.sqrt((P - p) @ (P - p)) + 1.0) * 0.5) ** 2 + 0.2 for P in (np.zeros(3), np.array([1.0, 0, 0]))]
        t = p[0]
        expect = (1.0 - t) * wb[0] / ((1.0 - t) * wb[0] + t * wb[1])
        assert abs(v / np.pi - expect) <= 1e-14
