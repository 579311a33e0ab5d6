"""Light probes (include/rtr_hip.h: rtr_probe_*, rtr_sh_*) without a GPU: the declarations and record layouts, the
host-only rtr_probe_ray, rtr_sh_basis, rtr_sh_irradiance and rtr_probe_lookup_one against the numpy restatement of the
contract (tests/_probe_ref.py) bit for bit, the orthonormality of the basis over the library's own directions, and the
irradiance of a constant."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G
import _probe_ref as PR

A = G.A
rtr = G.rtr

NAMES = ("rtr_probe_visibility", "rtr_probe_radiance", "rtr_probe_visibility_device", "rtr_probe_radiance_device",
         "rtr_probe_ray", "rtr_sh_basis", "rtr_sh_irradiance", "rtr_probe_lookup", "rtr_probe_lookup_device",
         "rtr_probe_lookup_one")
SAMPLES = (1, 5, 64)


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_header_declares_the_entries_and_the_abi_stays_4():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", text))
    lib = rtr.native.lib()
    for name in NAMES:
        assert name in declared and name in rtr.native.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("rtr_probe_point", "rtr_probe_vis", "rtr_probe_sh", "rtr_probe_grid"):
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+4\b", _header())
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert "rtr_test_last_probe" in rtr.native.TEST_EXPORTS


def test_record_layouts_equal_the_mirrors():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)

    def body(name):
        return " ".join(re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1).split())

    assert body("rtr_probe_point") == "double p[3];" and A.PROBE_POINT_DTYPE.itemsize == 24
    assert body("rtr_probe_vis") == "double c[9]; int32_t count, valid;" and A.PROBE_VIS_DTYPE.itemsize == 80
    assert body("rtr_probe_sh") == "double c[9][3]; int32_t count, valid;" and A.PROBE_SH_DTYPE.itemsize == 224
    assert body("rtr_probe_grid") == "double origin[3], spacing[3]; int32_t dims[3], pad;"
    assert C.sizeof(A.ProbeGridC) == A.PROBE_GRID_SIZE == 64
    assert [n for n, _ in A.ProbeGridC._fields_] == ["origin", "spacing", "dims", "pad"]
    assert A.PROBE_VIS_DTYPE.fields["count"][1] == 72 and A.PROBE_SH_DTYPE.fields["count"][1] == 216
    assert A.PROBE_SH_DTYPE["c"].shape == (9, 3)


def test_a_null_context_is_invalid():
    lib = rtr.native.lib()
    gp = rtr.native.gather_defaults()
    rp = A.make_params(16, 16, 1)
    pts = np.zeros(2, dtype=A.PROBE_POINT_DTYPE)
    vis = np.zeros(2, dtype=A.PROBE_VIS_DTYPE)
    sh = np.zeros(2, dtype=A.PROBE_SH_DTYPE)
    q = np.zeros(2, dtype=A.GATHER_POINT_DTYPE)
    q["n"][:, 1] = 1.0
    out = np.zeros(2, dtype=A.GATHER_OUT_DTYPE)
    grid = rtr.native.probe_grid((0, 0, 0), (1, 1, 1), (2, 1, 1))
    inv = A.RTR_ERR_INVALID
    assert lib.rtr_probe_visibility(None, C.byref(gp), pts.ctypes.data, vis.ctypes.data, 2) == inv
    assert lib.rtr_probe_radiance(None, C.byref(rp), C.byref(gp), pts.ctypes.data, sh.ctypes.data, 2) == inv
    assert lib.rtr_probe_visibility_device(None, C.byref(gp), pts.ctypes.data, vis.ctypes.data, 2, 1) == inv
    assert lib.rtr_probe_radiance_device(None, C.byref(rp), C.byref(gp), pts.ctypes.data, sh.ctypes.data, 2, 1) == inv
    assert lib.rtr_probe_lookup(None, C.byref(grid), sh.ctypes.data, q.ctypes.data, out.ctypes.data, 2) == inv
    assert lib.rtr_probe_lookup_device(None, C.byref(grid), sh.ctypes.data, q.ctypes.data, out.ctypes.data, 2, 1) == inv
    assert not vis.view(np.uint8).any() and not sh.view(np.uint8).any() and not out.view(np.uint8).any()


@pytest.mark.parametrize("samples", SAMPLES)
def test_probe_ray_equals_the_restatement(samples):
    p = PR.displaced_points(21, 0.5)
    assert len(p) == 48
    for seed, base, time, t_max in ((7, 0, 0.0, np.inf), (0xFFFFFFF1, 0xFFFFFFE0, 0.5, 150.0)):  # (k wraps modulo 2^32)
        got = rtr.native.probe_rays(p, samples=samples, seed=seed, point_base=base, time=time, t_max=t_max, t_min=0.25)
        d, st = PR.rays(len(p), samples, seed, base)
        assert got.shape == (len(p), samples)
        assert np.array_equal(_bits(got["direction"]), _bits(d))
        assert np.array_equal(got["rng_state"], st) and (st != 0).all()
        assert np.array_equal(_bits(got["origin"]), _bits(np.repeat(p[:, None, :], samples, axis=1)))
        assert (got["time"] == time).all() and (got["t_min"] == 0.25).all() and (got["t_max"] == t_max).all()
        assert (got["pad"] == 0).all()
    # the draws are the gathers': u of the gather contract before the normal is added, so the states agree
    _, gst = GR.rays(p, np.tile([0.0, 1.0, 0.0], (len(p), 1)), samples, 7, 0)
    assert np.array_equal(PR.rays(len(p), samples, 7, 0)[1], gst)


def test_probe_ray_rejects_bad_points_and_bad_params():
    lib = rtr.native.lib()
    ray = np.zeros(1, dtype=A.RAY_DTYPE)
    ray.view(np.uint8)[:] = 0xA5

    def call(gp, pt, k=0, s=0):
        return lib.rtr_probe_ray(C.byref(gp), pt.ctypes.data, k, s, ray.ctypes.data)

    good = np.zeros(1, dtype=A.PROBE_POINT_DTYPE)
    good["p"] = (1.0, 2.0, 3.0)
    gp = rtr.native.gather_defaults(samples=4)
    for a, value in ((0, np.nan), (2, np.inf), (1, -np.inf)):
        bad = good.copy()
        bad["p"][0, a] = value
        assert call(gp, bad) == A.RTR_ERR_INVALID, (a, value)
    assert call(gp, good, 0, 4) == call(gp, good, 0, -1) == call(gp, good, -1, 0) == A.RTR_ERR_INVALID
    for kw in (dict(samples=0), dict(samples=(1 << 20) + 1), dict(flags=2), dict(flags=1 | 4), dict(time=np.nan),
               dict(t_min=np.inf), dict(t_min=np.nan), dict(t_max=np.nan)):
        assert call(rtr.native.gather_defaults(**kw), good) == A.RTR_ERR_INVALID, kw
    gp = rtr.native.gather_defaults()
    gp.reserved[1] = 1.0
    assert call(gp, good) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_ray(None, good.ctypes.data, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_ray(C.byref(rtr.native.gather_defaults()), None, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert (ray.view(np.uint8) == 0xA5).all()  # nothing was written
    for kw in (dict(t_min=0.0), dict(t_min=-1.0), dict(t_max=-np.inf), dict(samples=1 << 20), dict(flags=1)):
        assert call(rtr.native.gather_defaults(**kw), good) == A.RTR_OK, kw
    with pytest.raises(rtr.RtrError):
        rtr.native.probe_rays(np.array([[0.0, np.nan, 0.0]]))
    with pytest.raises(rtr.RtrError):
        rtr.native.probe_rays(good["p"], samples=0)


@pytest.mark.parametrize("samples", SAMPLES)
def test_sh_basis_equals_the_restatement(samples):
    d, _ = PR.rays(48, samples, 7)
    assert np.array_equal(_bits(rtr.native.sh_basis(d)), _bits(PR.basis(d)))
    other = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [-0.0, 1.0, 0.0], [0.3, -1.7, 0.9], [0.0, 0.0, 0.0]])
    assert np.array_equal(_bits(rtr.native.sh_basis(other)), _bits(PR.basis(other)))  # taken as given, unit or not


def _coefficients(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((9, 3)) * 10.0 ** rng.integers(-2, 3, (9, 3))


@pytest.mark.parametrize("samples", SAMPLES)
def test_sh_irradiance_equals_the_restatement(samples):
    d, _ = PR.rays(48, samples, 7)
    normals = (d * np.linspace(0.25, 7.0, 48)[:, None, None]).reshape(-1, 3)  # normals need not be normalised
    c = _coefficients(samples)
    got = rtr.native.sh_irradiance(c, normals)
    want = np.array([PR.irradiance(c, n) for n in normals])
    assert np.array_equal(_bits(got), _bits(want))


def test_sh_irradiance_rejects_bad_normals():
    lib = rtr.native.lib()
    c = _coefficients(1)
    E = np.full(3, 7.0)
    for normal in ((0.0, 0.0, 0.0), (1e-200, 0.0, 0.0), (1e200, 1e200, 0.0), (np.nan, 1.0, 0.0), (0.0, np.inf, 0.0)):
        n = np.array(normal)
        assert lib.rtr_sh_irradiance(c.ctypes.data, n.ctypes.data, E.ctypes.data) == A.RTR_ERR_INVALID, normal
    n = np.array([0.0, 1.0, 0.0])
    assert lib.rtr_sh_irradiance(None, n.ctypes.data, E.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_sh_irradiance(c.ctypes.data, None, E.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_sh_irradiance(c.ctypes.data, n.ctypes.data, None) == A.RTR_ERR_INVALID
    assert (E == 7.0).all()
    with pytest.raises(rtr.RtrError):
        rtr.native.sh_irradiance(c, np.zeros((1, 3)))


def test_basis_is_orthonormal_over_the_library_directions():
    """One probe, N = 65 536, seed 7: the mean of 4 pi Y_i Y_j lies within 6 of its own sample standard errors of delta_ij
    for every pair but (0, 0), which is a constant (within 1e-15 of 1)."""
    N = 65536
    d = rtr.native.probe_rays(np.zeros((1, 3)), samples=N, seed=7)["direction"][0]
    assert np.array_equal(_bits(d), _bits(PR.rays(1, N, 7)[0][0]))
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 4 * 2.0 ** -53
    Y = rtr.native.sh_basis(d)
    worst = (0.0, 0.0, None)
    for i in range(9):
        for j in range(i, 9):
            x = PR.FOUR_PI * Y[:, i] * Y[:, j]
            delta = 1.0 if i == j else 0.0
            if (i, j) == (0, 0):
                assert np.abs(x - 1.0).max() <= 1e-15
                continue
            err = abs(x.mean() - delta)
            se = x.std(ddof=1) / np.sqrt(N)
            if err / se > worst[0]:
                worst = (err / se, err, (i, j))
            assert err <= 6 * se, (i, j, err, se)
    print("worst pair %s: %.2f standard errors, %.2e absolute" % (worst[2], worst[0], worst[1]))


def test_irradiance_of_a_constant_is_pi():
    """radiance 1 from every direction: c[0] = K0 per channel (the mean of Y0 * 1), the rest 0; E = pi for any normal"""
    c = np.zeros((9, 3))
    c[0] = PR.K0
    d, _ = PR.rays(4, 64, 3)
    normals = np.concatenate([d.reshape(-1, 3), [[0.0, 0.0, 5.0], [3.0, -4.0, 12.0]]])
    E = rtr.native.sh_irradiance(c, normals)
    assert np.abs(E / np.pi - 1.0).max() <= 1e-15


def _grid_case(dims, seed=5):
    """(grid, host grid, probes) with random coefficients"""
    origin, spacing = (-1.0, 0.5, 2.0), (0.5, 1.25, 2.0)
    n = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(seed)
    probes = np.zeros(n, dtype=A.PROBE_SH_DTYPE)
    probes["c"] = rng.standard_normal((n, 9, 3))
    probes["count"], probes["valid"] = 64, 1
    return rtr.native.probe_grid(origin, spacing, dims), (origin, spacing, dims), probes


def lookup_cases():
    """(name, grid, (origin, spacing, dims), probes, points, normals) of the lookup cases both the host form and the kernel
    are held to"""
    rng = np.random.default_rng(11)
    cases = []
    grid, host, probes = _grid_case((3, 2, 2))
    origin, spacing, dims = host
    inside = np.asarray(origin) + rng.random((24, 3)) * (np.asarray(dims) - 1) * np.asarray(spacing)
    outside = np.asarray(origin) + (rng.random((12, 3)) * 4.0 - 1.5) * (np.asarray(dims) - 1) * np.asarray(spacing)
    pts = np.concatenate([inside, outside, [[1e300, -1e300, 0.0]]])
    nrm = rng.standard_normal((len(pts), 3)) * 3.0
    cases.append(("inside and clamped", grid, host, probes, pts, nrm))
    one_bad = probes.copy()
    bad_index = 1 + 3 * (1 + 2 * 0)  # probe (1, 1, 0): a corner of cell (0, 0, 0)
    one_bad["valid"][bad_index] = 0
    one_bad["c"][bad_index] = np.nan  # an invalid probe's coefficients never enter a sum
    cell = np.asarray(origin) + np.array([0.3, 0.6, 0.45]) * np.asarray(spacing)  # strictly inside cell (0, 0, 0)
    cases.append(("one invalid corner", grid, host, one_bad, cell[None, :], np.array([[0.2, 1.0, -0.4]])))
    none = probes.copy()
    none["valid"] = 0
    cases.append(("all corners invalid", grid, host, none, cell[None, :], np.array([[0.2, 1.0, -0.4]])))
    g1, h1, p1 = _grid_case((1, 1, 1))
    cases.append(("1x1x1", g1, h1, p1, np.array([[0.0, 0.0, 0.0], [-1.0, 0.5, 2.0], [50.0, -3.0, 7.0]]),
                  np.array([[0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, -2.0, 0.0]])))
    g2, h2, p2 = _grid_case((4, 1, 3))
    o2, s2, d2 = h2
    q2 = np.asarray(o2) + rng.random((16, 3)) * np.array([3.0, 1.0, 2.0]) * np.asarray(s2)
    cases.append(("a flat axis", g2, h2, p2, q2, rng.standard_normal((16, 3))))
    return cases


@pytest.mark.parametrize("case", lookup_cases(), ids=lambda c: c[0])
def test_lookup_equals_the_restatement(case):
    name, grid, (origin, spacing, dims), probes, pts, nrm = case
    got = rtr.native.probe_lookup_host(grid, probes, pts, nrm)
    want = PR.lookup(origin, spacing, dims, probes, pts, nrm)
    assert _same_bits(got, want), name
    if name == "one invalid corner":
        assert got["count"][0] == 7 and got["valid"][0] == 1 and np.isfinite(got["v"]).all()
    if name == "all corners invalid":
        assert _same_bits(got, np.zeros(1, dtype=A.GATHER_OUT_DTYPE))
    if name == "inside and clamped":
        assert (got["valid"] == 1).all() and got["count"].max() == 8


def test_lookup_at_a_probe_equals_its_irradiance():
    grid, (origin, spacing, dims), probes = _grid_case((3, 2, 2))
    nrm = np.array([0.3, -1.7, 0.9])
    for iz in range(dims[2]):
        for iy in range(dims[1]):
            for ix in range(dims[0]):
                p = np.asarray(origin) + np.array([ix, iy, iz], dtype=np.float64) * np.asarray(spacing)
                got = rtr.native.probe_lookup_host(grid, probes, p[None, :], nrm[None, :])
                want = rtr.native.sh_irradiance(probes["c"][ix + dims[0] * (iy + dims[1] * iz)], nrm)
                assert np.array_equal(_bits(got["v"][0]), _bits(want)), (ix, iy, iz)
                assert got["count"][0] == 1 and got["valid"][0] == 1


def test_lookup_rejects_bad_grids_and_bad_queries():
    lib = rtr.native.lib()
    grid, _, probes = _grid_case((3, 2, 2))
    q = np.zeros(1, dtype=A.GATHER_POINT_DTYPE)
    q["n"] = (0.0, 1.0, 0.0)
    out = np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    out.view(np.uint8)[:] = 0xA5

    def call(g, query=q):
        return lib.rtr_probe_lookup_one(C.byref(g), probes.ctypes.data, query.ctypes.data, out.ctypes.data)

    for change in (lambda g: g.spacing.__setitem__(0, 0.0), lambda g: g.spacing.__setitem__(1, -1.0),
                   lambda g: g.spacing.__setitem__(2, np.inf), lambda g: g.spacing.__setitem__(0, np.nan),
                   lambda g: g.origin.__setitem__(1, np.nan), lambda g: g.dims.__setitem__(0, 0),
                   lambda g: g.dims.__setitem__(2, -1), lambda g: setattr(g, "pad", 1)):
        g = rtr.native.probe_grid((-1.0, 0.5, 2.0), (0.5, 1.25, 2.0), (3, 2, 2))
        change(g)
        assert call(g) == A.RTR_ERR_INVALID
    big = rtr.native.probe_grid((0, 0, 0), (1, 1, 1), (1 << 12, 1 << 12, 2))  # 2^25 probes
    assert call(big) == A.RTR_ERR_INVALID
    for field, a, value in (("p", 0, np.nan), ("p", 2, np.inf), ("n", 1, np.nan)):
        bad = q.copy()
        bad[field][0, a] = value
        assert call(grid, bad) == A.RTR_ERR_INVALID
    zero = q.copy()
    zero["n"] = 0.0
    assert call(grid, zero) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_lookup_one(None, probes.ctypes.data, q.ctypes.data, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_probe_lookup_one(C.byref(grid), None, q.ctypes.data, out.ctypes.data) == A.RTR_ERR_INVALID
    assert (out.view(np.uint8) == 0xA5).all()
    assert call(grid) == A.RTR_OK


def test_probe_grid_positions_and_checks():
    g = rtr.ProbeGrid.in_box((0.0, 1.0, 2.0), (2.0, 1.0, 5.0), (3, 1, 2))
    pos = g.positions()
    assert pos.shape == (6, 3)
    assert np.array_equal(pos[:3], [[0.0, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0, 1.0, 2.0]]) and np.array_equal(pos[5], [2.0, 1.0, 5.0])
    assert len(g.coefficients) == 6 and g.coefficients.dtype == A.PROBE_SH_DTYPE
    c = g.grid()
    assert tuple(c.dims) == (3, 1, 2) and tuple(c.spacing) == (1.0, 1.0, 3.0) and c.pad == 0
    for bad in (dict(dims=(0, 1, 1)), dict(spacing=(1.0, 0.0, 1.0)), dict(origin=(np.nan, 0.0, 0.0)), dict(dims=(1 << 12, 1 << 12, 2))):
        kw = dict(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), dims=(2, 2, 2))
        kw.update(bad)
        with pytest.raises(ValueError):
            rtr.ProbeGrid(**kw)
    with pytest.raises(ValueError):
        rtr.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2), coefficients=np.zeros(3, dtype=A.PROBE_SH_DTYPE))
