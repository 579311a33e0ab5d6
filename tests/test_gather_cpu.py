"""Hemisphere gathers (include/rtr_hip.h: rtr_gather_*) without a GPU: the declarations and record layouts, the host-only
rtr_gather_ray against the numpy restatement of the contract (tests/_gather_ref.py) bit for bit, the sampler's distribution,
the reduction order, and -- from the pinned CPU oracle -- that the inputs of the GPU tests are not trivial."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gather_ref as GR
import _golden as G

A = G.A
rtr = G.rtr

NAMES = ("rtr_gather_defaults", "rtr_gather_occlusion", "rtr_gather_radiance", "rtr_gather_occlusion_device",
         "rtr_gather_radiance_device", "rtr_gather_ray")
SAMPLES = (1, 5, 64, 100)


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_header_declares_the_entries_and_the_abi_stays_4():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rtr_[a-z_0-9]+)\s*\(", text))
    lib = rtr.native.lib()
    for name in NAMES:
        assert name in declared and name in rtr.native.EXPORTS, name
        assert getattr(lib, name) is not None
    for name in ("rtr_gather_point", "rtr_gather_params", "rtr_gather_out"):
        assert re.search(r"\}\s*%s\s*;" % name, text), name
    assert re.search(r"#define\s+RTR_ABI_VERSION\s+4\b", _header())
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4


def _c_fields(name):
    """(member, C type, array length) of `typedef struct name { ... } name;` in the header"""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for m in rest.split(","):
            m = m.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", m)
            out.append((arr.group(1), ctype, int(arr.group(2))) if arr else (m, ctype, 1))
    return out


CTYPES = {"double": (C.c_double, "<f8"), "int32_t": (C.c_int32, "<i4"), "uint32_t": (C.c_uint32, "<u4")}


def test_record_layouts_equal_the_mirrors():
    for name, dtype, size in (("rtr_gather_point", A.GATHER_POINT_DTYPE, 48), ("rtr_gather_out", A.GATHER_OUT_DTYPE, 32)):
        fields = _c_fields(name)
        want = np.dtype([(m, CTYPES[t][1], (k,)) if k > 1 else (m, CTYPES[t][1]) for m, t, k in fields])
        assert want == dtype and dtype.itemsize == size, name
    fields = _c_fields("rtr_gather_params")
    assert [(m, CTYPES[t][0] * k if k > 1 else CTYPES[t][0]) for m, t, k in fields] == list(A.GatherParamsC._fields_)
    assert C.sizeof(A.GatherParamsC) == A.GATHER_PARAMS_SIZE == 4 * 4 + 3 * 8 + 2 * 8
    p = rtr.native.gather_defaults()
    assert (p.samples, p.seed, p.point_base, p.flags, p.time, p.t_min, p.t_max) == (64, 0, 0, 0, 0.0, 0.001, np.inf)
    assert tuple(p.reserved) == (0.0, 0.0)
    p = rtr.native.gather_defaults(samples=5, reference_order=True)
    assert (p.samples, p.flags) == (5, A.FLAG_REFERENCE_ORDER)
    with pytest.raises(TypeError):
        rtr.native.gather_defaults(spp=3)


def test_a_null_context_is_invalid():
    lib = rtr.native.lib()
    gp = rtr.native.gather_defaults()
    rp = A.make_params(16, 16, 1)
    pts = np.zeros(2, dtype=A.GATHER_POINT_DTYPE)
    pts["n"][:, 1] = 1.0
    out = np.zeros(2, dtype=A.GATHER_OUT_DTYPE)
    assert lib.rtr_gather_occlusion(None, C.byref(gp), pts.ctypes.data, out.ctypes.data, 2) == A.RTR_ERR_INVALID
    assert lib.rtr_gather_radiance(None, C.byref(rp), C.byref(gp), pts.ctypes.data, out.ctypes.data, 2) == A.RTR_ERR_INVALID
    assert lib.rtr_gather_occlusion_device(None, C.byref(gp), pts.ctypes.data, out.ctypes.data, 2, 1) == A.RTR_ERR_INVALID
    assert lib.rtr_gather_radiance_device(None, C.byref(rp), C.byref(gp), pts.ctypes.data, out.ctypes.data, 2, 1) == A.RTR_ERR_INVALID
    assert not out.view(np.uint8).any()


@pytest.mark.parametrize("samples", SAMPLES)
def test_gather_ray_equals_the_restatement(samples):
    p, n = GR.golden_points(21)
    n = n * np.linspace(0.25, 7.0, len(n))[:, None]  # normals need not be normalised
    for seed, base, time, t_max in ((7, 0, 0.0, np.inf), (0xFFFFFFF1, 0xFFFFFFE0, 0.5, 150.0)):  # (k wraps modulo 2^32)
        got = rtr.native.gather_rays(p, n, samples=samples, seed=seed, point_base=base, time=time, t_max=t_max, t_min=0.25)
        d, st = GR.rays(p, n, samples, seed, base)
        assert got.shape == (len(p), samples)
        assert np.array_equal(_bits(got["direction"]), _bits(d))
        assert np.array_equal(got["rng_state"], st) and (st != 0).all()
        assert np.array_equal(_bits(got["origin"]), _bits(np.repeat(p[:, None, :], samples, axis=1)))
        assert (got["time"] == time).all() and (got["t_min"] == 0.25).all() and (got["t_max"] == t_max).all()
        assert (got["pad"] == 0).all()


def test_gather_ray_rejects_bad_points_and_bad_params():
    lib = rtr.native.lib()
    ray = np.zeros(1, dtype=A.RAY_DTYPE)
    ray.view(np.uint8)[:] = 0xA5

    def call(gp, pt, k=0, s=0):
        return lib.rtr_gather_ray(C.byref(gp), pt.ctypes.data, k, s, ray.ctypes.data)

    good = np.zeros(1, dtype=A.GATHER_POINT_DTYPE)
    good["p"], good["n"] = (1.0, 2.0, 3.0), (0.0, 2.0, 0.0)
    gp = rtr.native.gather_defaults(samples=4)
    for field, a, value in (("p", 0, np.nan), ("p", 2, np.inf), ("n", 1, -np.inf), ("n", 0, np.nan)):
        bad = good.copy()
        bad[field][0, a] = value
        assert call(gp, bad) == A.RTR_ERR_INVALID, (field, value)
    for normal in ((0.0, 0.0, 0.0), (1e-200, 0.0, 0.0), (1e200, 1e200, 0.0)):  # sqrt(n.n) as computed: 0, 0, inf
        bad = good.copy()
        bad["n"] = normal
        assert call(gp, bad) == A.RTR_ERR_INVALID, normal
    assert call(gp, good, 0, 4) == call(gp, good, 0, -1) == call(gp, good, -1, 0) == A.RTR_ERR_INVALID
    for kw in (dict(samples=0), dict(samples=(1 << 20) + 1), dict(flags=2), dict(flags=1 | 4), dict(time=np.nan),
               dict(t_min=np.inf), dict(t_min=np.nan), dict(t_max=np.nan)):
        assert call(rtr.native.gather_defaults(**kw), good) == A.RTR_ERR_INVALID, kw
    gp = rtr.native.gather_defaults()
    gp.reserved[1] = 1.0
    assert call(gp, good) == A.RTR_ERR_INVALID
    assert lib.rtr_gather_ray(None, good.ctypes.data, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_gather_ray(C.byref(rtr.native.gather_defaults()), None, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert (ray.view(np.uint8) == 0xA5).all()  # nothing was written
    for kw in (dict(t_min=0.0), dict(t_min=-1.0), dict(t_max=-np.inf), dict(samples=1 << 20), dict(flags=1)):
        assert call(rtr.native.gather_defaults(**kw), good) == A.RTR_OK, kw
    with pytest.raises(rtr.RtrError):
        rtr.native.gather_rays(good["p"], np.zeros((1, 3)))
    with pytest.raises(rtr.RtrError):
        rtr.native.gather_rays(good["p"], good["n"], samples=0)


def test_sampler_is_cosine_distributed_about_the_normal():
    M = 100000
    normal = np.array([[0.3, -1.7, 0.9]])
    got = rtr.native.gather_rays(np.zeros((1, 3)), normal, samples=M, seed=3)
    d = got["direction"][0]
    assert np.array_equal(_bits(d), _bits(GR.rays(np.zeros((1, 3)), normal, M, 3)[0][0]))
    w = normal[0] / np.sqrt((normal[0] ** 2).sum())
    cos = d @ w
    assert cos.min() >= -1e-15
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 4 * 2.0 ** -53
    sigma = np.sqrt(1.0 / 18.0 / M)  # a cosine density: E[cos] = 2/3, Var[cos] = 1/2 - 4/9 = 1/18
    assert abs(cos.mean() - 2.0 / 3.0) <= 5 * sigma


@pytest.mark.parametrize("samples", (1, 2, 5, 63, 64, 65, 100, 300))
def test_butterfly_restatement_equals_the_scalar_loop(samples):
    rng = np.random.default_rng(samples)
    x = rng.standard_normal((3, samples, 2)) * 10.0 ** rng.integers(-3, 4, (3, samples, 2))
    x[0, ::3] = 0.0  # blocked samples add nothing
    got = GR.reduce(x)
    for k in range(3):
        for c in range(2):
            assert _bits(got[k, c]) == _bits(GR.reduce_scalar(x[k, :, c])), (k, c)
    ones = np.ones((2, samples), dtype=np.int32)
    assert (GR.reduce(ones, divide=False) == samples).all()
    g = GR.group_size(samples)
    assert g == min(64, 1 << max(samples - 1, 0).bit_length()) and g & (g - 1) == 0


@pytest.mark.parametrize("sid,t_maxes", ((21, (np.inf, 150.0)), (23, (np.inf, 1.0))))
def test_inputs_of_the_gpu_tests_are_not_trivial(sid, t_maxes):
    """Unblocked counts of the 48 points at N = 64, seed 7, from the pinned oracle: over the two t_max of a scene at least
    one point fully blocked, one fully open and ten strictly between."""
    sc = G.scene(sid)
    p, n = GR.golden_points(sid)
    zero = full = between = 0
    for t_max in t_maxes:
        d, blocked = GR.oracle_blocked(sc, p, n, 64, seed=7, t_max=t_max)
        count, v = GR.occlusion(d, blocked)
        assert np.array_equal(count, 64 - blocked.sum(axis=1))
        zero += int((count == 0).sum())
        full += int((count == 64).sum())
        between += int(((count > 0) & (count < 64)).sum())
        print("scene %d t_max %r: counts %d .. %d, %d at 0, %d at N" % (sid, t_max, count.min(), count.max(),
                                                                         (count == 0).sum(), (count == 64).sum()))
    assert zero >= 1 and full >= 1 and between >= 10, (zero, full, between)
