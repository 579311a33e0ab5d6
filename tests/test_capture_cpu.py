"""Environment captures (include/rtr_hip.h: rtr_capture_*, rtr_cube_*, rtr_latlong_direction, rtr_write_rgbe) without a GPU:
the declarations and record layouts, and the host-only rtr_capture_ray, rtr_cube_lookup_one, rtr_latlong_direction,
rtr_cube_to_latlong and rtr_write_rgbe against the numpy restatement of the contract (tests/_capture_ref.py) bit for bit.
A written file goes through the host layer's own RGBE reader, the one its EnvironmentLight uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _capture_ref as CR
import _golden as G

rtr = G.rtr
A = rtr._abi

NAMES = ("rtr_capture_defaults", "rtr_capture_cube", "rtr_capture_cube_device", "rtr_capture_ray", "rtr_cube_lookup",
         "rtr_cube_lookup_device", "rtr_cube_lookup_one", "rtr_latlong_direction", "rtr_cube_to_latlong", "rtr_write_rgbe")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def test_declared_exported_and_the_abi_version_stays():
    text = _header()
    lib = rtr.native.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in rtr.native.EXPORTS
        getattr(lib, name)
    assert "rtr_test_last_capture" in rtr.native.TEST_EXPORTS
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert re.search(r"#define RTR_ABI_VERSION 4\b", text)


def test_struct_layout_and_defaults():
    body = re.search(r"typedef struct rtr_capture_params \{[^\n]*\n(.*?)\} rtr_capture_params;", _header(), re.S).group(1)
    body = " ".join(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split())
    assert body == "int32_t face_size, samples; uint32_t seed, point_base; int32_t jitter, pad; double time; double reserved[2];"
    assert C.sizeof(A.CaptureParamsC) == 48 == A.CAPTURE_PARAMS_SIZE
    assert [n for n, _ in A.CaptureParamsC._fields_] == ["face_size", "samples", "seed", "point_base", "jitter", "pad", "time",
                                                         "reserved"]
    p = rtr.native.capture_defaults()
    assert (p.face_size, p.samples, p.seed, p.point_base, p.jitter, p.pad, p.time) == (32, 16, 0, 0, 1, 0, 0.0)
    assert tuple(p.reserved) == (0.0, 0.0)
    with pytest.raises(TypeError):
        rtr.native.capture_defaults(flags=1)


def test_parameter_checks_run_before_any_device_work():
    """Without a context every entry returns RTR_ERR_INVALID: nothing of the device is touched on the way."""
    lib = rtr.native.lib()
    cp, rp = rtr.native.capture_defaults(face_size=2, samples=1), A.make_params(2, 2, 1)
    pts = rtr.native.probe_points(np.zeros((2, 3)))
    out = np.zeros(2 * 24, dtype=A.GATHER_OUT_DTYPE)
    inv = A.RTR_ERR_INVALID
    assert lib.rtr_capture_cube(None, C.byref(rp), C.byref(cp), pts.ctypes.data, out.ctypes.data, 2) == inv
    assert lib.rtr_capture_cube_device(None, C.byref(rp), C.byref(cp), pts.ctypes.data, out.ctypes.data, 2, 1) == inv
    assert lib.rtr_cube_lookup(None, 2, out.ctypes.data, pts.ctypes.data, out.ctypes.data, 2) == inv
    assert lib.rtr_cube_lookup_device(None, 2, out.ctypes.data, pts.ctypes.data, out.ctypes.data, 2, 1) == inv
    lib.rtr_capture_defaults(None)  # tolerated


CENTRE = np.array([[278.0, 273.5, -100.25], [1.0, 2.0, 3.0], [-5.5, 0.0, 1e3]])


@pytest.mark.parametrize("jitter", (0, 1))
@pytest.mark.parametrize("S", (1, 3, 8))
def test_capture_ray_equals_the_restatement(S, jitter):
    """Every texel of all six faces -- corners and centres included --, samples 0 .. 4, a non-zero point_base: direction and
    left-over state bit for bit, origin, time and the query defaults of t_min / t_max."""
    samples, seed, base = 5, 0x9E3779B9, 0xFFFFFFFE  # the second and third centres wrap modulo 2^32
    got = rtr.native.capture_rays(CENTRE, face_size=S, samples=samples, seed=seed, point_base=base, jitter=jitter, time=0.25)
    d, st = CR.rays(len(CENTRE), S, samples, seed, base, jitter)
    assert got.shape == (3, 6, S, S, samples)
    assert np.array_equal(_bits(got["direction"]), _bits(d))
    assert np.array_equal(got["rng_state"], st)
    assert np.array_equal(got["origin"], np.broadcast_to(CENTRE[:, None, None, None, None, :], got["origin"].shape))
    assert (got["time"] == 0.25).all() and (got["t_min"] == 0.001).all() and np.isinf(got["t_max"]).all()
    length = np.sqrt((got["direction"] ** 2).sum(-1))
    assert np.abs(length - 1.0).max() < 4e-16
    if not jitter:  # nothing is drawn: every sample of a texel has the same direction, other states
        assert (got["direction"] == got["direction"][..., :1, :]).all()
        assert len(np.unique(got["rng_state"])) == got["rng_state"].size
        if S % 2:  # the centre texel of an odd face looks down the axis
            axis = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
            assert np.array_equal(got["direction"][0, :, S // 2, S // 2, 0], axis)


def test_capture_ray_face_table_orientation():
    """Independent of the restatement's table: with S = 2 and no jitter the texel (a, b) of every face lies in the octant the
    usual cube-map table gives (u to the right, v downwards as seen from the centre)."""
    r = rtr.native.capture_rays(np.zeros((1, 3)), face_size=2, samples=1, jitter=0)["direction"][0, :, :, :, 0]
    for b in range(2):
        for a in range(2):
            u, v = (-1, 1)[a], (-1, 1)[b]
            want = [(1, -v, -u), (-1, -v, u), (u, 1, v), (u, -1, -v), (u, -v, 1), (-u, -v, -1)]
            for f in range(6):
                assert np.array_equal(np.sign(r[f, b, a]), np.array(want[f], dtype=np.float64)), (f, a, b)
                assert np.argmax(np.abs(r[f, b, a])) == f // 2


def test_capture_ray_rejects_bad_centres_and_bad_params():
    lib = rtr.native.lib()
    ray = np.zeros(1, dtype=A.RAY_DTYPE)
    good = rtr.native.probe_points(np.zeros((1, 3)))

    def call(cp, pt=good, k=0, f=0, a=0, b=0, s=0):
        return lib.rtr_capture_ray(C.byref(cp), pt.ctypes.data, k, f, a, b, s, ray.ctypes.data)

    ok = rtr.native.capture_defaults(face_size=3, samples=2)
    assert call(ok) == A.RTR_OK and call(ok, f=5, a=2, b=2, s=1) == A.RTR_OK
    for kw in (dict(k=-1), dict(f=-1), dict(f=6), dict(a=3), dict(a=-1), dict(b=3), dict(s=2), dict(s=-1)):
        assert call(ok, **kw) == A.RTR_ERR_INVALID, kw
    for value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad["p"][0, 1] = value
        assert call(ok, pt=bad) == A.RTR_ERR_INVALID
    for field, value in (("face_size", 0), ("face_size", 4097), ("samples", 0), ("samples", (1 << 20) + 1), ("jitter", 2),
                         ("jitter", -1), ("time", np.nan), ("time", np.inf)):
        cp = rtr.native.capture_defaults(face_size=3, samples=2)
        setattr(cp, field, value)
        assert call(cp) == A.RTR_ERR_INVALID, field
    for field in ("pad", "reserved"):
        cp = rtr.native.capture_defaults(face_size=3, samples=2)
        if field == "pad":
            cp.pad = 1
        else:
            cp.reserved[1] = 1.0
        assert call(cp) == A.RTR_ERR_INVALID, field
    assert lib.rtr_capture_ray(None, good.ctypes.data, 0, 0, 0, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_capture_ray(C.byref(ok), None, 0, 0, 0, 0, 0, ray.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_capture_ray(C.byref(ok), good.ctypes.data, 0, 0, 0, 0, 0, None) == A.RTR_ERR_INVALID
    ok4096 = rtr.native.capture_defaults(face_size=4096, samples=1)  # the largest face: its last texel's index fits
    assert call(ok4096, f=5, a=4095, b=4095) == A.RTR_OK
    with pytest.raises(rtr.RtrError):
        rtr.native.capture_ray([0.0, np.nan, 0.0], 0, 0, 0)


def _cube(S, seed=3):
    rng = np.random.default_rng(seed)
    t = np.zeros((6, S, S), dtype=A.GATHER_OUT_DTYPE)
    t["v"] = rng.uniform(0.05, 4.0, (6, S, S, 3))
    t["count"], t["valid"] = 16, 1
    return t


def _texel_centre(S, f, a, b):
    """the unnormalised direction of the header's table through the centre of texel (a, b): exact for S a power of two"""
    u, v = (2.0 * (a + 0.5)) / S - 1.0, (2.0 * (b + 0.5)) / S - 1.0
    return ((1, -v, -u), (-1, -v, u), (u, 1, v), (u, -1, -v), (u, -v, 1), (-u, -v, -1))[f]


def lookup_cases():
    """(name, texels [6, S, S], directions [n, 3]) of the lookup cases both the host form and the kernel (tests/
    test_capture.py) are held to"""
    rng = np.random.default_rng(11)
    cases = []
    for S in (1, 2, 3, 8):
        cases.append(("random directions, S = %d" % S, _cube(S), rng.standard_normal((200, 3)) * 10.0 ** rng.integers(-3, 4, (200, 1))))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    cases.append(("the six axes", _cube(4), np.concatenate([axes, 3.5 * axes, -0.0 + axes])))
    ties = [(sx * 1.0, sy * 1.0, 0.25) for sx in (1, -1) for sy in (1, -1)]          # |x| = |y| > |z|: x
    ties += [(0.25, sy * 2.0, sz * 2.0) for sy in (1, -1) for sz in (1, -1)]         # |y| = |z| > |x|: y
    ties += [(sx * 1.0, 0.5, sz * 1.0) for sx in (1, -1) for sz in (1, -1)]          # |x| = |z| > |y|: x
    ties += [(sx * 3.0, sy * 3.0, sz * 3.0) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]  # all equal: x
    cases.append(("ties", _cube(4), np.array(ties)))
    cases.append(("ties, S = 1", _cube(1), np.array(ties)))
    for S in (2, 8):
        centres = np.array([_texel_centre(S, f, a, b) for f in range(6) for b in range(S) for a in range(S)], dtype=np.float64)
        cases.append(("texel centres, S = %d" % S, _cube(S), centres))
    edges = []
    for f in range(6):  # on and next to the face's edges: the coordinates clamp, no other face is read
        for u, v in ((1.0, 0.3), (-1.0, -0.2), (0.4, 1.0), (0.1, -1.0), (0.999, 0.999), (-0.999, 0.97), (0.9, -0.999)):
            edges.append(((1, -v, -u), (-1, -v, u), (u, 1, v), (u, -1, -v), (u, -v, 1), (-u, -v, -1))[f])
    cases.append(("face edges", _cube(4), np.array(edges, dtype=np.float64)))
    bad = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [np.nan, 1.0, 0.0], [1.0, np.inf, 0.0], [0.0, 1.0, -np.inf],
                    [1e200, 1e200, 0.0], [1e-200, 0.0, 0.0], [5e-324, 0.0, 0.0],  # x*x + y*y + z*z overflows / is 0
                    [1e150, 1.0, 1.0], [1e-150, -1e-151, 0.0]])
    cases.append(("zero, NaN, inf, overflow and underflow of the length", _cube(3), bad))
    holed = _cube(4)
    holed["valid"][2, 1, 2] = 0
    holed["v"][2, 1, 2] = np.nan  # an invalid texel's value never becomes a result
    around = np.array([_texel_centre(4, 2, a, b) for b in range(4) for a in range(4)], dtype=np.float64)
    around = np.concatenate([around, around + np.array([0.11, 0.0, 0.07]), rng.standard_normal((100, 3))])
    cases.append(("one invalid texel", holed, around))
    return cases


@pytest.mark.parametrize("case", lookup_cases(), ids=lambda c: c[0])
def test_cube_lookup_one_equals_the_restatement(case):
    name, texels, dirs = case
    got = rtr.native.cube_lookup_host(texels, dirs)
    want = CR.lookup(texels, dirs)
    assert _same_bits(got, want), name
    S = texels.shape[1]
    if name.startswith("texel centres"):  # exactly that texel's bits, one texel used
        assert _same_bits(got["v"], texels["v"].reshape(-1, 3)) and (got["count"] == 1).all() and (got["valid"] == 1).all()
    if name.startswith("ties"):
        faces = [CR.face_uv(d)[0] for d in dirs]
        assert faces == [0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1]  # the sign of the winning axis, outermost
    if name.startswith("zero"):
        assert (got["valid"][:8] == 0).all() and (got["count"][:8] == 0).all() and (got["v"][:8] == 0).all()
        assert (got["valid"][8:] == 1).all()
    if name == "one invalid texel":
        assert got["valid"][6] == 0 and 0 < (got["valid"] == 0).sum() < len(dirs) // 2
        assert np.isfinite(got["v"]).all()
    if name == "face edges":
        assert (got["valid"] == 1).all() and (got["count"] <= 4).all() and (got["count"] >= 1).all()
    if S == 1:
        assert (got["count"][got["valid"] == 1] == 1).all()


def test_cube_lookup_one_rejects_bad_arguments():
    lib = rtr.native.lib()
    t, q, out = _cube(2), rtr.native.probe_points(np.ones((1, 3))), np.zeros(1, dtype=A.GATHER_OUT_DTYPE)
    assert lib.rtr_cube_lookup_one(2, t.ctypes.data, q.ctypes.data, out.ctypes.data) == A.RTR_OK
    for S in (0, -1, 4097):
        assert lib.rtr_cube_lookup_one(S, t.ctypes.data, q.ctypes.data, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_lookup_one(2, None, q.ctypes.data, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_lookup_one(2, t.ctypes.data, None, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_lookup_one(2, t.ctypes.data, q.ctypes.data, None) == A.RTR_ERR_INVALID
    with pytest.raises(ValueError):
        rtr.native.cube_lookup_host(np.zeros(23, dtype=A.GATHER_OUT_DTYPE), np.ones((1, 3)))


@pytest.mark.parametrize("W,H", ((8, 4), (7, 5), (1, 1), (64, 32)))
def test_latlong_direction_equals_numpy(W, H):
    for j in range(H):
        for i in range(W):
            got = rtr.native.latlong_direction(W, H, i, j)
            assert np.abs(got - CR.latlong_direction(W, H, i, j)).max() <= 1e-15, (i, j)
    d = np.zeros(3)
    lib = rtr.native.lib()
    for args in ((0, 4, 0, 0), (8, 0, 0, 0), (8, 4, 8, 0), (8, 4, 0, 4), (8, 4, -1, 0), (8, 4, 0, -1)):
        assert lib.rtr_latlong_direction(*args, d.ctypes.data) == A.RTR_ERR_INVALID, args
    assert lib.rtr_latlong_direction(8, 4, 0, 0, None) == A.RTR_ERR_INVALID
    top, mid = rtr.native.latlong_direction(64, 32, 0, 0), rtr.native.latlong_direction(65, 33, 32, 16)
    assert top[1] > 0.99 and np.abs(mid - np.array([1.0, 0.0, 0.0])).max() < 1e-15  # row 0 is up, the middle looks down +x


def test_cube_to_latlong_is_the_lookup_over_the_latlong_directions():
    holed = _cube(4)
    holed["valid"][4, 0, 0] = 0
    for texels, (W, H) in ((_cube(8), (16, 8)), (_cube(3), (9, 5)), (_cube(1), (4, 2)), (holed, (32, 16))):
        got = rtr.native.cube_to_latlong(texels, W, H)
        dirs = np.array([rtr.native.latlong_direction(W, H, i, j) for j in range(H) for i in range(W)])
        want = rtr.native.cube_lookup_host(texels, dirs)["v"].reshape(H, W, 3)
        assert got.shape == (H, W, 3) and np.array_equal(_bits(got), _bits(want))
    assert (got == 0).all(-1).any()  # the invalid texel's corner: zero, not NaN
    out = np.zeros((2, 4, 3))
    lib = rtr.native.lib()
    t = _cube(2)
    assert lib.rtr_cube_to_latlong(2, t.ctypes.data, 0, 2, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_to_latlong(0, t.ctypes.data, 4, 2, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_to_latlong(2, None, 4, 2, out.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_cube_to_latlong(2, t.ctypes.data, 4, 2, None) == A.RTR_ERR_INVALID


def _rgbe_image():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (6, 9, 3)) * 10.0 ** rng.integers(-6, 7, (6, 9, 1))
    img[0, 0] = 0.0
    img[0, 1] = (-1.0, 0.5, np.nan)        # negative and NaN count as 0
    img[0, 2] = (-3.0, -0.0, np.nan)       # all of them: a zero texel
    img[0, 3] = (9e-33, 1e-40, 0.0)        # below 1e-32
    img[0, 4] = (1e-32, 1e-33, 1e-36)      # at the threshold
    img[0, 5] = (1.0, 0.5, 0.25)           # powers of two: f = 0.5
    img[0, 6] = (255.0 / 256.0, 1.0 - 2.0 ** -53, 1e-3)
    img[0, 7] = (65504.0, 1.0, 1e-9)
    img[0, 8] = (np.nextafter(2.0, 0.0), 2.0 ** -20, 1.999)
    img[1, 0] = (1e30, 3e37, 1e38)         # near the top of the float range
    return img


def test_write_rgbe_bytes_and_decoding(tmp_path):
    img = _rgbe_image()
    path = str(tmp_path / "a.hdr")
    rtr.native.write_rgbe(path, img)
    data = open(path, "rb").read()
    assert data == CR.rgbe_bytes(img)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 6 +X 9\n"
    assert data.startswith(head) and len(data) == len(head) + 6 * 9 * 4
    q = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(6, 9, 4)
    for i in (0, 2, 3):
        assert (q[0, i] == 0).all(), i
    assert q[0, 1, 0] == 0 and q[0, 1, 2] == 0 and q[0, 1, 1] == 128 and q[0, 4, 3] != 0
    assert tuple(q[0, 5]) == (128, 64, 32, 129)
    dec = CR.rgbe_decode(data)
    clean = np.where(img > 0.0, img, 0.0)  # NaN and negative: 0
    step = np.where(q[..., 3] == 0, 0.0, 2.0 ** (q[..., 3].astype(np.float64) - 136.0))[..., None]
    assert (dec <= clean).all()
    written = q[..., 3] != 0
    assert (clean - dec < step)[written].all()
    assert (clean[~written] < 1e-32).all()
    assert (q[..., :3].max(-1)[written] >= 128).all()  # the largest channel's mantissa is normalised
    lib = rtr.native.lib()
    assert lib.rtr_write_rgbe(None, 9, 6, img.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_write_rgbe(path.encode(), 0, 6, img.ctypes.data) == A.RTR_ERR_INVALID
    assert lib.rtr_write_rgbe(path.encode(), 9, 6, None) == A.RTR_ERR_INVALID
    assert lib.rtr_write_rgbe(str(tmp_path / "no" / "dir.hdr").encode(), 9, 6, img.ctypes.data) == A.RTR_ERR_DEVICE
    with pytest.raises(ValueError):
        rtr.native.write_rgbe(path, np.zeros((4, 4)))


def test_a_written_file_reads_back_through_the_environment_lights_reader(tmp_path):
    """host/rtr_scene_api.h: EnvironmentLight reads the file with the layer's own RGBE reader; the texels it keeps are the
    float32 of mantissa * 2^(e - 136), the decode of the written bytes."""
    img = _rgbe_image()
    img[0, 0] = (2.0, 2.0, 1.5)
    path = str(tmp_path / "env.hdr")
    rtr.native.write_rgbe(path, img)
    got = rtr.hostscene.read_hdr(path)
    want = CR.rgbe_decode(open(path, "rb").read())
    assert got.dtype == np.float32 and got.shape == (6, 9, 3)
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(np.float64), want)
    cube = rtr.renderer.Cubemap(_cube(8))
    path2 = str(tmp_path / "cube.hdr")
    cube.save_hdr(path2, 16, 8)
    back = rtr.hostscene.read_hdr(path2).astype(np.float64)
    lat = cube.to_latlong(16, 8)
    assert back.shape == (8, 16, 3) and (back <= lat).all() and ((lat - back) / lat.max(-1, keepdims=True) < 2.0 ** -7).all()
    with pytest.raises(OSError):
        rtr.hostscene.read_hdr(str(tmp_path / "missing.hdr"))


def test_cubemap_class():
    t = _cube(4)
    cube = rtr.renderer.Cubemap(t.reshape(-1).reshape(6, 4, 4))
    assert cube.face_size == 4 and cube.radiance.shape == (6, 4, 4, 3)
    d = np.random.default_rng(2).standard_normal((32, 3))
    assert np.array_equal(_bits(cube.lookup(d)), _bits(CR.lookup(t, d)["v"]))
    assert np.array_equal(_bits(cube.to_latlong(8, 4)), _bits(rtr.native.cube_to_latlong(t, 8, 4)))
    with pytest.raises(ValueError):
        rtr.renderer.Cubemap(np.zeros((6, 4, 3), dtype=A.GATHER_OUT_DTYPE))
