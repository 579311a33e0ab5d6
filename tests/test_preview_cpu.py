"""Baked previews (include/rtr_hip.h: rtr_preview_*) without a GPU: the declarations and record layouts, the host-only
rtr_preview_ray against the numpy restatement of the contract (tests/_preview_ref.py) and Context.camera_ray's arithmetic bit
for bit, its argument checks, and the preconditions of the GPU tests (tests/test_preview.py): that the rays of the golden
scenes reach every branch of the material mapping in the stated numbers, and that under the environments the tests use both
lit and unlit surface samples occur.  The hits come from the pinned CPU oracle (rto_hits)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _golden as G
import _preview_ref as PR

rtr = G.rtr
A = rtr._abi
N = rtr.native

NAMES = ("rtr_preview_defaults", "rtr_preview_ray", "rtr_preview_samples", "rtr_preview_samples_device", "rtr_preview",
         "rtr_preview_device")
INV = A.RTR_ERR_INVALID


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _header():
    return open(os.path.join(G.ROOT, "include", "rtr_hip.h")).read()


def _body(name):
    body = re.search(r"typedef struct %s \{[^\n]*\n(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return " ".join(re.sub(r"/\*.*?\*/", "", body, flags=re.S).split())


def test_declared_exported_and_the_abi_version_stays():
    text = _header()
    lib = N.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in N.EXPORTS
        getattr(lib, name)
    assert A.RTR_ABI_VERSION == 4 and lib.rtr_abi_version() == 4
    assert re.search(r"#define RTR_ABI_VERSION 4\b", text)
    for k, name in enumerate(("MISS", "EMITTER", "SURFACE")):
        assert re.search(r"#define RTR_PREVIEW_%s %d\b" % (name, k), text)
    assert (A.PREVIEW_MISS, A.PREVIEW_EMITTER, A.PREVIEW_SURFACE) == (0, 1, 2)


def test_struct_layouts():
    assert _body("rtr_preview_params") == ("int32_t image_width, image_height; int32_t x0, y0, x1, y1; int32_t grid; int32_t flags; "
                                           "double t_min; double reserved[3];")
    assert _body("rtr_preview_sample") == "rtr_shade_query q; double direct[3]; int32_t kind, material;"
    assert C.sizeof(A.PreviewParamsC) == 64 == A.PREVIEW_PARAMS_SIZE and A.PREVIEW_SAMPLE_DTYPE.itemsize == 144
    assert [n for n, _ in A.PreviewParamsC._fields_] == ["image_width", "image_height", "x0", "y0", "x1", "y1", "grid", "flags",
                                                         "t_min", "reserved"]
    assert list(A.PREVIEW_SAMPLE_DTYPE.names) == ["q", "direct", "kind", "material"]
    assert A.PREVIEW_SAMPLE_DTYPE.fields["q"][0] == A.SHADE_QUERY_DTYPE and A.PREVIEW_SAMPLE_DTYPE.fields["direct"][1] == 112


def test_defaults():
    p = A.PreviewParamsC()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    N.lib().rtr_preview_defaults(C.byref(p))
    assert (p.image_width, p.image_height, p.x0, p.y0, p.x1, p.y1, p.grid, p.flags) == (0, 0, 0, 0, 0, 0, 1, 0)
    assert p.t_min == 0.001 and list(p.reserved) == [0.0, 0.0, 0.0]
    N.lib().rtr_preview_defaults(None)  # tolerated
    q = N.preview_params(32, 16, 3, region=(1, 2, 30, 9), t_min=0.5, reference_order=True)
    assert (q.image_width, q.image_height, q.x0, q.y0, q.x1, q.y1, q.grid, q.flags, q.t_min) == (32, 16, 1, 2, 30, 9, 3, 1, 0.5)


# ---- the ray ----

@pytest.mark.parametrize("shape", ((2, 2, 1), (2, 3, 8), (32, 32, 1), (32, 32, 2), (7, 5, 3), (16, 16, 8)))
@pytest.mark.parametrize("sid", (21, 1))
def test_ray_equals_the_restatement(sid, shape):
    """W = 2: the divisor 1; k = 8: s up to 63; scene 1 has a lens radius, which the preview ignores"""
    W, H, k = shape
    cam = G.scene(sid).camera
    p = N.preview_params(W, H, k, t_min=0.25 if k == 3 else None)
    got = N.preview_rays(cam, p)
    assert got.shape == (H, W, k * k)
    assert _same_bits(got, PR.numpy_rays(cam, W, H, k, t_min=p.t_min))
    assert (got["rng_state"] == 1).all() and (got["t_max"] == np.inf).all() and (got["time"] == cam["time0"][0]).all()
    last = np.zeros(1, dtype=A.RAY_DTYPE)
    assert N.lib().rtr_preview_ray(C.byref(N.camera_struct(cam)), C.byref(p), W - 1, H - 1, k * k - 1, last.ctypes.data) == 0
    assert _same_bits(last[0], got[H - 1, W - 1, k * k - 1])


def test_region_rays_are_the_image_rays():
    cam = G.scene(23).camera
    whole = N.preview_rays(cam, N.preview_params(32, 32, 2))
    x0, y0, x1, y1 = PR.RAGGED
    assert _same_bits(N.preview_rays(cam, N.preview_params(32, 32, 2, region=PR.RAGGED)), whole[y0:y1, x0:x1])
    assert _same_bits(PR.numpy_rays(cam, 32, 32, 2, PR.RAGGED), whole[y0:y1, x0:x1])


@pytest.mark.parametrize("sid", (21, 1, 24))
def test_grid_one_is_the_pixel_centre_ray(sid):
    """k = 1: the bits of Context.camera_ray (rtr_cli --pick), whose arithmetic is restated here without a context"""
    cam = G.scene(sid).camera
    W, H = 32, 24
    got = N.preview_rays(cam, N.preview_params(W, H, 1))
    c = cam[0]
    for i, j in ((0, 0), (31, 23), (5, 17), (16, 0)):
        u, v = (i + 0.5) / (W - 1), (j + 0.5) / (H - 1)
        d = (c["lower_left_corner"] + u * c["horizontal"] + v * c["vertical"]) - c["origin"]
        want = N.Context.make_rays(c["origin"][None, :], d[None, :], times=float(c["time0"]))
        assert _same_bits(got[j, i, 0], want[0]), (i, j)


def test_ray_checks_its_arguments():
    L = N.lib()
    cam = N.camera_struct(G.scene(21).camera)
    out = np.full(10, -7.0)

    def ray(p, i=0, j=0, s=0, cam=cam, o=out.ctypes.data):
        return L.rtr_preview_ray(C.byref(cam) if cam is not None else None, C.byref(p) if p is not None else None, i, j, s, o)

    good = N.preview_params(8, 6, 2)
    assert ray(good, 7, 5, 3) == 0
    out[:] = -7.0
    assert ray(None) == INV and ray(good, cam=None) == INV and ray(good, o=None) == INV
    for i, j, s in ((-1, 0, 0), (8, 0, 0), (0, -1, 0), (0, 6, 0), (0, 0, -1), (0, 0, 4)):
        assert ray(good, i, j, s) == INV, (i, j, s)
    for kw in (dict(image_width=1), dict(image_height=1), dict(x1=0), dict(x0=-1), dict(y1=7), dict(x1=9), dict(y0=6), dict(grid=0),
               dict(grid=9), dict(flags=2), dict(flags=3), dict(t_min=np.nan), dict(t_min=np.inf), dict(t_min=0.0),
               dict(t_min=2.0 ** -101), dict(t_min=-1.0)):
        p = N.preview_params(8, 6, 2)
        for name, value in kw.items():
            setattr(p, name, value)
        assert ray(p) == INV, kw
    for r in range(3):
        p = N.preview_params(8, 6, 2)
        p.reserved[r] = 1.0
        assert ray(p) == INV
    assert (out == -7.0).all()
    for kw in (dict(grid=8), dict(grid=1), dict(flags=1), dict(t_min=2.0 ** -100), dict(image_width=2, x1=2)):
        p = N.preview_params(8, 6, 2)
        for name, value in kw.items():
            setattr(p, name, value)
        assert ray(p) == 0, kw


def test_entries_want_a_context():
    """context first: a NULL context is RTR_ERR_INVALID whatever else is passed"""
    L = N.lib()
    p = N.preview_params(8, 6, 1)
    out = np.zeros(8 * 6 * 3)
    assert L.rtr_preview_samples(None, C.byref(p), out.ctypes.data) == INV
    assert L.rtr_preview_samples_device(None, C.byref(p), out.ctypes.data, 1) == INV
    assert L.rtr_preview(None, C.byref(p), None, out.ctypes.data, 8, None) == INV
    assert L.rtr_preview_device(None, C.byref(p), None, out.ctypes.data, 8, None, 1) == INV
    assert not out.any()


# ---- the preconditions of the GPU tests ----

@pytest.fixture(scope="module")
def oracle_samples():
    """(scene, k) -> (scene, the restated sample records of the 32 x 32 image from the oracle's hits, those hits)"""
    made = {}

    def get(sid, k):
        if (sid, k) not in made:
            sc = G.scene(sid)
            rays = PR.numpy_rays(sc.camera, 32, 32, k)
            hits = G.oracle_records(sc, "rto_hits", PR.hit_records(rays))
            made[sid, k] = (sc, PR.samples_of(sc, rays, hits)[0], hits.reshape(rays.shape))
        return made[sid, k]
    return get


@pytest.mark.parametrize("sid", PR.SCENES)
def test_the_rays_reach_every_branch_in_the_stated_numbers(oracle_samples, sid):
    sc, s, hits = oracle_samples(sid, 1)
    assert PR.counts_of(sc, s) == PR.COUNTS[sid]
    emit = s[s["kind"] == PR.EMITTER]
    if sid == 21:
        assert int(((s["kind"] == PR.SURFACE) & (hits["front_face"] == 0)).sum()) == 457  # lambertian back faces
        assert (hits["front_face"][s["kind"] == PR.EMITTER] == 1).all()
        assert (emit["direct"] > 0).any(axis=1).all()  # front faces: the emitter's colour
    if sid == 7:
        assert not emit["direct"].any()  # all back faces


def test_scene_nine_has_media_and_the_textured_scenes_are_textured():
    assert G.scene(9).has_media()
    for sid in PR.SCENES + PR.TEXTURED:
        assert not G.scene(sid).has_media()
    for sid in PR.TEXTURED:
        sc = G.scene(sid)
        assert (sc.textures["type"] != A.TEX_SOLID).any()
    assert G.scene(1).camera["lens_radius"][0] == 0.05


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("sid", PR.SCENES)
def test_lit_and_unlit_surface_samples_occur(oracle_samples, sid, k):
    """the whole expected frame from rto_hits + rtr_shade_ibl_one, under the environment with and without distance maps and
    for each selection of parts: wherever the grid is read, samples outside it or next to its invalid probe stay unlit"""
    sc, s, _ = oracle_samples(sid, k)
    surf = s["kind"] == PR.SURFACE
    for depth in (True, False):
        env = PR.environment(s["q"]["p"][surf], depth)
        for parts in (1, 2, 3):
            linear, lit = PR.frame_of(PR.IC.native_env(env, parts), s)
            _, added = PR.shade_samples(PR.IC.native_env(env, parts), s)
            added = added.reshape(s.shape)
            assert (added & surf).any(), (depth, parts)
            if parts & 1:  # (the chain alone leaves no sample of a rough surface unlit: its invalid texel is in level 0)
                assert (~added & surf).any(), (depth, parts)
            assert np.isfinite(linear).all()
            if parts == 3:  # (the diffuse term of a metal is 0: scene 24 under parts = 1)
                assert (linear[lit > 0] != 0).any()
            assert lit.min() >= 0 and lit.max() <= k * k
