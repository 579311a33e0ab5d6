"""Pins the CPU oracle (oracle/rt_oracle.cpp) against the golden vectors that
oracle/gen_golden.py produced by running the UNMODIFIED reference (oracle/_ref/ref_harness).

The reference ships no tests, so these vectors are the only pins of the path.
Everything here is bit-exact: the oracle restates the reference operation by operation in
IEEE double, g++ without FMA contraction, and glibc libm on both sides.
"""
import numpy as np
import pytest

import _golden as G

A = G.A


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_rng_known_answers():
    """core/rtweekend.h:24-50 and the samplers of core/vec3.h:226-269, g++ argument order."""
    gold = np.fromfile(G.os.path.join(G.GOLD, "rng.bin"), dtype="<f8").reshape(4, A.RNG_BLOCK_DOUBLES)
    lib = G.oracle()
    for row in gold:
        out = np.zeros(A.RNG_BLOCK_DOUBLES)
        n = lib.rto_rng_block(int(row[0]), out.ctypes.data)
        assert n == A.RNG_BLOCK_DOUBLES
        assert np.array_equal(_bits(out), _bits(row))


def test_sample_seed_never_zero():
    lib = G.oracle()
    seen = set()
    for i in range(0, 64, 7):
        for j in range(0, 64, 5):
            for s in range(3):
                v = lib.rto_sample_seed(1, 64, i, j, s)
                assert v != 0
                seen.add(v)
    assert len(seen) > 250  # distinct streams


@pytest.mark.parametrize("sid", [21, 23, 9, 4, 1, 8, 35])
def test_closest_hit_vectors(sid):
    """hittable::hit on whole scenes: BVH order, wrappers, primitives, media RNG."""
    sc = G.scene(sid)
    gold = G.records("hits_scene%02d.bin" % sid, A.HIT_DTYPE)
    out = G.oracle_records(sc, "rto_hits", gold)
    assert np.array_equal(out["hit"], gold["hit"])
    assert 0.2 < gold["hit"].mean() <= 1.0
    assert np.array_equal(out["rng_out"], gold["rng_out"])
    h = gold["hit"] == 1
    for f in ("front_face", "material"):
        assert np.array_equal(out[f][h], gold[f][h]), f
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(out[f][h]), _bits(gold[f][h])), f
    # u,v: only where the reference sets them (moving_sphere / constant_medium leave them unset)
    uv = h & ~np.isnan(gold["u"])
    assert uv.sum() > 0
    for f in ("u", "v"):
        assert np.array_equal(_bits(out[f][uv]), _bits(gold[f][uv])), f
        assert np.all(np.isnan(out[f][h & ~uv]))
    if sid in (9, 8):  # media consumed RNG inside traversal
        assert np.any(gold["rng_in"] != gold["rng_out"])


@pytest.mark.parametrize("sid", [23, 9, 35, 1011])
def test_material_vectors(sid):
    """material::sample / eval / pdf / emitted (materials/material.h), textures, perlin."""
    sc = G.scene(sid)
    gold = G.records("materials_scene%02d.bin" % sid, A.MAT_DTYPE)
    out = G.oracle_records(sc, "rto_materials", gold)
    if sid == 1011:  # the roughness x metallic grid of SURVEY 8c item 4
        pbr = sc.materials[sc.materials["type"] == A.MAT_PBR]
        rough = sc.textures["f"][pbr["tex"][:, 1], 0]
        metal = sc.textures["f"][pbr["tex"][:, 2], 0]
        assert sorted(set(rough.tolist())) == [0.01, 0.05, 0.2, 0.4, 1.0] and sorted(set(metal.tolist())) == [0.0, 0.5, 1.0]
        assert len(pbr) == 15
    for f in ("sample_ok", "rng_out", "is_transmission"):
        assert np.array_equal(out[f], gold[f]), f
    for f in ("eval", "pdf", "emitted"):
        assert np.array_equal(_bits(out[f]), _bits(gold[f])), f
    # the reference leaves `sampled` untouched for materials without sample(); where it writes, compare
    types = sc.materials["type"][gold["material"]]
    writes = np.isin(types, [A.MAT_LAMBERTIAN, A.MAT_METAL, A.MAT_DIELECTRIC])
    ok = writes | ((types == A.MAT_PBR) & (gold["sample_ok"] == 1))
    for f in ("s_wi", "s_f", "s_pdf"):
        assert np.array_equal(_bits(out[f][ok]), _bits(gold[f][ok])), f
    assert np.array_equal(out["is_specular"][ok], gold["is_specular"][ok])
    if sid == 1011:
        assert set(np.unique(types)) >= {A.MAT_LAMBERTIAN, A.MAT_METAL, A.MAT_DIELECTRIC, A.MAT_DIFFUSE_LIGHT, A.MAT_PBR}
    elif sid == 35:  # PBRMaterial with image albedo / roughness / metallic and NORMAL maps (material.h:247-261)
        pbr = sc.materials[sc.materials["type"] == A.MAT_PBR]
        assert len(pbr) == 3 and np.all(pbr["tex"][:, 3] >= 0)
        assert np.all(sc.textures["type"][pbr["tex"][:, 3]] == A.TEX_IMAGE) and np.all(sc.textures["a"][pbr["tex"][:, 3]] >= 0)
        assert ((types == A.MAT_PBR) & (gold["sample_ok"] == 1)).sum() > 20
    else:
        assert set(np.unique(types)) >= ({A.MAT_LAMBERTIAN, A.MAT_DIELECTRIC, A.MAT_DIFFUSE_LIGHT})


@pytest.mark.parametrize("sid", [21, 23, 15, 17, 18, 19, 24, 26])
def test_light_vectors(sid):
    """QuadLight / PointLight / DirectionalLight / SpotLight sample() and pdf() (lighting/*.h)."""
    sc = G.scene(sid)
    gold = G.records("lights_scene%02d.bin" % sid, A.LIGHTREC_DTYPE)
    out = G.oracle_records(sc, "rto_lights", gold)
    for f in ("Li", "wi", "pdf", "dist", "pdf_dir"):
        assert np.array_equal(_bits(out[f]), _bits(gold[f])), f
    assert np.array_equal(out["is_delta"], gold["is_delta"])
    if sid in (21, 23):
        assert (gold["pdf"] > 0).any() and (gold["pdf"] == 0).any()
    elif sid == 19:  # map-less EnvironmentLight: uniform sphere
        assert not gold["is_delta"].any() and np.all(gold["pdf"] == 1.0 / (4.0 * np.pi)) and np.all(np.isinf(gold["dist"]))
    elif sid in (24, 26):  # EnvironmentLight with a (synthetic) HDR map: 24 equirectangular, 26 angular probe
        assert sc.lights["type"][0] == A.LIGHT_ENV_MAP and sc.lights["f"][0][2] == (1.0 if sid == 26 else 0.0)
        assert not gold["is_delta"].any() and np.all(np.isinf(gold["dist"]))
        assert (gold["pdf"] > 0).mean() > 0.5 and len(np.unique(gold["pdf"])) > 20  # importance sampled, not uniform
        if sid == 26:
            assert (gold["pdf"] == 0).any()  # texels outside the probe's disc
    else:
        assert gold["is_delta"].all() and (gold["pdf_dir"] == 0).all()


LI_CASES = [(7, 1), (7, 4), (21, 4), (23, 4), (9, 1), (22, 4), (7, 0), (23, 2), (21, 3), (23, 3),
            (15, 4), (17, 4), (18, 4), (18, 3), (4, 1), (19, 4), (19, 3), (1, 1), (8, 1),
            (24, 4), (24, 3), (26, 4), (26, 3), (35, 4)]


@pytest.mark.parametrize("sid,integ", LI_CASES)
def test_li_records(sid, integ):
    """Integrator::Li per camera sample: radiance, RNG state at exit (draw count), segment counts."""
    name = "li_scene%02d_i%d.bin" % (sid, integ)
    info = G.MANIFEST["files"][name]
    sc = G.scene(sid)
    gold = G.records(name, A.LI_DTYPE)
    p = A.make_params(info["info"]["width"], info["info"]["height"], info["spp"], integrator=integ,
                      seed=info["seed"])
    out = G.oracle_records(sc, "rto_li", gold, params=p)
    assert np.array_equal(out["rng_exit"], gold["rng_exit"])
    if sid in (17, 19, 24, 26):
        # a directional light (and the environment light: dist = inf)'s shadow ray has t_max = inf - 0.001 = inf, which the harness's
        # counting wrapper (finite t_max = shadow ray) files under "closest": compare the total
        assert np.array_equal(out["n_closest"] + out["n_shadow"], gold["n_closest"] + gold["n_shadow"])
    else:
        assert np.array_equal(out["n_closest"], gold["n_closest"])
        assert np.array_equal(out["n_shadow"], gold["n_shadow"])
    assert np.array_equal(_bits(out["L"]), _bits(gold["L"]))
    assert gold["n_closest"].max() > (1 if sid == 4 else 3 if sid == 35 else 4)


IMG_CASES = ["img_scene07_i1_64_spp16.f64", "img_scene07_i4_64_spp16.f64", "img_scene21_i4_64_spp16.f64",
             "img_scene23_i4_64_spp16.f64", "img_scene09_i1_64_spp16.f64", "img_scene22_i4_64_spp16.f64",
             "img_scene21_i4_128_spp32.f64", "img_scene07_i0_48_spp8.f64", "img_scene23_i2_64_spp16.f64",
             "img_scene21_i3_64_spp16.f64", "img_scene23_i3_64_spp16.f64", "img_scene15_i4_64_spp16.f64",
             "img_scene17_i4_64_spp16.f64", "img_scene18_i4_64_spp16.f64", "img_scene18_i3_64_spp16.f64",
             "img_scene04_i1_64_spp16.f64", "img_scene19_i4_64_spp16.f64", "img_scene19_i3_64_spp16.f64", "img_scene01_i1_64_spp16.f64",
             "img_scene08_i1_64_spp16.f64", "img_scene24_i4_64_spp16.f64", "img_scene24_i3_64_spp16.f64",
             "img_scene26_i4_64_spp16.f64", "img_scene26_i3_64_spp16.f64", "img_scene35_i4_64_spp16.f64"]


@pytest.mark.parametrize("name", IMG_CASES)
def test_images(name):
    """Whole tile-threaded render (renderer/renderer.h:40-94) == reference, bit for bit."""
    img, info = G.image(name)
    sc = G.scene(info["scene"])
    p = A.make_params(info["width"], info["height"], info["spp"], integrator=info["integrator"], seed=info["seed"])
    out, stats = G.oracle_render(sc, p, threads=4)
    assert stats["samples"] == info["width"] * info["height"] * info["spp"]
    if info["scene"] in (17, 19, 24, 26):  # see test_li_records
        assert stats["closest_segments"] + stats["shadow_segments"] == \
            info["info"]["closest_segments"] + info["info"]["shadow_segments"]
    else:
        assert stats["closest_segments"] == info["info"]["closest_segments"]
        assert stats["shadow_segments"] == info["info"]["shadow_segments"]
    assert np.array_equal(_bits(out), _bits(img))
    assert G.rel_l2(out, img) == 0.0


PRIMITIVE_SCENES = {1001: "sphere", 1002: "moving_sphere", 1003: "xy_rect", 1004: "xz_rect", 1005: "yz_rect", 1006: "box",
                    1007: "translate(rotate_y(box))", 1008: "flip_face(xz_rect)", 1009: "constant_medium(sphere)",
                    1010: "constant_medium(translate(rotate_y(box)))"}


@pytest.mark.parametrize("sid", sorted(PRIMITIVE_SCENES))
def test_primitive_hit_vectors(sid):
    """hit() of every geometry class on its own (one object = the whole world, built by the
    reference's constructors): 256 rays each, incl. the RNG state a constant_medium leaves behind."""
    sc = G.scene(sid)
    gold = G.records("hits_scene%d.bin" % sid, A.HIT_DTYPE)
    out = G.oracle_records(sc, "rto_hits", gold)
    assert np.array_equal(out["hit"], gold["hit"]) and 0.15 < gold["hit"].mean() < 1.0
    assert np.array_equal(out["rng_out"], gold["rng_out"])
    h = gold["hit"] == 1
    for f in ("front_face", "material"):
        assert np.array_equal(out[f][h], gold[f][h]), f
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(out[f][h]), _bits(gold[f][h])), f
    uv = h & ~np.isnan(gold["u"])
    for f in ("u", "v"):
        assert np.array_equal(_bits(out[f][uv]), _bits(gold[f][uv])), f
    if sid in (1002, 1009, 1010):  # moving_sphere and constant_medium write no (u,v)
        assert not uv.any()
    if sid in (1009, 1010):
        assert np.any(gold["rng_in"] != gold["rng_out"])


@pytest.mark.parametrize("sid", [1012, 1013])
def test_exact_ties_in_t_resolve_like_the_reference(sid):
    """Harness scenes 1012 / 1013: coplanar overlapping rects with different materials, a box face in the plane of
    a rect, the same sphere twice -- as a hittable_list and under a bvh_node.  Every hit() of the reference
    accepts t == t_max, so the object its walk visits later wins; `material` in the reference's vectors tells which."""
    sc = G.scene(sid)
    gold = G.records("hits_scene%d.bin" % sid, A.HIT_DTYPE)
    out = G.oracle_records(sc, "rto_hits", gold)
    h = gold["hit"] == 1
    assert np.array_equal(out["hit"], gold["hit"]) and h.sum() > 800
    for f in ("front_face", "material"):
        assert np.array_equal(out[f][h], gold[f][h]), f
    for f in ("t", "p", "n"):
        assert np.array_equal(_bits(out[f][h]), _bits(gold[f][h])), f
    # the vectors do contain ties: visiting the list backwards changes the winner of some rays
    if sid == 1012:
        root = sc.nodes[sc.root]
        lc = sc.list_children.copy()
        lc[root["a"]:root["a"] + root["b"]] = lc[root["a"]:root["a"] + root["b"]][::-1]
        rev = G.rtr.Scene(sc.root, sc.nodes, lc, sc.materials, sc.textures, sc.perlin, sc.images, sc.image_bytes,
                          sc.lights, sc.camera, sc.background)
        other = G.oracle_records(rev, "rto_hits", gold)
        assert np.array_equal(other["hit"], gold["hit"])
        assert 100 < int((other["material"][h] != gold["material"][h]).sum())
        assert np.array_equal(_bits(other["t"][h]), _bits(gold["t"][h]))  # same t, another winner


ALL_OTHER_SCENES = [2, 5, 6, 10, 11, 12, 13, 14, 16, 20, 25, 27, 28, 30, 31, 32, 33, 34, 36, 37, 38, 39, 40, 41, 42]


@pytest.mark.parametrize("sid", ALL_OTHER_SCENES)
def test_every_other_reference_scene(sid):
    """Breadth: each remaining scene id of select_scene (scenes.cpp:1523-2096), flattened and rendered
    small by the reference (MIS integrator): the oracle reproduces the image bit for bit."""
    img, info = G.image("img_scene%02d_i4_32_spp4.f64" % sid)
    sc = G.scene(sid)
    p = A.make_params(info["width"], info["height"], info["spp"], integrator=4, seed=info["seed"])
    out, stats = G.oracle_render(sc, p, threads=4)
    assert stats["closest_segments"] + stats["shadow_segments"] == \
        info["info"]["closest_segments"] + info["info"]["shadow_segments"]
    assert np.array_equal(_bits(out), _bits(img))


def test_image_texture_fixture_really_has_texels():
    """scene 4 was flattened with a loaded image (not the cyan missing-file fallback)."""
    sc = G.scene(4)
    assert len(sc.images) == 1 and sc.images["width"][0] == 96 and len(sc.image_bytes) == 96 * 48 * 3
    img, _ = G.image("img_scene04_i1_64_spp16.f64")
    centre = img[10:26, 24:40]
    assert centre[..., 0].std() > 0.01  # a textured globe, not a flat colour


def test_scene07_integrator4_is_nearly_black():
    """the literal BASELINE config (scene07 + MIS) only sees the light's back face."""
    dark, _ = G.image("img_scene07_i4_64_spp16.f64")
    lit, _ = G.image("img_scene21_i4_64_spp16.f64")
    assert dark.mean() < 0.05 * lit.mean()


def test_tile_sharding_partitions_the_image():
    """tile_first/tile_stride own disjoint 16x16 tiles whose union is the whole image."""
    sc = G.scene(21)
    full, _ = G.oracle_render(sc, A.make_params(40, 40, 2), threads=2)
    acc = np.zeros_like(full)
    cover = np.zeros(full.shape[:2], dtype=int)
    for r in range(3):
        p = A.make_params(40, 40, 2, tile_first=r, tile_stride=3)
        part = np.full((40, 40, 3), np.nan)
        lib = G.oracle()
        d = sc.desc()
        assert lib.rto_render(G.C.byref(d), G.C.byref(p), part.ctypes.data, 40, 1, None) == 0
        own = ~np.isnan(part[..., 0])
        cover += own
        acc[own] = part[own]
    assert np.all(cover == 1)
    assert np.array_equal(acc, full)


def test_region_matches_full_image():
    sc = G.scene(23)
    full, _ = G.oracle_render(sc, A.make_params(48, 27, 3), threads=2)
    sub, _ = G.oracle_render(sc, A.make_params(48, 27, 3, region=(5, 3, 37, 20)), threads=2)
    assert np.array_equal(sub, full[3:20, 5:37])


# ---- vectors built ON the decisions of the shading functions (oracle/ref_harness.cpp: materials-edge, scatter,
# scatter-edge, lights-edge, pow5; oracle/gen_golden.py --add-shading-edges) ---------------------------------------
import _shading_edges as E  # noqa: E402


def _assert_same(out, gold, fields, mask=None):
    for f in fields:
        a, b = (out[f], gold[f]) if mask is None else (out[f][mask], gold[f][mask])
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        assert np.all(E.same(a, b)), f


@pytest.mark.parametrize("sid", E.MATERIAL_EDGE_SCENES)
def test_material_edge_vectors(sid):
    """material::sample / eval / pdf / emitted on constructed records: NaN operands (wi = -wo, zero vectors), dot
    products of +0, -0 and one step either side, the dielectric's critical angle and reflectance draw, near_zero,
    the frame thresholds, the ends of the texture coordinates.  Every output field the reference writes, bit for
    bit, a NaN equal to a NaN."""
    sc = G.scene(sid)
    gold = G.records(E.material_edge_name(sid), A.MAT_DTYPE)
    out = G.oracle_records(sc, "rto_materials", gold)
    for f in ("sample_ok", "rng_out", "is_transmission", "pad"):
        assert np.array_equal(out[f], gold[f]), f
    _assert_same(out, gold, ("eval", "pdf", "emitted"))
    ok = E.sample_written(sc, gold)
    _assert_same(out, gold, ("s_wi", "s_f", "s_pdf"), ok)
    assert np.array_equal(out["is_specular"][ok], gold["is_specular"][ok])


@pytest.mark.parametrize("name", sorted(E.SCATTER_FILES))
def test_scatter_vectors(name):
    """The legacy material::scatter of integrators 0 and 1 (material.h:103-112, :133-140, :176-193,
    constant_medium.h:19-24), random and constructed records: return value, generator state, scattered direction and
    attenuation where the class writes them; every other output is zero on both sides."""
    sc = G.scene(E.SCATTER_FILES[name])
    gold = G.records(name, A.MAT_DTYPE)
    out = G.oracle_records(sc, "rto_scatter", gold)
    for f in ("sample_ok", "rng_out", "is_specular", "is_transmission", "pad"):
        assert np.array_equal(out[f], gold[f]), f
    _assert_same(out, gold, ("s_wi", "s_f"), E.scatter_written(sc, gold))
    _assert_same(out, gold, ("s_pdf", "eval", "pdf", "emitted"))
    types = E.material_types(sc, gold)
    assert (gold["sample_ok"] == 1).any() and (gold["sample_ok"] == 0).any()
    assert (gold["sample_ok"][types == A.MAT_METAL] == 0).any()  # a reflection below the surface
    assert set(np.unique(types)) >= {A.MAT_LAMBERTIAN, A.MAT_METAL, A.MAT_DIELECTRIC, A.MAT_DIFFUSE_LIGHT, A.MAT_ISOTROPIC}


@pytest.mark.parametrize("sid", E.LIGHT_EDGE_SCENES)
def test_light_edge_vectors(sid):
    """Light::sample / pdf on constructed records (the plane of a QuadLight, its edges and corners, the spot cone, the
    positions of the delta lights, the cdf entries, the seam and the poles of the environment maps)."""
    sc = G.scene(sid)
    gold = G.records(E.light_edge_name(sid), A.LIGHTREC_DTYPE)
    out = G.oracle_records(sc, "rto_lights", gold)
    _assert_same(out, gold, E.LIGHT_FLOAT_FIELDS)
    assert np.array_equal(out["is_delta"], gold["is_delta"])


def test_shading_edge_fixtures_hit_what_they_aim_at():
    """Every named case of every *-edge fixture holds at least one record for which the harness found the case's condition
    true (with the reference's own expressions), and the reference's outputs show the branches taken."""
    for name in E.edge_files():
        cases = G.MANIFEST["files"][name]["info"]["cases"]
        assert len(cases) >= 1
        for case, count in cases.items():
            assert count >= 1, (name, case)
    sc = G.scene(E.EDGE_SCENE)
    gold = G.records(E.material_edge_name(E.EDGE_SCENE), A.MAT_DTYPE)
    types = E.material_types(sc, gold)
    straddle = E.dielectric_straddle(sc, gold, scatter=False)
    assert straddle.sum() >= 32 and set(gold["is_transmission"][straddle].tolist()) == {0, 1}
    lam = types == A.MAT_LAMBERTIAN
    assert (E.bits(gold["s_wi"][lam]) == E.bits(gold["n"][lam])).all(axis=1).any()  # near_zero fired: wi = unit(n) = n
    assert ((gold["pdf"] == 0) & np.signbit(gold["pdf"])).any()  # cosine = -0.0 passes `cosine < 0`
    assert np.isnan(gold["eval"]).any() and np.isnan(gold["pdf"]).any()
    sgold = G.records("scatter_edge_scene1014.bin", A.MAT_DTYPE)
    sstraddle = E.dielectric_straddle(sc, sgold, scatter=True)
    assert sstraddle.sum() >= 32
    lights = {sid: (G.scene(sid), G.records(E.light_edge_name(sid), A.LIGHTREC_DTYPE)) for sid in E.LIGHT_EDGE_SCENES}
    assert any(np.isnan(g["wi"]).any() for _, g in lights.values())
    assert any(np.isnan(g["pdf_dir"]).any() for _, g in lights.values())
    sc21, g21 = lights[21]
    edge = E.quad_alpha_beta_edge(sc21, g21)
    assert edge.sum() >= 8 and (g21["pdf_dir"][edge] == 0).any() and (g21["pdf_dir"][edge] > 0).any()
    sc18, g18 = lights[18]
    cone = E.spot_straddle(sc18, g18)
    li = g18["Li"][cone].sum(axis=1)
    assert cone.sum() >= 16 and (li == 0).any() and (li > 0).any()
    assert np.isinf(lights[15][1]["Li"]).any()  # a point light at its own position


def test_shading_edge_fixtures_are_small_data_files():
    names = E.edge_files() + list(E.SCATTER_FILES) + ["scene1014.rtrs"] + E.POW5_FILES
    for name in names:
        info = G.MANIFEST["files"][name]
        assert info["bytes"] == G.os.path.getsize(G.os.path.join(G.GOLD, name))
        assert info["bytes"] <= 160 * 1024 and info["argv"] and len(info["sha256"]) == 64


def test_pow5_host_is_within_one_ulp_of_glibc_pow():
    """rt_device.h: pow5 (x^5 in double-double arithmetic) against glibc's pow(x, 5.0) as the reference's harness computed it
    on 65 536 values: never more than one ulp apart, and the number of values that differ at all is the count
    oracle/gen_golden.py measured and wrote into the manifest -- fixed arithmetic, so a count and not a bound."""
    xy, committed = E.pow5_pairs()
    assert len(xy) == 65536 and (xy[:, 0] == 0).any() and (xy[:, 0] == 1).any() and (xy[:, 0] == 2.0 ** -215).any()
    got = G.rtr.native.pow5_host(xy[:, 0])
    want = np.ascontiguousarray(xy[:, 1])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want)) and np.all(got >= 0) and np.all(want >= 0)
    d = got.view(np.int64) - want.view(np.int64)  # same sign, finite: the distance in ulps
    print("pow5: %d of %d differ, largest distance %d ulp" % ((d != 0).sum(), len(d), np.abs(d).max()))
    assert np.abs(d).max() <= 1
    assert int((d != 0).sum()) == committed
