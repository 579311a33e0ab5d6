"""The host-only lowering (csrc/rt_lower.h: lower_scene) and the kernel-variant decisions that hang on it, without a GPU.

native.scene_plan (include/rtr_hip_test.h: rtr_test_scene_plan) runs the validator, lower_scene, pick_trav and
mega_variant on a scene and reports the facts, which references carry RT_TIE_FLAG / RT_GUARD_FLAG and the k_mega
instantiation a render would run.  Every expected value below follows from the rules written down in the comments of
rt_lower.h, rt_compile.h and rt_device.h (each test names its rule) or is one an existing test already holds; none is
output of the code under test.  Scenes are the smallest that can go wrong, built by hand with tests/_randscene.Builder."""
import numpy as np
import pytest

import _golden as G
import _randscene as R
import test_kernel_variants as KV

A = G.A
rtr = G.rtr
plan_of = rtr.native.scene_plan

TIE, GUARD = 1 << 30, 1 << 29  # RT_TIE_FLAG, RT_GUARD_FLAG (csrc/rt_device.h)
NO_BOX_MAX = 4  # RT_FAST_NO_BOX_MAX
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)  # RT_TRAV_*
BASE = G.scene(23)  # camera and empty arrays


def _builder():
    return R.Builder(np.random.default_rng(0))


def _scene(b, top, camera=None, images=None, image_bytes=None):
    root = b.hlist(top)
    return rtr.Scene(root, R._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), R._cat(b.mats, A.MATERIAL_DTYPE),
                     R._cat(b.texs, A.TEXTURE_DTYPE), BASE.perlin[:0], BASE.images[:0] if images is None else images,
                     BASE.image_bytes[:0] if image_bytes is None else image_bytes, R._cat(b.lights, A.LIGHT_DTYPE),
                     BASE.camera.copy() if camera is None else camera, np.array([0.5, 0.6, 0.8]))


def _grey(b):
    return b.material(A.MAT_LAMBERTIAN, [b.solid([0.5, 0.5, 0.5])])


def _light(b):
    b.quad_light([-2.0, 6.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])


def _tied_visits(plan):
    """visiting positions (the low bits of a reference's `reserved` word) of the references that carry RT_TIE_FLAG"""
    f = plan["ref_flags"]
    assert plan["n_tie_refs"] == int(((f & TIE) != 0).sum()) and plan["n_guard_refs"] == int(((f & GUARD) != 0).sum())
    return sorted(int(v) for v in f[(f & TIE) != 0] & ~(TIE | GUARD))


# ---- tie flags inside an instance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [True, False])
def test_coplanar_rects_of_one_instance(overlap):
    """Same plane and overlapping extents: both can tie exactly in t, both are flagged, and a scene with a tie-capable
    reference is not flat (RT_TRAV_FAST).  Disjoint extents: no ray meets both, nothing flagged, flat (RT_TRAV_FLAT)."""
    b = _builder()
    m = _grey(b)
    x0 = 0.5 if overlap else 2.0
    sc = _scene(b, [b.rect("xz", -1.0, 1.0, -1.0, 1.0, 0.0, m), b.rect("xz", x0, x0 + 2.0, -1.0, 1.0, 0.0, m)])
    p = plan_of(sc)
    assert p["fast_ok"] and p["n_refs"] == 2 and p["n_visits"] == 1 and p["n_steps"] == 1  # the default one-step program
    assert _tied_visits(p) == ([0, 1] if overlap else [])
    assert p["flat_scene"] == (not overlap) and not p["flat_guarded"]
    assert p["pick_trav"] == (FAST if overlap else FLAT)
    assert p["mega_trav"] == p["pick_trav"] and not p["mega_pair"]  # (no lights: no pair cast)


def test_concentric_spheres_of_opposite_radius_tie():
    """sphere(c, r) and sphere(c, -r) are the same surface (a glass shell's two sides): flagged by |r|.  The hollow one is
    a guarded reference of the one linearly scanned instance; a scene with ties takes the general compiled kernel."""
    b = _builder()
    m = _grey(b)
    sc = _scene(b, [b.sphere([0.0, 1.0, 0.0], 0.75, m), b.sphere([0.0, 1.0, 0.0], -0.75, m)])
    p = plan_of(sc)
    assert p["fast_ok"] and _tied_visits(p) == [0, 1] and p["n_guard_refs"] == 1
    assert (p["ref_flags"][1] & GUARD) and not (p["ref_flags"][0] & GUARD)
    assert not p["flat_scene"] and not p["flat_guarded"] and p["pick_trav"] == FAST
    other = _builder()
    sc = _scene(other, [other.sphere([0.0, 1.0, 0.0], 0.75, _grey(other)), other.sphere([0.0, 1.0, 0.0], 0.5, _grey(other))])
    assert _tied_visits(plan_of(sc)) == []


# ---- tie flags across instances (the comment above flag_ties_across_instances) ---------------------------------------
def _wall_box_floor(order, second_box=False):
    """wall, a translate(rotate_y(box)) whose bottom lies in the floor's plane y = 0, the floor; `order` names the list
    order.  Returns the scene and the visiting positions of {floor, bottom of the box, bottom of the second box}."""
    b = _builder()
    m = _grey(b)
    parts = {"wall": lambda: [b.rect("xy", -5.0, 5.0, -1.0, 4.0, -5.0, m)],
             "floor": lambda: [b.rect("xz", -5.0, 5.0, -5.0, 5.0, 0.0, m)],
             "box": lambda: [b.translate(b.rotate_y(b.box([0, 0, 0], [1, 1.5, 1], m), 20.0), [0.5, 0.0, -1.0])] +
                            ([b.translate(b.box([0, 0, 0], [1, 1, 1], m), [-3.0, 0.0, 0.5])] if second_box else [])}
    top, visit, where = [], 0, {}
    for name in order:
        nodes = parts[name]()
        top += nodes
        if name == "box":  # box.h: xy z1, xy z0, xz y1, xz y0 (the bottom: fourth side), yz x1, yz x0
            where["bottom"] = visit + 3
            if second_box:
                where["bottom2"] = visit + 6 + 3
            visit += 6 * len(nodes)
        else:
            where[name] = visit
            visit += 1
    return _scene(b, top), where


def test_cross_instance_tie_wall_box_floor():
    """[wall, box, floor]: wall and floor share the untransformed instance, which is scanned first, so the box (later
    instance) would win the tie in y = 0 although the reference visits the floor later: exactly floor and bottom are
    flagged.  [wall, floor, box]: instance order and visiting order agree, nothing is flagged."""
    sc, where = _wall_box_floor(["wall", "box", "floor"])
    p = plan_of(sc)
    assert p["fast_ok"] and p["n_refs"] == 8 and p["n_visits"] == 2
    assert _tied_visits(p) == sorted([where["bottom"], where["floor"]]) == [4, 7]
    assert not p["flat_scene"] and p["pick_trav"] == FAST
    sc, where = _wall_box_floor(["wall", "floor", "box"])
    p = plan_of(sc)
    assert _tied_visits(p) == [] and p["flat_scene"] and p["pick_trav"] == FLAT


def test_cross_instance_ties_under_a_top_tree(monkeypatch):
    """A sub-scene with a top tree meets its instances in any order: every coplanar pair across instances is flagged,
    also where list order and instance order agree.  RTR_TOP_MIN is read at every lowering."""
    sc, where = _wall_box_floor(["wall", "floor", "box"], second_box=True)
    p = plan_of(sc)
    assert not p["top_tree"] and _tied_visits(p) == [] and p["pick_trav"] == FLAT
    monkeypatch.setenv("RTR_TOP_MIN", "2")
    p = plan_of(sc)
    assert p["top_tree"] and _tied_visits(p) == sorted(where[k] for k in ("floor", "bottom", "bottom2")) == [1, 5, 11]
    assert p["pick_trav"] == FAST and p["mega_trav"] == TOP and not p["pair_cast"]
    monkeypatch.delenv("RTR_TOP_MIN")
    assert not plan_of(sc)["top_tree"]


# ---- DScene::shared_div (the comment of shared_div_allowed; rt_device.h: div_shared's range argument) --------------
def _flat_lit(b, extra=()):
    m = _grey(b)
    _light(b)
    return [b.rect("xz", -5.0, 5.0, -5.0, 5.0, 0.0, m), b.sphere([0.0, 1.0, 0.0], 0.5, m), b.sphere([2.0, 1.0, 0.0], 0.5, m)] + list(extra)


@pytest.mark.parametrize("coordinate,want", [(2.0 ** 61, 0), (2.0 ** 60, 1)])
def test_shared_div_coordinate_bound(coordinate, want):
    b = _builder()
    sc = _scene(b, _flat_lit(b, [b.sphere([coordinate, 0.0, 0.0], 1.0, _grey(b))]))
    assert plan_of(sc)["shared_div"] == want


@pytest.mark.parametrize("depth,want", [(31, 0), (30, 1)])
def test_shared_div_chain_depth(depth, want):
    b = _builder()
    node = b.sphere([0.0, 1.0, -2.0], 0.5, _grey(b))
    for _ in range(depth):
        node = b.translate(node, [0.01, 0.0, 0.0])
    p = plan_of(_scene(b, _flat_lit(b, [node])))
    assert p["fast_ok"] and p["shared_div"] == want


@pytest.mark.parametrize("span,want", [(2.0 ** -21, 0), (2.0 ** -20, 1)])
def test_shared_div_moving_sphere_time_span(span, want):
    b = _builder()
    ms = b.node(A.NODE_MOVING_SPHERE, _grey(b), f=[0.0, 1.0, -2.0, 0.0, 1.5, -2.0, 0.0, span, 0.5])
    assert plan_of(_scene(b, _flat_lit(b, [ms])))["shared_div"] == want


def test_shared_div_camera_time_and_environment(monkeypatch):
    b = _builder()
    top = _flat_lit(b)
    assert plan_of(_scene(b, top))["shared_div"] == 1
    cam = BASE.camera.copy()
    cam["time1"] = 2.0 ** 61
    assert plan_of(_scene(b, top, camera=cam))["shared_div"] == 0
    cam["time1"] = 2.0 ** 60
    assert plan_of(_scene(b, top, camera=cam))["shared_div"] == 1
    monkeypatch.setenv("RTR_NO_SHARED_DIV", "1")  # read at every lowering
    p = plan_of(_scene(b, top))
    assert p["shared_div"] == 0 and p["pair_cast"] == 0  # (the pair cast needs the shared divisions)
    monkeypatch.delenv("RTR_NO_SHARED_DIV")
    assert plan_of(_scene(b, top))["shared_div"] == 1


# ---- DScene::pair_cast (the comment of pair_cast_allowed) ------------------------------------------------------------
def test_pair_cast_needs_a_flat_lit_scene_of_packed_scans():
    b = _builder()
    sc = _scene(b, _flat_lit(b))
    p = plan_of(sc)
    assert p["flat_scene"] and p["shared_div"] and p["pair_cast"] == 1
    assert (p["pick_trav"], p["mega_trav"], p["mega_pair"]) == (FLAT, FLAT, 1)
    assert plan_of(sc, flags=A.FLAG_SPLIT_CASTS)["mega_pair"] == 0 and plan_of(sc, integrator=1)["mega_pair"] == 0  # RR: no shadow rays
    dark = _builder()
    top = _flat_lit(dark)
    dark.lights = []
    p = plan_of(_scene(dark, top))
    assert p["flat_scene"] and p["pair_cast"] == 0 and p["mega_pair"] == 0
    moving = _builder()
    p = plan_of(_scene(moving, _flat_lit(moving, [moving.moving_sphere([0.0, 1.0, -2.0], [0.0, 1.5, -2.0], 0.5, _grey(moving))])))
    assert p["flat_scene"] and p["shared_div"] and p["pair_cast"] == 0


@pytest.mark.parametrize("n_inst", [NO_BOX_MAX, NO_BOX_MAX + 1])
def test_pair_cast_instance_limit(n_inst):
    """at most RT_FAST_NO_BOX_MAX instances: beyond, the traversal tests instance boxes, which the pair walk does not"""
    b = _builder()
    m = _grey(b)
    _light(b)
    top = [b.translate(b.sphere([0.0, 1.0, 0.0], 0.4, m), [float(k), 0.0, 0.0]) for k in range(n_inst)]
    p = plan_of(_scene(b, top))
    assert p["flat_scene"] and p["n_visits"] == n_inst and p["pair_cast"] == (n_inst <= NO_BOX_MAX)


# ---- material and light class, uv_order_dependent ----------------------------------------------------------------------
def plan_class(p):
    """the class mega_variant reads off the facts: lean, QuadLights only without (u,v) reads, or everything"""
    return "lean" if p["lean_materials"] else ("quadlit" if p["quad_lights_only"] and not p["needs_uv"] else "full")


def test_material_classes():
    def scene_with(material, light="quad"):
        b = _builder()
        mat = material(b)
        if light == "quad":
            _light(b)
        else:
            b.simple_light(A.LIGHT_POINT, [1.0, 5.0, -1.0, 30.0, 28.0, 25.0])
        return _scene(b, [b.sphere([0.0, 1.0, 0.0], 0.5, mat), b.rect("xz", -5.0, 5.0, -5.0, 5.0, 0.0, _grey(b))])

    lean = plan_of(scene_with(_grey))
    assert plan_class(lean) == "lean" and lean["quad_lights_only"] and lean["n_material_types"] == 1 and lean["mega_ms"] == KV.LEAN
    quadlit = plan_of(scene_with(lambda b: b.material(A.MAT_METAL, f=[0.8, 0.8, 0.8, 0.1])))
    assert plan_class(quadlit) == "quadlit" and quadlit["n_material_types"] == 2 and quadlit["mega_ms"] == KV.QUADLIT
    full = plan_of(scene_with(_grey, light="point"))  # a point light clears quad_lights_only, and with it lean
    assert plan_class(full) == "full" and not full["quad_lights_only"] and not full["lean_materials"] and full["mega_ms"] == KV.FULL
    # a lambertian on a checker texture is not lean (the lean kernels read solid colours only); no (u,v) read: quadlit
    checker = plan_of(scene_with(lambda b: b.material(A.MAT_LAMBERTIAN, [b.checker(b.solid([0.1] * 3), b.solid([0.9] * 3))])))
    assert not checker["lean_materials"] and plan_class(checker) == "quadlit"
    assert plan_of(scene_with(_grey), integrator=1)["mega_ms"] == KV.LEAN  # RR has lean kernels too ...
    assert plan_of(scene_with(lambda b: b.material(A.MAT_METAL, f=[0.8] * 4)), integrator=1)["mega_ms"] == KV.FULL  # ... no quadlit


@pytest.mark.parametrize("image", [True, False])
def test_uv_order_dependent(image):
    """moving_sphere::hit writes no (u,v): with a material that reads them only the reference-order walk is right"""
    b = _builder()
    t = np.zeros(1, dtype=A.TEXTURE_DTYPE)
    t["type"], t["a"] = A.TEX_IMAGE, 0
    b.texs.append(t)
    tex = len(b.texs) - 1 if image else b.solid([0.5, 0.5, 0.5])
    ms = b.moving_sphere([0.0, 1.0, -2.0], [0.0, 1.5, -2.0], 0.5, b.material(A.MAT_LAMBERTIAN, [tex]))
    images = np.zeros(1, dtype=A.IMAGE_DTYPE)
    images["width"], images["height"], images["offset"] = 2, 2, 0
    sc = _scene(b, _flat_lit(b, [ms]), images=images, image_bytes=np.full(12, 128, dtype=np.uint8))
    p = plan_of(sc)
    assert p["needs_uv"] == 1  # (an image texture exists in both scenes; only who carries it differs)
    assert p["uv_order_dependent"] == image and p["pick_trav"] == (EXACT if image else FLAT)


# ---- the scenes of tests/test_kernel_variants.py ----------------------------------------------------------------------
def _mis_trav_by_name(name):
    """The k_mega traversal the variant matrix expects a MIS render of the scene to run, from what its name says it aims
    at (test_variant_scenes_are_what_they_aim_at, MEGA_TABLE): None where the name does not say."""
    if name.endswith("flat_guard"):
        return FLAT_GUARD  # one instance, linear, a guarded reference, no ties
    if name.endswith("_flat"):
        return FLAT
    if "many" in name:
        return TOP  # 200 objects: a top tree over the instances
    if "moved_media" in name or "hollow" in name:
        return PROGRAM_EXT  # media under wrappers / a guarded step: not a program of the traversal machine
    if "media" in name:
        return PROGRAM
    return None


@pytest.mark.parametrize("name", sorted(KV.SCENES))
def test_variant_scenes_get_the_kernel_they_aim_at(name):
    sc = KV._scene(name)
    p = plan_of(sc, integrator=KV.I_MIS)
    assert plan_class(p) == KV.material_class(sc) == KV.SCENES[name][1]
    assert (KV.I_MIS, p["mega_trav"], p["mega_ms"], p["mega_sorted"], p["mega_pair"]) in KV.MEGA_ROWS
    want = _mis_trav_by_name(name)
    if want is not None:
        assert p["mega_trav"] == want, (KV.TRAV_NAME[p["mega_trav"]], KV.TRAV_NAME[want])
    info = rtr.native.validate_scene(sc)
    assert p["fast_ok"] == info["fast_ok"] and p["has_media"] == info["has_media"] and p["fast_stack_words"] == info["fast_stack_words"]
    assert p["top_tree"] == (info["top_trees"] > 0 and info["fast_ok"])
    assert p["n_steps"] == (info["program_steps"] or int(info["fast_ok"])) and p["n_refs"] == info["fast_refs"]


@pytest.mark.parametrize("name", sorted(KV.PAIRED))
def test_flat_mis_scenes_with_and_without_the_pair_cast(name):
    """Every flat MIS class has a pair-cast scene and one that is not (KV.PAIRED), and each flag moves a MIS render to the
    kernel the matrix expects: FLAG_SPLIT_CASTS to the row without the pair cast, FLAG_SORTED_SHADING to the sorted row
    where there is one (QuadLights-only: sorted kernels do not pair), FLAG_STATIC_GRID to no other row."""
    sc = KV._scene(name)
    ms = {"lean": KV.LEAN, "quadlit": KV.QUADLIT, "full": KV.FULL}[KV.SCENES[name][1]]
    pair = int(KV.PAIRED[name])
    sortable = ms == KV.QUADLIT  # the one sorted row of the flat kernels: Row<MIS, RT_TRAV_FLAT, RT_MS_QUADLIT, true>
    want = {0: (0, pair), A.FLAG_STATIC_GRID: (0, pair), A.FLAG_SPLIT_CASTS: (0, 0),
            A.FLAG_SORTED_SHADING: (1, 0) if sortable else (0, pair)}
    for flags, (srt, pr) in want.items():
        p = plan_of(sc, integrator=KV.I_MIS, flags=flags)
        assert plan_class(p) == KV.SCENES[name][1] and p["pair_cast"] == pair, (name, flags)
        assert (p["mega_trav"], p["mega_ms"], p["mega_sorted"], p["mega_pair"]) == (FLAT, ms, srt, pr), (name, flags, p)
    for integ in (KV.I_PATH, KV.I_RR, KV.I_PBR, KV.I_NEE):  # only MIS casts a shadow ray and a closest-hit ray together
        assert not plan_of(sc, integrator=integ)["mega_pair"], (name, integ)
    n_moving = int((sc.nodes["type"] == A.NODE_MOVING_SPHERE).sum())
    n_inst = len(KV.instance_refs(sc))
    if pair:
        assert n_moving == 0 and n_inst <= NO_BOX_MAX, (name, n_moving, n_inst)  # (the rule of pair_cast_allowed)
    else:
        assert n_moving > 0 or n_inst > NO_BOX_MAX, (name, n_moving, n_inst)


def test_the_variant_matrix_reaches_every_megakernel_by_name(monkeypatch):
    """What tests/test_kernel_variants.py will launch on a GPU, computed here from native.scene_plan alone: every scene,
    every integrator, every flag set, one-shot and as an accumulator without and with moments (KV.planned_mega_names; the
    GPU matrix asserts per scene that exactly these ran).  The union is the whole table of 141 names, so a scene change
    that stops reaching a kernel fails here, by name, before anyone has a GPU."""
    names = set()
    for name in sorted(KV.SCENES):
        names |= KV.planned_mega_names(KV._scene(name))
    flat = len(names)
    monkeypatch.setenv("RTR_TOP_MIN", "2")  # read at every lowering: the RT_TRAV_TOP rows
    for name in KV.TOP_SCENES:
        names |= KV.planned_mega_names(KV._scene(name))
    monkeypatch.delenv("RTR_TOP_MIN")
    missing = sorted(map(KV.mega_name, KV.MEGA_TABLE - names))
    extra = sorted(map(KV.mega_name, names - KV.MEGA_TABLE))
    print("planned megakernel names: %d / %d (%d without the forced top trees)" % (len(names & KV.MEGA_TABLE), len(KV.MEGA_TABLE), flat))
    assert len(KV.MEGA_TABLE) == 141
    assert not missing and not extra, "no scene of the matrix reaches: %s; not in the table: %s" % (missing, extra)


def test_scene_plan_rejects_what_the_validator_rejects():
    b = _builder()
    sc = _scene(b, [b.sphere([0.0, 1.0, 0.0], 0.5, 7)])  # material index out of range
    with pytest.raises(rtr.RtrError) as e:
        plan_of(sc)
    assert e.value.code == A.RTR_ERR_INVALID
    with pytest.raises(rtr.RtrError):
        rtr.native.validate_scene(sc)
