"""Every kernel instantiation the launchers can pick, against the pinned CPU oracle.

csrc/rtr_mega.hip instantiates k_mega<integrator, traversal, material set, sorted, ACC, pair> and k_mega_queue, and
csrc/rt_wavefront.h wf_shade<integrator, phase, material set, sorted>; upload, the render flags and the kind of call
(one-shot render, accumulator pass, accumulator pass with moments) choose one per call.  The other render
tests cover scenes; this module covers the variants: it renders random scenes of each material palette
(tests/_randscene.py: full / quadlit / lean, and scenes of a single material type) with every integrator on both
pipelines, with and without the flags that change the kernel, one-shot and through accumulators, asks the context which
instantiation ran (Context.last_kernel: the host-side record of the test library) and compares each image with the
oracle.  The last test asserts that the union of what ran is the whole table below, by full name, so a variant that
nothing reaches any more, or a new one nobody renders, fails here instead of going unchecked.  The union lives in this
module: run it as a whole.  (tests/test_lowering_cpu.py computes the same union without a GPU, from the scenes alone.)"""
import numpy as np
import pytest

import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr

I_PATH, I_RR, I_PBR, I_NEE, I_MIS = 0, 1, 2, 3, 4  # RTR_INTEGRATOR_* (include/rtr_hip.h)
# RT_TRAV_* / RT_MS_* of csrc/rt_device.h
EXACT, MEDIA, FAST, PROGRAM, FLAT, TOP, PROGRAM_EXT, FLAT_GUARD = range(8)
LEAN, FULL, QUADLIT = 0, 1, 2
TRAV_NAME = ["EXACT", "MEDIA", "FAST", "PROGRAM", "FLAT", "TOP", "PROGRAM_EXT", "FLAT_GUARD"]
MS_NAME = ["LEAN", "FULL", "QUADLIT"]

# k_mega<integrator, traversal, material set, sorted, ACC, pair>: every Row of the instantiation lists at the end of
# csrc/rtr_mega.hip, written out as (integrator, traversal, material set, sorted, pair): 46
MEGA_ROWS = [
    # MIS (the list of rtr_mega_launch_mis): 22; the flat kernels have a pair-cast twin
    (I_MIS, FLAT, LEAN, 0, 0), (I_MIS, FLAT, LEAN, 0, 1), (I_MIS, FLAT, QUADLIT, 0, 0), (I_MIS, FLAT, QUADLIT, 0, 1),
    (I_MIS, FLAT, QUADLIT, 1, 0), (I_MIS, FLAT, FULL, 0, 0), (I_MIS, FLAT, FULL, 0, 1),
    (I_MIS, FLAT_GUARD, QUADLIT, 0, 0), (I_MIS, FLAT_GUARD, FULL, 0, 0),
    (I_MIS, FAST, LEAN, 0, 0), (I_MIS, FAST, QUADLIT, 0, 0), (I_MIS, FAST, FULL, 0, 0),
    (I_MIS, TOP, LEAN, 0, 0), (I_MIS, TOP, QUADLIT, 0, 0), (I_MIS, TOP, FULL, 0, 0),
    (I_MIS, PROGRAM_EXT, QUADLIT, 0, 0), (I_MIS, PROGRAM_EXT, FULL, 0, 0),
    (I_MIS, PROGRAM, QUADLIT, 0, 0), (I_MIS, PROGRAM, FULL, 0, 0),
    (I_MIS, MEDIA, FULL, 0, 0),
    (I_MIS, EXACT, LEAN, 0, 0), (I_MIS, EXACT, FULL, 0, 0),
    # RR (rtr_mega_launch_rr_path: no light code, so QuadLights-only scenes take the full set): 12
    (I_RR, FLAT, LEAN, 0, 0), (I_RR, FLAT, FULL, 0, 0), (I_RR, FLAT_GUARD, FULL, 0, 0),
    (I_RR, FAST, LEAN, 0, 0), (I_RR, FAST, FULL, 0, 0), (I_RR, TOP, LEAN, 0, 0), (I_RR, TOP, FULL, 0, 0),
    (I_RR, PROGRAM_EXT, FULL, 0, 0), (I_RR, PROGRAM, FULL, 0, 0), (I_RR, MEDIA, FULL, 0, 0),
    (I_RR, EXACT, LEAN, 0, 0), (I_RR, EXACT, FULL, 0, 0),
    # PATH / PBR / NEE (rtr_mega_launch_rr_path / rtr_mega_launch_pbr_nee): 4 each
    *[(i, t, FULL, 0, 0) for i in (I_PATH, I_PBR, I_NEE) for t in (FAST, TOP, PROGRAM_EXT, MEDIA)],
]
# The full name of every megakernel the library holds, (integrator, traversal, material set, sorted, pair, accum, queue):
# each row stands for k_mega<..., ACC, pair> with ACC = 0 (one-shot), 1 (accumulator pass) and 2 (with moments), and a
# pair row also for k_mega_queue<integrator, traversal, material set>, which one-shot renders run in its place unless
# FLAG_STATIC_GRID is set: 46 * 3 + 3 = 141
MEGA_TABLE = {(i, t, m, s, pr, acc, 0) for i, t, m, s, pr in MEGA_ROWS for acc in (0, 1, 2)} | \
             {(I_MIS, FLAT, m, 0, 1, 0, 1) for m in (LEAN, QUADLIT, FULL)}
assert len(MEGA_ROWS) == len(set(MEGA_ROWS)) == 46 and len(MEGA_TABLE) == 141


def mega_name(n):
    i, t, m, s, pr, acc, q = n
    if q:
        return "k_mega_queue<%d, %s, %s>" % (i, TRAV_NAME[t], MS_NAME[m])
    return "k_mega<%d, %s, %s, %s, %d, %s>" % (i, TRAV_NAME[t], MS_NAME[m], "true" if s else "false", acc, "true" if pr else "false")


# wf_shade<integrator, phase, material set, sorted>: the instantiations csrc/rt_wavefront.h (WF_SHADE) launches.  Phase
# 0 shades a whole segment; scenes with media AND lights split it into phases 1 and 2 around the shadow rays (MIS, NEE).
WF_TABLE = {
    (I_RR, 0, LEAN, 0), (I_RR, 0, FULL, 0), (I_RR, 0, FULL, 1),
    (I_PATH, 0, FULL, 0), (I_PATH, 0, FULL, 1), (I_PBR, 0, FULL, 0), (I_PBR, 0, FULL, 1),
    *[(I_NEE, ph, FULL, s) for ph in (0, 1, 2) for s in (0, 1)],
    (I_MIS, 0, LEAN, 0),
    *[(I_MIS, ph, ms, s) for ph in (0, 1, 2) for ms in (QUADLIT, FULL) for s in (0, 1)],
}
# instantiated (WF_SHADE_S compiles both sort flavours of every cell) but not reachable from any valid scene
WF_UNREACHABLE = {
    (I_RR, 0, LEAN, 1): "WavefrontPlan::sort is never set for lean scenes (rtr_render_device: plan.sort = !plan.lean && ...)",
    (I_MIS, 0, LEAN, 1): "WavefrontPlan::sort is never set for lean scenes (rtr_render_device: plan.sort = !plan.lean && ...)",
}
# (WavefrontPlan::trav, machine): the extend / connect stages -- lockstep per traversal, or the persistent machine
WF_PLAN_TABLE = {(t, m) for t in (FLAT, FAST, PROGRAM) for m in (0, 1)}

# name -> (scene factory, what it aims at).  Seeds were picked so each scene reaches its class (checked on the CPU
# below; the traversal the device compiles is checked by the coverage test at the end).
SCENES = {
    # lean: lambertian / diffuse_light, solid textures, QuadLights only
    "lean_flat": (lambda: R.random_scene(200, n_objects=6, ties=False, palette="lean"), "lean"),
    "lean_flat_guard": (lambda: R.random_scene(119, n_objects=5, ties=False, hollow=True, palette="lean"), "lean"),
    "lean_ties_lens": (lambda: R.random_scene(53, lens=0.1, palette="lean"), "lean"),
    "lean_many": (lambda: R.random_scene(54, n_objects=200, palette="lean"), "lean"),
    "lean_hollow": (lambda: R.random_scene(56, hollow=True, palette="lean"), "lean"),
    "lean_media": (lambda: R.random_scene(55, media=True, palette="lean"), "quadlit"),  # (isotropic: not lean)
    # quadlit: every material, solid textures, QuadLights only
    "quadlit_flat": (lambda: R.random_scene(204, n_objects=6, ties=False, palette="quadlit"), "quadlit"),
    "quadlit_flat_guard": (lambda: R.random_scene(119, n_objects=5, ties=False, hollow=True, palette="quadlit"), "quadlit"),
    "quadlit_ties": (lambda: R.random_scene(63, palette="quadlit"), "quadlit"),
    "quadlit_media": (lambda: R.random_scene(64, media=True, palette="quadlit"), "quadlit"),
    "quadlit_moved_media": (lambda: R.random_scene(65, moved_media=True, palette="quadlit"), "quadlit"),
    "quadlit_hollow_media": (lambda: R.random_scene(66, hollow=True, media=True, palette="quadlit"), "quadlit"),
    # full with delta lights (without them a random scene is QuadLights-only: no texture of the generator reads (u,v))
    "full_flat": (lambda: R.random_scene(71, n_objects=6, ties=False, delta_lights=True), "full"),
    "full_flat_guard": (lambda: R.random_scene(120, n_objects=5, ties=False, hollow=True, delta_lights=True), "full"),
    "full_ties": (lambda: R.random_scene(73, delta_lights=True), "full"),
    "full_media": (lambda: R.random_scene(74, media=True, delta_lights=True), "full"),
    "full_moved_media": (lambda: R.random_scene(75, moved_media=True, delta_lights=True), "full"),
    "full_hollow": (lambda: R.random_scene(76, hollow=True, delta_lights=True), "full"),
    # one material type: the wavefront shades without sorting
    "one_metal_quad": (lambda: R.single_type_scene(81, "metal", "quad"), "quadlit"),
    "one_metal_point": (lambda: R.single_type_scene(82, "metal", "point"), "full"),
    "one_fog_quad": (lambda: R.single_type_scene(83, "fog", "quad"), "quadlit"),
    "one_fog_point": (lambda: R.single_type_scene(84, "fog", "point"), "full"),
}
# Every flat MIS class has a pair-cast scene (at most four instances, no moving sphere: DScene::pair_cast) and one that
# is not: lean_flat is the lean pair scene, quadlit_flat and full_flat (six objects: more instances) are not paired.
PAIR_SCENES = {
    "quadlit_pair_flat": (lambda: R.random_scene(900, n_objects=3, ties=False, palette="quadlit"), "quadlit"),
    "full_pair_flat": (lambda: R.random_scene(900, n_objects=3, ties=False, delta_lights=True), "full"),
    "lean_moving_flat": (lambda: R.random_scene(902, n_objects=3, ties=False, palette="lean"), "lean"),  # a moving sphere
}
SCENE_ORDER = sorted(SCENES) + sorted(PAIR_SCENES)  # (positions seed the rays of the hit-record test)
SCENES.update(PAIR_SCENES)
# whether a MIS render with flags 0 runs a pair-cast kernel (checked on the CPU: tests/test_lowering_cpu.py)
PAIRED = {"lean_flat": True, "quadlit_pair_flat": True, "full_pair_flat": True,
          "lean_moving_flat": False, "quadlit_flat": False, "full_flat": False}
# media-free scenes rendered once more with a top tree forced over their instances (RT_TRAV_TOP)
TOP_SCENES = ["lean_flat", "lean_ties_lens", "quadlit_flat", "quadlit_ties", "full_flat", "full_ties", "one_metal_quad",
              "one_metal_point"]
W, H, SPP = 48, 32, 4

SEEN = {"mega": set(), "wf": set(), "plan": set(), "done": set()}  # what the render tests of this module launched


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _scene(name):
    return SCENES[name][0]()


def material_class(sc):
    """The material / light class lowering derives (csrc/rt_lower.h material_facts: lean_materials, quad_lights_only &&
    !needs_uv): the rule written out here, and checked against what the library itself reports (native.scene_plan)."""
    info = rtr.native.validate_scene(sc)
    quad_only = bool((sc.lights["type"] == A.LIGHT_QUAD).all())
    lean = quad_only and all(m["type"] in (A.MAT_LAMBERTIAN, A.MAT_DIFFUSE_LIGHT) and
                             sc.textures["type"][m["tex"][0]] == A.TEX_SOLID for m in sc.materials)
    plan = rtr.native.scene_plan(sc)
    assert (bool(plan["lean_materials"]), bool(plan["quad_lights_only"]), bool(plan["needs_uv"])) == (lean, quad_only, info["needs_uv"])
    return "lean" if lean else ("quadlit" if quad_only and not info["needs_uv"] else "full")


LINEAR_MAX = 12  # rt_compile.h kLinearMax: an instance with more references gets a box tree (no flat traversal then)


def instance_refs(sc):
    """References (primitives) per instance of the compiled scene: per chain of transforms above them."""
    counts = {}

    def walk(n, chain):
        t = sc.nodes["type"][n]
        if t in (A.NODE_SPHERE, A.NODE_MOVING_SPHERE, A.NODE_XY_RECT, A.NODE_XZ_RECT, A.NODE_YZ_RECT):
            counts[chain] = counts.get(chain, 0) + 1
        elif t == A.NODE_LIST:
            a, b = int(sc.nodes["a"][n]), int(sc.nodes["b"][n])
            for k in sc.list_children[a:a + b]:
                walk(int(k), chain)
        elif t in (A.NODE_TRANSLATE, A.NODE_ROTATE_Y):
            walk(int(sc.nodes["a"][n]), chain + (n,))
        else:
            assert t == A.NODE_FLIP_FACE, t  # (media-free scenes only)
            walk(int(sc.nodes["a"][n]), chain)

    walk(int(sc.root), ())
    return counts


def _wavefront_ok(info):
    return info["fast_ok"] or info["program_steps"] > 0


@pytest.mark.parametrize("palette", R.PALETTES)
def test_palette_scenes_reach_their_class(palette):
    """CPU: each palette's scenes are valid, hold only what the palette allows and trace on the oracle."""
    for seed, kw in [(1, {}), (2, dict(media=True)), (3, dict(hollow=True)), (4, dict(moved_media=True)), (5, dict(n_objects=90))]:
        sc = R.random_scene(seed, palette=palette, **kw)
        info = rtr.native.validate_scene(sc)
        types = set(sc.materials["type"].tolist())
        tex = set(sc.textures["type"].tolist())
        if palette != "full":
            assert (sc.lights["type"] == A.LIGHT_QUAD).all() and tex == {A.TEX_SOLID} and not info["needs_uv"], (seed, kw)
        if palette == "lean":
            assert types <= {A.MAT_LAMBERTIAN, A.MAT_DIFFUSE_LIGHT, A.MAT_ISOTROPIC}, (seed, kw)
        want = "quadlit" if palette == "lean" and info["has_media"] else palette
        if palette == "full":  # (QuadLights only and no image texture: the kernels' QuadLights-only set)
            want = "quadlit"
        assert material_class(sc) == want, (seed, kw)
        assert info["has_media"] == bool(kw.get("media") or kw.get("moved_media"))
        img, st = G.oracle_render(sc, A.make_params(24, 16, 2, integrator=4, seed=seed))
        assert np.isfinite(img).all() and img.mean() > 0
    assert material_class(R.random_scene(6, delta_lights=True)) == "full"
    with pytest.raises(ValueError):
        R.random_scene(6, delta_lights=True, palette=palette if palette != "full" else "lean")
    # a lambertian shell with a hollow inside and no transformed instance: the compiled scan with a guard (FLAT_GUARD)
    info = rtr.native.validate_scene(SCENES[palette + "_flat_guard"][0]())
    assert info["fast_ok"] and info["inverted_boxes"] == 1


@pytest.mark.parametrize("name", sorted(SCENES))
def test_variant_scenes_are_what_they_aim_at(name):
    """CPU: the class each scene of the matrix was picked for, and the traversal facts the kernels are chosen by."""
    sc = _scene(name)
    info = rtr.native.validate_scene(sc)
    assert material_class(sc) == SCENES[name][1]
    if name.endswith("flat_guard"):
        assert info["fast_ok"] and info["inverted_boxes"] == 1 and info["top_trees"] == 0
    elif name.endswith("_flat") or name.startswith("one_metal"):
        assert info["fast_ok"] and info["top_trees"] == 0 and not info["has_media"]
    if name.endswith("_flat"):
        # no box tree anywhere (and ties=False: no coplanar overlapping rects): the flat traversal.  (A scene with guarded
        # references is compiled in guard mode, which builds no box tree at any size.)
        assert max(instance_refs(sc).values()) <= LINEAR_MAX, instance_refs(sc)
    if name == "lean_many":
        assert info["top_trees"] == 1
    if "media" in name or name.startswith("one_fog"):
        assert info["has_media"] and info["program_steps"] > 0
    if name.endswith("hollow"):
        assert not info["fast_ok"] and info["program_steps"] > 0  # a guarded step: RT_TRAV_PROGRAM_EXT
    if name.startswith("one_"):
        assert len(set(sc.materials["type"].tolist())) == 1
    img, _ = G.oracle_render(sc, A.make_params(W, H, SPP, integrator=4, seed=3))
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.fixture(scope="module")
def ctx():
    c = rtr.Context(0)
    yield c
    c.close()


MEGA_FLAGS = A.FLAG_SORTED_SHADING | A.FLAG_SPLIT_CASTS | A.FLAG_STATIC_GRID  # what flags_in_effect reports of a megakernel


def mega_flag_sets(sc, integ):
    """The render flags the matrix runs the megakernel with: plain, the reference-order walk, sorted shading, and where the
    plain render is a pair cast its static grid (k_mega<..., pair> in place of k_mega_queue) and the split casts (the row
    without the pair cast)."""
    flags = [0, A.FLAG_REFERENCE_ORDER, A.FLAG_SORTED_SHADING]
    if rtr.native.scene_plan(sc, integ, 0)["mega_pair"]:
        flags += [A.FLAG_STATIC_GRID, A.FLAG_SPLIT_CASTS]
    return flags


def planned_mega_names(sc):
    """The full names _render_matrix will launch on ``sc``, from native.scene_plan alone (no GPU): every integrator with
    every flag set one-shot -- the job queue runs a pair variant unless FLAG_STATIC_GRID is set (csrc/rt_select.h:
    mega_queue) --, and every row so reached once more as an accumulator pass without and with moments."""
    names = set()
    for integ in (I_PATH, I_RR, I_PBR, I_NEE, I_MIS):
        for flags in mega_flag_sets(sc, integ):
            p = rtr.native.scene_plan(sc, integ, flags)
            row = (integ, p["mega_trav"], p["mega_ms"], p["mega_sorted"], p["mega_pair"])
            names.add(row + (0, int(bool(p["mega_pair"]) and not flags & A.FLAG_STATIC_GRID)))
            names |= {row + (1, 0), row + (2, 0)}
    return names


def _record(k, pipe, integ):
    """Enters what ran into SEEN; the full name of a megakernel, else None."""
    assert k is not None and k["pipeline"] == pipe and k["integrator"] == integ, k
    if pipe == A.PIPELINE_MEGAKERNEL:
        name = (integ, k["trav"], k["ms"], k["sorted"], k["pair"], k["accum"], k["queue"])
        assert not k["queue"] or (k["pair"] and k["accum"] == 0), k  # the queue is the one-shot twin of a pair kernel
        SEEN["mega"].add(name)
        return name
    assert k["shade_phases"] in (1, 6), k  # phase 0, or phases 1 and 2
    for ph in (0, 1, 2):
        if k["shade_phases"] >> ph & 1:
            SEEN["wf"].add((integ, ph, k["ms"], k["sorted"]))
    SEEN["plan"].add((k["trav"], k["machine"]))
    lean, quadlit = k["lean"] and integ in (I_RR, I_MIS), k["quadlit"] and integ == I_MIS
    assert k["ms"] == (LEAN if lean else (QUADLIT if quadlit else FULL)), k
    assert k["media"] == (k["trav"] == PROGRAM), k
    assert not k["pair"] and not k["queue"] and not k["accum"], k
    return None


def _lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def _sum_y2(ctx, p):
    """sum over the SPP samples of y * y of the per-sample radiance (rtr_li_samples), in sample order (tests/test_adaptive.py)"""
    jj, ii = np.mgrid[0:H, 0:W]
    q = np.zeros((H, W))
    for s in range(SPP):
        y = _lum(ctx.li_samples(p, np.stack([ii.ravel(), jj.ravel(), np.full(W * H, s)], axis=1))).reshape(H, W)
        q = q + y * y
    return q


def _accum_runs(ctx, integ, flags, row, want, wst, q_want, what):
    """The ACC = 1 and ACC = 2 twins of ``row``, which a render with ``flags`` reaches: accumulators that go to 2 and then to
    SPP samples, against the one-shot render with one chunk (bit for bit) and the oracle.  Returns the worst rel-L2."""
    p = A.make_params(W, H, SPP, integrator=integ, seed=300 + integ, pipeline=A.PIPELINE_MEGAKERNEL, flags=flags, spp_chunks=1)
    one = ctx.render(p)
    assert _record(ctx.last_kernel(), A.PIPELINE_MEGAKERNEL, integ)[:5] == row, what
    worst = 0.0
    for moments in (False, True):
        acc_name = row + (2 if moments else 1, 0)
        with ctx.accumulator(p, moments=moments) as acc:
            closest = shadow = 0
            for target in (2, SPP):
                acc.render(target)
                st = ctx.stats()
                assert ctx.last_kernel()["accum"] == acc_name[5], (what, ctx.last_kernel())
                assert _record(ctx.last_kernel(), A.PIPELINE_MEGAKERNEL, integ) == acc_name, (what, ctx.last_kernel())
                closest, shadow = closest + st["closest_segments"], shadow + st["shadow_segments"]
            got = acc.resolve()
            q = acc.moments() if moments else None
        assert np.array_equal(_bits(got), _bits(one)), (what, "accum", moments)
        err = G.rel_l2(got, want)
        worst = max(worst, err)
        assert err <= 1e-12, (what, "accum", moments, err)
        assert (closest, shadow) == (wst["closest_segments"], wst["shadow_segments"]), (what, "accum", moments)
        if moments:
            with ctx.accumulator(p, moments=True) as straight:
                straight.render(SPP)
                assert _record(ctx.last_kernel(), A.PIPELINE_MEGAKERNEL, integ) == acc_name, what
                q_straight = straight.moments()
            assert np.array_equal(_bits(q), _bits(q_straight)), (what, "moments in two passes")
            scale = max(float(np.max(np.abs(q_want))), 1e-300)
            dq = float(np.max(np.abs(q - q_want)))
            print("%s: max |Q - sum y^2| / max |Q| = %.3e" % (what, dq / scale))
            assert dq <= 1e-12 * scale, (what, "moments", dq, scale)
    return worst


def _render_matrix(ctx, name, sc, tag):
    """Every integrator on both pipelines, plain and with each flag that changes the kernel, against the oracle; then
    every megakernel row so reached as an accumulator without and with moments.  Returns the worst rel-L2 of the runs
    that have always been here, of the static-grid and split-cast runs of pair-cast scenes, and of the accumulators."""
    info = rtr.native.validate_scene(sc)
    guarded = bool(info["inverted_boxes"]) and not info["fast_ok"]
    worst = {"": 0.0, "pair": 0.0, "accum": 0.0}
    launched = set()
    M, WF = A.PIPELINE_MEGAKERNEL, A.PIPELINE_WAVEFRONT
    for integ in (I_PATH, I_RR, I_PBR, I_NEE, I_MIS):
        p0 = A.make_params(W, H, SPP, integrator=integ, seed=300 + integ)
        want, wst = G.oracle_render(sc, p0)
        mega_flags = mega_flag_sets(sc, integ)
        runs = [(M, f) for f in mega_flags[:3]]
        if _wavefront_ok(info):
            runs += [(WF, 0), (WF, A.FLAG_WF_PERSISTENT)]
        runs += [(M, f) for f in mega_flags[3:]]
        images, ran, rows = {}, {}, {}
        for pipe, flags in runs:
            p = A.make_params(W, H, SPP, integrator=integ, seed=300 + integ, pipeline=pipe, flags=flags)
            what = "%s.i%d.pipe%d.flags%d" % (tag, integ, pipe, flags)
            if flags == A.FLAG_WF_PERSISTENT and (guarded or "moved_media" in name):
                # the machine runs no guarded steps and no media under transforms: it refuses (test_random_scenes)
                with pytest.raises(rtr.RtrError) as e:
                    ctx.render(p)
                assert e.value.code == A.RTR_ERR_UNSUPPORTED, what
                continue
            got = ctx.render(p)
            st = ctx.stats()
            k = ctx.last_kernel()
            full = _record(k, pipe, integ)
            assert st["closest_segments"] == wst["closest_segments"] and st["shadow_segments"] == wst["shadow_segments"], what
            err = G.rel_l2(got, want)
            key = "pair" if pipe == M and flags in (A.FLAG_STATIC_GRID, A.FLAG_SPLIT_CASTS) else ""
            worst[key] = max(worst[key], err)
            assert err <= 1e-12, (what, err)  # same paths (segment counts equal); libm last bits only
            images[(pipe, flags)] = got
            if pipe == M:
                # flags_in_effect: each flag exactly where it changed the kernel
                k0 = ran.setdefault(0, k)  # (the plain run comes first)
                effect = (A.FLAG_SORTED_SHADING if k["sorted"] else 0) | \
                         (A.FLAG_SPLIT_CASTS if flags & A.FLAG_SPLIT_CASTS and k0["pair"] and not k["pair"] else 0) | \
                         (A.FLAG_STATIC_GRID if flags & A.FLAG_STATIC_GRID and k["pair"] and not k["queue"] else 0)
                assert st["flags_in_effect"] & MEGA_FLAGS == effect, (what, st["flags_in_effect"], k)
                ran[flags] = k
                rows.setdefault(full[:5], flags)
                launched.add(full)
        # variants that differ only in the order of the work compute the same numbers
        assert np.array_equal(_bits(images[(M, A.FLAG_SORTED_SHADING)]), _bits(images[(M, 0)])), (tag, integ, "sorted")
        if (WF, A.FLAG_WF_PERSISTENT) in images:
            assert np.array_equal(_bits(images[(WF, A.FLAG_WF_PERSISTENT)]), _bits(images[(WF, 0)])), (tag, integ, "machine")
        if SCENES[name][1] == "lean":
            # the lean kernels against the kernels with every material's code (reference order: RT_MS_LEAN; guarded and
            # program scenes: the QuadLights-only / full sets) -- one scene, one set of numbers
            assert np.array_equal(_bits(images[(M, A.FLAG_REFERENCE_ORDER)]), _bits(images[(M, 0)])), (tag, integ, "lean")
        if len(mega_flags) > 3:
            # a pair-cast scene: the job queue (plain), the pair kernel on the static grid and the two single casts
            assert ran[0]["pair"] and ran[0]["queue"], (tag, ran[0])
            assert ran[A.FLAG_STATIC_GRID]["pair"] and not ran[A.FLAG_STATIC_GRID]["queue"], (tag, ran[A.FLAG_STATIC_GRID])
            assert not ran[A.FLAG_SPLIT_CASTS]["pair"] and not ran[A.FLAG_SPLIT_CASTS]["queue"], (tag, ran[A.FLAG_SPLIT_CASTS])
            for f in (A.FLAG_STATIC_GRID, A.FLAG_SPLIT_CASTS):
                assert all(ran[f][x] == ran[0][x] for x in ("trav", "ms", "sorted")), (tag, f, ran[f])
                assert np.array_equal(_bits(images[(M, f)]), _bits(images[(M, 0)])), (tag, integ, "flags %d" % f)
        else:
            assert not any(k["pair"] or k["queue"] for k in ran.values()), (tag, integ, ran)
        q_want = {}
        for row, flags in rows.items():
            ref = flags & A.FLAG_REFERENCE_ORDER
            if ref not in q_want:
                q_want[ref] = _sum_y2(ctx, A.make_params(W, H, SPP, integrator=integ, seed=300 + integ, flags=ref))
            what = "%s.i%d.accum.flags%d" % (tag, integ, flags)
            worst["accum"] = max(worst["accum"], _accum_runs(ctx, integ, flags, row, want, wst, q_want[ref], what))
            launched |= {row + (1, 0), row + (2, 0)}
    # what the library's plan says of the scene (checked against the whole table on the CPU) is what ran
    planned = planned_mega_names(sc)
    assert launched == planned, (tag, sorted(map(mega_name, launched ^ planned)))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_variant_hit_records_equal_the_oracle(ctx, name):
    """Hit records of each palette's scenes, both traversals: bit-exact t / p / n on surfaces, allclose in media."""
    sc = _scene(name)
    ctx.upload(sc)
    rays = R.random_rays(500 + SCENE_ORDER.index(name), 4000)
    ora = G.oracle_records(sc, "rto_hits", rays)
    h = ora["hit"] == 1
    fog = h & np.isin(ora["material"], np.flatnonzero(sc.materials["type"] == A.MAT_ISOTROPIC))
    surf = h & ~fog
    for exact_order in (False, True):
        ctx.reference_order(exact_order)
        dev = ctx.test_records("hits", rays)
        ctx.reference_order(False)
        tag = (name, exact_order)
        assert np.array_equal(dev["hit"], ora["hit"]) and np.array_equal(dev["rng_out"], ora["rng_out"]), tag
        for f in ("front_face", "material"):
            assert np.array_equal(dev[f][h], ora[f][h]), (tag, f)
        for f in ("t", "p", "n"):
            assert np.array_equal(_bits(dev[f][surf]), _bits(ora[f][surf])), (tag, f)
            assert np.allclose(dev[f][fog], ora[f][fog], rtol=1e-13, atol=1e-13), (tag, f, "medium")  # OCML log


def _residues(key, worst, paired):
    """the runs that have always been under ``key`` keep it; the static-grid / split-cast runs and the accumulators have
    keys of their own"""
    G.residue(key + ".worst_rel_l2", worst[""], 1e-12)
    if paired:
        G.residue(key + ".pair.worst_rel_l2", worst["pair"], 1e-12)
    G.residue(key + ".accum.worst_rel_l2", worst["accum"], 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_variant_renders_equal_the_oracle(ctx, name):
    sc = _scene(name)
    ctx.upload(sc)
    worst = _render_matrix(ctx, name, sc, name)
    _residues("variants.%s" % name, worst, name in PAIRED and PAIRED[name])
    SEEN["done"].add(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TOP_SCENES)
def test_variant_renders_with_a_top_tree_equal_the_oracle(ctx, monkeypatch, name):
    """RTR_TOP_MIN=2 (read at every upload): the same scenes through the per-lane instance walk (RT_TRAV_TOP)."""
    monkeypatch.setenv("RTR_TOP_MIN", "2")
    sc = _scene(name)
    ctx.upload(sc)
    worst = _render_matrix(ctx, name, sc, name + ".top")
    _residues("variants.%s.top" % name, worst, False)
    SEEN["done"].add(name + ".top")


@pytest.mark.gpu
def test_every_kernel_variant_ran_and_was_compared():
    """The union of what the render tests above launched is the whole table: every megakernel instantiation by its full
    name (accumulator twins, pair-cast twins and job-queue kernels included), every reachable wf_shade cell and every extend / connect form of the wavefront."""
    missing = sorted((set(SCENES) | {n + ".top" for n in TOP_SCENES}) - SEEN["done"])
    assert not missing, "render tests of this module did not run or did not pass: %s" % missing
    assert not set(WF_UNREACHABLE) & WF_TABLE
    mega_missing = sorted(map(mega_name, MEGA_TABLE - SEEN["mega"]))
    mega_extra = sorted(map(mega_name, SEEN["mega"] - MEGA_TABLE))
    wf_missing = sorted((i, ph, MS_NAME[m], s) for i, ph, m, s in WF_TABLE - SEEN["wf"])
    wf_extra = sorted((i, ph, MS_NAME[m], s) for i, ph, m, s in SEEN["wf"] - WF_TABLE)
    print("kernel variants: %d / %d megakernel names, %d / %d wf_shade (+ %d unreachable, listed), %d / %d wavefront plans" %
          (len(SEEN["mega"] & MEGA_TABLE), len(MEGA_TABLE), len(SEEN["wf"] & WF_TABLE), len(WF_TABLE), len(WF_UNREACHABLE),
           len(SEEN["plan"] & WF_PLAN_TABLE), len(WF_PLAN_TABLE)))
    assert len(MEGA_TABLE) == 141
    assert not mega_missing and not mega_extra, "megakernels not launched: %s; launched but not in the table: %s" % (mega_missing, mega_extra)
    assert not wf_missing and not wf_extra, ("wf_shade", wf_missing, wf_extra)
    assert SEEN["plan"] == WF_PLAN_TABLE, ("wavefront plans", sorted(WF_PLAN_TABLE - SEEN["plan"]))
