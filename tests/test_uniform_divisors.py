"""Divisions by numbers that are the same for a whole scene or launch (csrc/rt_device.h: udiv, div_pi, SceneConsts; the
image size in k_mega_queue's prologue): the quotient must be the bits of the reference's n / d wherever it is used.

  * udiv beside the compiler's division over the numerators its call sites can see, for the divisors of the scene tables
    of scenes 21 and 23, pi and image sizes;
  * the scene table against a second evaluation of its expressions, and its replacement by the next upload;
  * light_pdf on the corner and the edges of a quad light, where the numerator of alpha or beta is +-0 or a step beside
    it, and on lights whose edge has length 0 or a length below udiv's range (the plain division);
  * small renders against the CPU oracle, bit for bit: odd image sizes, and scenes of 1, 2, 3 and 7 quad lights (1 / n
    is no power of two).

Images of 1 x 8 and 8 x 1 pixels are left out of the renders: the library refuses an image below 2 x 2 (params_check), so
W - 1 = 0 never reaches a kernel; test_one_pixel_wide_images_are_refused pins that, and udiv's fallback for a zero divisor
is exercised by the division test and by the light with a zero-length edge."""
import numpy as np
import pytest

import _flatscenes as F
import _golden as G
import _randscene as R
import _shading_edges as E

A = G.A
N = G.rtr.native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(rtr):
    c = rtr.Context(0)
    yield c
    c.close()


def _len2(v):
    """len2 of csrc/rt_device.h: x * x + y * y + z * z, left to right, no contraction"""
    v = np.asarray(v, dtype=np.float64)
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def lit_scene(n_lights):
    """a room (one sphere), three grey spheres and n_lights emitting rectangles under the ceiling, each with its QuadLight"""
    b = R.Builder(np.random.default_rng(0))
    top = [b.sphere([0.0, 0.0, 0.0], 14.0, F._grey(b, 0.8))]
    for k, (c, r) in enumerate((([-2.0, 0.5, 0.0], 1.0), ([1.5, 0.2, 1.0], 0.8), ([0.0, -1.0, -2.5], 1.3))):
        top.append(b.sphere(c, r, F._grey(b, 0.3 + 0.2 * k)))
    emit = b.material(A.MAT_DIFFUSE_LIGHT, [b.solid([7.0, 7.0, 7.0])])
    for k in range(n_lights):
        x0, x1, z0, z1, y = -6.0 + 1.7 * k, -6.0 + 1.7 * k + 1.2 + 0.05 * k, -3.0 + 0.1 * k, -1.5, 6.0
        top.append(b.flip_face(b.rect("xz", x0, x1, z0, z1, y, emit)))
        b.quad_light([x0, y, z0], [x1 - x0, 0.0, 0.0], [0.0, 0.0, z1 - z0], [7.0, 7.0, 7.0])
    return F._scene(b, top)


def degenerate_light_scene():
    """lights: 0 an ordinary quad; 1 with U = 0 (len2(U) = 0: alpha = n / 0); 2 with |U|^2 = 1e-120, below udiv's range;
    3 with a non-finite edge.  The normals are given, not derived: a zero edge has no cross product to normalise."""
    b = R.Builder(np.random.default_rng(0))
    top = [b.sphere([0.0, 0.0, 0.0], 14.0, F._grey(b, 0.8))]
    b.quad_light([-1.0, 6.0, -1.0], [2.0, 0.0, 0.0], [0.0, 0.0, 1.5], [7.0, 7.0, 7.0])
    down = [0.0, -1.0, 0.0]
    b.simple_light(A.LIGHT_QUAD, [2.0, 6.0, -1.0] + [0.0, 0.0, 0.0] + [0.0, 0.0, 1.5] + [5.0, 5.0, 5.0] + down + [1.0])
    b.simple_light(A.LIGHT_QUAD, [-4.0, 6.0, -1.0] + [1e-60, 0.0, 0.0] + [0.0, 0.0, 1.5] + [5.0, 5.0, 5.0] + down + [1.5e-60])
    b.simple_light(A.LIGHT_QUAD, [4.0, 6.0, -1.0] + [np.inf, 0.0, 0.0] + [0.0, 0.0, 1.5] + [5.0, 5.0, 5.0] + down + [1.0])
    return F._scene(b, top)


# ---- the division itself ---------------------------------------------------------------------------------------------------
def _numerators():
    rng = np.random.default_rng(18)
    tiny = [0.0, 2.0 ** -301, 2.0 ** -300, np.nextafter(2.0 ** -300, 0.0), np.nextafter(2.0 ** -300, 1.0), 5e-324, 2.0 ** -1074,
            2.0 ** -1060, 2.0 ** -1023, np.nextafter(2.0 ** -1022, 0.0), 2.0 ** -1022, 2.0 ** -600, 2.0 ** -299]
    huge = [2.0 ** 199, 2.0 ** 200, np.nextafter(2.0 ** 200, np.inf), 2.0 ** 201, 2.0 ** 900, 1.7e308, np.inf, np.nan]
    special = np.array(tiny + huge)
    parts = [special, -special]
    parts.append(rng.uniform(-1000.0, 1000.0, 40000))                                  # dot(planar, U)
    parts.append(rng.uniform(0.0, 1.0, 20000))                                          # cosines
    parts.append(np.ldexp(rng.uniform(0.5, 1.0, 20000), rng.integers(-320, 210, 20000)) * rng.choice([-1.0, 1.0], 20000))
    parts.append(np.ldexp(rng.uniform(0.5, 1.0, 4000), rng.integers(-1074, -1000, 4000)))  # denormals
    i = rng.integers(0, 65535, 40000).astype(np.float64)
    parts.append(i + rng.integers(0, 2 ** 32, 40000) * 2.3283064365386963e-10)         # i + rng_next: the camera's
    parts.append(np.arange(0.0, 1024.0))                                                # i + 0
    num = np.concatenate(parts)
    # udiv's guard is a vote of the wave: one numerator outside [2^-300, 2^200] sends its 64 lanes to the plain
    # division.  Both kinds of wave are wanted: the numerators in range first, in waves of their own (at most one
    # mixed), then the others, which also carry lanes in range through the plain division
    a = np.abs(num)
    in_range = (a >= 2.0 ** -300) & (a <= 2.0 ** 200)
    mixed = num[~in_range]
    mixed = np.concatenate([mixed, num[in_range][:len(mixed)]])
    return np.concatenate([num[in_range], rng.permutation(mixed)])


def test_udiv_is_the_plain_division(ctx):
    divisors = []
    for sid in (21, 23):
        ctx.upload(G.scene(sid))
        table, _ = ctx.scene_consts()
        assert len(table["lights"]) >= 1
        divisors += [table["lights"][:, 0], table["lights"][:, 2]]
    divisors.append(np.array([np.pi, 1.0, 2.0, 3.0, 799.0, 65534.0]))
    # divisors that are not `safe` take the plain division whole: an edge of length 0, sizes outside [2^-100, 2^100]
    divisors.append(np.array([0.0, -0.0, 2.0 ** -101, 2.0 ** 101, 1e-120, np.inf, np.nan, 2.0 ** -100, 2.0 ** 100]))
    divisors = np.concatenate(divisors)
    num = _numerators()
    a = np.abs(num).reshape(-1)[:len(num) // 64 * 64].reshape(-1, 64)
    short = ((a >= 2.0 ** -300) & (a <= 2.0 ** 200)).all(axis=1)
    assert short.sum() > 1000 and (~short).sum() > 50  # waves that take the short form, waves that vote for the plain one
    bad, tested = ctx.udiv_mismatches(num, divisors)
    print("udiv: %d numerators x %d divisors, %d mismatches" % (len(num), len(divisors), bad))
    assert tested == len(num) * len(divisors)
    assert bad == 0


# ---- the scene table -------------------------------------------------------------------------------------------------------
def _check_table(ctx, sc):
    table, again = ctx.scene_consts()
    n = len(sc.lights)
    assert len(table["lights"]) == n
    assert table["words"].tobytes() == again["words"].tobytes()
    assert n == 0 or table["inv_n_lights"] == 1.0 / n
    assert table["pi"] == np.pi and abs(table["rcp_pi"] * np.pi - 1.0) <= 2.0 ** -51
    u2, v2 = _len2(sc.lights["f"][:, 3:6]), _len2(sc.lights["f"][:, 6:9])
    assert np.all(E.same(table["lights"][:, 0], u2)) and np.all(E.same(table["lights"][:, 2], v2))
    for d, r in ((u2, table["lights"][:, 1]), (v2, table["lights"][:, 3])):
        ok = (np.abs(d) >= 2.0 ** -100) & (np.abs(d) <= 2.0 ** 100)
        assert np.all(np.abs(r[ok] * d[ok] - 1.0) <= 2.0 ** -51)  # r within an ulp of 1 / d, the product rounded once
    safe = (np.abs(u2) >= 2.0 ** -100) & (np.abs(u2) <= 2.0 ** 100) & (np.abs(v2) >= 2.0 ** -100) & (np.abs(v2) <= 2.0 ** 100)
    assert np.array_equal(table["safe"], safe.astype(np.int64))
    return table


def test_scene_table_equals_its_second_evaluation_and_follows_the_upload(ctx):
    seen = []
    for sc in (G.scene(21), lit_scene(7), G.scene(23), degenerate_light_scene(), lit_scene(3), G.scene(21)):
        ctx.upload(sc)
        seen.append(_check_table(ctx, sc))
    assert [len(t["lights"]) for t in seen] == [1, 7, len(G.scene(23).lights), 4, 3, 1]
    assert list(seen[3]["safe"]) == [1, 0, 0, 0]
    assert seen[0]["words"].tobytes() == seen[5]["words"].tobytes()
    assert seen[1]["inv_n_lights"] == 1.0 / 7.0


# ---- light_pdf on the corner and the edges ---------------------------------------------------------------------------------
def _edge_records(sc, seed=0):
    rng = np.random.default_rng(seed)
    recs = []
    places = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (1.0, 0.5), (0.5, 1.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5)]
    for k in range(len(sc.lights)):
        f = sc.lights["f"][k]
        q, u, v, n = f[0:3], f[3:6], f[6:9], f[12:15]
        u = np.where(np.isfinite(u), u, 1.0)
        for (a, b) in places:
            target = q + a * u + b * v
            origins = [target + n]  # one unit in front, leaving along -normal: t = 1, planar = a U + b V up to rounding
            for axis in range(3):
                for way in (-np.inf, np.inf):
                    o = (target + n).copy()
                    o[axis] = np.nextafter(o[axis], way)
                    origins.append(o)
            for o in origins:
                recs.append((k, o, -n))
            for _ in range(6):  # oblique rays at the same place
                o = target + n * rng.uniform(0.5, 4.0) + rng.uniform(-2.0, 2.0, 3) * (1.0 - np.abs(n))
                recs.append((k, o, target - o))
    out = np.zeros(len(recs), dtype=A.LIGHTREC_DTYPE)
    for r, (k, o, d) in zip(out, recs):
        r["light"], r["p"], r["dir"], r["u"] = k, o, d, (0.25, 0.75)
    return out


@pytest.mark.parametrize("name", ["scene21", "scene23", "seven_lights", "degenerate_edges"])
def test_light_pdf_on_corner_and_edges(ctx, name):
    sc = {"scene21": lambda: G.scene(21), "scene23": lambda: G.scene(23), "seven_lights": lambda: lit_scene(7),
          "degenerate_edges": degenerate_light_scene}[name]()
    ctx.upload(sc)
    recs = _edge_records(sc)
    gold = G.oracle_records(sc, "rto_lights", recs)
    outs = [("full", ctx.test_records("lights", recs))]
    plan = N.scene_plan(sc)
    if plan["quad_lights_only"] and not plan["needs_uv"]:
        outs.append(("quadlit", ctx.test_records("lights", recs, ms=N.MS_QUADLIT)))
    if plan["lean_materials"]:
        outs.append(("lean", ctx.test_records("lights", recs, ms=N.MS_LEAN)))
    inside = int((gold["pdf_dir"] > 0).sum())
    print("%s: %d records, %d with a pdf, %d NaN" % (name, len(gold), inside, int(np.isnan(gold["pdf_dir"]).sum())))
    if name != "degenerate_edges":
        assert 0 < inside < len(gold)  # the records sit on the decision: some land on the light, some beside it
    for tag, out in outs:
        for f in E.LIGHT_FLOAT_FIELDS:
            bad = np.flatnonzero(~E.rows(E.same(out[f], gold[f])))
            for k in bad[:8]:
                print("%s %s: record %d light %d %s device %r reference %r" % (name, tag, k, gold["light"][k], f, out[f][k], gold[f][k]))
            assert len(bad) == 0, (name, tag, f)
        assert np.array_equal(out["is_delta"], gold["is_delta"])


# ---- renders ---------------------------------------------------------------------------------------------------------------
FORMS = {"queue": dict(), "static": dict(flags=A.FLAG_STATIC_GRID), "wavefront": dict(pipeline=A.PIPELINE_WAVEFRONT)}


def _render_equals_oracle(ctx, sc, w, h, spp, seed, forms=FORMS):
    ref = None
    for form, kw in forms.items():
        p = A.make_params(w, h, spp, integrator=A.INTEGRATOR_MIS, seed=seed, spp_chunks=1, **kw)
        if ref is None:
            ref, _ = G.oracle_render(sc, p, threads=0)
        out = ctx.render(p)
        k = ctx.last_kernel()
        print("%dx%d %s: %s" % (w, h, form, {a: k[a] for a in ("pipeline", "integrator", "trav", "ms", "pair", "queue")}))
        assert np.array_equal(E.bits(out), E.bits(ref)), (w, h, form, G.rel_l2(out, ref))


@pytest.mark.parametrize("w,h", [(2, 2), (17, 16)])
def test_small_renders_of_scene21_equal_the_oracle(ctx, w, h):
    sc = G.scene(21)
    ctx.upload(sc)
    _render_equals_oracle(ctx, sc, w, h, 3, seed=5)
    assert np.isfinite(ctx.render(A.make_params(w, h, 3, seed=5))).all()


def test_small_render_of_scene23_equals_the_oracle(ctx):
    """two lights and the QuadLights-only kernels: 1 / n_lights and both tables entries in compute_light_pdf's loop.  This
    scene's path calls sin and cos (OCML here, glibc in the oracle), so the bar against the oracle is test_gpu_parity's
    REL_L2_BAR (1e-3, BASELINE.json's tolerance), not bit equality; the job-queue kernel and its static twin are the same
    device arithmetic and must agree bit for bit."""
    sc = G.scene(23)
    ctx.upload(sc)
    outs = []
    for form, kw in FORMS.items():
        p = A.make_params(32, 16, 4, integrator=A.INTEGRATOR_MIS, seed=7, spp_chunks=1, **kw)
        outs.append(ctx.render(p))
    ref, _ = G.oracle_render(sc, A.make_params(32, 16, 4, integrator=A.INTEGRATOR_MIS, seed=7, spp_chunks=1), threads=0)
    assert np.array_equal(E.bits(outs[1]), E.bits(outs[0]))
    for form, out in zip(FORMS, outs):
        err = G.rel_l2(out, ref)
        print("scene 23, 32x16 spp 4, %s: rel-L2 against the oracle %.3e" % (form, err))
        assert err <= 1e-3


@pytest.mark.parametrize("w,h", [(1, 8), (8, 1)])
def test_one_pixel_wide_images_are_refused(ctx, w, h):
    """W - 1 = 0 or H - 1 = 0 would be the divisor of camera_sample: the library takes no such image"""
    ctx.upload(G.scene(21))
    with pytest.raises(G.rtr.RtrError) as e:
        ctx.render(A.make_params(w, h, 3))
    assert e.value.code == A.RTR_ERR_INVALID


@pytest.mark.parametrize("n_lights", [1, 2, 3, 7])
def test_scenes_of_several_quad_lights_equal_the_oracle(ctx, n_lights):
    sc = lit_scene(n_lights)
    ctx.upload(sc)
    _render_equals_oracle(ctx, sc, 16, 16, 4, seed=11)
