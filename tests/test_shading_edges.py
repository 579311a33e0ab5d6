"""The shading functions of csrc/rt_device.h (mat_prepare, mat_sample, mat_eval, mat_pdf, mat_eval_pdf, mat_scatter,
light_sample, light_pdf, the environment-map code, the textures, pow5) against the reference ON their decisions: the
constructed records of oracle/ref_harness.cpp (materials-edge, scatter-edge, lights-edge; tests/_shading_edges.py) and the
random scatter vectors, through the unit kernels of include/rtr_hip_test.h.  The CPU oracle equals the same fixtures bit
for bit (tests/test_oracle_golden.py).

Bars: decisions and NaN masks equal on every record; bit-exact wherever the path is + - * / sqrt only; elsewhere the bar
of test_gpu_parity.test_unit_materials (relative 1e-11: OCML's sin / cos against glibc's, pow5 against pow)."""
import numpy as np
import pytest

import _golden as G
import _shading_edges as E

A = G.A
N = G.rtr.native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(rtr):
    c = rtr.Context(0)
    yield c
    c.close()


def _upload(ctx, sid):
    sc = G.scene(sid)
    ctx.upload(sc)
    return sc


def _report(tag, f, out, gold, good):
    """print the records of a field that miss their bar before the assertion fails on them"""
    bad = np.flatnonzero(~E.rows(good))
    for k in bad[:8]:
        print("%s: record %d material/light %d  %s device %r reference %r" % (tag, k, gold[k][0], f, out[f][k], gold[f][k]))
    return len(bad)


def _check_float_fields(tag, out, gold, fields, exact, mask=None):
    """NaN masks equal; bit-exact on `exact` records, relative 1e-11 on the others"""
    sel = np.ones(len(gold), dtype=bool) if mask is None else mask
    for f in fields:
        assert np.array_equal(np.isnan(out[f][sel]), np.isnan(gold[f][sel])), (tag, f, "NaN mask")
        ex = sel & exact
        assert _report(tag, f, out, gold, E.rows(E.same(out[f], gold[f])) | ~ex) == 0, (tag, f, "not bit-exact")
        assert _report(tag, f, out, gold, E.rows(E.close(out[f], gold[f], 1e-11)) | ~sel) == 0, (tag, f, "outside 1e-11")


def _materials_exact(sc, gold):
    """records whose whole path is + - * / sqrt: metal, lambertian over a solid or image texture, diffuse_light, and the
    dielectric's reflect branch"""
    types, tex = E.material_types(sc, gold), E.first_texture_types(sc, gold)
    plain = np.isin(tex, [A.TEX_SOLID, A.TEX_IMAGE])
    return (types == A.MAT_METAL) | ((types == A.MAT_LAMBERTIAN) & plain) | ((types == A.MAT_DIFFUSE_LIGHT) & plain) | \
        ((types == A.MAT_DIELECTRIC) & (gold["is_transmission"] == 0))


def _scatter_exact(sc, gold):
    """all of scatter except the dielectric (pow5 against pow decides nothing here, but refract is left at 1e-11 as in
    sample) and an albedo from a noise or checker texture (sin)"""
    types, tex = E.material_types(sc, gold), E.first_texture_types(sc, gold)
    return (types != A.MAT_DIELECTRIC) & ~np.isin(tex, [A.TEX_NOISE, A.TEX_CHECKER])


def _check_materials(tag, sc, out, gold):
    for f in ("sample_ok", "rng_out", "is_transmission"):
        assert np.array_equal(out[f], gold[f]), (tag, f, np.flatnonzero(out[f] != gold[f])[:8])
    ok = E.sample_written(sc, gold)
    assert np.array_equal(out["is_specular"][ok], gold["is_specular"][ok]), tag
    exact = _materials_exact(sc, gold)
    _check_float_fields(tag, out, gold, ("eval", "pdf", "emitted"), exact)
    _check_float_fields(tag, out, gold, ("s_wi", "s_f", "s_pdf"), exact, ok)
    # the fused mat_eval_pdf of the MIS kernels equals mat_eval and mat_pdf in every bit
    assert np.array_equal(out["pad"], np.zeros_like(out["pad"])), (tag, "mat_eval_pdf", np.flatnonzero(out["pad"])[:8])


def _check_scatter(tag, sc, out, gold):
    for f in ("sample_ok", "rng_out", "is_specular", "is_transmission", "pad"):
        assert np.array_equal(out[f], gold[f]), (tag, f, np.flatnonzero(out[f] != gold[f])[:8])
    _check_float_fields(tag, out, gold, ("s_wi", "s_f"), _scatter_exact(sc, gold), E.scatter_written(sc, gold))
    _check_float_fields(tag, out, gold, ("s_pdf", "eval", "pdf", "emitted"), np.ones(len(gold), dtype=bool))


@pytest.mark.parametrize("sid", E.MATERIAL_EDGE_SCENES)
def test_material_edge_records(ctx, sid):
    sc = _upload(ctx, sid)
    gold = G.records(E.material_edge_name(sid), A.MAT_DTYPE)
    _check_materials("materials_edge%d" % sid, sc, ctx.test_records("materials", gold), gold)


@pytest.mark.parametrize("name", sorted(E.SCATTER_FILES))
def test_scatter_records(ctx, name):
    """mat_scatter had no unit vector: only whole Li records of integrators 0 and 1 saw it"""
    sc = _upload(ctx, E.SCATTER_FILES[name])
    gold = G.records(name, A.MAT_DTYPE)
    _check_scatter(name, sc, ctx.test_records("scatter", gold), gold)


@pytest.mark.parametrize("sid", [21, 23, 15, 17, 18, 19])
def test_light_edge_records(ctx, sid):
    """QuadLight, PointLight, DirectionalLight, SpotLight and the map-less EnvironmentLight: + - * / sqrt only, every field
    bit-exact, a NaN equal to a NaN"""
    _upload(ctx, sid)
    gold = G.records(E.light_edge_name(sid), A.LIGHTREC_DTYPE)
    out = ctx.test_records("lights", gold)
    _check_float_fields("lights_edge%d" % sid, out, gold, E.LIGHT_FLOAT_FIELDS, np.ones(len(gold), dtype=bool))
    assert np.array_equal(out["is_delta"], gold["is_delta"])


@pytest.mark.parametrize("sid", [24, 26])
def test_environment_map_edge_records(ctx, sid):
    """The rules of test_gpu_parity.test_delta_and_environment_lights on the edge records of the two mapped environment
    lights: sin / cos / acos / atan2 come from OCML here and from glibc there, so an ulp in (u, v) could select the
    neighbouring texel on a record that sits on a cell boundary by construction; records outside 1e-9 are counted
    against the committed measurement (tests/golden/gpu_residue.json).  Measured on an MI355X: 0 records on every field
    of both scenes, as for the CPU oracle -- the 1 % of the provisional bar is a cap that nothing uses."""
    _upload(ctx, sid)
    gold = G.records(E.light_edge_name(sid), A.LIGHTREC_DTYPE)
    out = ctx.test_records("lights", gold)
    assert np.array_equal(out["pdf"] == 0, gold["pdf"] == 0)
    for f in ("Li", "pdf", "pdf_dir"):
        assert np.array_equal(np.isnan(out[f]), np.isnan(gold[f])), f
        ok = E.rows(E.close(out[f], gold[f], 1e-9))
        _report("lights_edge%d" % sid, f, out, gold, ok)
        G.residue("lights_edge_scene%02d.%s.records_outside_1e-9" % (sid, f), int((~ok).sum()), int(0.01 * len(ok)))
    assert np.array_equal(np.isnan(out["wi"]), np.isnan(gold["wi"]))
    assert np.nanmax(np.abs(out["wi"] - gold["wi"])) <= 1e-12
    assert np.all(np.isinf(out["dist"])) and np.array_equal(out["is_delta"], gold["is_delta"])


MS_CASES = [(21, N.MS_LEAN), (21, N.MS_QUADLIT), (23, N.MS_QUADLIT), (23, N.MS_LEAN), (E.EDGE_SCENE, N.MS_QUADLIT),
            (E.EDGE_SCENE, N.MS_LEAN), (18, N.MS_QUADLIT)]


@pytest.mark.parametrize("sid,ms", MS_CASES)
def test_material_set_instantiations_equal_the_full_one(ctx, sid, ms):
    """mat_prepare<MS> ... light_pdf<MS> of RT_MS_LEAN / RT_MS_QUADLIT, the instantiations the headline kernels are built from
    (albedo, roughness and metallic from the lowered record), against RT_MS_FULL on the same records: the same device
    code, so every output bit.  A scene mega_variant would not give such a kernel is refused, the records untouched."""
    sc = _upload(ctx, sid)
    plan = N.scene_plan(sc)
    allowed = plan["lean_materials"] if ms == N.MS_LEAN else (plan["quad_lights_only"] and not plan["needs_uv"])
    assert bool(allowed) == ((sid, ms) in [(21, N.MS_LEAN), (21, N.MS_QUADLIT), (23, N.MS_QUADLIT)])
    sets = []
    if sid in E.MATERIAL_EDGE_SCENES:
        mats = G.records(E.material_edge_name(sid), A.MAT_DTYPE)
        sets += [("materials", mats), ("scatter", mats)]
    if sid in E.LIGHT_EDGE_SCENES:
        sets += [("lights", G.records(E.light_edge_name(sid), A.LIGHTREC_DTYPE)),
                 ("lights", G.records("lights_scene%02d.bin" % sid, A.LIGHTREC_DTYPE))]
    assert sets
    for kind, recs in sets:
        if not allowed:
            with pytest.raises(G.rtr.RtrError) as e:
                ctx.test_records(kind, recs, ms=ms)
            assert e.value.code == A.RTR_ERR_UNSUPPORTED
            buf = recs.copy()  # the entry point itself, on an array the test keeps
            rc = getattr(N.test_lib(), "rtr_test_%s_ms" % kind)(ctx._h, buf.ctypes.data, len(buf), int(ms))
            assert rc == A.RTR_ERR_UNSUPPORTED and buf.tobytes() == recs.tobytes()
            continue
        full = ctx.test_records(kind, recs)
        assert ctx.test_records(kind, recs, ms=N.MS_FULL).tobytes() == full.tobytes()
        out = ctx.test_records(kind, recs, ms=ms)
        for f in out.dtype.names:
            a, b = out[f], full[f]
            if a.dtype.kind == "f":
                assert np.all(E.same(a, b)), (kind, f)
            else:
                assert np.array_equal(a, b), (kind, f)
        if kind == "materials":
            assert not out["pad"].any()


def test_pow5_device_equals_the_host_build(ctx):
    """pow5 on the device against rtr_test_pow5_host on the 65 536 values of the pow5 fixtures, bit for bit: both are the
    same fused multiply-adds without contraction, so the device inherits the host's committed distance to glibc's
    pow(x, 5.0) (test_oracle_golden.test_pow5_host_is_within_one_ulp_of_glibc_pow)."""
    xy, _ = E.pow5_pairs()
    x = np.ascontiguousarray(xy[:, 0])
    dev, host = ctx.test_records("pow5", x), N.pow5_host(x)
    bad = np.flatnonzero(E.bits(dev) != E.bits(host))
    for k in bad[:8]:
        print("pow5: x %r device %r host %r" % (x[k], dev[k], host[k]))
    assert len(bad) == 0
