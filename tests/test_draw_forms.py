"""A random draw in (-1, 1) as a double on the device (csrc/rt_device.h: rng_sym): the lean kernels place the generator's
state in the low word of a double with a constant high word and subtract a constant -- one addition where the reference's
text, -1.0 + s * 2^-31, converts, scales and adds.  It is exact, so every draw, everything computed from draws and every
state the generator is left in must be what the plain text gives, bit for bit.  (The same device for rng_next's
s * 2^-32 passed these tests too, measured inside the run-to-run spread and was taken out: profiles/r21_draws.txt.)

  * the joined form beside the plain text for all 2^32 states (include/rtr_hip_test.h: rtr_test_draw_forms);
  * the functions that draw -- random_in_unit_sphere, random_in_unit_disk, random_cosine_direction, rng_range(0.25, 7.5),
    rng_int(0, 6) -- from 2^20 seeded states, lane by lane, with the joined form and in the plain text (the test library's
    second instantiation): every output bit and every exit state (rtr_test_draw_callers);
  * scene 21 at 64x64 spp 16, MIS, through the job-queue kernel and through the static grid: the reference's stored image
    bit for bit.
tests/test_draw_forms_cpu.py holds the host build to the same text."""
import numpy as np
import pytest

import _golden as G
import _shading_edges as E

A = G.A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(rtr):
    c = rtr.Context(0)
    yield c
    c.close()


def test_joined_form_is_the_plain_text_on_every_state(ctx):
    bad, tested, first = ctx.draw_forms()
    print("draw forms: %d states, %d mismatches%s" % (tested, bad, ", one at s = %#010x" % (first - 1) if first else ""))
    assert bad == 0
    assert tested == 2 ** 32


def test_every_caller_draws_the_same_bits_and_leaves_the_same_state(ctx):
    n = 2 ** 20
    for seed in (21, 0xD1CE):
        bad, tested, first = ctx.draw_callers(seed, n)
        print("draw callers, seed %d: %d lanes, %d mismatches%s" % (seed, tested, bad, ", one from state %#010x" % first if first else ""))
        assert bad == 0
        assert tested == n
    # a lane count that ends inside a wave
    assert ctx.draw_callers(3, 1000)[:2] == (0, 1000)


FORMS = {"queue": dict(), "static": dict(flags=A.FLAG_STATIC_GRID)}


@pytest.mark.parametrize("form", FORMS)
def test_scene21_is_the_stored_image(ctx, form):
    img, info = G.image("img_scene21_i4_64_spp16.f64")
    assert (info["width"], info["height"], info["spp"]) == (64, 64, 16)
    ctx.upload(G.scene(21))
    p = A.make_params(info["width"], info["height"], info["spp"], integrator=A.INTEGRATOR_MIS, seed=info["seed"],
                      pipeline=A.PIPELINE_MEGAKERNEL, spp_chunks=1, **FORMS[form])
    out = ctx.render(p)
    k = ctx.last_kernel()
    print("scene 21 %s: %s" % (form, {a: k[a] for a in ("pipeline", "integrator", "trav", "ms", "pair", "queue")}))
    assert bool(k["queue"]) == (form == "queue")
    assert np.array_equal(E.bits(out), E.bits(img)), (form, G.rel_l2(out, img))
