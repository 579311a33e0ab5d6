"""1.0 / d and sqrt(x) of a lane's own numbers in the shading of the lean MIS kernels (csrc/rt_device.h: rcp_lane, sqrt_lane
and sqrt_rcp_lane, which takes a root and its reciprocal under one vote): a wave whose lanes all hold operands in the
ordinary range takes a short form of the compiler's expansion, every other wave the expansion itself, so the result must be
the compiler's bits wherever it is used.  (The general quotient n / d was built the same way, measured inside the
run-to-run spread and taken out again with its kernel: profiles/r20_lane_div.txt.)

  * each short form beside the compiler's result on 2^26 operands: random mantissas under every exponent of the accepted
    window, and in every fourth wave one lane on or beside a window edge, zero, a denormal, an infinity or a NaN
    (include/rtr_hip_test.h: rtr_test_rcp_lane, rtr_test_sqrt_lane).  The kernel reports how many operands it compared and
    how many sat in a wave that voted for the short form: both kinds of wave must occur;
  * renders of scene 21 (MIS and RR) and scene 23 through the job-queue kernel and its static twin against the CPU oracle:
    bit for bit on scene 21; scene 23 calls sin and cos (OCML here, glibc in the oracle), so there the two kernels must
    agree bit for bit and stay within test_gpu_parity's 1e-3 of the oracle, as in tests/test_uniform_divisors.py."""
import numpy as np
import pytest

import _golden as G
import _shading_edges as E

A = G.A
N = G.rtr.native

pytestmark = pytest.mark.gpu

TOTAL = 2 ** 26


@pytest.fixture(scope="module")
def ctx(rtr):
    c = rtr.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("op", N.LANE_OPS)
def test_short_form_is_the_compilers_result(ctx, op):
    bad, tested, short, first = ctx.lane_mismatches(op)
    print("%s_lane: %d operands, %d in waves that voted for the short form, %d mismatches" % (op, tested, short, bad))
    if bad:
        a, _, got, want = first.view(np.float64)
        print("  first: operand %r (%#018x): got %r (%#018x), expected %r (%#018x)" % (a, first[0], got, first[2], want, first[3]))
    assert tested == TOTAL
    # three waves in four hold operands in range only; the fourth carries one edge value, often one outside the window
    assert TOTAL // 2 < short < TOTAL
    assert bad == 0


FORMS = {"queue": dict(), "static": dict(flags=A.FLAG_STATIC_GRID)}


@pytest.mark.parametrize("integrator", [A.INTEGRATOR_MIS, A.INTEGRATOR_RR])
def test_scene21_equals_the_oracle(ctx, integrator):
    sc = G.scene(21)
    ctx.upload(sc)
    ref = None
    for form, kw in FORMS.items():
        p = A.make_params(64, 64, 16, integrator=integrator, seed=20, spp_chunks=1, **kw)
        if ref is None:
            ref, _ = G.oracle_render(sc, p, threads=0)
        out = ctx.render(p)
        k = ctx.last_kernel()
        print("scene 21 integrator %d %s: %s" % (integrator, form, {a: k[a] for a in ("pipeline", "integrator", "trav", "ms", "pair", "queue")}))
        assert np.array_equal(E.bits(out), E.bits(ref)), (integrator, form, G.rel_l2(out, ref))


def test_scene23_kernels_agree_and_follow_the_oracle(ctx):
    sc = G.scene(23)
    ctx.upload(sc)
    outs = []
    for form, kw in FORMS.items():
        p = A.make_params(64, 36, 8, integrator=A.INTEGRATOR_MIS, seed=20, spp_chunks=1, **kw)
        outs.append(ctx.render(p))
        k = ctx.last_kernel()
        print("scene 23 %s: %s" % (form, {a: k[a] for a in ("pipeline", "integrator", "trav", "ms", "pair", "queue")}))
    ref, _ = G.oracle_render(sc, A.make_params(64, 36, 8, integrator=A.INTEGRATOR_MIS, seed=20, spp_chunks=1), threads=0)
    assert np.array_equal(E.bits(outs[1]), E.bits(outs[0]))
    for form, out in zip(FORMS, outs):
        err = G.rel_l2(out, ref)
        print("scene 23, 64x36 spp 8, %s: rel-L2 against the oracle %.3e" % (form, err))
        assert err <= 1e-3
