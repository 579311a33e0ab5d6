"""The arithmetic of the lane-varying short forms (csrc/rt_device.h: rcp_short, sqrt_short and their windows) in its host
build, element by element, against the host's own 1.0 / d and sqrt(x).  The host divides and takes square
roots correctly rounded (IEEE 754), which is what the device's expansions deliver too, so equality here is the
specification: a refined seed followed by the expansion's tail must land on the correctly rounded result for every operand
inside the window, and an operand outside it must not take the short form at all.

The host has no v_rcp_f64 / v_rsq_f64.  Its seeds are the correctly rounded reciprocal and reciprocal square root, taken
twice: as they are, and with their low 29 bits cleared -- an error of up to 2^29 ulp, the accuracy the ISA manual gives the
two instructions (see rt_device.h).  With the exact seed every operand must come out correctly rounded.  With the coarse
one the same holds but for one class that is excluded by name: a divisor whose mantissa is all ones (the value below a power
of two) is the classical exception of Newton-Raphson reciprocal refinement -- the refined reciprocal of 2^k (1 - 2^-53)
lands on the tie 2^-k (1 + 2^-53) and rounds to even, 2^-k, from any seed within 2^-27, and the tail (the compiler's own
last three instructions) cannot leave it; the result is then the neighbour of the rounded one, which the test asserts.
The GPU test (tests/test_lane_division.py) holds the short forms to the compiler's expansion on such divisors too.
No GPU needed."""
import numpy as np

import _golden as G

N = G.rtr.native


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _window(x, lo, hi, positive=False):
    a = x if positive else np.abs(x)
    return (a >= 2.0 ** lo) & (a < (np.inf if hi == 1024 else 2.0 ** hi))


def _random(rng, n, lo, hi, signed=True):
    x = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(lo, hi, n))
    return x * rng.choice([-1.0, 1.0], n) if signed else x


COARSE = 29  # bits cleared in the coarse seed


def _all_ones(d):
    return (_bits(d) & np.uint64(2 ** 52 - 1)) == np.uint64(2 ** 52 - 1)


def _check(op, a, inside):
    """both seeds; returns how many elements took the short form"""
    with np.errstate(all="ignore"):
        want = 1.0 / a if op == "rcp" else np.sqrt(a)
    nan = np.isnan(want)
    for coarse in (0, COARSE):
        got, took = N.lane_host(op, a, coarse_bits=coarse)
        assert np.array_equal(took, inside), op  # the window is the documented one, edge for edge
        assert np.array_equal(np.isnan(got), nan), op
        differs = (_bits(got) != _bits(want)) & ~nan
        if coarse and op == "rcp":  # the exception of the module's docstring: the neighbour of the rounded result
            exc = differs & took & _all_ones(a)
            assert np.all(np.abs(_bits(got[exc]).astype(np.int64) - _bits(want[exc]).astype(np.int64)) == 1), op
            differs &= ~exc
        bad = np.flatnonzero(differs)
        for k in bad[:8]:
            print("%s (seed -%d bits): a %r got %r want %r" % (op, coarse, a[k], got[k], want[k]))
        assert len(bad) == 0, (op, coarse, len(bad))
    return int(took.sum())


def test_the_edge_list():
    s = N.lane_specials()
    assert len(s) == 68 and len(np.unique(_bits(s))) == 68
    for e in (-767, -300, -200, -100, 100, 200):
        for v in (2.0 ** e, np.nextafter(2.0 ** e, 0.0), np.nextafter(2.0 ** e, np.inf)):
            assert v in s and -v in s
    assert np.isnan(s).sum() == 6 and np.isinf(s).sum() == 2 and (s == 0).sum() == 2
    assert 5e-324 in s and 2.0 ** -1022 in s and 2.0 ** -1023 in s and np.finfo(np.float64).max in s


def test_short_forms_on_the_edge_list():
    s = N.lane_specials()
    n_short = _check("rcp", s, _window(s, -100, 100))
    assert 0 < n_short < len(s)
    n_short = _check("sqrt", s, _window(s, -767, 1024, positive=True))
    assert 0 < n_short < len(s)


def test_short_forms_on_random_operands_in_the_window():
    rng = np.random.default_rng(2020)
    n = 10 ** 6
    d = _random(rng, n, -100, 100)
    assert _check("rcp", d, np.ones(n, dtype=bool)) == n
    x = _random(rng, n, -767, 1024, signed=False)
    assert _check("sqrt", x, np.ones(n, dtype=bool)) == n
    # mantissas at the ends of a binade, where a reciprocal or a root sits closest to a rounding boundary
    m = np.concatenate([1.0 + np.arange(1, 2049) * 2.0 ** -52, 2.0 - np.arange(1, 2049) * 2.0 ** -52])
    for e in (-100, -1, 0, 1, 99):
        dd = np.ldexp(m, e)
        _check("rcp", dd, np.ones(len(dd), dtype=bool))
        _check("rcp", -dd, np.ones(len(dd), dtype=bool))
    for e in (-767, -766, -1, 0, 1, 1022, 1023):
        xx = np.ldexp(m, e)
        _check("sqrt", xx, np.ones(len(xx), dtype=bool))
