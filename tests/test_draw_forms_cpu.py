"""A random draw in (-1, 1) as a double (csrc/rt_device.h: draw_sym_join) in its host build, bit for bit against the
reference's text -1.0 + s * 2^-31 for random_double(-1, 1), s the 32-bit state of the generator.  The joined form places s
in the low word of a double with a constant high word and subtracts a constant; both operands and the difference are
representable, so nothing may differ in any bit, the sign of zero at s = 2^31 included.  The expected values are numpy's: a
uint32 converts to float64 exactly, the product with a power of two is exact, and -1.0 + x is one correctly rounded IEEE
addition (which here does not round either).  (The same device for s * 2^-32 was built, held to these tests, measured
inside the run-to-run spread and taken out again: profiles/r21_draws.txt; rng_next is the reference's text.)
No GPU needed."""
import itertools
import os

import numpy as np

import _golden as G

N = G.rtr.native


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _check(s):
    s = np.ascontiguousarray(s, dtype=np.uint32)
    x = s.astype(np.float64)
    want = -1.0 + x * 2.0 ** -31
    got = N.draw_host(s)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    for k in bad[:8]:
        print("s %#010x got %r (%#018x) want %r (%#018x)" % (s[k], got[k], _bits(got)[k], want[k], _bits(want)[k]))
    assert len(bad) == 0, len(bad)
    return len(s)


def _few_bits():
    """every s with at most two bits set, and every s with at most two bits clear"""
    few = {0}
    for a in range(32):
        few.add(1 << a)
    for a, b in itertools.combinations(range(32), 2):
        few.add((1 << a) | (1 << b))
    return np.array(sorted(few | {0xFFFFFFFF ^ v for v in few}), dtype=np.uint32)


def test_states_with_few_bits_set_or_clear():
    s = _few_bits()
    assert len(s) == 2 * (1 + 32 + 32 * 31 // 2)
    assert _check(s) == len(s)


def test_the_named_states():
    s = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1], dtype=np.uint32)
    _check(s)
    got = N.draw_host(s)
    assert _bits(got)[3] == 0  # the zero is a positive one, as the reference's -1.0 + 1.0
    assert got[0] == -1.0 and got[-1] == 1.0 - 2.0 ** -31


def test_a_stride_over_the_whole_range():
    """2^24 states, 256 apart, from an odd start so that the low bits are not all zero: against numpy, and again through the
    library's own comparison loop (which the exhaustive test below relies on)"""
    s = (np.arange(2 ** 24, dtype=np.uint64) * 256 + 0x5B).astype(np.uint32)
    assert _check(s) == 2 ** 24
    assert N.draw_host_range(0x5B, 2 ** 24, 256, threads=2) == (0, 2 ** 24)


def test_every_state():
    """all 2^32 states, compared inside the library by up to 16 threads (about a second per thread at 2^28 states)"""
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    assert N.draw_host_range(0, 2 ** 32, 1, threads=threads) == (0, 2 ** 32)


def test_the_comparison_loop_covers_its_range():
    """its split over threads visits every state of a range once, the last state of all included"""
    for threads in (1, 3, 16):
        assert N.draw_host_range(2 ** 32 - 1000, 1000, 1, threads=threads) == (0, 1000)
        assert N.draw_host_range(0, 7, 2 ** 29, threads=threads) == (0, 7)
