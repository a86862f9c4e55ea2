"""mhx_percentile_rank (include/mhx.h): the position rule of nth-percentile
(mcmc-fitting.lisp:1495-1506) that the device's order statistics use, against the rule of
walker.py::_percentile restated here with exact rationals.  Host only: no device is needed."""
import ctypes as C
from fractions import Fraction

import pytest

PCTS = [(0, 1), (5, 2), (25, 1), (50, 1), (75, 1), (841, 10), (195, 2), (100, 1)]


@pytest.fixture(scope="module")
def capi():
    import lisp_mcmc_amd
    return lisp_mcmc_amd.capi


def rank(capi, length, num, den):
    pos, between = C.c_int64(-1), C.c_int32(-1)
    rc = capi.lib().mhx_percentile_rank(length, num, den, C.byref(pos), C.byref(between))
    return rc, pos.value, between.value


def test_rank_equals_the_mirrors_rational_rule_for_every_length(capi):
    for num, den in PCTS:
        # what _percentile makes of the number a caller writes (50, 2.5, 84.1, ...)
        n = Fraction(num, den)
        assert Fraction(float(n)).limit_denominator(1000) == n
        for length in range(1, 3001):
            q = n * (length - 1) / 100
            lo = q.numerator // q.denominator
            assert rank(capi, length, num, den) == (capi.OK, lo, int(q != lo)), (num, den, length)


def test_the_median_is_the_references_integer_arithmetic(capi):
    # (* 50 (- len 1) 1/100): even lengths fall between two elements, odd ones on one
    for length in range(1, 200):
        assert rank(capi, length, 50, 1) == (capi.OK, (length - 1) // 2, (length - 1) % 2)


def test_ends_and_large_lengths(capi):
    assert rank(capi, 1, 100, 1) == (capi.OK, 0, 0)
    assert rank(capi, 7, 0, 1) == (capi.OK, 0, 0)
    assert rank(capi, 7, 100, 1) == (capi.OK, 6, 0)
    big = 2 ** 31 - 1
    q = Fraction(841, 10) * (big - 1) / 100
    assert rank(capi, big, 841, 10) == (capi.OK, q.numerator // q.denominator, 1)


def test_bad_arguments_are_einval_and_outputs_may_be_null(capi):
    lib = capi.lib()
    for length, num, den in ((0, 50, 1), (-3, 50, 1), (10, 50, 0), (10, 50, -2), (10, -1, 1),
                             (10, 101, 1), (10, 1001, 10)):
        assert rank(capi, length, num, den)[0] == capi.EINVAL, (length, num, den)
        assert lib.mhx_last_error()
    assert lib.mhx_percentile_rank(10, 50, 1, None, None) == capi.OK
    assert rank(capi, 10, 1000, 10) == (capi.OK, 9, 0)
