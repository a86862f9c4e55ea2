"""The host-only parts of walker-get-data-and-fit (mcmc-fitting.lisp:1230-1255): mhx_band_count,
the reference's (ceiling (* 0.66 take)) in single-float arithmetic, and the mirror's x-fit, the
reference's linspace (mcmc-fitting.lisp:235-248) in exact rationals.  No device is needed."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def count(mhx, take):
    k = C.c_int64(-1)
    rc = mhx.capi.lib().mhx_band_count(take, C.byref(k))
    return rc, k.value


def test_band_count_is_the_single_float_product(mhx):
    differ = 0
    for take in range(1, 5001):
        want = int(np.ceil(np.float32(0.66) * np.float32(take)))
        assert count(mhx, take) == (mhx.capi.OK, want), take
        assert mhx.band_count(take) == want
        differ += want != -((-66 * take) // 100)
    assert differ == 38  # the takes where the double / rational reading gives another count


@pytest.mark.parametrize("take, k", [(150, 100), (300, 199), (350, 232), (600, 397), (1, 1), (3, 2),
                                     (25, 17), (50, 33), (100, 66), (1000, 660), (1024, 676),
                                     (4096, 2704), (30000, 19800)])
def test_band_count_literals(mhx, take, k):
    assert count(mhx, take) == (mhx.capi.OK, k)


@pytest.mark.parametrize("take", [0, -1, -1000])
def test_band_count_refuses_a_take_below_one(mhx, take):
    assert count(mhx, take)[0] == mhx.capi.EINVAL
    assert mhx.capi.lib().mhx_band_count(5, None) == mhx.capi.OK  # (a NULL output is allowed)


@pytest.mark.parametrize("lo, hi", [(2000.0, 2997.0), (-4.0, 10.0), (0.1, 0.3), (0.0, 1.0),
                                    (-1e-7, 3e-7), (1.0, 1.0), (1e15, 1e15 + 8.0)])
def test_x_fit_is_the_rational_linspace(mhx, lo, hi):
    got = mhx.fit_linspace(lo, hi)
    assert got.shape == (1000,) and got.dtype == np.float64
    step = Fraction(hi - lo) / 999       # (rational (- end start)): of the DOUBLE difference
    want = [float(Fraction(lo) + i * step) for i in range(1000)]
    assert got.tolist() == want
    assert got[0] == lo
    if Fraction(lo) + Fraction(hi - lo) == Fraction(hi):  # (the difference was exact)
        assert got[-1] == hi
    assert (np.diff(got) >= 0).all()


def test_x_fit_ends_are_the_data_ends_exactly(mhx):
    for lo, hi in ((2000.0, 2997.0), (-4.0, 10.0), (0.1, 0.3)):
        got = mhx.fit_linspace(lo, hi)
        assert got[0] == lo and got[-1] == hi and len(got) == 1000
