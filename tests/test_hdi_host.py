"""CPU checks of the highest-density interval's definition (include/mhx.h, mhx_get_hdi): the numpy
yardstick of tests/hdi_cases.py against an independent O(n^2) statement of it, mhx_hdi_span through
the ABI against Python's integers, and the package's host definition hdi() against the yardstick."""
import ctypes as C
import math

import numpy as np
import pytest

import hdi_cases as hd


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def plain_order(values):
    """ascending, -0 before +0, NaNs last: Python's own sort of (is NaN, value, is not negative)"""
    return sorted(values, key=lambda v: (math.isnan(v), 0.0 if math.isnan(v) else v, math.copysign(1.0, v) > 0))


def plain_hdi(values, num, den):
    """the definition stated over ALL intervals of g + 1 consecutive order statistics: the first one
    that no other is narrower than"""
    s = plain_order(values)
    n = len(s)
    g = min((n * num) // (100 * den), n - 1)
    widths = [s[j + g] - s[j] for j in range(n - g)]
    for j, w in enumerate(widths):
        if all(w <= other for other in widths):
            return s[j], s[j + g], j, sum(1 for other in widths if other == w)
    raise AssertionError("no least width among finite values")


def crafted_columns():
    rng = np.random.default_rng(95)
    base = np.array([1.0, -2.5, 1e-3, -1e5, 0.0, -0.0, 7.0, -0.125])
    pool = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)])
    cols = [np.array([3.5]), np.array([-0.0, 0.0]), np.array([0.0, -0.0, 0.0, -0.0, 1.0]),
            np.array([2.0, 1.0]), np.arange(10.0), np.arange(10.0)[::-1].copy(), np.full(7, -2.5),
            np.array([0.0, 1.0, 2.0, 10.0, 11.0, 12.0]),          # two runs of equal width: the lower wins
            np.array([0.0, 1.0, 1.0 + 2.0 ** -52, 2.0, 3.0])]     # neighbours in the last bit
    for n in (2, 3, 9, 17, 33, 64, 65, 100, 200):
        cols.append(rng.choice(pool, n))                            # ties, signed zeros, last-bit neighbours
        cols.append(rng.normal(0.0, 2.0, n))
        cols.append(np.round(rng.exponential(1.0, n), 1))           # skewed, pressed against 0, many ties
    return cols


def test_the_yardstick_is_the_definition_over_all_intervals():
    tied = away = 0
    for x in crafted_columns():
        lo, hi, pos, _, status, ties = hd.column(x, hd.MASSES, 0)
        assert status == 0
        for q, (num, den) in enumerate(hd.MASSES):
            wlo, whi, wpos, wties = plain_hdi(x.tolist(), num, den)
            assert (pos[q], ties[q]) == (wpos, wties), (x, num, den)
            assert lo[q] == np.float64(wlo).view(np.uint64) and hi[q] == np.float64(whi).view(np.uint64), (x, num, den)
            tied += wties > 1
            away += wpos > 0
    assert tied > 30 and away > 30, (tied, away)          # the inputs reach the tie rule and the scan
    # -0 sorts before +0 and comes back as itself; mass 100 is the window's least and greatest value
    lo, hi, pos, rungs, _, _ = hd.column(np.array([0.0, -0.0, 5.0]), [(100, 1), (1, 1000)], 3)
    assert lo.tolist() == [1 << 63, 1 << 63] and hi.tolist() == [np.float64(5.0).view(np.uint64), 1 << 63]
    assert rungs.tolist() == [1 << 63, 0, np.float64(5.0).view(np.uint64)] and pos.tolist() == [0, 0]


def test_the_ladder_and_the_status_of_values_that_are_not_finite():
    x = np.array([1.0, np.nan, -np.inf, 3.0, -np.nan, np.inf, 2.0])
    _, _, _, rungs, status, _ = hd.column(x, [], 7)
    assert status == 1
    want = [-np.inf, 1.0, 2.0, 3.0, np.inf]
    assert rungs[:5].tolist() == [np.float64(v).view(np.uint64) for v in want]
    assert (rungs[5:] == hd.NAN_BITS).all()                         # every NaN last, and canonical
    # ranks repeat where the window is shorter than the ladder, and follow floor(i (n - 1) / (L - 1))
    _, _, _, rungs, status, _ = hd.column(np.array([3.0, 1.0, 2.0]), [], 8)
    assert status == 0 and rungs.view(np.float64).tolist() == [1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 3.0]


def test_the_crafted_histories_exercise_the_tie_rule_and_the_scan():
    """the figures of the definition's first run in numpy: of the 15000 (chain, column, take, mass)
    cases of the crafted d = 2 histories 2950 have more than one position of least width and 5551
    their winner away from j = 0"""
    walks = hd.d2_walks()
    cases = tied = away = 0
    for take in hd.TAKES:
        want = hd.want_hdi(hd.windows_of(walks, take), [0, 1], hd.ISSUE_MASSES)
        cases += want["pos"].size
        tied += int((want["ties"] > 1).sum())
        away += int((want["pos"] > 0).sum())
    assert (cases, tied, away) == (15000, 2950, 5551)


def test_hdi_span_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()

    def ask(n, num, den):
        g = C.c_int64(-7)
        rc = lib.mhx_hdi_span(n, num, den, C.byref(g))
        return rc, g.value

    rng = np.random.default_rng(7)
    cases = [(1, 1, 1), (1, 100, 1), (1, 95, 1), (2, 100, 1), (2, 50, 1), (2, 1, 1000), (1000, 95, 1),
             (1000, 1365, 20), (57, 10, 1), (2048, 1, 1000), (2 ** 31 - 1, 10 ** 8, 10 ** 6),
             (2 ** 31 - 1, 10 ** 8 - 1, 10 ** 6), (2 ** 31 - 1, 1, 10 ** 6), (2 ** 63 - 1, 10 ** 8 - 1, 10 ** 6),
             (2 ** 63 - 1, 10 ** 8, 10 ** 6), (2 ** 63 - 1, 99999, 1000)]
    for _ in range(2000):
        den = int(rng.integers(1, 10 ** 6 + 1))
        cases.append((int(rng.integers(1, 2 ** 62)), int(rng.integers(1, 100 * den + 1)), den))
        cases.append((int(rng.integers(1, 5000)), int(rng.integers(1, 100 * den + 1)), den))
    for n, num, den in cases:
        assert ask(n, num, den) == (capi.OK, hd.span(n, num, den)), (n, num, den)
    assert ask(1, 1, 1)[1] == 0 and ask(10, 100, 1)[1] == 9 and ask(2 ** 31 - 1, 10 ** 8, 10 ** 6)[1] == 2 ** 31 - 2
    for n, num, den in [(0, 95, 1), (-1, 95, 1), (10, 0, 1), (10, -1, 1), (10, 101, 1), (10, 95, 0), (10, 95, -1),
                        (10, 95, 10 ** 6 + 1), (10, 10 ** 8 + 1, 10 ** 6), (10, 2001, 20)]:
        rc, g = ask(n, num, den)
        assert rc == capi.EINVAL and g == -7 and lib.mhx_last_error(), (n, num, den)
    assert lib.mhx_hdi_span(10, 95, 1, None) == capi.OK                  # no output asked for
    assert mhx.hdi_span(1000, 95) == 950 and mhx.hdi_span(1000, (1365, 20)) == 682 and mhx.hdi_span(3, 2.5) == 0
    for bad in ((0, 95), (10, 0), (10, 100.5), (10, (1, 10 ** 6 + 1)), (10, (2 ** 40, 1))):
        with pytest.raises(ValueError):
            mhx.hdi_span(*bad)


def test_the_host_definition_against_the_yardstick(mhx):
    for x in crafted_columns():
        for mass in hd.MASSES:
            lo, hi, pos = mhx.hdi(x, mass)
            wlo, whi, wpos, _, _, _ = hd.column(x, [mass], 0)
            assert (np.float64(lo).view(np.uint64), np.float64(hi).view(np.uint64), pos) == (wlo[0], whi[0], wpos[0])
    x = np.round(np.random.default_rng(1).exponential(1.0, 1000), 2)
    lo, hi, pos = mhx.hdi(x.tolist(), 95)                                  # a number of per cent
    # (a posterior pressed against 0: the narrowest interval lies below the equal-tailed one)
    assert (lo, hi, pos) == mhx.hdi(x, (95, 1)) and lo < np.percentile(x, 2.5) and hi < np.percentile(x, 97.5)
    with pytest.raises(ValueError):
        mhx.hdi([], 95)
    with pytest.raises(ValueError):
        mhx.hdi([1.0, 2.0], 0)
