"""make_histo / make_histo_x (lisp-mcmc_amd/walker.py) against a literal transcription of
make-histo's count-for-bins (mcmc-fitting.lisp:1548-1557: successive `position` / `subseq`) over
boundaries formed as the reference's linspace forms them (mcmc-fitting.lisp:235-248) with
Fractions.  Needs no device."""
from fractions import Fraction

import numpy as np
import pytest


@pytest.fixture(scope="module")
def walker():
    from lisp_mcmc_amd import walker
    return walker


def linspace(start, end, n):
    """(linspace start end :len n): exact rationals from the DOUBLE difference, coerced at the end"""
    step = Fraction(end - start) / (n - 1)
    return [float(Fraction(start) + i * step) for i in range(n)]


def count_for_bins(sequence, num_bins):
    """make-histo as written: bin n takes, of what is left, the elements before the first one that
    boundary n is not >= to ((position b seq :test-not #'>=)), or all of it"""
    seq = list(sequence)
    boundaries = linspace(min(seq), max(seq), num_bins + 1)
    out = []
    for n in range(1, num_bins + 1):
        pos = next((i for i, v in enumerate(seq) if not boundaries[n] >= v), len(seq))
        out.append(pos)
        seq = seq[pos:]
    return out, boundaries


def sequences():
    rng = np.random.default_rng(1541)
    for case in range(900):
        n = int(rng.integers(1, 61))
        kind = case % 3
        if kind == 0:
            v = rng.normal(rng.normal(0.0, 100.0), 10.0 ** rng.integers(-3, 4), n)
        elif kind == 1:  # tied values, some of them neighbours in the last bit
            pool = rng.normal(0.0, 3.0, 5)
            pool = np.concatenate([pool, np.nextafter(pool, np.inf)])
            v = rng.choice(pool, n)
        else:
            v = rng.integers(-20, 21, n).astype(np.float64)
        yield np.sort(v), int(rng.integers(1, 25))


def test_make_histo_is_count_for_bins(walker):
    dropped = cases = 0
    for v, bins in sequences():
        want, boundaries = count_for_bins(v, bins)
        assert walker.histo_edges(v[0], v[-1], bins) == boundaries, (v, bins)
        got = walker.make_histo(v, bins)
        assert got == want and all(isinstance(c, int) for c in got), (v, bins)
        assert sum(got) <= len(v)
        dropped += boundaries[-1] < v[-1]
        assert (sum(got) < len(v)) == (boundaries[-1] < v[-1])
        cases += 1
    assert cases == 900
    # the last boundary can round below the greatest value, which then lies in no bin
    assert dropped > 0


@pytest.mark.parametrize("v, bins, want", [
    ([4.25] * 7, 5, [7, 0, 0, 0, 0]),      # all equal: every boundary is that value
    ([-3.0], 3, [1, 0, 0]),                # one value
    ([1.0, 2.0, 2.0, 9.0], 1, [4]),        # one bin
    ([0.0, 1.0, 2.0], 2, [2, 1]),          # a value on an inner boundary belongs below it
])
def test_make_histo_edge_cases(walker, v, bins, want):
    assert count_for_bins(v, bins)[0] == want
    assert walker.make_histo(v, bins) == want


def test_make_histo_x(walker):
    x = walker.make_histo_x(list(range(101)), 20)
    assert len(x) == 20 and x[0] == 2.5 and x[-1] == 100.0
    assert x == linspace(2.5, 100.0, 20)
    rng = np.random.default_rng(1559)
    for _ in range(50):
        v = np.sort(rng.normal(3.0, 2.0, int(rng.integers(2, 40))))
        bins = int(rng.integers(2, 25))
        start = v[0] + (v[-1] - v[0]) / bins / 2
        assert walker.make_histo_x(v, bins) == linspace(start, v[-1], bins)
    # one bin: the reference's linspace of one element divides by zero; the centre is returned
    assert walker.make_histo_x([1.0, 3.0], 1) == [2.0]
