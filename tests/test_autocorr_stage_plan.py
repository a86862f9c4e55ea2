"""CPU checks of the stage arithmetic of the autocorrelation read-out (carve_autocorr in
csrc/mhx_stage.hpp), driven as tests/test_histo_stage_plan.py drives the histogram read-outs: a
small program compiled against the header answers for a grid of shapes.  A portion's carved bytes
stay within the budget, its pieces lie in the engine's order - rho first - without reaching into
each other, and by the planner's accounting (the bytes asked for plus one alignment unit per
piece) one more chain would not fit."""
import itertools

import pytest

import autocorr_cases as ac

B = 1 << 26
NCS, MAX_LAGS = (1, 2, 8, 33, 63), (1, 255, 1023)


@pytest.fixture(scope="module")
def ask():
    if ac.carver_answers([]) is None:
        pytest.skip("no g++")
    return ac.carver_answers


def pieces(nc, max_lag):
    """bytes per chain of every piece, in the buffer's order: rho, tau, ess, half_mean, half_var,
    n_lags, n_used, status"""
    return [8 * nc * (max_lag + 1), 8 * nc, 8 * nc, 16 * nc, 16 * nc, 4, 4, 4 * nc]


def portion(nc, max_lag):
    """the chains of one portion, by the planner's accounting"""
    need = pieces(nc, max_lag)
    return (B - 256 * len(need)) // sum(need)


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit(ask):
    cases = list(itertools.product(NCS, MAX_LAGS))
    assert len(cases) == 15
    for (nc, max_lag), line in zip(cases, ask(["%d %d" % c for c in cases])):
        head, *carvings = line.split("|")
        P, fits = (int(w) for w in head.split())
        need = pieces(nc, max_lag)
        per, slack = sum(need), 256 * len(need)
        assert fits == 1, line                                    # one chain always fits: at most about 0.5 MB
        assert per + slack < (1 << 20)
        assert P == portion(nc, max_lag) >= 1, (nc, max_lag, line)
        assert (P + 1) * per + slack > B, (nc, max_lag, line)    # one more chain would not fit
        for n, carving in zip((1, P), carvings):
            total, *off = (int(w) for w in carving.split())
            size = [n * v for v in need]
            assert len(off) == len(need), (nc, max_lag, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (nc, max_lag, n, off)    # rho comes first
            for k in range(len(off)):
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (nc, max_lag, n, k, off)
            assert total <= B, (nc, max_lag, n, total)
    # the call of the two-portion GPU test: 33 columns of 1024 lags, about 272 KB a chain
    assert sum(pieces(33, 1023)) == 272060 and portion(33, 1023) == 246
