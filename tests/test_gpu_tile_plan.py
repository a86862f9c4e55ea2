"""The tile plan of the batch sweeps.  `-m gpu`: needs an MI355X.

sweep_yw() and sweep() form, once per sweep and per function, a wave-uniform plan - windows and
tiles as 32-bit counts, whether the second half of the last two-array tile exists, the data
points of the ragged last window, scalar bases of the arrays that advance per tile - and issue
their LDS-DMA and seed loads from a scalar base plus a constant lane offset.  What such a plan
can get wrong sits at the ends of a dataset and where a per-64-windows reload happens, so the
datasets here are the smallest that reach each of those places:

    n = 1, 64, 65        one partly filled window
    n = 2047, 2049       one ragged window; two windows, the second nearly empty
    n = 6144             three whole windows: the 16-wave yw tile whose second half does not exist
    n = 8193             a ragged fifth window
    n = 131072, 131073   64 windows and 65: the (wi & 63) == 0 reload of the window masks and of
                         the seeds' x

in both kernel families, 37 chains (a partial last workgroup in both), with the two-array "yw"
layout and without it (MHX_NO_YW=1).  The layout and the plan must not show in any bit.
"""
import os

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

CHAINS = 37
SIZES = [1, 64, 65, 2047, 2049, 6144, 8193, 131072, 131073]
WALK_SIZES = [2049, 6144, 131073]

# tolerance against the faithful oracle: that of tests/test_gpu_parity.py (stated there)
REL = 1e-12
PRIOR_ULP = 2.0 ** -52 * 1e10


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def engine_pair(mhx, spec, wpg, th0):
    """(engine without the yw layout, engine with it) in kernel family `wpg`"""
    out = []
    os.environ["MHX_FAMILY_WPG"] = wpg
    try:
        for flag in ("1", None):
            if flag:
                os.environ["MHX_NO_YW"] = flag
            try:
                e = spec.engine(mhx, CHAINS, seed=8)
                e.init_chains(th0)  # finalises the problem under these settings
            finally:
                os.environ.pop("MHX_NO_YW", None)
            out.append(e)
    finally:
        os.environ.pop("MHX_FAMILY_WPG", None)
    return out


def proposal_vectors(theta_star):
    th = pb.perturbed(theta_star, 64, 0.02, seed=4)   # all-recurrence vectors: yw tiles
    th[5, 4] = 1e-4                                   # ... but for three: a narrow peak,
    th[21, 7] = -0.03                                 # a negative width,
    th[40, 3] = 7.5                                   # a centre far outside the data
    return th


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("wpg", ["8", "16"])
def test_plan_leaves_every_bit_alone(mhx, orc, n, wpg):
    """Log-posteriors of 64 vectors - all-recurrence ones, which take the yw tiles, and the three
    odd ones that make their workgroup fall back to the three-array tiles - are the same bits
    with and without the yw layout, and equal the oracle's mirror of the summation order."""
    s = pb.two_peak(n=n, seed=40 + n % 7)
    op = s.oracle(orc)
    th0 = pb.perturbed(s.theta_star, CHAINS, 0.01, seed=3)
    a, b = engine_pair(mhx, s, wpg, th0)
    try:
        th = proposal_vectors(s.theta_star)
        ga, gb = a.logpost(th), b.logpost(th)
        assert np.array_equal(ga, gb), (n, wpg)
        for c in (0, 1, 5, 21, 40, 63):
            assert gb[c] == op.logpost_mirror(th[c]), (n, wpg, c)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("n", WALK_SIZES)
@pytest.mark.parametrize("wpg", ["8", "16"])
def test_short_walk_same_states_in_both_layouts(mhx, n, wpg):
    """A settled walk (small steps around theta*: nearly every sweep takes the yw tiles) ends in
    the same states and the same proposal factor whichever layout its sweeps take."""
    s = pb.two_peak(n=n, seed=40 + n % 7)
    th0 = pb.perturbed(s.theta_star, CHAINS, 0.01, seed=3)
    a, b = engine_pair(mhx, s, wpg, th0)
    try:
        l0 = np.diag(0.003 * np.abs(s.theta_star))
        for e in (a, b):
            e.adaptive_begin(900, 10.0, 1, l_matrix=l0)
            e.adaptive_advance(1 << 40)
        sa, sb = a.state(), b.state()
        for k in ("theta", "logpost", "best_logpost", "age", "length"):
            assert np.array_equal(sa[k], sb[k]), (n, wpg, k)
        assert np.array_equal(a.lmatrix(), b.lmatrix())
    finally:
        a.close()
        b.close()


def two_lengths(n_short=1500, n_long=9000, seed=6):
    """A global fit of two functions on the SAME eight parameters whose datasets are one window
    and five windows long: the plan is a thing of the function, not of the sweep."""
    s = pb.Spec(8)
    for k, n in enumerate((n_short, n_long)):
        one = pb.two_peak(n=n, seed=seed + k)
        (model, shape, idx), (x, y, sig, lik), b = one.fns[0], one.data[0], one.bounds[0]
        s.add(model, shape, idx, x, y, sig, lik, b)
        s.theta_star = one.theta_star
    return s


@pytest.mark.parametrize("wpg", ["8", "16"])
def test_plan_is_formed_per_function(mhx, orc, wpg):
    """Two functions of different lengths in one problem: same bits in both layouts, and the
    faithful oracle's value within the tolerance tests/test_gpu_parity.py holds global fits to."""
    s = two_lengths()
    assert s.K == 2 and len(s.data[0][0]) <= 2048 < 4 * 2048 < len(s.data[1][0]) <= 5 * 2048
    op = s.oracle(orc)
    th0 = pb.perturbed(s.theta_star, CHAINS, 0.01, seed=3)
    a, b = engine_pair(mhx, s, wpg, th0)
    try:
        th = proposal_vectors(s.theta_star)
        ga, gb = a.logpost(th), b.logpost(th)
        assert np.array_equal(ga, gb), wpg
        # (not vector 40: its centre lies 7 outside its bound, where the prior -1e10 (exp(x) - 1)
        # turns one ulp of exp into more than the stated 2^-52 * 1e10 per violated bound)
        for c in (0, 1, 2, 5, 21, 63):
            n_viol = 0
            for bd in s.bounds:
                idx, lo, hi = bd
                v = th[c][idx]
                n_viol += int((~((np.asarray(lo) < v) & (v < np.asarray(hi)))).sum())
            ref = op.logpost(th[c])
            tol = REL * op.abs_terms(th[c]) + 4 * PRIOR_ULP * n_viol + 1e-300
            assert abs(gb[c] - ref) <= tol, (wpg, c, gb[c], ref, tol)
    finally:
        a.close()
        b.close()
