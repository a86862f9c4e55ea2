"""The statistical yardstick (tests/stat_cases.py) holds and has power, on the CPU: its CDFs
against mpmath where that imports and against each other everywhere, the PIT of its exact draws,
its float64 reference sampler through every check the GPU tests apply (same problems, chain
counts, start seeds, step count, proposal matrices and temperatures), the six planted faults each
beyond a threshold, the closed-form acceptance figures, and the oracle's normals through the
checks tests/test_gpu_rng_stream.py applies to the device's - so that a failure on the GPU can be
placed."""
import math

import numpy as np
import pytest

import stat_cases as sc


def _mpmath():
    try:
        import mpmath
    except ImportError:
        return None
    return mpmath


def test_cdfs():
    x = np.array([-9.0, -5.5, -2.0, -0.3, 0.0, 0.7, 1.0, 3.3, 6.0, 8.2])
    p = sc.ndtr(x)
    assert np.allclose(p + sc.ndtr(-x), 1.0, rtol=0, atol=2e-16)
    assert np.allclose(sc.ndtri(p[:8]), x[:8], rtol=1e-11, atol=0)   # (beyond: 1 - p has few digits left)
    r = np.array([1e-6, 0.1, 1.0, 2.5, 7.0, 30.0, 60.0])
    for d in (2, 4):                                 # chi^2_d is Gamma(d/2, 1/2)
        assert np.allclose(sc.chi2_cdf_even(r, d), sc.gamma_p(d / 2.0, r / 2.0), rtol=1e-13, atol=4e-16)
    for a in (1, 7, 193, 3130):                      # the series against the finite Poisson sum
        xs = a + math.sqrt(a) * np.array([-6.0, -3.0, -1.0, 0.0, 0.5, 2.0, 5.0])
        xs = xs[xs > 0]
        # (1 - the sum of a terms cancels in the lower tail: an absolute error of a few a 2^-53)
        assert np.allclose(sc.gamma_p(a, xs), sc.gamma_p_poisson_sum(a, xs), rtol=1e-9, atol=8 * a * 2.0 ** -53 + 1e-15), a
    assert sc.gamma_p(5.5, np.array([-1.0, 0.0, 1e9]))[[0, 1, 2]].tolist() == [0.0, 0.0, 1.0]
    mp = _mpmath()
    if mp is not None:
        with mp.workprec(120):
            assert np.allclose(p, [float(mp.ncdf(float(v))) for v in x], rtol=4e-15, atol=0)
            for a in (1.0, 2.5, 65.33, 1044.0, 3130.0):
                xs = a + math.sqrt(a) * np.array([-5.0, -2.0, 0.0, 1.0, 4.0])
                xs = xs[xs > 0]
                ref = [float(mp.gammainc(a, 0, float(v), regularized=True)) for v in xs]
                assert np.allclose(sc.gamma_p(a, xs), ref, rtol=1e-11, atol=1e-16), a
            ref = [float(mp.gammainc(2, 0, float(v) / 2, regularized=True)) for v in r]
            assert np.allclose(sc.chi2_cdf_even(r, 4), ref, rtol=1e-13, atol=4e-16)   # (1 - exp(-h)(1 + h))


def test_thresholds_are_the_derived_ones():
    assert 2.0 * float(sc.ndtr(-sc.Z_MAX)) == pytest.approx(3.8e-8, rel=0.01)
    assert 2.0 * math.exp(-2.0 * sc.KS_MAX ** 2) == pytest.approx(1e-7, rel=0.05)
    assert sc.MAX_ABS_NORMAL == pytest.approx(8.5717, abs=1e-4)


@pytest.mark.parametrize("name", sc.NAMES)
def test_exact_draws_pass_and_the_problems_are_what_the_docstring_says(name):
    cs = sc.case(name)
    assert cs.spec.d == cs.d and len(cs.spec.data[0][0]) == (sc.RATE_POINTS if name == "rate1" else sc.N_POINTS)
    for T in sc.TEMPERATURES:
        tg = cs.target(T)
        th = sc.start_draws(cs, T)
        st = sc.sample_statistics(tg, th)
        print(sc.report("%s T=%g exact draws" % (name, T), st))
        assert not sc.violations(st), sc.violations(st)
        if name == "wall1":
            assert (th < cs.hi).all()
            assert cs.hi == pytest.approx(cs.beta[0] + 0.5 * math.sqrt(cs.cov[0, 0]), rel=1e-14)
            # the wall is hard at this scale: all wall1 runs of the suite together (2 temperatures,
            # 2 proposal matrices, host and GPU) expect fewer than 1e-3 states beyond it
            assert cs.leak(T) * sc.CHAINS * 8 < 1e-3
        if name == "rate1":
            assert tg.mean / tg.sd[0] > 13.0          # the rate stays 13 sigma from 0 ...
            for kind in sc.L_KINDS:                    # ... and so does every proposal
                assert cs.negative_proposal_probability(kind, T) < 1e-30


def test_the_gaussian_posteriors_are_the_normal_equations_solution():
    """beta^ and Sigma from the high-precision elimination against numpy's least squares in float64,
    and the reference sampler's quadratic form against the sum over the points it abbreviates"""
    for name in ("const1", "line2", "cubic4", "global3"):
        cs = sc.case(name)
        rows, ys, sig = [], [], []
        for (model, shape, idx), (x, y, s, lik) in zip(cs.spec.fns, cs.spec.data):
            for xv, yv, sv in zip(x, y, s):
                r = np.zeros(cs.d)
                for j, k in enumerate(idx):
                    r[k] += xv ** j
                rows.append(r / sv)
                ys.append(yv / sv)
                sig.append(sv)
        A, b = np.array(rows), np.array(ys)
        beta = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.allclose(cs.beta, beta, rtol=1e-10, atol=1e-12)
        assert np.allclose(cs.cov, np.linalg.inv(A.T @ A), rtol=1e-9)
        th = cs.target(1.0).draw(sc.philox(5), 7)
        direct = np.array([-0.5 * np.sum((A @ t - b) ** 2) for t in th])
        got = cs.logpost(th)
        assert np.allclose((got - got[0]) - (direct - direct[0]), 0.0, atol=1e-9 * np.abs(direct).max())


def walk_rng(cs, T, kind):
    return sc.philox([cs.seed, int(T), sc.L_KINDS.index(kind), 77])


@pytest.mark.slow
@pytest.mark.parametrize("kind", sc.L_KINDS)
@pytest.mark.parametrize("T", sc.TEMPERATURES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_reference_sampler_preserves_every_posterior(name, T, kind):
    cs = sc.case(name)
    tg = cs.target(T)
    th0 = sc.start_draws(cs, T)
    s = 0.3 if kind == "bad" else 2.38
    rng = walk_rng(cs, T, kind)
    th, _ = sc.reference_walk(cs, T, cs.l_matrix(kind, T), th0, sc.N_STEPS - 1, rng)
    th, moved = sc.reference_walk(cs, T, cs.l_matrix(kind, T), th, 1, rng)
    st = sc.sample_statistics(tg, th)
    if name == "const1" and T == 1.0:        # the last step's acceptance, in closed form
        p = sc.accept_stationary_1d(s)
        st["last_step_acceptance"] = sc.z_stat(sc.binomial_z(int(moved.sum()), moved.size, p))
    print(sc.report("%s T=%g L=%s reference sampler" % (name, T, kind), st))
    assert not sc.violations(st), sc.violations(st)
    if name == "wall1":
        assert (th < cs.hi).all()


# (fault, problem, T, L, chains).  The first four are gross (|z| of hundreds) in the design of the
# GPU tests' line2 case already at a quarter of their chains.  z_mean is what the deliberately bad
# L is for: steps of 0.3 sd carry a shift of 0.02 per draw a long way before a rejection pulls
# back (|z| > 80; with the good L it is 5 ... 7 at 65 536 chains: at the threshold).  stale_prob is
# the weakest: second order in the step's change of log-posterior, it widens the distribution by a
# part in a hundred - |z| = 4.7 and sqrt(C) D = 2.7 on line2, inside the thresholds; on cubic4 with
# the good L, where the proposals change the log-posterior most, |z| = 4.4 ... 8.4 and
# sqrt(C) D = 3.5 ... 4.4 over three seeds tried: found every time, by the radius' Kolmogorov
# statistic at least, but not by much.  A fault of this size in ONE kernel variant is at the edge of what 65 536 chains show.
POWER = [("ignore_T", "line2", 3.0, "good", 16384), ("times_T", "line2", 3.0, "good", 16384),
         ("no_log", "line2", 1.0, "good", 16384), ("u_from_z", "line2", 1.0, "good", 16384),
         ("z_mean", "line2", 1.0, "bad", 65536), ("stale_prob", "cubic4", 3.0, "good", 65536)]


@pytest.mark.parametrize("fault,name,T,kind,chains", POWER, ids=[p[0] for p in POWER])
def test_planted_faults_are_found(fault, name, T, kind, chains):
    """a design of the GPU tests (64 steps from exact draws, same start seed) with one fault planted
    in the sampler: a statistic must leave its threshold"""
    cs = sc.case(name)
    tg = cs.target(T)
    th0 = sc.start_draws(cs, T, chains)
    th, _ = sc.reference_walk(cs, T, cs.l_matrix(kind, T), th0, sc.N_STEPS, walk_rng(cs, T, kind), fault=fault)
    st = sc.sample_statistics(tg, th)
    print(sc.report("%s %s T=%g L=%s C=%d" % (fault, name, T, kind, chains), st))
    assert sc.violations(st), (fault, sc.worst(st))


@pytest.mark.parametrize("name", ["line2", "cubic4"])
def test_closed_form_acceptance_from_the_mode(name):
    cs = sc.case(name)
    C = sc.CHAINS
    for T in (1.0, 4.0):
        for s in (0.6, 1.7):
            tg = cs.target(1.0)
            th0 = np.tile(cs.beta, (C, 1))
            th, acc = sc.reference_walk(cs, T, s * tg.chol, th0, 1, sc.philox([cs.seed, int(T), int(10 * s)]))
            st = sc.mode_step_statistics(tg, th, acc, s, T)
            print(sc.report("%s T=%g s=%g one step from the mode" % (name, T, s), st))
            assert not sc.violations(st), sc.violations(st)


STREAM_SEED = 0x9E3779B97F4A7C15


def test_oracle_normals_pass_the_stream_checks(orc):
    """orc_rng_normal on 32 chains x 1000 draws x 63 lanes = 2.0e6 values"""
    f = orc.lib().orc_rng_normal
    chains, draws, lanes = 32, 1000, 63
    z = np.array([f(STREAM_SEED, c, t, l) for c in range(chains) for t in range(draws) for l in range(lanes)])
    st = sc.stream_statistics(z.reshape(chains, draws, lanes))
    print(sc.report("orc_rng_normal, %d values" % z.size, st))
    assert not sc.violations(st), sc.violations(st)
    # ... and the checks see a stream that is subtly wrong: a tail that is too light (|z| capped
    # where a 26-bit uniform would cap it), odd lanes that repeat their neighbour once in 50 draws
    bad = z.reshape(chains, draws, lanes).copy()
    bad[:, ::50, 1::2] = bad[:, ::50, 0:-1:2]
    assert any(k.startswith("corr") for k in sc.violations(sc.stream_statistics(bad)))
    light = np.clip(z, -3.3, 3.3).reshape(chains, draws, lanes)
    assert sc.violations(sc.stream_statistics(light))
