"""The stepping kernels preserve the exact posterior.  Every other test of the stepping path
compares the device with a restatement of the project's own specification; these ask whether
that specification, as the kernels run it, samples the posterior: C chains start at EXACT draws
of a posterior known in closed form (tests/stat_cases.py), take 64 steps (mhx_many_steps at
T = 1, 64 mhx_take_step calls at T = 3), and their final states must still be exact draws,
independent across chains - held to the yardstick's statistics at its derived thresholds
(|z| <= 5.5, sqrt(C) D <= 2.9; tests/test_stat_host.py shows the same design passing for a float64
sampler and failing for six planted faults).

Out of scope: the distribution at the end of walker-adaptive-steps.  Annealing, adaptation and
the automatic shutdown are the reference's algorithm, are only approximately stationary, and are
already compared bit for bit with the oracle."""
import os

import numpy as np
import pytest

import stat_cases as sc

pytestmark = pytest.mark.gpu

SEED = 20250611
SEED_HIGH = (0xA5A5F00D << 32) | SEED      # the same low word, a non-zero Philox key[1]
PER_ENGINE = sc.CHAINS // sc.ENGINES


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def steps(e, n, L, T):
    if T == 1.0:
        e.many_steps(n, L)
    else:
        for _ in range(n):
            e.take_step(L, T)


def finish(mhx, e, n_steps):
    """the final states of an engine, after the checks every run gets: all chains took all steps
    and none was frozen (no proposal had a NaN log-posterior)"""
    st, status = e.state(), e.chain_status()[0]
    assert (status != mhx.capi.CHAIN_FP_TRAP).all()
    assert (st["age"] == n_steps + 1).all() and (st["length"] == n_steps + 1).all()
    return st["theta"]


_pooled = {}


def pooled_run(mhx, cs, T, kind, seed):
    """(theta before the last step, final theta) [CHAINS, d]: four engines of 16 384 chains with
    chain_offset 0, 16384, ... and one seed (the history rings bound the engine: 1024 slots of
    d <= 4 are about 0.7 GB for 16 384 chains)"""
    key = (cs.name, T, kind, seed)
    if key not in _pooled:
        th0 = sc.start_draws(cs, T)
        L = cs.l_matrix(kind, T)
        before, after = [], []
        for i in range(sc.ENGINES):
            e = cs.spec.engine(mhx, PER_ENGINE, seed=seed, chain_offset=i * PER_ENGINE)
            e.init_chains(th0[i * PER_ENGINE:(i + 1) * PER_ENGINE])
            steps(e, sc.N_STEPS - 1, L, T)
            before.append(e.state()["theta"])
            steps(e, 1, L, T)
            after.append(finish(mhx, e, sc.N_STEPS))
            e.close()
        _pooled.clear()                      # (one run is kept: the next test of the same case)
        _pooled[key] = (np.concatenate(before), np.concatenate(after))
    return _pooled[key]


def check(label, stats):
    print(sc.report(label, stats))
    assert not sc.violations(stats), (label, sc.violations(stats))


@pytest.mark.parametrize("kind", sc.L_KINDS)
@pytest.mark.parametrize("T", sc.TEMPERATURES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_batch_kernels_preserve_the_posterior(mhx, name, T, kind):
    cs = sc.case(name)
    before, theta = pooled_run(mhx, cs, T, kind, SEED)
    tg = cs.target(T)
    st = sc.sample_statistics(tg, theta)
    if name == "const1" and T == 1.0:
        # the last step's acceptance: whether the state changed is a Bernoulli(p) across chains
        moved = (before != theta).any(axis=1)
        p = sc.accept_stationary_1d(0.3 if kind == "bad" else 2.38)
        st["last_step_acceptance"] = sc.z_stat(sc.binomial_z(int(moved.sum()), moved.size, p))
    if name == "wall1":
        assert (theta < cs.hi).all()          # the wall is hard at this scale (stat_cases)
    check("%s T=%g L=%s" % (name, T, kind), st)


def test_the_high_word_of_the_seed_is_used(mhx):
    """Philox key[1] = seed >> 32: a second seed with the same low word gives another walk, which
    passes on its own"""
    cs = sc.case("line2")
    _, first = pooled_run(mhx, cs, 1.0, "good", SEED)
    first = first.copy()
    _, second = pooled_run(mhx, cs, 1.0, "good", SEED_HIGH)
    assert SEED_HIGH & 0xFFFFFFFF == SEED and SEED_HIGH >> 32
    same = (first == second).all(axis=1)
    # (two chains end alike only where both rejected all 64 proposals: never at 36 % acceptance)
    assert not same.any(), int(same.sum())
    check("line2 T=1 L=good, high seed word", sc.sample_statistics(cs.target(1.0), second))


@pytest.mark.parametrize("name", ["line2", "cubic4"])
def test_one_step_from_the_mode(mhx, name):
    """every chain at the mode, one mhx_take_step with L = s chol(Sigma): the accepted fraction is
    (1 + s^2 / T)^(-d/2), the accepted proposals have whitened variance s^2 / (1 + s^2 / T)"""
    cs = sc.case(name)
    tg = cs.target(1.0)
    e = cs.spec.engine(mhx, PER_ENGINE, seed=SEED + 1)
    mode = np.tile(cs.beta, (PER_ENGINE, 1))
    for T in (1.0, 4.0):
        for s in (0.6, 1.7):
            e.init_chains(mode)
            e.take_step(s * tg.chol, T)
            theta = finish(mhx, e, 1)
            moved = (theta != mode).any(axis=1)
            check("%s T=%g s=%g one step from the mode" % (name, T, s),
                  sc.mode_step_statistics(tg, theta, moved, s, T))
    e.close()


def split_engine(mhx, spec, chains, persistent, **kw):
    """an engine finalised in the tile-sliced split mode, as one persistent launch per portion or
    as two launches per iteration (the autouse fixture pins MHX_SPLIT=0: the switches are set
    here, as tests/test_gpu_split.py does)"""
    keys = ("MHX_SPLIT", "MHX_TSPLIT", "MHX_PERSIST_TS")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    if not persistent:
        os.environ["MHX_PERSIST_TS"] = "0"
        os.environ["MHX_TSPLIT"] = "4"
    try:
        e = spec.engine(mhx, chains, **kw)
        name = e.kernel_name()               # finalises under this setting
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return e, name


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "two_launches"])
def test_split_modes_preserve_the_posterior(mhx, persistent):
    """line2 on 8192 points, the shortest dataset that opens split mode for 256 walkers: 64 times
    256 walkers from fresh exact draws in fresh engines with chain_offset = 256 r (no stream is
    used twice), 16 384 independent final states.  The persistent form has its own
    accept-and-publish order, so it is a case of its own."""
    cs = sc.case("line2", 8192)
    tg = cs.target(1.0)
    walkers, reps = 256, 64
    th0 = tg.draw(sc.philox(cs.seed + 8192), walkers * reps)
    L = cs.l_matrix("good", 1.0)
    out = []
    for r in range(reps):
        e, name = split_engine(mhx, cs.spec, walkers, persistent, seed=SEED, chain_offset=walkers * r)
        assert "tsplit x" in name and ("persistent" in name) == persistent, name
        e.init_chains(th0[r * walkers:(r + 1) * walkers])
        e.many_steps(sc.N_STEPS, L)
        out.append(finish(mhx, e, sc.N_STEPS))
        e.close()
    check("line2 N=8192 %s" % name.split("/")[1], sc.sample_statistics(tg, np.concatenate(out)))


def test_truth_through_a_read_out(mhx):
    """ensemble_percentiles(take=1) of one 16 384-chain engine after the walk: one newest step per
    chain, hence independent draws; its 2.5, 50 and 97.5 % points against the Gaussian quantiles
    within 5.5 sqrt(q (1 - q) / C) / phi(z_q) posterior sigmas"""
    cs = sc.case("line2")
    tg = cs.target(1.0)
    C = PER_ENGINE
    e = cs.spec.engine(mhx, C, seed=SEED + 2)
    e.init_chains(tg.draw(sc.philox(cs.seed + 2), C))
    e.many_steps(sc.N_STEPS, cs.l_matrix("good", 1.0))
    finish(mhx, e, sc.N_STEPS)
    qs = [0.025, 0.5, 0.975]
    got = e.ensemble_percentiles(1, [(5, 2), (50, 1), (195, 2)])
    e.close()
    assert got["n_pooled"] == C and (got["status"] == 0).all()
    zq = sc.ndtri(np.array(qs))
    for i, q in enumerate(qs):
        se = np.sqrt(q * (1 - q) / C) / (np.exp(-0.5 * zq[i] ** 2) / np.sqrt(2 * np.pi))
        dev = (got["out"][i] - (cs.beta + zq[i] * tg.sd)) / tg.sd
        print("line2 ensemble percentile %4.1f %%: %s posterior sigmas off, allowed %.4f" % (100 * q, dev, 5.5 * se))
        assert (np.abs(dev) <= 5.5 * se).all(), (q, dev, se)
