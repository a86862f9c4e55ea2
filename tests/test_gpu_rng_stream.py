"""The device's own normal draws, read back through a walk that takes every proposal.

The engine's only datasets are empty, it has no bounds, theta_0 = 0 and L = I: every
log-posterior is 0, the accept test (0 - 0) / T > log u holds for every u < 1, so every proposal
is taken (age == length is checked) and the step IS the draw: theta after the first step is z
exactly (0 + 1 z_j and exact zeros), later increments are z to ulp(|theta|).  d = 63, so every
z lane 0 ... 62 is in use beside lane 63's accept uniform.  (One function cannot carry 63
parameters and need not: the line on the empty dataset reads two of them, all 63 are proposed
and walk.  Two functions of 32 and 31 parameters would be a kernel compiled at run time - ten
seconds of hiprtc in a clean tree - for the same stepping code.)

Per value: the first step of every chain and lane equals orc_rng_normal(seed, chain, draw, slot)
bit for bit, for seeds with an empty, a low-only, a high-only and a full 64-bit Philox key and
for chain_offset 0 and 2^32 - 513, the largest mhx_create accepts for 512 chains (its check is
chain_offset + n_chains <= 2^32 - 1: the last 32-bit chain id, 0xFFFFFFFF, is not given out -
DESIGN section 8).  A draw counter beyond 2^32 cannot be reached by stepping: it stays untested.

Distribution and independence: tests/stat_cases.py stream_statistics over all 512 x 1000 x 63 =
3.2e7 increments, at the derived thresholds; tests/test_stat_host.py applies the same checks to
the oracle's stream on the CPU."""
import numpy as np
import pytest

import problems as pb
import stat_cases as sc

pytestmark = pytest.mark.gpu

D, CHAINS, DRAWS = 63, 512, 1000
SEEDS = [0, 1234, 0xDEADBEEF << 32, 0x9E3779B97F4A7C15]
OFFSETS = [0, (1 << 32) - 1 - CHAINS]


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def free_walk_engine(mhx, **kw):
    s = pb.Spec(D)
    s.add(pb.POLY, (), [0, 1], [], [], None, pb.NORMAL)
    e = s.engine(mhx, CHAINS, **kw)
    e.init_chains(np.zeros(D))
    return e


def oracle_normals(orc, seed, offset, draw=0):
    f = orc.lib().orc_rng_normal
    return np.array([[f(seed, offset + c, draw, l) for l in range(D)] for c in range(CHAINS)])


@pytest.mark.parametrize("offset", OFFSETS, ids=["offset0", "offset_max"])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed0", "seed_low", "seed_high_only", "seed_full"])
def test_first_draw_equals_the_oracle_per_value(mhx, orc, seed, offset):
    e = free_walk_engine(mhx, seed=seed, chain_offset=offset)
    e.many_steps(1, np.eye(D))
    st = e.state()
    print(e.kernel_name())
    e.close()
    assert (st["age"] == 2).all() and (st["length"] == 2).all() and (st["logpost"] == 0.0).all()
    want = oracle_normals(orc, seed, offset)
    assert np.array_equal(st["theta"], want), int((st["theta"] != want).sum())


def test_chain_ids_beyond_32_bits_are_refused(mhx):
    """(OFFSETS[1] is accepted: the per-value test runs on it)"""
    with pytest.raises(mhx.MhxError) as ei:
        mhx.Engine(CHAINS, 2, seed=1, chain_offset=(1 << 32) - CHAINS + 1)
    assert ei.value.code == mhx.capi.EINVAL


def test_the_stream_is_standard_normal_and_independent(mhx, orc):
    seed = SEEDS[3]
    e = free_walk_engine(mhx, seed=seed)
    e.many_steps(DRAWS, np.eye(D))
    st = e.state()
    assert (st["age"] == DRAWS + 1).all() and (st["length"] == DRAWS + 1).all()   # every proposal taken
    tr = e.traces(DRAWS + 1, cols=list(range(D)))
    e.close()
    assert (tr["n_out"] == DRAWS + 1).all()
    v = tr["values"]                                   # [chains, steps newest first, lanes]
    assert np.array_equal(v[:, 0, :], st["theta"]) and not v[:, -1, :].any()
    z = (v[:, :-1, :] - v[:, 1:, :])[:, ::-1, :]       # increments, oldest first: draw t, lane j
    del v, tr
    assert np.array_equal(z[:, 0, :], oracle_normals(orc, seed, 0))
    # a later draw: the oracle's to the rounding of theta + z (the difference back is exact), half
    # an ulp of a theta below 256
    t = DRAWS - 1
    assert np.abs(st["theta"]).max() < 256.0
    assert np.allclose(z[:, t, :], oracle_normals(orc, seed, 0, draw=t), rtol=0, atol=2.0 ** -46)
    stats = sc.stream_statistics(z)
    for k in sorted(stats):
        print("  %-26s %10.3f   [%g, %g]" % ((k,) + stats[k][:3]))
    print(sc.report("device normals, %d values" % z.size, stats))
    assert not sc.violations(stats), sc.violations(stats)
