"""mhx_get_residuals on the device against the numpy yardstick of its definition
(tests/resid_cases.py), walker by walker, from the model values mhx_eval_function returns:

  fit                                  bit for bit mhx_eval_function itself
  z, chi2, sum_z, dw, max_abs_z        bit for bit the yardstick (a NaN stands for any NaN)
  n_pos, n_runs, n_out, max_index,
  status                               exactly

Every operation of the definition is a single IEEE rounding in a stated order, so there is no
tolerance anywhere.  Covered: the lane, row and block edges of the neighbour rule, a split of the
points into chunks, planted extremes, every kernel path, datasets per walker in all four sigma
kinds and both forms, a group, the ABI's edges and the mirror's walker_set_get_residuals family."""
import numpy as np
import pytest

import problems as pb
import resid_cases as rc

pytestmark = pytest.mark.gpu

CHUNK = 1 << 17                 # kFitChunkPoints
KEYS = ("chi2", "sum_z", "dw", "max_abs_z", "max_index", "n_pos", "n_runs", "n_out", "status")


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.RESID_BLOCK == rc.BLOCK
    return lisp_mcmc_amd


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return rc.same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def check(e, fn, theta, lik, y_of, sigma_of, z_limit=3.0, flagged=(), where=""):
    """Engine.residuals of function fn against the yardstick on every chain; y_of(c), sigma_of(c):
    walker c's data.  Returns the pointwise result."""
    r = e.residuals(fn, theta, z_limit=z_limit, pointwise=True)
    bare = e.residuals(fn, theta, z_limit=z_limit)
    assert set(bare) == set(KEYS) and set(r) == set(KEYS) | {"fit", "z"}
    th = e.state()["best_theta"] if theta is None else np.asarray(theta, dtype=np.float64)
    v = e.eval_function(fn, th)
    assert rc.same_bits(r["fit"], v), where
    for c in range(e.n_chains):
        at = (where, fn, c)
        want = rc.yardstick(lik, v[c], y_of(c), sigma_of(c), z_limit)
        assert rc.same_bits(r["z"][c], want["z"]), at
        assert r["status"][c] == want["status"] == (rc.NONFINITE if c in flagged else 0), at
        for k in ("n_pos", "n_runs", "n_out", "max_index"):
            assert r[k][c] == want[k], (at, k, r[k][c], want[k])
        assert rc.same_bits(r["max_abs_z"][c], want["max_abs_z"]), at
        if c not in flagged:
            for k in ("chi2", "sum_z", "dw"):
                assert rc.same_bits(r[k][c], want[k]), (at, k, r[k][c], want[k])
    clean = [c for c in range(e.n_chains) if c not in flagged]
    for k in KEYS:              # the pointwise outputs change nothing
        assert same(bare[k][clean], r[k][clean]), (where, k)
    return r


def shared(y, sigma):
    return (lambda c: y), (lambda c: sigma)


# ---- 1. the line model: lanes, rows and blocks of the neighbour rule --------------------------------
def line_engine(mhx, n_chains, N, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(-4.0, 10.0, N) if N > 1 else np.array([2.5])
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    e = mhx.Engine(n_chains, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, x, y, sig)
    start = np.array([-1.0, 2.0]) * (1.0 + 0.02 * rng.standard_normal((n_chains, 2)))
    e.init_chains(start)
    return e, y, sig, start


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 2 * 256 + 3])
def test_line_model_lane_row_and_block_edges(mhx, N):
    capi, lib = mhx.capi, mhx.capi.lib()
    for n_chains in (9, 7):                # no multiple of the waves per workgroup
        e, y, sig, start = line_engine(mhx, n_chains, N, seed=N + n_chains)
        assert np.array_equal(e.state()["best_theta"], start)
        r0 = check(e, 0, None, rc.NORMAL, *shared(y, sig), where="most-likely")
        other = start * (1.0 + 0.01 * np.random.default_rng(N).standard_normal(start.shape))
        r1 = check(e, 0, other, rc.NORMAL, *shared(y, sig), z_limit=1.5, where="given")
        assert not rc.same_bits(r0["chi2"], r1["chi2"])
        assert same(check(e, 0, start, rc.NORMAL, *shared(y, sig), where="the same given")["dw"], r0["dw"])
        # outputs partly NULL: every other one, then the others
        full = {k: r0[k].copy() for k in KEYS + ("fit", "z")}
        order = ("fit", "z") + KEYS
        for keep in (0, 1):
            got = {k: np.zeros_like(full[k]) for i, k in enumerate(order) if i % 2 == keep}
            ptr = [got[k].ctypes.data_as(capi.i64p if got[k].dtype == np.int64 else
                                         capi.i32p if got[k].dtype == np.int32 else capi.f64p)
                   if k in got else None for k in order]
            assert lib.mhx_get_residuals(e._h, 0, None, 3.0, *ptr) == capi.OK
            for k in got:
                assert same(got[k], full[k]), (keep, k)
        assert lib.mhx_get_residuals(e._h, 0, None, 3.0, *([None] * 11)) == capi.OK
        assert e.summary_timing() >= 0.0
        e.close()


def test_hand_cases_through_the_device(mhx):
    """N = 1 gives dw = 0 and one run; z = (+1, -1, +1) gives three runs and dw = 8"""
    e = mhx.Engine(1, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [1.0], [0.5], [1.0])
    e.init_chains(np.array([0.0, 1.0]))
    r = check(e, 0, None, rc.NORMAL, *shared(np.array([0.5]), np.array([1.0])))
    assert (r["dw"][0], r["n_runs"][0], r["chi2"][0], r["max_index"][0]) == (0.0, 1, 0.25, 0)
    e.close()
    e = mhx.Engine(1, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    x, y = np.array([1.0, 2.0, 3.0]), np.array([0.0, 3.0, 2.0])
    e.set_dataset(0, x, y, np.ones(3))
    e.init_chains(np.array([0.0, 1.0]))
    r = check(e, 0, None, rc.NORMAL, *shared(y, np.ones(3)))
    assert list(r["z"][0]) == [1.0, -1.0, 1.0]
    assert (r["n_runs"][0], r["dw"][0], r["chi2"][0], r["sum_z"][0], r["n_pos"][0]) == (3, 8.0, 3.0, 1.0, 2)
    assert (r["max_abs_z"][0], r["max_index"][0]) == (1.0, 0)
    e.close()


# ---- 2. a split of the points -----------------------------------------------------------------------
def test_points_beyond_one_chunk(mhx):
    """the first block of the second chunk takes its neighbour from the chunk before"""
    N = CHUNK + 5
    rng = np.random.default_rng(1)
    x = np.linspace(-4.0, 10.0, N)
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    start = np.array([-1.0, 2.0]) * (1.0 + 0.002 * rng.standard_normal((3, 2)))
    # a change of sign exactly across the split, and the greatest |z| just beyond it (the chains'
    # lines lie within 0.1 of -1 + 2 x, sigma is at least 0.2: 50 and 60 sigma decide the signs)
    y[CHUNK - 1] += 50.0 * sig[CHUNK - 1]                # z < 0 for every chain
    y[CHUNK] -= 60.0 * sig[CHUNK]                        # z > 0
    y[CHUNK + 1] += 10.0 * sig[CHUNK + 1]
    e = mhx.Engine(3, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, x, y, sig)
    e.init_chains(start)
    r = check(e, 0, None, rc.NORMAL, *shared(y, sig))
    assert (r["status"] == 0).all() and (r["n_runs"] > 1000).all()
    assert (r["z"][:, CHUNK - 1] < -40.0).all() and (r["z"][:, CHUNK] > 50.0).all()
    assert list(r["max_index"]) == [CHUNK] * 3 and (r["max_abs_z"] > 50.0).all()
    e.close()


# ---- 3. planted extremes ----------------------------------------------------------------------------
def test_planted_extremes_ties_zeros_and_the_limit(mhx):
    N = 300
    rng = np.random.default_rng(3)
    x = np.arange(N, dtype=np.float64)
    zt = rng.integers(-8, 9, N) * 0.25                   # exact quarters within +-2
    zt[0], zt[N - 1] = 5.0, -5.0                          # two equal |z| maxima: the earlier wins
    zt[10], zt[11] = 0.0, -0.0
    zt[20], zt[21], zt[22] = 3.0, -3.0, 3.25              # the limit hit exactly is not counted
    y = x - zt                                            # sigma 1: z = v - y, exact
    e = mhx.Engine(3, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, x, y, np.ones(N))
    th = np.array([[0.0, 1.0], [-0.5, 1.0], [0.5, 1.0]])
    e.init_chains(th)
    assert np.array_equal(e.eval_function(0, th), x[None, :] + th[:, :1])
    r = check(e, 0, None, rc.NORMAL, *shared(y, np.ones(N)))
    assert np.array_equal(r["z"][0], zt) and r["z"][0][10] == 0.0
    assert list(r["max_abs_z"]) == [5.0, 5.5, 5.5] and list(r["max_index"]) == [0, N - 1, 0]
    inside = np.abs(zt[1:N - 1])
    assert r["n_out"][0] == 2 + int((inside > 3.0).sum()) == 3
    assert r["n_pos"][0] == int((zt > 0).sum())           # the zeros are not positive
    s = zt > 0
    assert r["n_runs"][0] == 1 + int((s[1:] != s[:-1]).sum())
    # z_limit: infinite and negative limits are numbers like any other
    assert list(e.residuals(0, z_limit=np.inf)["n_out"]) == [0, 0, 0]
    assert list(e.residuals(0, z_limit=-1.0)["n_out"]) == [N, N, N]
    e.close()


# ---- 4. every kernel path ---------------------------------------------------------------------------
def spread(s, n, seed, scale=0.02):
    return pb.perturbed(s.theta_star, n, scale, seed=seed)


def test_config2_two_peak_on_the_ahead_of_time_kernel(mhx):
    s = pb.two_peak(n=300, seed=3)
    e = s.engine(mhx, 6)
    th = spread(s, 6, 1)
    e.init_chains(th)
    assert "gauss22_normal" in e.kernel_name()
    _, y, sig, _ = s.data[0]
    check(e, 0, None, rc.NORMAL, *shared(y, sig))
    check(e, 0, spread(s, 6, 2), rc.NORMAL, *shared(y, sig), z_limit=2.0)
    e.close()


def test_the_cutoff_likelihood(mhx):
    s = pb.two_peak(n=257, seed=4, lik=pb.CUTOFF)
    e = s.engine(mhx, 6)
    e.init_chains(spread(s, 6, 3))
    assert "gauss22_cutoff" in e.kernel_name()
    _, y, sig, _ = s.data[0]
    check(e, 0, None, rc.CUTOFF, *shared(y, sig))
    e.close()


def test_the_generic_kernel(mhx, monkeypatch):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    s = pb.two_peak(n=200, seed=6)
    e = s.engine(mhx, 6)
    e.init_chains(spread(s, 6, 4))
    assert "generic" in e.kernel_name()
    _, y, sig, _ = s.data[0]
    check(e, 0, None, rc.NORMAL, *shared(y, sig))
    e.close()


def test_a_peak_count_specialised_at_run_time(mhx):
    rng = np.random.default_rng(6)
    th = np.array([0.5, 0.3, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08, 0.4, 0.5, 0.1])
    x = np.linspace(0.0, 1.0, 260)
    sig = rng.uniform(0.05, 0.15, x.size)
    y = pb.model_eval_np(pb.GAUSS, (2, 3), th, x) + sig * rng.standard_normal(x.size)
    s = pb.Spec(11)
    s.add(pb.GAUSS, (2, 3), range(11), x, y, sig, pb.NORMAL)
    s.theta_star = th
    e = s.engine(mhx, 6)
    e.init_chains(spread(s, 6, 5))
    assert "rtc[PeaksModel<2, 3, false>" in e.kernel_name()
    check(e, 0, None, rc.NORMAL, *shared(y, sig))
    e.close()


def expr_engine(mhx, n_chains, lik_expr=None):
    rng = np.random.default_rng(7)
    x = np.linspace(0.0, 3.0, 290)
    sig = rng.uniform(0.05, 0.2, x.size)
    th = np.array([2.0, 0.7, 1.5])
    y = th[0] * np.exp(-x / th[1]) + np.log(th[2] + x * x) + sig * rng.standard_normal(x.size)
    e = mhx.Engine(n_chains, 3, 1)
    e.set_expr_recognition(False)
    e.set_function_expr(0, "a*exp(-x/tau) + log(c + x*x)", ["a", "tau", "c"], [0, 1, 2])
    if lik_expr is None:
        e.set_dataset(0, x, y, sig)
    else:
        e.set_dataset(0, x, y, sig, likelihood=mhx.capi.LIK_EXPR)
        e.set_likelihood_expr(0, lik_expr)
    e.init_chains(pb.perturbed(th, n_chains, 0.03, seed=8))
    assert "rtc[expr" in e.kernel_name()
    return e, y, sig


def test_an_expression_compiled_as_written(mhx):
    e, y, sig = expr_engine(mhx, 6)
    check(e, 0, None, rc.NORMAL, *shared(y, sig))
    e.close()


def test_poisson_and_a_rate_that_is_not_positive(mhx):
    """Pearson residuals; a v_i <= 0 in one chain sets that chain's status and no other's"""
    s = pb.poisson_peaks(n=280)
    e = s.engine(mhx, 6)
    e.init_chains(s.theta_star)
    assert "gauss15_poisson" in e.kernel_name()
    _, y, _, _ = s.data[0]
    th = spread(s, 6, 9, 0.01)
    clean = check(e, 0, th, rc.POISSON, *shared(y, None))
    spoilt = th.copy()
    spoilt[4, 0] = -3.0                    # the background of chain 4 below zero: v < 0 between the peaks
    assert (e.eval_function(0, spoilt[4]) <= 0.0).any()
    r = check(e, 0, spoilt, rc.POISSON, *shared(y, None), flagged=(4,))
    assert list(r["status"]) == [0, 0, 0, 0, rc.NONFINITE, 0] and np.isnan(r["z"][4]).any()
    for k in KEYS + ("fit", "z"):
        for c in (0, 1, 2, 3, 5):
            assert same(r[k][c], clean[k][c]), (k, c)
    e.close()


# ---- 5. a dataset per walker ------------------------------------------------------------------------
NONE, SHARED, PER_CHAIN, PER_POINT = 0, 1, 2, 3


def plane_data(N, C, kind, seed):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 5.0, N)
    truth = np.array([1.0, 0.5]) + 0.3 * rng.standard_normal((C, 2))
    if kind == NONE:
        sigma, rows = None, np.ones((C, N))
    elif kind == SHARED:
        sigma = rng.uniform(0.05, 0.2, N)
        rows = np.tile(sigma, (C, 1))
    elif kind == PER_CHAIN:
        sigma = rng.uniform(0.05, 0.2, C)
        rows = np.repeat(sigma[:, None], N, axis=1)
    else:
        sigma = rows = rng.uniform(0.05, 0.2, (C, N))
    y = truth[:, :1] + truth[:, 1:] * x[None, :] + rows * rng.standard_normal((C, N))
    return x, y, sigma, rows, truth


@pytest.mark.parametrize("kind", [NONE, SHARED, PER_CHAIN, PER_POINT])
@pytest.mark.parametrize("N", [130, 300])           # pitch 256 and 384
def test_planes_every_sigma_kind_in_both_forms(mhx, monkeypatch, N, kind):
    C = 5
    x, y, sigma, rows, truth = plane_data(N, C, kind, seed=10 * N + kind)
    assert len({tuple(r) for r in y}) == C           # distinct rows: a wrong row gives other numbers
    runs = {}
    for no_lds in ("0", "1"):
        monkeypatch.setenv("MHX_PLANES_NO_LDS", no_lds)
        e = mhx.Engine(C, 2, 1)
        e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
        e.set_dataset_planes(0, x, y, sigma, kind)
        e.init_chains(truth)
        assert ("+planes(streamed)" if no_lds == "1" else "+planes(") in e.kernel_name()
        sig_of = (lambda c: None) if kind == NONE else (lambda c: rows[c])
        runs[no_lds] = check(e, 0, None, rc.NORMAL, lambda c: y[c], sig_of, where="planes %s" % no_lds)
        given = truth[::-1].copy()                   # every walker at another walker's parameters
        check(e, 0, given, rc.NORMAL, lambda c: y[c], sig_of, where="planes given")
        e.close()
    for k in KEYS + ("fit", "z"):
        assert same(runs["0"][k], runs["1"][k]), k
    assert len(set(runs["0"]["chi2"].tolist())) == C


@pytest.mark.parametrize("kind", [NONE, SHARED, PER_CHAIN, PER_POINT])
def test_planes_beyond_one_chunk_of_points(mhx, kind):
    """the second chunk of a dataset per walker: what a point indexes moves on to the chunk's first
    point - x, the walker's row of y, a shared sigma or the walker's row of it - and a walker's one
    sigma does not"""
    C, N = 2, CHUNK + 257
    x, y, sigma, rows, truth = plane_data(N, C, kind, seed=900 + kind)
    e = mhx.Engine(C, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset_planes(0, x, y, sigma, kind)
    e.init_chains(truth)
    sig_of = (lambda c: None) if kind == NONE else (lambda c: rows[c])
    r = check(e, 0, None, rc.NORMAL, lambda c: y[c], sig_of, where="planes, two chunks")
    assert r["z"].shape == (C, N) and r["chi2"][0] != r["chi2"][1]
    e.close()


def test_a_global_fit_mixing_a_plane_function_with_a_shared_one(mhx):
    C, N = 5, 130
    x, y, sigma, rows, truth = plane_data(N, C, PER_CHAIN, seed=77)
    rng = np.random.default_rng(78)
    x1 = np.linspace(-1.0, 1.0, 70)
    s1 = rng.uniform(0.1, 0.2, x1.size)
    y1 = 1.0 + 0.5 * x1 + s1 * rng.standard_normal(x1.size)
    e = mhx.Engine(C, 3, 2)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_function(1, mhx.capi.MODEL_POLY, (), [0, 2])
    e.set_dataset_planes(0, x, y, sigma, PER_CHAIN)
    e.set_dataset(1, x1, y1, s1)
    e.init_chains(np.column_stack([truth, truth[:, 1] + 0.1]))
    assert "+planes(" in e.kernel_name()
    check(e, 0, None, rc.NORMAL, lambda c: y[c], lambda c: rows[c], where="mixed, planes")
    check(e, 1, None, rc.NORMAL, *shared(y1, s1), where="mixed, shared")
    e.close()


# ---- 6. a group -------------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=270, seed=4)
    n = 11
    start = spread(s, n, 7)
    given = spread(s, n, 8)
    e = s.engine(mhx, n)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0])
    s.apply(g)
    e.init_chains(start)
    g.init_chains(start)
    for theta in (None, given):
        whole = g.residuals(0, theta, pointwise=True)
        one = e.residuals(0, theta, pointwise=True)
        parts = [x.residuals(0, None if theta is None else theta[f:f + k], pointwise=True)
                 for x, (f, k) in zip(g.engines, g.ranges)]
        for k in one:
            assert same(whole[k], one[k]), k
            assert same(whole[k], np.concatenate([p[k] for p in parts])), k
    e.close()
    g.close()
    # planes: every engine of the group reads its own rows
    C, N = 7, 130
    x, y, sigma, rows, truth = plane_data(N, C, PER_POINT, seed=5)
    e = mhx.Engine(C, 2, 1)
    g = mhx.Group(C, 2, 1, devices=[0, 0])
    for t in (e, g):
        t.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
        t.set_dataset_planes(0, x, y, sigma, PER_POINT)
        t.init_chains(truth)
    whole, one = g.residuals(0, pointwise=True), e.residuals(0, pointwise=True)
    for k in one:
        assert same(whole[k], one[k]), k
    e.close()
    g.close()


# ---- 7. the ABI's edges -----------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = mhx.Engine(2, 2, 1)
    e.set_function(0, capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0], np.full(5, 0.2))
    chi2 = np.full(2, 7.5)
    runs = np.full(2, -3, dtype=np.int32)
    fit = np.full((2, 5), 1.25)
    outs = (fit.ctypes.data_as(capi.f64p), None, chi2.ctypes.data_as(capi.f64p), None, None, None, None,
            None, runs.ctypes.data_as(capi.i32p), None, None)
    assert lib.mhx_get_residuals(e._h, 0, None, 3.0, *outs) == capi.ESTATE          # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    for fn in (-1, 1):
        assert lib.mhx_get_residuals(e._h, fn, None, 3.0, *outs) == capi.EINVAL
    assert lib.mhx_get_residuals(e._h, 0, None, float("nan"), *outs) == capi.EINVAL
    assert "z_limit" in lib.mhx_last_error().decode()
    assert lib.mhx_get_residuals(None, 0, None, 3.0, *outs) == capi.EINVAL
    assert list(chi2) == [7.5, 7.5] and list(runs) == [-3, -3] and (fit == 1.25).all()   # untouched on error
    assert lib.mhx_get_residuals(e._h, 0, None, 3.0, *outs) == capi.OK
    assert (chi2 != 7.5).all() and (runs >= 1).all() and (fit != 1.25).all()
    with pytest.raises(ValueError):
        e.residuals(0, np.zeros((3, 2)))
    e.close()
    # an expression likelihood: refused by name
    x, y, _ = expr_engine(mhx, 2, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")
    chi2[:] = 7.5
    assert lib.mhx_get_residuals(x._h, 0, None, 3.0, *((None,) + outs[1:])) == capi.EUNSUPPORTED
    assert "MHX_LIK_EXPR" in lib.mhx_last_error().decode() and list(chi2) == [7.5, 7.5]
    with pytest.raises(mhx.MhxError) as err:
        x.residuals(0)
    assert err.value.code == capi.EUNSUPPORTED
    x.close()


# ---- 8. the mirror ----------------------------------------------------------------------------------
def test_the_mirrors_residual_family(mhx):
    rng = np.random.default_rng(12)
    x = np.linspace(0.0, 1.0, 150)
    sig = np.full(x.size, 0.1)
    one = np.array([0.5, 0.3, 1.0, 0.4, 0.06])
    y = pb.model_eval_np(pb.GAUSS, (2, 1), one, x) + sig * rng.standard_normal(x.size)
    w = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"]]),
                          data=[x, y], params=[":b0", 0.5, ":b1", 0.3, ":a1", 1.0, ":mu1", 0.4, ":w1", 0.06],
                          data_error=0.1, n_chains=3, seed=2, history_capacity=1024)
    mhx.walker_adaptive_steps(w, 600)
    e = w.engine
    for sol in (":median", ":most-likely"):
        every = mhx.walker_set_get_residuals(w, take=400, which_solution=sol)
        assert len(every) == 3
        for c in range(3):
            mine = mhx.walker_get_residuals(w, take=400, chain=c, which_solution=sol)
            assert len(mine) == 3 and all(np.array_equal(a, b) for a, b in zip(mine, every[c])), (sol, c)
            assert np.array_equal(every[c][0], x) and np.array_equal(every[c][2], sig)
    assert mhx.walker_get_residuals(w, take=400, chain=1) == mhx.walker_set_get_residuals(w, take=400)[1]
    med = np.array([[p[k] for k in w.param_keys] for p in mhx.walker_set_get(w, ":median-params", take=400)])
    for sol, theta in ((":median", med), (":most-likely", None)):
        raw = e.residuals(0, theta, z_limit=2.0)
        gof = mhx.walker_set_goodness_of_fit(w, take=400, which_solution=sol, z_limit=2.0)
        for c in range(3):
            g = gof[c]
            assert set(g) == {"chi2", "dof", "reduced-chi2", "mean-z", "durbin-watson", "runs", "n-pos",
                              "runs-z", "max-z", "max-z-index", "n-out", "status"}
            assert g["chi2"] == raw["chi2"][c] and g["dof"] == 150 - 5
            assert g["reduced-chi2"] == raw["chi2"][c] / 145.0 and g["mean-z"] == raw["sum_z"][c] / 150.0
            assert g["durbin-watson"] == raw["dw"][c] / raw["chi2"][c]
            assert (g["runs"], g["n-pos"], g["n-out"]) == (raw["n_runs"][c], raw["n_pos"][c], raw["n_out"][c])
            assert g["runs-z"] == mhx.runs_z(g["n-pos"], 150 - g["n-pos"], g["runs"])
            assert (g["max-z"], g["max-z-index"], g["status"]) == (raw["max_abs_z"][c], raw["max_index"][c], 0)
            assert g == mhx.walker_goodness_of_fit(w, chain=c, take=400, which_solution=sol, z_limit=2.0)
    # a most-likely step that is not finite raises in the single-walker form, for that walker only
    pr, th = e.trace(1, 400)
    th[0] = 1e308
    pr[0] = 1e9                              # (the best of the walk: it becomes the most-likely step)
    e.set_history(1, pr, th)
    assert not np.isfinite(e.eval_function(0, e.state()["best_theta"][1])).all()
    with pytest.raises(FloatingPointError):
        mhx.walker_goodness_of_fit(w, chain=1, which_solution=":most-likely")
    assert mhx.walker_goodness_of_fit(w, chain=0, which_solution=":most-likely")["status"] == 0
    flags = [g["status"] for g in mhx.walker_set_goodness_of_fit(w, which_solution=":most-likely")]
    assert flags == [0, mhx.capi.RESID_NONFINITE, 0]
    e.close()
