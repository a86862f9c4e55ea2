"""mhx_get_candidate_scores on the device, bit for bit and exactly, with no tolerance anywhere:

  score        the serial sum over the selected functions (cand_cases.total) of the chi2 that
               Engine.residuals - one call per candidate, the read-out this one batches - returns on
               the same engine; and once, independently, of resid_cases.yardstick's chi2 on
               Engine.eval_function's values
  best_index,
  best_score,
  n_bad        cand_cases.rank of those scores

Covered: the lane, row and block edges of the line model with 1 .. 65 candidates and 1 .. 16 kept,
candidates per chain and planted ties, points beyond 2^17, a call of two portions, every kernel
path, a Poisson rate that is not positive, datasets per walker in all four sigma kinds, global fits,
a group, the ABI's edges, the mirror's search and maps, and the acceptance case of the search:
eleven spectra whose dips lie up to four widths from the guess."""
import math

import numpy as np
import pytest

import cand_cases as cc
import problems as pb
import resid_cases as rc

pytestmark = pytest.mark.gpu

INF = math.inf
B = 1 << 26                     # kStageBudget


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.CAND_KEEP_MAX == cc.KEEP_MAX
    return lisp_mcmc_amd


def per_chain(e, cand):
    cand = np.asarray(cand, dtype=np.float64)
    return cand if cand.ndim == 3 else np.broadcast_to(cand, (e.n_chains,) + cand.shape)


def reference(e, cand, fn=-1):
    """score [n_chains, m] from Engine.residuals, one call per candidate and selected function"""
    rows = per_chain(e, cand)
    fns = range(e.K) if fn < 0 else [fn]
    score = np.zeros(rows.shape[:2])
    for j in range(rows.shape[1]):
        rs = [e.residuals(k, np.ascontiguousarray(rows[:, j])) for k in fns]
        for c in range(e.n_chains):
            score[c, j] = cc.total([r["chi2"][c] for r in rs], any(r["status"][c] != 0 for r in rs))
    return score


def check(e, cand, fn=-1, keeps=(1, 3, 16), want=None, where=""):
    """Engine.candidate_scores against the reference and the ranking rule; returns the scores"""
    want = reference(e, cand, fn) if want is None else want
    for keep in keeps:
        r = e.candidate_scores(cand, fn=fn, keep=keep, scores=True)
        bare = e.candidate_scores(cand, fn=fn, keep=keep)
        assert set(r) == {"score", "best_index", "best_score", "n_bad"} and set(bare) == set(r) - {"score"}
        assert r["best_index"].shape == r["best_score"].shape == (e.n_chains, keep)
        assert rc.same_bits(r["score"], want), (where, keep, np.argwhere(r["score"] != want)[:4])
        for c in range(e.n_chains):
            idx, val, bad = cc.rank(want[c], keep)
            assert np.array_equal(r["best_index"][c], idx), (where, keep, c, r["best_index"][c], idx)
            assert rc.same_bits(r["best_score"][c], val), (where, keep, c)
            assert r["n_bad"][c] == bad, (where, keep, c)
        for k in bare:              # asking for the scores changes nothing
            assert np.array_equal(bare[k], r[k]), (where, keep, k)
    return want


# ---- 1. the line model: lanes, rows and blocks, few and many candidates ------------------------------
def line_engine(mhx, n_chains, N, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(-4.0, 10.0, N) if N > 1 else np.array([2.5])
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    e = mhx.Engine(n_chains, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, x, y, sig)
    e.init_chains(np.array([-1.0, 2.0]) * (1.0 + 0.02 * rng.standard_normal((n_chains, 2))))
    return e, x, y, sig


def line_candidates(m, seed):
    return np.array([-1.0, 2.0]) * (1.0 + 0.05 * np.random.default_rng(seed).standard_normal((m, 2)))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 515])
def test_line_model_shared_candidates(mhx, N):
    e, x, y, sig = line_engine(mhx, 3, N, seed=N)
    for m in (1, 2, 7, 64, 65):
        cand = line_candidates(m, 100 * N + m)
        want = check(e, cand, fn=0 if m == 2 else -1, where="N %d m %d" % (N, m))
        assert np.isfinite(want).all() and (len(set(want[0].tolist())) == m)
        assert (want == want[0]).all()              # the same data and candidates: the same bits
        if m == 7:                                  # keep > m: the rest is (-1, +inf)
            r = e.candidate_scores(cand, keep=9)
            assert (r["best_index"][:, 7:] == -1).all() and (r["best_score"][:, 7:] == INF).all()
            assert sorted(r["best_index"][0, :7].tolist()) == list(range(7))
    assert e.summary_timing() >= 0.0
    e.close()


def test_the_scores_from_the_definition_alone(mhx):
    """resid_cases.yardstick on mhx_eval_function's values: no read-out of the engine is trusted"""
    e, x, y, sig = line_engine(mhx, 3, 257, seed=5)
    cand = line_candidates(7, 6)
    v = e.eval_function(0, cand)                                            # [m, N]
    want = np.array([cc.total([rc.yardstick(rc.NORMAL, v[j], y, sig)["chi2"]]) for j in range(7)])
    check(e, cand, want=np.tile(want, (3, 1)), where="yardstick")
    e.close()


# ---- 2. candidates per chain, and ties ---------------------------------------------------------------
def test_per_chain_candidates_are_the_shared_ones_chain_by_chain_and_ties_go_to_the_smaller_index(mhx):
    e, x, y, sig = line_engine(mhx, 5, 300, seed=2)
    m = 11
    cand = np.array([line_candidates(m, 40 + c) for c in range(5)])         # [5, m, 2]
    cand[:, 8] = cand[:, 2]                                                 # the same vector twice
    cand[:, 5] = cand[:, 2]                                                 # ... three times
    cand[3, 0] = cand[3, 10]
    want = check(e, cand, keeps=(1, 4, 11), where="per chain")
    assert len({tuple(r) for r in want}) == 5                               # every chain its own candidates
    own = e.candidate_scores(cand, keep=m, scores=True)
    for c in range(5):
        as_shared = e.candidate_scores(cand[c], keep=m, scores=True)
        for k in own:
            assert np.array_equal(own[k][c], as_shared[k][c]), (c, k)
        assert want[c, 2] == want[c, 5] == want[c, 8]
        order = own["best_index"][c].tolist()
        at = order.index(2)
        assert order[at:at + 3] == [2, 5, 8]                                # equal scores: ascending index
    order = own["best_index"][3].tolist()
    assert order.index(0) + 1 == order.index(10)
    e.close()


# ---- 3. many points, many chains -------------------------------------------------------------------
def test_points_beyond_one_chunk_of_the_residuals(mhx):
    """2^17 + 300 points: mhx_get_residuals works through two chunks, this call through 514 blocks"""
    e, x, y, sig = line_engine(mhx, 2, (1 << 17) + 300, seed=9)
    check(e, line_candidates(3, 10), keeps=(1, 3), where="chunk boundary")
    e.close()


def test_a_call_of_two_portions(mhx):
    n, N, m, keep = 300, 2560, 3000, 2
    nb = (N + rc.BLOCK - 1) // rc.BLOCK
    per_item = 8 * m * 2 + 4 + 4 * keep + 8 * keep + 8 * m + 8 * m * nb     # carve_cand, a chain
    portion = (B - 6 * 256) // per_item
    assert 1 <= portion < 180 + 120 <= 2 * portion and portion > 180         # two portions; the cut is in [180, 300)
    e, x, y, sig = line_engine(mhx, n, N, seed=12)
    cand = np.array([-1.0, 2.0]) * (1.0 + 0.05 * np.random.default_rng(13).standard_normal((n, m, 2)))
    big = e.candidate_scores(cand, keep=keep, scores=True)
    e.close()
    # the chains across the cut on an engine that takes them in one portion (the data are shared)
    e, _, _, _ = line_engine(mhx, 120, N, seed=12)
    few = e.candidate_scores(cand[180:], keep=keep, scores=True)
    for k in few:
        assert np.array_equal(big[k][180:], few[k]), k
    check(e, cand[180:, :5], keeps=(2,), where="two portions")                # and those against the residuals
    assert rc.same_bits(few["score"][:, :5], e.candidate_scores(cand[180:, :5], scores=True)["score"])
    e.close()


# ---- 4. every kernel path --------------------------------------------------------------------------
def spread(s, n, seed, scale=0.02):
    return pb.perturbed(s.theta_star, n, scale, seed=seed)


def run_spec(mhx, s, name, n=7, seed=1):
    e = s.engine(mhx, n)
    e.init_chains(spread(s, n, seed))
    assert name in e.kernel_name(), e.kernel_name()
    want = check(e, spread(s, 9, seed + 1, 0.05), keeps=(1, 4), where=name)
    assert np.isfinite(want).all()
    own = np.array([spread(s, 9, seed + 2 + c, 0.05) for c in range(n)])
    check(e, own, keeps=(3,), where=name + ", per chain")
    e.close()


def test_two_peak_on_the_ahead_of_time_kernel(mhx):
    run_spec(mhx, pb.two_peak(n=334, seed=3), "gauss22_normal", n=11)


def test_the_generic_kernel(mhx, monkeypatch):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    run_spec(mhx, pb.two_peak(n=334, seed=6), "generic", n=5)


def test_the_cutoff_likelihood(mhx):
    run_spec(mhx, pb.two_peak(n=257, seed=4, lik=pb.CUTOFF), "gauss22_cutoff")


def test_three_peaks_specialised_at_run_time(mhx):
    rng = np.random.default_rng(6)
    th = np.array([0.5, 0.3, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08, 0.4, 0.5, 0.1])
    x = np.linspace(0.0, 1.0, 334)
    sig = rng.uniform(0.05, 0.15, x.size)
    y = pb.model_eval_np(pb.GAUSS, (2, 3), th, x) + sig * rng.standard_normal(x.size)
    s = pb.Spec(11)
    s.add(pb.GAUSS, (2, 3), range(11), x, y, sig, pb.NORMAL)
    s.theta_star = th
    run_spec(mhx, s, "rtc[PeaksModel<2, 3, false>")


def test_lorentzians(mhx):
    rng = np.random.default_rng(7)
    th = np.array([0.2, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08])
    x = np.linspace(0.0, 1.0, 600)
    sig = rng.uniform(0.05, 0.15, x.size)
    y = pb.model_eval_np(pb.LORENTZ, (1, 2), th, x) + sig * rng.standard_normal(x.size)
    s = pb.Spec(7)
    s.add(pb.LORENTZ, (1, 2), range(7), x, y, sig, pb.NORMAL)
    s.theta_star = th
    run_spec(mhx, s, "PeaksModel<1, 2, true>")


def expr_engine(mhx, n_chains, likelihood_expr=None):
    rng = np.random.default_rng(11)
    n = 334
    X = np.column_stack([rng.uniform(-1, 2, n), rng.uniform(0, 3, n)])
    th = np.array([0.4, 1.3, -0.7, 0.25])
    sig = rng.uniform(0.1, 0.3, n)
    y = th[0] + th[1] * X[:, 0] + th[2] * X[:, 1] + th[3] * X[:, 0] * X[:, 1] + sig * rng.standard_normal(n)
    e = mhx.Engine(n_chains, 4, 1)
    e.set_expr_recognition(False)
    e.set_function_expr(0, "a + b*xcol0 + c*xcol1 + d*xcol0*xcol1", list("abcd"), [0, 1, 2, 3])
    if likelihood_expr is None:
        e.set_dataset(0, X, y, sig)
    else:
        e.set_dataset(0, X, y, sig, likelihood=mhx.capi.LIK_EXPR)
        e.set_likelihood_expr(0, likelihood_expr)
    e.init_chains(pb.perturbed(th, n_chains, 0.05, seed=2))
    assert "rtc[expr" in e.kernel_name(), e.kernel_name()
    return e, th


def test_an_expression_compiled_as_written_over_two_columns_of_x(mhx):
    e, th = expr_engine(mhx, 6)
    check(e, pb.perturbed(th, 9, 0.1, seed=3), keeps=(1, 4), where="expression")
    check(e, np.array([pb.perturbed(th, 9, 0.1, seed=4 + c) for c in range(6)]), keeps=(2,), where="expression, own")
    e.close()


def test_poisson_and_a_rate_that_is_not_positive(mhx):
    """one candidate's rate falls below zero between the peaks: its score is +inf, it counts in n_bad
    and ranks last; no other candidate's score moves"""
    s = pb.poisson_peaks(n=280)
    e = s.engine(mhx, 6)
    e.init_chains(s.theta_star)
    assert "gauss15_poisson" in e.kernel_name()
    cand = spread(s, 9, 9, 0.01)
    clean = check(e, cand, keeps=(1, 9), where="poisson")
    assert np.isfinite(clean).all()
    spoilt = cand.copy()
    spoilt[4, 0] = -3.0
    assert (e.eval_function(0, spoilt[4]) <= 0.0).any()
    got = check(e, spoilt, keeps=(1, 9), where="poisson, spoilt")
    assert (got[:, 4] == INF).all()
    rest = [j for j in range(9) if j != 4]
    assert rc.same_bits(got[:, rest], clean[:, rest])
    r = e.candidate_scores(spoilt, keep=9)
    assert list(r["n_bad"]) == [1] * 6 and (r["best_index"][:, 8] == 4).all() and (r["best_score"][:, 8] == INF).all()
    assert (r["best_score"][:, :8] < INF).all()
    e.close()


# ---- 5. a dataset per walker -----------------------------------------------------------------------
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
@pytest.mark.parametrize("N", [65, 334])
def test_planes_every_sigma_kind(mhx, N, kind):
    C = 11
    x, y, sigma, rows, truth = plane_data(N, C, kind, seed=10 * N + kind)
    e = mhx.Engine(C, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset_planes(0, x, y, sigma, kind)
    e.init_chains(truth)
    assert "+planes(" in e.kernel_name()
    rng = np.random.default_rng(N + kind)
    cand = np.array([1.0, 0.5]) + 0.3 * rng.standard_normal((9, 2))
    want = check(e, cand, keeps=(1, 4), where="planes, shared candidates")
    assert len({tuple(r) for r in want}) == C            # every walker its own data
    # ... and as a yardstick of its own: walker c's data, from the values alone
    v = e.eval_function(0, cand)
    for c in (0, C - 1):
        mine = [cc.total([rc.yardstick(rc.NORMAL, v[j], y[c], None if kind == NONE else rows[c])["chi2"]])
                for j in range(9)]
        assert rc.same_bits(want[c], mine), c
    own = truth[:, None, :] + 0.1 * rng.standard_normal((C, 9, 2))
    check(e, own, keeps=(3,), where="planes, per chain")
    e.close()


# ---- 6. global fits ----------------------------------------------------------------------------------
def test_two_functions_that_share_a_parameter(mhx):
    rng = np.random.default_rng(3)
    x0, x1 = np.linspace(0.0, 5.0, 300), np.linspace(-1.0, 1.0, 70)
    s0, s1 = rng.uniform(0.05, 0.2, x0.size), rng.uniform(0.1, 0.2, x1.size)
    y0 = 1.0 + 0.5 * x0 + s0 * rng.standard_normal(x0.size)
    y1 = 1.0 - 0.3 * x1 + s1 * rng.standard_normal(x1.size)
    C = 5
    e = mhx.Engine(C, 3, 2)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_function(1, mhx.capi.MODEL_POLY, (), [0, 2])
    e.set_dataset(0, x0, y0, s0)
    e.set_dataset(1, x1, y1, s1)
    e.init_chains(np.array([1.0, 0.5, -0.3]) * (1.0 + 0.05 * rng.standard_normal((C, 3))))
    cand = np.array([1.0, 0.5, -0.3]) * (1.0 + 0.1 * rng.standard_normal((9, 3)))
    both = check(e, cand, fn=-1, keeps=(1, 4), where="both")
    a = check(e, cand, fn=0, keeps=(2,), where="function 0")
    b = check(e, cand, fn=1, keeps=(2,), where="function 1")
    assert rc.same_bits(both, (0.0 + a) + b) and not rc.same_bits(both, a)
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
    cand = np.array([1.0, 0.5, 0.6]) + 0.3 * rng.standard_normal((9, 3))
    both = check(e, cand, fn=-1, keeps=(1, 4), where="mixed")
    a, b = check(e, cand, fn=0, keeps=(1,)), check(e, cand, fn=1, keeps=(1,))
    assert rc.same_bits(both, (0.0 + a) + b)
    assert (b == b[0]).all() and len({tuple(r) for r in a}) == C          # the shared function, the planes
    e.close()


# ---- 7. a group ------------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=270, seed=4)
    n = 11
    start = spread(s, n, 7)
    e = s.engine(mhx, n)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0])
    s.apply(g)
    e.init_chains(start)
    g.init_chains(start)
    shared = spread(s, 9, 8, 0.05)
    own = np.array([spread(s, 9, 20 + c, 0.05) for c in range(n)])
    for cand in (shared, own):
        whole = g.candidate_scores(cand, keep=4, scores=True)
        one = e.candidate_scores(cand, keep=4, scores=True)
        for k in one:
            assert np.array_equal(whole[k], one[k]), k
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
    cand = truth[:, None, :] + 0.1 * np.random.default_rng(6).standard_normal((C, 9, 2))
    whole, one = g.candidate_scores(cand, keep=3, scores=True), e.candidate_scores(cand, keep=3, scores=True)
    for k in one:
        assert np.array_equal(whole[k], one[k]), k
    assert len(set(one["best_score"][:, 0].tolist())) == C
    e.close()
    g.close()


# ---- 8. the ABI's edges ----------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = mhx.Engine(2, 2, 1)
    e.set_function(0, capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0], np.full(5, 0.2))
    cand = np.array([[-1.0, 2.0], [0.0, 1.5], [-1.0, 2.1]])
    cp = cand.ctypes.data_as(capi.f64p)
    score = np.full((2, 3), 7.5)
    index = np.full((2, 2), -3, dtype=np.int32)
    best = np.full((2, 2), 1.25)
    bad = np.full(2, -5, dtype=np.int32)
    outs = (score.ctypes.data_as(capi.f64p), index.ctypes.data_as(capi.i32p), best.ctypes.data_as(capi.f64p),
            bad.ctypes.data_as(capi.i32p))
    call = lib.mhx_get_candidate_scores
    assert call(e._h, 0, cp, 3, 0, 2, *outs) == capi.ESTATE                  # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    assert call(e._h, 0, cp, 0, 0, 2, *outs) == capi.EINVAL                  # m = 0
    assert call(e._h, 0, cp, -1, 0, 2, *outs) == capi.EINVAL
    for keep in (0, 17, -1):
        assert call(e._h, 0, cp, 3, 0, keep, *outs) == capi.EINVAL
        assert "keep" in lib.mhx_last_error().decode()
    for fn in (-2, 1):
        assert call(e._h, fn, cp, 3, 0, 2, *outs) == capi.EINVAL
    assert call(e._h, 0, None, 3, 0, 2, *outs) == capi.EINVAL                # cand NULL
    assert call(None, 0, cp, 3, 0, 2, *outs) == capi.EINVAL
    assert (score == 7.5).all() and (index == -3).all() and (best == 1.25).all() and (bad == -5).all()
    assert call(e._h, 0, cp, 3, 0, 2, *outs) == capi.OK
    want = reference(e, cand, 0)
    assert rc.same_bits(score, want) and list(bad) == [0, 0]
    for c in range(2):
        idx, val, _ = cc.rank(want[c], 2)
        assert np.array_equal(index[c], idx) and rc.same_bits(best[c], val)
    # every output NULL, then one at a time; fn -1 and 16 kept of 3
    assert call(e._h, -1, cp, 3, 0, 16, None, None, None, None) == capi.OK
    for k in range(4):
        fresh = [np.zeros_like(a) for a in (score, index, best, bad)]
        ptr = [fresh[i].ctypes.data_as(capi.f64p if fresh[i].dtype == np.float64 else capi.i32p) if i == k else None
               for i in range(4)]
        assert call(e._h, -1, cp, 3, 0, 2, *ptr) == capi.OK
        assert np.array_equal(fresh[k], (score, index, best, bad)[k]), k
    with pytest.raises(ValueError):
        e.candidate_scores(np.zeros((3, 3)))
    with pytest.raises(mhx.MhxError) as err:
        e.candidate_scores(cand, fn=5)
    assert err.value.code == capi.EINVAL
    e.close()
    # an expression likelihood: refused by name, for the function alone and among all
    x, _ = expr_engine(mhx, 2, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")
    c4 = np.zeros((3, 4))
    score[:] = 7.5
    for fn in (0, -1):
        assert call(x._h, fn, c4.ctypes.data_as(capi.f64p), 3, 0, 2, *outs) == capi.EUNSUPPORTED
        assert "MHX_LIK_EXPR" in lib.mhx_last_error().decode() and (score == 7.5).all()
    with pytest.raises(mhx.MhxError) as err:
        x.candidate_scores(c4)
    assert err.value.code == capi.EUNSUPPORTED
    x.close()


# ---- 9. the mirror, and the acceptance case ------------------------------------------------------------
KEYS = ["bg", "a1", "mu1", "w1", "a2", "mu2", "w2"]
GUESS = np.array([0.2, 1.0, 0.3, 0.03, 0.7, 0.7, 0.04])


def spectra(mhx):
    """eleven spectra of 334 points: two Lorentzians on a constant, widths 0.03 and 0.04, the centres
    drawn up to four widths from the guess every walker starts at"""
    rng = np.random.default_rng(13)
    C, N = 11, 334
    x = np.linspace(0.0, 1.0, N)
    mu1, mu2 = rng.uniform(0.15, 0.45, C), rng.uniform(0.55, 0.85, C)
    truth = np.column_stack([np.full(C, 0.2), np.full(C, 1.0), mu1, np.full(C, 0.03), np.full(C, 0.7), mu2,
                             np.full(C, 0.04)])
    sigma = rng.uniform(0.02, 0.04, C)
    y = np.array([pb.model_eval_np(pb.LORENTZ, (1, 2), truth[c], x) for c in range(C)])
    y = y + sigma[:, None] * rng.standard_normal((C, N))
    w = mhx.walker_set_create(function=mhx.models.lorentz_peaks(["bg"], [["a1", "mu1", "w1"], ["a2", "mu2", "w2"]]),
                              datasets=[[x, y[c]] for c in range(C)],
                              params=[dict(zip(KEYS, GUESS)) for c in range(C)],
                              data_error=[float(s) for s in sigma], seed=3)
    assert np.array_equal(w.engine.state()["best_theta"], np.tile(GUESS, (C, 1)))
    return w, x, y, sigma


def lorentz_jacobian(th, x):
    J = [np.ones_like(x)]
    for k in range(2):
        A, mu, w = th[1 + 3 * k: 4 + 3 * k]
        t = (x - mu) / w
        q = 1.0 / (1.0 + t * t)
        J += [q, A * q * q * 2.0 * t / w, A * q * q * 2.0 * t * t / w]
    return np.array(J)


def grid_9x9(mhx):
    return mhx.candidate_grid(dict(zip(KEYS, GUESS)), {"mu1": np.linspace(0.1, 0.5, 9), "mu2": np.linspace(0.5, 0.9, 9)})


def test_the_mirrors_search_and_maps(mhx):
    w, x, y, sigma = spectra(mhx)
    e, C = w.engine, 11
    cand, shape = grid_9x9(mhx)
    assert shape == (9, 9)
    want = reference(e, cand)
    found = mhx.walker_set_search(w, candidates=cand, keep=4)
    lp = np.array([e.logpost(np.ascontiguousarray(np.tile(cand[j], (C, 1)))) for j in range(81)]).T   # [C, 81]
    for c in range(C):
        idx, val, _ = cc.rank(want[c], 4)
        best = idx[int(np.argmax(lp[c, idx]))]                      # the greatest log-posterior of the kept
        s = found[c]
        assert set(s) == {"params", "index", "chi2", "logpost", "n-bad"}
        assert s["index"] == best and s["chi2"] == want[c, best] and s["logpost"] == lp[c, best] and s["n-bad"] == 0
        assert list(s["params"]) == KEYS and list(s["params"].values()) == cand[best].tolist()
        assert mhx.walker_search(w, chain=c, candidates=cand, keep=4) == s
    plain = mhx.walker_set_search(w, candidates=cand, keep=1, with_prior=False)
    assert [s["index"] for s in plain] == [int(cc.rank(want[c], 1)[0][0]) for c in range(C)]
    assert all(s["logpost"] is None for s in plain)
    # axes: every walker's own most-likely vector (here the guess) with the keys replaced - the same grid
    by_axes = mhx.walker_set_search(w, axes={"mu1": np.linspace(0.1, 0.5, 9), "mu2": np.linspace(0.5, 0.9, 9)}, keep=4)
    assert by_axes == found
    # a map around each walker's own solution: the per-candidate residuals at the substituted vectors
    axes = {"mu2": np.array([0.6, 0.7, 0.8]), "a1": np.array([0.9, 1.1])}
    cm = mhx.walker_set_chi2_map(w, axes)
    assert cm["chi2"].shape == (C, 3, 2) and list(cm["axes"]) == ["mu2", "a1"]
    for i, v2 in enumerate(axes["mu2"]):
        for j, a1 in enumerate(axes["a1"]):
            th = np.tile(GUESS, (C, 1))
            th[:, 5], th[:, 1] = v2, a1
            assert rc.same_bits(cm["chi2"][:, i, j], 0.0 + e.residuals(0, th)["chi2"]), (i, j)
    assert rc.same_bits(cm["delta-chi2"], cm["chi2"] - cm["chi2"].reshape(C, -1).min(axis=1)[:, None, None])
    one = mhx.walker_set_chi2_map(w, {"mu1": np.linspace(0.2, 0.4, 5)})
    assert one["chi2"].shape == (C, 5)
    # apply=True: the walkers stand at the winners
    assert np.array_equal(e.state()["theta"], np.tile(GUESS, (C, 1)))
    mhx.walker_set_search(w, candidates=cand, keep=4, apply=True)
    winners = np.array([cand[s["index"]] for s in found])
    st = e.state()
    assert np.array_equal(st["theta"], winners) and np.array_equal(st["best_theta"], winners)
    e.close()


def test_search_then_polish_reaches_every_least_squares_point(mhx):
    """the acceptance case.  On the CPU restatement (numpy normal equations, the same least_squares):
    the polish alone left 10 of these 11 walkers at reduced chi-square 3 .. 82; after the 9 x 9 search
    every walker ended at Newton decrement <= 3e-16 and reduced chi-square 0.91 .. 1.10"""
    w, x, y, sigma = spectra(mhx)
    e, C, N = w.engine, 11, 334

    def reduced(theta):
        return e.residuals(0, np.ascontiguousarray(theta))["chi2"] / (N - 7)

    def decrement(th, c):
        g = lorentz_jacobian(th, x) / sigma[c]
        u = (y[c] - pb.model_eval_np(pb.LORENTZ, (1, 2), th, x)) / sigma[c]
        b = g @ u
        return float(b @ np.linalg.solve(g @ g.T, b))
    alone = mhx.walker_set_least_squares(w, iterations=25)
    print("the polish alone: reduced chi-square %s" % np.round(reduced(alone["theta"]), 2).tolist())
    assert (reduced(alone["theta"]) > 1.5).any()                     # local: the wrong basin keeps its walkers
    cand, _ = grid_9x9(mhx)
    found = mhx.walker_set_search(w, candidates=cand, keep=4, apply=True)
    start = np.array([list(s["params"].values()) for s in found])
    assert np.array_equal(e.state()["best_theta"], start)
    r = mhx.walker_set_least_squares(w, iterations=25)
    dec = [decrement(r["theta"][c], c) for c in range(C)]
    red = reduced(r["theta"])
    print("search, then polish: greatest Newton decrement %.3g, reduced chi-square %s"
          % (max(dec), np.round(red, 2).tolist()))
    assert max(dec) <= 1e-8
    assert (red <= 1.5).all()
    again = mhx.walker_set_least_squares(w, iterations=25, theta0=start)      # theta0: the same start, given
    assert np.array_equal(again["theta"], r["theta"])
    e.close()
