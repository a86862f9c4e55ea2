"""mhx_get_waic on the device against the numpy yardstick of its definition (tests/waic_cases.py),
chain by chain, from the model values mhx_eval_function returns at the steps of mhx_get_trace:

  pw_acc = (M, S, mean, M2)  bit for bit
  pw_p = M2 / (n - 1)        bit for bit
  pw_lppd                    within 2^-52 |L| + 2^-53 |lppd_i| of M + ln(S / n) from mpmath, L = ln(S / n)
                             with the quotient taken in binary64 first: one ulp for the engine's log
                             (the bound tests/test_device_math_cpu.py pins) plus the final addition
  lppd, p_waic               within N 2^-53 sum |term_i| of math.fsum of the pointwise outputs
  elpd                       bit for bit the totals' difference
  n_high, n_used, status     exactly

over every kernel path (ahead-of-time, generic, run-time specialised, expressions, an expression
likelihood), windows that straddle the wrap point of a ring a real walk has filled, takes above a
chain's length, one-step and empty windows, blocks of points that are not whole, a split of the
points, a non-finite step, a group, the ABI's edges and the mirror's walker_set_waic family."""
import math

import numpy as np
import pytest

import problems as pb
import waic_cases as wc

pytestmark = pytest.mark.gpu

PTS = wc.BLOCK // 64            # kWaicPts: the points of a lane
CHUNK = 1 << 17                 # kFitChunkPoints
U = 2.0 ** -53


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.WAIC_BLOCK == wc.BLOCK
    return lisp_mcmc_amd


def crafted(rng, n, centre, spread):
    """a Metropolis-like walk, newest first: runs of repeated steps"""
    centre = np.asarray(centre, float)
    prob, theta = np.empty(n), np.empty((n, centre.size))
    p, th = 0.0, centre.copy()
    for i in range(n):
        if i == 0 or rng.random() < 0.4:
            p = rng.normal(-50.0, 3.0)
            th = centre * (1.0 + spread * rng.standard_normal(centre.size))
        prob[i], theta[i] = p, th
    return prob[::-1].copy(), theta[::-1].copy()


def check_lppd(got, M, quot, where):
    import mpmath
    mpmath.mp.prec = 120
    for i in range(len(got)):
        L = mpmath.log(mpmath.mpf(float(quot[i])))
        ref = mpmath.mpf(float(M[i])) + L
        tol = 2.0 ** -52 * abs(float(L)) + U * abs(float(ref))
        assert abs(float(mpmath.mpf(float(got[i])) - ref)) <= tol, (where, i, float(got[i]), float(ref))


def check_totals(r, c, where):
    N = r["pw_lppd"].shape[1]
    lp, pp = r["pw_lppd"][c], r["pw_p"][c]
    assert abs(r["lppd"][c] - math.fsum(lp)) <= N * U * math.fsum(np.abs(lp)), where
    if np.isnan(pp).any():
        assert np.isnan(r["p_waic"][c]), where
    else:
        assert abs(r["p_waic"][c] - math.fsum(pp)) <= N * U * math.fsum(np.abs(pp)), where
    want = r["lppd"][c] - r["p_waic"][c]         # (a NaN - one step - is a NaN, whatever its payload)
    assert wc.same_bits(r["elpd"][c], want) or (np.isnan(want) and np.isnan(r["elpd"][c])), where
    with np.errstate(invalid="ignore"):
        assert r["n_high"][c] == int((pp > 0.4).sum()), where


def check(e, fn, take, lik, y, sigma, chains=None, flagged=(), **kw):
    """Engine.waic of function fn against the yardstick on `chains` (None: all)"""
    r = e.waic(fn, take, pointwise=True, accumulators=True)
    for c in (range(e.n_chains) if chains is None else chains):
        where = (fn, take, c)
        _, th = e.trace(c, take)
        n = len(th)
        assert r["n_used"][c] == n, where
        if c in flagged:
            assert r["status"][c] & wc.NONFINITE, where
            continue
        ell = wc.terms(lik, e.eval_function(fn, th), y, sigma, **kw)
        want = wc.yardstick(ell)
        assert want["status"] == (wc.ONE_STEP if n == 1 else 0), where       # (nothing crafted is not finite)
        assert r["status"][c] == want["status"], where
        assert wc.same_bits(r["pw_acc"][c], want["acc"]), where
        assert wc.same_bits(r["pw_p"][c], want["pw_p"]), where
        check_lppd(r["pw_lppd"][c], want["acc"][:, 0], want["quot"], where)
        check_totals(r, c, where)
    return r


# ---- 1. the line model: blocks, windows, takes -----------------------------------------------------
def line_engine(mhx, n_chains, N, ring, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(-4.0, 10.0, N) if N > 1 else np.array([2.5])
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    e = mhx.Engine(n_chains, 2, 1, history_capacity=ring)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, x, y, sig)
    e.init_chains(np.array([-1.0, 2.0]))
    return e, y, sig


LENGTHS = [1, 2, 3, 64, 65, 150, 300]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 64 * PTS - 1, 64 * PTS + 1, 2 * 64 * PTS + 3])
def test_line_model_blocks_windows_and_takes(mhx, N):
    rng = np.random.default_rng(N)
    # (history_capacity 64 and 256 are what is asked for; the engine never makes a ring shorter
    # than its adaptation window, so both hold 1024 steps, and a history that is SET lies in the
    # ring's first slots however long it was: none of these windows crosses the wrap point.  The
    # windows that do are test_a_real_walk_in_a_wrapped_ring's.)
    for ring, extra in ((64, [1500, 40]), (256, [])):
        lengths = LENGTHS + extra             # nine chains and seven: no multiple of the waves per group
        e, y, sig = line_engine(mhx, len(lengths), N, ring, seed=N)
        cap = e.history_capacity()
        assert cap >= ring
        for c, n in enumerate(lengths):
            e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.05))
        held = e.state()["length"]
        assert list(held[:7]) == LENGTHS
        for take in (1, 2, 3, 64, 256):
            r = check(e, 0, take, wc.NORMAL, y, sig)
            assert list(r["n_used"][:7]) == [min(take, n) for n in LENGTHS]
            assert list(r["status"][:7]) == [wc.ONE_STEP if min(take, n) == 1 else 0 for n in LENGTHS]
        if extra:       # the widest window the ring serves, of a walk longer than the ring
            check(e, 0, cap, wc.NORMAL, y, sig, chains=[7, 8])
        e.close()


def test_five_chains_and_the_hand_case_through_the_device(mhx):
    rng = np.random.default_rng(5)
    e, y, sig = line_engine(mhx, 5, 130, 64)
    for c in range(5):
        e.set_history(c, *crafted(rng, 20 + 7 * c, [-1.0, 2.0], 0.05))
    check(e, 0, 64, wc.NORMAL, y, sig)
    e.close()
    # one point, y = 0, sigma = 1, the values 0 (newest) and 2: a line through x = 1
    h = mhx.Engine(1, 2, 1)
    h.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    h.set_dataset(0, [1.0], [0.0], [1.0])
    h.init_chains(np.array([0.0, 0.0]))
    h.set_history(0, [-1.0, -2.0], [[0.0, 0.0], [1.0, 1.0]])
    assert list(h.eval_function(0, np.array([[0.0, 0.0], [1.0, 1.0]])).ravel()) == [0.0, 2.0]
    r = check(h, 0, 2, wc.NORMAL, [0.0], [1.0])
    c = -0.9189385332046727
    M, S, mean, m2 = r["pw_acc"][0, 0]
    assert (M, mean, m2) == (c, c - 1.0, 2.0) and r["pw_p"][0, 0] == 2.0 and r["p_waic"][0] == 2.0
    assert abs(S - (1.0 + math.exp(-2.0))) <= 2 * U
    assert abs(r["pw_lppd"][0, 0] - -1.4851577027216454) <= 4 * U
    assert r["n_high"][0] == 1 and r["n_used"][0] == 2 and r["status"][0] == 0
    h.close()


# ---- 2. every kernel path ---------------------------------------------------------------------------
def fill(e, rng, centre, spread, lengths):
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted(rng, n, centre, spread))


SIX = [1, 2, 40, 97, 150, 130]


def test_config2_two_peak_on_the_ahead_of_time_kernel(mhx):
    s = pb.two_peak(n=300, seed=3)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "gauss22_normal" in e.kernel_name()
    fill(e, np.random.default_rng(1), s.theta_star, 0.02, SIX)
    _, y, sig, _ = s.data[0]
    for take in (150, 64):
        check(e, 0, take, wc.NORMAL, y, sig)
    e.close()


def test_the_cutoff_likelihood_clamps_terms(mhx):
    s = pb.two_peak(n=257, seed=4, lik=pb.CUTOFF)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "gauss22_cutoff" in e.kernel_name()
    rng = np.random.default_rng(2)
    _, y, sig, _ = s.data[0]
    for c, n in enumerate(SIX):
        pr, th = crafted(rng, n, s.theta_star, 0.02)
        th[::3, 0] += 30.0            # every third step's background is far off: its terms clamp
        e.set_history(c, pr, th)
    _, th = e.trace(4, 150)
    ell = wc.terms(wc.CUTOFF, e.eval_function(0, th), y, sig)
    assert (ell == -5000.0).any() and (ell > -5000.0).any()
    check(e, 0, 150, wc.CUTOFF, y, sig)
    e.close()


@pytest.mark.parametrize("logfact_double", [False, True])
def test_five_peak_poisson(mhx, logfact_double):
    s = pb.poisson_peaks(n=280)
    e = s.engine(mhx, 6, history_capacity=64, poisson_logfact_double=logfact_double)
    e.init_chains(s.theta_star)
    assert "gauss15_poisson" in e.kernel_name()
    fill(e, np.random.default_rng(3), s.theta_star, 0.01, SIX)
    _, y, _, _ = s.data[0]
    for c in range(6):                # (mirror_tlog restates the table branch: every rate clear of 1)
        assert (e.eval_function(0, e.trace(c, 150)[1]) > 1.0625).all()
    check(e, 0, 150, wc.POISSON, y, None, logfact_double=logfact_double)
    e.close()


def test_the_generic_kernel(mhx, monkeypatch):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    s = pb.two_peak(n=200, seed=6)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "generic" in e.kernel_name()
    fill(e, np.random.default_rng(4), s.theta_star, 0.02, SIX)
    _, y, sig, _ = s.data[0]
    check(e, 0, 150, wc.NORMAL, y, sig)
    e.close()
    p = pb.poisson_peaks(n=130)
    e = p.engine(mhx, 3, history_capacity=64)
    e.init_chains(p.theta_star)
    assert "generic" in e.kernel_name()
    fill(e, np.random.default_rng(5), p.theta_star, 0.01, [1, 30, 66])
    check(e, 0, 150, wc.POISSON, p.data[0][1], None)
    e.close()


def test_a_peak_count_specialised_at_run_time(mhx):
    rng = np.random.default_rng(6)
    th = np.array([0.5, 0.3, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08, 0.4, 0.5, 0.1])
    x = np.linspace(0.0, 1.0, 260)
    sig = rng.uniform(0.05, 0.15, x.size)
    y = pb.model_eval_np(pb.GAUSS, (2, 3), th, x) + sig * rng.standard_normal(x.size)
    s = pb.Spec(11)
    s.add(pb.GAUSS, (2, 3), range(11), x, y, sig, pb.NORMAL)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(th)
    assert "rtc[PeaksModel<2, 3, false>" in e.kernel_name()
    fill(e, rng, th, 0.02, SIX)
    check(e, 0, 150, wc.NORMAL, y, sig)
    e.close()


def expr_engine(mhx, n_chains, lik_expr=None):
    rng = np.random.default_rng(7)
    x = np.linspace(0.0, 3.0, 290)
    sig = rng.uniform(0.05, 0.2, x.size)
    th = np.array([2.0, 0.7, 1.5])
    y = th[0] * np.exp(-x / th[1]) + np.log(th[2] + x * x) + sig * rng.standard_normal(x.size)
    e = mhx.Engine(n_chains, 3, 1, history_capacity=64)
    e.set_expr_recognition(False)
    e.set_function_expr(0, "a*exp(-x/tau) + log(c + x*x)", ["a", "tau", "c"], [0, 1, 2])
    if lik_expr is None:
        e.set_dataset(0, x, y, sig)
    else:
        e.set_dataset(0, x, y, sig, likelihood=mhx.capi.LIK_EXPR)
        e.set_likelihood_expr(0, lik_expr)
    e.init_chains(th)
    assert "rtc[expr" in e.kernel_name()
    fill(e, rng, th, 0.03, SIX[:n_chains])
    return e, y, sig


def test_an_expression_compiled_as_written(mhx):
    e, y, sig = expr_engine(mhx, 6)
    check(e, 0, 150, wc.NORMAL, y, sig)
    e.close()


def test_an_expression_likelihood(mhx):
    e, y, sig = expr_engine(mhx, 6, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")

    def term(yy, m, err):
        d = (yy - m) / err
        return 0.0 - (0.5 * (d * d))
    check(e, 0, 150, wc.EXPR, y, sig, lik_term=term)
    e.close()


def test_two_columns_of_x_take_the_constants_from_the_host(mhx):
    """a second column of x sits where the normal likelihood's constants would: the call uploads them"""
    rng = np.random.default_rng(11)
    n = 270
    X = np.column_stack([rng.uniform(-1, 2, n), rng.uniform(0, 3, n)])
    th = np.array([0.4, 1.3, -0.7, 0.25])
    sig = rng.uniform(0.1, 0.3, n)
    y = th[0] + th[1] * X[:, 0] + th[2] * X[:, 1] + th[3] * X[:, 0] * X[:, 1] + sig * rng.standard_normal(n)
    e = mhx.Engine(3, 4, 1, history_capacity=64)
    e.set_function_expr(0, "a + b*xcol0 + c*xcol1 + d*xcol0*xcol1", list("abcd"), [0, 1, 2, 3])
    e.set_dataset(0, X, y, sig)
    e.init_chains(th)
    fill(e, rng, th, 0.05, [2, 33, 120])
    check(e, 0, 150, wc.NORMAL, y, sig)
    e.close()


def test_a_two_function_global_fit_once_per_function(mhx):
    s = pb.global_fit(n_each=140, n_sets=2)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "pvoigt2" in e.kernel_name()
    fill(e, np.random.default_rng(8), s.theta_star, 0.01, SIX)
    for fn in (0, 1):
        _, y, sig, _ = s.data[fn]
        check(e, fn, 150, wc.NORMAL, y, sig)
    e.close()


# ---- 3. a real walk ---------------------------------------------------------------------------------
def test_a_real_walk_in_a_wrapped_ring(mhx):
    s = pb.two_peak(n=600, seed=6)
    e = s.engine(mhx, 64, seed=3, history_capacity=2048)
    e.init_chains(pb.perturbed(s.theta_star, 64, 0.01, seed=9))
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(3200)
    R = e.history_capacity()
    length = e.state()["length"]
    assert int(length.min()) >= 3000 and int(length.max()) < 2 * R and R == 2048
    _, y, sig, _ = s.data[0]
    r = check(e, 0, 300, wc.NORMAL, y, sig, chains=[0, 21, 42, 63])
    assert (r["status"] == 0).all() and (r["n_used"] == 300).all()
    assert (r["p_waic"] > 0).all() and (r["lppd"] >= r["elpd"]).all()
    # Windows that straddle the ring's wrap point.  Nothing has cut this walk since init_chains,
    # so every step taken was pushed: entry k sits in slot k mod R, the newest in slot
    # (length - 1) mod R, and a window of `take` steps passes slot 0 into slot R - 1 exactly when
    # that slot number is below take - 1.  One chain over the whole ring, one over a window that
    # ends 150 steps beyond the wrap.
    newest = (length - 1) & (R - 1)
    for c, take in ((7, R), (50, int(newest[50]) + 151)):
        assert 0 <= newest[c] < take - 1 <= R - 1 and length[c] >= take, (c, newest[c], take)
        check(e, 0, take, wc.NORMAL, y, sig, chains=[c])
    whole = e.waic(0, R)
    assert (whole["status"] == 0).all() and (whole["n_used"] == R).all() and (whole["p_waic"] > 0).all()
    print("waic 64 chains take 2048 N 600: kernels %.3f ms" % e.summary_timing())
    e.close()


# ---- 4. a split of the points -----------------------------------------------------------------------
def test_points_beyond_one_chunk(mhx):
    N = CHUNK + 300
    e, y, sig = line_engine(mhx, 2, N, 64, seed=1)
    rng = np.random.default_rng(9)
    for c in range(2):
        e.set_history(c, *crafted(rng, 3, [-1.0, 2.0], 0.05))
    r = e.waic(0, 3, pointwise=True)
    assert (r["status"] == 0).all() and list(r["n_used"]) == [3, 3]
    for c in range(2):
        check_totals(r, c, ("split", c))
    # the far side of the split against the yardstick, and the totals' bits without pointwise outputs
    _, th = e.trace(1, 3)
    ell = wc.terms(wc.NORMAL, e.eval_function(0, th)[:, CHUNK - 5:], y[CHUNK - 5:], sig[CHUNK - 5:])
    assert wc.same_bits(r["pw_p"][1, CHUNK - 5:], wc.yardstick(ell)["pw_p"])
    bare = e.waic(0, 3)
    for k in ("elpd", "lppd", "p_waic"):
        assert wc.same_bits(bare[k], r[k]), k
    assert np.array_equal(bare["n_high"], r["n_high"])
    e.close()


# ---- 5. a step that is not finite -------------------------------------------------------------------
def test_a_non_finite_step_flags_its_chain_only(mhx):
    rng = np.random.default_rng(10)
    walks = [crafted(rng, 30, [-1.0, 2.0], 0.1) for _ in range(3)]
    runs = []
    for spoil in (False, True):
        e, y, sig = line_engine(mhx, 3, 70, 64, seed=2)
        for c, (pr, th) in enumerate(walks):
            th = th.copy()
            if spoil and c == 1:
                th[11] = [1e308, 1e308]
            e.set_history(c, pr, th)
        runs.append(e.waic(0, 30, pointwise=True, accumulators=True))
        if spoil:
            check(e, 0, 30, wc.NORMAL, y, sig, flagged=(1,))
        e.close()
    clean, spoilt = runs
    assert list(clean["status"]) == [0, 0, 0] and list(spoilt["status"]) == [0, 1, 0]
    for k in ("elpd", "lppd", "p_waic", "pw_lppd", "pw_p", "pw_acc"):
        for c in (0, 2):
            assert wc.same_bits(clean[k][c], spoilt[k][c]), (k, c)


def test_an_empty_window_is_flagged(mhx):
    """:burn-walks may take every step of a walk: n_used 0 and MHX_WAIC_NONFINITE, the others untouched"""
    rng = np.random.default_rng(13)
    e, y, sig = line_engine(mhx, 3, 70, 64, seed=3)
    for c, n in enumerate((3, 5, 9)):
        e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.1))
    e.modify("burn-walks", 3)
    assert list(e.state()["length"]) == [0, 2, 6]
    r = check(e, 0, 64, wc.NORMAL, y, sig, flagged=(0,))
    assert list(r["n_used"]) == [0, 2, 6] and list(r["status"]) == [wc.NONFINITE, 0, 0]
    e.close()


# ---- 6. a group -------------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=270, seed=4)
    n = 11
    rng = np.random.default_rng(7)
    walks = [crafted(rng, int(k), s.theta_star, 0.02) for k in rng.integers(1, 200, n)]
    e = s.engine(mhx, n, history_capacity=64)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0], history_capacity=64)
    s.apply(g)
    e.init_chains(s.theta_star)
    g.init_chains(s.theta_star)
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
        i = 0 if c < g.ranges[1][0] else 1
        g.engines[i].set_history(c - g.ranges[i][0], pr, th)
    for take in (1, 150):
        whole = g.waic(0, take, pointwise=True, accumulators=True)
        one = e.waic(0, take, pointwise=True, accumulators=True)
        parts = [x.waic(0, take, pointwise=True, accumulators=True) for x in g.engines]
        for k in one:
            if one[k].dtype == np.float64:
                assert wc.same_bits(whole[k], one[k]), (take, k)
                assert wc.same_bits(whole[k], np.concatenate([p[k] for p in parts])), (take, k)
            else:
                assert np.array_equal(whole[k], one[k]), (take, k)
                assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), (take, k)
    e.close()
    g.close()


# ---- 7. the ABI's edges -----------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = mhx.Engine(2, 2, 1, history_capacity=64)
    e.set_function(0, capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0], np.full(5, 0.2))
    none = (None,) * 9
    elpd = np.full(2, 7.5)
    used = np.full(2, -3, dtype=np.int32)
    outs = (elpd.ctypes.data_as(capi.f64p), None, None, None, None, None, None,
            used.ctypes.data_as(capi.i32p), None)
    assert lib.mhx_get_waic(e._h, 0, 5, *outs) == capi.ESTATE           # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    cap = e.history_capacity()
    for take in (0, -1, cap + 1):
        assert lib.mhx_get_waic(e._h, 0, take, *outs) == capi.EINVAL
    for fn in (-1, 1):
        assert lib.mhx_get_waic(e._h, fn, 5, *outs) == capi.EINVAL
    assert lib.mhx_get_waic(None, 0, 5, *outs) == capi.EINVAL
    assert list(elpd) == [7.5, 7.5] and list(used) == [-3, -3]           # untouched on error
    assert lib.mhx_get_waic(e._h, 0, 5, *none) == capi.OK                # all-NULL outputs
    assert e.summary_timing() >= 0.0
    assert lib.mhx_get_waic(e._h, 0, 5, *outs) == capi.OK
    assert list(used) == [1, 1] and np.isnan(elpd).all()       # (one step: p_waic is the IEEE 0/0)
    r = e.waic(0, 5)
    assert list(r["status"]) == [capi.WAIC_ONE_STEP] * 2 and np.isnan(r["p_waic"]).all()
    e.close()
    # a dataset per walker: refused by name
    p = mhx.Engine(2, 2, 1, history_capacity=64)
    p.set_function(0, capi.MODEL_POLY, (), [0, 1])
    x = np.linspace(0.0, 1.0, 9)
    p.set_dataset_planes(0, x, np.vstack([1.0 + 2.0 * x, 1.5 + x]))
    p.init_chains(np.array([1.0, 2.0]))
    elpd[:] = 7.5
    assert lib.mhx_get_waic(p._h, 0, 5, *outs) == capi.EUNSUPPORTED
    assert "planes" in lib.mhx_last_error().decode() and list(elpd) == [7.5, 7.5]
    with pytest.raises(mhx.MhxError) as err:
        p.waic(0, 5)
    assert err.value.code == capi.EUNSUPPORTED
    p.close()


# ---- 8. the mirror ----------------------------------------------------------------------------------
KEYS8 = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]


def test_the_mirrors_waic_family(mhx):
    rng = np.random.default_rng(12)
    x = np.linspace(0.0, 1.0, 150)
    sig = np.full(x.size, 0.1)
    one = np.array([0.5, 0.3, 1.0, 0.4, 0.06])
    y = pb.model_eval_np(pb.GAUSS, (2, 1), one, x) + sig * rng.standard_normal(x.size)
    w1 = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"]]),
                           data=[x, y], params=[":b0", 0.5, ":b1", 0.3, ":a1", 1.0, ":mu1", 0.4, ":w1", 0.06],
                           data_error=sig, n_chains=3, seed=2, history_capacity=1024)
    p2 = []
    for k, v in zip(KEYS8, [0.5, 0.3, 1.0, 0.4, 0.06, 0.1, 0.7, 0.08]):
        p2 += [":" + k, v]
    w2 = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"], ["a2", "mu2", "w2"]]),
                           data=[x, y], params=p2, data_error=sig, n_chains=3, seed=3, history_capacity=1024)
    for w in (w1, w2):
        mhx.walker_adaptive_steps(w, 800)
    every = mhx.walker_set_waic(w1, take=500, pointwise=True)
    assert len(every) == 3
    raw = w1.engine.waic(0, 500, pointwise=True)
    for c in range(3):
        mine = mhx.walker_waic(w1, chain=c, take=500, pointwise=True)
        assert set(mine) == {"elpd", "lppd", "p-waic", "waic", "n-high", "n-used", "status", "pointwise", "se"}
        for k in mine:
            assert np.array_equal(mine[k], every[c][k]), (c, k)
        assert mine["waic"] == -2.0 * mine["elpd"] and mine["elpd"] == raw["elpd"][c]
        assert mine["n-used"] == 500 and mine["status"] == 0 and mine["pointwise"].shape == (150,)
        assert wc.same_bits(mine["pointwise"], raw["pw_lppd"][c] - raw["pw_p"][c])
        assert mine["se"] == float(np.sqrt(150 * np.var(mine["pointwise"], ddof=1)))
        assert "pointwise" not in mhx.walker_waic(w1, chain=c, take=500)
    # one-peak data under a one-peak and a two-peak model: numbers of the right shape (which model
    # wins, and by what margin, nobody has measured: no assertion about it)
    cmp_ = mhx.waic_compare(mhx.walker_waic(w1, take=500, pointwise=True),
                            mhx.walker_waic(w2, take=500, pointwise=True))
    assert set(cmp_) == {"elpd-diff", "se"} and all(np.isfinite(v) for v in cmp_.values())
    print("waic_compare one peak against two on one-peak data: %r" % (cmp_,))
    # a step that is not finite raises, as walker_get_data_and_fit does
    pr, th = w1.engine.trace(1, 500)
    th[3] = 1e308
    w1.engine.set_history(1, pr, th)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_waic(w1, take=500)
    with pytest.raises(FloatingPointError):
        mhx.walker_waic(w1, chain=1, take=500)
    assert mhx.walker_waic(w1, chain=0, take=500)["status"] == 0
