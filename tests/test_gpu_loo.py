"""mhx_get_loo on the device against the numpy yardstick of its definition (tests/loo_cases.py),
chain by chain, from the model values mhx_eval_function returns at the steps of mhx_get_trace:

  tail, pw_acc's T_1, l_cut, S_b   bit for bit (at a sample of each chain's points: the ends, the
                                   borders of the waves and blocks, a few between)
  pw_lppd, lppd                    bit for bit Engine.waic's on the same engine, every point
  n_used, status                   exactly; n_high against the device's own pw_khat
  khat, sigma, pw_elpd             against mpmath at 120 bits fed the device's own (tail, l_cut, S_b):
                                   within 8 times the distance the yardstick keeps from mpmath
                                   (loo_cases.DEV_*, measured by tests/test_loo_host.py) plus 8 ulp of
                                   the value
  elpd_loo, lppd                   within N 2^-53 sum |term_i| of math.fsum of the pointwise outputs
                                   (and bit for bit loo_cases.block_sum of them: the definition's order)
  p_loo                            bit for bit the totals' difference

over windows with and without a tail, the caller's tail lengths, a ring of 8192 (M = 272, the columns
read from the stage), a chain that never moved, a non-finite step, every kernel path, a wrapped ring,
MHX_LOO_NO_LDS=1, a call split into portions and chunks of points, a group, the ABI's edges and the
mirror's walker_set_loo family."""
import math

import numpy as np
import pytest

import loo_cases as lc
import problems as pb
import waic_cases as wc
from test_gpu_waic import SIX, crafted, expr_engine, fill, line_engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FLOATS = ("elpd_loo", "p_loo", "lppd", "pw_elpd", "pw_khat", "pw_lppd", "pw_acc", "tail")
INTS = ("n_high", "n_used", "status")


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.LOO_BLOCK == lc.BLOCK
    return lisp_mcmc_amd


def sample_points(N, seed, k=3):
    """the ends, the borders of the waves and of the blocks, and k points between"""
    edge = [p for p in (0, 1, 62, 63, 64, 65, 255, 256, 257, N - 2, N - 1) if 0 <= p < N]
    rng = np.random.default_rng(seed)
    return sorted(set(edge[:2] + edge[-2:] + [p for p in edge if p % 64 in (63, 0)][:4] +
                      list(rng.integers(0, N, k))))


def ulp(v):
    return math.ulp(abs(float(v)))


def check_against_mpmath(n, tail, acc, khat, elpd, where):
    import mpmath
    mpmath.mp.prec = 120
    k_mp, s_mp, e_mp, fitted = lc.estimate_mp(n, tail, acc[1], acc[2])
    assert fitted == bool(np.isfinite(khat)), where
    if fitted:
        assert abs(float(mpmath.mpf(float(khat)) - k_mp)) <= 8 * lc.DEV_KHAT + 8 * ulp(khat), (where, khat, float(k_mp))
        assert abs(float(mpmath.mpf(float(acc[3])) - s_mp)) <= 8 * lc.DEV_SIGMA * float(s_mp) + 8 * ulp(acc[3]), \
            (where, acc[3], float(s_mp))
    else:
        assert acc[3] == 0.0, where
    assert abs(float(mpmath.mpf(float(elpd)) - e_mp)) <= 8 * lc.DEV_ELPD + 8 * ulp(elpd), (where, elpd, float(e_mp))


def check_totals(r, c, k_limit, where):
    N = r["pw_elpd"].shape[1]
    for tot, pw in (("elpd_loo", "pw_elpd"), ("lppd", "pw_lppd")):
        t = r[pw][c]
        if np.isfinite(t).all():
            assert abs(r[tot][c] - math.fsum(t)) <= N * U * math.fsum(np.abs(t)), (where, tot)
            assert lc.same_bits(r[tot][c], lc.block_sum(t)), (where, tot)
        else:
            assert np.isnan(r[tot][c]), (where, tot)
    want = r["lppd"][c] - r["elpd_loo"][c]
    assert lc.same_bits(r["p_loo"][c], want) or (np.isnan(want) and np.isnan(r["p_loo"][c])), where
    assert r["n_high"][c] == int((r["pw_khat"][c] > k_limit).sum()), where


def check(e, fn, take, lik, y, sigma, tail_len=0, k_limit=0.7, chains=None, flagged=(), n_mp=1, **kw):
    """Engine.loo of function fn against the yardstick on `chains` (None: all)"""
    r = e.loo(fn, take, tail=tail_len, k_limit=k_limit, pointwise=True, accumulators=True)
    w = e.waic(fn, take, pointwise=True)
    N = r["pw_elpd"].shape[1]
    P = lc.tail_length(take, tail_len)
    assert r["tail"].shape == (e.n_chains, N, P)
    y = np.asarray(y, dtype=np.float64)
    sig = None if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), y.shape)
    for c in (range(e.n_chains) if chains is None else chains):
        where = (fn, take, tail_len, c)
        _, th = e.trace(c, take)
        n = len(th)
        assert r["n_used"][c] == n == w["n_used"][c], where
        if c in flagged:
            assert r["status"][c] & lc.NONFINITE, where
            continue
        M = lc.tail_length(n, tail_len)
        assert lc.same_bits(r["pw_lppd"][c], w["pw_lppd"][c]) and lc.same_bits(r["lppd"][c], w["lppd"][c]), where
        assert np.isnan(r["tail"][c][:, M:]).all() and not np.isnan(r["tail"][c][:, :M]).any(), where
        flat = bool(np.isinf(r["pw_khat"][c]).any()) and M > 0
        assert r["status"][c] == (lc.SHORT if n < 25 else 0) | (lc.FLAT if flat else 0) | (lc.EMPTY if n == 0 else 0), where
        check_totals(r, c, k_limit, where)
        if n == 0:
            assert np.isnan(r["pw_elpd"][c]).all() and np.isinf(r["pw_khat"][c]).all(), where
            continue
        pts = sample_points(N, 1000 * take + c)
        ell = wc.terms(lik, e.eval_function(fn, th)[:, pts], y[pts], None if sig is None else sig[pts], **kw)
        want = lc.yardstick(ell, tail_len, k_limit)
        assert want["M"] == M and not want["status"] & lc.NONFINITE, where      # (nothing crafted is not finite)
        assert lc.same_bits(r["tail"][c][pts][:, :M], want["tail"]), where
        assert lc.same_bits(r["pw_acc"][c][pts][:, :3], want["acc"][:, :3]), where
        assert np.array_equal(np.isfinite(r["pw_khat"][c][pts]), want["fitted"]), where
        # (the yardstick itself, at every sampled point: the same x_k, another logarithm)
        f = want["fitted"]
        got_k, got_s, got_e = r["pw_khat"][c][pts], r["pw_acc"][c][pts][:, 3], r["pw_elpd"][c][pts]
        assert (np.abs(got_k[f] - want["pw_khat"][f]) <= 8 * lc.DEV_KHAT + 8 * np.spacing(np.abs(got_k[f]))).all(), where
        assert (np.abs(got_s[f] - want["acc"][f, 3]) <= (8 * lc.DEV_SIGMA + 8 * 2 * U) * got_s[f]).all(), where
        assert (got_s[~f] == 0.0).all(), where
        assert (np.abs(got_e - want["pw_elpd"]) <= 8 * lc.DEV_ELPD + 8 * np.spacing(np.abs(got_e))).all(), where
        for p in pts[::max(1, len(pts) // n_mp)][:n_mp]:
            check_against_mpmath(n, r["tail"][c][p][:M], r["pw_acc"][c][p], r["pw_khat"][c][p], r["pw_elpd"][c][p],
                                 where + (p,))
    return r


# ---- 1. the line model: blocks, windows, takes, tails -----------------------------------------------
LENGTHS = [1, 2, 24, 25, 64, 65, 150, 300, 1500]


@pytest.mark.parametrize("N", [1, 63, 65, 257, 515])
def test_line_model_blocks_windows_takes_and_tails(mhx, N):
    rng = np.random.default_rng(N)
    for lengths, combos in ((LENGTHS, [(1, 0), (24, 0), (25, 0), (64, 0), (256, 0), (1024, 0), (256, 5), (256, 40),
                                       (1024, 40)]),
                            (LENGTHS[2:], [(25, 5), (1024, 0)])):      # nine chains and seven
        e, y, sig = line_engine(mhx, len(lengths), N, 64, seed=N)
        for c, n in enumerate(lengths):
            e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.05))
        assert list(e.state()["length"]) == [min(n, 1024) for n in lengths]     # (the ring holds 1024)
        for take, tail_len in combos:
            r = check(e, 0, take, wc.NORMAL, y, sig, tail_len=tail_len)
            assert list(r["n_used"]) == [min(take, n) for n in lengths]
            short = [lc.SHORT if min(take, n) < 25 else 0 for n in lengths]
            assert [int(s) & lc.SHORT for s in r["status"]] == short
        e.close()


def test_a_ring_of_8192_has_a_tail_of_272_and_reads_the_stage(mhx):
    rng = np.random.default_rng(8192)
    e, y, sig = line_engine(mhx, 3, 65, 8192, seed=4)
    assert e.history_capacity() == 8192
    for c, n in enumerate((8192, 8192, 5000)):
        e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.05))
    assert lc.tail_length(8192) == 272
    r = check(e, 0, 8192, wc.NORMAL, y, sig, chains=[0, 2])
    assert list(r["n_used"]) == [8192, 8192, 5000] and r["tail"].shape[2] == 272
    check(e, 0, 8192, wc.NORMAL, y, sig, tail_len=1024, chains=[1])        # (M = 1024 and 1000: the longest sort)
    e.close()


# ---- 2. a chain that never moved; a step that is not finite ------------------------------------------
def test_a_chain_that_never_moved_comes_back_clean(mhx):
    e, y, sig = line_engine(mhx, 2, 70, 64, seed=5)
    rng = np.random.default_rng(5)
    e.set_history(0, np.full(40, -3.0), np.tile([-1.02, 2.01], (40, 1)))
    e.set_history(1, *crafted(rng, 40, [-1.0, 2.0], 0.05))
    r = check(e, 0, 64, wc.NORMAL, y, sig)
    # (the walk beside it: ties across the cut of a tail of 8 can leave x* = 0 at a point, which check()
    # holds to the yardstick point by point)
    assert r["status"][0] == lc.FLAT and r["status"][1] & ~lc.FLAT == 0 and r["n_high"][0] == 70
    ell = wc.terms(wc.NORMAL, e.eval_function(0, np.array([[-1.02, 2.01]])), y, sig)
    assert lc.same_bits(r["pw_elpd"][0], ell[0]) and np.isinf(r["pw_khat"][0]).all()
    assert lc.same_bits(r["pw_acc"][0][:, 2], np.full(70, 32.0)) and (r["pw_acc"][0][:, 3] == 0.0).all()
    assert e.loo(0, 64, k_limit=np.inf)["n_high"][0] == 0
    e.close()


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
        runs.append(e.loo(0, 30, pointwise=True, accumulators=True))
        if spoil:
            check(e, 0, 30, wc.NORMAL, y, sig, flagged=(1,))
        e.close()
    clean, spoilt = runs
    assert (clean["status"] & ~lc.FLAT == 0).all() and spoilt["status"][1] & lc.NONFINITE
    assert spoilt["status"][0] == clean["status"][0] and spoilt["status"][2] == clean["status"][2]
    for k in FLOATS:
        for c in (0, 2):
            assert lc.same_bits(clean[k][c], spoilt[k][c]), (k, c)


def test_an_empty_window(mhx):
    rng = np.random.default_rng(13)
    e, y, sig = line_engine(mhx, 3, 70, 64, seed=3)
    for c, n in enumerate((3, 5, 40)):
        e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.1))
    e.modify("burn-walks", 3)
    assert list(e.state()["length"]) == [0, 2, 37]
    r = check(e, 0, 64, wc.NORMAL, y, sig)
    assert list(r["n_used"]) == [0, 2, 37] and r["status"][0] == lc.SHORT | lc.EMPTY and r["status"][1] == lc.SHORT
    e.close()


# ---- 3. every kernel path -----------------------------------------------------------------------------
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


def test_five_peak_poisson(mhx):
    s = pb.poisson_peaks(n=280)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "gauss15_poisson" in e.kernel_name()
    fill(e, np.random.default_rng(3), s.theta_star, 0.01, SIX)
    _, y, _, _ = s.data[0]
    for c in range(6):                # (mirror_tlog restates the table branch: every rate clear of 1)
        assert (e.eval_function(0, e.trace(c, 150)[1]) > 1.0625).all()
    check(e, 0, 150, wc.POISSON, y, None)
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


# ---- 4. a real walk ---------------------------------------------------------------------------------
def test_a_real_walk_in_a_wrapped_ring(mhx):
    s = pb.two_peak(n=300, seed=6)
    e = s.engine(mhx, 16, seed=3, history_capacity=2048)
    e.init_chains(pb.perturbed(s.theta_star, 16, 0.01, seed=9))
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(3200)
    R = e.history_capacity()
    length = e.state()["length"]
    assert int(length.min()) >= 3000 and int(length.max()) < 2 * R and R == 2048
    _, y, sig, _ = s.data[0]
    r = check(e, 0, 300, wc.NORMAL, y, sig, chains=[0, 15])
    assert (r["status"] & ~lc.FLAT == 0).all() and (r["n_used"] == 300).all()
    # a window over the whole ring passes the wrap point (test_gpu_waic has the slot arithmetic)
    newest = (length - 1) & (R - 1)
    assert 0 <= newest[7] < R - 1
    check(e, 0, R, wc.NORMAL, y, sig, chains=[7])
    whole = e.loo(0, R)
    assert (whole["n_used"] == R).all() and (whole["p_loo"] > 0).all()
    print("loo 16 chains take 2048 N 300: kernels %.3f ms, khat > 0.7 at %s points"
          % (e.summary_timing(), list(whole["n_high"])))
    e.close()


# ---- 5. LDS against the stage; portions and chunks ------------------------------------------------------
def test_keys_in_lds_and_keys_from_the_stage_give_the_same_bits(mhx, monkeypatch):
    lengths = [1, 24, 25, 65, 300, 1000, 1024]
    runs = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("MHX_LOO_NO_LDS", knob)          # (read when the problem is finalised)
        rng = np.random.default_rng(21)
        e, y, sig = line_engine(mhx, len(lengths), 131, 64, seed=21)
        for c, n in enumerate(lengths):
            e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.05))
        runs[knob] = [e.loo(0, take, tail=tail, pointwise=True, accumulators=True)
                      for take, tail in ((24, 0), (25, 0), (1000, 0), (1024, 0), (1024, 40))]
        if knob == "1":
            check(e, 0, 1024, wc.NORMAL, y, sig, chains=[4, 6])
        e.close()
    for a, b in zip(runs["0"], runs["1"]):
        for k in FLOATS:
            assert lc.same_bits(a[k], b[k]), k
        for k in INTS:
            assert np.array_equal(a[k], b[k]), k


def test_portions_and_chunks_of_points_give_the_bits_of_one_piece(mhx):
    """1024 staged terms of 9000 points are 74 MB: a chain a portion, its points in two chunks of whole
    blocks - split after point 7424 with the accumulators and the tail asked for, after 7936 without.
    A point's results depend on its own column alone, so an engine that holds only the points around
    both splits - one portion, one chunk - must give the same pointwise bits."""
    N, lo, hi = 9000, 7300, 8100
    rng = np.random.default_rng(31)
    walks = [crafted(rng, n, [-1.0, 2.0], 0.05) for n in (1024, 300, 1024)]
    x = np.linspace(-4.0, 10.0, N)
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    got = []
    for sl in (slice(0, N), slice(lo, hi)):
        e = mhx.Engine(3, 2, 1, history_capacity=64)
        e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
        e.set_dataset(0, x[sl], y[sl], sig[sl])
        e.init_chains(np.array([-1.0, 2.0]))
        for c, (pr, th) in enumerate(walks):
            e.set_history(c, pr, th)
        got.append(e.loo(0, 1024, pointwise=True, accumulators=True))
        if sl.start == 0:
            bare = e.loo(0, 1024)
        e.close()
    split, piece = got
    for k in ("pw_elpd", "pw_khat", "pw_lppd", "pw_acc", "tail"):
        assert lc.same_bits(split[k][:, lo:hi], piece[k]), k
    for c in range(3):
        check_totals(split, c, 0.7, ("split", c))
    for k in ("elpd_loo", "p_loo", "lppd"):
        assert lc.same_bits(bare[k], split[k]), k
    for k in INTS:
        assert np.array_equal(bare[k], split[k]), k
    assert list(split["n_used"]) == [1024, 300, 1024] and (split["status"] & ~lc.FLAT == 0).all()


# ---- 6. a group ---------------------------------------------------------------------------------------
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
        whole = g.loo(0, take, pointwise=True, accumulators=True)
        one = e.loo(0, take, pointwise=True, accumulators=True)
        parts = [x.loo(0, take, pointwise=True, accumulators=True) for x in g.engines]
        for k in one:
            if one[k].dtype == np.float64:
                assert lc.same_bits(whole[k], one[k]), (take, k)
                assert lc.same_bits(whole[k], np.concatenate([p[k] for p in parts])), (take, k)
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
    none = (None,) * 11
    elpd = np.full(2, 7.5)
    used = np.full(2, -3, dtype=np.int32)
    outs = (elpd.ctypes.data_as(capi.f64p), None, None, None, used.ctypes.data_as(capi.i32p)) + (None,) * 6
    assert lib.mhx_get_loo(e._h, 0, 5, 0, 0.7, *outs) == capi.ESTATE            # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    cap = e.history_capacity()
    for take in (0, -1, cap + 1):
        assert lib.mhx_get_loo(e._h, 0, take, 0, 0.7, *outs) == capi.EINVAL
    for fn in (-1, 1):
        assert lib.mhx_get_loo(e._h, fn, 5, 0, 0.7, *outs) == capi.EINVAL
    for tail in (-1, capi.LOO_MAX_TAIL + 1):
        assert lib.mhx_get_loo(e._h, 0, 5, tail, 0.7, *outs) == capi.EINVAL
    assert lib.mhx_get_loo(e._h, 0, 5, 0, float("nan"), *outs) == capi.EINVAL
    assert lib.mhx_get_loo(None, 0, 5, 0, 0.7, *outs) == capi.EINVAL
    assert lib.mhx_group_get_loo(None, 0, 5, 0, 0.7, *outs) == capi.EINVAL
    assert list(elpd) == [7.5, 7.5] and list(used) == [-3, -3]                   # untouched on error
    assert lib.mhx_get_loo(e._h, 0, 5, 0, 0.7, *none) == capi.OK                 # all-NULL outputs
    assert e.summary_timing() >= 0.0
    assert lib.mhx_get_loo(e._h, 0, 5, 0, 0.7, *outs) == capi.OK
    assert list(used) == [1, 1] and np.isfinite(elpd).all()
    r = e.loo(0, 5, pointwise=True, accumulators=True)
    assert list(r["status"]) == [capi.LOO_SHORT] * 2 and r["tail"].shape == (2, 5, 0)
    assert lc.same_bits(r["pw_elpd"], r["pw_lppd"])        # (one step: its term, either way)
    # a window too long for the stage at its first block of points is refused, and the refusal names
    # the greatest take that fits
    big = mhx.Engine(1, 2, 1, history_capacity=65536)
    big.set_function(0, capi.MODEL_POLY, (), [0, 1])
    xs = np.linspace(0.0, 1.0, 300)
    big.set_dataset(0, xs, 1.0 + 2.0 * xs, np.full(300, 0.2))
    big.init_chains(np.array([1.0, 2.0]))
    elpd[:] = 7.5
    assert lib.mhx_get_loo(big._h, 0, 65536, 0, 0.7, *outs) == capi.EUNSUPPORTED
    msg = lib.mhx_last_error().decode()
    assert "64 MiB" in msg and "greatest take that fits is 32" in msg and list(elpd) == [7.5, 7.5]
    big.close()
    e.close()
    # a dataset per walker: refused by name
    p = mhx.Engine(2, 2, 1, history_capacity=64)
    p.set_function(0, capi.MODEL_POLY, (), [0, 1])
    x = np.linspace(0.0, 1.0, 9)
    p.set_dataset_planes(0, x, np.vstack([1.0 + 2.0 * x, 1.5 + x]))
    p.init_chains(np.array([1.0, 2.0]))
    assert lib.mhx_get_loo(p._h, 0, 5, 0, 0.7, *outs) == capi.EUNSUPPORTED
    assert "planes" in lib.mhx_last_error().decode() and list(elpd) == [7.5, 7.5]
    with pytest.raises(mhx.MhxError) as err:
        p.loo(0, 5)
    assert err.value.code == capi.EUNSUPPORTED
    p.close()


# ---- 8. the mirror ----------------------------------------------------------------------------------
KEYS8 = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]


def test_the_mirrors_loo_family(mhx):
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
    every = mhx.walker_set_loo(w1, take=500, pointwise=True)
    assert len(every) == 3
    raw = w1.engine.loo(0, 500, pointwise=True)
    short = w1.engine.loo(0, 500, tail=20, k_limit=0.5, pointwise=True)
    for c in range(3):
        mine = mhx.walker_loo(w1, chain=c, take=500, pointwise=True)
        assert set(mine) == {"elpd-loo", "p-loo", "looic", "lppd", "n-high", "n-used", "status", "pointwise", "khat",
                             "se"}
        for k in mine:
            assert np.array_equal(mine[k], every[c][k]), (c, k)
        assert mine["looic"] == -2.0 * mine["elpd-loo"] and mine["elpd-loo"] == raw["elpd_loo"][c]
        assert mine["p-loo"] == raw["p_loo"][c] and mine["lppd"] == raw["lppd"][c]
        assert mine["n-used"] == 500 and mine["status"] & ~lc.FLAT == 0 and mine["pointwise"].shape == (150,)
        assert lc.same_bits(mine["pointwise"], raw["pw_elpd"][c]) and lc.same_bits(mine["khat"], raw["pw_khat"][c])
        assert mine["se"] == float(np.sqrt(150 * np.var(mine["pointwise"], ddof=1)))
        assert "pointwise" not in mhx.walker_loo(w1, chain=c, take=500)
        other = mhx.walker_loo(w1, chain=c, take=500, tail=20, k_limit=0.5, pointwise=True)
        assert lc.same_bits(other["khat"], short["pw_khat"][c]) and other["n-high"] == short["n_high"][c]
    cmp_ = mhx.loo_compare(mhx.walker_loo(w1, take=500, pointwise=True), mhx.walker_loo(w2, take=500, pointwise=True))
    assert set(cmp_) == {"elpd-diff", "se"} and all(np.isfinite(v) for v in cmp_.values())
    print("loo_compare one peak against two on one-peak data: %r" % (cmp_,))
    # a step that is not finite raises, as walker_waic does
    pr, th = w1.engine.trace(1, 500)
    th[3] = 1e308
    w1.engine.set_history(1, pr, th)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_loo(w1, take=500)
    with pytest.raises(FloatingPointError):
        mhx.walker_loo(w1, chain=1, take=500)
    assert not mhx.walker_loo(w1, chain=0, take=500)["status"] & lc.NONFINITE
