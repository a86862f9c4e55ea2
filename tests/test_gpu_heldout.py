"""mhx_get_heldout on the device against the numpy yardstick of its definition
(tests/heldout_cases.py over tests/waic_cases.py), chain by chain, from the model values
mhx_eval_function returns at the caller's x for the steps of mhx_get_trace:

  pw_acc = (M, S, mean_v, M2_v)  bit for bit
  pw_lpd                         within 2^-52 |L| + 2^-53 |lpd_i| of M + ln(S / n) from mpmath (check_lppd
                                 of tests/test_gpu_waic.py: one ulp for the engine's log plus the addition)
  lpd                            bit for bit the block-ordered sum of the returned pw_lpd
  n_scored, n_used, status       exactly; an unused point is 0.0 in every output

and against the device itself: given its own (x, y, sigma) a shared-data engine returns the bits of
mhx_get_waic, and mean_v the bits of mhx_get_fit_percentiles' mean.  Over every kernel path, a
dataset per walker, chunks of points, portions of chains, a group, a wrapped ring, the flags, the
ABI's edges and the K-fold layer."""
import itertools
import math

import numpy as np
import pytest

import heldout_cases as hc
import problems as pb
import waic_cases as wc
from test_gpu_waic import SIX, check_lppd, crafted, expr_engine, fill, line_engine

pytestmark = pytest.mark.gpu

CHUNK = 1 << 17
KINDS = (hc.SIGMA_NONE, hc.SIGMA_SHARED, hc.SIGMA_PER_CHAIN, hc.SIGMA_PER_POINT)


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.HELDOUT_BLOCK == hc.BLOCK
    return lisp_mcmc_amd


def values(e, fn, take, x, chains):
    """{chain: the model values [n, m] at x of the chain's window, newest first}"""
    return {c: e.eval_function(fn, e.trace(c, take)[1], x).reshape(-1, np.shape(x)[-1]) for c in chains}


def check(e, fn, take, lik, x, y, sigma, kind, use, vals, flagged=(), sparse=False, **kw):
    """Engine.heldout of function fn against the yardstick on the chains of vals"""
    r = e.heldout(fn, take, x, y, sigma=sigma, sigma_kind=kind, use=use, pointwise=True, accumulators=True)
    C, m = e.n_chains, np.shape(x)[-1]
    ya = np.asarray(y, dtype=np.float64)
    rows = hc.sigma_rows(sigma, kind, C, m)
    for c, v in vals.items():
        where = (fn, take, c, kind, ya.ndim, None if use is None else np.ndim(use))
        n = len(v)
        uc = None if use is None else (np.asarray(use)[c] if np.ndim(use) == 2 else np.asarray(use))
        assert r["n_used"][c] == n, where
        assert wc.same_bits(r["lpd"][c], hc.block_sum(r["pw_lpd"][c])), where
        if c in flagged:
            assert r["status"][c] & hc.NONFINITE, where
            continue
        yc = ya[c] if ya.ndim == 2 else ya
        want = hc.yardstick(wc.terms(lik, v, yc, None if lik == wc.POISSON else rows[c], **kw), v, uc)
        assert r["status"][c] == want["status"], where
        assert r["n_scored"][c] == want["n_scored"], where
        assert wc.same_bits(r["pw_acc"][c], want["acc"]), where
        used = want["used"]
        assert (r["pw_lpd"][c][~used] == 0.0).all() and (r["pw_acc"][c][~used] == 0.0).all(), where
        if not used.any():
            assert r["lpd"][c] == 0.0 and r["status"][c] & hc.NO_POINTS, where
        pick = np.flatnonzero(used)
        if sparse:
            pick = pick[::5]
        check_lppd(r["pw_lpd"][c][pick], want["acc"][pick, 0], want["quot"][pick], where)
    return r


# ---- 1. the line model, at the edges -------------------------------------------------------------
LENGTHS = [1, 2, 3, 64, 65, 150, 300]
COMBOS = list(itertools.product(KINDS, (False, True), (0, 1, 2)))       # sigma kind, y per chain, use


def masks(rng, C, m):
    """use [m] and [C, m]: about half the points; the second block unused where there is one;
    chain 2 uses nothing at all and chain 3 nothing of its first block"""
    shared = (rng.random(m) < 0.5).astype(np.uint8)
    each = (rng.random((C, m)) < 0.5).astype(np.uint8) * 3
    shared[0] = 1
    shared[hc.BLOCK:2 * hc.BLOCK] = 0
    each[2] = 0
    each[3, :hc.BLOCK] = 0
    return shared, each


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 257, 515])
def test_line_model_blocks_windows_kinds_and_masks(mhx, m):
    rng = np.random.default_rng(m)
    turn = 0
    for ring, extra in ((64, [1500, 40]), (256, [])):
        lengths = LENGTHS + extra             # nine chains and seven: no multiple of the waves per group
        C = len(lengths)
        e, _, _ = line_engine(mhx, C, 50, ring, seed=m)           # (the engine's own 50 points are not read)
        for c, n in enumerate(lengths):
            e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.05))
        x = rng.uniform(-5.0, 11.0, m)                            # NOT the dataset's x
        y2 = -1.0 + 2.0 * x[None, :] + 0.4 * rng.standard_normal((C, m))
        sig = {hc.SIGMA_NONE: None, hc.SIGMA_SHARED: rng.uniform(0.2, 0.5, m),
               hc.SIGMA_PER_CHAIN: rng.uniform(0.2, 0.5, C), hc.SIGMA_PER_POINT: rng.uniform(0.2, 0.5, (C, m))}
        shared, each = masks(rng, C, m)
        for take in (1, 2, 3, 64, 256):
            vals = values(e, 0, take, x, range(C))
            assert [len(vals[c]) for c in range(7)] == [min(take, n) for n in LENGTHS]
            for k in range(3 if m > 65 else 5):   # every combination comes up, over the takes and the two engines
                kind, per_chain, use_kind = COMBOS[turn % len(COMBOS)]
                turn += 1
                use = (None, shared, each)[use_kind]
                r = check(e, 0, take, wc.NORMAL, x, y2 if per_chain else y2[0], sig[kind], kind, use, vals,
                          sparse=m > 65 and k > 0)
                if use_kind == 2:       # (check has held every chain to the yardstick's status)
                    assert r["status"][2] == hc.NO_POINTS and r["lpd"][2] == 0.0 and r["n_scored"][2] == 0
                    assert r["status"][3] == (hc.NO_POINTS if m <= hc.BLOCK else 0)
                else:
                    assert (r["status"] == 0).all()
        e.close()
    assert turn >= len(COMBOS)


# ---- 2. device against device ---------------------------------------------------------------------
def same_as_waic(e, fn, take, x, y, sigma):
    """given the engine's own data the held-out read-out is mhx_get_waic's, bit for bit, and its
    mean_v is mhx_get_fit_percentiles' mean"""
    w = e.waic(fn, take, pointwise=True, accumulators=True)
    h = e.heldout(fn, take, x, y, sigma=sigma, pointwise=True, accumulators=True)
    assert wc.same_bits(h["pw_lpd"], w["pw_lppd"]) and wc.same_bits(h["lpd"], w["lppd"]), fn
    assert wc.same_bits(h["pw_acc"][..., 0:2], w["pw_acc"][..., 0:2]), fn
    assert np.array_equal(h["n_used"], w["n_used"]) and np.array_equal(h["status"], w["status"] & 1), fn
    assert (h["n_scored"] == np.shape(x)[-1]).all(), fn
    _, mean, sd, used, _ = e.fit_percentiles(fn, take, xs=x, pcts=())
    assert wc.same_bits(h["pw_acc"][..., 2], mean) and np.array_equal(used, h["n_used"]), fn
    with np.errstate(all="ignore"):
        var = h["pw_acc"][..., 3] / (h["n_used"][:, None] - 1.0)
    assert wc.same_bits(np.sqrt(var)[h["n_used"] > 1], sd[h["n_used"] > 1]), fn
    return h


def test_config2_two_peak_on_the_ahead_of_time_kernel(mhx):
    s = pb.two_peak(n=300, seed=3)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "gauss22_normal" in e.kernel_name()
    fill(e, np.random.default_rng(1), s.theta_star, 0.02, SIX)
    x, y, sig, _ = s.data[0]
    for take in (150, 64):
        same_as_waic(e, 0, take, x, y, sig)
    # ... and against the yardstick, at other points, with a y and a mask per chain
    rng = np.random.default_rng(2)
    xs = np.sort(rng.uniform(0.0, 1.0, 270))
    y2 = pb.model_eval_np(pb.GAUSS, (2, 2), s.theta_star, xs)[None, :] + 0.1 * rng.standard_normal((6, 270))
    use = (rng.random((6, 270)) < 0.7).astype(np.uint8)
    check(e, 0, 150, wc.NORMAL, xs, y2, np.full(6, 0.1), hc.SIGMA_PER_CHAIN, use, values(e, 0, 150, xs, range(6)),
          sparse=True)
    e.close()


def test_the_cutoff_likelihood(mhx):
    s = pb.two_peak(n=257, seed=4, lik=pb.CUTOFF)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "gauss22_cutoff" in e.kernel_name()
    rng = np.random.default_rng(2)
    x, y, sig, _ = s.data[0]
    for c, n in enumerate(SIX):
        pr, th = crafted(rng, n, s.theta_star, 0.02)
        th[::3, 0] += 30.0            # every third step's background is far off: its terms clamp
        e.set_history(c, pr, th)
    same_as_waic(e, 0, 150, x, y, sig)
    vals = values(e, 0, 150, x, [4])
    ell = wc.terms(wc.CUTOFF, vals[4], y, sig)
    assert (ell == -5000.0).any() and (ell > -5000.0).any()
    check(e, 0, 150, wc.CUTOFF, x, y, sig, hc.SIGMA_SHARED, None, vals, sparse=True)
    e.close()


@pytest.mark.parametrize("logfact_double", [False, True])
def test_five_peak_poisson(mhx, logfact_double):
    s = pb.poisson_peaks(n=280)
    e = s.engine(mhx, 6, history_capacity=64, poisson_logfact_double=logfact_double)
    e.init_chains(s.theta_star)
    assert "gauss15_poisson" in e.kernel_name()
    fill(e, np.random.default_rng(3), s.theta_star, 0.01, SIX)
    x, y, _, _ = s.data[0]
    vals = values(e, 0, 150, x, range(6))
    for c in range(6):                # (mirror_tlog restates the table branch: every rate clear of 1)
        assert (vals[c] > 1.0625).all()
    same_as_waic(e, 0, 150, x, y, None)
    # other counts per chain at the same x (the rates stay what they are)
    y2 = np.random.default_rng(4).poisson(np.maximum(vals[5][0], 1.0), (6, x.size)).astype(np.float64)
    check(e, 0, 150, wc.POISSON, x, y2, None, hc.SIGMA_NONE, None, vals, sparse=True, logfact_double=logfact_double)
    e.close()


def test_the_generic_kernel(mhx, monkeypatch):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    s = pb.two_peak(n=200, seed=6)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "generic" in e.kernel_name()
    fill(e, np.random.default_rng(4), s.theta_star, 0.02, SIX)
    x, y, sig, _ = s.data[0]
    same_as_waic(e, 0, 150, x, y, sig)
    e.close()
    p = pb.poisson_peaks(n=130)
    e = p.engine(mhx, 3, history_capacity=64)
    e.init_chains(p.theta_star)
    assert "generic" in e.kernel_name()
    fill(e, np.random.default_rng(5), p.theta_star, 0.01, [1, 30, 66])
    same_as_waic(e, 0, 150, p.data[0][0], p.data[0][1], None)
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
    same_as_waic(e, 0, 150, x, y, sig)
    e.close()


def expr_data():
    """the x expr_engine (tests/test_gpu_waic.py) sets its dataset at"""
    return np.linspace(0.0, 3.0, 290)


def test_an_expression_compiled_as_written(mhx):
    e, y, sig = expr_engine(mhx, 6)
    same_as_waic(e, 0, 150, expr_data(), y, sig)
    e.close()


def test_an_expression_likelihood(mhx):
    e, y, sig = expr_engine(mhx, 6, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")
    x = expr_data()
    same_as_waic(e, 0, 150, x, y, sig)

    def term(yy, m, err):
        d = (yy - m) / err
        return 0.0 - (0.5 * (d * d))
    # `error` per chain and point, handed to the expression untouched
    rng = np.random.default_rng(8)
    err = rng.uniform(0.05, 0.2, (6, x.size))
    check(e, 0, 150, wc.EXPR, x, y, err, hc.SIGMA_PER_POINT, None, values(e, 0, 150, x, range(6)), sparse=True,
          lik_term=term)
    e.close()


def test_two_columns_of_x(mhx):
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
    same_as_waic(e, 0, 150, np.ascontiguousarray(X.T), y, sig)
    e.close()


def test_both_functions_of_a_global_fit(mhx):
    s = pb.global_fit(n_each=140, n_sets=2)
    e = s.engine(mhx, 6, history_capacity=64)
    e.init_chains(s.theta_star)
    assert "pvoigt2" in e.kernel_name()
    fill(e, np.random.default_rng(8), s.theta_star, 0.01, SIX)
    for fn in (0, 1):
        x, y, sig, _ = s.data[fn]
        same_as_waic(e, fn, 150, x, y, sig)
    e.close()


# ---- 3. a dataset per walker is served --------------------------------------------------------------
@pytest.mark.parametrize("kind", [hc.SIGMA_PER_CHAIN, hc.SIGMA_PER_POINT])
def test_a_planes_engine_gives_the_bits_of_eleven_one_chain_yardsticks(mhx, kind):
    rng = np.random.default_rng(20 + kind)
    C, n = 11, 270
    th = np.array([0.5, 0.3, 1.0, 0.4, 0.06])
    x = np.linspace(0.0, 1.0, n)
    sig = rng.uniform(0.05, 0.15, C) if kind == hc.SIGMA_PER_CHAIN else rng.uniform(0.05, 0.15, (C, n))
    y = pb.model_eval_np(pb.GAUSS, (2, 1), th, x)[None, :] + 0.1 * rng.standard_normal((C, n))
    e = mhx.Engine(C, 5, 1, history_capacity=64)
    e.set_function(0, mhx.capi.MODEL_GAUSS_PEAKS, (2, 1), list(range(5)))
    e.set_dataset_planes(0, x, y, sig, kind)
    e.init_chains(th)
    fill(e, rng, th, 0.02, [int(k) for k in rng.integers(1, 160, C)])
    with pytest.raises(mhx.MhxError):           # (WAIC's refusal stands)
        e.waic(0, 150)
    r = check(e, 0, 150, wc.NORMAL, x, y, sig, kind, None, values(e, 0, 150, x, range(C)), sparse=True)
    assert (r["status"] == 0).all() and (r["n_scored"] == n).all()
    e.close()


# ---- 4. chunks of points, portions of chains, a group ----------------------------------------------
def test_points_beyond_one_chunk(mhx):
    m = CHUNK + 3
    e, _, _ = line_engine(mhx, 2, 50, 64, seed=1)
    rng = np.random.default_rng(9)
    for c in range(2):
        e.set_history(c, *crafted(rng, 3, [-1.0, 2.0], 0.05))
    x = rng.uniform(-5.0, 11.0, m)
    y2 = -1.0 + 2.0 * x[None, :] + 0.4 * rng.standard_normal((2, m))
    sig = rng.uniform(0.2, 0.5, (2, m))
    use = (rng.random((2, m)) < 0.5).astype(np.uint8)
    use[:, CHUNK - 2:] = 1
    r = e.heldout(0, 3, x, y2, sigma=sig, use=use, pointwise=True, accumulators=True)
    assert (r["status"] == 0).all() and list(r["n_used"]) == [3, 3]
    assert list(r["n_scored"]) == [int(use[c].sum()) for c in range(2)]
    far = slice(CHUNK - 300, m)                 # both sides of the split against the yardstick
    for c in range(2):
        assert wc.same_bits(r["lpd"][c], hc.block_sum(r["pw_lpd"][c])), c
        v = e.eval_function(0, e.trace(c, 3)[1], x[far])
        want = hc.yardstick(wc.terms(wc.NORMAL, v, y2[c, far], sig[c, far]), v, use[c, far])
        assert wc.same_bits(r["pw_acc"][c, far], want["acc"]), c
        assert (r["pw_lpd"][c][use[c] == 0] == 0.0).all(), c
    bare = e.heldout(0, 3, x, y2, sigma=sig, use=use)      # the totals' bits without pointwise outputs
    assert wc.same_bits(bare["lpd"], r["lpd"]) and np.array_equal(bare["n_scored"], r["n_scored"])
    e.close()


def test_portions_of_chains_and_a_group_give_the_same_bits(mhx):
    """300 chains at 4101 points with every output: 65 bytes a point and chain, 251 chains to a
    portion of 64 MiB - the engine works through two, each engine of the group through one"""
    C, m = 300, 4101
    rng = np.random.default_rng(15)
    walks = [crafted(rng, 2, [-1.0, 2.0], 0.05) for _ in range(C)]
    xd = np.linspace(-4.0, 10.0, 50)
    e = mhx.Engine(C, 2, 1, history_capacity=64)
    g = mhx.Group(C, 2, 1, devices=[0, 0], history_capacity=64)
    for t in (e, g):
        t.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
        t.set_dataset(0, xd, -1.0 + 2.0 * xd, np.full(50, 0.3))
        t.init_chains(np.array([-1.0, 2.0]))
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
        i = 0 if c < g.ranges[1][0] else 1
        g.engines[i].set_history(c - g.ranges[i][0], pr, th)
    x = rng.uniform(-5.0, 11.0, m)
    y2 = -1.0 + 2.0 * x[None, :] + 0.4 * rng.standard_normal((C, m))
    sig = rng.uniform(0.2, 0.5, (C, m))
    use = (rng.random((C, m)) < 0.5).astype(np.uint8)
    kw = dict(sigma=sig, use=use, pointwise=True, accumulators=True)
    one = e.heldout(0, 2, x, y2, **kw)
    whole = g.heldout(0, 2, x, y2, **kw)
    for k in one:
        if one[k].dtype == np.float64:
            assert wc.same_bits(whole[k], one[k]), k
        else:
            assert np.array_equal(whole[k], one[k]), k
    assert (one["status"] == 0).all() and np.array_equal(one["n_scored"], use.sum(axis=1))
    # per-chain sigma scalars and a shared y move with a group's chains too
    s1 = rng.uniform(0.2, 0.5, C)
    a, b = e.heldout(0, 2, x, y2[0], sigma=s1, sigma_kind=hc.SIGMA_PER_CHAIN), \
        g.heldout(0, 2, x, y2[0], sigma=s1, sigma_kind=hc.SIGMA_PER_CHAIN)
    assert wc.same_bits(a["lpd"], b["lpd"])
    for c in (0, 250, 251, 299):                # either side of the engine's portion boundary
        v = e.eval_function(0, e.trace(c, 2)[1], x)
        want = hc.yardstick(wc.terms(wc.NORMAL, v, y2[c], sig[c]), v, use[c])
        assert wc.same_bits(one["pw_acc"][c], want["acc"]), c
        assert wc.same_bits(one["lpd"][c], hc.block_sum(one["pw_lpd"][c])), c
    e.close()
    g.close()


# ---- 5. a real walk in a wrapped ring ---------------------------------------------------------------
def test_a_real_walk_in_a_wrapped_ring(mhx):
    s = pb.two_peak(n=300, seed=6)
    e = s.engine(mhx, 8, seed=3, history_capacity=1024)
    e.init_chains(pb.perturbed(s.theta_star, 8, 0.01, seed=9))
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(1500)
    R = e.history_capacity()
    length = e.state()["length"]
    assert R == 1024 and int(length.min()) > R and int(length.max()) < 2 * R
    rng = np.random.default_rng(5)
    xs = np.sort(rng.uniform(0.0, 1.0, 300))
    y2 = pb.model_eval_np(pb.GAUSS, (2, 2), s.theta_star, xs)[None, :] + 0.1 * rng.standard_normal((8, 300))
    use = (rng.random((8, 300)) < 0.6).astype(np.uint8)
    r = check(e, 0, 400, wc.NORMAL, xs, y2, np.full(300, 0.1), hc.SIGMA_SHARED, use,
              values(e, 0, 400, xs, [0, 3, 7]), sparse=True)
    assert (r["status"] == 0).all() and (r["n_used"] == 400).all()
    # windows that straddle the wrap point: entry k sits in slot k mod R, so a window of `take` steps
    # passes slot 0 exactly when the newest slot is below take - 1
    newest = (length - 1) & (R - 1)
    for c, take in ((1, R), (5, int(newest[5]) + 151)):
        assert 0 <= newest[c] < take - 1 <= R - 1 and length[c] >= take, (c, newest[c], take)
        check(e, 0, take, wc.NORMAL, xs, y2, np.full(300, 0.1), hc.SIGMA_SHARED, use, values(e, 0, take, xs, [c]),
              sparse=True)
    e.close()


# ---- 6. the flags -----------------------------------------------------------------------------------
def test_flags(mhx):
    rng = np.random.default_rng(10)
    walks = [crafted(rng, 30, [-1.0, 2.0], 0.1) for _ in range(3)]
    m = 70
    x = rng.uniform(-5.0, 11.0, m)
    y = -1.0 + 2.0 * x + 0.4 * rng.standard_normal(m)
    sig = rng.uniform(0.2, 0.5, m)
    runs = []
    for spoil in (False, True):                 # a step that is not finite flags its chain only
        e, _, _ = line_engine(mhx, 3, 50, 64, seed=2)
        for c, (pr, th) in enumerate(walks):
            th = th.copy()
            if spoil and c == 1:
                th[11] = [1e308, 1e308]
            e.set_history(c, pr, th)
        runs.append(e.heldout(0, 30, x, y, sigma=sig, pointwise=True, accumulators=True))
        if not spoil:
            keep = e
        else:
            e.close()
    clean, spoilt = runs
    assert list(clean["status"]) == [0, 0, 0] and list(spoilt["status"]) == [0, hc.NONFINITE, 0]
    for k in ("lpd", "pw_lpd", "pw_acc"):
        for c in (0, 2):
            assert wc.same_bits(clean[k][c], spoilt[k][c]), (k, c)
    # a value that is not finite at ONE point: flagged where the chain uses it, nothing where it does not
    e = keep
    xb = x.copy()
    xb[17] = 1.7e308                            # -1 + 2 x overflows there, whatever the step
    assert np.isinf(e.eval_function(0, np.array([-1.0, 2.0]), xb)[17])
    use = np.ones((3, m), dtype=np.uint8)
    use[0, 17] = use[2, 17] = 0
    r = e.heldout(0, 30, xb, y, sigma=sig, use=use, pointwise=True, accumulators=True)
    assert list(r["status"]) == [0, hc.NONFINITE, 0] and list(r["n_scored"]) == [m - 1, m, m - 1]
    for c in (0, 2):
        assert r["pw_lpd"][c, 17] == 0.0 and (r["pw_acc"][c, 17] == 0.0).all()
        ok = np.arange(m) != 17
        assert wc.same_bits(r["pw_acc"][c][ok], clean["pw_acc"][c][ok]), c
        assert wc.same_bits(r["lpd"][c], hc.block_sum(r["pw_lpd"][c])) and np.isfinite(r["lpd"][c])
    # an empty window is flagged (:burn-walks may take every step of a walk)
    for c, n in enumerate((3, 5, 9)):
        e.set_history(c, *crafted(rng, n, [-1.0, 2.0], 0.1))
    e.modify("burn-walks", 3)
    assert list(e.state()["length"]) == [0, 2, 6]
    r = check(e, 0, 64, wc.NORMAL, x, y, sig, hc.SIGMA_SHARED, None, values(e, 0, 64, x, [1, 2]))
    assert list(r["n_used"]) == [0, 2, 6] and list(r["status"]) == [hc.NONFINITE, 0, 0]
    e.close()


# ---- 7. the ABI's edges -----------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = mhx.Engine(2, 2, 1, history_capacity=64)
    e.set_function(0, capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0], np.full(5, 0.2))
    m = 6
    x, xp = capi.as_f64(np.linspace(0.0, 5.0, m))
    y, yp = capi.as_f64(1.0 + np.arange(m))
    s, sp = capi.as_f64(np.full(m, 0.5))
    bad_s, bad_sp = capi.as_f64([0.5, 0.5, 0.5, 0.0, 0.5, 0.5])
    lpd = np.full(2, 7.5)
    ns, nu, st = (np.full(2, -3, dtype=np.int32) for _ in range(3))
    pw, acc = np.full((2, m), 7.5), np.full((2, m, 4), 7.5)
    outs = [lpd.ctypes.data_as(capi.f64p), ns.ctypes.data_as(capi.i32p), pw.ctypes.data_as(capi.f64p),
            acc.ctypes.data_as(capi.f64p), nu.ctypes.data_as(capi.i32p), st.ctypes.data_as(capi.i32p)]

    def call(h=None, fn=0, take=5, xcols=xp, n_cols=1, mm=m, yy=yp, sigma=sp, kind=capi.SIGMA_SHARED, o=outs):
        return lib.mhx_get_heldout(e._h if h is None else h, fn, take, xcols, n_cols, mm, yy, 0, sigma, kind,
                                   None, 0, *o)

    def untouched():
        return (lpd == 7.5).all() and (pw == 7.5).all() and (acc == 7.5).all() and \
            all((a == -3).all() for a in (ns, nu, st))
    assert call() == capi.ESTATE and untouched()                        # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    cap = e.history_capacity()
    for take in (0, -1, cap + 1):
        assert call(take=take) == capi.EINVAL
    for fn in (-1, 1):
        assert call(fn=fn) == capi.EINVAL
    assert call(n_cols=2) == capi.EINVAL and "column" in lib.mhx_last_error().decode()
    assert call(mm=0) == capi.EINVAL and call(xcols=None) == capi.EINVAL and call(yy=None) == capi.EINVAL
    for kind in (-1, 4, capi.SIGMA_NONE):                                # NONE goes with a NULL sigma only
        assert call(kind=kind) == capi.EINVAL
    assert call(sigma=None) == capi.EINVAL
    assert call(sigma=bad_sp) == capi.EINVAL and "sigma[3]" in lib.mhx_last_error().decode()
    assert lib.mhx_get_heldout(None, 0, 5, xp, 1, m, yp, 0, sp, capi.SIGMA_SHARED, None, 0, *outs) == capi.EINVAL
    assert untouched()                                                   # untouched on every error
    assert call(o=[None] * 6) == capi.OK                                 # all-NULL outputs
    assert e.summary_timing() >= 0.0
    full = e.heldout(0, 5, x, y, sigma=s, pointwise=True, accumulators=True)
    for k in range(6):                                                   # every output NULL in turn
        lpd[:], pw[:], acc[:] = 7.5, 7.5, 7.5
        ns[:], nu[:], st[:] = -3, -3, -3
        assert call(o=[None if j == k else p for j, p in enumerate(outs)]) == capi.OK
        for j, (mine, ref) in enumerate(zip((lpd, ns, pw, acc, nu, st),
                                            (full[n] for n in ("lpd", "n_scored", "pw_lpd", "pw_acc", "n_used",
                                                               "status")))):
            if j == k:
                assert (mine == (7.5 if mine.dtype == np.float64 else -3)).all(), (k, j)
            elif mine.dtype == np.float64:
                assert wc.same_bits(mine, ref), (k, j)
            else:
                assert np.array_equal(mine, ref), (k, j)
    assert list(full["n_used"]) == [1, 1] and list(full["n_scored"]) == [m, m] and list(full["status"]) == [0, 0]
    e.close()
    s5 = pb.poisson_peaks(n=130)
    p = s5.engine(mhx, 2, history_capacity=64)
    p.init_chains(s5.theta_star)
    with pytest.raises(mhx.MhxError) as err:                             # a Poisson y that is no count
        p.heldout(0, 5, np.linspace(0.0, 1.0, 4), [3.0, 2.5, 1.0, 0.0])
    assert err.value.code == capi.EINVAL and "y[1]" in str(err.value)
    p.close()


# ---- 8. K-fold ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [":interleaved", ":blocks"])
def test_kfold(mhx, scheme):
    rng = np.random.default_rng(48)
    K, n, S = 3, 48, 2
    x = np.linspace(0.0, 1.0, n)
    th = np.array([0.5, 1.0, 0.45, 0.1])
    sig = rng.uniform(0.05, 0.15, n)
    ys = [pb.model_eval_np(pb.GAUSS, (1, 1), th, x) + sig * rng.standard_normal(n) for _ in range(S)]
    fn = mhx.models.gauss_peaks(["b0"], [["a1", "mu1", "w1"]])
    params = [":b0", 0.5, ":a1", 1.0, ":mu1", 0.45, ":w1", 0.1]
    w = mhx.walker_set_kfold_create(function=fn, datasets=[[x, y] for y in ys], params=params, data_error=sig,
                                    K=K, scheme=scheme, history_capacity=64)
    e = w.engine
    assert e.n_chains == S * K and w.kfold["K"] == K and wc.same_bits(w.kfold["sigma"], np.vstack([sig, sig]))
    folds = w.kfold["folds"]
    assert np.array_equal(folds, mhx.kfold_folds(n, K, scheme))
    # the walker's log-posterior is the sum over its TRAINING points, plus its constant
    trial = th * (1.0 + 0.05 * rng.standard_normal((S * K, 4)))
    got = e.logpost(trial)
    half = wc.HALF_LOG_2PI
    for c in range(S * K):
        s_, k = divmod(c, K)
        train = folds != k
        v = pb.model_eval_np(pb.GAUSS, (1, 1), trial[c], x)
        z = (ys[s_] - v) / sig
        terms = np.concatenate([(half - np.log(sig[train])) - 0.5 * z[train] ** 2,
                                half - np.log(sig[~train] * 2.0 ** 400)])
        assert abs(got[c] - math.fsum(terms)) <= 1e-12 * math.fsum(np.abs(terms)), (c, got[c], math.fsum(terms))
    # ... and does not change by a bit when the held-out y are other numbers
    y_other = np.array([np.where(folds == c % K, 50.0 + rng.normal(0, 30, n), ys[c // K]) for c in range(S * K)])
    scaled = [np.where(folds == c % K, sig * 2.0 ** 400, sig) for c in range(S * K)]
    w2 = mhx.walker_set_create(function=fn, datasets=[[x, y] for y in y_other], params=params, data_error=scaled,
                               history_capacity=64)
    assert wc.same_bits(w2.engine.logpost(trial), got)
    w2.engine.close()
    # histories are set, not walked
    fill(e, rng, th, 0.03, [40, 64, 33, 50, 64, 21])
    res = mhx.walker_set_kfold(w, take=64)
    use = np.array([folds == c % K for c in range(S * K)], dtype=np.uint8)
    raw = e.heldout(0, 64, x, np.repeat(np.array(ys), K, axis=0), sigma=np.repeat(np.vstack([sig, sig]), K, axis=0),
                    use=use, pointwise=True)
    assert len(res) == S
    for s_, entry in enumerate(res):
        assert set(entry) == {"elpd-kfold", "pointwise", "se", "n-used", "status"}
        pw = entry["pointwise"]
        assert pw.shape == (n,) and entry["status"] == 0 and entry["n-used"] == [[40, 64, 33], [50, 64, 21]][s_]
        for i in range(n):                      # every point exactly once: under the walker that did not see it
            assert wc.same_bits(pw[i], raw["pw_lpd"][s_ * K + folds[i], i])
            assert [raw["pw_lpd"][s_ * K + k, i] != 0.0 for k in range(K)].count(True) == 1
        assert entry["se"] == float(np.sqrt(n * np.var(pw, ddof=1)))
        assert entry["elpd-kfold"] == float(np.cumsum(raw["lpd"][s_ * K:(s_ + 1) * K])[-1])
        assert abs(entry["elpd-kfold"] - math.fsum(pw)) <= n * 2.0 ** -53 * math.fsum(np.abs(pw))
    assert "pointwise" not in mhx.walker_set_kfold(w, take=64, pointwise=False)[0]
    cmp_ = mhx.waic_compare(res[0], res[1])
    assert set(cmp_) == {"elpd-diff", "se"} and all(np.isfinite(v) for v in cmp_.values())
    # walker_set_score_data: each walker's own spectrum, which walker_set_waic refuses on such a set
    with pytest.raises(mhx.MhxError):
        mhx.walker_set_waic(w, take=64)
    own = mhx.walker_set_score_data(w, [x, np.repeat(np.array(ys), K, axis=0)], data_error=sig, take=64,
                                    pointwise=True)
    full = e.heldout(0, 64, x, np.repeat(np.array(ys), K, axis=0), sigma=sig, pointwise=True, accumulators=True)
    for c, entry in enumerate(own):
        assert set(entry) == {"lpd", "n-scored", "n-used", "status", "pointwise", "se", "fit-mean", "fit-stddev",
                              "z-pred"}
        assert entry["lpd"] == full["lpd"][c] and entry["n-scored"] == n and entry["status"] == 0
        assert wc.same_bits(entry["pointwise"], full["pw_lpd"][c]) and wc.same_bits(entry["fit-mean"], full["pw_acc"][c, :, 2])
        assert entry["se"] == float(np.sqrt(n * np.var(entry["pointwise"], ddof=1)))
        var = full["pw_acc"][c, :, 3] / (entry["n-used"] - 1.0)
        assert np.allclose(entry["z-pred"], (ys[c // K] - entry["fit-mean"]) / np.sqrt(sig ** 2 + var), rtol=1e-13)
    one = mhx.walker_score_data(w, [x, ys[0]], data_error=sig, chain=4, take=64)
    assert set(one) == {"lpd", "n-scored", "n-used", "status"} and one["n-used"] == 64
    pr, tr = e.trace(1, 64)
    tr[3] = 1e308
    e.set_history(1, pr, tr)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_kfold(w, take=64)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_score_data(w, [x, ys[0]], data_error=sig, take=64)
    assert mhx.walker_score_data(w, [x, ys[0]], data_error=sig, chain=0, take=64)["status"] == 0
    e.close()
