"""walker-get-data-and-fit (mcmc-fitting.lisp:1230-1255) on the device: mhx_eval_function against
the oracle's reference-order formulas, per value, within 1e-12 sum |terms| (the bound DESIGN 3.1
states for the direct kernel's log-posterior, applied per value); mhx_get_fit_bands against host
selection from mhx_get_trace + mhx_eval_function + numpy max / min, bit for bit, every chain; the
mirror's walker_get_data_and_fit family; the group form; the ABI's edges.

Worst |device - oracle| / sum |terms| measured on MI355X (build csrc:57229aab12d4cac8): 1.3e-14
(three Gaussians without a background), 2.8e-15 (config 3's five peaks), below 8e-16 for every
other model - DESIGN 4.2."""
import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

REL = 1e-12
LF_X, LF_Y = [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0]
TWO_PEAK = ("(lambda (x &key b0 b1 a1 mu1 w1 a2 mu2 w2 &allow-other-keys)"
            " (+ (+ b0 (* b1 x))"
            "    (* a1 (exp (- (expt (/ (- x mu1) w1) 2))))"
            "    (* a2 (exp (- (expt (/ (- x mu2) w2) 2))))))")
KEYS8 = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


@pytest.fixture(scope="module")
def orc():
    import oraclelib
    return oraclelib


# ---- 4. model values against the faithful formulas -----------------------------------------------
def oracle_values(orc, model, shape, p, x):
    sh = np.asarray(shape or (0,), dtype=np.int32)
    p = np.ascontiguousarray(p, dtype=np.float64)
    return np.array([orc.lib().orc_model_eval(model, sh.ctypes.data_as(orc.i32p),
                                              p.ctypes.data_as(orc.f64p), len(p), float(xi)) for xi in x])


def abs_terms(model, shape, p, x):
    """sum |terms| of the model at x: the background's monomials and the peak values, in absolute
    value (the other models: their additive pieces)"""
    x = np.asarray(x, float)
    if model == pb.POLY:
        return sum(abs(c) * np.abs(x) ** j for j, c in enumerate(p))
    if model in (pb.GAUSS, pb.LORENTZ):
        nbg, npk = shape
        t = sum((abs(c) * np.abs(x) ** j for j, c in enumerate(p[:nbg])), np.zeros_like(x))
        for k in range(npk):
            A, mu, w = p[nbg + 3 * k: nbg + 3 * k + 3]
            u = (x - mu) / w
            t = t + np.abs(A) * (np.exp(-u * u) if model == pb.GAUSS else 1 / (1 + u * u))
        return t
    if model == pb.PVOIGT2:
        A, b0, b1, mu1, w1, e1, mu2, w2, e2, rho, c2 = p
        u1, u2 = (x - mu1) / w1, (x - mu2) / w2
        pk = lambda e, u: abs(e) / (1 + u * u) + abs(1 - e) * np.exp(-u * u)  # noqa: E731
        return abs(b0) + abs(b1 * x) + abs(c2 * x * x) + abs(A) * (pk(e1, u1) + abs(rho) * pk(e2, u2))
    if model == pb.LORDER:
        scale, lw, x0, mix, bg0, bg1 = p
        u = (x - x0) / lw
        q = 1 + u * u
        return (abs(scale) * (abs(np.cos(mix) * 2 * u) + abs(np.sin(mix)) * (1 + u * u)) / (q * q)
                + abs(bg0) + abs(bg1 * x))
    if model == pb.EXPDECAY:
        return abs(p[0]) * np.exp(-x / p[1]) + abs(p[2])
    if model == pb.SINUS:
        return abs(p[0]) + abs(p[3])
    raise NotImplementedError


def x_on_and_off(x, seed):
    """the dataset's own x and points between, before and beyond them"""
    rng = np.random.default_rng(seed)
    lo, hi = x.min(), x.max()
    off = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), 777)
    return np.concatenate([x[:: max(1, len(x) // 300)], off])


WORST = {}


def check_values(mhx, orc, s, name, n_vec=4, scale=0.01):
    e = s.engine(mhx, 1)
    th = pb.perturbed(s.theta_star, n_vec, scale, seed=21)
    for k, (model, shape, idx) in enumerate(s.fns):
        xd = s.data[k][0]
        xs = x_on_and_off(xd, seed=k)
        got = e.eval_function(k, th, xs)
        assert got.shape == (n_vec, len(xs))
        worst = 0.0
        for i in range(n_vec):
            p = th[i][idx]
            ref = oracle_values(orc, model, shape, p, xs)
            terms = abs_terms(model, shape, p, xs)
            ratio = np.abs(got[i] - ref) / terms
            worst = max(worst, float(ratio.max()))
        WORST[name] = max(WORST.get(name, 0.0), worst)
        print("eval_function %s fn %d: worst |device - oracle| / sum|terms| = %.3e" % (name, k, worst))
        assert worst <= REL, (name, k, worst)
        # xcols == NULL: the dataset's own x, the same bits as passing it
        own = e.eval_function(k, th)
        assert own.shape == (n_vec, len(xd))
        assert np.array_equal(own.view(np.uint64), e.eval_function(k, th, xd).view(np.uint64))
    name_k = e.kernel_name()
    e.close()
    return name_k


def single(model, shape, p, x=None, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(-1, 2, 777) if x is None else x
    sig = rng.uniform(0.1, 0.2, x.size)
    s = pb.Spec(len(p))
    s.add(model, shape, range(len(p)), x, np.zeros_like(x), sig, pb.NORMAL)
    s.theta_star = np.asarray(p, float)
    return s


ENUMERATED = [
    ("poly5", pb.POLY, (), [0.3, -1.0, 0.5, 0.2, -0.1]),
    ("poly2", pb.POLY, (), [0.3, -1.0]),
    ("poly8", pb.POLY, (), [0.3, -1.0, 0.5, 0.2, -0.1, 0.05, 0.01, -0.02]),
    ("lorentz12", pb.LORENTZ, (1, 2), [0.1, 1.0, 0.2, 0.1, 0.5, 1.2, 0.3]),
    ("gauss31", pb.GAUSS, (3, 1), [0.1, 0.2, -0.1, 1.0, 0.4, 0.2]),
    ("gauss03", pb.GAUSS, (0, 3), [1.0, 0.0, 0.2, 0.5, 1.0, 0.1, 0.8, 1.5, 0.3]),
    ("expdecay", pb.EXPDECAY, (), [2.0, 0.7, 0.1]),
    ("sinusoid", pb.SINUS, (), [1.5, 3.0, 0.4, -0.2]),
    ("pvoigt2", pb.PVOIGT2, (), [1.2, 0.1, -0.2, 0.3, 0.1, 0.4, 1.1, 0.2, 0.7, 0.8, 0.05]),
]


@pytest.mark.parametrize("name, model, shape, p", ENUMERATED, ids=[c[0] for c in ENUMERATED])
def test_values_of_every_enumerated_model(mhx, orc, name, model, shape, p):
    check_values(mhx, orc, single(model, shape, p), name)


def test_values_of_the_benchmark_problems(mhx, orc):
    assert "gauss22_normal" in check_values(mhx, orc, pb.two_peak(n=3000, seed=3), "config2 two-peak")
    assert "gauss15_poisson" in check_values(mhx, orc, pb.poisson_peaks(n=3000), "config3 five-peak")
    assert "pvoigt2" in check_values(mhx, orc, pb.global_fit(n_each=400, n_sets=3), "pvoigt2 global")
    assert "lorder" in check_values(mhx, orc, pb.lorder(), "lorder", scale=0.001)


def test_values_on_the_generic_kernels(mhx, orc, monkeypatch):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    for name, model, shape, p in ENUMERATED:
        assert "generic" in check_values(mhx, orc, single(model, shape, p), name + " (generic)")
    assert "generic" in check_values(mhx, orc, pb.two_peak(n=1500, seed=3), "two-peak (generic)")


def test_values_of_expression_models_and_closures(mhx):
    import sexpr_eval
    s = pb.two_peak(n=1200, seed=8)
    x, y, sig, _ = s.data[0]
    params = []
    for k, v in zip(KEYS8, s.theta_star):
        params += [":" + k, float(v)]
    body = mhx.sexpr.parse(TWO_PEAK)[2]
    xs = x_on_and_off(x, seed=2)
    th = pb.perturbed(s.theta_star, 3, 0.02, seed=4)
    for as_written in (False, True):
        w = mhx.walker_create(function=mhx.models.lisp(TWO_PEAK, as_written=as_written),
                              data=[x, y], params=params, data_error=sig)
        assert ("rtc[expr" in w.engine.kernel_name()) == as_written
        got = w.engine.eval_function(0, th, xs)
        worst = 0.0
        for i in range(len(th)):
            for j in range(0, len(xs), 7):
                env = dict(zip(KEYS8, th[i]))
                env["x"] = float(xs[j])
                ref = sexpr_eval.evaluate(body, env)
                terms = abs_terms(pb.GAUSS, (2, 2), th[i], xs[j:j + 1])[0]
                worst = max(worst, abs(got[i, j] - ref) / terms)
        print("eval_function closure as_written=%s: worst ratio %.3e" % (as_written, worst))
        assert worst <= REL, (as_written, worst)
        own = w.engine.eval_function(0, th)
        assert np.array_equal(own, w.engine.eval_function(0, th, x))
    # an expression through the ABI's own text, with a division, exp and log
    e = mhx.Engine(1, 3, 1)
    e.set_function_expr(0, "a*exp(-x/tau) + log(c + x*x)", ["a", "tau", "c"], [0, 1, 2])
    xe = np.linspace(0.0, 3.0, 500)
    e.set_dataset(0, xe, np.zeros_like(xe), np.full(500, 0.1))
    t3 = np.array([[2.0, 0.7, 1.5], [1.1, 1.9, 0.3]])
    got = e.eval_function(0, t3, xs)
    for i, (a, tau, c) in enumerate(t3):
        ref = a * np.exp(-xs / tau) + np.log(c + xs * xs)
        terms = np.abs(a * np.exp(-xs / tau)) + np.abs(np.log(c + xs * xs))
        assert (np.abs(got[i] - ref) <= REL * terms).all(), i
    e.close()


def test_values_over_two_columns_of_x(mhx):
    rng = np.random.default_rng(5)
    n = 900
    X = np.column_stack([rng.uniform(-1, 2, n), rng.uniform(0, 3, n)])
    e = mhx.Engine(1, 4, 1)
    e.set_function_expr(0, "a + b*xcol0 + c*xcol1 + d*xcol0*xcol1", list("abcd"), [0, 1, 2, 3])
    e.set_dataset(0, X, np.zeros(n), np.full(n, 0.1))
    th = np.array([[0.4, 1.3, -0.7, 0.25], [1.0, -1.0, 2.0, 0.5]])
    Xo = np.column_stack([rng.uniform(-2, 3, 333), rng.uniform(-1, 4, 333)])
    for Xq, arg in ((X, None), (X, X.T), (Xo, Xo.T)):
        got = e.eval_function(0, th, arg)
        for i, t in enumerate(th):
            pieces = [np.full(len(Xq), t[0]), t[1] * Xq[:, 0], t[2] * Xq[:, 1], t[3] * Xq[:, 0] * Xq[:, 1]]
            ref = ((pieces[0] + pieces[1]) + pieces[2]) + pieces[3]
            assert (np.abs(got[i] - ref) <= REL * sum(np.abs(q) for q in pieces)).all(), i
    assert np.array_equal(e.eval_function(0, th), e.eval_function(0, th, X.T))
    with pytest.raises(mhx.MhxError) as err:   # n_cols is not the function's
        e.eval_function(0, th, X[:, 0])
    assert err.value.code == mhx.capi.EINVAL
    e.close()


# ---- 5. band == evaluation, bit for bit -------------------------------------------------------------
def host_selection(prob, k):
    """the k steps of greatest prob of a NEWEST-FIRST list, equal probs newer first, NaN last: a
    stable sort of the newest-first list"""
    key = np.where(np.isnan(prob), -np.inf, prob)
    order = sorted(range(len(prob)), key=lambda i: (np.isnan(prob[i]), -key[i]))  # (stable)
    return order[:k]


def check_bands(mhx, e, fn, take, xs, chains=None):
    """fit_bands of every chain against trace + host selection + eval_function + numpy"""
    ring = e.history_capacity()
    ymax, ymin, nsel, status = e.fit_bands(fn, take, xs)
    lengths = e.state()["length"]
    for c in (range(e.n_chains) if chains is None else chains):
        prob, th = e.trace(c, ring)                  # ALL the steps the ring holds
        take_c = min(take, int(lengths[c]))
        k = min(mhx.band_count(take_c), len(prob))
        assert nsel[c] == k, (take, c, nsel[c], k)
        pick = host_selection(prob, k)
        vals = e.eval_function(fn, th[pick], xs)
        finite = np.isfinite(vals).all()
        assert status[c] == (0 if finite else 1), (take, c)
        if finite:
            assert np.array_equal(ymax[c].view(np.uint64), vals.max(axis=0).view(np.uint64)), (take, c)
            assert np.array_equal(ymin[c].view(np.uint64), vals.min(axis=0).view(np.uint64)), (take, c)
    return ymax, ymin, nsel, status


def line_engine(mhx, n_chains, **kw):
    e = mhx.Engine(n_chains, 2, 1, **kw)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    return e


def crafted(rng, n, d, centre, spread):
    """a Metropolis-like walk, newest first: runs of repeated steps"""
    prob, theta = np.empty(n), np.empty((n, d))
    p, th = 0.0, centre.copy()
    for i in range(n):
        if i == 0 or rng.random() < 0.4:
            p = rng.normal(-50.0, 3.0)
            th = centre * (1.0 + spread * rng.standard_normal(d))
        prob[i], theta[i] = p, th
    return prob[::-1].copy(), theta[::-1].copy()


def test_bands_of_crafted_line_histories(mhx):
    rng = np.random.default_rng(1)
    lengths = [1, 2, 3, 9, 64, 65, 150, 151, 1000, 1023, 1024, 300]
    e = line_engine(mhx, len(lengths), history_capacity=1024)
    e.init_chains(np.array([-1.0, 2.0]))
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted(rng, n, 2, np.array([-1.0, 2.0]), 0.3))
    for m in (1, 64, 1000, 1001):
        xs = np.linspace(-4.0, 10.0, m) if m > 1 else np.array([2.5])
        for take in (1, 3, 150, 1000, 1024):
            check_bands(mhx, e, 0, take, xs)
    # the dataset's own x
    ymax, _, _, _ = e.fit_bands(0, 150)
    assert ymax.shape == (len(lengths), 5)
    assert np.array_equal(ymax, e.fit_bands(0, 150, np.array(LF_X))[0])
    e.close()


def test_ties_at_the_threshold_and_a_nan_prob(mhx):
    e = line_engine(mhx, 3, history_capacity=64)
    e.init_chains(np.array([-1.0, 2.0]))
    # chain 0: ten steps, probs tie in threes with DIFFERENT parameters: newest first decides
    prob = np.array([-3.0, -1.0, -2.0, -1.0, -2.0, -2.0, -1.0, -3.0, -2.0, -0.0])
    # (the intercepts of the tied -2 steps 2 and 4 lie far outside the others': which of them is
    # taken shows in the envelope)
    theta = np.column_stack([[0.0, 1.0, 50.0, 3.0, -50.0, 5.0, 6.0, 7.0, 8.0, 9.0],
                             0.5 * np.arange(10.0) - 2.0])
    e.set_history(0, prob, theta)
    # chain 1: +0 and -0 are one prob; chain 2: a NaN prob (sorts last) and an inf
    p1 = np.array([0.0, -0.0, -1.0, 0.0, -0.0, -5.0])
    e.set_history(1, p1, theta[:6] * 1.5)
    p2 = np.array([-2.0, np.nan, -1.0, -3.0, -np.inf, -1.5, np.nan, -2.5])
    e.set_history(2, p2, theta[:8] - 3.0)
    xs = np.linspace(-4.0, 10.0, 64)
    for take in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
        _, _, nsel, _ = check_bands(mhx, e, 0, take, xs)
    # (take 7 of chain 0: ceiling(0.66 * 7) = 5: -0.0, the three -1 and the NEWEST -2, step 2)
    pr, th = e.trace(0, 64)
    pick = host_selection(pr, 5)
    assert sorted(pick) == [1, 2, 3, 6, 9]
    ymax, ymin, nsel, _ = e.fit_bands(0, 7, xs)
    vals = e.eval_function(0, th[pick], xs)
    assert nsel[0] == 5 and np.array_equal(ymax[0], vals.max(axis=0))
    other = e.eval_function(0, th[[1, 3, 4, 6, 9]], xs)     # (an older -2 instead: another band)
    assert not np.array_equal(other.max(axis=0), vals.max(axis=0)) or \
        not np.array_equal(other.min(axis=0), vals.min(axis=0))
    e.close()


def test_bands_of_config2_histories_of_different_lengths(mhx):
    s = pb.two_peak(n=2000, seed=5)
    rng = np.random.default_rng(2)
    lengths = [5, 150, 700, 1024, 3000, 1500]
    e = s.engine(mhx, len(lengths), history_capacity=1024)
    e.init_chains(s.theta_star)
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted(rng, n, 8, s.theta_star, 0.02))
    lens = e.state()["length"]          # (a history longer than the ring is cut to it when set)
    assert list(lens[:4]) == lengths[:4] and lens[4] >= 1024
    xs = mhx.fit_linspace(0.0, 1.0)
    for take in (1, 3, 150, 1000, 1024):
        _, _, nsel, _ = check_bands(mhx, e, 0, take, xs)
        # a take above a chain's length counts from the length
        assert nsel[0] == mhx.band_count(min(take, 5))
        assert nsel[4] == mhx.band_count(min(take, int(lens[4])))
    e.close()


def test_bands_of_a_real_walk(mhx):
    s = pb.two_peak(n=2000, seed=6)
    C_ = 256
    e = s.engine(mhx, C_, seed=3, history_capacity=2048)
    e.init_chains(pb.perturbed(s.theta_star, C_, 0.01, seed=9))
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(3200)
    assert int(e.state()["length"].min()) >= 3000      # the ring (2048) has wrapped
    xs = mhx.fit_linspace(0.0, 1.0)
    for take in (150, 1000):
        ymax, ymin, nsel, status = check_bands(mhx, e, 0, take, xs)
        assert (status == 0).all() and (nsel == mhx.band_count(take)).all()
        assert (ymax >= ymin).all()
    e.fit_bands(0, 1000, xs)
    print("fit_bands 256 chains take 1000 m 1000: kernels %.3f ms" % e.summary_timing())
    e.close()


# ---- 6. a non-finite selected value ----------------------------------------------------------------
def test_a_non_finite_value_is_flagged_for_its_chain_only(mhx):
    x = np.linspace(0.0, 1.0, 50)
    w = mhx.walker_create(function=mhx.models.poly("b", "m"), data=[x, 1.0 + 2.0 * x],
                          params=[":b", 1.0, ":m", 2.0], data_error=0.1, n_chains=3,
                          history_capacity=64)
    e = w.engine
    rng = np.random.default_rng(3)
    for c in range(3):
        pr, th = crafted(rng, 30, 2, np.array([1.0, 2.0]), 0.1)
        if c == 1:
            th[int(np.argmax(pr))] = [1e308, 1e308]      # b + m x overflows for x > 0
        e.set_history(c, pr, th)
    _, _, _, status = e.fit_bands(0, 30, x)
    assert list(status) == [0, 1, 0]
    assert mhx.walker_get_data_and_fit(w, take=30, chain=0)[6] is not None
    with pytest.raises(FloatingPointError):
        mhx.walker_get_data_and_fit(w, take=30, chain=1)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_get_data_and_fit(w, take=30)


# ---- 7 / 8. the mirror ---------------------------------------------------------------------------
def test_the_mirrors_data_and_fit(mhx):
    s = pb.two_peak(n=600, seed=12)
    x, y, sig, _ = s.data[0]
    params = []
    for k, v in zip(KEYS8, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"], ["a2", "mu2", "w2"]]),
                          data=[x, y], params=params, data_error=sig, n_chains=5, seed=2,
                          history_capacity=2048)
    mhx.walker_adaptive_steps(w, 1500)
    e = w.engine
    x_fit = mhx.fit_linspace(x.min(), x.max())
    for which, get in ((":most-likely", ":most-likely-step"), (":median", ":median-params")):
        for xs, ys in ((None, None), (0.5, -2.0)):
            every = mhx.walker_set_get_data_and_fit(w, take=1500, which_solution=which, x_shift=xs, y_shift=ys)
            assert len(every) == 5
            for c in range(5):
                one = mhx.walker_get_data_and_fit(w, take=1500, which_solution=which, x_shift=xs,
                                                  y_shift=ys, chain=c)
                assert one == every[c]
                xf, mx, mn, yf, xd, yd, pl = one
                sol = mhx.walker_get(w, get, 1500, chain=c)
                sol = sol.params if which == ":most-likely" else sol
                assert pl == sol
                th = np.array([pl[k] for k in w.param_keys])
                want = e.eval_function(0, th, x_fit)
                assert yf == [(ys or 0) + v if ys else v for v in want]
                assert xf == [(xs + v) if xs else v for v in x_fit]
                assert xd == [(xs + v) if xs else v for v in x] and yd == [(ys + v) if ys else v for v in y]
                nos = mhx.walker_get_data_and_fit_no_stddev(w, take=1500, which_solution=which,
                                                            x_shift=xs, y_shift=ys, chain=c)
                assert nos == [xf, yf, xd, yd, pl]
                if which == ":most-likely":   # take covers the ring: the best step is selected
                    assert (np.array(mx) >= np.array(yf)).all() and (np.array(yf) >= np.array(mn)).all()
    # residuals: y_fit from the dataset's own x on the device, a single stddev spread out
    xd, res, sd = mhx.walker_get_residuals(w, take=1500, chain=3)
    med = mhx.walker_get(w, ":median-params", 1500, chain=3)
    th = np.array([med[k] for k in w.param_keys])
    assert res == list(e.eval_function(0, th) - y) and xd == list(x) and sd == list(sig)
    w1 = mhx.walker_create(function=mhx.models.poly("b", "m"), data=[LF_X, LF_Y],
                           params=[":b", -1.0, ":m", 2.0], data_error=0.2)
    assert mhx.walker_get_residuals(w1)[2] == [0.2] * 5
    # a walk longer than the ring: said, in walker_get's words
    w2 = mhx.walker_create(function=mhx.models.poly("b", "m"), data=[LF_X, LF_Y],
                           params=[":b", -1.0, ":m", 2.0], data_error=0.2, history_capacity=256)
    mhx.walker_adaptive_steps_full(w2, n=700, temperature=1, auto=None)
    with pytest.warns(mhx.walker.HistoryTruncated):
        out = mhx.walker_get_data_and_fit(w2, take=200)
    assert len(out[1]) == 1000


# ---- 9. a group ------------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=1500, seed=4)
    n = 11
    rng = np.random.default_rng(7)
    walks = [crafted(rng, int(k), 8, s.theta_star, 0.02) for k in rng.integers(1, 600, n)]
    e = s.engine(mhx, n, history_capacity=512)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0], history_capacity=512)
    s.apply(g)
    e.init_chains(s.theta_star)
    g.init_chains(s.theta_star)
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
        i = 0 if c < g.ranges[1][0] else 1
        g.engines[i].set_history(c - g.ranges[i][0], pr, th)
    xs = mhx.fit_linspace(0.0, 1.0)
    for take in (1, 150, 512):
        whole, single_ = g.fit_bands(0, take, xs), e.fit_bands(0, take, xs)
        parts = [x.fit_bands(0, take, xs) for x in g.engines]
        for k in range(4):
            assert np.array_equal(whole[k], single_[k]), (take, k)
            assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), (take, k)
    e.close()
    g.close()


# ---- 10. the ABI's edges ---------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = line_engine(mhx, 2, history_capacity=64)
    xs = np.linspace(0.0, 1.0, 7)
    xp = xs.ctypes.data_as(capi.f64p)
    th = np.array([-1.0, 2.0])
    thp = th.ctypes.data_as(capi.f64p)
    out = np.zeros(7)
    op = out.ctypes.data_as(capi.f64p)
    # bands before mhx_init_chains; evaluation needs no chains
    assert lib.mhx_get_fit_bands(e._h, 0, 5, xp, 1, 7, None, None, None, None) == capi.ESTATE
    assert lib.mhx_eval_function(e._h, 0, thp, 1, xp, 1, 7, op) == capi.OK
    assert np.array_equal(out, th[0] + th[1] * xs) or np.allclose(out, th[0] + th[1] * xs, rtol=1e-15)
    e.init_chains(th)
    cap = e.history_capacity()
    for take in (0, -1, cap + 1):
        assert lib.mhx_get_fit_bands(e._h, 0, take, xp, 1, 7, None, None, None, None) == capi.EINVAL
    for fn in (-1, 1):
        assert lib.mhx_get_fit_bands(e._h, fn, 5, xp, 1, 7, None, None, None, None) == capi.EINVAL
        assert lib.mhx_eval_function(e._h, fn, thp, 1, xp, 1, 7, op) == capi.EINVAL
    assert lib.mhx_get_fit_bands(e._h, 0, 5, xp, 1, 0, None, None, None, None) == capi.EINVAL
    assert lib.mhx_eval_function(e._h, 0, thp, 1, xp, 1, 0, op) == capi.EINVAL
    assert lib.mhx_get_fit_bands(e._h, 0, 5, xp, 2, 7, None, None, None, None) == capi.EINVAL
    assert lib.mhx_eval_function(e._h, 0, thp, 1, xp, 2, 7, op) == capi.EINVAL
    assert lib.mhx_eval_function(e._h, 0, None, 1, xp, 1, 7, op) == capi.EINVAL
    assert lib.mhx_eval_function(e._h, 0, thp, -1, xp, 1, 7, op) == capi.EINVAL
    assert lib.mhx_eval_function(None, 0, thp, 1, xp, 1, 7, op) == capi.EINVAL
    # the dataset's own x: m is its point count
    assert lib.mhx_eval_function(e._h, 0, thp, 1, None, 1, 4, op) == capi.EINVAL
    assert lib.mhx_eval_function(e._h, 0, thp, 1, None, 1, 5, op) == capi.OK
    # NULL outputs are allowed, each on its own
    assert lib.mhx_get_fit_bands(e._h, 0, 5, xp, 1, 7, None, None, None, None) == capi.OK
    nsel = np.zeros(2, dtype=np.int32)
    assert lib.mhx_get_fit_bands(e._h, 0, 5, xp, 1, 7, None, None,
                                 nsel.ctypes.data_as(capi.i32p), None) == capi.OK
    assert list(nsel) == [1, 1]      # one step so far: k = min(ceiling(0.66), 1)
    assert lib.mhx_eval_function(e._h, 0, thp, 0, xp, 1, 7, None) == capi.OK
    assert e.summary_timing() >= 0.0
    e.close()


def test_portions_of_points_and_vectors(mhx):
    """more points than one portion holds, and many vectors: the same values as piece by piece"""
    e = line_engine(mhx, 1)
    m = (1 << 17) + 1000
    xs = np.linspace(-3.0, 3.0, m)
    th = np.column_stack([np.linspace(-1, 1, 70), np.linspace(2, 3, 70)])
    got = e.eval_function(0, th, xs)
    for i in (0, 33, 69):
        assert np.array_equal(got[i], e.eval_function(0, th[i], xs))
    assert np.array_equal(got[:, :100], e.eval_function(0, th, xs[:100]))
    assert np.array_equal(got[:, -100:], e.eval_function(0, th, xs[-100:]))
    e.close()
