"""mhx_get_normal_equations on the device against the numpy yardstick of its definition
(tests/normeq_cases.py), walker by walker, from the model values mhx_eval_function returns at the
walker's vector and at every perturbed one:

  jtj, jtr, chi2, g      bit for bit the yardstick (a NaN stands for any NaN), except where status
                         flags the chain: its numbers are unspecified
  status                 exactly

Every operation of the definition is a single IEEE rounding in a stated order, so there is no
tolerance anywhere but in the last test, which holds the polish to the analytic gradient (Newton
decrement <= 1e-8, as tests/test_normeq_host.py states).  Covered: point counts around the
sub-step and block edges, shared and per-chain steps, a zero step and one below the spacing of
doubles, a split of the points into chunks, the widest gather map, a global fit, every kernel path,
datasets per walker in all four sigma kinds and both forms, a group, the ABI's edges and the
mirror."""
import numpy as np
import pytest

import normeq_cases as nc
import problems as pb

pytestmark = pytest.mark.gpu

CHUNK = 1 << 17                 # kFitChunkPoints
KEYS = ("jtj", "jtr", "chi2", "status")


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    assert lisp_mcmc_amd.capi.NORMEQ_BLOCK == nc.BLOCK and CHUNK % nc.BLOCK == 0
    return lisp_mcmc_amd


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return nc.same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def check(e, fn, theta, steps, lik, y_of, sigma_of, reads, flagged=(), where=""):
    """Engine.normal_equations of function fn against the yardstick on every chain; y_of(c),
    sigma_of(c): walker c's data.  Returns the pointwise result and the yardstick's."""
    import lisp_mcmc_amd
    r = e.normal_equations(fn, theta, steps, pointwise=True)
    bare = e.normal_equations(fn, theta, steps)
    assert set(bare) == set(KEYS) and set(r) == set(KEYS) | {"g"}
    th = e.state()["best_theta"] if theta is None else np.asarray(theta, dtype=np.float64)
    hs = lisp_mcmc_amd.normeq_steps(th) if steps is None else np.broadcast_to(np.asarray(steps, float), th.shape)
    wants = []
    for c in range(e.n_chains):
        at = (where, fn, c)
        want = nc.yardstick(lambda t: e.eval_function(fn, t), lik, th[c], hs[c], reads, y_of(c), sigma_of(c))
        wants.append(want)
        assert r["status"][c] == want["status"] == (nc.NONFINITE if c in flagged else 0), at
        if c not in flagged:
            for k in ("jtj", "jtr", "chi2", "g"):
                assert nc.same_bits(r[k][c], want[k]), (at, k, r[k][c], want[k])
            assert np.array_equal(r["jtj"][c], r["jtj"][c].T), at
    clean = [c for c in range(e.n_chains) if c not in flagged]
    for k in KEYS:              # the pointwise output changes nothing
        assert same(bare[k][clean], r[k][clean]), (where, k)
    return r, wants


def shared(y, sigma):
    return (lambda c: y), (lambda c: sigma)


# ---- 1. the line model: point counts and steps -------------------------------------------------------
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


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 3])
def test_line_model_point_counts_and_steps(mhx, N):
    for n_chains in (9, 7):                # no multiple of the waves per workgroup
        e, y, sig, start = line_engine(mhx, n_chains, N, seed=N + n_chains)
        rng = np.random.default_rng(N)
        r0, _ = check(e, 0, None, None, nc.NORMAL, *shared(y, sig), [0, 1], where="most-likely")
        other = start * (1.0 + 0.01 * rng.standard_normal(start.shape))
        r1, _ = check(e, 0, other, [1e-3, 2e-3], nc.NORMAL, *shared(y, sig), [0, 1], where="given, shared steps")
        assert not nc.same_bits(r0["chi2"], r1["chi2"])
        per = rng.uniform(1e-4, 1e-2, start.shape)
        check(e, 0, other, per, nc.NORMAL, *shared(y, sig), [0, 1], where="given, per-chain steps")
        # one step 0: the column is exactly +0.0, for that chain only
        per[2, 1] = 0.0
        rz, _ = check(e, 0, other, per, nc.NORMAL, *shared(y, sig), [0, 1], where="a zero step")
        assert not rz["g"][2, 1].any() and not np.signbit(rz["g"][2, 1]).any()
        assert rz["jtr"][2, 1] == 0.0 and not rz["jtj"][2, 1].any() and not rz["jtj"][2, :, 1].any()
        assert not np.signbit(rz["jtj"][2]).any() and rz["jtj"][2, 0, 0] > 0.0 and rz["jtj"][3, 1, 1] > 0.0
        # one step below the spacing of doubles at theta: dh == 0, flagged, the neighbours untouched
        per[2, 1] = 1e-3
        tiny = per.copy()
        tiny[4, 0] = 1e-30
        rt, _ = check(e, 0, other, tiny, nc.NORMAL, *shared(y, sig), [0, 1], flagged=(4,), where="dh == 0")
        rp, _ = check(e, 0, other, per, nc.NORMAL, *shared(y, sig), [0, 1], where="per-chain again")
        for k in KEYS + ("g",):
            for c in range(n_chains):
                if c != 4:
                    assert same(rt[k][c], rp[k][c]), (k, c)
        assert e.summary_timing() >= 0.0
        e.close()


def test_hand_case_through_the_device(mhx):
    e = mhx.Engine(1, 2, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [2.0], [3.5], [0.5])
    e.init_chains(np.array([1.0, 1.0]))
    r, _ = check(e, 0, None, [0.5, 0.25], nc.NORMAL, *shared(np.array([3.5]), np.array([0.5])), [0, 1])
    assert r["chi2"][0] == 1.0 and r["g"][0].tolist() == [[2.0], [4.0]]
    assert r["jtj"][0].tolist() == [[4.0, 8.0], [8.0, 16.0]] and r["jtr"][0].tolist() == [2.0, 4.0]
    e.close()


# ---- 2. chunks and call forms --------------------------------------------------------------------------
def test_points_beyond_one_chunk_and_call_forms(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    N = CHUNK + 1024 + 5
    e, y, sig, start = line_engine(mhx, 2, N, seed=1)
    hs = np.array([1e-3, 1e-4])
    r, _ = check(e, 0, None, hs, nc.NORMAL, *shared(y, sig), [0, 1])
    again = e.normal_equations(0, None, hs, pointwise=True)
    for k in r:
        assert same(r[k], again[k]), k                  # the same bits on a second call
    # outputs partly NULL: every other one, then the others
    order = ("jtj", "jtr", "chi2", "g", "status")
    hp = hs.ctypes.data_as(capi.f64p)
    for keep in (0, 1):
        got = {k: np.zeros_like(r[k]) for i, k in enumerate(order) if i % 2 == keep}
        ptr = [got[k].ctypes.data_as(capi.i32p if got[k].dtype == np.int32 else capi.f64p)
               if k in got else None for k in order]
        assert lib.mhx_get_normal_equations(e._h, 0, None, hp, 0, *ptr) == capi.OK
        for k in got:
            assert same(got[k], r[k]), (keep, k)
    assert lib.mhx_get_normal_equations(e._h, 0, None, hp, 0, *([None] * 5)) == capi.OK
    e.close()


# ---- 3. the widest gather map --------------------------------------------------------------------------
def test_a_polynomial_of_32_coefficients_through_a_shuffled_gather_map(mhx, monkeypatch):
    """the greatest task count (561) and LDS tile; the 31 places the function does not read are 0
    (on the generic kernel: a polynomial type of its own would be compiled for seconds first)"""
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    rng = np.random.default_rng(2)
    d, N, C = 63, 1100, 2
    idx = rng.permutation(d)[:32]
    x = np.linspace(-1.0, 1.0, N)
    coef = rng.uniform(-1.0, 1.0, 32)
    sig = rng.uniform(0.05, 0.1, N)
    y = pb.model_eval_np(pb.POLY, (), coef, x) + sig * rng.standard_normal(N)
    theta = rng.uniform(-1.0, 1.0, (C, d))
    theta[:, idx] = coef * (1.0 + 0.01 * rng.standard_normal((C, 32)))
    e = mhx.Engine(C, d, 1)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [int(t) for t in idx])
    e.set_dataset(0, x, y, sig)
    e.init_chains(theta)
    assert "generic" in e.kernel_name()
    r, _ = check(e, 0, None, None, nc.NORMAL, *shared(y, sig), idx)
    unread = sorted(set(range(d)) - set(idx.tolist()))
    assert len(unread) == 31
    for k, ax in (("jtj", 1), ("jtj", 2), ("jtr", 1), ("g", 1)):
        part = np.take(r[k], unread, axis=ax)
        assert not part.any() and not np.signbit(part).any(), k
    assert (r["jtj"][:, idx, idx] > 0.0).all()
    e.close()


# ---- 4. a global fit -----------------------------------------------------------------------------------
def test_two_functions_that_share_a_parameter(mhx):
    from importlib import import_module
    walker = import_module("lisp-mcmc_amd.walker")
    rng = np.random.default_rng(3)
    x0, x1 = np.linspace(0.0, 5.0, 130), np.linspace(-1.0, 1.0, 70)
    s0, s1 = rng.uniform(0.05, 0.2, x0.size), rng.uniform(0.1, 0.2, x1.size)
    y0 = 1.0 + 0.5 * x0 + s0 * rng.standard_normal(x0.size)
    y1 = 1.0 - 0.3 * x1 + s1 * rng.standard_normal(x1.size)
    C = 5
    e = mhx.Engine(C, 3, 2)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_function(1, mhx.capi.MODEL_POLY, (), [0, 2])
    e.set_dataset(0, x0, y0, s0)
    e.set_dataset(1, x1, y1, s1)
    th = np.array([1.0, 0.5, -0.3]) * (1.0 + 0.05 * rng.standard_normal((C, 3)))
    e.init_chains(th)
    ra, _ = check(e, 0, None, None, nc.NORMAL, *shared(y0, s0), [0, 1], where="function 0")
    rb, _ = check(e, 1, None, None, nc.NORMAL, *shared(y1, s1), [0, 2], where="function 1")
    assert not ra["jtj"][:, 2].any() and not rb["jtj"][:, 1].any()
    F, b, chi2, status = walker._normal_equations_all(e, th, mhx.normeq_steps(th))
    assert same(F, ra["jtj"] + rb["jtj"]) and same(b, ra["jtr"] + rb["jtr"]) and same(chi2, ra["chi2"] + rb["chi2"])
    assert not status.any()
    e.close()


# ---- 5. every kernel path ------------------------------------------------------------------------------
def spread(s, n, seed, scale=0.02):
    return pb.perturbed(s.theta_star, n, scale, seed=seed)


def run_spec(mhx, s, name, lik=nc.NORMAL, n=11, seed=1):
    e = s.engine(mhx, n)
    e.init_chains(spread(s, n, seed))
    assert name in e.kernel_name(), e.kernel_name()
    _, y, sig, _ = s.data[0]
    check(e, 0, None, None, lik, *shared(y, sig), range(s.d), where=name)
    check(e, 0, spread(s, n, seed + 1), spread(s, n, seed + 2, 0.3) * 1e-5, lik, *shared(y, sig), range(s.d),
          where=name + ", given")
    e.close()


@pytest.mark.parametrize("n", [334, 1500])
def test_two_peak_on_the_ahead_of_time_kernel(mhx, n):
    run_spec(mhx, pb.two_peak(n=n, seed=3), "gauss22_normal")


@pytest.mark.parametrize("n", [334, 1500])
def test_the_generic_kernel(mhx, monkeypatch, n):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    run_spec(mhx, pb.two_peak(n=n, seed=6), "generic")


def test_the_cutoff_likelihood_is_the_normal_one_here(mhx):
    run_spec(mhx, pb.two_peak(n=334, seed=4, lik=pb.CUTOFF), "gauss22_cutoff", lik=nc.CUTOFF)


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


LORENTZ_12 = ("(lambda (x &key bg a1 mu1 w1 a2 mu2 w2 &allow-other-keys)"
              " (+ bg (/ a1 (+ 1 (expt (/ (- x mu1) w1) 2))) (/ a2 (+ 1 (expt (/ (- x mu2) w2) 2)))))")


def test_lorentzians_enumerated_and_the_closure_as_text(mhx, monkeypatch):
    rng = np.random.default_rng(7)
    th = np.array([0.2, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08])
    x = np.linspace(0.0, 1.0, 1500)
    sig = rng.uniform(0.05, 0.15, x.size)
    y = pb.model_eval_np(pb.LORENTZ, (1, 2), th, x) + sig * rng.standard_normal(x.size)
    s = pb.Spec(7)
    s.add(pb.LORENTZ, (1, 2), range(7), x, y, sig, pb.NORMAL)
    s.theta_star = th
    run_spec(mhx, s, "PeaksModel<1, 2, true>")
    keys, expr = mhx.sexpr.lambda_to_expr(LORENTZ_12)
    for no_recognise, name in (("0", "PeaksModel<1, 2, true>"), ("1", "rtc[expr")):
        monkeypatch.setenv("MHX_NO_RECOGNISE", no_recognise)
        e = mhx.Engine(11, 7, 1)
        e.set_function_expr(0, expr, keys, list(range(7)))
        e.set_dataset(0, x, y, sig)
        e.init_chains(spread(s, 11, 5))
        assert name in e.kernel_name(), e.kernel_name()
        check(e, 0, None, None, nc.NORMAL, *shared(y, sig), range(7), where="text " + no_recognise)
        e.close()


def test_an_expression_over_two_columns_of_x(mhx):
    rng = np.random.default_rng(11)
    n = 334
    X = np.column_stack([rng.uniform(-1, 2, n), rng.uniform(0, 3, n)])
    th = np.array([0.4, 1.3, -0.7, 0.25])
    sig = rng.uniform(0.1, 0.3, n)
    y = th[0] + th[1] * X[:, 0] + th[2] * X[:, 1] + th[3] * X[:, 0] * X[:, 1] + sig * rng.standard_normal(n)
    e = mhx.Engine(11, 4, 1)
    e.set_function_expr(0, "a + b*xcol0 + c*xcol1 + d*xcol0*xcol1", list("abcd"), [0, 1, 2, 3])
    e.set_dataset(0, X, y, sig)
    e.init_chains(pb.perturbed(th, 11, 0.05, seed=2))
    check(e, 0, None, None, nc.NORMAL, *shared(y, sig), range(4))
    e.close()


def test_poisson_and_a_rate_that_is_not_positive(mhx, monkeypatch):
    """Fisher scoring; a v_i <= 0 in one chain sets that chain's status and no other's (on the
    generic kernel: a two-peak Poisson type would be compiled for seconds first)"""
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    s = pb.poisson_peaks(n=600, npk=2)
    n = 11
    e = s.engine(mhx, n)
    e.init_chains(s.theta_star)
    assert "generic" in e.kernel_name()
    _, y, _, _ = s.data[0]
    th = spread(s, n, 9, 0.01)
    clean, wants = check(e, 0, th, None, nc.POISSON, *shared(y, None), range(s.d))
    z = e.residuals(0, th, pointwise=True)["z"]
    for c in range(n):
        assert nc.same_bits(wants[c]["u"], -z[c]), c
    spoilt = th.copy()
    spoilt[4, 0] = -3.0                    # the background of chain 4 below zero: v < 0 between the peaks
    assert (e.eval_function(0, spoilt[4]) <= 0.0).any()
    hs = mhx.normeq_steps(th)
    r, _ = check(e, 0, spoilt, hs, nc.POISSON, *shared(y, None), range(s.d), flagged=(4,))
    ref, _ = check(e, 0, th, hs, nc.POISSON, *shared(y, None), range(s.d))
    for k in KEYS + ("g",):
        for c in range(n):
            if c != 4:
                assert same(r[k][c], ref[k][c]), (k, c)
    e.close()


def test_u_is_the_exact_negation_of_the_residuals(mhx):
    s = pb.two_peak(n=334, seed=8)
    e = s.engine(mhx, 11)
    th = spread(s, 11, 4)
    e.init_chains(th)
    _, y, sig, _ = s.data[0]
    r, wants = check(e, 0, None, None, nc.NORMAL, *shared(y, sig), range(8))
    res = e.residuals(0, None, pointwise=True)
    for c in range(11):
        assert nc.same_bits(wants[c]["u"], -res["z"][c]), c
        # chi2 sums the same squares in another order: the same number to rounding, not to the bit
        assert abs(r["chi2"][c] - res["chi2"][c]) <= 334 * 2.0 ** -52 * r["chi2"][c]
    e.close()


# ---- 6. a dataset per walker ---------------------------------------------------------------------------
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
def test_planes_every_sigma_kind_in_both_forms(mhx, monkeypatch, kind):
    C, N = 5, 300
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
        runs[no_lds], _ = check(e, 0, None, None, nc.NORMAL, lambda c: y[c], sig_of, [0, 1],
                                where="planes %s" % no_lds)
        given = truth[::-1].copy()                   # every walker at another walker's parameters
        check(e, 0, given, None, nc.NORMAL, lambda c: y[c], sig_of, [0, 1], where="planes given")
        e.close()
    for k in KEYS + ("g",):
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
    r, _ = check(e, 0, None, None, nc.NORMAL, lambda c: y[c], sig_of, [0, 1], where="planes, two chunks")
    assert r["g"].shape == (C, 2, N) and r["chi2"][0] != r["chi2"][1]
    e.close()


# ---- 7. a group ----------------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=334, seed=4)
    n = 11
    start, given = spread(s, n, 7), spread(s, n, 8)
    per = spread(s, n, 9, 0.3) * 1e-5
    e = s.engine(mhx, n)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0])
    s.apply(g)
    e.init_chains(start)
    g.init_chains(start)
    for theta, steps in ((None, None), (given, per), (given, per[0])):
        whole = g.normal_equations(0, theta, steps, pointwise=True)
        one = e.normal_equations(0, theta, steps, pointwise=True)
        for k in one:
            assert same(whole[k], one[k]), k
    e.close()
    g.close()
    C, N = 7, 130
    x, y, sigma, rows, truth = plane_data(N, C, PER_POINT, seed=5)
    e = mhx.Engine(C, 2, 1)
    g = mhx.Group(C, 2, 1, devices=[0, 0])
    for t in (e, g):
        t.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
        t.set_dataset_planes(0, x, y, sigma, PER_POINT)
        t.init_chains(truth)
    whole, one = g.normal_equations(0, pointwise=True), e.normal_equations(0, pointwise=True)
    for k in one:
        assert same(whole[k], one[k]), k
    e.close()
    g.close()


# ---- 8. the ABI's edges --------------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = mhx.Engine(2, 2, 1)
    e.set_function(0, capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0], np.full(5, 0.2))
    jtj, chi2 = np.full((2, 2, 2), 7.5), np.full(2, 7.5)
    status = np.full(2, -3, dtype=np.int32)
    outs = (jtj.ctypes.data_as(capi.f64p), None, chi2.ctypes.data_as(capi.f64p), None, status.ctypes.data_as(capi.i32p))

    def call(h, fn, steps, per_chain=0):
        hs = np.ascontiguousarray(steps, dtype=np.float64)
        return lib.mhx_get_normal_equations(h, fn, None, hs.ctypes.data_as(capi.f64p), per_chain, *outs)
    ok = [1e-3, 1e-3]
    assert call(e._h, 0, ok) == capi.ESTATE                                   # before mhx_init_chains
    e.init_chains(np.array([-1.0, 2.0]))
    for fn in (-1, 1):
        assert call(e._h, fn, ok) == capi.EINVAL
    for bad in (-1e-3, float("nan"), float("inf")):
        assert call(e._h, 0, [1e-3, bad]) == capi.EINVAL
        assert "step" in lib.mhx_last_error().decode()
        assert call(e._h, 0, [[1e-3, 1e-3], [bad, 1e-3]], 1) == capi.EINVAL    # the second chain's
    assert lib.mhx_get_normal_equations(e._h, 0, None, None, 0, *outs) == capi.EINVAL
    assert call(None, 0, ok) == capi.EINVAL
    assert (jtj == 7.5).all() and list(chi2) == [7.5, 7.5] and list(status) == [-3, -3]   # untouched on error
    assert call(e._h, 0, ok) == capi.OK
    assert (jtj != 7.5).all() and (chi2 != 7.5).all() and list(status) == [0, 0]
    with pytest.raises(ValueError):
        e.normal_equations(0, np.zeros((3, 2)))
    with pytest.raises(ValueError):
        e.normal_equations(0, None, np.zeros(3))
    e.close()
    # an expression likelihood: refused by name
    rng = np.random.default_rng(7)
    x = np.linspace(0.0, 3.0, 290)
    sig = rng.uniform(0.05, 0.2, x.size)
    y = 2.0 * np.exp(-x / 0.7) + sig * rng.standard_normal(x.size)
    t = mhx.Engine(2, 2, 1)
    t.set_expr_recognition(False)
    t.set_function_expr(0, "a*exp(-x/tau)", ["a", "tau"], [0, 1])
    t.set_dataset(0, x, y, sig, likelihood=capi.LIK_EXPR)
    t.set_likelihood_expr(0, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")
    t.init_chains(np.array([2.0, 0.7]))
    chi2[:] = 7.5
    assert call(t._h, 0, ok) == capi.EUNSUPPORTED
    assert "MHX_LIK_EXPR" in lib.mhx_last_error().decode() and list(chi2) == [7.5, 7.5]
    with pytest.raises(mhx.MhxError) as err:
        t.normal_equations(0)
    assert err.value.code == capi.EUNSUPPORTED
    t.close()


# ---- 9. the mirror -------------------------------------------------------------------------------------
def same_entry(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
    return True


def test_laplace_of_a_set_and_of_one_walker_and_its_l_matrix(mhx):
    rng = np.random.default_rng(12)
    x = np.linspace(0.0, 1.0, 150)
    one = np.array([0.5, 0.3, 1.0, 0.4, 0.06])
    y = pb.model_eval_np(pb.GAUSS, (2, 1), one, x) + 0.1 * rng.standard_normal(x.size)
    w = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"]]),
                          data=[x, y], params=[":b0", 0.5, ":b1", 0.3, ":a1", 1.0, ":mu1", 0.4, ":w1", 0.06],
                          data_error=0.1, n_chains=3, seed=2, history_capacity=1024)
    every = mhx.walker_set_laplace(w)
    assert len(every) == 3
    raw = w.engine.normal_equations(0)
    for c in range(3):
        assert same_entry(every[c], mhx.walker_laplace(w, chain=c))
        s = every[c]
        assert s["status"] == 0 and s["chi2"] == raw["chi2"][c] and s["dof"] == 150 - 5
        assert np.array_equal(s["gradient"], raw["jtr"][c])
        assert np.allclose(s["covariance-matrix"] @ raw["jtj"][c], np.eye(5), atol=1e-8)
    held = mhx.walker_set_laplace(w, fixed=[":b1"])[0]
    assert held["varied-keys"] == ["b0", "a1", "mu1", "w1"] and not held["l-matrix"][1].any()
    # the l-matrix goes straight into the walk: one per walker, bit for bit
    L = np.array([s["l-matrix"] for s in every])
    w.engine.adaptive_begin(200, 10.0, 1, l_matrix=L)
    assert np.array_equal(w.engine.lmatrix(), L)
    w.engine.adaptive_advance(1 << 30)
    assert (w.engine.state()["length"] > 1).all()
    mhx.walker_adaptive_steps_full(w, n=200, temperature=10, l_matrix=L[0])
    w.engine.close()


def lorentz_jacobian(th, x):
    J = [np.ones_like(x)]
    for k in range(2):
        A, mu, w = th[1 + 3 * k: 4 + 3 * k]
        t = (x - mu) / w
        q = 1.0 / (1.0 + t * t)
        J += [q, A * q * q * 2.0 * t / w, A * q * q * 2.0 * t * t / w]
    return np.array(J)


def test_least_squares_polishes_eleven_spectra(mhx):
    rng = np.random.default_rng(13)
    C, N = 11, 334
    x = np.linspace(0.0, 1.0, N)
    truth = np.array([0.2, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08]) * (1.0 + 0.02 * rng.standard_normal((C, 7)))
    sigma = rng.uniform(0.02, 0.04, C)
    y = np.array([pb.model_eval_np(pb.LORENTZ, (1, 2), truth[c], x) for c in range(C)])
    y = y + sigma[:, None] * rng.standard_normal((C, N))
    keys = ["bg", "a1", "mu1", "w1", "a2", "mu2", "w2"]
    start = truth * (1.0 + 0.05 * rng.standard_normal((C, 7)))
    w = mhx.walker_set_create(function=mhx.models.lorentz_peaks(["bg"], [["a1", "mu1", "w1"], ["a2", "mu2", "w2"]]),
                              datasets=[[x, y[c]] for c in range(C)],
                              params=[dict(zip(keys, start[c])) for c in range(C)],
                              data_error=[float(s) for s in sigma], seed=3)
    assert np.array_equal(w.engine.state()["best_theta"], start)
    before = w.engine.logpost(start)
    r = mhx.walker_set_least_squares(w, iterations=25)
    assert np.array_equal(w.engine.state()["theta"], start)                   # apply=False moves nothing

    def decrement(th, c):
        g = lorentz_jacobian(th, x) / sigma[c]
        u = (y[c] - pb.model_eval_np(pb.LORENTZ, (1, 2), th, x)) / sigma[c]
        b = g @ u
        return float(b @ np.linalg.solve(g @ g.T, b))
    dec = [decrement(r["theta"][c], c) for c in range(C)]
    print("greatest Newton decrement %.3g, iterations %s" % (max(dec), r["iterations"].tolist()))
    assert max(dec) <= 1e-8
    assert (r["objective"] > before).all() and len(r["laplace"]) == C
    assert all(s["status"] == 0 and s["newton-decrement"] <= 1e-6 for s in r["laplace"])
    assert [list(p) for p in r["params"]] == [keys] * C
    again = mhx.walker_set_least_squares(w, iterations=25, apply=True)
    assert np.array_equal(again["theta"], r["theta"])
    st = w.engine.state()
    assert np.array_equal(st["theta"], r["theta"]) and np.array_equal(st["best_theta"], r["theta"])
    w.engine.close()
