"""A dataset per walker (mhx_set_dataset_planes, walker_set_create) against the oracle used as it
is: one Problem per walker holding that walker's (x, y, sigma), one orc.Walker per walker with
chain_id = c.  `-m gpu`: needs an MI355X.

Tolerance: the project's own (tests/test_gpu_parity.py): 1e-12 * abs_terms + 4 * PRIOR_ULP *
violations.  Sizes: 334 points (one ragged block pair, resident in LDS in every sigma kind and
family) and 1500 points (streamed; more than one 8-wave tile); C = 11 walkers (two workgroups of
the 8-wave family, the second partial); every walker's y drawn from its own perturbed theta."""
import numpy as np
import pytest

import problems as pb
from test_gpu_parity import PRIOR_ULP, n_violations, tol_for

pytestmark = pytest.mark.gpu

NONE, SHARED, PER_CHAIN, PER_POINT = 0, 1, 2, 3
KINDS = [NONE, SHARED, PER_CHAIN, PER_POINT]
C11 = 11


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


class Planes:
    """C walkers on `n` points of pb.two_peak's problem (or its Lorentzian {1, 2} cousin): one
    pb.Spec per walker for the oracle, the planes for the engine"""

    def __init__(self, n, C, kind, seed=1, model=pb.GAUSS, shape=(2, 2)):
        rng = np.random.default_rng(1000 + seed)
        base = pb.two_peak(n=n, seed=seed)
        self.x = base.data[0][0]
        if model == pb.GAUSS:
            self.theta_star = base.theta_star
        else:  # bg a1 mu1 w1 a2 mu2 w2
            self.theta_star = np.array([0.5, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08])
        self.d = self.theta_star.size
        self.model, self.shape, self.kind, self.C, self.n = model, shape, kind, C, n
        self.truth = pb.perturbed(self.theta_star, C, 0.02, seed=seed + 7)
        if kind == NONE:
            self.sigma, rows = None, np.ones((C, n))
        elif kind == SHARED:
            self.sigma = rng.uniform(0.05, 0.15, n)
            rows = np.tile(self.sigma, (C, 1))
        elif kind == PER_CHAIN:
            self.sigma = rng.uniform(0.05, 0.15, C)
            rows = np.repeat(self.sigma[:, None], n, axis=1)
        else:
            self.sigma = rows = rng.uniform(0.05, 0.15, (C, n))
        self.rows = rows
        noise = np.where(kind == NONE, 0.1, rows) * rng.standard_normal((C, n))
        self.y = np.array([pb.model_eval_np(model, shape, self.truth[c], self.x) for c in range(C)]) + noise
        th = self.theta_star
        lo, hi = np.minimum(th * 0.5, th * 1.5), np.maximum(th * 0.5, th * 1.5)
        self.bounds = (list(range(self.d)), lo, hi)
        self.specs = []
        for c in range(C):
            s = pb.Spec(self.d)
            s.add(model, shape, range(self.d), self.x, self.y[c], None if kind == NONE else rows[c],
                  pb.NORMAL, self.bounds)
            s.theta_star = th
            self.specs.append(s)

    def oracles(self, orc):
        return [s.oracle(orc) for s in self.specs]

    def sigma_of(self, rows):
        if self.kind in (NONE, SHARED):
            return self.sigma
        return np.ascontiguousarray(self.sigma[rows])

    def define(self, e, rows=None):
        rows = slice(None) if rows is None else rows
        e.set_function(0, self.model, self.shape, list(range(self.d)))
        e.set_dataset_planes(0, self.x, np.ascontiguousarray(self.y[rows]), self.sigma_of(rows), self.kind)
        e.set_bounds(0, *self.bounds)
        return e

    def engine(self, mhx, rows=None, **kw):
        C = self.C if rows is None else len(self.y[rows])
        return self.define(mhx.Engine(C, self.d, 1, **kw), rows)

    def start(self, seed=3):
        return pb.perturbed(self.theta_star, self.C, 0.01, seed=seed)


_cases = {}


def case(n, C, kind, **kw):
    key = (n, C, kind, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Planes(n, C, kind, **kw)
    return _cases[key]


def form_of(e):
    name = e.kernel_name()
    assert "+planes(" in name, name
    return name.split("+planes(")[1].split(")")[0]


# ---- 1. mhx_logpost against the per-walker oracles ---------------------------------------------
@pytest.mark.parametrize("n", [334, 1500])
@pytest.mark.parametrize("kind", KINDS)
def test_logpost_against_the_per_walker_oracles(mhx, orc, n, kind):
    p = case(n, C11, kind)
    ops = p.oracles(orc)
    th = pb.perturbed(p.theta_star, C11, 0.3, seed=5)       # (wide: some bounds are violated)
    assert sum(n_violations(p.specs[0], t) for t in th) > 0
    e = p.engine(mhx)
    got, parts = e.logpost(np.tile(th, (3, 1)), parts=True)
    assert form_of(e) == ("resident" if n == 334 else "streamed")
    for i in range(C11):
        ref, rparts = ops[i].logpost(th[i], parts=True)
        nv = n_violations(p.specs[i], th[i])
        tol = tol_for(ops[i], th[i], nv)
        print("kind %d n %d walker %d: |gpu - oracle| = %.3g, tol %.3g" % (kind, n, i, abs(got[i] - ref), tol))
        assert abs(got[i] - ref) <= tol, (i, got[i], ref, tol)
        assert abs(parts[i, 0] - rparts[0]) <= tol
        assert abs(parts[i, 1] - rparts[1]) <= 4 * PRIOR_ULP * max(1, nv)
        # rows i, i + C, i + 2C: the data of walker i mod C - the same bits
        assert got[i] == got[i + C11] == got[i + 2 * C11]
    # ... and another walker's data gives another number
    assert len(set(e.logpost(np.tile(th[0], (C11, 1))).tolist())) == C11
    e.close()


# ---- 2. the same bits in both forms and both families ------------------------------------------
def _walk_plain(p, mhx, th0, L):
    e = p.engine(mhx, seed=17)
    lp = e.logpost(th0)
    e.init_chains(th0)
    e.many_steps(300, L)
    st = e.state()
    out = {"form": form_of(e), "name": e.kernel_name(), "lp": lp, "theta": st["theta"],
           "logpost": st["logpost"], "age": st["age"], "trace": [e.trace(c, 30) for c in range(p.C)]}
    e.close()
    return out


@pytest.mark.parametrize("n,kind", [(334, PER_CHAIN), (334, PER_POINT), (334, SHARED), (334, NONE),
                                    (1500, PER_CHAIN), (1500, PER_POINT)])
def test_same_bits_across_forms_and_families(mhx, monkeypatch, n, kind):
    p = case(n, C11, kind)
    th0 = p.start()
    L = np.diag(0.004 * np.abs(p.theta_star))
    runs = {}
    for wpg in ("8", "16"):
        for no_lds in ("0", "1"):
            monkeypatch.setenv("MHX_FAMILY_WPG", wpg)
            monkeypatch.setenv("MHX_PLANES_NO_LDS", no_lds)
            runs[wpg, no_lds] = _walk_plain(p, mhx, th0, L)
    for wpg in ("8", "16"):
        assert runs[wpg, "0"]["form"] == ("resident" if n == 334 else "streamed")
        assert runs[wpg, "1"]["form"] == "streamed"
        assert runs[wpg, "0"]["name"].startswith("w" + wpg + "/")
    ref = runs["8", "0"]
    assert len(np.unique(ref["age"])) > 1 or ref["age"][0] > 1        # (the walk did move)
    for key, r in runs.items():
        for k in ("lp", "theta", "logpost", "age"):
            assert np.array_equal(r[k], ref[k]), (key, k)
        for c in range(p.C):
            assert np.array_equal(r["trace"][c][0], ref["trace"][c][0]), (key, c)
            assert np.array_equal(r["trace"][c][1], ref["trace"][c][1]), (key, c)


# ---- 3. mhx_step_injected against the oracle walkers -------------------------------------------
def run_injected(mhx, orc, e, ops, specs, th0, theta_star, n_steps, seed=0, T=None, scale=0.02):
    """tests/test_gpu_parity.py's run_injected with one oracle problem per walker"""
    rng = np.random.default_rng(seed)
    C, d = th0.shape
    e.init_chains(th0)
    ws = [orc.Walker(ops[c], th0[c]) for c in range(C)]
    L = np.array([np.tril(rng.normal(size=(d, d))) * scale * np.abs(theta_star)[:, None] for _ in range(C)])
    n_acc = 0
    for it in range(n_steps):
        z = rng.standard_normal((C, d))
        u = 1.0 - rng.random(C)
        Ts = np.ones(C) if T is None else T[it]
        acc = e.step_injected(L, z, u, Ts)
        st = e.state()
        for c in range(C):
            a = ws[c].take_step_injected(L[c], z[c], u[c], Ts[c])
            th_o, pr_o = ws[c].last()
            if a != acc[c]:
                pytest.fail("accept decision differs (walker %d step %d)" % (c, it))
            n_acc += int(a)
            assert np.array_equal(st["theta"][c], th_o), (c, it)
            assert abs(st["logpost"][c] - pr_o) <= tol_for(ops[c], th_o, n_violations(specs[c], th_o))
    for c in range(C):
        assert st["length"][c] == ws[c].length and st["age"][c] == ws[c].age
        bt, bp = ws[c].best()
        assert np.array_equal(st["best_theta"][c], bt)
        n1, d1 = ws[c].acceptance(50)
        assert e.acceptance(50)[c] == n1 / d1
        pr, th = e.trace(c, 30)
        opr, oth = ws[c].trace(30)
        assert np.array_equal(th, oth) and np.allclose(pr, opr, rtol=0, atol=1e-6)
    return n_acc


def test_step_injected_against_the_oracle_walkers(mhx, orc):
    p = case(334, C11, PER_CHAIN)
    e = p.engine(mhx)
    n_acc = run_injected(mhx, orc, e, p.oracles(orc), p.specs, p.start(seed=22), p.theta_star, 60)
    assert 0 < n_acc < 60 * C11
    e.close()


# ---- 4. mhx_adaptive_* against the oracle walkers ----------------------------------------------
def compare_adaptive(mhx, orc, p, e, seed, n=3200, temperature=10.0, auto=1,
                     checkpoints=(1, 199, 200, 201, 1000, 1001, 2000)):
    """tests/test_gpu_parity.py's compare_adaptive with one oracle problem per walker"""
    ops = p.oracles(orc)
    th0 = p.start(seed=seed)
    e.init_chains(th0)
    ws = [orc.Walker(ops[c], th0[c]) for c in range(p.C)]
    e.adaptive_begin(n, temperature, auto)
    for c, w in enumerate(ws):
        w.adaptive_begin(n, temperature, auto, seed=seed, chain_id=c)
    assert np.array_equal(e.lmatrix(), np.array([w.current_l() for w in ws]))
    done = 0
    for m in list(checkpoints) + [1 << 40]:
        running = e.adaptive_advance(m - done)
        for w in ws:
            w.adaptive_advance(m - done)
        done = m
        st = e.state()
        status, loop_i = e.chain_status()
        Ls, Ts = e.lmatrix(), e.temperature()
        for c, w in enumerate(ws):
            th, pr = w.last()
            assert loop_i[c] == w.loop_index, (c, m)
            assert status[c] == w.status, (c, m)
            assert np.array_equal(st["theta"][c], th), (c, m)
            assert st["age"][c] == w.age and st["length"][c] == w.length
            assert np.array_equal(Ls[c], w.current_l()), (c, m)
            assert Ts[c] == w.temperature
        if running == 0:
            break
    assert all(w.status == orc.DONE for w in ws)
    return ws


@pytest.mark.parametrize("n,kind", [(334, PER_CHAIN), (1500, PER_POINT)])
def test_adaptive_against_the_oracle_walkers(mhx, orc, n, kind):
    p = case(n, 6, kind, seed=4)
    e = p.engine(mhx, seed=77)
    assert form_of_after_finalise(e, p) == ("resident" if n == 334 else "streamed")
    compare_adaptive(mhx, orc, p, e, seed=77)
    e.close()


def form_of_after_finalise(e, p):
    e.logpost(p.theta_star[None, :])
    return form_of(e)


# ---- 5. repacking --------------------------------------------------------------------------------
def _walk_adaptive(e, th0, n=3200, chunk=150):
    e.init_chains(th0)
    e.adaptive_begin(n, 10.0, 1)
    while e.adaptive_advance(chunk) > 0:
        pass
    st = e.state()
    st["L"] = e.lmatrix()
    return st


@pytest.mark.parametrize("n_steps", [3200, 6000])
def test_repacking_keeps_every_walker_on_its_own_planes(mhx, orc, monkeypatch, n_steps):
    """11 walkers are dealt over three workgroups when a run begins (ChainState::slot_chain) and,
    under MHX_COMPACT_ALWAYS=1, packed again as they finish; MHX_NO_COMPACT=1 leaves slot s with
    walker s.  n = 6000: the walks end at different loop indices (as tests/test_gpu_lifecycle.py's
    do), so slots are given up while others still walk."""
    p = case(334, C11, PER_CHAIN)
    th0 = p.start(seed=31)
    finals = {}
    for var in ("MHX_COMPACT_ALWAYS", "MHX_NO_COMPACT"):
        monkeypatch.delenv("MHX_COMPACT_ALWAYS", raising=False)
        monkeypatch.delenv("MHX_NO_COMPACT", raising=False)
        monkeypatch.setenv(var, "1")
        e = p.engine(mhx, seed=78)
        finals[var] = _walk_adaptive(e, th0, n=n_steps)
        assert form_of(e) == "resident"
        e.close()
    a, b = finals["MHX_COMPACT_ALWAYS"], finals["MHX_NO_COMPACT"]
    print("n %d: ages %s" % (n_steps, sorted(set(a["age"].tolist()))))
    if n_steps == 6000:
        assert len(set(a["age"].tolist())) >= 2
    for k in ("theta", "logpost", "best_theta", "best_logpost", "age", "length", "L"):
        assert np.array_equal(a[k], b[k]), k
    # ... and it is the oracle's walk (walker 10, the last slot of the partial workgroup)
    ops = p.oracles(orc)
    w = orc.Walker(ops[10], th0[10])
    w.adaptive_begin(n_steps, 10.0, 1, seed=78, chain_id=10)
    w.adaptive_advance(1 << 40)
    assert np.array_equal(a["theta"][10], w.last()[0]) and a["age"][10] == w.age


# ---- 6. independence of the company ------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(334, PER_CHAIN), (1500, PER_POINT)])
def test_a_walker_does_not_depend_on_its_company(mhx, n, kind):
    p = case(n, C11, kind)
    th0 = p.start(seed=41)
    e = p.engine(mhx, seed=79)
    full = _walk_adaptive(e, th0)
    e.close()
    for c in (0, 7, 10):
        one = p.engine(mhx, rows=[c], seed=79, chain_offset=c)
        got = _walk_adaptive(one, th0[c:c + 1])
        one.close()
        for k in ("theta", "logpost", "L", "age"):
            assert np.array_equal(got[k][0], full[k][c]), (c, k)


# ---- 7. against the shared path ----------------------------------------------------------------
@pytest.mark.parametrize("n", [334, 1500])
def test_equal_planes_against_the_shared_path(mhx, orc, n):
    s = pb.two_peak(n=n, seed=6)
    x, y, sig, _ = s.data[0]
    op = s.oracle(orc)
    th = pb.perturbed(s.theta_star, C11, 0.3, seed=8)
    shared = s.engine(mhx, C11)
    want = shared.logpost(th)
    shared.close()
    e = mhx.Engine(C11, s.d, 1)
    e.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    e.set_dataset_planes(0, x, np.tile(y, (C11, 1)), sig, SHARED)
    e.set_bounds(0, *s.bounds[0])
    got = e.logpost(th)
    e.close()
    for i in range(C11):
        assert abs(got[i] - want[i]) <= 2 * tol_for(op, th[i], n_violations(s, th[i])), i


# ---- 8. a global fit: function 0 on planes, function 1 on a shared dataset ---------------------
def test_global_fit_of_planes_and_a_shared_dataset(mhx, orc):
    C = 5
    p = case(334, C, PER_CHAIN, seed=9)
    rng = np.random.default_rng(12)
    d = p.d + 1                                   # the line's slope; its intercept is b0 (shared)
    theta_star = np.append(p.theta_star, 0.4)
    xl = np.sort(rng.uniform(0.0, 2.0, 200))
    sl = rng.uniform(0.05, 0.1, 200)
    yl = theta_star[0] + theta_star[8] * xl + sl * rng.standard_normal(200)
    lo, hi = np.minimum(theta_star * 0.5, theta_star * 1.5), np.maximum(theta_star * 0.5, theta_star * 1.5)
    specs, ops = [], []
    for c in range(C):
        s = pb.Spec(d)
        s.add(pb.GAUSS, (2, 2), range(8), p.x, p.y[c], p.rows[c], pb.NORMAL, (list(range(8)), lo[:8], hi[:8]))
        s.add(pb.POLY, (), [0, 8], xl, yl, sl, pb.NORMAL, ([8], lo[8:], hi[8:]))
        s.theta_star = theta_star
        specs.append(s)
        ops.append(s.oracle(orc))
    e = mhx.Engine(C, d, 2)
    e.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    e.set_dataset_planes(0, p.x, p.y, p.sigma, PER_CHAIN)
    e.set_bounds(0, list(range(8)), lo[:8], hi[:8])
    e.set_function(1, pb.POLY, (), [0, 8])
    e.set_dataset(1, xl, yl, sl)
    e.set_bounds(1, [8], lo[8:], hi[8:])
    th = pb.perturbed(theta_star, C, 0.3, seed=13)
    got = e.logpost(th)
    assert form_of(e) == "streamed"               # (the shared function stages its tiles in LDS)
    for c in range(C):
        assert abs(got[c] - ops[c].logpost(th[c])) <= tol_for(ops[c], th[c], n_violations(specs[c], th[c])), c
    T = np.random.default_rng(5).uniform(1.0, 10.0, size=(25, C))
    run_injected(mhx, orc, e, ops, specs, pb.perturbed(theta_star, C, 0.01, seed=14), theta_star, 25, T=T)
    e.close()


# ---- 9. other kernels through hiprtc -----------------------------------------------------------
LORENTZ_12 = ("(lambda (x &key bg a1 mu1 w1 a2 mu2 w2 &allow-other-keys)"
              " (+ bg (/ a1 (+ 1 (expt (/ (- x mu1) w1) 2))) (/ a2 (+ 1 (expt (/ (- x mu2) w2) 2)))))")
LKEYS = ["bg", "a1", "mu1", "w1", "a2", "mu2", "w2"]


def test_lorentz_peaks_enumerated_recognised_and_as_written(mhx, orc, monkeypatch):
    p = case(334, C11, PER_CHAIN, seed=10, model=pb.LORENTZ, shape=(1, 2))
    ops = p.oracles(orc)
    th = pb.perturbed(p.theta_star, C11, 0.3, seed=15)
    e = p.engine(mhx)
    enum = e.logpost(th)
    assert "PeaksModel<1, 2, true>" in e.kernel_name() and form_of(e) == "resident"
    e.close()
    tols = [tol_for(ops[i], th[i], n_violations(p.specs[i], th[i])) for i in range(C11)]
    for i in range(C11):
        assert abs(enum[i] - ops[i].logpost(th[i])) <= tols[i], i
    keys, expr = mhx.sexpr.lambda_to_expr(LORENTZ_12)
    assert keys == LKEYS

    def as_text():
        t = mhx.Engine(C11, p.d, 1)
        t.set_function_expr(0, expr, keys, list(range(p.d)))
        t.set_dataset_planes(0, p.x, p.y, p.sigma, PER_CHAIN)
        t.set_bounds(0, *p.bounds)
        out = t.logpost(th), t.kernel_name()
        t.close()
        return out
    got, name = as_text()
    assert "PeaksModel<1, 2, true>" in name and "+planes(resident)" in name
    assert np.array_equal(got, enum)               # (recognised: the enumerated model's kernel)
    monkeypatch.setenv("MHX_NO_RECOGNISE", "1")
    got, name = as_text()
    assert "expr:normal+planes(resident)" in name
    for i in range(C11):
        assert abs(got[i] - enum[i]) <= tols[i], i
    # an enumerated model without a compile-time type (MHX_NO_RTC_SPECIALISE=1: the run-time
    # dispatch on the model id) walks the planes too
    monkeypatch.delenv("MHX_NO_RECOGNISE")
    monkeypatch.setenv("MHX_NO_RTC_SPECIALISE", "1")
    e = p.engine(mhx)
    got = e.logpost(th)
    assert "generic:normal+planes(resident)" in e.kernel_name()
    e.close()
    for i in range(C11):
        assert abs(got[i] - ops[i].logpost(th[i])) <= tols[i], i


# ---- 10. the Python surface --------------------------------------------------------------------
def test_walker_set_create_and_its_read_outs(mhx, tmp_path):
    p = case(334, C11, PER_CHAIN)
    keys = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
    starts = p.start(seed=51)
    params = [[v for k, t in zip(keys, starts[c]) for v in (":" + k, float(t))] for c in range(C11)]
    datasets = mhx.data_separated([p.x] + [p.y[c] for c in range(C11)])
    w = mhx.walker_set_create(function=mhx.models.gauss_peaks(keys[:2], [keys[2:5], keys[5:]]),
                              datasets=datasets, params=params, data_error=list(p.sigma),
                              log_prior=mhx.prior_bounds({k: (lo, hi) for k, lo, hi in
                                                          zip(keys, p.bounds[1], p.bounds[2])}), seed=80)
    assert w.n_chains == C11 and "+planes(resident)" in w.engine.kernel_name()
    mhx.walker_adaptive_steps(w, n=3200)
    # the same walk as the engine's own entry points give
    e = p.engine(mhx, seed=80)
    ref = _walk_adaptive(e, starts)
    e.close()
    st = w.engine.state()
    assert np.array_equal(st["theta"], ref["theta"]) and np.array_equal(st["age"], ref["age"])
    med = mhx.walker_set_get(w, ":median-params")
    for c in range(C11):
        assert med[c] == mhx.walker_get(w, ":median-params", chain=c)
    for c in (0, 4, 10):
        fit = mhx.walker_get_data_and_fit(w, chain=c)
        assert np.array_equal(fit[4], p.x) and np.array_equal(fit[5], p.y[c])
        nosd = mhx.walker_get_data_and_fit_no_stddev(w, chain=c)
        assert np.array_equal(nosd[3], p.y[c])
        xs, res, sd = mhx.walker_get_residuals(w, chain=c)
        th = np.array([mhx.walker_get(w, ":median-params", take=1000, chain=c)[k] for k in keys])
        y_fit = w.engine.eval_function(0, th)
        assert np.array_equal(xs, p.x) and np.array_equal(sd, np.full(p.n, p.sigma[c]))
        assert np.array_equal(res, y_fit - p.y[c])      # (walker-plot-residuals: fit minus data)
    allfit = mhx.walker_set_get_data_and_fit(w)
    assert all(np.array_equal(allfit[c][5], p.y[c]) for c in range(C11))
    assert allfit[7][:4] == mhx.walker_get_data_and_fit(w, chain=7)[:4]
    with pytest.raises(mhx.MhxError) as err:
        mhx.walker_save(w, str(tmp_path / "w.lisp"))
    assert err.value.code == mhx.capi.EUNSUPPORTED and "dataset per walker" in str(err.value)
    w.engine.close()


# ---- 11. a group -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [PER_CHAIN, PER_POINT])
def test_group_hands_every_engine_its_rows(mhx, kind):
    p = case(334, C11, kind)
    th0 = p.start(seed=61)
    e = p.engine(mhx, seed=81)
    a = _walk_adaptive(e, th0, chunk=400)
    e.close()
    g = mhx.Group(C11, p.d, 1, devices=[0, 0], seed=81)
    assert g.ranges == [(0, 6), (6, 5)]
    p.define(g)
    g.init_chains(th0)
    g.adaptive_begin(3200, 10.0, 1)
    while g.adaptive_advance(400) > 0:
        pass
    b = g.state()
    for k in ("theta", "logpost", "best_theta", "age", "length"):
        assert np.array_equal(a[k], b[k]), k
    g.close()


# ---- 12. refusals ------------------------------------------------------------------------------
def test_refusals_name_the_combination_and_leave_the_engine_usable(mhx, orc):
    p = case(334, C11, PER_CHAIN)
    lib, capi = mhx.capi.lib(), mhx.capi
    e = mhx.Engine(C11, p.d, 1)
    e.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    e.set_bounds(0, *p.bounds)

    def refused(code, *words, **kw):
        with pytest.raises(mhx.MhxError) as err:
            e.set_dataset_planes(0, kw.get("x", p.x), kw.get("y", p.y), kw.get("sigma", p.sigma),
                                 kw.get("kind", PER_CHAIN), kw.get("lik", capi.LIK_NORMAL))
        assert err.value.code == code, str(err.value)
        for word in words:
            assert word in str(err.value), str(err.value)
    refused(capi.EUNSUPPORTED, "MHX_LIK_NORMAL_CUTOFF", "dataset per walker", lik=capi.LIK_NORMAL_CUTOFF)
    refused(capi.EUNSUPPORTED, "MHX_LIK_POISSON", "dataset per walker", lik=capi.LIK_POISSON)
    refused(capi.EUNSUPPORTED, "MHX_LIK_EXPR", "dataset per walker", lik=capi.LIK_EXPR)
    refused(capi.EINVAL, lik=9)
    bad = p.sigma.copy()
    bad[3] = 0.0
    refused(capi.EINVAL, "sigma[3]", sigma=bad)
    # (what ctypes lets through: n == 0, NULL pointers, a sigma_kind that is none of the four)
    xp, yp, sp = (a.ctypes.data_as(capi.f64p) for a in (p.x, np.ascontiguousarray(p.y), p.sigma))
    for args in ((xp, yp, sp, PER_CHAIN, 0), (None, yp, sp, PER_CHAIN, p.n), (xp, None, sp, PER_CHAIN, p.n),
                 (xp, yp, sp, 4, p.n), (xp, yp, sp, -1, p.n), (xp, yp, None, PER_CHAIN, p.n),
                 (xp, yp, sp, NONE, p.n)):
        assert lib.mhx_set_dataset_planes(e._h, 0, *args, capi.LIK_NORMAL) == capi.EINVAL, args[3:]
    # the engine is usable afterwards: a valid call, and the oracle's numbers
    e.set_dataset_planes(0, p.x, p.y, p.sigma, PER_CHAIN)
    ops = p.oracles(orc)
    th = p.start()
    got = e.logpost(th)
    for i in range(C11):
        assert abs(got[i] - ops[i].logpost(th[i])) <= tol_for(ops[i], th[i])
    # a shared dataset replaces the planes, and planes replace it again
    e.set_dataset(0, p.x, p.y[2], p.rows[2])
    assert "planes" not in (e.logpost(th), e.kernel_name())[1]
    assert abs(e.logpost(th)[5] - ops[2].logpost(th[5])) <= tol_for(ops[2], th[5])
    e.set_dataset_planes(0, p.x, p.y, p.sigma, PER_CHAIN)
    assert np.array_equal(e.logpost(th), got)
    e.close()
    # MHX_ADAPT_POOLED: refused at the call
    e = mhx.Engine(C11, p.d, 1, adapt_mode=capi.ADAPT_POOLED)
    e.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    refused(capi.EUNSUPPORTED, "MHX_ADAPT_POOLED", "dataset per walker")
    e.set_dataset(0, p.x, p.y[0], p.rows[0])
    assert np.isfinite(e.logpost(th)).all()
    e.close()
    # two columns of x elsewhere in the problem: refused when the problem is finalised
    e = mhx.Engine(C11, p.d, 2)
    e.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    e.set_dataset_planes(0, p.x, p.y, p.sigma, PER_CHAIN)
    e.set_function_expr(1, "b0 + b1 * xcol0 * xcol1", ["b0", "b1"], [0, 1])
    e.set_dataset(1, np.stack([p.x, p.x], axis=1), p.y[0], p.rows[0])
    with pytest.raises(mhx.MhxError) as err:
        e.logpost(th)
    assert err.value.code == capi.EUNSUPPORTED and "two columns" in str(err.value)
    e.set_function(1, pb.POLY, (), [0, 1])
    e.set_dataset(1, p.x, p.y[0], p.rows[0])
    assert np.isfinite(e.logpost(th)).all()
    e.close()
