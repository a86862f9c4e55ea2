"""Derived quantities (walker-with-exp, mcmc-fitting.lisp:1052-1064, and the posterior of its
expression): mhx_get_derived / mhx_group_get_derived against the host route on injected and on
walked histories.  Every chain of every engine is checked.  Arithmetic bodies, percentiles, mean
and standard deviation are compared BIT FOR BIT (IEEE operations in a fixed order on both sides);
exp / log bodies with test_gpu_expr_math.same against the probe that runs the same routines, and
the single calls exp(a), log(a) within 1 ulp of mpmath (the bound include/mhx.h states)."""
import math
import time

import numpy as np
import pytest

import exprprobe
import problems as pb
import sexpr_eval
import test_gpu_expr_math as em
from test_gpu_walker_set_get import PCTS, crafted_walk, inject, line_engine

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 9, 64, 65, 1023, 1024, 2047, 2048]
TAKES = (1, 2, 10, 1000, 2048)
ARITH = ["(+ (* :a :b) (/ :a (- :b 3.5)))", "(sqrt (abs :a))", "(max :a (min :b 0.5) -1.0)",
         "(floor :a)", "(expt :b 3)", "(if (< :a :b) (* 2 :a) (- :b))", "(* :a :b (sqrt pi))",
         "(/ :a :b)", "(+ prob (abs :b))"]


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """the same doubles bit for bit, any NaN standing for any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def same_pct(a, b):
    """percentiles: the same doubles bit for bit, but for a zero's sign - order_key holds -0 and +0
    interchangeable, so which of the two an order statistic lands on is not defined"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)) |
                                              ((a == 0.0) & (b == 0.0))))


def translate(mhx, forms):
    """Lisp keyword forms -> (parsed forms, names, C texts) over one list of names"""
    names, texts, parsed = [], [], []
    for f in forms:
        nm, text = mhx.sexpr.keyword_exp_to_expr(f)
        names += [k for k in nm if k not in names]
        texts.append(text)
        parsed.append(mhx.sexpr.parse(f))
    return parsed, names, texts


def ieee_env(keys, theta, prob=None):
    """the environment of sexpr_eval.evaluate as numpy doubles: the same binary64 operations, but
    a division by zero gives the IEEE inf / NaN (the device's answer, status 1) where a Python
    float - like SBCL - would trap.  Evaluate under np.errstate(all="ignore")."""
    env = {":" + k: np.float64(theta[j]) for j, k in enumerate(keys)}
    if prob is not None:
        env["prob"] = np.float64(prob)
    return env


def host_at(parsed, keys, theta, prob=None):
    env = ieee_env(keys, theta, prob)
    with np.errstate(all="ignore"):
        return [float(sexpr_eval.evaluate(f, env)) for f in parsed]


def host_values(parsed, keys, pr, th):
    """[n_expr][n] what SBCL would compute at every step (tests/sexpr_eval)"""
    out = np.empty((len(parsed), len(pr)))
    for s in range(len(pr)):
        out[:, s] = host_at(parsed, keys, th[s], pr[s])
    return out


def mean_stddev(v):
    """M:1518-1527 in Python floats: serial sums newest first"""
    v = [float(x) for x in v]
    s = v[0]
    for x in v[1:]:
        s = s + x
    m = s / len(v)
    q = (v[0] - m) * (v[0] - m)
    for x in v[1:]:
        q = q + (x - m) * (x - m)
    return m, (math.sqrt(q / (len(v) - 1)) if len(v) > 1 else math.nan)


def check_against_host(mhx, e, walks, keys, forms, takes):
    from lisp_mcmc_amd import walker as mirror
    parsed, names, texts = translate(mhx, forms)
    index = [keys.index(k) for k in names]
    full = [host_values(parsed, keys, pr, th) for pr, th in walks]
    best = e.state()
    for take in takes:
        r = e.derived(texts, names, index, take, PCTS, values=True)
        for c, (pr, th) in enumerate(walks):
            t = min(take, len(pr))
            assert r["n_used"][c] == t, (take, c)
            want = full[c][:, :t]
            assert same_bits(r["values"][c, :, :t], want), (take, c)
            assert np.isnan(r["values"][c, :, t:]).all(), (take, c)   # not written
            for q in range(len(forms)):
                wp = [mirror._percentile(p, want[q]) for p in PCTS]
                assert same_pct(r["pct"][c, :, q], wp), (take, c, q)
                m, sd = mean_stddev(want[q])
                assert same_bits(r["mean"][c, q], m), (take, c, q)
                assert same_bits(r["stddev"][c, q], sd), (take, c, q)
                assert r["status"][c, q] == (0 if np.isfinite(want[q]).all() else 1), (take, c, q)
            wb = host_at(parsed, keys, best["best_theta"][c], best["best_logpost"][c])
            assert same_bits(r["at_most_likely"][c], wb), (take, c)


def test_arithmetic_bodies_and_summaries_d2(mhx):
    rng = np.random.default_rng(101)
    e = line_engine(mhx, 66, history_capacity=2048)
    e.init_chains([-1.0, 2.0])
    walks = inject(e, rng, LENGTHS * 6 + list(rng.integers(1, 2049, 6)))
    check_against_host(mhx, e, walks, ["a", "b"], ARITH, TAKES)
    e.close()


def test_arithmetic_bodies_wide_d_names_out_of_order(mhx):
    rng = np.random.default_rng(102)
    e = line_engine(mhx, 24, d=33, used=range(0, 32, 4), history_capacity=2048)
    e.init_chains(np.linspace(-1.0, 2.0, 33))
    walks = inject(e, rng, LENGTHS * 2 + list(rng.integers(1, 2049, 4)))
    keys = ["p%d" % j for j in range(33)]
    forms = ["(/ (* :p30 :p7) (+ 1.5 (abs :p2)))", "(- :p32 :p0)", "(max :p7 :p30)",
             "(* :p2 (sqrt pi) prob)"]
    check_against_host(mhx, e, walks, keys, forms, TAKES)
    e.close()


def test_identities(mhx):
    rng = np.random.default_rng(103)
    e = line_engine(mhx, 30, history_capacity=2048)
    e.init_chains([-1.0, 2.0])
    walks = inject(e, rng, LENGTHS * 3)
    st = e.state()
    for take in TAKES:
        r = e.derived(["a", "b", "prob"], ["a", "b"], [0, 1], take, PCTS, values=True)
        pct, used = e.percentiles(take, PCTS)
        assert np.array_equal(r["n_used"], used)
        assert same_bits(r["pct"][:, :, 0], pct[:, :, 0]) and same_bits(r["pct"][:, :, 1], pct[:, :, 1])
        for c in range(e.n_chains):
            pr, th = e.trace(c, take)
            assert same_bits(r["values"][c, 2, :len(pr)], pr), (take, c)
            assert same_bits(r["values"][c, 0, :len(pr)], th[:, 0]), (take, c)
        assert same_bits(r["at_most_likely"][:, 0], st["best_theta"][:, 0])
        assert same_bits(r["at_most_likely"][:, 2], st["best_logpost"])
    e.close()


def uniform_history(e, rng, lengths, lo, hi):
    walks = []
    for c, n in enumerate(lengths):
        pr, th = rng.normal(-50.0, 3.0, n), rng.uniform(lo, hi, (n, e.d))
        e.set_history(c, pr, th)
        walks.append((pr, th))
    return walks


def test_exp_log_bodies_against_the_probe_and_mpmath(mhx):
    import mpmath as mp
    mp.mp.prec = 200
    rng = np.random.default_rng(104)
    e = line_engine(mhx, 12, history_capacity=2048)
    e.init_chains([-1.0, 2.0])
    walks = uniform_history(e, rng, [1, 2, 65, 1023, 2048, 300] * 2, -6.0, 6.0)
    bodies = ["exp(a) * b", "log(abs(a) + 0.5) / b", "exp(-ipow((a - b) / 2.5, 2))",
              "exp(a)", "log(a)"]
    r = e.derived(bodies, ["a", "b"], [0, 1], 2048, [50], values=True)
    rows = np.concatenate([th for _, th in walks])
    got = np.concatenate([r["values"][c, :, :len(pr)] for c, (pr, _) in enumerate(walks)], axis=1)
    with pytest.MonkeyPatch.context() as mpatch:
        for k in ("MHX_EXPR_OCML_MATH", "MHX_FAMILY_WPG"):
            mpatch.delenv(k, raising=False)
        mpatch.setenv("MHX_EXPR_EXACT_DIV", "1")
        mpatch.setenv("MHX_SPLIT", "0")
        for q, body in enumerate(bodies):
            want = exprprobe.evaluate(mhx, body, ["a", "b"], rows)
            bad = np.flatnonzero(~em.same(got[q], want))
            assert bad.size == 0, (body, bad[:5], got[q][bad[:5]], want[bad[:5]])
    a = rows[:, 0]
    ref = np.array([em.LD(mp.nstr(mp.exp(mp.mpf(float(v))), 30)) for v in a], dtype=em.LD)
    worst = em.ulps(got[3], ref).max()
    print("exp(a): worst %.4f ulp over %d values" % (worst, a.size))
    assert worst < 1.0
    pos = a > 0
    assert np.isnan(got[4][~pos]).all()
    ref = np.array([em.LD(mp.nstr(mp.log(mp.mpf(float(v))), 30)) for v in a[pos]], dtype=em.LD)
    worst = em.ulps(got[4][pos], ref).max()
    print("log(a): worst %.4f ulp over %d values" % (worst, int(pos.sum())))
    assert worst < 1.0
    e.close()


def test_values_that_are_not_finite(mhx):
    rng = np.random.default_rng(105)
    e = line_engine(mhx, 4, history_capacity=1024)
    e.init_chains([1.0, 2.0])
    walks = uniform_history(e, rng, [200, 200, 200, 200], 0.5, 6.0)
    pr, th = walks[1]
    th[7, 0] = -3.0            # log(a) of a negative step
    e.set_history(1, pr, th)
    pr, th = walks[2]
    th[0, 0] = 0.0             # 1 / a at a = 0 (where the engine's log is NaN: not finite either)
    e.set_history(2, pr, th)
    r = e.derived(["log(a)", "1 / a", "a + b"], ["a", "b"], [0, 1], 200, [0, 50, 100], values=True)
    assert r["status"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0]]
    assert np.isnan(r["values"][2, 0, 0]) and np.isfinite(r["values"][2, 0, 1:]).all()
    assert np.isnan(r["values"][1, 0, 7]) and np.isfinite(np.delete(r["values"][1, 0], 7)).all()
    assert np.isnan(r["pct"][1, 2, 0]) and np.isfinite(r["pct"][1, :2, 0]).all()   # the NaN sorts last
    assert np.isnan(r["mean"][1, 0])
    assert r["values"][2, 1, 0] == np.inf and r["pct"][2, 2, 1] == np.inf
    assert np.isfinite(r["pct"][2, :2, 1]).all()
    e.close()


def test_portions(mhx):
    """4096 chains x 16 expressions at capacity 1024: 128 KiB of values per chain, eight portions"""
    rng = np.random.default_rng(106)
    n = 4096
    e = line_engine(mhx, n, history_capacity=1024)
    e.init_chains([-1.0, 2.0])
    lengths = rng.integers(1, 1025, n)
    lengths[:4] = [1, 2, 1023, 1024]
    for c in range(n):
        e.set_history(c, rng.normal(-50.0, 3.0, lengths[c]), rng.normal(0.0, 2.0, (lengths[c], 2)))
    bodies = ["a + %d * b" % k for k in range(8)] + ["a * b - %d" % k for k in range(8)]
    r = e.derived(bodies, ["a", "b"], [0, 1], 1024, PCTS)
    assert np.array_equal(r["n_used"], lengths)
    for q, body in enumerate(bodies):
        one = e.derived([body], ["a", "b"], [0, 1], 1024, PCTS)
        assert same_bits(r["pct"][:, :, q], one["pct"][:, :, 0]), q
        assert same_bits(r["mean"][:, q], one["mean"][:, 0]), q
        assert same_bits(r["stddev"][:, q], one["stddev"][:, 0]), q
        assert same_bits(r["at_most_likely"][:, q], one["at_most_likely"][:, 0]), q
    e.close()


def test_a_real_walk_through_a_wrapped_ring(mhx):
    """256 chains of the two-peak problem, ring 1024, 3000 iterations: peak area and amplitude
    ratio of every chain against the host route from get_trace"""
    from lisp_mcmc_amd import walker as mirror
    s = pb.two_peak(n=1500, seed=21)
    n = 256
    e = s.engine(mhx, n, seed=5)
    e.init_chains(pb.perturbed(s.theta_star, n, 0.01, seed=8))
    e.adaptive_begin(3000, 10.0, 1)
    e.adaptive_advance(1 << 30)
    keys = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
    forms = ["(* :a1 :w1 (sqrt pi))", "(/ :a2 :a1)"]
    parsed, names, texts = translate(mhx, forms)
    index = [keys.index(k) for k in names]
    st = e.state()
    assert (st["length"] > 1024).any()          # the ring has wrapped
    for take in (1000, 1024):
        r = e.derived(texts, names, index, take, PCTS, values=True)
        for c in range(n):
            pr, th = e.trace(c, take)
            assert r["n_used"][c] == len(pr)
            want = host_values(parsed, keys, pr, th)
            assert same_bits(r["values"][c, :, :len(pr)], want), (take, c)
            for q in range(2):
                assert same_pct(r["pct"][c, :, q], [mirror._percentile(p, want[q]) for p in PCTS])
                m, sd = mean_stddev(want[q])
                assert same_bits(r["mean"][c, q], m) and same_bits(r["stddev"][c, q], sd), (take, c)
            assert same_bits(r["at_most_likely"][c], host_at(parsed, keys, st["best_theta"][c]))
    e.close()


def test_the_walker_functions(mhx):
    """walker_with_exp / walker_exp_get and their set forms on a small walker set"""
    from lisp_mcmc_amd import walker as mirror
    rng = np.random.default_rng(107)
    e = line_engine(mhx, 5, history_capacity=1024)
    e.init_chains([-1.0, 2.0])
    walks = inject(e, rng, [1, 9, 300, 1024, 700])

    class W:
        engine, param_keys, n_chains = e, ["m", "b"], 5
    exp = "(* :m :b (sqrt pi))"
    parsed = mhx.sexpr.parse(exp)
    st = e.state()
    whole = mirror.walker_set_with_exp(W, exp)
    for c in range(5):
        env = {":m": float(st["best_theta"][c, 0]), ":b": float(st["best_theta"][c, 1])}
        assert mirror.walker_with_exp(W, exp, chain=c) == whole[c] == sexpr_eval.evaluate(parsed, env)
    for get in (":median", ":95cr", ":iqr", ":mean", ":stddev", ":stddev-normal", ":values",
                (":percentile", 84.1), ":most-likely"):
        allc = mirror.walker_set_exp_get(W, exp, get, take=500)
        for c, (pr, th) in enumerate(walks):
            one = mirror.walker_exp_get(W, exp, get, take=500, chain=c)
            assert same_bits(np.asarray(one), np.asarray(allc[c])), (get, c)
            v = host_values([parsed], ["m", "b"], pr[:500], th[:500])[0]
            if get == ":median":
                assert one == mirror._percentile(50, v)
            if get == ":95cr":
                assert one == [mirror._percentile(2.5, v), mirror._percentile(97.5, v)]
            if get == ":stddev-normal":
                assert one == mirror._percentile(84.1, v) - mirror._percentile(50, v)
            if get == ":values":
                assert same_bits(one, v)
    with pytest.raises(KeyError):
        mirror.walker_with_exp(W, "(* :m :nope)")
    with pytest.raises(mhx.sexpr.SexprError):
        mirror.walker_with_exp(W, "(gamma :m)")
    e.close()


def test_group_equals_its_engines(mhx):
    s = pb.two_peak(n=1500, seed=4)
    n = 49
    th0 = pb.perturbed(s.theta_star, n, 0.01, seed=6)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0], seed=10)
    s.apply(g)
    g.init_chains(th0)
    g.adaptive_begin(30000, 10.0, 1)
    g.adaptive_advance(1500)
    assert g.ranges == [(0, 25), (25, 24)]
    bodies, names, index = ["a1 * w1 * sqrt(3.14159265358979323846)", "a2 / a1", "exp(prob / 1e4)"], \
        ["a1", "w1", "a2"], [2, 4, 5]
    for take in (1, 200, 1024):
        whole = g.derived(bodies, names, index, take, PCTS, values=True)
        parts = [x.derived(bodies, names, index, take, PCTS, values=True) for x in g.engines]
        for k in whole:
            assert same_bits(whole[k].astype(np.float64),
                             np.concatenate([p[k] for p in parts]).astype(np.float64)), (take, k)
    g.close()


def test_edges_through_the_abi(mhx, tmp_path, monkeypatch):
    import ctypes as C
    import os
    capi, lib = mhx.capi, mhx.capi.lib()
    monkeypatch.setenv("MHX_RTC_CACHE_DIR", str(tmp_path))
    e = line_engine(mhx, 3)

    def call(h, exprs, take, fn=lib.mhx_get_derived, out=None, n_expr=None):
        ex = (C.c_char_p * max(len(exprs), 1))(*[t.encode() for t in exprs])
        nm = (C.c_char_p * 2)(b"a", b"b")
        _, ip = capi.as_i32([0, 1])
        _, nump = capi.as_i32([50])
        _, denp = capi.as_i32([1])
        o = out.ctypes.data_as(capi.f64p) if out is not None else None
        return fn(h, ex, len(exprs) if n_expr is None else n_expr, nm, ip, 2, take, nump, denp, 1,
                  o, None, None, None, None, None, None)

    assert call(e._h, ["a"], 10) == capi.ESTATE
    e.init_chains([-1.0, 2.0])
    cap = e.history_capacity()
    assert call(e._h, ["a"], 10, n_expr=0) == capi.EINVAL
    assert call(e._h, ["a"] * 17, 10) == capi.EINVAL
    assert call(e._h, ["a"], 0) == capi.EINVAL
    assert call(e._h, ["a"], cap + 1) == capi.EINVAL
    assert call(None, ["a"], 10) == capi.EINVAL
    for ident, text in (("nosuch", "a + nosuch"), ("x", "a * x"), ("bounds_total", "bounds_total + b"),
                        ("xcol1", "xcol1")):
        assert call(e._h, ["b", text], 10) == capi.EINVAL
        msg = lib.mhx_last_error().decode()
        assert "'%s'" % ident in msg and "hiprtc" not in msg, msg
    # the same texts a second time compile nothing: one file in the on-disk cache, and the call
    # that found the module in the process costs a fraction of the one that compiled it
    salt = "%d.0" % int(time.time() * 1e3 % 1e9)
    texts = ["a * b + " + salt, "a - " + salt]
    t0 = time.perf_counter()
    assert call(e._h, texts, 10) == 0            # all outputs NULL
    cold = time.perf_counter() - t0
    files = sorted(os.listdir(str(tmp_path)))
    assert len(files) == 1
    out = np.zeros((3, 2))
    t0 = time.perf_counter()
    assert call(e._h, texts, 10, out=out) == 0
    warm = time.perf_counter() - t0
    assert sorted(os.listdir(str(tmp_path))) == files
    print("derived module: first call %.3f s, second %.5f s" % (cold, warm))
    assert warm < 0.25 * cold
    assert np.array_equal(out, [[-2.0 + float(salt), -1.0 - float(salt)]] * 3)
    e2 = line_engine(mhx, 2)                      # another engine, the same texts: the same module
    e2.init_chains([-1.0, 2.0])
    assert call(e2._h, texts, 1) == 0
    assert sorted(os.listdir(str(tmp_path))) == files
    e2.close()
    g = mhx.Group(4, 2, 1, devices=[0, 0])
    assert call(g._h, ["a"], 10, fn=lib.mhx_group_get_derived) == capi.ESTATE
    assert call(None, ["a"], 10, fn=lib.mhx_group_get_derived) == capi.EINVAL
    g.close()
    e.close()
