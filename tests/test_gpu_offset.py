"""Peak models at x far from the origin, on the device.  The peak kernels form t = fma(x, iw, c)
with c = fl(-mu iw); c's rounding is a shift of mu by up to |mu| 2^-53 - nothing near the origin,
where every other test of the model kernels lives, and far outside 1e-12 sum |term| at
x ~ mu ~ 2000.  The bound that does hold - 1e-12 sum |term| + the argument term of
tests/offset_cases.py, derived from the kernels' operations - is proven for the
oracle's mirror on the CPU (tests/test_offset_host.py); here the device must EQUAL the mirror at
the same vectors, keep the bound against high precision in the recurrence and in the direct form,
give the same bits in both kernel families and with and without tile skipping, and walk as the
mirror's walker does.  Per value (mhx_eval_function): every peaks model within the bound, while
lorder, the polynomial and the expression kernels, which form their arguments as the reference
does, keep 1e-12 sum |terms| alone at the same offsets.

Worst measured / bound per model on MI355X: DESIGN 4.2."""
import os

import numpy as np
import pytest

import offset_cases as oc
import problems as pb
from test_gpu_fit_bands import ENUMERATED, KEYS8, TWO_PEAK, abs_terms, x_on_and_off

pytestmark = pytest.mark.gpu
REL = oc.REL


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def engine_under(mhx, spec, chains, env, **kw):
    """an engine created and finalised with the given switches set (they are read at
    mhx_set_dataset or when the problem is finalised)"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        e = spec.engine(mhx, chains, **kw)
        e.kernel_name()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return e


def hp_err(got, ref):
    E = oc.hp()
    return np.array([float(abs(E.num(float(g)) - r)) for g, r in zip(got, ref)])


# ---- log-posteriors --------------------------------------------------------------------------------
def check_logposts(mhx, orc, off, span, n, case):
    s, th, ref, scale = case(off, span, n)
    op = s.oracle(orc)
    rec1 = engine_under(mhx, s, 1, {})
    rec19 = engine_under(mhx, s, 19, {})
    direct = engine_under(mhx, s, 1, {"MHX_NO_RECURRENCE": "1"})
    assert "gauss22_normal" in rec1.kernel_name()
    a = rec1.logpost(th)
    rows = np.arange(19 * 2) % len(th)                 # more rows than chains, every vector twice
    a19 = rec19.logpost(th[rows])
    b = direct.logpost(th)
    for e in (rec1, rec19, direct):
        e.close()
    assert np.array_equal(a19, a[rows])
    for form, got in ((True, a), (False, b)):
        orc.mirror_set_recurrence(form)
        try:
            mir = np.array([op.logpost_mirror(t) for t in th])
        finally:
            orc.mirror_set_recurrence(True)
        assert np.array_equal(got, mir), (off, span, n, form, got - mir)
        err = hp_err(got, ref)
        bound = REL * scale + np.array([oc.logpost_bound(s, t, form) for t in th])
        print("(%g, %g) n = %d %s: worst |device - hp| / sum|term| = %.2e, / bound = %.3f"
              % (off, span, n, "recurrence" if form else "direct", (err / scale).max(), (err / bound).max()))
        assert (err <= bound).all(), (off, span, n, form, err / bound)
    return a, b


@pytest.mark.parametrize("n", [300, 2049, 6000])
@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_logposts_equal_the_mirror_and_keep_the_argument_bound(mhx, orc, off, span, n):
    check_logposts(mhx, orc, off, span, n, oc.two_peak_case)


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_wide_peaks_by_the_recurrence(mhx, orc, off, span):
    a, b = check_logposts(mhx, orc, off, span, 6000, oc.two_peak_wide_case)
    assert (a != b).any()                              # the recurrence really ran


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_five_peak_poisson_logposts(mhx, orc, off, span):
    """config 3's kernel: run-time-masked peak loops, the seeds' constants in LDS, the Poisson
    term.  Two of the vectors have peaks wide enough for the recurrence at n = 1500"""
    s, th, ref, scale = oc.five_peak_case(off, span)
    op = s.oracle(orc)
    rec = engine_under(mhx, s, 19, {})
    direct = engine_under(mhx, s, 1, {"MHX_NO_RECURRENCE": "1"})
    assert "gauss15_poisson" in rec.kernel_name()
    a, b = rec.logpost(th), direct.logpost(th)
    rec.close()
    direct.close()
    assert (a[6:] != b[6:]).any()
    for form, got in ((True, a), (False, b)):
        orc.mirror_set_recurrence(form)
        try:
            mir = np.array([op.logpost_mirror(t) for t in th])
        finally:
            orc.mirror_set_recurrence(True)
        assert np.array_equal(got, mir), (off, span, form, got - mir)
        err = hp_err(got, ref)
        bound = REL * scale + np.array([oc.logpost_bound(s, t, form) for t in th])
        print("(%g, %g) five peaks %s: worst |device - hp| / sum|term| = %.2e, / bound = %.3f"
              % (off, span, "recurrence" if form else "direct", (err / scale).max(), (err / bound).max()))
        assert (err <= bound).all(), (off, span, form, err / bound)


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_pseudo_voigt_global_fit_logposts(mhx, off, span):
    """config 4's kernel has no mirror: its fast path (one shared reciprocal, table exps whose
    argument rounds iw g and c g separately) against high precision, with that form's own delta"""
    s, th, ref, scale = oc.pvoigt_case(off, span)
    e = engine_under(mhx, s, 19, {})
    assert "pvoigt2" in e.kernel_name()
    got = e.logpost(th)
    e.close()
    err = hp_err(got, ref)
    bound = REL * scale + np.array([oc.logpost_bound(s, t, False) for t in th])
    print("(%g, %g) pvoigt2 global fit: worst |device - hp| / sum|term| = %.2e, / bound = %.3f"
          % (off, span, (err / scale).max(), (err / bound).max()))
    assert (err <= bound).all(), (off, span, err / bound)
    assert bool((err > REL * scale).any()) == ((off, span) != (0.0, 1.0))


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_both_families_give_the_same_bits(mhx, off, span):
    s, th, _, _ = oc.two_peak_case(off, span, 6000)
    thw = oc.two_peak_wide_case(off, span, 6000)[1]
    got = []
    for wpg in ("8", "16"):
        e = engine_under(mhx, s, 1, {"MHX_FAMILY_WPG": wpg})
        assert e.kernel_name().startswith("w%s/" % wpg)
        got.append(e.logpost(np.concatenate([th, thw])))
        e.close()
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_tile_skipping_is_exact_at_an_offset(mhx, orc, off, span):
    """tile_mask forms fma(xlo, iw, c) with the SAME c as the sweep: what it leaves out is a no-op
    away from the origin too.  Narrow peaks (0.002 of the span), so that most windows leave one out"""
    s = oc.two_peak_at(off, span, 5000, seed=44)
    th = oc.perturbed(s, n=40, seed=8, d_mu=0.2)
    th[:, 4] = 0.002 * span * (1.0 + 0.3 * np.cos(np.arange(40)))
    th[:, 7] = 0.002 * span * (1.0 + 0.3 * np.sin(np.arange(40)))
    th[::7, 2] *= -1.0                                 # some negative amplitudes
    on = engine_under(mhx, s, 1, {"MHX_NO_TILE_SKIP": "0"})
    no = engine_under(mhx, s, 1, {"MHX_NO_TILE_SKIP": "1"})
    ga, pa = on.logpost(th, parts=True)
    gb, pb_ = no.logpost(th, parts=True)
    on.close()
    no.close()
    assert np.isfinite(ga).all()
    assert np.array_equal(ga, gb) and np.array_equal(pa, pb_)
    op = s.oracle(orc)
    assert np.array_equal(ga[::4], [op.logpost_mirror(t) for t in th[::4]])


def test_a_walk_at_an_offset_equals_the_mirrors(mhx, orc):
    """proposals cross the fast / guarded and the seeding-class borders at other places than at
    the origin; theta, logpost and age of every chain against orc.Walker(mirror=True)"""
    s = oc.two_peak_at(2000.0, 1.0, 6000, seed=31)
    op = s.oracle(orc)
    C_, iters = 3, 300
    th0 = oc.perturbed(s, n=C_, seed=5, d_mu=0.01, d_rel=0.02)
    th0[1, [4, 7]] = [0.5, 0.6]                        # one chain starts where the recurrence runs
    e = s.engine(mhx, C_, seed=17)
    e.init_chains(th0)
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(iters)
    st = e.state()
    e.close()
    for c in range(C_):
        w = orc.Walker(op, th0[c], mirror=True)
        w.adaptive_begin(30000, 10.0, 1, seed=17, chain_id=c)
        w.adaptive_advance(iters)
        th, pr = w.last()
        assert st["age"][c] == w.age, c
        assert np.array_equal(st["theta"][c], th) and st["logpost"][c] == pr, c


# ---- per value: mhx_eval_function ------------------------------------------------------------------
OFFSETS = oc.CASES[1:]
WORST = {}


def placed_single(model, shape, p, off, span, seed=0):
    """an ENUMERATED model of test_gpu_fit_bands (built on x in [-1, 2]) placed at the offset"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 2.0, 777)
    s = pb.Spec(len(p))
    s.add(model, shape, range(len(p)), x, np.zeros_like(x), rng.uniform(0.1, 0.2, x.size), pb.NORMAL)
    s.theta_star = np.asarray(p, float)
    return oc.place(s, off, span)


def check_values(mhx, s, name, bound_of, n_vec=4, theta=None, must_need_the_term=None):
    """eval_function of every function of s at its dataset's x and off it, against high precision;
    bound_of(model, shape, p, xs) -> the per-value bound beyond REL * sum |terms| (None: REL alone)"""
    e = s.engine(mhx, 1)
    th = oc.perturbed(s, n=n_vec, seed=21) if theta is None else theta
    worst, beyond_rel = 0.0, 0.0
    for k, (model, shape, idx) in enumerate(s.fns):
        xs = x_on_and_off(s.data[k][0], seed=k)
        got = e.eval_function(k, th, xs)
        for i in range(len(th)):
            p = th[i][idx]
            err = hp_err(got[i], oc.hp_values(model, shape, p, xs))
            terms = abs_terms(model, shape, p, xs)
            extra = 0.0 if bound_of is None else bound_of(model, shape, p, xs)
            worst = max(worst, float((err / (REL * terms + extra)).max()))
            beyond_rel = max(beyond_rel, float((err / terms).max()))
    kname = e.kernel_name()
    e.close()
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print("eval_function %s: worst |device - hp| / bound = %.3f, / sum|terms| = %.2e"
          % (name, worst, beyond_rel))
    assert worst <= 1.0, (name, worst)
    if must_need_the_term is not None:
        assert (beyond_rel > REL) == must_need_the_term, (name, beyond_rel)
    return kname


PEAK_SPECS = [c for c in ENUMERATED if c[0] in ("gauss03", "gauss31", "lorentz12", "pvoigt2")]


@pytest.mark.parametrize("off, span", OFFSETS, ids=oc.CASE_IDS[1:])
def test_values_of_the_peak_models(mhx, off, span):
    for name, model, shape, p in PEAK_SPECS:
        check_values(mhx, placed_single(model, shape, p, off, span), "%s at (%g, %g)" % (name, off, span),
                     oc.argument_term)
    k = check_values(mhx, oc.place(pb.poisson_peaks(n=1500), off, span),
                     "config3 five peaks at (%g, %g)" % (off, span), oc.argument_term)
    assert "gauss15_poisson" in k


def test_the_tails_of_gauss03_need_the_argument_term(mhx):
    """no background: sum |terms| is the peaks themselves, and on a flank |dg/dx| delta is
    2 |u| |mu| / |w| 2^-53 of the value: the inputs are the hard ones"""
    name, model, shape, p = [c for c in ENUMERATED if c[0] == "gauss03"][0]
    check_values(mhx, placed_single(model, shape, p, 2000.0, 1.0), "gauss03 tails", oc.argument_term,
                 must_need_the_term=True)
    check_values(mhx, placed_single(model, shape, p, 0.0, 1.0), "gauss03 at the origin", oc.argument_term,
                 must_need_the_term=False)


@pytest.mark.parametrize("off, span", [(2000.0, 1.0), (1e5, 1.0)], ids=["off2000", "off1e5"])
def test_values_on_the_generic_kernels(mhx, monkeypatch, off, span):
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    for name, model, shape, p in PEAK_SPECS:
        k = check_values(mhx, placed_single(model, shape, p, off, span),
                         "%s (generic) at (%g, %g)" % (name, off, span), oc.argument_term)
        assert "generic" in k
    k = check_values(mhx, oc.place(pb.poisson_peaks(n=1500), off, span),
                     "config3 five peaks (generic) at (%g, %g)" % (off, span), oc.argument_term)
    assert "generic" in k


@pytest.mark.parametrize("off, span", [(2000.0, 1.0), (1023.5, 1.0)], ids=["off2000", "off1023.5"])
def test_values_of_a_run_time_specialised_shape(mhx, off, span):
    """three Gaussians on a linear background: PeaksModel<2, 3> through hiprtc, the shape
    test_gpu_fuzz.py's test_run_time_specialised_peaks_fuzz uses"""
    npk, n = 3, 1500
    rng = np.random.default_rng(npk)
    x = np.linspace(0.0, 1.0, n)
    sig = rng.uniform(0.05, 0.15, n)
    th = [0.5, 0.3]
    for k in range(npk):
        th += [rng.uniform(0.6, 1.2), (k + 0.6) / (npk + 0.2), rng.uniform(0.03, 0.07)]
    th = np.array(th)
    s = pb.Spec(len(th))
    s.add(pb.GAUSS, (2, npk), range(len(th)), x, pb.model_eval_np(pb.GAUSS, (2, npk), th, x), sig, pb.NORMAL)
    s.theta_star = th
    k = check_values(mhx, oc.place(s, off, span), "rtc gauss23 at (%g, %g)" % (off, span), oc.argument_term)
    assert "rtc[PeaksModel<2, 3, false>" in k, k


# ---- the controls: arguments formed as the reference forms them --------------------------------------
def test_lorder_keeps_rel_alone(mhx):
    s = pb.lorder()                                    # x = 2000 ... 2997 as it is
    th = pb.perturbed(s.theta_star, 4, 0.001, seed=21)
    assert "lorder" in check_values(mhx, s, "lorder (control)", None, theta=th)


@pytest.mark.parametrize("off, span", OFFSETS, ids=oc.CASE_IDS[1:])
def test_poly5_and_the_expression_kernel_keep_rel_alone(mhx, off, span):
    x = off + span * np.linspace(0.0, 1.0, 777)
    s = pb.Spec(5)
    s.add(pb.POLY, (), range(5), x, np.zeros_like(x), np.full(777, 0.1), pb.NORMAL)
    s.theta_star = np.array([0.3, -1.0, 0.5, 0.2, -0.1])
    th = pb.perturbed(s.theta_star, 4, 0.01, seed=21)
    check_values(mhx, s, "poly5 (control) at (%g, %g)" % (off, span), None, theta=th)
    # the two-peak lambda, as written: (/ (- x mu) w), the reference's own form
    s2 = oc.two_peak_at(off, span, 1200, seed=8)
    x2, y2, sig2, _ = s2.data[0]
    params = []
    for k, v in zip(KEYS8, s2.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(function=mhx.models.lisp(TWO_PEAK, as_written=True), data=[x2, y2],
                          params=params, data_error=sig2)
    assert "rtc[expr" in w.engine.kernel_name()
    xs = x_on_and_off(x2, seed=2)
    th2 = oc.perturbed(s2, n=3, seed=4)
    got = w.engine.eval_function(0, th2, xs)
    worst = 0.0
    for i in range(len(th2)):
        err = hp_err(got[i], oc.hp_values(pb.GAUSS, (2, 2), th2[i], xs))
        worst = max(worst, float((err / abs_terms(pb.GAUSS, (2, 2), th2[i], xs)).max()))
    print("expression two-peak (control) at (%g, %g): worst / sum|terms| = %.2e" % (off, span, worst))
    assert worst <= REL, (off, span, worst)


# ---- the two other models whose argument is formed differently from the reference's ---------------------
def test_sinusoid_and_expdecay_at_2000(mhx):
    x = 2000.0 + np.linspace(0.0, 3.0, 777)

    def one(model, p):
        s = pb.Spec(len(p))
        s.add(model, (), range(len(p)), x, np.zeros_like(x), np.full(777, 0.1), pb.NORMAL)
        s.theta_star = np.asarray(p, float)
        return s

    sin_p = np.array([1.5, 3.0, 0.4, -0.2])
    check_values(mhx, one(pb.SINUS, sin_p), "sinusoid at 2000",
                 lambda m, sh, p, xs: oc.sinusoid_term(p, xs), theta=pb.perturbed(sin_p, 4, 0.01, seed=21))
    # x / tau <= 700: the exponential stays a normal number; c = 0 asks for RELATIVE accuracy
    for p in ([2.0, 3.0, 0.0], [2.0, 2003.0 / 699.0, 0.0], [2.0, 700.0, 0.1]):
        assert (x / p[1]).max() <= 700.0
        th = np.array(p)[None, :] * np.array([[1.0, 1.0, 1.0], [0.9, 1.01, 1.0], [-1.1, 1.02, 1.0]])
        check_values(mhx, one(pb.EXPDECAY, p), "expdecay tau %.3g at 2000" % p[1],
                     lambda m, sh, q, xs: oc.expdecay_term(q, xs), theta=th)


def test_print_worst_ratios():
    for name in sorted(WORST):
        print("worst measured / bound  %-44s %.3f" % (name, WORST[name]))
