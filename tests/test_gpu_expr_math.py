"""Per-value accuracy of the run-time compiled expression kernels (csrc/mhx_rtc.cpp) against high
precision: each routine an expression calls - gexp, tlog / mlog, the hoisted reciprocals of `/`,
mhx_ux_ipow and ocml's functions - as compiled for gfx950, one value at a time
(tests/exprprobe.py reads f(row) out of mhx_logpost bit for bit).  References: numpy longdouble
(80-bit) for bulk arguments, mpmath at the edges.  Errors are in ulps of the reference's exponent,
2^(ilogb(ref) - 52), and 2^-1074 for subnormal results.

The exp and the log outside 1/16 of 1 are also tied bit for bit to the oracle's restatements
(orc_mirror_gexp, orc_mirror_tlog), which tests/test_device_math_cpu.py measures on millions of
points."""
import math

import numpy as np
import pytest

import exprprobe

pytestmark = pytest.mark.gpu

LD = np.longdouble
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = 2.0 ** -1022
TINY = 2.0 ** -1074
NAMES = ["s", "a", "b"]
# the default program: row r computes ROUTINES[s] (s = its selector column)
ROUTINES = [("exp", "exp(a + x)"), ("log", "log(a + x)"), ("div", "(a + x) / b"),
            ("ipow", "ipow(a + x, b)"), ("sqrt", "sqrt(a + x)"), ("abs", "abs(a + x)"),
            ("floor", "floor(a + x)"), ("min", "min(a + x, b)"), ("max", "max(a + x, b)"),
            ("sin", "sin(a + x)"), ("cos", "cos(a + x)"), ("tan", "tan(a + x)"),
            ("atan", "atan(a + x)"), ("tanh", "tanh(a + x)"), ("pow", "pow(a + x, b)")]
SEL = {name: i for i, (name, _) in enumerate(ROUTINES)}
EVERYTHING = exprprobe.select_chain([body for _, body in ROUTINES])
EXPLOG = exprprobe.select_chain([ROUTINES[0][1], ROUTINES[1][1]])
LOG_WINDOW = (0.9375, 1.0625)   # tlog sends [0.9375, 1.0625) through mlog


def ulps(got, ref):
    """|got - ref| / 2^(ilogb(ref) - 52), the unit 2^-1074 for subnormal (or zero) ref"""
    ref = np.asarray(ref, dtype=LD)
    _, e = np.frexp(np.abs(ref))                  # |ref| = m 2^e, m in [0.5, 1): ilogb = e - 1
    unit = np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))
    return (np.abs(np.asarray(got, dtype=LD) - ref) / unit).astype(np.float64)


def same(a, b):
    """equal values, NaN matching NaN (a zero's sign does not survive the probe)"""
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def rows_for(sel, a, b=0.0):
    a = np.asarray(a, dtype=np.float64).ravel()
    r = np.empty((a.size, 3))
    r[:, 0], r[:, 1], r[:, 2] = float(sel), a, b
    return r


def random_doubles(rng, n, e_lo, e_hi, sign=1):
    """n doubles 2^e (1 + f), e uniform in [e_lo, e_hi], f uniform in its 52 bits"""
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    expo = rng.integers(e_lo + 1023, e_hi + 1024, n).astype(np.uint64)
    v = ((expo << np.uint64(52)) | mant).view(np.float64)
    return v if sign > 0 else (-v if sign < 0 else v * rng.choice([-1.0, 1.0], n))


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def run(mhx, body, rows, **env):
    """evaluate under exactly the given switches (the others unset)"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ("MHX_EXPR_EXACT_DIV", "MHX_EXPR_OCML_MATH", "MHX_FAMILY_WPG"):
            mp.delenv(k, raising=False)
        mp.setenv("MHX_SPLIT", "0")
        for k, v in env.items():
            mp.setenv(k, v)
        return exprprobe.evaluate(mhx, body, NAMES, rows)


# ---- arguments ------------------------------------------------------------------------------------


def exp_args():
    rng = np.random.default_rng(11)
    bulk = np.concatenate([rng.uniform(-r, r, 340000) for r in (1.0, 30.0, 708.0)])
    sub = rng.uniform(-745.2, -708.4, 50000)           # subnormal results
    return bulk, sub


def exp_edges():
    import mpmath as mp
    mp.mp.prec = 200
    over = float(mp.log(mp.mpf(DBL_MAX)))              # ln(DBL_MAX)
    under = float(-1075 * mp.log(2))                    # exp(x) = 2^-1075: rounds to 0 below
    e = [0.0, -0.0, 1000.0, -1000.0, np.nextafter(1000.0, 2e3), np.nextafter(-1000.0, -2e3),
         1e300, -1e300, DBL_MAX, -DBL_MAX, -745.2, -745.1, -708.4, 709.0, 710.0, -746.0,
         np.nan, np.inf, -np.inf]
    for c in (over, under, 709.78, -708.39641853226408):   # (the last: exp = DBL_MIN)
        v = c
        for _ in range(6):
            v = np.nextafter(v, -np.inf)
        for _ in range(13):
            e.append(v)
            v = np.nextafter(v, np.inf)
    return np.array(e)


def log_args():
    rng = np.random.default_rng(12)
    table = random_doubles(rng, 400000, -1022, 1023)
    table = table[(table < LOG_WINDOW[0]) | (table >= LOG_WINDOW[1])]
    k = np.arange(1, 54, dtype=np.float64)
    near = np.concatenate([rng.uniform(*LOG_WINDOW, 200000),
                           1.0 + rng.uniform(-1, 1, 50000) * 2.0 ** -rng.integers(5, 50, 50000),
                           1.0 + 2.0 ** -k, 1.0 - 2.0 ** -k])
    near = near[(near >= LOG_WINDOW[0]) & (near < LOG_WINDOW[1])]
    edges = [LOG_WINDOW[0], LOG_WINDOW[1], 1.0, DBL_MIN, DBL_MAX, np.nextafter(DBL_MIN, 1.0)]
    for c in LOG_WINDOW + (1.0,):
        edges += [np.nextafter(c, 0.0), np.nextafter(np.nextafter(c, 0.0), 0.0), np.nextafter(c, 2.0),
                  np.nextafter(np.nextafter(c, 2.0), 2.0)]
    edges = np.concatenate([edges, np.ldexp(1.0, np.arange(-1022, 1024))])
    sub = np.concatenate([(rng.integers(1, 1 << 52, 20000, dtype=np.uint64)).view(np.float64),
                          np.ldexp(1.0, np.arange(-1074, -1022)),
                          [TINY, np.nextafter(DBL_MIN, 0.0), 3 * TINY]])
    bad = np.array([0.0, -0.0, -1.0, -TINY, -DBL_MIN, -DBL_MAX, -np.inf, np.inf, np.nan, -1e-300])
    return table, near, edges, sub, bad


def div_args():
    rng = np.random.default_rng(13)
    n = 200000
    a = random_doubles(rng, n, -500, 500, sign=0)
    b = random_doubles(rng, n, -1020, 1019, sign=0)
    q = a.astype(LD) / b.astype(LD)
    ok = (np.abs(q) >= DBL_MIN) & (np.abs(q) <= DBL_MAX)
    a, b = a[ok], b[ok]
    # divisor extremes: 1/b overflows (|b| < 2^-1024) or is subnormal (|b| > 2^1022), a/b finite
    bx = np.concatenate([random_doubles(rng, 2000, 1022, 1023, sign=0),
                         (rng.integers(1, 1 << 50, 2000, dtype=np.uint64)).view(np.float64)
                         * rng.choice([-1.0, 1.0], 2000)])
    ax = np.where(np.abs(bx) > 1.0, random_doubles(rng, 4000, 900, 1000, sign=0),
                  random_doubles(rng, 4000, -1000, -900, sign=0))
    return a, b, ax, bx


def ipow_args():
    rng = np.random.default_rng(14)
    ns = list(range(-40, 41)) + [127, 255, 1023, -127, -255, -1023]
    bases = np.concatenate([[1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0, -3.0, 1.0 + 2.0 ** -30],
                            rng.uniform(0.5, 2.0, 12), -rng.uniform(0.5, 2.0, 12),
                            rng.uniform(-30, 30, 12)])
    u, n = np.meshgrid(bases, np.array(ns, dtype=np.float64))
    return u.ravel(), n.ravel()


def intexp(base, power):
    """SBCL's intexp for a double base and an integer power (src/code/irrat.lisp):
    (cond ((minusp power) (/ (intexp base (- power))))
          (t (do ((nextn (ash power -1) (ash nextn -1))
                  (total (if (oddp power) base 1) (if (oddp nextn) (* base total) total)))
                 ((zerop nextn) total)
               (setq base (* base base)))))
    The do's step forms see the OLD nextn and the squared base."""
    if power < 0:
        t = intexp(base, -power)
        return 1.0 / t if t != 0.0 else math.copysign(math.inf, t)
    nextn, total = power >> 1, (base if power & 1 else 1.0)
    while nextn != 0:
        base = base * base
        if nextn & 1:
            total = base * total
        nextn >>= 1
    return total


def exact_args():
    rng = np.random.default_rng(15)
    sq = np.concatenate([random_doubles(rng, 20000, -1022, 1023), [0.0, TINY, DBL_MIN, DBL_MAX, 4.0, 2.0],
                         (rng.integers(1, 1 << 52, 2000, dtype=np.uint64)).view(np.float64)])
    ab = np.concatenate([random_doubles(rng, 20000, -1022, 1023, sign=0), [-TINY, -np.inf, np.inf]])
    fl = np.concatenate([rng.uniform(-1e3, 1e3, 20000), random_doubles(rng, 20000, -30, 60, sign=0),
                         [0.5, -0.5, 1.0, -1.0, 0.999999, -0.999999, 2.0 ** 52 + 0.5, -(2.0 ** 52) - 0.5,
                          2.0 ** 53, np.nextafter(1.0, 0.0), -np.nextafter(1.0, 0.0), -TINY, 1e300,
                          -1e300, np.inf, -np.inf]])
    ma = rng.uniform(-10, 10, 20000)
    mb = np.where(rng.random(20000) < 0.1, ma, rng.uniform(-10, 10, 20000))
    return sq, ab, fl, ma, mb


def ocml_args():
    rng = np.random.default_rng(16)
    return {"sin": rng.uniform(-10, 10, 20000), "cos": rng.uniform(-10, 10, 20000),
            "tan": rng.uniform(-1.5, 1.5, 20000), "atan": np.concatenate(
                [rng.uniform(-10, 10, 10000), random_doubles(rng, 10000, -30, 30, sign=0)]),
            "tanh": rng.uniform(-20, 20, 20000),
            "pow": (rng.uniform(1e-3, 10, 20000), rng.uniform(-30, 30, 20000))}


# ---- the default program: every routine, one hiprtc compile --------------------------------------


@pytest.fixture(scope="module")
def dflt(mhx):
    """{key: (a, b, device values)} of the default configuration (reciprocal division, the
    engine's exp and log)"""
    parts, keys = [], []

    def add(key, sel, a, b=0.0):
        r = rows_for(SEL[sel], a, b)
        parts.append(r)
        keys.append((key, r.shape[0]))

    eb, es = exp_args()
    add("exp", "exp", eb)
    add("exp_sub", "exp", es)
    add("exp_edge", "exp", exp_edges())
    lt, ln, le, lsub, lbad = log_args()
    for k, v in (("log_table", lt), ("log_near", ln), ("log_edge", le), ("log_sub", lsub),
                 ("log_bad", lbad)):
        add(k, "log", v)
    a, b, ax, bx = div_args()
    add("div", "div", a, b)
    add("div_x", "div", ax, bx)
    u, n = ipow_args()
    add("ipow", "ipow", u, n)
    sq, ab, fl, ma, mb = exact_args()
    add("sqrt", "sqrt", sq)
    add("abs", "abs", ab)
    add("floor", "floor", fl)
    add("min", "min", ma, mb)
    add("max", "max", ma, mb)
    for k, v in ocml_args().items():
        if k == "pow":
            add(k, k, v[0], v[1])
        else:
            add(k, k, v)
    rows = np.concatenate(parts)
    got = run(mhx, EVERYTHING, rows)
    out, o = {}, 0
    for (k, m), r in zip(keys, parts):
        out[k] = (r[:, 1], r[:, 2], got[o:o + m])
        o += m
    return out


def test_exp_below_one_ulp_and_equal_to_the_mirror(dflt, orc):
    """gexp on ~10^6 arguments uniform on |x| <= 1, 30 and 708: < 1 ulp of the 80-bit expl, and
    bit for bit the oracle's restatement (orc_mirror_gexp)"""
    x, _, got = dflt["exp"]
    u = ulps(got, np.exp(x.astype(LD)))
    print("exp: max %.4f ulp over %d arguments" % (u.max(), x.size))
    assert u.max() < 1.0, x[np.argmax(u)]
    mir = orc.mirror_gexp(x)
    assert np.all(same(got, mir)), x[~same(got, mir)][:5]


def test_exp_subnormal_results(dflt, orc):
    """exp on [-745.2, -708.4]: results below DBL_MIN, within 2^-1074 (the subnormals' ulp)"""
    x, _, got = dflt["exp_sub"]
    err = np.abs(got.astype(LD) - np.exp(x.astype(LD)))
    print("exp subnormal results: max error %.4f x 2^-1074" % float(err.max() / LD(TINY)))
    assert err.max() <= LD(TINY), x[np.argmax(err)]
    assert np.all(same(got, orc.mirror_gexp(x)))


def test_exp_edges(dflt, orc):
    """exp(0) == 1; both sides of ln(DBL_MAX) and of the underflow to 0 against mpmath; beyond
    |x| = 1000 inf / 0; NaN -> NaN and +-inf -> NaN (an infinite argument comes from an operation
    the reference would have trapped on: mhx_device.hpp gexp, include/mhx.h)"""
    import mpmath as mp
    mp.mp.prec = 200
    x, _, got = dflt["exp_edge"]
    assert np.all(same(got, orc.mirror_gexp(x)))
    for xi, g in zip(x.tolist(), got.tolist()):
        if not math.isfinite(xi):
            assert math.isnan(g), xi
            continue
        true = mp.exp(mp.mpf(xi))
        if xi == 0.0:
            assert g == 1.0
        elif xi > 1000.0:
            assert g == math.inf, xi
        elif xi < -745.2:
            assert g == 0.0, xi
        elif g == math.inf:
            assert true >= mp.mpf(DBL_MAX), xi          # overflow only where RN may overflow
        else:
            assert math.isfinite(g), xi
            unit = mp.mpf(2) ** max(int(mp.floor(mp.log(true, 2))) - 52, -1074)
            assert abs(mp.mpf(g) - true) <= unit, (xi, g)  # 1 ulp; 2^-1074 when subnormal


def test_log_table_branch(dflt, orc):
    """tlog's table branch: positive normals over the whole exponent range outside
    [0.9375, 1.0625): < 0.75 ulp (the bound the CPU restatement is held to), bit for bit
    orc_mirror_tlog"""
    x, _, got = dflt["log_table"]
    u = ulps(got, np.log(x.astype(LD)))
    print("log (table): max %.4f ulp over %d arguments" % (u.max(), x.size))
    assert u.max() < 0.75, x[np.argmax(u)]
    mir = orc.mirror_tlog(x)
    assert np.all(same(got, mir)), x[~same(got, mir)][:5]


def test_log_near_one_through_mlog(dflt):
    """mlog (v_rcp_f64 + two Newton steps for f/(2+f)) on [0.9375, 1.0625), 1 +- 2^-k included:
    < 1 ulp (measured 0.54).  Only the hardware can measure this one."""
    x, _, got = dflt["log_near"]
    u = ulps(got, np.log(x.astype(LD)))
    print("log (mlog, within 1/16 of 1): max %.4f ulp over %d arguments" % (u.max(), x.size))
    assert u.max() < 1.0, x[np.argmax(u)]


def test_log_edges(dflt, orc):
    """both window edges and their neighbours, 1 (exactly 0), DBL_MIN, DBL_MAX, every power of two"""
    x, _, got = dflt["log_edge"]
    assert np.all(got[x == 1.0] == 0.0)
    u = ulps(got, np.log(x.astype(LD)))
    inside = (x >= LOG_WINDOW[0]) & (x < LOG_WINDOW[1])
    assert u[inside].max() < 1.0, x[inside][np.argmax(u[inside])]
    assert u[~inside].max() < 0.75, x[~inside][np.argmax(u[~inside])]
    assert np.all(same(got[~inside], orc.mirror_tlog(x[~inside])))


def test_log_of_positive_subnormals_is_finite(dflt):
    """positive subnormals: the reference's (log x) is libm's, finite (-708.4 .. -744.4); mlog
    scales them into the normal range.  < 1 ulp (measured 0.50; NaN before mlog scaled them)."""
    x, _, got = dflt["log_sub"]
    assert np.all(np.isfinite(got)), x[~np.isfinite(got)][:5]
    u = ulps(got, np.log(x.astype(LD)))
    print("log (subnormal arguments): max %.4f ulp over %d arguments" % (u.max(), x.size))
    assert u.max() < 1.0, x[np.argmax(u)]


def test_log_invalid_arguments_are_nan(dflt):
    """0, -0, negatives, -inf, +inf, NaN -> NaN: a NaN log-posterior marks the chain as trapped,
    where the reference errors"""
    x, _, got = dflt["log_bad"]
    assert np.all(np.isnan(got)), list(zip(x, got))


def test_division_default_within_one_and_a_half_ulp(dflt):
    """(a + x) / b with b a parameter: the compiler hoists RN(1/b) out of the sweep
    (#pragma clang fp reciprocal(on)) and multiplies.  |b| in [2^-1020, 2^1020], quotient normal:
    within 1.5 ulp of the exact quotient (a * RN(1/b) can be 1.5 ulp from RN(a/b), not 1;
    measured 1.41 ulp, 1.3 % of the quotients above 1 ulp)"""
    a, b, got = dflt["div"]
    u = ulps(got, a.astype(LD) / b.astype(LD))
    print("division (reciprocal): max %.4f ulp, %.3f %% above 1 ulp, %d quotients"
          % (u.max(), 100.0 * np.mean(u > 1.0), a.size))
    assert u.max() < 1.5, (a[np.argmax(u)], b[np.argmax(u)])
    with np.errstate(all="ignore"):
        hoisted = a * (1.0 / b)
    assert np.all(same(got, hoisted))   # what the compiler made of it, exactly


def test_division_default_divisor_extremes(dflt):
    """b where 1/b overflows (|b| < 2^-1024: a * inf) or is subnormal (|b| > 2^1022: bits lost),
    a / b an ordinary number: the quotient is a * RN(1/b) as include/mhx.h documents - inf in
    the first case, a few ulp off in the second (measured 3.9)"""
    a, b, got = dflt["div_x"]
    with np.errstate(all="ignore"):
        hoisted = a * (1.0 / b)
        exact = a / b
    assert np.all(np.isfinite(exact))
    assert np.all(same(got, hoisted)), (a[~same(got, hoisted)][:3], b[~same(got, hoisted)][:3])
    small = np.abs(b) < 2.0 ** -1024
    assert np.all(np.isinf(got[small]))
    big = np.abs(b) > 2.0 ** 1022
    u = ulps(got[big], a[big].astype(LD) / b[big].astype(LD))
    print("division by |b| > 2^1022 (reciprocal): max %.4g ulp" % u.max())


def test_division_exact_with_switch(mhx):
    """MHX_EXPR_EXACT_DIV=1: IEEE divisions - bit for bit a / b, divisor extremes included"""
    a, b, ax, bx = div_args()
    a, b = np.concatenate([a[:50000], ax]), np.concatenate([b[:50000], bx])
    got = run(mhx, "(a + x) / b", rows_for(0, a, b), MHX_EXPR_EXACT_DIV="1")
    with np.errstate(all="ignore"):
        want = a / b
    assert np.all(same(got, want)), (a[~same(got, want)][:3], b[~same(got, want)][:3])


def test_ipow_is_sbcl_intexp(dflt):
    """ipow(u, n), n in -40..40 and +-127, +-255, +-1023, negative bases included: bit for bit
    SBCL's intexp order of multiplications (restated above)"""
    u, n, got = dflt["ipow"]
    want = np.array([intexp(ui, int(ni)) for ui, ni in zip(u.tolist(), n.tolist())])
    bad = ~same(got, want)
    assert not bad.any(), list(zip(u[bad][:3], n[bad][:3], got[bad][:3], want[bad][:3]))


def test_sqrt_abs_floor_min_max_exact(dflt):
    """correctly rounded sqrt (the reference's is), and abs / floor / min / max, bit for bit"""
    x, _, got = dflt["sqrt"]
    assert np.all(same(got, np.sqrt(x))), x[~same(got, np.sqrt(x))][:5]
    x, _, got = dflt["abs"]
    assert np.all(same(got, np.abs(x)))
    x, _, got = dflt["floor"]
    assert np.all(same(got, np.floor(x))), x[~same(got, np.floor(x))][:5]
    a, b, got = dflt["min"]
    assert np.all(got == np.where(a < b, a, b))
    a, b, got = dflt["max"]
    assert np.all(got == np.where(a > b, a, b))


def test_ocml_functions_are_wired(dflt):
    """sin cos tan atan tanh pow reach the functions of their names: <= 2 ulp over moderate
    ranges (a wiring test; ocml's own accuracy is not this project's).  Measured maxima on
    gfx950: sin 0.73, cos 0.69, tan 0.85, atan 1.28, tanh 0.74, pow 1.19 ulp."""
    refs = {"sin": np.sin, "cos": np.cos, "tan": np.tan, "atan": np.arctan, "tanh": np.tanh}
    for k, f in refs.items():
        x, _, got = dflt[k]
        u = ulps(got, f(x.astype(LD)))
        print("%s: max %.4f ulp" % (k, u.max()))
        assert u.max() <= 2.0, (k, x[np.argmax(u)])
    a, b, got = dflt["pow"]
    u = ulps(got, np.power(a.astype(LD), b.astype(LD)))
    print("pow: max %.4f ulp" % u.max())
    assert u.max() <= 2.0, (a[np.argmax(u)], b[np.argmax(u)])


# ---- the other configurations ---------------------------------------------------------------------


def explog_rows():
    eb, _ = exp_args()
    lt, ln, _, lsub, _ = log_args()
    rng = np.random.default_rng(17)
    ex = eb[rng.choice(eb.size, 100000, replace=False)]
    lg = np.concatenate([lt[:50000], ln[:50000], lsub[:5000]])
    return ex, lg, np.concatenate([rows_for(0, ex), rows_for(1, lg)])


def test_ocml_math_switch(mhx):
    """MHX_EXPR_OCML_MATH=1: ocml's exp and log - < 1 ulp, log(x <= 0) NaN, subnormal log finite"""
    ex, lg, rows = explog_rows()
    _, _, _, _, bad = log_args()
    rows = np.concatenate([rows, rows_for(1, bad)])
    got = run(mhx, EXPLOG, rows, MHX_EXPR_OCML_MATH="1")
    ge, gl, gb = got[:ex.size], got[ex.size:ex.size + lg.size], got[ex.size + lg.size:]
    ue, ul = ulps(ge, np.exp(ex.astype(LD))), ulps(gl, np.log(lg.astype(LD)))
    print("ocml exp: max %.4f ulp; ocml log: max %.4f ulp" % (ue.max(), ul.max()))
    assert ue.max() < 1.0 and ul.max() < 1.0
    assert np.all(np.isfinite(gl))
    xle0 = bad <= 0.0
    assert np.all(np.isnan(gb[xle0 | np.isnan(bad)]))


def test_families_give_identical_bits(mhx, orc):
    """MHX_FAMILY_WPG=8 and =16: the same exp / log bits (the same LDS tables, the other
    kernel family)"""
    ex, lg, rows = explog_rows()
    g8 = run(mhx, EXPLOG, rows, MHX_FAMILY_WPG="8")
    g16 = run(mhx, EXPLOG, rows, MHX_FAMILY_WPG="16")
    assert np.all(same(g8, g16))
    assert np.all(same(g8[:ex.size], orc.mirror_gexp(ex)))
