"""The statistical yardstick: problems whose posterior is known in closed form, exact draws from
them, the probability integral transform of a sample, statistics with their exact null standard
errors, closed-form acceptance probabilities, and a float64 numpy sampler of the specification
with switchable planted faults.  Shared by tests/test_stat_host.py (the yardstick holds and has
power, on the CPU), tests/test_gpu_stationarity.py (the stepping kernels preserve the exact
posterior) and tests/test_gpu_rng_stream.py (the device's own normals).  Plain numpy and math;
the normal equations are solved in offset_cases.hp()'s arithmetic (mpmath where it imports, else
long double).

THE PROBLEMS (flat priors unless stated, x = linspace(-1, 1, N), N = 64 points: the smallest size
that still runs the sweep, the butterfly and a padded tile):
  const1   POLY degree 0, normal likelihood, per-point sigma: theta ~ N(theta^, 1 / sum w)
  line2    POLY degree 1: theta ~ N(beta^, (A' W A)^-1), d = 2
  cubic4   POLY degree 3, d = 4
  global3  two POLY lines sharing the slope (K = 2, d = 3: the sum over functions); Gaussian from
           the stacked design matrix
  wall1    const1 with mhx_set_bounds putting the upper bound 0.5 posterior sigma above theta^:
           the truncated normal.  The prior is -1e10 (exp(1e-5 m) - 1) at a distance m beyond the
           bound, about -1e5 m: the target leaks beyond the wall on the scale 1e-5 T, a mass of
           phi(b) / Phi(b) 1e-5 sqrt(T) / sigma (b = 0.5 / sqrt(T)).  At const1's own scale
           (sigma ~ 0.012) that is 4e-4 - tens of states out of 65 536 - so wall1 is const1 with
           y and sigma multiplied by WALL_SCALE = 1e6: sigma ~ 1.2e4, a leak of about 1e-9 per state
           (leak(), asserted), 2e-4 states over all the wall1 runs of the suite.  At that scale
           the wall is hard and NO final state may lie outside the bound (asserted).
  rate1    POLY degree 0 with the Poisson likelihood, counts drawn with true rate 3: the rate is
           Gamma(sum k + 1, rate N).  On N = 1024 points, not 64: a proposal with a negative rate
           is a NaN log-posterior, where the reference signals and the engine freezes the chain
           (MHX_CHAIN_FP_TRAP) - correct, but not the Metropolis kernel.  The proposal is
           rate + L z with rate ~ (mean, sd), so it is negative with probability
           Phi(-mean / sqrt(sd^2 + L^2)) per draw: at N = 64, T = 3, L = 2.38 sd that is
           Phi(-3.1) = 9e-4 - one chain in twenty frozen within 64 steps - and still 4e-8 at
           T = 1 (8e6 draws per run).  At N = 1024 it is Phi(-12.4) at T = 3: no proposal is
           negative, which negative_proposal_probability() states and the tests assert (together
           with: no chain ends in MHX_CHAIN_FP_TRAP).
At temperature T the target is posterior^(1/T): covariance T Sigma for the Gaussian cases, the
same bound for wall1, Gamma(sum k / T + 1, rate N / T) for rate1.

THE THRESHOLDS are derived, not measured: |z| <= 5.5 for every z-score (p = 3.8e-8 two-sided),
sqrt(C) D <= 2.9 for every Kolmogorov statistic (asymptotic p = 2 exp(-2 2.9^2) = 1e-7).  A test
has at most ~300 statistics: a family-wise false-alarm rate of ~1e-5 at the fixed seeds."""
import functools
import math

import numpy as np

import offset_cases as oc
import problems as pb

Z_MAX = 5.5
KS_MAX = 2.9
N_POINTS = 64
RATE_POINTS = 1024
N_STEPS = 64
CHAINS = 65536            # the GPU tests' pooled chains ...
ENGINES = 4               # ... as engines of CHAINS / ENGINES with chain_offset 0, 16384, ...
TEMPERATURES = (1.0, 3.0)
WALL_SCALE = 1e6
WALL_SIGMAS = 0.5         # the upper bound, in posterior sigmas above theta^
MAX_ABS_NORMAL = math.sqrt(2.0 * 53.0 * math.log(2.0))   # Box-Muller's ceiling: u1 >= 2^-53

NAMES = ("const1", "line2", "cubic4", "global3", "wall1", "rate1")
L_KINDS = ("good", "bad")       # (2.38 / sqrt(d)) chol(T Sigma); diag(0.3 sd): deliberately bad


def philox(seed):
    return np.random.Generator(np.random.Philox(seed))


def start_draws(cs, T, chains=CHAINS):
    """the exact draws the walks of problem cs at temperature T start from, on the CPU and on the
    GPU.  (The seed takes T in: a Gaussian case at T = 3 is otherwise the T = 1 walk rescaled,
    draw for draw and accept test for accept test, and its statistics repeat T = 1's.)"""
    return cs.target(T).draw(philox([cs.seed, int(T)]), chains)


# ---- the normal distribution, vectorised from math.erfc -------------------------------------------
_erfc = np.frompyfunc(math.erfc, 1, 1)
_SQRT2 = math.sqrt(2.0)


def ndtr(x):
    """Phi(x), elementwise, to a few ulp in both tails"""
    return 0.5 * np.asarray(_erfc(-np.asarray(x, dtype=np.float64) / _SQRT2), dtype=np.float64)


def ndtri(p):
    """Phi^-1(p), elementwise: Acklam's rational start (1.2e-9 relative) and two Halley steps on
    ndtr; p is clipped to [1e-300, 1 - 2^-53]"""
    p = np.clip(np.asarray(p, dtype=np.float64), 1e-300, 1.0 - 2.0 ** -53)
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
         1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
         6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
         -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
         3.754408661907416e+00)
    x = np.empty_like(p)
    lo, hi = p < 0.02425, p > 1.0 - 0.02425
    mid = ~(lo | hi)
    q = p[mid] - 0.5
    r = q * q
    x[mid] = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q / \
             (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0)
    for sel, sign in ((lo, 1.0), (hi, -1.0)):
        q = np.sqrt(-2.0 * np.log(p[sel] if sign > 0 else 1.0 - p[sel]))
        x[sel] = sign * (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / \
            ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0)
    for _ in range(2):
        e = ndtr(x) - p
        u = e * math.sqrt(2.0 * math.pi) * np.exp(0.5 * x * x)
        x = x - u / (1.0 + 0.5 * x * u)
    return x


def chi2_cdf_even(r, d):
    """P(chi^2_d <= r) for even d: 1 - exp(-r/2) sum_{j < d/2} (r/2)^j / j!"""
    assert d % 2 == 0 and d >= 2
    h = 0.5 * np.asarray(r, dtype=np.float64)
    term, tot = np.ones_like(h), np.ones_like(h)
    for j in range(1, d // 2):
        term = term * h / j
        tot = tot + term
    return -np.expm1(-h) if d == 2 else 1.0 - np.exp(-h) * tot


def gamma_p(a, x):
    """the regularised lower incomplete gamma function P(a, x), elementwise in x > 0, any a > 0:
    the series exp(-x) x^a sum_n x^n / Gamma(a + n + 1), every term positive, the first formed in
    log space, the later ones by their ratio x / (a + n).  For an integer a this is the Poisson
    sum P(Poisson(x) >= a) = 1 - sum_{j < a} exp(-x) x^j / j! (gamma_p_poisson_sum)."""
    x0 = np.asarray(x, dtype=np.float64)
    cap = a + 40.0 * math.sqrt(a) + 200.0     # (beyond it P = 1 to every digit; bounds the series)
    ok = np.isfinite(x0) & (x0 > 0) & (x0 <= cap)
    x = np.where(ok, x0, 1.0)                 # (0 at and below 0, NaN for a NaN: filled in below)
    term = np.exp(-x + a * np.log(x) - math.lgamma(a + 1.0))
    tot = term.copy()
    n = 0
    top = float(np.max(x)) if x.size else 0.0
    while x.size:
        n += 1
        term = term * x / (a + n)
        tot = tot + term
        if a + n > top and float(np.max(term / np.maximum(tot, 1e-300))) < 1e-17:
            break
    return np.where(ok, np.minimum(tot, 1.0), np.where(x0 <= 0, 0.0, np.where(x0 > cap, 1.0, np.nan)))


def gamma_p_poisson_sum(a, x):
    """P(a, x) for an integer a as the finite Poisson sum, every term in log space"""
    a = int(a)
    x = np.asarray(x, dtype=np.float64)
    lx = np.log(x)
    q = np.zeros_like(x)
    for j in range(a):
        q = q + np.exp(-x + j * lx - math.lgamma(j + 1.0))
    return 1.0 - q


# ---- the targets ---------------------------------------------------------------------------------
class GaussianTarget:
    kind = "gauss"

    def __init__(self, mean, cov, T):
        self.mean, self.T = np.asarray(mean, dtype=np.float64), float(T)
        self.cov = T * np.asarray(cov, dtype=np.float64)
        self.chol = np.linalg.cholesky(self.cov)
        self.d = self.mean.size
        self.sd = np.sqrt(np.diag(self.cov))

    def draw(self, rng, C):
        return self.mean + rng.standard_normal((C, self.d)) @ self.chol.T

    def scores(self, theta):
        """the whitened sample: chol(T Sigma)^-1 (theta - mean), N(0, I) under the target"""
        return np.linalg.solve(self.chol, (np.asarray(theta) - self.mean).T).T

    def pit(self, theta):
        """columns that are U(0, 1) under the target, and their names"""
        w = self.scores(theta)
        cols, names = [ndtr(w[:, j]) for j in range(self.d)], ["w%d" % j for j in range(self.d)]
        if self.d in (2, 4):
            cols.append(chi2_cdf_even((w * w).sum(axis=1), self.d))
            names.append("radius")
        return np.stack(cols, axis=1), names


class _Scalar:
    d = 1

    def scores(self, theta):
        """normal scores Phi^-1(F(theta)): N(0, 1) under the target"""
        return ndtri(self.cdf(np.asarray(theta).reshape(-1)))[:, None]

    def pit(self, theta):
        return self.cdf(np.asarray(theta).reshape(-1))[:, None], ["w0"]


class TruncatedTarget(_Scalar):
    """N(mean, T sigma^2) below the bound `hi`"""
    kind = "trunc"

    def __init__(self, mean, sigma, hi, T):
        self.mean, self.T, self.hi = float(mean), float(T), float(hi)
        self.s = float(sigma) * math.sqrt(T)
        self.sd = np.array([self.s])            # (the scale the proposals are sized by)
        self.b = (self.hi - self.mean) / self.s

    def draw(self, rng, C):
        out = np.empty(0)
        while out.size < C:                      # rejection from the untruncated normal
            t = self.mean + self.s * rng.standard_normal(2 * C)
            out = np.concatenate([out, t[t < self.hi]])
        return out[:C, None]

    def cdf(self, t):
        return np.minimum(ndtr((t - self.mean) / self.s) / float(ndtr(self.b)), 1.0)


class GammaTarget(_Scalar):
    """Gamma(sum k / T + 1, rate n / T): the posterior^(1/T) of a Poisson rate under a flat prior"""
    kind = "gamma"

    def __init__(self, sum_k, n, T):
        self.T = float(T)
        self.a, self.rate = sum_k / self.T + 1.0, n / self.T
        self.mean = self.a / self.rate
        self.sd = np.array([math.sqrt(self.a) / self.rate])

    def draw(self, rng, C):
        return rng.gamma(self.a, 1.0 / self.rate, C)[:, None]

    def cdf(self, t):
        return gamma_p(self.a, self.rate * t)


# ---- the problems --------------------------------------------------------------------------------
def _solve_normal_equations(rows, sigma, y):
    """(beta^, Sigma = (A' W A)^-1) as float64 from the design rows (high-precision numbers),
    sigma and y (float64), by Gauss-Jordan elimination in high precision"""
    E = oc.hp()
    d = len(rows[0])
    M = [[E.num(0) for _ in range(d)] for _ in range(d)]
    b = [E.num(0) for _ in range(d)]
    for r, s, yv in zip(rows, sigma, y):
        w = E.num(1) / (E.num(float(s)) * E.num(float(s)))
        for j in range(d):
            if r[j] == 0:
                continue
            b[j] = b[j] + w * r[j] * E.num(float(yv))
            for k in range(d):
                M[j][k] = M[j][k] + w * r[j] * r[k]
    aug = [M[j] + [E.num(1 if k == j else 0) for k in range(d)] + [b[j]] for j in range(d)]
    for j in range(d):                          # (symmetric positive definite: no pivoting)
        piv = aug[j][j]
        aug[j] = [v / piv for v in aug[j]]
        for i in range(d):
            if i != j:
                f = aug[i][j]
                aug[i] = [vi - f * vj for vi, vj in zip(aug[i], aug[j])]
    cov = np.array([[float(aug[j][d + k]) for k in range(d)] for j in range(d)])
    beta = np.array([float(aug[j][2 * d]) for j in range(d)])
    return beta, 0.5 * (cov + cov.T)


class Case:
    """one problem: spec (problems.Spec, for the engine and the oracle), d, target(T), the float64
    log-posterior of the reference sampler (logpost: [C, d] -> [C], constants dropped), start
    seed"""

    def target(self, T):
        raise NotImplementedError

    def l_matrix(self, kind, T):
        t = self.target(T)
        if kind == "bad":
            return np.diag(0.3 * t.sd)
        if t.kind == "gauss":
            return (2.38 / math.sqrt(t.d)) * t.chol
        return np.diag(2.38 * t.sd)


class _Linear(Case):
    """functions (idx, x, y, sigma) of POLY models over a shared parameter vector"""

    def __init__(self, name, d, fns, seed, bounds=None):
        self.name, self.d, self.seed = name, d, seed
        self.spec = pb.Spec(d)
        E = oc.hp()
        rows, sig, ys = [], [], []
        for k, (idx, x, y, s) in enumerate(fns):
            self.spec.add(pb.POLY, (), idx, x, y, s, pb.NORMAL, bounds if k == 0 else None)
            for xv in x:
                r = [E.num(0) for _ in range(d)]
                p = E.num(1)
                for j in idx:                   # POLY: p[0] + p[1] x + p[2] x^2 + ...
                    r[j] = r[j] + p
                    p = p * E.num(float(xv))
                rows.append(r)
            sig += list(s)
            ys += list(y)
        self.beta, self.cov = _solve_normal_equations(rows, sig, ys)
        # the reference sampler's log-posterior, from the data in float64: -1/2 t' M t + b' t
        A = np.array([[float(v) for v in r] for r in rows])
        w = 1.0 / np.square(np.array(sig))
        self._M, self._b = A.T @ (A * w[:, None]), A.T @ (w * np.array(ys))
        self.bounds = bounds

    def logpost(self, th):
        return ((th @ (-0.5 * self._M)) * th).sum(axis=1) + th @ self._b

    def target(self, T):
        return GaussianTarget(self.beta, self.cov, T)


class _Wall(_Linear):
    def __init__(self, name, fns, seed):
        _Linear.__init__(self, name, 1, fns, seed)
        sigma = math.sqrt(self.cov[0, 0])
        self.hi = float(self.beta[0] + WALL_SIGMAS * sigma)
        self.lo = float(self.beta[0] - 1e3 * sigma)          # (never reached)
        self.bounds = ([0], [self.lo], [self.hi])
        self.spec.bounds[0] = self.bounds

    def logpost(self, th):
        p = th[:, 0]
        m = np.minimum(np.abs(p - self.hi), np.abs(p - self.lo))
        pen = np.where((self.lo < p) & (p < self.hi), 0.0, -1e10 * np.expm1(m * 1e-5))
        return _Linear.logpost(self, th) + pen

    def target(self, T):
        return TruncatedTarget(self.beta[0], math.sqrt(self.cov[0, 0]), self.hi, T)

    def leak(self, T):
        """the target's mass beyond the bound (module docstring)"""
        t = self.target(T)
        phi = math.exp(-0.5 * t.b * t.b) / math.sqrt(2.0 * math.pi)
        return phi / float(ndtr(t.b)) * 1e-5 * T / t.s


class _Rate(Case):
    def __init__(self, name, x, k, seed):
        self.name, self.d, self.seed = name, 1, seed
        self.spec = pb.Spec(1)
        self.spec.add(pb.POLY, (), [0], x, k, None, pb.POISSON)
        self.sum_k, self.n = float(np.sum(k)), len(k)
        self.bounds = None

    def logpost(self, th):
        lam = th[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum_k * np.log(lam) - self.n * lam     # NaN below 0: never accepted

    def target(self, T):
        return GammaTarget(self.sum_k, self.n, T)

    def negative_proposal_probability(self, kind, T):
        """P(rate + L z < 0) per draw in stationarity, the rate taken as N(mean, sd)"""
        t = self.target(T)
        L = float(self.l_matrix(kind, T)[0, 0])
        return float(ndtr(-t.mean / math.sqrt(t.sd[0] ** 2 + L * L)))


def _data(seed, n, truth, scale=1.0):
    rng = philox(seed)
    x = np.linspace(-1.0, 1.0, n)
    sig = rng.uniform(0.05, 0.15, n)
    y = pb.model_eval_np(pb.POLY, (), np.asarray(truth, dtype=np.float64), x) + sig * rng.standard_normal(n)
    return x, y * scale, sig * scale


@functools.lru_cache(maxsize=None)
def case(name, n=None):
    """the problem `name`; n: another number of points (the split-mode test's line2 on 8192)"""
    n = n or (RATE_POINTS if name == "rate1" else N_POINTS)
    if name == "const1":
        return _Linear(name, 1, [([0],) + _data(101, n, [0.7])], seed=1001)
    if name == "line2":
        return _Linear(name, 2, [([0, 1],) + _data(102, n, [0.4, -0.8])], seed=1002)
    if name == "cubic4":
        return _Linear(name, 4, [([0, 1, 2, 3],) + _data(103, n, [0.3, -0.5, 0.9, 0.6])], seed=1003)
    if name == "global3":       # theta = (a0, b, a1): a0 + b x on one dataset, a1 + b x on the other
        return _Linear(name, 3, [([0, 1],) + _data(104, n, [0.2, 0.5]),
                                 ([2, 1],) + _data(105, n, [-0.3, 0.5])], seed=1004)
    if name == "wall1":
        return _Wall(name, [([0],) + _data(101, n, [0.7], WALL_SCALE)], seed=1005)
    if name == "rate1":
        k = philox(106).poisson(3.0, n).astype(np.float64)
        return _Rate(name, np.linspace(-1.0, 1.0, n), k, seed=1006)
    raise KeyError(name)


# ---- statistics: name -> (value, lo, hi, kind) -------------------------------------------------------
def z_stat(v):
    return (float(v), -Z_MAX, Z_MAX, "z")


def ks_statistic(u):
    """sqrt(n) D of a sample against U(0, 1)"""
    u = np.sort(np.asarray(u, dtype=np.float64))
    n = u.size
    i = np.arange(1, n + 1)
    return math.sqrt(n) * max(float(np.max(i / n - u)), float(np.max(u - (i - 1) / n)))


def binned_chi2_z(u, bins):
    """the equiprobable chi^2 of a U(0, 1) sample over `bins` bins as (chi^2 - (bins - 1)) /
    sqrt(2 (bins - 1))"""
    u = np.asarray(u, dtype=np.float64)
    k = np.minimum((u * bins).astype(np.int64), bins - 1)
    cnt = np.bincount(k, minlength=bins)
    e = u.size / bins
    return (float(np.sum(np.square(cnt - e)) / e) - (bins - 1)) / math.sqrt(2.0 * (bins - 1))


def moment_z(w):
    """z-scores of the first four moments of an N(0, 1) sample (SE 1/sqrt C, sqrt(2/C),
    sqrt(15/C), sqrt(96/C))"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    C = w.size
    w2 = w * w
    return (float(np.mean(w)) * math.sqrt(C), (float(np.mean(w2)) - 1.0) / math.sqrt(2.0 / C),
            float(np.mean(w2 * w)) / math.sqrt(15.0 / C), (float(np.mean(w2 * w2)) - 3.0) / math.sqrt(96.0 / C))


def sample_statistics(target, theta):
    """every statistic of a sample theta [C, d] that should be exact independent draws of
    `target`: the four moments of every whitened coordinate, every cross moment, the Kolmogorov
    statistic and a 64-bin chi^2 of every PIT column"""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, target.d)
    C = theta.shape[0]
    w = target.scores(theta)
    out = {}
    for j in range(target.d):
        for nm, v in zip(("mean", "var", "m3", "m4"), moment_z(w[:, j])):
            out["%s[%d]" % (nm, j)] = z_stat(v)
        for k in range(j):
            out["cross[%d,%d]" % (k, j)] = z_stat(float(np.mean(w[:, j] * w[:, k])) * math.sqrt(C))
    U, names = target.pit(theta)
    for j, nm in enumerate(names):
        out["ks[%s]" % nm] = (ks_statistic(U[:, j]), 0.0, KS_MAX, "ks")
        out["chi2[%s]" % nm] = z_stat(binned_chi2_z(U[:, j], 64))
    return out


def violations(stats):
    return {k: v for k, v in stats.items() if not (v[1] <= v[0] <= v[2])}   # (a NaN is one)


def worst(stats):
    """(max |z|, max sqrt(C) D) of a set of statistics"""
    z = [abs(v[0]) for v in stats.values() if v[3] == "z"]
    ks = [v[0] for v in stats.values() if v[3] == "ks"]
    return (max(z) if z else 0.0), (max(ks) if ks else 0.0)


def report(label, stats):
    z, ks = worst(stats)
    return "%-34s max |z| %5.2f   max sqrt(C) D %5.2f   (%d statistics)" % (label, z, ks, len(stats))


def binomial_z(count, n, p):
    return (count - n * p) / math.sqrt(n * p * (1.0 - p))


# ---- closed-form acceptance probabilities -----------------------------------------------------------
def accept_from_mode(s, T, d):
    """one step from the mode with L = s chol(Sigma) at temperature T is accepted with
    probability (1 + s^2 / T)^(-d/2)"""
    return (1.0 + s * s / T) ** (-0.5 * d)


def accepted_variance(s, T):
    """... and the accepted proposals have this whitened variance per coordinate"""
    return s * s / (1.0 + s * s / T)


def accept_stationary_1d(s):
    """in stationarity, d = 1 and T = 1: a proposal of s posterior sigmas is accepted with
    probability (2 / pi) arctan(2 / s)"""
    return 2.0 / math.pi * math.atan(2.0 / s)


def mode_step_statistics(target1, theta, moved, s, T):
    """one step of every chain from the mode with L = s chol(Sigma) at temperature T (target1: the
    target at T = 1; theta [C, d] after the step, moved [C]: it was accepted): the accepted
    fraction as a binomial z-score, and the whitened second moment of the accepted proposals,
    coordinate by coordinate, against accepted_variance (they are N(0, v): SE v sqrt(2 / n))"""
    moved = np.asarray(moved, dtype=bool)
    w = target1.scores(np.asarray(theta)[moved])
    n, v = w.shape[0], accepted_variance(s, T)
    out = {"accepted": z_stat(binomial_z(int(moved.sum()), moved.size, accept_from_mode(s, T, target1.d)))}
    for j in range(target1.d):
        out["accepted_var[%d]" % j] = z_stat((float(np.mean(w[:, j] ** 2)) / v - 1.0) / math.sqrt(2.0 / n))
    return out


# ---- the reference sampler ---------------------------------------------------------------------------
FAULTS = ("ignore_T", "times_T", "no_log", "u_from_z", "z_mean", "stale_prob")


def reference_walk(cs, T, L, theta0, n, rng, fault=None):
    """n steps of the specification in float64, vectorised over the chains theta0 [C, d]:
    proposal theta + L z, accepted when (p1 > p0) or ((p1 - p0) / T > log u), u on (0, 1].
    Returns (theta [C, d], moved [C]: the last step was accepted).  fault: one of FAULTS, planted:
      ignore_T    p1 - p0 > log u            times_T   (p1 - p0) T > log u
      no_log      (p1 - p0) / T > u - 1      u_from_z  u = Phi(z_0)
      z_mean      z + 0.02                   stale_prob  10 % of the accepted steps keep the old p0"""
    assert fault is None or fault in FAULTS
    th = np.array(theta0, dtype=np.float64).reshape(-1, cs.d)
    C = th.shape[0]
    L = np.asarray(L, dtype=np.float64)
    p0 = cs.logpost(th)
    acc = np.zeros(C, dtype=bool)
    for _ in range(n):
        z = rng.standard_normal((C, cs.d))
        if fault == "z_mean":
            z = z + 0.02
        u = ndtr(z[:, 0]) if fault == "u_from_z" else 1.0 - rng.random(C)
        prop = th + z @ L.T
        p1 = cs.logpost(prop)
        with np.errstate(invalid="ignore", divide="ignore"):
            dl = p1 - p0
            lhs = dl if fault == "ignore_T" else dl * T if fault == "times_T" else dl / T
            acc = (p1 > p0) | (lhs > (u - 1.0 if fault == "no_log" else np.log(u)))
        th[acc] = prop[acc]
        new = np.where(acc, p1, p0)
        if fault == "stale_prob":
            stale = acc & (rng.random(C) < 0.1)
            new[stale] = p0[stale]
        p0 = new
    return th, acc


# ---- a stream of normals: z [chains, draws, lanes] ------------------------------------------------------
def _poisson_range(mu, p=1e-7):
    """[lo, hi] with P(X < lo) <= p/2 and P(X > hi) <= p/2 for X ~ Poisson(mu)"""
    pmf, k, cdf, lo, hi = math.exp(-mu), 0, 0.0, 0, None
    while hi is None:
        if cdf + pmf <= 0.5 * p:
            lo = k + 1
        cdf += pmf
        if 1.0 - cdf <= 0.5 * p and k >= mu:
            hi = k
        k += 1
        pmf *= mu / k
    return lo, hi


def _pair_z(pairs):
    """sqrt(n) r of the pairs (a, b) given slab by slab, for the values and for their squares"""
    acc = np.zeros((2, 6))
    for a, b in pairs:
        a, b = np.ravel(a), np.ravel(b)
        for q, (s, t) in enumerate(((a, b), (a * a, b * b))):
            acc[q] += (s.size, s.sum(), t.sum(), np.dot(s, t), np.dot(s, s), np.dot(t, t))
    out = []
    for n, sa, sb, sab, saa, sbb in acc:
        cov = sab / n - sa / n * sb / n
        out.append(math.sqrt(n) * cov / math.sqrt((saa / n - (sa / n) ** 2) * (sbb / n - (sb / n) ** 2)))
    return out


def stream_statistics(z):
    """every statistic of z [chains, draws, lanes] that should be independent N(0, 1): the four
    moments, a 256-bin equiprobable chi^2 against Phi, Kolmogorov on a fixed subsample of 2^20
    (every (size // 2^20)-th value), the counts of |z| > k for k = 1..4 as binomial z-scores, the
    count of |z| > 5 inside its two-sided Poisson range at p = 1e-7, max |z| <= sqrt(2 53 ln 2),
    and sqrt(n) times the correlation of z and of z^2 between neighbouring lanes of a draw, the
    same lane in consecutive draws, the same lane and draw in neighbouring chains, and the first
    and the last lane"""
    z = np.asarray(z, dtype=np.float64)
    assert z.ndim == 3
    flat = z.reshape(-1)
    n = flat.size
    out = {}
    for nm, v in zip(("mean", "var", "m3", "m4"), moment_z(flat)):
        out[nm] = z_stat(v)
    bins = 256
    edges = ndtri(np.arange(1, bins) / bins)
    cnt = np.zeros(bins)
    for lo in range(0, n, 1 << 22):
        cnt += np.bincount(np.searchsorted(edges, flat[lo:lo + (1 << 22)]), minlength=bins)
    e = n / bins
    out["chi2_256"] = z_stat((float(np.sum(np.square(cnt - e)) / e) - (bins - 1)) / math.sqrt(2.0 * (bins - 1)))
    m = min(n, 1 << 20)
    out["ks"] = (ks_statistic(ndtr(flat[::max(n // m, 1)][:m])), 0.0, KS_MAX, "ks")
    az = np.abs(flat)
    for k in (1, 2, 3, 4):
        out["tail%d" % k] = z_stat(binomial_z(int(np.count_nonzero(az > k)), n, math.erfc(k / _SQRT2)))
    lo, hi = _poisson_range(n * math.erfc(5.0 / _SQRT2))
    out["tail5"] = (float(np.count_nonzero(az > 5.0)), float(lo), float(hi), "count")
    out["max_abs"] = (float(az.max()), 0.0, MAX_ABS_NORMAL, "max")
    del az
    C = z.shape[0]
    for nm, pairs in (("lanes", ((z[c, :, :-1], z[c, :, 1:]) for c in range(C))),
                      ("draws", ((z[c, :-1, :], z[c, 1:, :]) for c in range(C))),
                      ("chains", ((z[c], z[c + 1]) for c in range(C - 1))),
                      ("first_last_lane", ((z[c, :, 0], z[c, :, -1]) for c in range(C)))):
        r1, r2 = _pair_z(pairs)
        out["corr_z[%s]" % nm], out["corr_z2[%s]" % nm] = z_stat(r1), z_stat(r2)
    return out
