"""Peak models far from the origin: problems placed on x = off + span * [0, 1], a high-precision
reference of the reference's formulas, and the ARGUMENT TERM of the kernels' accuracy bound
("The argument of a peak"), shared by tests/test_offset_host.py (the mirror, on the
CPU) and tests/test_gpu_offset.py (the device).

The bound, derived from the kernels' operations (csrc/mhx_device.hpp, PeaksModel::prepare):
    iw = fl(g / w)           g = sqrt(log2 e) for a Gaussian, 1 for a Lorentzian
    c  = fl(-mu iw)          = -mu iw (1 + e2),  |e2| <= 2^-53
    t  = fma(x, iw, c)       = iw (x - mu - mu e2) (1 + e3)
so the device's peak is the reference formula's with its ARGUMENT moved by mu e2, at most
    delta = |mu| 2^-53                                                  (direct form)
and the value moves by at most |A| |dg/dx| delta.  The relative roundings of iw (common to both
products) and of t (e3) scale t as a whole; near the origin they are what the existing
1e-12 sum |term| holds, and at an offset they are |x - mu| / |mu| times smaller than delta: the one
explicit factor SAFETY = 2 stands for them.
On a window that goes by the uniform-grid recurrence a value is the seed's (formed at the lane's
actual x) advanced as if the later points sat exactly on x_seed + j 64 h; the host accepts a grid
whose points depart from it by what mhx_set_dataset's rule tolerates, 8 ulp of the window's max |x|:
    delta = |mu| 2^-53 + 8 ulp(max |x| of the window)                   (recurrence)
(there SAFETY also covers a seed and a later point that depart to opposite sides).  The
pseudo-Voigt's fast path rounds iw g and c g separately: delta = (|x| + 2 |mu|) 2^-53 for its
Gaussians.  The log-posterior propagates it: sum_i |d term_i / d f_i| sum_k |A_k| |dg_k/dx|(x_i) delta_k.
Nothing here is fitted to a measurement; a bound needs no extra precision and is plain numpy."""
import functools
import math

import numpy as np

import problems as pb

REL = 1e-12          # the bound every kernel is held to near the origin: REL * sum |term|
SAFETY = 2.0         # the one safety factor of the argument term (see above)
U53 = 2.0 ** -53
SQRT_LOG2E = math.sqrt(math.log2(math.e))
WINDOW = 2048        # points of a seeding window (kPadPoints)

# offset, span.  (0, 1): the control - the helpers reproduce what the suite measures at the origin;
# (1023.5, 1): ulp(x) doubles in the middle of the data
CASES = [(0.0, 1.0), (2000.0, 1.0), (2000.0, 1e-3), (-2000.0, 1.0), (1e5, 1.0), (1023.5, 1.0)]
CASE_IDS = ["off%g_span%g" % c for c in CASES]
N_VECTORS = 12


# ---- the high-precision arithmetic -------------------------------------------------------------
class _Mp:
    name = "mpmath, 120 bits"

    def __init__(self, mpmath):
        self.mp = mpmath.mp.clone()
        self.mp.prec = 120
        self.num, self.exp, self.log = self.mp.mpf, self.mp.exp, self.mp.log
        self.sin, self.cos, self.pi = self.mp.sin, self.mp.cos, +self.mp.pi


class _Ld:
    name = "numpy longdouble"

    def __init__(self):
        self.num, self.exp, self.log, self.sin, self.cos = (np.longdouble, np.exp, np.log, np.sin,
                                                            np.cos)
        self.pi = np.longdouble(4) * np.arctan(np.longdouble(1))


@functools.lru_cache(maxsize=None)
def hp():
    """mpmath at >= 100 bits when it imports, else a long double of >= 63 mantissa bits; neither: an
    error - the tests that need it fail, they do not skip"""
    try:
        import mpmath
    except ImportError:
        mpmath = None
    if mpmath is not None:
        return _Mp(mpmath)
    if np.finfo(np.longdouble).nmant >= 63:
        return _Ld()
    raise RuntimeError("no high-precision arithmetic: mpmath does not import and numpy's long double "
                       "has %d mantissa bits" % np.finfo(np.longdouble).nmant)


def _horner(E, c, x):
    if len(c) == 0:
        return E.num(0)
    acc = c[-1]
    for cj in c[-2::-1]:
        acc = acc * x + cj
    return acc


def hp_values(model, shape, p, x):
    """the formulas of oracle/mhx_oracle.c's orc_model_eval in high precision: a list, one per x
    (x: float64 values, or numbers that are in high precision already)"""
    E = hp()
    p = [E.num(float(v)) for v in p]
    one = E.num(1)
    out = []
    if model in (pb.GAUSS, pb.LORENTZ):
        nbg, npk = shape
        bg, peaks = p[:nbg], [p[nbg + 3 * k: nbg + 3 * k + 3] for k in range(npk)]
    for xv in (x if len(x) and isinstance(x[0], type(one)) else [E.num(v) for v in x]):
        if model == pb.POLY:
            f = _horner(E, p, xv)
        elif model in (pb.GAUSS, pb.LORENTZ):
            f = _horner(E, bg, xv)
            for A, mu, w in peaks:
                t = (xv - mu) / w
                f = f + (A * E.exp(-(t * t)) if model == pb.GAUSS else A / (one + t * t))
        elif model == pb.LORDER:
            u = (xv - p[2]) / p[1]
            q = one + u * u
            num = E.cos(p[3]) * (-2 * u) + E.sin(p[3]) * (one - u * u)
            f = ((p[0] * num) / (q * q) + p[4]) + p[5] * xv
        elif model == pb.EXPDECAY:
            f = p[0] * E.exp(-(xv / p[1])) + p[2]
        elif model == pb.SINUS:
            f = p[0] * E.sin(p[1] * xv + p[2]) + p[3]
        elif model == pb.PVOIGT2:
            u1, u2 = (xv - p[3]) / p[4], (xv - p[6]) / p[7]
            s1, s2 = u1 * u1, u2 * u2
            pv1 = p[5] / (one + s1) + (one - p[5]) * E.exp(-s1)
            pv2 = p[8] / (one + s2) + (one - p[8]) * E.exp(-s2)
            f = ((p[1] + p[2] * xv) + p[10] * (xv * xv)) + p[0] * (pv1 + p[9] * pv2)
        else:
            raise NotImplementedError(model)
        out.append(f)
    return out


def hp_error(got, ref):
    """|got - ref| per value as float64, the difference taken in high precision"""
    E = hp()
    return np.array([float(abs(E.num(float(g)) - r)) for g, r in zip(got, ref)])


_DATASETS = {}


def _dataset_hp(s, k):
    """x, y and the per-point constants of dataset k in high precision, per dataset and not per
    vector: (x, y, sigma, a - log sigma) for the normal likelihood, (x, y, None, -log-factorial(y))
    for Poisson - the reference's log-factorial is a running sum of single floats
    (orc_log_factorial): a constant of the data, taken as the oracle gives it"""
    key = (id(s), k)
    if key not in _DATASETS:
        E = hp()
        x, y, sig, lik = s.data[k]
        xs, ys = [E.num(float(v)) for v in x], [E.num(float(v)) for v in y]
        if lik == pb.POISSON:
            import oraclelib
            lf = oraclelib.lib().orc_log_factorial
            _DATASETS[key] = (s, xs, ys, None, [-E.num(lf(float(v), 0)) for v in y])
        else:
            a = -E.log(2 * E.pi) / 2
            sg = [E.num(float(v)) for v in sig]
            _DATASETS[key] = (s, xs, ys, sg, [a - E.log(v) for v in sg])
    return _DATASETS[key][1:]


def hp_logpost(s, theta):
    """(log-posterior, sum |term|) of a Spec whose bounds are off, summed over the points and the
    functions.  Normal: per point orc_log_normal's (a + b) + c with a = -1/2 log 2 pi,
    b = -log sigma, c = -1/2 ((y - f) / sigma)^2; with the cutoff that term clamped from below,
    (max -5000d0 term) M:426; Poisson: orc_log_poisson's (k log lambda - lambda) - log-factorial(k).
    The first in high precision, the second a float"""
    E = hp()
    total, scale = E.num(0), 0.0
    for k, ((model, shape, idx), (x, y, sig, lik), b) in enumerate(zip(s.fns, s.data, s.bounds)):
        assert lik in (pb.NORMAL, pb.CUTOFF, pb.POISSON) and b is None
        xs, ys, sg, cst = _dataset_hp(s, k)
        f = hp_values(model, shape, np.asarray(theta)[idx], xs)
        for i in range(len(xs)):
            if lik == pb.POISSON:
                term = (ys[i] * E.log(f[i]) - f[i]) + cst[i]
            else:
                q = (ys[i] - f[i]) / sg[i]
                term = cst[i] - q * q / 2
                if lik == pb.CUTOFF and term < -5000:
                    term = E.num(-5000)
            total += term
            scale += abs(float(term))
    return total, scale


# ---- problems placed at an offset ----------------------------------------------------------------
def roles(s):
    """what every parameter of the problem's vector is: 'A', 'mu', 'w', 'bg0', 'bg1', ..., 'shape'
    (eta, rho); peaks problems only"""
    r = [None] * s.d
    for model, shape, idx in s.fns:
        if model in (pb.GAUSS, pb.LORENTZ):
            nbg, npk = shape
            local = ["bg%d" % j for j in range(nbg)] + ["A", "mu", "w"] * npk
        elif model == pb.PVOIGT2:
            local = ["A", "bg0", "bg1", "mu", "w", "shape", "mu", "w", "shape", "shape", "bg2"]
        else:
            raise NotImplementedError("not a peaks model: %r" % (model,))
        for j, g in enumerate(idx):
            assert r[g] in (None, local[j])
            r[g] = local[j]
    return r


def _model_np(model, shape, p, x):
    return pb.pvoigt_eval(p, x) if model == pb.PVOIGT2 else pb.model_eval_np(model, shape, p, x)


def place(s, off, span):
    """a problems.py peaks problem built on x in [0, 1] (or any range: x -> off + span x), moved to
    x = off + span * x: centres and widths move along, amplitudes, sigmas and the noise stay, the
    background keeps its constant term only (a slope at an offset cancels in the reference's
    arithmetic as well and would blur what is measured), bounds are off (no prior).  Normal data:
    y keeps its residual against the model at theta*; Poisson counts stay (their rate does)"""
    r = roles(s)
    th = s.theta_star.copy()
    for j, g in enumerate(r):
        if g == "mu":
            th[j] = off + span * th[j]
        elif g == "w":
            th[j] = span * th[j]
        elif g.startswith("bg") and g != "bg0":
            th[j] = 0.0
    out = pb.Spec(s.d)
    for (model, shape, idx), (x, y, sig, lik) in zip(s.fns, s.data):
        xn = off + span * x
        if lik == pb.POISSON:
            assert shape[0] <= 1
            yn = y
        else:
            yn = (y - _model_np(model, shape, s.theta_star[idx], x)) + _model_np(model, shape, th[idx], xn)
        out.add(model, shape, idx, xn, yn, sig, lik, None)
    out.theta_star = th
    out.off, out.span = off, span
    return out


def perturbed(s, n=N_VECTORS, seed=11, d_mu=0.02, d_rel=0.10):
    """n vectors around theta*: centres moved ADDITIVELY by d_mu of the span (problems.perturbed
    multiplies: 1 % of 2000 is forty widths), widths, amplitudes and the constant background by
    d_rel of themselves, eta and rho by d_mu of themselves; background slopes stay exactly 0"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, s.d))
    th = np.tile(s.theta_star, (n, 1))
    for j, g in enumerate(roles(s)):
        if g == "mu":
            th[:, j] += d_mu * s.span * z[:, j]
        elif g in ("w", "A", "bg0"):
            th[:, j] *= 1.0 + d_rel * z[:, j]
        elif g == "shape":
            th[:, j] *= 1.0 + d_mu * z[:, j]
    return th


def two_peak_at(off, span, n, seed=1):
    return place(pb.two_peak(n=n, seed=seed, bounds=False), off, span)


@functools.lru_cache(maxsize=None)
def two_peak_case(off, span, n):
    """(spec, the 12 vectors, their high-precision log-posteriors, their sum |term|): computed once
    per process and shared; nobody changes them"""
    s = two_peak_at(off, span, n, seed=1000 + n)
    th = perturbed(s, seed=n)
    ref = [hp_logpost(s, t) for t in th]
    th.setflags(write=False)
    return s, th, [r[0] for r in ref], np.array([r[1] for r in ref])


WIDE = [(0.5, 0.6), (0.5, 0.6), (0.45, 0.7), (0.6, 0.5), (0.15, None), (None, 0.25)]


@functools.lru_cache(maxsize=None)
def two_peak_wide_case(off, span, n):
    """the same problem with six vectors whose peaks are WIDE, in units of the span: at n = 6000
    the recurrence takes a peak from 0.41 (a seed per window), 0.205 (two) and 0.1025 (four) on -
    S * 64 h iw <= 1, h = span / 5999 - so four vectors send both peaks and the background through
    it and two send one peak through a re-seeded class next to a direct one.  The 12 vectors of
    two_peak_case are the hard ones for the argument term (narrow peaks: steep flanks); these make
    sure the recurrence ran"""
    s = two_peak_case(off, span, n)[0]
    th = perturbed(s, n=len(WIDE), seed=n + 1)
    r = roles(s)
    for row, ws in zip(th, WIDE):
        for j, w in zip([j for j, g in enumerate(r) if g == "w"], ws):
            if w is not None:
                row[j] = w * span
    ref = [hp_logpost(s, t) for t in th]
    th.setflags(write=False)
    return s, th, [q[0] for q in ref], np.array([q[1] for q in ref])


@functools.lru_cache(maxsize=None)
def five_peak_case(off, span, n=1500):
    """config 3's problem (five Gaussians on a constant background, Poisson counts) placed at the
    offset: six perturbed vectors and two whose peaks 0, 2 and 4 are two spans wide - at n = 1500 a
    model of more than two peaks sends a peak through the recurrence from 32 * 64 h iw <= 1,
    w >= 1.64 span, on - next to direct ones.  (spec, vectors, high-precision log-posteriors,
    sum |term|), computed once"""
    s = place(pb.poisson_peaks(n=n, seed=n), off, span)
    th = perturbed(s, n=8, seed=n + 2)
    for j in (3, 9, 15):
        th[6:, j] = 2.0 * span * np.array([1.0, 1.07])
    ref = [hp_logpost(s, t) for t in th]
    th.setflags(write=False)
    return s, th, [q[0] for q in ref], np.array([q[1] for q in ref])


@functools.lru_cache(maxsize=None)
def pvoigt_case(off, span):
    """config 4's shape (three datasets sharing the pseudo-Voigt's shape parameters, x not a grid)
    placed at the offset, eight vectors: the same tuple"""
    s = place(pb.global_fit(n_each=400, n_sets=3, seed=3), off, span)
    th = perturbed(s, n=8, seed=17)
    ref = [hp_logpost(s, t) for t in th]
    th.setflags(write=False)
    return s, th, [q[0] for q in ref], np.array([q[1] for q in ref])


# ---- the argument term ---------------------------------------------------------------------------
def window_ulps(x):
    """per point: ulp of the max |x| of its 2048-point window (the grid rule's yardstick)"""
    x = np.asarray(x, float)
    out = np.empty_like(x)
    for i0 in range(0, len(x), WINDOW):
        w = x[i0:i0 + WINDOW]
        out[i0:i0 + WINDOW] = np.spacing(max(abs(w[0]), abs(w[-1])))
    return out


def grid_step(x):
    """h when x is one grid by mhx_set_dataset's rule, else 0"""
    x = np.asarray(x, float)
    if len(x) < 2:
        return 0.0
    h = (x[-1] - x[0]) / (len(x) - 1)
    tol = 8.0 * 2.0 ** -52 * max(abs(x[0]), abs(x[-1]))
    ok = h != 0.0 and bool((np.abs(x - (x[0] + np.arange(len(x)) * h)) <= tol).all())
    return h if ok else 0.0


def peaks_of(model, shape, p):
    """[(|weight|, mu, w, 'gauss' | 'lorentz')]: the peak-shaped terms of a model"""
    if model in (pb.GAUSS, pb.LORENTZ):
        nbg, npk = shape
        kind = "gauss" if model == pb.GAUSS else "lorentz"
        return [(abs(p[nbg + 3 * k]), p[nbg + 3 * k + 1], p[nbg + 3 * k + 2], kind) for k in range(npk)]
    if model == pb.PVOIGT2:
        A, _, _, mu1, w1, e1, mu2, w2, e2, rho, _ = p
        return [(abs(A * e1), mu1, w1, "lorentz"), (abs(A * (1 - e1)), mu1, w1, "gauss"),
                (abs(A * rho * e2), mu2, w2, "lorentz"), (abs(A * rho * (1 - e2)), mu2, w2, "gauss")]
    return []


def argument_term(model, shape, p, x, recurrence=False, grid_x=None, sweep=False):
    """SAFETY * sum_k |A_k| |dg_k/dx|(x) delta_k per point of x, float64.  recurrence: x is the
    dataset's own grid (grid_x defaults to it) and the peaks that the kernel advances by the
    recurrence - Gaussians of a model with a skipping rule whose width passes S * 64 h iw <= 1,
    S = 8 for at most two peaks (three seeding classes), else 32 - carry the grid's 8 ulp too.
    sweep: the log-posterior kernels' fast path instead of mhx_eval_function's guarded form - the
    same operations for the Gaussian and Lorentzian peaks; the pseudo-Voigt's Gaussians take
    t = fma(x, fl(iw g), fl(c g)), two roundings more: delta = (|x| + 2 |mu|) 2^-53"""
    x = np.asarray(x, float)
    total = np.zeros_like(x)
    pk = peaks_of(model, shape, p)
    h = grid_step(x if grid_x is None else grid_x) if recurrence and model == pb.GAUSS else 0.0
    ulps = window_ulps(x) if h != 0.0 else None
    for a, mu, w, kind in pk:
        u = (x - mu) / w
        with np.errstate(over="ignore", under="ignore"):
            if kind == "gauss":
                slope = 2.0 * np.abs(u) / abs(w) * np.exp(-u * u)
            else:
                slope = 2.0 * np.abs(u) / abs(w) / (1.0 + u * u) ** 2
        delta = abs(mu) * U53
        if sweep and model == pb.PVOIGT2 and kind == "gauss":
            delta = (np.abs(x) + 2.0 * abs(mu)) * U53
        if h != 0.0:
            period = 8 if len(pk) <= 2 else 32
            if period * 64.0 * abs(h) * SQRT_LOG2E / abs(w) <= 1.0 + 1e-9:
                delta = delta + 8.0 * ulps
        total = total + a * slope * delta
    return SAFETY * total


def sinusoid_term(p, x):
    """|A| (|om x| + |ph|) 2^-53 for the argument om x + ph, which the device may contract to one
    fma; SAFETY covers the form of two roundings"""
    return SAFETY * abs(p[0]) * (np.abs(p[1] * np.asarray(x, float)) + abs(p[2])) * U53


def expdecay_term(p, x):
    """x * fl(1 / tau) against x / tau: two roundings on the argument, |x / tau| 2^-52 relative on
    the exponential (derived from both roundings: no further factor)"""
    x = np.asarray(x, float)
    return abs(p[0]) * np.exp(-x / p[1]) * np.abs(x / p[1]) * 2.0 ** -52


def logpost_bound(s, theta, recurrence):
    """the argument term of the log-posterior: sum_i |d term_i / d f_i| * argument_term(x_i) with
    d term / d f = (y - f) / sigma^2 (normal), y / f - 1 (Poisson)"""
    total = 0.0
    for (model, shape, idx), (x, y, sig, lik) in zip(s.fns, s.data):
        p = np.asarray(theta)[idx]
        f = _model_np(model, shape, p, x)
        dterm = np.abs(y / f - 1.0) if lik == pb.POISSON else np.abs(y - f) / (sig * sig)
        total += float(np.sum(dterm * argument_term(model, shape, p, x, recurrence, sweep=True)))
    return total
