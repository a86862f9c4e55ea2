"""The reference's own fitting API over the MI355X engine.

Host-side mirror of the exported Lisp surface of afranson/Lisp-MCMC for the
walker-adaptive-steps path (M: = mcmc-fitting.lisp):

    walker-create                M:1132-1163   walker_create
    mcmc-fit                     M:1165-1175   mcmc_fit
    walker-adaptive-steps        M:946-947     walker_adaptive_steps
    walker-adaptive-steps-full   M:862-942     walker_adaptive_steps_full
    walker-many-steps            M:849-853     walker_many_steps
    walker-take-step             M:1072-1095   walker_take_step
    walker-get                   M:487-543     walker_get
    walker-set-get               M:1029-1030   walker_set_get
    walker-get-data-and-fit      M:1230-1255   walker_get_data_and_fit (+ _no_stddev M:1208-1227,
                                               walker_get_residuals M:1271-1283,
                                               walker_set_get_data_and_fit)
    walker-with-exp              M:1052-1064   walker_with_exp, walker_set_with_exp; its posterior
                                               walker_exp_get, walker_set_exp_get
    walker-param-histo           M:1361-1369   walker_param_histo (the two lists, no plot;
                                               make_histo / make_histo_x M:1541-1564),
                                               walker_set_param_histo
    walker-plot-corner           M:1333-1359   walker_set_corner_grid (pair counts on a grid)
    walker-modify                M:547-580     walker_modify
    prior-bounds-let             M:346-369     prior_bounds
    mfit-walker-estop            M:860-861     request_stop

Same names (kebab-case -> snake_case), same argument meaning, same error behaviour where
the path defines one.  All stepping and every log-posterior is computed by libmhx.so on
the GPU; this file only lays data out the way clean-data / clean-data-error do
(M:774-825) and turns device read-backs into the reference's return shapes.

Extension: n_chains > 1 makes a walker SET that steps in one batch (the reference maps a
list of walkers sequentially, M:1029-1033); `chain=` selects a member on read-back.
"""
from fractions import Fraction

import math
import warnings

import numpy as np

from . import _capi as capi
from .engine import Engine, hdi_span, split_rhat
from .models import Model

_LIKS = {
    None: capi.LIK_NORMAL,
    "normal": capi.LIK_NORMAL, "log-liklihood-normal": capi.LIK_NORMAL,
    "normal-weighted": capi.LIK_NORMAL, "log-liklihood-normal-weighted": capi.LIK_NORMAL,
    "normal-cutoff": capi.LIK_NORMAL_CUTOFF, "log-liklihood-normal-cutoff": capi.LIK_NORMAL_CUTOFF,
    "poisson": capi.LIK_POISSON, "log-poisson": capi.LIK_POISSON,
}


def _key(k):
    """:much-better-name -> much_better_name (the identifier used on both sides of the ABI)"""
    from .sexpr import mangle
    return mangle(str(k))


class WalkerStep:
    """(defstruct walker-step prob params) M:462-464; params is a {key: value} plist"""

    def __init__(self, prob, params):
        self.prob = float(prob)
        self.params = params

    def __repr__(self):
        return "#S(WALKER-STEP :PROB %r :PARAMS %r)" % (self.prob, self.params)


class PriorBounds:
    """The value of a prior whose body is `bounds-total` of (prior-bounds-let ((key lo hi) ...))"""

    def __init__(self, bounds, body=None):
        self.bounds = [(_key(k), float(lo), float(hi)) for k, (lo, hi) in dict(bounds).items()]
        self.body = body  # Lisp text of the prior-bounds-let body, None = bounds-total


def prior_bounds(bounds, body=None):
    """(prior-bounds-let ((:a lo hi) ...) BODY) M:346-369 as a log-prior designator.
    -1d10 (exp(1d-5 * distance) - 1) outside (lo, hi), strict at both ends; a key missing from
    the plist reads as 0d0 (M:353).  BODY is the Lisp text of the form's body and may use
    bounds-total and the parameter names, e.g. nv-specific.lisp:31-34's
    '(+ bounds-total (if (> mu1 mu2) -1e9 0e0))'; None means `bounds-total`."""
    return PriorBounds(bounds, body)


class LikelihoodExpr:
    """What (create-log-liklihood-function #'(lambda (y model error) ...)) returns, M:402-416"""

    def __init__(self, text):
        from . import sexpr
        self.text = text
        self.expr = sexpr.likelihood_lambda_to_expr(text)


def create_log_liklihood_function(text):
    """(create-log-liklihood-function log-liklihood-function) M:402-416 as a :log-liklihood
    designator.  TEXT is the Lisp text of the 3-argument closure, e.g.
    '(lambda (y model error) (declare (ignore error)) (- (* y (log model)) model))'; the
    log-likelihood is the sum of its values over the points.  `error` is the point's sigma (the
    docstring's meaning; the reference's code hands every call the whole stddev list).  The
    function the walker fits must then be an expression model (models.lisp / models.expr)."""
    return LikelihoodExpr(text)


log_prior_flat = None  # (log-prior-flat params data) => 0d0, M:340-343


def _force_list(item):  # M:755-759
    return list(item) if isinstance(item, (list, tuple)) else [item]


def _depth(t):  # get-depth M:761-772
    if isinstance(t, (int, float, np.floating, np.integer)):
        return 0
    if isinstance(t, np.ndarray):
        return t.ndim
    return 1 + _depth(t[0])


def _vector_x(ds):
    """a dataset [X, y] whose x elements are vectors - "multiple or linked independent variables",
    M:1136-1137: X [n][2] (one row per point), y [n]"""
    try:
        return (len(ds) == 2 and np.ndim(ds[0]) == 2 and np.ndim(ds[1]) == 1
                and np.shape(ds[0])[0] == np.shape(ds[1])[0] and np.shape(ds[0])[1] in (1, 2)
                and np.shape(ds[0])[0] != 2)
    except (TypeError, ValueError):
        return False


def _clean_data(data, n_fn):  # M:807-825
    if _vector_x(data):
        return _clean_data([data], n_fn)
    if len(data) == n_fn and all(_vector_x(ds) for ds in data):
        return [[np.asarray(ds[0], dtype=np.float64), np.asarray(ds[1], dtype=np.float64)] for ds in data]
    dep = _depth(data)
    if dep == 1:
        raise ValueError("clean-data: data is of insufficient depth or improperly structured.")
    if dep == 2:
        return _clean_data([data], n_fn)
    if len(data) == n_fn:
        return [[np.asarray(col, dtype=np.float64) for col in ds] for ds in data]
    raise ValueError("clean-data: insufficient number of datasets, %d, for the given number of "
                     "functions, %d." % (len(data), n_fn))


def _clean_data_error(stddev, ys):
    """clean-data-error M:774-805 for the layouts the path uses: a number broadcasts to every
    y; a structure equal to the y structure is taken as is; anything else broadcasts its
    first element."""
    def first(t):
        while not isinstance(t, (int, float, np.floating, np.integer)):
            t = t[0]
        return float(t)
    if isinstance(stddev, (int, float, np.floating, np.integer)):
        return [np.full(y.shape, float(stddev)) for y in ys]
    sd = _force_list(stddev)
    if len(sd) == len(ys) and all(
            not isinstance(s, (int, float, np.floating, np.integer)) and len(s) == len(y)
            for s, y in zip(sd, ys)):
        return [np.asarray(s, dtype=np.float64) for s in sd]
    if len(ys) == 1 and len(sd) == len(ys[0]) and all(
            isinstance(s, (int, float, np.floating, np.integer)) for s in sd):
        return [np.asarray(sd, dtype=np.float64)]
    return [np.full(y.shape, first(stddev)) for y in ys]


def _plist(params):
    """(:b -1 :m 2) / {'b': -1, 'm': 2} -> keys in plist order (plist-keys M:190-193), values"""
    if isinstance(params, dict):
        items = list(params.items())
    else:
        p = list(params)
        if len(p) % 2:
            raise ValueError("params plist must have an even number of elements")
        items = [(p[i], p[i + 1]) for i in range(0, len(p), 2)]
    keys, vals = [], []
    for k, v in items:
        k = _key(k)
        if k in keys:
            continue  # first value wins, like getf (M:195-198)
        if not isinstance(v, (int, float, np.floating, np.integer)):
            # :single-item styles (M:7-14, M:1153-1155): one key holding a list / vector /
            # d x 1 array; expanded to key_0, key_1, ... (what (elt key i) translates to)
            flat = np.asarray(v, dtype=np.float64).reshape(-1)
            for i, vi in enumerate(flat):
                keys.append("%s_%d" % (k, i))
                vals.append(float(vi))
            continue
        keys.append(k)
        vals.append(float(v))
    return keys, np.asarray(vals, dtype=np.float64)


class Walker:
    """(defstruct walker ...) M:467-479 backed by device state."""

    def __init__(self, engine, function, param_keys, data, data_error, log_liklihood, log_prior):
        self.engine = engine
        self.function = function
        self.param_keys = param_keys
        self.param_style = ":multiple-kwargs"
        self.data = data
        self.data_error = data_error
        self.log_liklihood = log_liklihood
        self.log_prior = log_prior
        self.n_chains = engine.n_chains
        # walker_set_create: {"y": [n_chains][n], "sigma": [n_chains][n]} of function 0, whose
        # self.data / self.data_error hold walker 0's; None: every walker fits self.data
        self.planes = None

    def data_of(self, fn_number=0, chain=0):
        """the dataset [x, y] function fn_number of walker `chain` fits"""
        data = self.data[fn_number]
        if self.planes is not None and fn_number == 0:
            return [data[0], self.planes["y"][chain]]
        return data

    def data_error_of(self, fn_number=0, chain=0):
        """... and its stddev per point"""
        if self.planes is not None and fn_number == 0:
            return self.planes["sigma"][chain]
        return self.data_error[fn_number]

    # struct accessors (exported M:480)
    def _step(self, th, pr):
        return WalkerStep(pr, dict(zip(self.param_keys, (float(v) for v in th))))

    def last_step(self, chain=0):
        s = self.engine.state()
        return self._step(s["theta"][chain], s["logpost"][chain])

    def most_likely_step(self, chain=0):
        s = self.engine.state()
        return self._step(s["best_theta"][chain], s["best_logpost"][chain])

    def length(self, chain=0):
        return int(self.engine.state()["length"][chain])

    def age(self, chain=0):
        return int(self.engine.state()["age"][chain])

    def walk(self, chain=0, take=None):
        return walker_get(self, get=":steps", take=take, chain=chain)

    def status(self):
        return self.engine.chain_status()[0]

    def _raise_on_trap(self):
        st = self.status()
        if (st == capi.CHAIN_FP_TRAP).any():
            bad = np.flatnonzero(st == capi.CHAIN_FP_TRAP)
            raise FloatingPointError(
                "walker(s) %s: the reference would have signalled an unhandled floating-point "
                "trap here (non-finite log-posterior, or 0/0 in cholesky-decomp M:597); the "
                "walker is left where it stood" % bad[:8].tolist())


def walker_create(function=None, data=None, params=None, data_error=None, log_liklihood=None,
                  log_prior=None, param_bounds=None, n_chains=1, theta0=None, device=0, seed=0,
                  chain_offset=0, history_capacity=0, adapt_mode=capi.ADAPT_FAITHFUL,
                  poisson_logfact_double=False):
    """(walker-create &key function data params data-error log-liklihood log-prior param-bounds)
    M:1132-1163.  function: a models.Model or a list of them; everything else as the reference:
    each argument may be one item or a list with one item per function (global fit)."""
    del param_bounds  # (declare (ignorable param-bounds)) M:1141
    fns = _force_list(function)
    if not all(isinstance(f, Model) for f in fns):
        raise TypeError(":function must be a model designator (lisp_mcmc_amd.models), see "
                        "INTEGRATION.md: a Lisp/Python closure cannot run on the GPU")
    K = len(fns)
    dsets = _clean_data(data, K)
    ys = [ds[1] for ds in dsets]
    sig = _clean_data_error(1 if data_error is None else data_error, ys)
    keys, vals = _plist(params)
    liks = _force_list(log_liklihood) if isinstance(log_liklihood, (list, tuple)) else [log_liklihood] * K
    pris = _force_list(log_prior) if isinstance(log_prior, (list, tuple)) else [log_prior] * K
    if len(liks) != K or len(pris) != K:
        raise ValueError("one log-liklihood / log-prior per function")
    eng = Engine(n_chains, len(keys), K, device=device, seed=seed, chain_offset=chain_offset,
                 adapt_mode=adapt_mode, history_capacity=history_capacity,
                 poisson_logfact_double=poisson_logfact_double)
    if any(getattr(f, "as_written", False) for f in fns):
        eng.set_expr_recognition(False)
    for k, f in enumerate(fns):
        missing = [q for q in f.keys if q not in keys]
        if missing:
            raise KeyError("function %d reads keys %s that :params does not supply" % (k, missing))
        if f.model_id == capi.MODEL_EXPR:
            eng.set_function_expr(k, f.expr, f.keys, [keys.index(q) for q in f.keys])
        else:
            eng.set_function(k, f.model_id, f.shape, [keys.index(q) for q in f.keys])
        lk = liks[k]
        if isinstance(lk, LikelihoodExpr):
            eng.set_dataset(k, dsets[k][0], dsets[k][1], sig[k], capi.LIK_EXPR)
            eng.set_likelihood_expr(k, lk.expr)
        else:
            if isinstance(lk, str):
                lk = lk.lstrip("#':").lower()
            if lk not in _LIKS:
                raise capi.MhxError(capi.EUNSUPPORTED, "unknown :log-liklihood %r" % (liks[k],))
            eng.set_dataset(k, dsets[k][0], dsets[k][1], sig[k], _LIKS[lk])
        pr = pris[k]
        if pr is None:
            eng.set_bounds(k, [], [], [])
        elif isinstance(pr, PriorBounds):
            eng.set_bounds(k, [keys.index(q) if q in keys else -1 for q, _, _ in pr.bounds],
                           [lo for _, lo, _ in pr.bounds], [hi for _, _, hi in pr.bounds])
            if pr.body:
                from . import sexpr
                eng.set_prior_expr(k, sexpr.prior_body_to_expr(pr.body), keys, range(len(keys)))
        else:
            raise capi.MhxError(capi.EUNSUPPORTED,
                                ":log-prior must be None (log-prior-flat) or prior_bounds(...)")
    eng.init_chains(vals if theta0 is None else np.asarray(theta0, dtype=np.float64))
    w = Walker(eng, fns, keys, dsets, sig, liks, pris)
    w._raise_on_trap()
    return w


def data_separated(columns):
    """nv-data->separated (nv-specific.lisp:5-6): the columns of one file, x first, as one
    dataset [x, y] per remaining column"""
    cols = list(columns)
    return [[cols[0], c] for c in cols[1:]]


def _is_number(v):
    return isinstance(v, (int, float, np.floating, np.integer))


def planes_layout(datasets, params, data_error=None):
    """The arrays of a walker set with one dataset per walker (Engine.set_dataset_planes), from what
    walker_set_create is given; no engine, no device.
      datasets    a list of [x, y], one per walker; every x equal bit for bit (ValueError names
                  the first walker whose x differs)
      params      one plist for all walkers, or a list of one plist per walker with the same keys
                  in the same order
      data_error  None (SIGMA_NONE), one number (SIGMA_PER_CHAIN, the same for every walker), one
                  number per walker (SIGMA_PER_CHAIN), one list per point (SIGMA_SHARED), or one
                  list per point per walker (SIGMA_PER_POINT).  A list of numbers as long as the
                  walkers is taken per walker (nv-data-std-dev) even when the points are as many.
    Returns a dict: x [n], y [C][n], sigma (None or the array of its kind), sigma_kind, keys,
    theta0 [C][d] and sigma_rows [C][n] (every walker's stddev per point, for the read-outs)."""
    dsets = [list(ds) for ds in datasets]
    if not dsets or any(len(ds) != 2 for ds in dsets):
        raise ValueError("datasets must be a non-empty list of [x, y], one per walker")
    C_ = len(dsets)
    x = np.ascontiguousarray(dsets[0][0], dtype=np.float64)
    if x.ndim != 1 or x.size == 0:
        raise ValueError("x must be one column of at least one point")
    y = np.empty((C_, x.size))
    for c, (xc, yc) in enumerate(dsets):
        xc = np.ascontiguousarray(xc, dtype=np.float64)
        if xc.shape != x.shape or xc.tobytes() != x.tobytes():
            raise ValueError("walker %d: its x differs from walker 0's (a walker set shares one x)" % c)
        yc = np.asarray(yc, dtype=np.float64)
        if yc.shape != x.shape:
            raise ValueError("walker %d: y must be as long as x" % c)
        y[c] = yc
    n = x.size
    if data_error is None:
        kind, sigma, rows = capi.SIGMA_NONE, None, np.ones((C_, n))
    elif _is_number(data_error):
        kind, sigma = capi.SIGMA_PER_CHAIN, np.full(C_, float(data_error))
        rows = np.full((C_, n), float(data_error))
    else:
        de = list(data_error)
        if len(de) == C_ and all(_is_number(v) for v in de):
            kind, sigma = capi.SIGMA_PER_CHAIN, np.asarray(de, dtype=np.float64)
            rows = np.repeat(sigma[:, None], n, axis=1)
        elif len(de) == n and all(_is_number(v) for v in de):
            kind, sigma = capi.SIGMA_SHARED, np.asarray(de, dtype=np.float64)
            rows = np.repeat(sigma[None, :], C_, axis=0)
        elif len(de) == C_ and all(not _is_number(v) and len(v) == n for v in de):
            kind, sigma = capi.SIGMA_PER_POINT, np.ascontiguousarray(de, dtype=np.float64)
            rows = sigma
        else:
            raise ValueError("data_error must be None, a number, one number per walker, one list "
                             "per point, or one list per point per walker")
    if isinstance(params, dict) or (len(params) and isinstance(list(params)[0], str)):
        keys, vals = _plist(params)
        theta0 = np.repeat(vals[None, :], C_, axis=0)
    else:
        pl = [_plist(q) for q in params]
        if len(pl) != C_:
            raise ValueError("params: one plist, or one per walker (%d given for %d walkers)" % (len(pl), C_))
        keys = pl[0][0]
        for c, (kc, _) in enumerate(pl):
            if kc != keys:
                raise ValueError("walker %d: its params have other keys, or another order, than walker 0's" % c)
        theta0 = np.array([v for _, v in pl], dtype=np.float64)
    return {"x": x, "y": y, "sigma": sigma, "sigma_kind": kind, "keys": keys, "theta0": theta0,
            "sigma_rows": rows}


def walker_set_create(function=None, datasets=None, params=None, data_error=None, log_prior=None,
                      log_liklihood=None, device=0, seed=0, chain_offset=0, history_capacity=0):
    """A walker set in which every walker fits a dataset of its own over a shared x - what
    nv-specific.lisp:50-66 builds one walker at a time (file->nv-walkers): `datasets` as
    data_separated returns them, one starting guess for all or one per walker, one stddev for all
    or one per walker.  ONE function, the normal likelihood (#'log-liklihood-normal or None).  The
    result is an ordinary Walker of len(datasets) chains that walk in one launch: walker c does what
    a single walker on dataset c would do with chain_id c."""
    if isinstance(function, (list, tuple)):
        if len(function) != 1:
            raise capi.MhxError(capi.EUNSUPPORTED, "walker_set_create takes one function")
        function = function[0]
    if not isinstance(function, Model):
        raise TypeError(":function must be a model designator (lisp_mcmc_amd.models)")
    lk = log_liklihood.lstrip("#':").lower() if isinstance(log_liklihood, str) else log_liklihood
    if lk not in _LIKS or _LIKS[lk] != capi.LIK_NORMAL:
        raise capi.MhxError(capi.EUNSUPPORTED, "walker_set_create: a dataset per walker takes the "
                            "normal likelihood only, not %r" % (log_liklihood,))
    lay = planes_layout(datasets, params, data_error)
    keys, f = lay["keys"], function
    missing = [q for q in f.keys if q not in keys]
    if missing:
        raise KeyError("the function reads keys %s that :params does not supply" % (missing,))
    eng = Engine(len(lay["y"]), len(keys), 1, device=device, seed=seed, chain_offset=chain_offset,
                 history_capacity=history_capacity)
    if getattr(f, "as_written", False):
        eng.set_expr_recognition(False)
    if f.model_id == capi.MODEL_EXPR:
        eng.set_function_expr(0, f.expr, f.keys, [keys.index(q) for q in f.keys])
    else:
        eng.set_function(0, f.model_id, f.shape, [keys.index(q) for q in f.keys])
    eng.set_dataset_planes(0, lay["x"], lay["y"], lay["sigma"], lay["sigma_kind"])
    if log_prior is None:
        eng.set_bounds(0, [], [], [])
    elif isinstance(log_prior, PriorBounds):
        pr = log_prior
        eng.set_bounds(0, [keys.index(q) if q in keys else -1 for q, _, _ in pr.bounds],
                       [lo for _, lo, _ in pr.bounds], [hi for _, _, hi in pr.bounds])
        if pr.body:
            from . import sexpr
            eng.set_prior_expr(0, sexpr.prior_body_to_expr(pr.body), keys, range(len(keys)))
    else:
        raise capi.MhxError(capi.EUNSUPPORTED,
                            ":log-prior must be None (log-prior-flat) or prior_bounds(...)")
    eng.init_chains(lay["theta0"])
    w = Walker(eng, [f], keys, [[lay["x"], lay["y"][0]]], [lay["sigma_rows"][0]], [log_liklihood],
               [log_prior])
    w.planes = {"y": lay["y"], "sigma": lay["sigma_rows"]}
    w._raise_on_trap()
    return w


def walker_adaptive_steps_full(walker, n=100000, temperature=1e3, auto=":prob-settle",
                               sampling_optimization=":covariance", max_walker_length=None,
                               l_matrix=None):
    """(walker-adaptive-steps-full walker &key n temperature auto sampling-optimization
    max-walker-length l-matrix) M:862"""
    if sampling_optimization not in (":covariance", "covariance"):
        raise capi.MhxError(capi.EUNSUPPORTED, ":best-value is outside the accelerated path")
    if auto in (":slope-settle", "slope-settle"):
        raise capi.MhxError(capi.EUNSUPPORTED, ":slope-settle is outside the accelerated path")
    walker.engine.adaptive_steps_full(int(np.floor(n)), temperature, 1 if auto else 0,
                                      max_walker_length or 0, l_matrix)
    walker._raise_on_trap()
    return None


def walker_adaptive_steps(walker, n=30000):
    """(walker-adaptive-steps walker &optional (n 30000)) M:946-947"""
    return walker_adaptive_steps_full(walker, n=n, temperature=10, auto=":prob-settle")


def mcmc_fit(**kw):
    """(mcmc-fit &key ...) = walker-create + walker-adaptive-steps M:1165-1175"""
    w = walker_create(**kw)
    walker_adaptive_steps(w)
    return w


def walker_many_steps(walker, n, l_matrix=None):
    """(walker-many-steps the-walker n &optional l-matrix) M:849-853"""
    if l_matrix is None:  # M:851 diag(1e-2 (single float!) * median-params)
        med = walker_get(walker, get=":median-params")
        l_matrix = np.diag([float(np.float32(1e-2)) * v for v in med.values()])
    walker.engine.many_steps(n, l_matrix)
    walker._raise_on_trap()


def walker_take_step(walker, l_matrix=None, temperature=1, z=None, u=None, rng=None):
    """(walker-take-step walker &key l-matrix (temperature 1)) M:1072-1095.  z / u are the
    numbers alexandria:gaussian-random (M:687) and (random 1.0d0) (M:1092) would return
    (the parity hook, mhx_step_injected); when all are omitted the device draws its own
    (mhx_take_step), as the reference does."""
    e = walker.engine
    if l_matrix is None:  # M:1074
        ml = walker_get(walker, get=":most-likely-params", take=1000)
        l_matrix = np.diag([float(np.float32(1e-2)) * v for v in ml.values()])
    if z is None and u is None and rng is None:
        # the reference draws its own randomness (M:687, M:1092): so does the device (Philox,
        # the chain's next draw) - mhx_take_step
        e.take_step(l_matrix, temperature)
        walker._raise_on_trap()
        return None
    rng = rng or np.random.default_rng()
    if z is None:
        z = rng.standard_normal((e.n_chains, e.d))
    if u is None:
        u = 1.0 - rng.random(e.n_chains)
    acc = e.step_injected(l_matrix, z, u, temperature)
    walker._raise_on_trap()
    return acc


def request_stop(walker):
    """(setf mfit-walker-estop t) M:860-861"""
    walker.engine.request_stop()


def _percentile(n, seq):  # nth-percentile M:1493-1504
    copy = np.sort(np.asarray(seq, dtype=np.float64))
    pos = Fraction(n).limit_denominator(1000) * (len(copy) - 1) / 100
    lo = pos.numerator // pos.denominator
    if pos == lo:
        return float(copy[lo])
    return float((copy[lo] + copy[lo + 1]) / 2)


class HistoryTruncated(UserWarning):
    """walker-get was asked about more steps than the device history ring still holds"""


def lplist_covariance(v):
    """lplist-covariance M:614-643 of N parameter vectors [N, d], in the reference's own order of
    operations: averages (/ (reduce #'+ x) N) M:626, then per entry the serial sum over the points
    of (/ (* a_ik a_jk) N) M:636-643 - the division inside the sum.  np.cumsum accumulates strictly
    left to right (np.sum adds pairwise), so the result has the reference's bits."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    n, d = v.shape
    avg = np.cumsum(v, axis=0)[-1] / n
    an = v - avg
    cov = np.empty((d, d))
    for i in range(d):
        for j in range(d):
            cov[i, j] = np.cumsum((an[:, i] * an[:, j]) / n)[-1]
    return cov


def _l_matrix_value(st, L):
    """the value or condition of (walker-get :l-matrix) for a status of the device's ring_l_matrix"""
    if st == capi.L_CAUGHT:
        raise ArithmeticError("(walker-get :l-matrix): type-error / division-by-zero / "
                              "floating-point-overflow (the conditions M:891-894 handles)")
    if st == capi.L_INVALID:
        raise FloatingPointError("(walker-get :l-matrix): floating-point-invalid-operation")
    return L if st == capi.L_OK else np.zeros((0, 0))


_LIST_SELECTORS = ("steps", "log-liklihoods", "params", "param", "unique-steps", "forward-steps")


def _list_selector(g, steps, prob, param):
    """the list-valued selectors of M:487-543 over a window's newest-first steps"""
    if g == "steps":
        return steps
    if g == "log-liklihoods":  # M:540
        return [s.prob for s in steps]
    if g == "params":
        return [s.params for s in steps]
    if g == "param":
        return [s.params[_key(param)] for s in steps]
    if g == "unique-steps":  # M:492-496: `equal` on two double-floats is eql - the same BITS
        bits = np.asarray(prob, dtype=np.float64).view(np.uint64)  # (0.0 / -0.0 differ, NaN = NaN)
        return [steps[i].params for i in range(len(steps))
                if i + 1 >= len(steps) or bits[i] != bits[i + 1]]
    # "forward-steps", M:497-502
    return [steps[i].params for i in range(len(steps) - 1)
            if not steps[i].prob <= steps[i + 1].prob]


def walker_get(walker, get=":steps", take=None, param=None, chain=0):
    """(walker-get walker &key get take param) M:487-543, served from the device trace."""
    e = walker.engine
    g = str(get).lstrip(":").lower()
    keys = walker.param_keys
    cap = int(e.state()["length"][chain])
    t = cap if take is None else min(int(take), cap)
    if g == "most-likely-params":  # M:511-515 (struct slot, not windowed)
        return dict(walker.most_likely_step(chain).params)
    if g == "acceptance":  # M:506-508
        a = e.acceptance(max(t, 1))[chain]
        return Fraction(int(round(a * t)), t)
    if g == "l-matrix":  # M:543
        st, L, _ = e.proposal_factor(chain, max(t, 1))
        return _l_matrix_value(st, L)
    prob, th = e.trace(chain, t)
    if len(prob) < t:
        # the reference keeps every step of a walk (M:549); the engine keeps the newest
        # history_capacity in its device ring.  A window that reaches past the ring is answered
        # with what is there - and says so, instead of silently being about a shorter walk.
        warnings.warn(HistoryTruncated(
            "walker-get %s :take %d: the device history ring holds the newest %d of the walk's %d "
            "steps; create the walker with history_capacity >= the walk's length to keep them all"
            % (get, t, len(prob), cap)), stacklevel=2)
    steps = [walker._step(th[i], prob[i]) for i in range(len(prob))]
    if g in _LIST_SELECTORS:
        return _list_selector(g, steps, prob, param)
    if g == "most-likely-step":  # M:503-505 over the window; ties keep the later element
        best = steps[0]
        for s in steps[1:]:
            best = best if best.prob > s.prob else s
        return best
    if g == "median-params":  # M:516-523
        return {k: _percentile(50, th[:, j]) for j, k in enumerate(keys)}
    if g == "covariance-matrix":  # M:541: (lplist-covariance unique-steps)
        u = np.array([[p[k] for k in keys] for p in walker_get(walker, ":unique-steps", take, chain=chain)])
        return lplist_covariance(u)
    if g == "stddev-params":  # M:525-539 diagonal of the l-matrix
        if cap < 10:
            return {k: 0.0 for k in keys}
        L = walker_get(walker, ":l-matrix", take, chain=chain)
        return {k: float(L[j, j]) for j, k in enumerate(keys)}
    raise ValueError("unknown :get %r" % (get,))


_SUMMARY_SELECTORS = ("median-params", "stddev-params", "l-matrix", "covariance-matrix",
                      "most-likely-step", "most-likely-params", "acceptance")


def walker_set_get(walker, get=":steps", take=None, param=None):
    """(walker-set-get the-walker-set &key get take param) M:1029-1030: walker-get mapped over
    the set - a list with one entry per chain, each what walker_get(..., chain=c) returns.

    The summarising selectors (:median-params :stddev-params :l-matrix :covariance-matrix
    :most-likely-step :most-likely-params :acceptance) are served by ONE batched device call for
    all chains (include/mhx.h, mhx_get_percentiles and its kin): no history crosses to the host.
    The list-valued selectors (:steps :params :param :log-liklihoods :unique-steps :forward-steps)
    take ONE mhx_get_traces call for the set: the device filters, and only the columns the
    selector reads come back.  A condition is raised
    for the first chain (in chain order) that walker_get would raise it for, as mapcar would;
    HistoryTruncated is warned once per call when any chain's window reached past its ring."""
    e = walker.engine
    g = str(get).lstrip(":").lower()
    if g not in _SUMMARY_SELECTORS and g not in _LIST_SELECTORS:
        raise ValueError("unknown :get %r" % (get,))
    keys = walker.param_keys
    n = e.n_chains
    state = e.state()  # every chain's length (and most likely step): read ONCE
    cap = state["length"].astype(np.int64)
    t = cap.copy() if take is None else np.minimum(int(take), cap)
    if g == "most-likely-params":  # M:511-515 (struct slot, not windowed)
        return [dict(zip(keys, (float(v) for v in state["best_theta"][c]))) for c in range(n)]
    ring = e.history_capacity()
    widest = max(int(t.max()), 1)

    def truncated(held, wanted, count):
        warnings.warn(HistoryTruncated(
            "walker-set-get %s :take %s: the device history ring holds the newest %d steps of a "
            "walk and %d of the set's %d windows reach past it (the widest asks for %d); create the "
            "walker with history_capacity >= the walks' length to keep them all"
            % (get, take, held, count, n, wanted)), stacklevel=3)

    if g in ("acceptance", "l-matrix", "stddev-params"):
        if widest > ring:
            # walker_get hands such a window to the device, which refuses it: the chain that
            # asks for it raises (unless an earlier chain raises first) - in walker_get's words
            return [walker_get(walker, get, take, param, chain=c) for c in range(n)]
        if g == "acceptance":  # M:506-508
            a = e.acceptance(widest)
            return [Fraction(int(round(a[c] * int(t[c]))), int(t[c])) for c in range(n)]
        st, L, _ = e.proposal_factors(widest)
        out = []
        for c in range(n):
            if g == "stddev-params" and cap[c] < 10:  # M:528-529
                out.append({k: 0.0 for k in keys})
                continue
            Lc = _l_matrix_value(int(st[c]), L[c].copy())
            out.append(Lc if g == "l-matrix" else {k: float(Lc[j, j]) for j, k in enumerate(keys)})
        return out
    past = int((t > ring).sum())
    window = min(widest, ring)
    if g == "median-params":  # M:516-523
        med, _ = e.percentiles(window, [(50, 1)])
        if past:
            truncated(ring, widest, past)
        return [{k: float(med[c, 0, j]) for j, k in enumerate(keys)} for c in range(n)]
    if g == "covariance-matrix":  # M:541
        cov, _, _ = e.covariances(window)
        if past:
            truncated(ring, widest, past)
        return [cov[c].copy() for c in range(n)]
    if g == "most-likely-step":  # M:503-505 over the window
        pr, th = e.window_best(window)
        if past:
            truncated(ring, widest, past)
        return [walker._step(th[c], pr[c]) for c in range(n)]
    if take is not None and int(take) < 1:  # (no window the device could be asked for)
        out, short = [], 0
        for c in range(n):
            prob, th = e.trace(c, int(t[c]))
            short += len(prob) < t[c]
            steps = [walker._step(th[i], prob[i]) for i in range(len(prob))]
            out.append(_list_selector(g, steps, prob, param))
        if short:
            truncated(ring, widest, short)
        return out
    # ONE device call for the whole set: the selector's filter, only the columns it reads
    every = list(range(len(keys)))
    if g == "param":
        k = _key(param)
        cols = [list(keys).index(k)] if k in keys else [capi.TRACE_PROB]
    else:
        cols = {"steps": [capi.TRACE_PROB] + every, "log-liklihoods": [capi.TRACE_PROB]}.get(g, every)
    r = e.traces(window, cols, filter={"unique-steps": "unique", "forward-steps": "forward"}.get(g, "steps"))
    short = int((r["n_used"] < t).sum())
    if short:
        truncated(ring, widest, short)
    out = []
    for c in range(n):
        rows = r["values"][c, :int(r["n_out"][c])]
        if g == "steps":
            out.append([walker._step(v[1:], v[0]) for v in rows])
        elif g == "log-liklihoods":  # M:540
            out.append(rows[:, 0].tolist())
        elif g == "param":
            if k not in keys and len(rows):
                raise KeyError(k)  # (what the first step's plist answers in walker_get)
            out.append(rows[:, 0].tolist())
        else:  # :params, :unique-steps M:492-496, :forward-steps M:497-502
            out.append([dict(zip(keys, v.tolist())) for v in rows])
    return out


def fit_linspace(lo, hi, n=1000):
    """(linspace lo hi :len n) M:235-248: exact rationals from the double `hi - lo`, coerced to
    double at the end"""
    lo, hi = float(lo), float(hi)
    step = Fraction(hi - lo) / (n - 1)
    start = Fraction(lo)
    return np.array([float(start + i * step) for i in range(n)])


def _fit_inputs(walker, take, x_column, y_column, fn_number, chain=0):
    """what M:1232-1241 binds: the data columns and x-fit of one function (of walker `chain`)"""
    data = walker.data_of(fn_number, chain)
    x_data = np.asarray(data[x_column], dtype=np.float64)
    y_data = np.asarray(data[y_column], dtype=np.float64)
    if x_data.ndim != 1:
        raise capi.MhxError(capi.EUNSUPPORTED, "walker-get-data-and-fit draws one column of x: "
                            "a vector-valued x has no min and max (use Engine.eval_function)")
    return x_data, y_data, fit_linspace(x_data.min(), x_data.max())


def _fit_solution(walker, which_solution, take, chains=None):
    """M:1243-1246 for every chain (chains None) or one: the parameter plists and their vectors"""
    get = ":most-likely-step" if str(which_solution).lstrip(":").lower() == "most-likely" \
        else ":median-params"
    if chains is None:
        sol = walker_set_get(walker, get, take)
    else:
        sol = [walker_get(walker, get, take, chain=chains)]
    plists = [dict(s.params) if isinstance(s, WalkerStep) else s for s in sol]
    th = np.array([[p[k] for k in walker.param_keys] for p in plists], dtype=np.float64)
    return plists, th


def _shift(v, by):
    return list(v) if by is None else [by + float(a) for a in v]


def _band_take(walker, take, lengths, who):
    """the window the ring can serve, with walker_get's warning when the walk is longer"""
    ring = walker.engine.history_capacity()
    if int(lengths.max()) > ring:
        warnings.warn(HistoryTruncated(
            "%s :take %s: the device history ring holds the newest %d of the walk's %d steps; "
            "create the walker with history_capacity >= the walk's length to keep them all"
            % (who, take, ring, int(lengths.max()))), stacklevel=3)
    return min(max(int(take), 1), ring)


def walker_get_data_and_fit_no_stddev(walker, take=1000, x_column=0, y_column=1, fn_number=0,
                                      which_solution=":most-likely", x_shift=None, y_shift=None,
                                      chain=0):
    """(walker-get-data-and-fit-no-stddev walker &key take x-column y-column fn-number
    which-solution x-shift y-shift) M:1208-1227 -> [x_fit, y_fit, x_data, y_data, params]; the
    model is evaluated by the device's own code (mhx_eval_function)."""
    cap = walker.length(chain)
    take = cap if take is None or take > cap else int(take)
    x_data, y_data, x_fit = _fit_inputs(walker, take, x_column, y_column, fn_number, chain)
    plists, th = _fit_solution(walker, which_solution, take, chain)
    y_fit = walker.engine.eval_function(fn_number, th[0], x_fit)
    return [_shift(x_fit, x_shift), _shift(y_fit, y_shift), _shift(x_data, x_shift),
            _shift(y_data, y_shift), plists[0]]


def _data_and_fit(walker, take, x_column, y_column, fn_number, which_solution, x_shift, y_shift,
                  chains, who):
    e = walker.engine
    lengths = e.state()["length"].astype(np.int64)
    x_data, y_data, x_fit = _fit_inputs(walker, take, x_column, y_column, fn_number)
    big = int(lengths.max()) if take is None else int(take)
    # (every chain clamps `take` to its own length, M:1232-1234: on the device for the band, in
    # walker_get / walker_set_get for the solution)
    which = range(e.n_chains) if chains is None else [chains]
    ymax, ymin, _, status = e.fit_bands(
        fn_number, _band_take(walker, big, lengths[list(which)], who), x_fit)
    bad = [c for c in which if status[c]]
    if bad:
        raise FloatingPointError(
            "%s: the model is not finite at a step of walker(s) %s: the reference would have "
            "signalled a floating-point trap here" % (who, bad[:8]))
    plists, th = _fit_solution(walker, which_solution, take, chains)
    y_fit = e.eval_function(fn_number, th, x_fit)
    ys = 0 if y_shift is None else y_shift  # (+ (if y-shift y-shift 0) ...) M:1252-1253
    out = []
    for i, c in enumerate(which):
        if walker.planes is not None:  # (a dataset per walker: walker c's own columns)
            x_data, y_data, _ = _fit_inputs(walker, take, x_column, y_column, fn_number, c)
        out.append([_shift(x_fit, x_shift), [ys + float(v) for v in ymax[c]],
                    [ys + float(v) for v in ymin[c]], _shift(y_fit[i], y_shift),
                    _shift(x_data, x_shift), _shift(y_data, y_shift), plists[i]])
    return out


def walker_get_data_and_fit(walker, take=1000, x_column=0, y_column=1, fn_number=0,
                            which_solution=":most-likely", x_shift=None, y_shift=None, chain=0):
    """(walker-get-data-and-fit walker &key take x-column y-column fn-number which-solution
    x-shift y-shift) M:1230-1255 -> [x_fit, max_ys, min_ys, y_fit, x_data, y_data, params]:
    the fit on 1000 points between the data's least and greatest x and the envelope of the model
    over the ceiling(0.66 take) most probable steps of the walk, both computed on the device
    (mhx_get_fit_bands, mhx_eval_function).  Raises FloatingPointError where the reference would
    have trapped on a non-finite model value."""
    return _data_and_fit(walker, take, x_column, y_column, fn_number, which_solution, x_shift,
                         y_shift, int(chain), "walker-get-data-and-fit")[0]


def walker_set_get_data_and_fit(walker, take=1000, x_column=0, y_column=1, fn_number=0,
                                which_solution=":most-likely", x_shift=None, y_shift=None):
    """walker-get-data-and-fit mapped over the set: entry c is what
    walker_get_data_and_fit(..., chain=c) returns, from ONE fit_bands call, one eval_function
    call and one walker_set_get."""
    return _data_and_fit(walker, take, x_column, y_column, fn_number, which_solution, x_shift,
                         y_shift, None, "walker-set-get-data-and-fit")


def _credible_pcts(band, who):
    """the (lo, median, hi) percentiles of a band: ':95cr', ':iqr' or (':percentile', lo, hi)"""
    if isinstance(band, (tuple, list)):
        if len(band) != 3 or str(band[0]).lstrip(":").lower() != "percentile":
            raise ValueError("%s: a band is ':95cr', ':iqr' or (':percentile', lo, hi), not %r" % (who, band))
        lo, hi = band[1], band[2]
    else:
        pair = {"95cr": (2.5, 97.5), "iqr": (25, 75)}.get(str(band).lstrip(":").lower())
        if pair is None:
            raise ValueError("%s: a band is ':95cr', ':iqr' or (':percentile', lo, hi), not %r" % (who, band))
        lo, hi = pair
    if not 0 <= lo <= hi <= 100:
        raise ValueError("%s: the band's percentiles must satisfy 0 <= lo <= hi <= 100, not %r, %r" % (who, lo, hi))
    return [lo, 50, hi]


def _fit_credible(walker, take, points, band, x_column, fn_number, chains, who):
    e = walker.engine
    lengths = e.state()["length"].astype(np.int64)
    data = walker.data_of(fn_number, 0)
    x_data = np.asarray(data[x_column], dtype=np.float64)
    if x_data.ndim != 1:
        raise capi.MhxError(capi.EUNSUPPORTED, "%s draws one column of x: a vector-valued x has no min "
                            "and max (use Engine.fit_percentiles)" % who)
    x_fit = fit_linspace(x_data.min(), x_data.max(), int(points))
    which = range(e.n_chains) if chains is None else [chains]
    big = int(lengths.max()) if take is None else int(take)
    pct, mean, sd, _, status = e.fit_percentiles(
        fn_number, _band_take(walker, big, lengths[list(which)], who), x_fit, _credible_pcts(band, who))
    bad = [c for c in which if status[c] & capi.FITPCT_NONFINITE]
    if bad:
        raise FloatingPointError(
            "%s: the model is not finite at a step of walker(s) %s: the reference would have "
            "signalled a floating-point trap here" % (who, bad[:8]))
    return [[list(x_fit), list(pct[c, 2]), list(pct[c, 0]), list(pct[c, 1]), list(mean[c]), list(sd[c])]
            for c in which]


def walker_get_fit_credible(walker, take=1000, points=1000, band=":95cr", x_column=0, fn_number=0,
                            chain=0):
    """The credible band of the fit: [x_fit, hi, lo, median, mean, stddev], the pointwise
    posterior of function fn_number over the walk's newest `take` steps at `points` points between
    the data's least and greatest x (fit_linspace, as walker_get_data_and_fit), computed on the
    device (mhx_get_fit_percentiles, which has the definition).  band: ':95cr' (the 2.5 and 97.5
    per cent points), ':iqr' (25, 75) or (':percentile', lo, hi); the median is the 50 per cent
    point; stddev is NaN for a walk of one step.  Where walker_get_data_and_fit's max_ys / min_ys
    are the reference's envelope - whose width depends on take - these are percentiles with a
    coverage meaning.  Raises FloatingPointError where a model value of the window is not finite.
    The device call is the whole set's: for more than a few walkers call
    walker_set_get_fit_credible once."""
    return _fit_credible(walker, take, points, band, x_column, fn_number, int(chain),
                         "walker-get-fit-credible")[0]


def walker_set_get_fit_credible(walker, take=1000, points=1000, band=":95cr", x_column=0, fn_number=0):
    """walker_get_fit_credible mapped over the set: entry c is what
    walker_get_fit_credible(..., chain=c) returns, from ONE device call per function."""
    return _fit_credible(walker, take, points, band, x_column, fn_number, None,
                         "walker-set-get-fit-credible")


def _residual_solution(which_solution, who):
    s = str(which_solution).lstrip(":").lower()
    if s not in ("median", "most-likely"):
        raise ValueError("%s: which_solution is ':median' or ':most-likely', not %r" % (who, which_solution))
    return s


def _residual_columns(walker, fn_number, chain, x_column=0, y_column=1):
    """(x_data, y_data, stddev per point) of walker `chain`; a stddev of one number is spread over
    the points (M:1280)"""
    data = walker.data_of(fn_number, chain)
    x_data = np.asarray(data[x_column], dtype=np.float64)
    y_data = np.asarray(data[y_column], dtype=np.float64)
    sd = np.asarray(walker.data_error_of(fn_number, chain), dtype=np.float64).reshape(-1)
    if sd.size == 1:
        sd = np.full(len(y_data), sd[0])
    return x_data, y_data, sd


def walker_get_residuals(walker, take=1000, x_column=0, y_column=1, fn_number=0, chain=0,
                         which_solution=":median"):
    """the data of walker-plot-residuals M:1271-1283 without the plot: [x_data, y_fit - y_data,
    stddev] at the median parameters over `take` (which_solution ':most-likely': at the walker's
    most-likely parameters); y_fit at the dataset's own x, which is on the device already; a
    stddev of one number is spread over the points (M:1280)."""
    cap = walker.length(chain)
    take = cap if take is None or take > cap else int(take)
    x_data, y_data, sd = _residual_columns(walker, fn_number, chain, x_column, y_column)
    if _residual_solution(which_solution, "walker-get-residuals") == "median":
        _, th = _fit_solution(walker, ":median", take, chain)
        th = th[0]
    else:
        th = walker.engine.state()["best_theta"][chain]
    y_fit = walker.engine.eval_function(fn_number, th)
    return [list(x_data), [float(a - b) for a, b in zip(y_fit, y_data)], list(sd)]


def runs_z(n_pos, n_neg, runs):
    """Wald and Wolfowitz's score of `runs` runs of equal sign among n_pos positive and n_neg other
    residuals: (runs - mu) / sqrt(var) with N = n_pos + n_neg, mu = 2 n_pos n_neg / N + 1,
    var = (mu - 1)(mu - 2) / (N - 1).  Far below zero: too few runs, the residuals are structured
    (a peak is missing).  NaN where it is undefined (N < 2, or all residuals of one sign)."""
    n_pos, n_neg, runs = float(n_pos), float(n_neg), float(runs)
    N = n_pos + n_neg
    if N < 2.0:
        return float("nan")
    mu = 2.0 * n_pos * n_neg / N + 1.0
    var = (mu - 1.0) * (mu - 2.0) / (N - 1.0)
    if not var > 0.0:
        return float("nan")
    return (runs - mu) / math.sqrt(var)


def _residual_call(walker, take, fn_number, which_solution, z_limit, pointwise, who):
    """ONE mhx_get_residuals call for the set, at the medians over `take` (one
    mhx_get_percentiles call) or at the most-likely parameters (which the device holds)"""
    e = walker.engine
    theta = None
    if _residual_solution(which_solution, who) == "median":
        _, theta = _fit_solution(walker, ":median", take)
    return e.residuals(fn_number, theta, z_limit=z_limit, pointwise=pointwise)


def walker_set_get_residuals(walker, take=1000, fn_number=0, which_solution=":median"):
    """walker_get_residuals mapped over the set: entry c is what walker_get_residuals(..., chain=c)
    returns - [x_data, y_fit - y_data, stddev] of walker c's own data - from ONE
    mhx_get_percentiles call (none for ':most-likely') and ONE mhx_get_residuals call, whose fit
    values are mhx_eval_function's bits; the raw y is subtracted here, as walker_get_residuals
    does."""
    r = _residual_call(walker, take, fn_number, which_solution, 3.0, True, "walker-set-get-residuals")
    out = []
    for c in range(walker.engine.n_chains):
        x_data, y_data, sd = _residual_columns(walker, fn_number, c)
        out.append([list(x_data), [float(a - b) for a, b in zip(r["fit"][c], y_data)], list(sd)])
    return out


def _goodness_of_fit(walker, take, fn_number, which_solution, z_limit, chains, who):
    r = _residual_call(walker, take, fn_number, which_solution, z_limit, False, who)
    fns = _force_list(walker.function)
    n_points = len(np.asarray(walker.data_of(fn_number, 0)[1]).reshape(-1))
    dof = n_points - len(set(fns[fn_number].keys))
    which = range(walker.engine.n_chains) if chains is None else [chains]
    bad = [c for c in which if r["status"][c] & capi.RESID_NONFINITE]
    if bad and chains is not None:
        raise FloatingPointError(
            "%s: a model value or a residual of walker(s) %s is not finite: the reference would have "
            "signalled a floating-point trap here" % (who, bad[:8]))
    out = []
    for c in which:
        chi2, n_pos = float(r["chi2"][c]), int(r["n_pos"][c])
        with np.errstate(all="ignore"):
            out.append({"chi2": chi2, "dof": dof,
                        "reduced-chi2": float(np.float64(chi2) / np.float64(dof)),
                        "mean-z": float(r["sum_z"][c] / np.float64(n_points)),
                        "durbin-watson": float(r["dw"][c] / r["chi2"][c]),
                        "runs": int(r["n_runs"][c]), "n-pos": n_pos,
                        "runs-z": runs_z(n_pos, n_points - n_pos, int(r["n_runs"][c])),
                        "max-z": float(r["max_abs_z"][c]), "max-z-index": int(r["max_index"][c]),
                        "n-out": int(r["n_out"][c]), "status": int(r["status"][c])})
    return out


def walker_set_goodness_of_fit(walker, take=1000, fn_number=0, which_solution=":median", z_limit=3.0):
    """Which walkers of the set fit badly: for every walker, from ONE mhx_get_residuals call (which
    has the definitions) at the medians over `take` (':most-likely': at the most-likely
    parameters), the dict {"chi2": the sum of the squared standardized residuals z (fit minus data
    over the point's error), "dof": the points minus the distinct parameters function fn_number
    reads, "reduced-chi2", "mean-z", "durbin-watson": sum (z_i - z_{i-1})^2 / chi2 (2 for
    uncorrelated residuals, towards 0 for structured ones), "runs": the runs of equal sign,
    "n-pos", "runs-z": runs_z of them, "max-z" and "max-z-index": the greatest |z| and its point,
    "n-out": the points with |z| > z_limit, "status": 0 or RESID_NONFINITE (the sums of such a
    walker mean nothing)}.  No fit values cross to the host."""
    return _goodness_of_fit(walker, take, fn_number, which_solution, z_limit, None,
                            "walker-set-goodness-of-fit")


def walker_goodness_of_fit(walker, chain=0, take=1000, fn_number=0, which_solution=":median", z_limit=3.0):
    """One walker's entry of walker_set_goodness_of_fit.  Raises FloatingPointError where a model
    value or a residual of that walker is not finite, as walker_waic does.  The device call is the
    whole set's: for more than a few walkers call walker_set_goodness_of_fit once."""
    return _goodness_of_fit(walker, take, fn_number, which_solution, z_limit, int(chain),
                            "walker-goodness-of-fit")[0]


# ---------------------------------------------------------------------- before the walk: Laplace
# The classical answer beside the sampled one, and a proposal to start the walk from: the normal
# equations of every walker come from ONE device call per function (mhx_get_normal_equations,
# whose comment in include/mhx.h has the definition, bit for bit); what is done with them here -
# the inverse, the Cholesky factor, the polish - is numpy's linear algebra and is NOT bit-defined.
LAPLACE_NONFINITE, LAPLACE_NOT_POSITIVE = 1, 2


def laplace_summary(F, b, chi2, n_points, varied, status=0):
    """The Laplace (Gauss-Newton) summary of ONE walker from its normal equations F [d, d], b [d],
    chi2 over n_points points, host arithmetic: `varied` are the places of theta that were varied
    (p of them; the others are fixed: their rows and columns of F are zero).  A dict of
    "chi2", "dof" = n_points - p, "reduced-chi2", "gradient" = b [d], "covariance-matrix" = F^-1
    over the varied places [p, p], "stddev-params" [d] (0 for a fixed place), "correlation" [p, p],
    "newton-decrement" = b^T F^-1 b, "l-matrix" = chol(F^-1) 2.38 / sqrt(p) laid into [d, d] with
    a zero row and column for a fixed place, and "status": 0, LAPLACE_NONFINITE (a value of the
    device's or of F is not finite) or LAPLACE_NOT_POSITIVE (F has no Cholesky factor); what cannot
    be formed then is None."""
    F = np.asarray(F, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    d = b.size
    varied = [int(t) for t in varied]
    p = len(varied)
    dof = int(n_points) - p
    out = {"chi2": float(chi2), "dof": dof,
           "reduced-chi2": float(np.float64(chi2) / np.float64(dof)) if dof > 0 else float("nan"),
           "gradient": b.copy(), "covariance-matrix": None, "stddev-params": None, "correlation": None,
           "newton-decrement": None, "l-matrix": None, "status": 0}
    Fv, bv = F[np.ix_(varied, varied)], b[varied]
    if status or not (np.isfinite(Fv).all() and np.isfinite(bv).all() and np.isfinite(chi2)):
        out["status"] = LAPLACE_NONFINITE
        return out
    try:
        np.linalg.cholesky(Fv)
        cov = np.linalg.inv(Fv)
        cov = 0.5 * (cov + cov.T)
        lc = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        out["status"] = LAPLACE_NOT_POSITIVE
        return out
    sd = np.sqrt(np.diag(cov))
    stddev, L = np.zeros(d), np.zeros((d, d))
    stddev[varied] = sd
    L[np.ix_(varied, varied)] = lc * (2.38 / np.sqrt(p))
    out.update({"covariance-matrix": cov, "stddev-params": stddev, "correlation": cov / np.outer(sd, sd),
                "newton-decrement": float(bv @ np.linalg.solve(Fv, bv)), "l-matrix": L})
    return out


def _normal_equations_all(engine, theta, steps):
    """(F, b, chi2, status) of every walker, summed over the functions of a global fit in
    ascending k: one mhx_get_normal_equations call per function"""
    F = b = chi2 = status = None
    for k in range(engine.K):
        r = engine.normal_equations(k, theta, steps)
        if F is None:
            F, b, chi2, status = r["jtj"], r["jtr"], r["chi2"], r["status"].copy()
        else:
            with np.errstate(all="ignore"):
                F, b, chi2 = F + r["jtj"], b + r["jtr"], chi2 + r["chi2"]
            status |= r["status"]
    return F, b, chi2, status


def _laplace_steps(walker, theta, steps, fixed):
    """the steps [n_chains, d] of a Laplace call: `steps` None (normeq_steps of theta), an array [d]
    or [n_chains, d], or a plist / dict key -> h for some keys; 0 for the keys named in `fixed`"""
    from .engine import normeq_steps
    e = walker.engine
    keys = list(walker.param_keys)
    hs = normeq_steps(theta)
    if isinstance(steps, dict) or (isinstance(steps, (list, tuple)) and steps and isinstance(steps[0], str)):
        for k, h in zip(*_plist(steps)):
            hs[:, keys.index(k)] = float(h)
    elif steps is not None:
        hs = np.broadcast_to(np.asarray(steps, dtype=np.float64), (e.n_chains, e.d)).copy()
    fixed_at = sorted(keys.index(_key(k)) for k in fixed)
    hs[:, fixed_at] = 0.0
    return hs, [t for t in range(e.d) if t not in fixed_at]


def _laplace(walker, theta, steps, fixed, chains):
    e = walker.engine
    if theta is None:
        theta = e.state()["best_theta"]
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    hs, varied = _laplace_steps(walker, theta, steps, fixed)
    F, b, chi2, status = _normal_equations_all(e, theta, hs)
    n_points = sum(len(np.asarray(walker.data_of(k, 0)[-1]).reshape(-1)) for k in range(e.K))
    out = []
    for c in (range(e.n_chains) if chains is None else [chains]):
        s = laplace_summary(F[c], b[c], chi2[c], n_points, varied, int(status[c]))
        s["params"] = dict(zip(walker.param_keys, (float(v) for v in theta[c])))
        s["varied-keys"] = [walker.param_keys[t] for t in varied]
        out.append(s)
    return out


def _laplace_theta(walker, which_solution, take, who):
    if _residual_solution(which_solution, who) == "median":
        return _fit_solution(walker, ":median", take)[1]
    return None


def walker_set_laplace(walker, which_solution=":most-likely", take=1000, steps=None, fixed=()):
    """The classical least-squares answer of every walker of the set, at its most-likely parameters
    (which_solution ':median': at the medians over `take`): a list with, walker by walker,
    laplace_summary's dict - chi2, dof, reduced-chi2, gradient, covariance-matrix (J^T W J)^-1 over
    the varied keys, stddev-params, correlation, newton-decrement, l-matrix, status - and "params"
    and "varied-keys".  `steps`: the half-widths of the central differences (_laplace_steps);
    keys named in `fixed` are held.  F and b are summed over the functions of a global fit in
    ascending k.  The "l-matrix" is a proposal factor walker_adaptive_steps_full takes as
    l_matrix=: np.array([s["l-matrix"] for s in ...]) gives every walker its own.  One device call
    per function for the whole set, a dataset per walker included; the linear algebra is numpy's
    and not bit-defined."""
    return _laplace(walker, _laplace_theta(walker, which_solution, take, "walker-set-laplace"), steps, fixed, None)


def walker_laplace(walker, chain=0, which_solution=":most-likely", take=1000, steps=None, fixed=()):
    """One walker's entry of walker_set_laplace.  The device call is the whole set's: for more than
    a few walkers call walker_set_laplace once."""
    return _laplace(walker, _laplace_theta(walker, which_solution, take, "walker-laplace"), steps, fixed,
                    int(chain))[0]


def least_squares(normal_equations, objective, theta0, iterations=25, damping=1e-3):
    """Levenberg-Marquardt for many walkers at once, over two callables (host arithmetic, not
    bit-defined): normal_equations(theta [n, d]) -> (F [n, d, d], b [n, d]) with F delta = b the
    Gauss-Newton step that raises the fit, and objective(theta [n, d]) -> [n], what must not fall
    (the log-posterior, so that the soft bounds hold).  Per walker and iteration
    (F + lambda diag F) delta = b is solved and theta + delta is taken only where the objective
    RISES; lambda, `damping` at first, is divided by 10 on success and multiplied by 10 on
    failure.  A place whose row of F is zero (a fixed key) does not move.  Returns {"theta",
    "objective", "iterations": the last iteration (1-based) that moved the walker, 0 if none,
    "damping": lambda at the end, "history": the objective after every iteration [iterations + 1,
    n]}."""
    theta = np.array(theta0, dtype=np.float64, ndmin=2)
    n, d = theta.shape
    obj = np.asarray(objective(theta), dtype=np.float64).copy()
    lam = np.full(n, float(damping))
    used = np.zeros(n, dtype=np.int64)
    history = [obj.copy()]
    for it in range(1, int(iterations) + 1):
        F, b = normal_equations(theta)[:2]
        F, b = np.asarray(F, dtype=np.float64), np.asarray(b, dtype=np.float64)
        trial = theta.copy()
        ok = np.zeros(n, dtype=bool)
        for c in range(n):
            dg = np.diag(F[c]).copy()
            live = dg > 0.0
            if not live.any() or not (np.isfinite(F[c]).all() and np.isfinite(b[c]).all()):
                continue
            A = F[c][np.ix_(live, live)] + lam[c] * np.diag(dg[live])
            try:
                delta = np.linalg.solve(A, b[c][live])
            except np.linalg.LinAlgError:
                continue
            if np.isfinite(delta).all():
                trial[c, live] = theta[c, live] + delta
                ok[c] = True
        with np.errstate(all="ignore"):
            new = np.asarray(objective(trial), dtype=np.float64)
            took = ok & (new > obj)
        theta[took], obj[took], used[took] = trial[took], new[took], it
        lam = np.where(took, lam / 10.0, lam * 10.0)
        history.append(obj.copy())
    return {"theta": theta, "objective": obj, "iterations": used, "damping": lam, "history": np.array(history)}


def _axes_items(axes):
    """a key -> values map (a dict, or a plist key values key values ...) as [(key, values [n_k])]"""
    if isinstance(axes, dict):
        items = list(axes.items())
    else:
        a = list(axes)
        if len(a) % 2:
            raise ValueError("axes plist must have an even number of elements")
        items = [(a[i], a[i + 1]) for i in range(0, len(a), 2)]
    out = []
    for k, v in items:
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if v.size < 1:
            raise ValueError("axis %s has no values" % _key(k))
        if _key(k) in [q for q, _ in out]:
            raise ValueError("axis %s is named twice" % _key(k))
        out.append((_key(k), v))
    if not out:
        raise ValueError("no axes")
    return out


def _grid_rows(keys, base, items):
    """base [..., d] with the places of the axes' keys replaced by their Cartesian product in
    row-major order, the first axis slowest: ([..., m, d], shape)"""
    keys = list(keys)
    for k, _ in items:
        if k not in keys:
            raise ValueError("axis %s is not a parameter (%s)" % (k, " ".join(keys)))
    shape = tuple(len(v) for _, v in items)
    m = int(np.prod(shape))
    base = np.asarray(base, dtype=np.float64)
    cand = np.repeat(base[..., None, :], m, axis=-2)
    mesh = np.meshgrid(*(v for _, v in items), indexing="ij")
    for (k, _), g in zip(items, mesh):
        cand[..., keys.index(k)] = g.reshape(-1)
    return np.ascontiguousarray(cand), shape


def candidate_grid(params, axes):
    """The starts of a brute-force search: `params` (a plist or dict, the base vector) with the keys
    of `axes` (key -> values) replaced by the Cartesian product of the axes' values.  Returns (cand
    [m, d], shape): row-major, the first axis slowest, shape = the axes' lengths, so that
    scores.reshape(shape) is the map over the axes."""
    keys, vals = _plist(params)
    return _grid_rows(keys, vals, _axes_items(axes))


def walker_set_search(walker, candidates=None, axes=None, keep=4, with_prior=True, apply=False):
    """The brute-force stage before a polish, for every walker of the set: each walker tries the
    candidates against its own data in ONE device call (Engine.candidate_scores over all functions)
    and the `keep` least chi-squares are kept.  candidates: [m, d] for all walkers or [n_chains, m,
    d]; or axes (key -> values): every walker's own most-likely parameters with those keys replaced
    by the axes' Cartesian product (candidate_grid's order).  with_prior ranks the kept ones again
    by Engine.logpost - `keep` calls of [n_chains, d] rows, row = walker - so that the soft bounds
    count: the winner has the greatest log-posterior among the kept, among equals the lesser
    chi-square; without it the winner is the least chi-square.  A candidate whose chi-square is not
    finite never wins.  Returns, walker by walker, {"params", "index" (into the candidates),
    "chi2", "logpost" (None without the prior), "n-bad": candidates that were not finite}; a walker
    none of whose candidates is finite gets index -1 and its most-likely parameters.  apply=True
    calls init_chains at the winners: the walkers stand there and their histories are reset."""
    e = walker.engine
    n, d = e.n_chains, e.d
    if (candidates is None) == (axes is None):
        raise ValueError("walker-set-search: give candidates or axes, one of them")
    start = None
    if candidates is None:
        start = e.state()["best_theta"]
        cand, _ = _grid_rows(walker.param_keys, start, _axes_items(axes))
    else:
        cand = np.ascontiguousarray(candidates, dtype=np.float64)
    r = e.candidate_scores(cand, fn=-1, keep=keep)
    idx, chi = r["best_index"], r["best_score"]
    if start is None:
        start = e.state()["best_theta"]
    rows_of = (lambda j: cand[np.arange(n), j]) if cand.ndim == 3 else (lambda j: cand[j])
    usable = (idx >= 0) & np.isfinite(chi)
    pick = np.zeros(n, dtype=np.int64)
    lp = None
    if with_prior:
        lp = np.full(idx.shape, -np.inf)
        for k in range(idx.shape[1]):
            rows = np.where(usable[:, k, None], rows_of(np.maximum(idx[:, k], 0)), start)
            with np.errstate(all="ignore"):
                v = np.asarray(e.logpost(np.ascontiguousarray(rows)), dtype=np.float64)
            lp[:, k] = np.where(usable[:, k] & ~np.isnan(v), v, -np.inf)
        pick = np.argmax(lp, axis=1)  # (the first of equals: the lesser chi-square)
    found = usable[np.arange(n), pick]
    win = np.where(found, idx[np.arange(n), pick], -1)
    theta = np.ascontiguousarray(np.where(found[:, None], rows_of(np.maximum(win, 0)), start))
    if apply:
        e.init_chains(theta)
    return [{"params": dict(zip(walker.param_keys, (float(v) for v in theta[c]))),
             "index": int(win[c]), "chi2": float(chi[c, pick[c]]),
             "logpost": float(lp[c, pick[c]]) if with_prior else None,
             "n-bad": int(r["n_bad"][c])} for c in range(n)]


def walker_search(walker, chain=0, candidates=None, axes=None, keep=4, with_prior=True):
    """One walker's entry of walker_set_search.  The device call is the whole set's: for more than a
    few walkers call walker_set_search once."""
    return walker_set_search(walker, candidates=candidates, axes=axes, keep=keep,
                             with_prior=with_prior)[int(chain)]


def walker_set_chi2_map(walker, axes, which_solution=":most-likely", take=1000):
    """The chi-square map around every walker's own solution - what one draws to see whether a
    second minimum exists: the walker's most-likely parameters (which_solution ':median': the
    medians over `take`) with the one or two keys of `axes` (key -> values) replaced by the axes'
    values, scored over all functions in one device call.  Returns {"axes": {key: values}, "chi2"
    [n_chains, *shape] (+inf where not finite), "delta-chi2": chi2 minus the walker's least}."""
    e = walker.engine
    items = _axes_items(axes)
    if len(items) > 2:
        raise ValueError("walker-set-chi2-map: one or two axes, not %d" % len(items))
    theta = _laplace_theta(walker, which_solution, take, "walker-set-chi2-map")
    if theta is None:
        theta = e.state()["best_theta"]
    cand, shape = _grid_rows(walker.param_keys, theta, items)
    chi = e.candidate_scores(cand, fn=-1, keep=1, scores=True)["score"].reshape((e.n_chains,) + shape)
    low = chi.reshape(e.n_chains, -1).min(axis=1).reshape((e.n_chains,) + (1,) * len(shape))
    with np.errstate(invalid="ignore"):
        delta = np.where(np.isfinite(chi), chi - low, np.inf)
    return {"axes": {k: v for k, v in items}, "chi2": chi, "delta-chi2": delta}


def walker_set_least_squares(walker, iterations=25, apply=False, theta0=None):
    """Polish every walker of the set to its least-squares point before the walk: least_squares
    from the walkers' most-likely parameters (theta0 [n_chains, d]: from there instead, the
    winners of walker_set_search, say), driven by Engine.normal_equations (summed over the
    functions of a global fit) and Engine.logpost - (2 p + 1) model sweeps and one log-posterior
    per iteration for the WHOLE set.  Returns {"theta" [n_chains, d], "params": the plists,
    "laplace": walker_set_laplace's entries at the polished parameters, "iterations",
    "objective"}.  apply=True calls init_chains on the result: the walkers stand there and their
    histories are reset, as that call documents."""
    from .engine import normeq_steps
    e = walker.engine
    if theta0 is None:
        theta0 = e.state()["best_theta"]
    else:
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        if theta0.shape != (e.n_chains, e.d):
            raise ValueError("walker-set-least-squares: theta0 must be [n_chains, d] = [%d, %d]"
                             % (e.n_chains, e.d))

    def equations(theta):
        F, b, _, _ = _normal_equations_all(e, theta, normeq_steps(theta))
        return F, b
    r = least_squares(equations, lambda theta: e.logpost(np.ascontiguousarray(theta)),
                      theta0, iterations=iterations)
    theta = np.ascontiguousarray(r["theta"])
    lap = _laplace(walker, theta, None, (), None)
    if apply:
        e.init_chains(theta)
    return {"theta": theta, "params": [s["params"] for s in lap], "laplace": lap,
            "iterations": r["iterations"], "objective": r["objective"]}


_EXP_PERCENTILES = {"median": (50,), "95cr": (2.5, 97.5), "iqr": (25, 75),
                    "stddev-normal": (50, 84.1)}
_EXP_SELECTORS = ("most-likely", "median", "95cr", "iqr", "mean", "stddev", "stddev-normal",
                  "values", "percentile")


def exp_selector(get):
    """(selector, percentiles the device is asked for) of walker_exp_get's `get`: ':median',
    ':95cr', ... or (':percentile', n)"""
    arg = None
    if isinstance(get, (tuple, list)):
        if len(get) != 2:
            raise ValueError("unknown :get %r" % (get,))
        get, arg = get
    g = str(get).lstrip(":").lower()
    if g not in _EXP_SELECTORS or (g == "percentile") != (arg is not None):
        raise ValueError("unknown :get %r" % (get,))
    if g == "percentile":
        if not 0 <= float(arg) <= 100:
            raise ValueError("a percentile lies in [0, 100], not %r" % (arg,))
        return g, (arg,)
    return g, _EXP_PERCENTILES.get(g, ())


def _exp_call(walker, exp):
    """(names, places in theta, C text) of a walker-with-exp form; KeyError for a keyword that
    is no parameter key of the walker"""
    from . import sexpr
    names, text = sexpr.keyword_exp_to_expr(exp)
    keys = list(walker.param_keys)
    for k in names:
        if k not in keys:
            raise KeyError(":" + k)
    return names, [keys.index(k) for k in names], text


def _exp_window(walker, take):
    e = walker.engine
    return max(1, min(int(take), e.history_capacity()))


def _exp_results(g, pcts, r, values):
    """what walker_exp_get returns, chain by chain, from Engine.derived's arrays"""
    out = []
    for c in range(r["n_used"].shape[0]):
        p = [float(v) for v in r["pct"][c, :, 0]]
        if g == "most-likely":
            out.append(float(r["at_most_likely"][c, 0]))
        elif g in ("median", "percentile"):
            out.append(p[0])
        elif g == "95cr":  # M:1508-1509
            out.append([p[0], p[1]])
        elif g == "iqr":  # M:1511-1513
            out.append(p[1] - p[0])
        elif g == "stddev-normal":  # M:1529-1535: the 84.1 point minus the median
            out.append(p[1] - p[0])
        elif g == "mean":
            out.append(float(r["mean"][c, 0]))
        elif g == "stddev":
            out.append(float(r["stddev"][c, 0]))
        else:  # values, newest first
            out.append(values[c, 0, :int(r["n_used"][c])].copy())
    return out


def _exp_hdi_selector(get):
    """('hdi', mass) or ('quantiles', points) where `get` is one of walker_exp_get's two selectors
    that order the window, else None"""
    if isinstance(get, (tuple, list)) and len(get) == 2:
        g = str(get[0]).lstrip(":").lower()
        if g in ("hdi", "quantiles"):
            return g, get[1]
    return None


def walker_set_exp_get(walker, exp, get=":median", take=1000):
    """walker_exp_get for every chain of the set from ONE device call (mhx_get_derived; (":hdi",
    mass) and (":quantiles", points): mhx_get_derived_hdi): a list with, chain by chain, exactly
    what walker_exp_get(..., chain=c) returns."""
    ordered = _exp_hdi_selector(get)
    if ordered is not None:
        names, index, text = _exp_call(walker, exp)
        window = _exp_window(walker, take)
        if ordered[0] == "hdi":
            r = walker.engine.derived_hdi([text], names, index, window, [ordered[1]])
            return [[float(r["lo"][c, 0, 0]), float(r["hi"][c, 0, 0])] for c in range(r["lo"].shape[0])]
        r = walker.engine.derived_hdi([text], names, index, window, [], ladder=int(ordered[1]))
        return [r["ladder"][c, 0].copy() for c in range(r["ladder"].shape[0])]
    g, pcts = exp_selector(get)
    names, index, text = _exp_call(walker, exp)
    r = walker.engine.derived([text], names, index, _exp_window(walker, take), pcts,
                              values=g == "values")
    return _exp_results(g, pcts, r, r.get("values"))


def walker_exp_get(walker, exp, get=":median", take=1000, chain=0):
    """The posterior of walker-with-exp's expression over the walker's newest `take` steps: the
    form is evaluated at every step of the window on the device (mhx_get_derived) and summarised
    there.  get: :most-likely (walker_with_exp), :median, :95cr (a [lo, hi] pair), :iqr, :mean,
    :stddev (NaN for a one-step window), :stddev-normal (the 84.1 point minus the median,
    M:1529-1535), :values (newest first), (":percentile", n), (":hdi", mass) - the narrowest [lo,
    hi] that holds `mass` per cent of the window's values (mhx_get_derived_hdi, which has the
    definition) - or (":quantiles", points): the sorted window at that many evenly spaced ranks."""
    return walker_set_exp_get(walker, exp, get, take)[chain]


def walker_set_with_exp(walker, exp, take=1000):
    """walker_with_exp for every chain of the set from one device call"""
    return walker_set_exp_get(walker, exp, ":most-likely", take)


def walker_with_exp(walker, exp, take=1000, chain=0):
    """(walker-with-exp walker exp &key take) M:1052-1064: the form `exp` (Lisp text) with every
    keyword replaced by that parameter of the walker's most-likely step, evaluated - on the
    device, in binary64, in the form's own order of operations.  `take` is accepted as in the
    reference, where :most-likely-params ignores it too (M:511-515).  KeyError for a keyword
    that is no parameter key, SexprError for an operator the device grammar lacks."""
    return walker_set_with_exp(walker, exp, take)[chain]


def _exact_linspace(start, end, n):
    """(linspace start end :len n) M:235-248 for doubles: (rational start) + i (rational (end -
    start)) / (n - 1) exactly - integers over one common denominator - each coerced to double by
    one correctly rounded division"""
    start, end = float(start), float(end)
    ps, qs = start.as_integer_ratio()
    pd, qd = (end - start).as_integer_ratio()
    den = qs * qd * (n - 1)
    first, step = ps * qd * (n - 1), pd * qs
    return [(first + i * step) / den for i in range(n)]


def histo_edges(bottom, top, num_bins):
    """make-histo's boundaries M:1547: (linspace bottom top :len num-bins + 1).  The last can
    round below `top`: make-histo then leaves the greatest values out of every bin."""
    return _exact_linspace(bottom, top, int(num_bins) + 1)


def _histo_x(bottom, top, num_bins):
    """make-histo-x's list M:1563-1564 from the extremes.  One bin: the reference divides by
    zero (a linspace of one element); the bin's centre is returned here."""
    bottom, top = float(bottom), float(top)
    start = bottom + (top - bottom) / num_bins / 2
    return [start] if num_bins == 1 else _exact_linspace(start, top, num_bins)


def make_histo(sequence, num_bins):
    """(make-histo sequence num-bins) M:1542-1557 on an ASCENDING sequence, as walker-param-histo
    hands it over: count n = the values not yet counted that are <= boundary n, i.e. a value falls
    in the first bin whose upper boundary is not below it.  num_bins is required (the reference's
    automatic count is not mirrored)."""
    v = np.asarray(sequence, dtype=np.float64)
    upto = np.searchsorted(v, histo_edges(v.min(), v.max(), num_bins)[1:], side="right")
    return [int(c) for c in np.diff(upto, prepend=0)]


def make_histo_x(sequence, num_bins):
    """(make-histo-x sequence num-bins) M:1559-1564: the abscissae the reference plots the counts
    at - from half a bin above the least value to the greatest, in num_bins exact steps"""
    v = np.asarray(sequence, dtype=np.float64)
    return _histo_x(v.min(), v.max(), int(num_bins))


def walker_param_histo(walker, key, take=10000, bins=20, chain=0):
    """(walker-param-histo walker key &key take bins) M:1361-1369 without the plot: (histo_x,
    histo), the two lists the reference hands to gnuplot, of one chain's trace."""
    values = sorted(walker_get(walker, ":param", take=take, param=key, chain=chain))
    return make_histo_x(values, bins), make_histo(values, bins)


def _bin_window(walker, take, who):
    """the window the device serves for :take `take` (None: every walk whole),
    with walker_set_get's warning when a walk's window reaches past the ring"""
    e = walker.engine
    cap = e.state()["length"].astype(np.int64)
    t = cap if take is None else np.minimum(int(take), cap)
    ring = e.history_capacity()
    widest = max(int(t.max()), 1)
    if int((t > ring).sum()):
        warnings.warn(HistoryTruncated(
            "%s :take %s: the device history ring holds the newest %d steps of a walk and %d of the "
            "set's %d windows reach past it (the widest asks for %d); create the walker with "
            "history_capacity >= the walks' length to keep them all"
            % (who, take, ring, int((t > ring).sum()), e.n_chains, widest)), stacklevel=3)
    return min(widest, ring)


def _reference_edges(walker, window, cols, bins):
    """make-histo's own boundaries for every chain and column, [n_chains, n_cols, bins + 1], and
    the extremes they come from: the 0 and 100 per cent points of the window, from the device"""
    pct, _ = walker.engine.percentiles(window, [(0, 1), (100, 1)])
    lo, hi = pct[:, 0, cols], pct[:, 1, cols]
    edges = np.array([[histo_edges(lo[c, j], hi[c, j], bins) for j in range(len(cols))]
                      for c in range(lo.shape[0])])
    return edges, lo, hi


def _key_columns(walker, keys):
    names = list(walker.param_keys) if keys is None else [_key(k) for k in keys]
    return names, [list(walker.param_keys).index(k) for k in names]


def walker_set_param_histo(walker, keys=None, take=10000, bins=20):
    """walker_param_histo for every chain of the set and every key (None: all) from three device
    calls and no history moved: the extremes (mhx_get_percentiles), the reference's exact
    boundaries formed on the host, the counts (mhx_get_histograms).  A list with, chain by chain,
    {key: (histo_x, histo)} - what walker_param_histo(walker, key, take, bins, chain=c) returns."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-param-histo")
    edges, lo, hi = _reference_edges(walker, window, cols, int(bins))
    counts = walker.engine.histograms(window, cols, edges)["counts"]
    return [{k: (_histo_x(lo[c, j], hi[c, j], int(bins)), counts[c, j].tolist())
             for j, k in enumerate(names)} for c in range(counts.shape[0])]


def walker_set_trace(walker, keys=None, take=None, thin=1, start=0, which=":steps", envelope=False,
                     prob=True):
    """the steps of every chain of the set as ARRAYS, for sets too large for lists of objects: one
    mhx_get_traces call.  keys: the parameters wanted (None: all); take: the window (None: every
    walk whole); which: :steps, :unique-steps or :forward-steps; thin, start: the reference's
    (thin list thin start) M:149-157 of what `which` keeps, newest first.  A dict of
      values   {key: [n_chains, rows]}, the rows of chain c beyond n_out[c] are zero
      prob     [n_chains, rows] the steps' log-posteriors (None with prob=False)
      n_out, n_kept, n_used  [n_chains]: rows written, steps `which` kept, steps the window held
    and with envelope=True lo and hi {key: [n_chains, rows]}, prob_lo and prob_hi: the smallest and
    greatest value among the `thin` kept steps a row stands for (include/mhx.h has the rule)."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-trace")
    lead = [capi.TRACE_PROB] if prob else []
    r = walker.engine.traces(window, lead + cols, filter=which, stride=int(thin), start=int(start),
                             envelope=envelope)
    at = len(lead)
    out = {"values": {k: r["values"][:, :, at + j].copy() for j, k in enumerate(names)},
           "prob": r["values"][:, :, 0].copy() if prob else None,
           "n_out": r["n_out"], "n_kept": r["n_kept"], "n_used": r["n_used"]}
    if envelope:
        for side in ("lo", "hi"):
            out[side] = {k: r[side][:, :, at + j].copy() for j, k in enumerate(names)}
            out["prob_" + side] = r[side][:, :, 0].copy() if prob else None
    return out


def walker_set_catepillar(walker, take=None, points=None):
    """the numbers behind walker-catepillar-plots M:1294-1309 and walker-liklihood-plot M:1313-1320
    for every walker of the set, without the plots.  points None: every step - each key's :param
    list and the :log-liklihoods, as arrays.  points p: at most about p rows a walk, for a plot p
    pixels wide: stride = ceil(window / p), and for every bucket of `stride` steps its first
    value and its extremes, so that no excursion is lost to the thinning.  A dict of stride,
    n_out [n_chains] (rows of each chain, newest first; the rest are zero), params {key: {"first":
    [n_chains, rows]}} and log_liklihoods {"first": ...}, with "lo" and "hi" beside "first" when
    points is given."""
    window = _bin_window(walker, take, "walker-set-catepillar")
    stride = 1 if points is None else max(1, -(-window // int(points)))
    r = walker_set_trace(walker, None, take=window, thin=stride, envelope=points is not None)
    sides = [("first", "values", "prob")] + ([("lo", "lo", "prob_lo"), ("hi", "hi", "prob_hi")] if points is not None else [])
    return {"stride": stride, "n_out": r["n_out"],
            "params": {k: {s: r[v][k] for s, v, _ in sides} for k in r["values"]},
            "log_liklihoods": {s: r[p] for s, _, p in sides}}


def permute_params(params):
    """walker-plot-corner's pair list M:1334-1340: (p_i, p_j) for i < j, i outermost"""
    return [(params[i], params[j]) for i in range(len(params) - 1) for j in range(i + 1, len(params))]


def walker_set_corner_grid(walker, take=None, bins=20, keys=None):
    """walker-plot-corner M:1333-1359 as counts: for every chain of the set, the reference's list
    of key pairs and, for each, the bins x bins grid of step counts - cell [i, j]: the first key
    in bin i+1 and the second in bin j+1 of make-histo's boundaries for that chain and key - in
    place of the scatter of every step (mhx_get_pair_grids; no history moved).  A list with, chain
    by chain, [((key1, key2), grid), ...] in the reference's pair order; take None: the whole walk."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-corner-grid")
    edges, _, _ = _reference_edges(walker, window, cols, int(bins))
    places = permute_params(list(range(len(cols))))
    counts = walker.engine.pair_grids(window, cols, places, edges)["counts"]
    return [[((names[a], names[b]), counts[c, q].copy()) for q, (a, b) in enumerate(places)]
            for c in range(counts.shape[0])]


def _serial_sum(v, start=None):
    """v[0] + v[1] + ... in that order (np.cumsum is a serial sum), from `start` if given"""
    v = np.asarray(v, dtype=np.float64)
    if start is not None:
        v = np.concatenate(([start], v))
    return np.cumsum(v)[-1]


def autocorr(sequence, max_lag):
    """The definitions of mhx_get_autocorr (include/mhx.h) on the host, for one NEWEST-FIRST
    sequence: (acf, tau, ess, status) - rho_0 .. rho_L with L = min(max_lag, len - 1), Geyer's
    initial-positive-sequence autocorrelation time, len / tau, and the status bits
    (capi.AUTOCORR_NONFINITE / _CONSTANT / _OPEN).  Every sum in the device's serial order, so the
    numbers are the device's to the last bit; also the per-chain host route (one trace, this)."""
    x = np.asarray(sequence, dtype=np.float64)
    t, max_lag = len(x), int(max_lag)
    if t < 1 or x.ndim != 1:
        raise ValueError("autocorr needs a sequence of at least one step")
    if not 1 <= max_lag <= capi.MAX_AUTOCORR_LAG:
        raise ValueError("max_lag must be in [1,%d]" % capi.MAX_AUTOCORR_LAG)
    with np.errstate(all="ignore"):
        dev = x - _serial_sum(x) / t
        lags = min(max_lag, t - 1)
        c = np.array([_serial_sum(dev[:t - k] * dev[k:], 0.0) / t for k in range(lags + 1)])
        rho = c / c[0]
        total, is_open = 0.0, True
        for j in range((lags + 1) // 2):
            p = rho[2 * j] + rho[2 * j + 1]
            if not p > 0:
                is_open = False
                break
            total = total + p
        constant = bool(c[0] == 0)
        tau = float(rho[0]) if constant else float(2.0 * total - 1.0)
        ess = float(np.float64(t) / np.float64(tau))
    status = (0 if np.isfinite(x).all() else capi.AUTOCORR_NONFINITE) | \
        (capi.AUTOCORR_CONSTANT if constant else 0) | (capi.AUTOCORR_OPEN if is_open else 0)
    return rho, tau, ess, status


def walker_set_autocorr(walker, keys=None, take=1000, max_lag=255, acf=False):
    """For every chain of the set and every key (None: all), what its newest `take` steps are
    worth - one device call (mhx_get_autocorr), no history moved.  A list with, chain by chain,
    {key: {"tau": the integrated autocorrelation time (Geyer's initial positive sequence over
    lags up to max_lag), "ess": steps / tau, "status": 0, or a sum of 1 (a value that is not
    finite), 2 (the chain did not move: tau is NaN) and 4 (max_lag too small: tau is a lower
    bound)}}; acf=True adds "acf", the autocorrelations of lags 0 to min(max_lag, steps - 1).
    The reference has no counterpart: it judges a walk by its caterpillar plots."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-autocorr")
    r = walker.engine.autocorr(window, cols, int(max_lag), acf=acf)
    out = []
    for c in range(r["tau"].shape[0]):
        entry = {}
        for j, k in enumerate(names):
            entry[k] = {"tau": float(r["tau"][c, j]), "ess": float(r["ess"][c, j]),
                        "status": int(r["status"][c, j])}
            if acf:
                entry[k]["acf"] = r["acf"][c, j, :r["n_lags"][c] + 1].copy()
        out.append(entry)
    return out


def walker_autocorr(walker, key, take=1000, max_lag=255, chain=0):
    """one chain's entry of walker_set_autocorr for one key: {"tau", "ess", "status"}"""
    return walker_set_autocorr(walker, [key], take, max_lag)[chain][_key(key)]


def walker_set_rhat(walker, keys=None, take=1000):
    """split R-hat of every key (None: all) over the set's chains: {key: rhat}, each chain's
    newest `take` steps cut in two halves (mhx_get_autocorr's half moments, mhx_split_rhat).
    ValueError when the chains' windows differ in length or hold fewer than four steps: pick a
    take no longer than the shortest walk."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-rhat")
    r = walker.engine.autocorr(window, cols, 1)
    return dict(zip(names, (float(v) for v in split_rhat(r["half_mean"], r["half_var"], r["n_used"]))))


def _order_keys(x):
    """the 64-bit keys the device orders doubles by: -0 before +0, every NaN last"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    k[np.isnan(x)] = np.uint64(2 ** 64 - 1)
    return k


def hdi(sequence, mass):
    """The definition of mhx_get_hdi (include/mhx.h) on the host, for one sequence in any order:
    (lo, hi, pos) of the narrowest interval between two order statistics that holds `mass` per
    cent - a number or a (num, den) pair - of the values: with s the values in ascending order and
    g = hdi_span(len, mass), the least pos whose s[pos + g] - s[pos] no other exceeds.  Also the
    per-chain host route (one trace, this)."""
    x = np.ascontiguousarray(sequence, dtype=np.float64)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("hdi needs a sequence of at least one value")
    g = hdi_span(len(x), mass)
    s = x[np.argsort(_order_keys(x), kind="stable")]
    with np.errstate(all="ignore"):
        pos = int(np.argmin(s[g:] - s[:len(x) - g]))
    return float(s[pos]), float(s[pos + g]), pos


def walker_set_hdi(walker, mass=95, keys=None, take=1000):
    """The highest-density interval of every key (None: all) of every chain of the set - one
    device call (mhx_get_hdi, which has the definition), no history moved: the narrowest interval
    that holds `mass` per cent (a number or a (num, den) pair) of the chain's newest `take` steps.
    Where a posterior is skewed or pressed against a bound, :95cr's equal tails can leave out its
    most probable value; this interval cannot.  A list with, chain by chain, {key: [lo, hi]}.  The
    reference has no counterpart: its intervals are equal-tailed."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-hdi")
    r = walker.engine.hdi(window, [mass], cols)
    return [{k: [float(r["lo"][c, 0, j]), float(r["hi"][c, 0, j])] for j, k in enumerate(names)}
            for c in range(r["lo"].shape[0])]


def walker_hdi(walker, mass=95, keys=None, take=1000, chain=0):
    """one chain's entry of walker_set_hdi: {key: [lo, hi]}"""
    return walker_set_hdi(walker, mass, keys, take)[chain]


def walker_set_quantiles(walker, points=101, keys=None, take=1000):
    """The quantile function of every key (None: all) of every chain of the set at `points` evenly
    spaced ranks (2..4096) of its newest `take` steps, for an ECDF, a violin or a Q-Q plot - one
    device call (mhx_get_hdi's ladder), no history moved.  A list with, chain by chain,
    {key: array [points]}: entry i is the sorted window's value of rank floor(i (n - 1) /
    (points - 1)), so entry 0 is the least and the last entry the greatest."""
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-quantiles")
    lad = walker.engine.hdi(window, [], cols, ladder=int(points))["ladder"]
    return [{k: lad[c, j].copy() for j, k in enumerate(names)} for c in range(lad.shape[0])]


_ENSEMBLE_PERCENTILES = {"median-params": (50,), "95cr": (2.5, 97.5), "iqr": (25, 75),
                         "stddev-normal": (50, 84.1)}


def walker_set_ensemble_get(walker, get=":median-params", take=1000, keys=None, include=None):
    """ONE posterior for the whole set: the chains' newest `take` steps pooled, and for every key
    (None: all) a point of that pool - one device call (mhx_get_ensemble_percentiles), no history
    moved, exact whatever the set's size.  get: :median-params, :95cr (a [lo, hi] pair), :iqr,
    :stddev-normal (the 84.1 point minus the median, M:1529-1535) or (":percentile", n); the
    points and result shapes are walker_exp_get's.  include: one truth value per chain, to leave
    out chains that never converged (walker_set_rhat, a poor :most-likely-step); None: all.
    Returns {key: value}.  The reference has no counterpart: walker-set-get answers per chain."""
    arg = None
    if isinstance(get, (tuple, list)):
        if len(get) != 2:
            raise ValueError("unknown :get %r" % (get,))
        get, arg = get
    g = str(get).lstrip(":").lower()
    if (g not in _ENSEMBLE_PERCENTILES and g != "percentile") or (g == "percentile") != (arg is not None):
        raise ValueError("unknown :get %r" % (get,))
    if g == "percentile":
        _, pcts = exp_selector((":percentile", arg))
    else:
        pcts = _ENSEMBLE_PERCENTILES[g]
    names, cols = _key_columns(walker, keys)
    window = _bin_window(walker, take, "walker-set-ensemble-get")
    p = walker.engine.ensemble_percentiles(window, pcts, cols, include)["out"]
    out = {}
    for j, k in enumerate(names):
        v = [float(x) for x in p[:, j]]
        if g in ("median-params", "percentile"):
            out[k] = v[0]
        elif g == "95cr":  # M:1508-1509
            out[k] = [v[0], v[1]]
        else:  # iqr M:1511-1513; stddev-normal M:1529-1535
            out[k] = v[1] - v[0]
    return out


def _waic(walker, take, pointwise, chains, who):
    e = walker.engine
    window = _bin_window(walker, take, who)
    parts = [e.waic(k, window, pointwise=pointwise) for k in range(e.K)]
    status = np.bitwise_or.reduce([r["status"] for r in parts])
    which = range(e.n_chains) if chains is None else [chains]
    bad = [c for c in which if status[c] & capi.WAIC_NONFINITE]
    if bad:
        raise FloatingPointError(
            "%s: a model value or a likelihood term is not finite at a step of walker(s) %s: the "
            "reference would have signalled a floating-point trap here" % (who, bad[:8]))
    out = []
    for c in which:
        lppd, p = _serial_sum([r["lppd"][c] for r in parts]), _serial_sum([r["p_waic"][c] for r in parts])
        elpd = lppd - p if len(parts) > 1 else parts[0]["elpd"][c]
        entry = {"elpd": float(elpd), "lppd": float(lppd), "p-waic": float(p), "waic": float(-2.0 * elpd),
                 "n-high": int(sum(int(r["n_high"][c]) for r in parts)),
                 "n-used": int(parts[0]["n_used"][c]), "status": int(status[c])}
        if pointwise:
            pw = np.concatenate([r["pw_lppd"][c] - r["pw_p"][c] for r in parts])
            entry["pointwise"] = pw
            with np.errstate(all="ignore"):
                entry["se"] = float(np.sqrt(pw.size * np.var(pw, ddof=1))) if pw.size > 1 else float("nan")
        out.append(entry)
    return out


def walker_set_waic(walker, take=1000, pointwise=False):
    """Which model should have been fitted: WAIC (Watanabe; Gelman, Hwang and Vehtari 2014) of
    every chain of the set over its newest `take` steps - one device call per function of a global
    fit (mhx_get_waic, which has the definition), no history moved.  A list with, chain by chain,
    {"elpd": the expected log pointwise predictive density lppd - p_waic, "lppd", "p-waic": the
    effective number of parameters, "waic": -2 elpd, "n-high": the points whose variance term
    exceeds 0.4 (the approximation is unreliable there), "n-used": the window, "status": 0 or
    WAIC_ONE_STEP}, the totals summed over the functions.  pointwise=True adds "pointwise", the
    elpd_i of all functions' points one after another, and "se" = sqrt(N var(elpd_i)) (the
    variance with N - 1): what waic_compare takes.  Raises FloatingPointError where a model value
    or a likelihood term of a window is not finite: the reference would have trapped there.  The
    reference has no counterpart: it compares models by eye (walker-plot-residuals)."""
    return _waic(walker, take, pointwise, None, "walker-set-waic")


def walker_waic(walker, chain=0, take=1000, pointwise=False):
    """One chain's entry of walker_set_waic (and only that chain's trap).  The device call is the
    whole set's - there is no per-chain form of mhx_get_waic - and with pointwise=True the
    pointwise arrays of every chain come back before one is picked: for more than a few chains
    call walker_set_waic once and index its result."""
    return _waic(walker, take, pointwise, int(chain), "walker-waic")[0]


def waic_compare(a, b):
    """Two models on the SAME data, from two pointwise results of walker_waic (host arithmetic):
    {"elpd-diff": sum(a_i - b_i), positive where a predicts better, "se": sqrt(N var(a_i - b_i)),
    the standard error of that difference (the variance with N - 1)}.  ValueError unless both
    hold the same number of points."""
    pa = np.asarray(a["pointwise"] if isinstance(a, dict) else a, dtype=np.float64).reshape(-1)
    pb = np.asarray(b["pointwise"] if isinstance(b, dict) else b, dtype=np.float64).reshape(-1)
    if pa.size != pb.size or pa.size < 1:
        raise ValueError("waic_compare: the two results hold %d and %d points: WAIC compares models "
                         "on the same data" % (pa.size, pb.size))
    diff = pa - pb
    with np.errstate(all="ignore"):
        se = float(np.sqrt(diff.size * np.var(diff, ddof=1))) if diff.size > 1 else float("nan")
    return {"elpd-diff": float(np.sum(diff)), "se": se}


loo_compare = waic_compare      # (the same difference and standard error, of two walker_loo results)


def _loo(walker, take, tail, k_limit, pointwise, chains, who):
    e = walker.engine
    window = _bin_window(walker, take, who)
    parts = [e.loo(k, window, tail=0 if tail is None else int(tail), k_limit=k_limit, pointwise=pointwise)
             for k in range(e.K)]
    status = np.bitwise_or.reduce([r["status"] for r in parts])
    which = range(e.n_chains) if chains is None else [chains]
    bad = [c for c in which if status[c] & capi.LOO_NONFINITE]
    if bad:
        raise FloatingPointError(
            "%s: a model value or a likelihood term is not finite at a step of walker(s) %s: the "
            "reference would have signalled a floating-point trap here" % (who, bad[:8]))
    out = []
    for c in which:
        elpd = _serial_sum([r["elpd_loo"][c] for r in parts])
        lppd = _serial_sum([r["lppd"][c] for r in parts])
        p = lppd - elpd if len(parts) > 1 else parts[0]["p_loo"][c]
        entry = {"elpd-loo": float(elpd), "p-loo": float(p), "looic": float(-2.0 * elpd), "lppd": float(lppd),
                 "n-high": int(sum(int(r["n_high"][c]) for r in parts)),
                 "n-used": int(parts[0]["n_used"][c]), "status": int(status[c])}
        if pointwise:
            pw = np.concatenate([r["pw_elpd"][c] for r in parts])
            entry["pointwise"] = pw
            entry["khat"] = np.concatenate([r["pw_khat"][c] for r in parts])
            with np.errstate(all="ignore"):
                entry["se"] = float(np.sqrt(pw.size * np.var(pw, ddof=1))) if pw.size > 1 else float("nan")
        out.append(entry)
    return out


def walker_set_loo(walker, take=1000, tail=None, k_limit=0.7, pointwise=False):
    """Which model should have been fitted, where walker_set_waic's n-high says WAIC cannot tell:
    PSIS-LOO (Vehtari, Gelman and Gabry 2017) of every chain of the set over its newest `take` steps
    - one device call per function of a global fit (mhx_get_loo, which has the definition), no
    history moved.  A list with, chain by chain, {"elpd-loo": the leave-one-out expected log
    pointwise predictive density, "p-loo": lppd - elpd-loo, the effective number of parameters,
    "looic": -2 elpd-loo, "lppd", "n-high": the points whose Pareto khat exceeds k_limit (their
    estimate is unreliable: influential points and outliers), "n-used": the window, "status": a sum
    of LOO_SHORT, LOO_FLAT, LOO_EMPTY}, the totals summed over the functions.  tail: the tail
    length, None for the rule min(n // 5, ceil(3 sqrt n)) - shorten it for an autocorrelated chain.
    pointwise=True adds "pointwise", the elpd_i of all functions' points one after another, "khat"
    beside them and "se" = sqrt(N var(elpd_i)) (the variance with N - 1): what loo_compare takes.
    Raises FloatingPointError where a model value or a likelihood term of a window is not finite."""
    return _loo(walker, take, tail, k_limit, pointwise, None, "walker-set-loo")


def walker_loo(walker, chain=0, take=1000, tail=None, k_limit=0.7, pointwise=False):
    """One chain's entry of walker_set_loo (and only that chain's trap).  The device call is the
    whole set's: for more than a few chains call walker_set_loo once and index its result."""
    return _loo(walker, take, tail, k_limit, pointwise, int(chain), "walker-loo")[0]


def _score_sigma(data_error, n_chains, m):
    """(sigma, sigma_kind, rows [n_chains or 1, m]) of a :data-error for Engine.heldout: None, one
    number, one per point, one per walker, or one list per point per walker (a list of numbers as
    long as the points is taken per point)"""
    if data_error is None:
        return None, capi.SIGMA_NONE, np.ones((1, m))
    sa = np.asarray(data_error, dtype=np.float64)
    if sa.ndim == 0:
        sa = np.full(m, float(sa))
    if sa.shape == (m,):
        return sa, capi.SIGMA_SHARED, sa[None, :]
    if sa.shape == (n_chains,):
        return sa, capi.SIGMA_PER_CHAIN, np.repeat(sa[:, None], m, axis=1)
    if sa.shape == (n_chains, m):
        return sa, capi.SIGMA_PER_POINT, sa
    raise ValueError("data_error must be None, a number, one number per point, one per walker, or one "
                     "list per point per walker")


def _score_data(walker, data, data_error, take, fn_number, pointwise, chains, who, use=None):
    e = walker.engine
    window = _bin_window(walker, take, who)
    x, y = data
    ya = np.asarray(y, dtype=np.float64)
    m = ya.shape[-1]
    sigma, kind, rows = _score_sigma(data_error, e.n_chains, m)
    r = e.heldout(fn_number, window, x, ya, sigma=sigma, sigma_kind=kind, use=use, pointwise=pointwise,
                  accumulators=pointwise)
    which = range(e.n_chains) if chains is None else [chains]
    bad = [c for c in which if r["status"][c] & capi.HELDOUT_NONFINITE]
    if bad:
        raise FloatingPointError(
            "%s: a model value or a likelihood term is not finite at a step of walker(s) %s: the "
            "reference would have signalled a floating-point trap here" % (who, bad[:8]))
    lk = walker.log_liklihood[fn_number]
    lk = lk.lstrip("#':").lower() if isinstance(lk, str) else lk
    normal = (lk is None or isinstance(lk, str)) and _LIKS.get(lk) in (capi.LIK_NORMAL, capi.LIK_NORMAL_CUTOFF)
    out = []
    for c in which:
        entry = {"lpd": float(r["lpd"][c]), "n-scored": int(r["n_scored"][c]), "n-used": int(r["n_used"][c]),
                 "status": int(r["status"][c])}
        if pointwise:
            n = entry["n-used"]
            pw, acc = r["pw_lpd"][c], r["pw_acc"][c]
            used = np.ones(m, dtype=bool) if use is None else (np.asarray(use)[c] if np.ndim(use) == 2
                                                               else np.asarray(use)) != 0
            entry["pointwise"] = pw
            with np.errstate(all="ignore"):
                ps = pw[used]
                entry["se"] = float(np.sqrt(ps.size * np.var(ps, ddof=1))) if ps.size > 1 else float("nan")
                var = acc[:, 3] / np.float64(n - 1)
                entry["fit-mean"], entry["fit-stddev"] = acc[:, 2].copy(), np.sqrt(var)
                if normal:
                    yc = ya[c] if ya.ndim == 2 else ya
                    sc = rows[c if rows.shape[0] > 1 else 0]
                    entry["z-pred"] = (yc - acc[:, 2]) / np.sqrt(sc * sc + var)
        out.append(entry)
    return out


def walker_set_score_data(walker, data, data_error=None, take=1000, fn_number=0, pointwise=False):
    """Scores data the walk did NOT see under every walker's newest `take` steps - a repeated
    measurement, a fold left out of the fit, or (for a set with a dataset per walker, which
    walker_set_waic refuses) each walker's own spectrum: the log pointwise predictive density
    (mhx_get_heldout, which has the definition), one device call, no history moved.  data: [x, y]
    for every walker, or [x, [y per walker]]; data_error None, a number, one per point, one per
    walker or one list per point per walker; the likelihood is function fn_number's own.  A list
    with, walker by walker, {"lpd", "n-scored": the points, "n-used": the window, "status"}.
    pointwise=True adds "pointwise" (lpd_i) and "se" = sqrt(N var(lpd_i)) (the variance with N - 1) -
    what waic_compare takes - and, in host arithmetic that is not bit-defined, "fit-mean" and
    "fit-stddev" (the posterior mean and sqrt(M2 / (n - 1)) of the model at each x) and, for the
    normal likelihoods, "z-pred" = (y - fit-mean) / sqrt(sigma^2 + fit-stddev^2), the predictive
    z-score.  Raises FloatingPointError where a model value or a term of a window is not finite."""
    return _score_data(walker, data, data_error, take, fn_number, pointwise, None, "walker-set-score-data")


def walker_score_data(walker, data, data_error=None, chain=0, take=1000, fn_number=0, pointwise=False):
    """One walker's entry of walker_set_score_data (and only that walker's trap).  The device call
    is the whole set's: for more than a few walkers call walker_set_score_data once."""
    return _score_data(walker, data, data_error, take, fn_number, pointwise, int(chain), "walker-score-data")[0]


def kfold_folds(n, K, scheme=":interleaved"):
    """The fold of each of n points for K-fold cross-validation, an int32 array [n] of 0 .. K-1.
    ":interleaved": point i is in fold i mod K (for a spectrum: every fold spans the whole x range).
    ":blocks": K contiguous runs whose lengths differ by at most one, the longer ones first (for
    data correlated along x).  ValueError unless 1 <= K <= n."""
    n, K = int(n), int(K)
    if n < 1 or K < 1 or K > n:
        raise ValueError("kfold_folds: K = %d folds of n = %d points: 1 <= K <= n is needed" % (K, n))
    s = str(scheme).lstrip(":").lower()
    if s == "interleaved":
        return (np.arange(n) % K).astype(np.int32)
    if s == "blocks":
        base, longer = divmod(n, K)
        return np.repeat(np.arange(K), [base + 1 if k < longer else base for k in range(K)]).astype(np.int32)
    raise ValueError("kfold_folds: scheme must be :interleaved or :blocks, not %r" % (scheme,))


KFOLD_SIGMA_SCALE = 2.0 ** 400


def walker_set_kfold_create(function=None, datasets=None, params=None, data_error=None, K=10,
                            scheme=":interleaved", log_prior=None, **kw):
    """K-fold cross-validation as one walker set: len(datasets) * K walkers, walker s K + k fitting
    dataset s WITHOUT the points of fold k (kfold_folds).  A thin layer over walker_set_create: a
    held-out point keeps its place and gets sigma_i * 2^400 (SIGMA_PER_POINT).  The factor is a
    power of two, so 1 / sigma and y / sigma scale exactly, the point's squared residual is 2^-800
    of its value and vanishes from the walker's sum to the last bit: the walk is the walk on the
    training points alone.  The walker's constant carries -400 log 2 per held-out point, so the
    :log-liklihoods of such walkers are shifted by that much - the same for every step, which no
    walk and no percentile notices.  datasets, params (one plist, or one per dataset) and
    data_error as walker_set_create takes them; the rest of its keywords pass through.  The walker
    remembers w.kfold = {"K", "folds", "sigma": the unscaled stddev [len(datasets), n]}; after the
    walk walker_set_kfold scores every fold under the walker that did not see it."""
    dsets = [list(ds) for ds in datasets]
    lay = planes_layout(dsets, params, data_error)
    n = lay["x"].size
    folds = kfold_folds(n, K, scheme)
    K = int(K)
    each, errors = [], []
    for s, ds in enumerate(dsets):
        for k in range(K):
            each.append(ds)
            errors.append(np.where(folds == k, lay["sigma_rows"][s] * KFOLD_SIGMA_SCALE, lay["sigma_rows"][s]))
    one_plist = isinstance(params, dict) or (len(params) and isinstance(list(params)[0], str))
    w = walker_set_create(function=function, datasets=each,
                          params=params if one_plist else [q for q in params for _ in range(K)],
                          data_error=errors, log_prior=log_prior, **kw)
    w.kfold = {"K": K, "folds": folds, "sigma": np.array(lay["sigma_rows"], dtype=np.float64)}
    return w


def walker_set_kfold(walker, take=1000, pointwise=True):
    """The K-fold estimate of a walker_set_kfold_create set: ONE device call (mhx_get_heldout with a
    `use` mask per walker) scores fold k of dataset s under walker s K + k, which did not see it,
    with the unscaled stddev.  A list with, dataset by dataset, {"elpd-kfold": the K walkers' lpd
    added in fold order, "n-used": their windows, "status": their status bits or-ed}; pointwise=True
    adds "pointwise", every point's held-out lpd exactly once and in x order, and "se" =
    sqrt(N var(lpd_i)) (the variance with N - 1): what waic_compare takes, against another model's
    K-fold result or a walker_waic / walker_loo result on the same points.  Raises
    FloatingPointError where a model value or a term of a window is not finite."""
    kf = getattr(walker, "kfold", None)
    if kf is None or walker.planes is None:
        raise ValueError("walker_set_kfold: the walker was not made by walker_set_kfold_create")
    e, K, folds = walker.engine, kf["K"], kf["folds"]
    n_sets = e.n_chains // K
    window = _bin_window(walker, take, "walker-set-kfold")
    use = np.array([folds == (c % K) for c in range(e.n_chains)], dtype=np.uint8)
    r = e.heldout(0, window, walker.data[0][0], walker.planes["y"], sigma=np.repeat(kf["sigma"], K, axis=0),
                  sigma_kind=capi.SIGMA_PER_POINT, use=use, pointwise=pointwise)
    bad = [c for c in range(e.n_chains) if r["status"][c] & capi.HELDOUT_NONFINITE]
    if bad:
        raise FloatingPointError(
            "walker-set-kfold: a model value or a likelihood term is not finite at a step of walker(s) "
            "%s: the reference would have signalled a floating-point trap here" % (bad[:8],))
    out = []
    for s in range(n_sets):
        mine = slice(s * K, (s + 1) * K)
        entry = {"elpd-kfold": float(_serial_sum(r["lpd"][mine])), "n-used": [int(v) for v in r["n_used"][mine]],
                 "status": int(np.bitwise_or.reduce(r["status"][mine]))}
        if pointwise:
            pw = r["pw_lpd"][s * K + folds, np.arange(folds.size)]
            entry["pointwise"] = pw
            with np.errstate(all="ignore"):
                entry["se"] = float(np.sqrt(pw.size * np.var(pw, ddof=1))) if pw.size > 1 else float("nan")
        out.append(entry)
    return out


def waic_merge(acc, n_used):
    """ONE WAIC from the chains of a set that share their data: pools the accumulators pw_acc
    [n_chains, N, 4] = (M, S, mean, M2) of Engine.waic(..., accumulators=True) over the chains,
    n_used [n_chains] their windows.  (mean, M2) merge by Chan's pairwise update, chain after
    chain; (M, S) by shifting every chain's S to the greatest M.  Host arithmetic in numpy, NOT
    bit-defined: it agrees with one accumulation over the concatenated windows to rounding.  A
    dict of elpd, lppd, p_waic, n (the pooled steps), pw_lppd and pw_p [N]."""
    acc = np.asarray(acc, dtype=np.float64)
    n_used = np.asarray(n_used, dtype=np.int64).reshape(-1)
    if acc.ndim != 3 or acc.shape[2] != 4 or acc.shape[0] != n_used.size or n_used.size < 1:
        raise ValueError("acc must be [n_chains, N, 4] and n_used [n_chains]")
    if (n_used < 1).any():
        raise ValueError("every chain must bring at least one step")
    M = acc[:, :, 0].max(axis=0)
    with np.errstate(all="ignore"):
        S = (acc[:, :, 1] * np.exp(acc[:, :, 0] - M[None, :])).sum(axis=0)
        n, mean, m2 = float(n_used[0]), acc[0, :, 2].copy(), acc[0, :, 3].copy()
        for c in range(1, n_used.size):
            nb = float(n_used[c])
            delta = acc[c, :, 2] - mean
            tot = n + nb
            mean = mean + delta * (nb / tot)
            m2 = m2 + acc[c, :, 3] + delta * delta * (n * nb / tot)
            n = tot
        pw_p = m2 / (n - 1.0)
        pw_lppd = M + np.log(S / n)
    lppd, p = float(np.sum(pw_lppd)), float(np.sum(pw_p))
    return {"elpd": lppd - p, "lppd": lppd, "p_waic": p, "n": int(n), "pw_lppd": pw_lppd, "pw_p": pw_p}


def walker_modify(walker, modify=None, **kw):
    """(walker-modify ...) M:547-580: only :add-step is on the accelerated path and it is
    performed by the device inside walker-take-step; the list-surgery actions are host-side
    post-processing the engine does not take over yet."""
    m = str(modify).lstrip(":").lower()
    if m == "burn-walks":
        walker.engine.modify(m, kw["burn_number"])
    elif m == "keep-walks":
        walker.engine.modify(m, kw["keep_number"])
    elif m in ("reset", "reset-to-most-likely"):
        walker.engine.modify(m)
        return walker
    elif m == "delete":
        walker.engine.close()
    else:  # :add-step happens on the device inside walker-take-step; :add-walks is unused (M:556)
        raise capi.MhxError(capi.EUNSUPPORTED,
                            "walker-modify %s is not part of the accelerated path" % (modify,))
    return None
