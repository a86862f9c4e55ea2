"""Engine: the batched C ABI (include/mhx.h) as a Python object.  Plumbing only -- all
arithmetic happens in libmhx.so's gfx950 kernels."""
import ctypes as C

import numpy as np

from . import _capi as capi


def percentile_ratio(p):
    """a percentile as the (num, den) the ABI takes: the rational walker._percentile uses"""
    from fractions import Fraction
    f = Fraction(p).limit_denominator(1000)
    return f.numerator, f.denominator


def normeq_steps(theta):
    """the default half-widths of normal_equations' central differences: cbrt(2^-52) |theta_t|, the
    step that balances a central difference's truncation against its rounding, with 1.0 in place
    of |theta_t| where theta_t is 0"""
    th = np.abs(np.asarray(theta, dtype=np.float64))
    return np.cbrt(2.0 ** -52) * np.where(th == 0.0, 1.0, th)


class _Summaries:
    """walker-set-get's batched read-backs (include/mhx.h): every chain in one launch.  Shared by
    Engine (mhx_get_*) and Group (mhx_group_get_*)."""
    _summary_prefix = "mhx_get_"

    def _summary(self, name):
        return getattr(capi.lib(), self._summary_prefix + name)

    def percentiles(self, take, pcts):
        """[n_chains, len(pcts), d] nth-percentile of every parameter over the newest `take`
        steps, and n_used [n_chains]; pcts: numbers (50, 2.5, ...) or (num, den) pairs"""
        rat = [p if isinstance(p, tuple) else percentile_ratio(p) for p in pcts]
        num, nump = capi.as_i32([r[0] for r in rat] or [0])
        den, denp = capi.as_i32([r[1] for r in rat] or [1])
        out = np.zeros((self.n_chains, len(rat), self.d))
        used = np.zeros(self.n_chains, dtype=np.int32)
        capi.check(self._summary("percentiles")(self._h, int(take), nump, denp, len(rat),
                                                out.ctypes.data_as(capi.f64p),
                                                used.ctypes.data_as(capi.i32p)))
        return out, used

    def covariances(self, take):
        """:covariance-matrix of every chain: cov [n_chains, d, d], n_unique, status"""
        cov = np.zeros((self.n_chains, self.d, self.d))
        nu = np.zeros(self.n_chains, dtype=np.int32)
        st = np.zeros(self.n_chains, dtype=np.int32)
        capi.check(self._summary("covariances")(self._h, int(take), cov.ctypes.data_as(capi.f64p),
                                                nu.ctypes.data_as(capi.i32p),
                                                st.ctypes.data_as(capi.i32p)))
        return cov, nu, st

    def proposal_factors(self, take):
        """:l-matrix of every chain: status [n_chains], L [n_chains, d, d], n_forward"""
        L = np.zeros((self.n_chains, self.d, self.d))
        st = np.zeros(self.n_chains, dtype=np.int32)
        nf = np.zeros(self.n_chains, dtype=np.int32)
        capi.check(self._summary("proposal_factors")(self._h, int(take),
                                                     L.ctypes.data_as(capi.f64p),
                                                     st.ctypes.data_as(capi.i32p),
                                                     nf.ctypes.data_as(capi.i32p)))
        return st, L, nf

    def window_best(self, take):
        """:most-likely-step over the window, every chain: prob [n_chains], theta [n_chains, d]"""
        pr = np.zeros(self.n_chains)
        th = np.zeros((self.n_chains, self.d))
        capi.check(self._summary("window_best")(self._h, int(take), pr.ctypes.data_as(capi.f64p),
                                                th.ctypes.data_as(capi.f64p)))
        return pr, th


    def fit_bands(self, fn, take, x=None, m=None):
        """walker-get-data-and-fit's envelopes for every chain (mhx_get_fit_bands): the greatest
        and smallest value of function `fn` over each chain's band_count(take) most probable
        steps, at the points x ([m] or [n_cols, m]; None: the function's own dataset x, `m` its
        point count).  Returns ymax [n_chains, m], ymin [n_chains, m], n_selected, status."""
        xa, xp, n_cols, m = _x_columns(self, fn, x, m)
        ymax = np.zeros((self.n_chains, m))
        ymin = np.zeros((self.n_chains, m))
        nsel = np.zeros(self.n_chains, dtype=np.int32)
        st = np.zeros(self.n_chains, dtype=np.int32)
        capi.check(self._summary("fit_bands")(self._h, int(fn), int(take), xp, n_cols, m,
                                              ymax.ctypes.data_as(capi.f64p),
                                              ymin.ctypes.data_as(capi.f64p),
                                              nsel.ctypes.data_as(capi.i32p),
                                              st.ctypes.data_as(capi.i32p)))
        return ymax, ymin, nsel, st

    def fit_percentiles(self, fn, take, xs=None, pcts=((5, 2), (50, 1), (195, 2)), m=None):
        """the pointwise posterior of the fit curve of every chain (mhx_get_fit_percentiles, which
        has the definition): at each of the points xs ([m] or [n_cols, m]; None: the function's
        own dataset x, `m` its point count) the percentiles pcts - numbers or (num, den) pairs, by
        default the 2.5, 50 and 97.5 per cent points - the mean and the standard deviation of
        function `fn` over each chain's newest `take` steps.  Returns pct [n_chains, len(pcts), m],
        mean and stddev [n_chains, m], n_used [n_chains] and status [n_chains] (a sum of
        FITPCT_NONFINITE 1, FITPCT_ONE_STEP 2, FITPCT_EMPTY 4)."""
        xa, xp, n_cols, m = _x_columns(self, fn, xs, m)
        rat = [p if isinstance(p, tuple) else percentile_ratio(p) for p in pcts]
        num, nump = capi.as_i32([r[0] for r in rat] or [0])
        den, denp = capi.as_i32([r[1] for r in rat] or [1])
        pct = np.zeros((self.n_chains, len(rat), m))
        mean, sd = np.zeros((self.n_chains, m)), np.zeros((self.n_chains, m))
        used = np.zeros(self.n_chains, dtype=np.int32)
        st = np.zeros(self.n_chains, dtype=np.int32)
        capi.check(self._summary("fit_percentiles")(
            self._h, int(fn), int(take), xp, n_cols, m, nump, denp, len(rat),
            pct.ctypes.data_as(capi.f64p), mean.ctypes.data_as(capi.f64p), sd.ctypes.data_as(capi.f64p),
            used.ctypes.data_as(capi.i32p), st.ctypes.data_as(capi.i32p)))
        return pct, mean, sd, used, st

    def derived(self, exprs, names, index, take, percentiles=(), values=False):
        """walker-with-exp for every step of every chain, and its posterior (mhx_get_derived): the
        C-syntax expressions `exprs` over names[i] = theta[index[i]] (and `prob`) on each chain's
        newest `take` steps.  A dict of at_most_likely [n_chains, n_expr] (the expression at the
        chain's most-likely step), pct [n_chains, len(percentiles), n_expr], mean and stddev
        [n_chains, n_expr] (stddev is NaN for a one-step window), n_used [n_chains], status
        [n_chains, n_expr] (1: a value of the window is not finite) and, with values=True, values
        [n_chains, n_expr, take] newest first (NaN beyond n_used).  percentiles: numbers or
        (num, den) pairs, as for percentiles()."""
        exprs, names = list(exprs), list(names)
        rat = [p if isinstance(p, tuple) else percentile_ratio(p) for p in percentiles]
        num, nump = capi.as_i32([r[0] for r in rat] or [0])
        den, denp = capi.as_i32([r[1] for r in rat] or [1])
        idx, idxp = capi.as_i32(list(index) or [0])
        ex = (C.c_char_p * max(len(exprs), 1))(*[t.encode() for t in exprs])
        nm = (C.c_char_p * max(len(names), 1))(*[t.encode() for t in names])
        n, ne = self.n_chains, len(exprs)
        out = {"at_most_likely": np.zeros((n, ne)), "pct": np.zeros((n, len(rat), ne)),
               "mean": np.zeros((n, ne)), "stddev": np.zeros((n, ne)),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, ne), dtype=np.int32)}
        vp = None
        if values:
            out["values"] = np.full((n, ne, int(take)), np.nan)
            vp = out["values"].ctypes.data_as(capi.f64p)
        capi.check(self._summary("derived")(
            self._h, ex, ne, nm, idxp, len(names), int(take), nump, denp, len(rat),
            out["at_most_likely"].ctypes.data_as(capi.f64p), out["pct"].ctypes.data_as(capi.f64p),
            out["mean"].ctypes.data_as(capi.f64p), out["stddev"].ctypes.data_as(capi.f64p), vp,
            out["n_used"].ctypes.data_as(capi.i32p), out["status"].ctypes.data_as(capi.i32p)))
        return out

    def _bin_args(self, cols, edges):
        cols = [int(c) for c in cols]
        ea = np.ascontiguousarray(edges, dtype=np.float64)
        if ea.ndim not in (2, 3) or ea.shape[-2] != len(cols) or \
                (ea.ndim == 3 and ea.shape[0] != self.n_chains):
            raise ValueError("edges must be [n_cols, n_bins + 1] or [n_chains, n_cols, n_bins + 1], "
                             "not %r for %d columns" % (ea.shape, len(cols)))
        return cols, ea, int(ea.shape[-1]) - 1, int(ea.ndim == 3)

    def histograms(self, take, cols, edges):
        """make-histo's counts (M:1541-1557) of the parameters `cols` over every chain's newest
        `take` steps (mhx_get_histograms).  edges: [n_cols, n_bins + 1], one set for every chain,
        or [n_chains, n_cols, n_bins + 1]; a value v falls in bin n = the smallest n in 1..n_bins
        with v <= edges[n].  A dict of counts [n_chains, n_cols, n_bins], outside [n_chains,
        n_cols, 2] (below edges[0], above edges[-1]), n_used [n_chains] and status [n_chains,
        n_cols] (1: the column held a NaN, which is counted nowhere)."""
        cols, ea, nb, per_chain = self._bin_args(cols, edges)
        ca, colp = capi.as_i32(cols or [0])
        n, nc = self.n_chains, len(cols)
        out = {"counts": np.zeros((n, nc, nb), dtype=np.int32), "outside": np.zeros((n, nc, 2), dtype=np.int32),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, nc), dtype=np.int32)}
        capi.check(self._summary("histograms")(
            self._h, int(take), colp, nc, nb, ea.ctypes.data_as(capi.f64p), per_chain,
            *(out[k].ctypes.data_as(capi.i32p) for k in ("counts", "outside", "n_used", "status"))))
        return out

    def pair_grids(self, take, cols, pairs, edges):
        """the joint counts of parameter pairs over every chain's newest `take` steps
        (mhx_get_pair_grids): the corner plot as grids.  pairs: (a, b) places in `cols`; edges
        and the bin rule as for histograms().  A dict of counts [n_chains, n_pairs, n_bins,
        n_bins] (cell [i, j]: cols[a] in bin i+1 and cols[b] in bin j+1), n_inside [n_chains,
        n_pairs], n_used [n_chains] and status [n_chains, n_pairs] (1: either column held a NaN)."""
        cols, ea, nb, per_chain = self._bin_args(cols, edges)
        pairs = [(int(a), int(b)) for a, b in pairs]
        ca, colp = capi.as_i32(cols or [0])
        pa, pap = capi.as_i32([a for a, _ in pairs] or [0])
        pb, pbp = capi.as_i32([b for _, b in pairs] or [0])
        n, nc, npairs = self.n_chains, len(cols), len(pairs)
        out = {"counts": np.zeros((n, npairs, nb, nb), dtype=np.int32),
               "n_inside": np.zeros((n, npairs), dtype=np.int32),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, npairs), dtype=np.int32)}
        capi.check(self._summary("pair_grids")(
            self._h, int(take), colp, nc, pap, pbp, npairs, nb, ea.ctypes.data_as(capi.f64p), per_chain,
            *(out[k].ctypes.data_as(capi.i32p) for k in ("counts", "n_inside", "n_used", "status"))))
        return out

    def autocorr(self, take, cols, max_lag, acf=False):
        """how much every chain's newest `take` steps of the parameters `cols` are worth
        (mhx_get_autocorr, which has the definitions): a dict of tau and ess [n_chains, n_cols] -
        the integrated autocorrelation time by Geyer's initial positive sequence over lags up to
        max_lag, and n_used / tau - status [n_chains, n_cols] (AUTOCORR_NONFINITE 1, _CONSTANT 2,
        _OPEN 4: max_lag was too small, tau is a lower bound), n_lags and n_used [n_chains], and
        the moments of the window's two halves, half_mean and half_var [n_chains, n_cols, 2], for
        split_rhat() - NaN where a window has fewer than two steps.  acf=True adds acf [n_chains,
        n_cols, max_lag + 1], NaN beyond n_lags."""
        cols = [int(c) for c in cols]
        ca, colp = capi.as_i32(cols or [0])
        n, nc = self.n_chains, len(cols)
        out = {"tau": np.zeros((n, nc)), "ess": np.zeros((n, nc)),
               "n_lags": np.zeros(n, dtype=np.int32),
               "half_mean": np.full((n, nc, 2), np.nan), "half_var": np.full((n, nc, 2), np.nan),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, nc), dtype=np.int32)}
        if acf:
            out["acf"] = np.full((n, nc, int(max_lag) + 1), np.nan)
        capi.check(self._summary("autocorr")(
            self._h, int(take), colp, nc, int(max_lag),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None
              for k in ("tau", "ess", "acf", "half_mean", "half_var")),
            *(out[k].ctypes.data_as(capi.i32p) for k in ("n_lags", "n_used", "status"))))
        return out

    def _hdi_outputs(self, masses, nc, ladder):
        rat = [m if isinstance(m, tuple) else percentile_ratio(m) for m in masses]
        n, nm, L = self.n_chains, len(rat), int(ladder)
        out = {"lo": np.zeros((n, nm, nc)), "hi": np.zeros((n, nm, nc)),
               "pos": np.zeros((n, nm, nc), dtype=np.int32), "ladder": np.zeros((n, nc, L)),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, nc), dtype=np.int32)}
        num, nump = capi.as_i32([r[0] for r in rat] or [0])
        den, denp = capi.as_i32([r[1] for r in rat] or [1])
        args = (nump, denp, nm, L, out["lo"].ctypes.data_as(capi.f64p), out["hi"].ctypes.data_as(capi.f64p),
                out["pos"].ctypes.data_as(capi.i32p), out["ladder"].ctypes.data_as(capi.f64p),
                out["n_used"].ctypes.data_as(capi.i32p), out["status"].ctypes.data_as(capi.i32p))
        return out, args, (num, den)

    def hdi(self, take, masses, cols=None, ladder=0):
        """the highest-density intervals of the parameters `cols` (None: all, in order) over every
        chain's newest `take` steps (mhx_get_hdi, which has the definition): for each mass - a
        number of per cent or a (num, den) pair, as for percentiles() - the narrowest interval
        between two order statistics that holds it.  A dict of lo, hi and pos [n_chains,
        len(masses), n_cols] (pos: the rank of lo in the sorted window), ladder [n_chains, n_cols,
        ladder] (the sorted window at `ladder` evenly spaced ranks: 0, or 2..4096), n_used
        [n_chains] and status [n_chains, n_cols] (1: the column holds a value that is not finite;
        its lo, hi and pos are then unspecified)."""
        cols = list(range(self.d)) if cols is None else [int(c) for c in cols]
        ca, colp = capi.as_i32(cols or [0])
        out, args, keep = self._hdi_outputs(masses, len(cols), ladder)
        capi.check(self._summary("hdi")(self._h, int(take), colp, len(cols), *args))
        return out

    def derived_hdi(self, exprs, names, index, take, masses, ladder=0):
        """hdi() of derived quantities (mhx_get_derived_hdi): the expressions of derived() in the
        columns' place, expression k as column k."""
        exprs, names = list(exprs), list(names)
        idx, idxp = capi.as_i32(list(index) or [0])
        ex = (C.c_char_p * max(len(exprs), 1))(*[t.encode() for t in exprs])
        nm = (C.c_char_p * max(len(names), 1))(*[t.encode() for t in names])
        out, args, keep = self._hdi_outputs(masses, len(exprs), ladder)
        capi.check(self._summary("derived_hdi")(self._h, ex, len(exprs), nm, idxp, len(names), int(take), *args))
        return out

    def ensemble_percentiles(self, take, pcts, cols=None, include=None):
        """ONE posterior from all chains (mhx_get_ensemble_percentiles, which has the definitions):
        nth-percentile of the pool of every included chain's newest `take` steps, for the
        parameters `cols` (None: all, in order).  include: [n_chains] truth values, None: every
        chain.  A dict of out [len(pcts), n_cols], n_pooled (the pool's size), n_used [n_chains]
        (0 for an excluded chain) and status [n_cols] (1: the pool's column holds a NaN).  pcts:
        numbers or (num, den) pairs, as for percentiles()."""
        rat = [p if isinstance(p, tuple) else percentile_ratio(p) for p in pcts]
        num, nump = capi.as_i32([r[0] for r in rat] or [0])
        den, denp = capi.as_i32([r[1] for r in rat] or [1])
        cols = list(range(self.d)) if cols is None else [int(c) for c in cols]
        ca, colp = capi.as_i32(cols or [0])
        incp = None
        if include is not None:
            inc = np.ascontiguousarray(np.asarray(include).astype(bool), dtype=np.uint8)
            if inc.shape != (self.n_chains,):
                raise ValueError("include must be [n_chains = %d], not %r" % (self.n_chains, inc.shape))
            incp = inc.ctypes.data_as(capi.u8p)
        out = {"out": np.zeros((len(rat), len(cols))), "n_used": np.zeros(self.n_chains, dtype=np.int32),
               "status": np.zeros(len(cols), dtype=np.int32)}
        pooled = C.c_int64(0)
        capi.check(self._summary("ensemble_percentiles")(
            self._h, int(take), colp, len(cols), incp, nump, denp, len(rat),
            out["out"].ctypes.data_as(capi.f64p), C.byref(pooled), out["n_used"].ctypes.data_as(capi.i32p),
            out["status"].ctypes.data_as(capi.i32p)))
        out["n_pooled"] = pooled.value
        return out

    def waic(self, fn, take, pointwise=False, accumulators=False):
        """WAIC of every chain for function `fn` over the newest `take` steps (mhx_get_waic, which
        has the definition): a dict of elpd, lppd, p_waic [n_chains] (waic = -2 elpd), n_high
        [n_chains] (points whose variance term exceeds 0.4), n_used and status [n_chains]
        (WAIC_NONFINITE 1, WAIC_ONE_STEP 2).  pointwise=True adds pw_lppd and pw_p [n_chains, N];
        accumulators=True adds pw_acc [n_chains, N, 4], the (M, S, mean, M2) waic_merge pools."""
        n = self.n_chains
        pts = getattr(self, "_datasets", {}).get(int(fn), (0, 1))[0]
        if (pointwise or accumulators) and pts < 1:
            raise ValueError("waic: function %d has no dataset set through this object" % int(fn))
        out = {"elpd": np.zeros(n), "lppd": np.zeros(n), "p_waic": np.zeros(n),
               "n_high": np.zeros(n, dtype=np.int32), "n_used": np.zeros(n, dtype=np.int32),
               "status": np.zeros(n, dtype=np.int32)}
        if pointwise:
            out["pw_lppd"] = np.zeros((n, pts))
            out["pw_p"] = np.zeros((n, pts))
        if accumulators:
            out["pw_acc"] = np.zeros((n, pts, 4))
        capi.check(self._summary("waic")(
            self._h, int(fn), int(take),
            *(out[k].ctypes.data_as(capi.f64p) for k in ("elpd", "lppd", "p_waic")),
            out["n_high"].ctypes.data_as(capi.i32p),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None for k in ("pw_lppd", "pw_p", "pw_acc")),
            out["n_used"].ctypes.data_as(capi.i32p), out["status"].ctypes.data_as(capi.i32p)))
        return out

    def loo(self, fn, take, tail=0, k_limit=0.7, pointwise=False, accumulators=False):
        """PSIS-LOO of every chain for function `fn` over the newest `take` steps (mhx_get_loo, which
        has the definition): a dict of elpd_loo, p_loo, lppd [n_chains] (looic = -2 elpd_loo), n_high
        [n_chains] (points whose Pareto khat exceeds k_limit), n_used and status [n_chains] (LOO_NONFINITE
        1, LOO_SHORT 2, LOO_FLAT 4, LOO_EMPTY 8).  tail: the tail length, 0 for the rule
        (loo_tail_length).  pointwise=True adds pw_elpd, pw_khat and pw_lppd [n_chains, N];
        accumulators=True adds pw_acc [n_chains, N, 4] = (T_1, l_cut, S_b, sigma) and tail
        [n_chains, N, P], T_1 .. T_M ascending and NaN beyond, P = loo_tail_length(take, tail)."""
        n = self.n_chains
        pts = getattr(self, "_datasets", {}).get(int(fn), (0, 1))[0]
        if (pointwise or accumulators) and pts < 1:
            raise ValueError("loo: function %d has no dataset set through this object" % int(fn))
        out = {"elpd_loo": np.zeros(n), "p_loo": np.zeros(n), "lppd": np.zeros(n),
               "n_high": np.zeros(n, dtype=np.int32), "n_used": np.zeros(n, dtype=np.int32),
               "status": np.zeros(n, dtype=np.int32)}
        if pointwise:
            for k in ("pw_elpd", "pw_khat", "pw_lppd"):
                out[k] = np.zeros((n, pts))
        if accumulators:
            out["pw_acc"] = np.zeros((n, pts, 4))
            ok = int(take) >= 0 and 0 <= int(tail) <= capi.LOO_MAX_TAIL     # (else the call itself refuses)
            out["tail"] = np.zeros((n, pts, loo_tail_length(int(take), int(tail)) if ok else 0))
        capi.check(self._summary("loo")(
            self._h, int(fn), int(take), int(tail), float(k_limit),
            *(out[k].ctypes.data_as(capi.f64p) for k in ("elpd_loo", "p_loo", "lppd")),
            *(out[k].ctypes.data_as(capi.i32p) for k in ("n_high", "n_used", "status")),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None
              for k in ("pw_elpd", "pw_khat", "pw_lppd", "pw_acc", "tail"))))
        return out

    def heldout(self, fn, take, x, y, sigma=None, sigma_kind=None, use=None, pointwise=False,
                accumulators=False, y_per_chain=None, use_per_chain=None):
        """The log pointwise predictive density of data the caller hands in - a fold left out of the
        fit, a repeated measurement, a walker's own spectrum - under every chain's newest `take`
        steps of function `fn` (mhx_get_heldout, which has the definition).  x [m] or [n_cols, m],
        shared by the chains; y [m] or [n_chains, m]; sigma None, a number or [m] (SIGMA_SHARED),
        [n_chains] (SIGMA_PER_CHAIN) or [n_chains, m] (SIGMA_PER_POINT); use None (every point), [m]
        or [n_chains, m]: chain c scores point i where its entry is nonzero.  The kinds are read off
        the shapes unless given (a sigma of one dimension whose length fits both is SIGMA_SHARED).
        A dict of lpd [n_chains], n_scored (points used), n_used (steps) and status [n_chains]
        (HELDOUT_NONFINITE 1, HELDOUT_NO_POINTS 2).  pointwise=True adds pw_lpd [n_chains, m];
        accumulators=True adds pw_acc [n_chains, m, 4] = (M, S, mean_v, M2_v), the log-sum-exp pair
        of the terms and the Welford pair of the model values.  A point a chain does not use is 0.0
        everywhere.  An engine with a dataset per walker is served."""
        n = self.n_chains
        xa, xp, n_cols, m = _x_columns(self, fn, np.asarray(x, dtype=np.float64), None)
        ya, yp = capi.as_f64(y)
        if y_per_chain is None:
            y_per_chain = ya.ndim == 2
        if ya.shape != ((n, m) if y_per_chain else (m,)):
            raise ValueError("y must be [m] or [n_chains, m] with m = %d, n_chains = %d" % (m, n))
        sa, sp = None, None
        if sigma is None:
            if sigma_kind not in (None, capi.SIGMA_NONE):
                raise ValueError("sigma is None exactly with SIGMA_NONE")
            sigma_kind = capi.SIGMA_NONE
        else:
            sa = np.asarray(sigma, dtype=np.float64)
            if sigma_kind is None:
                if sa.ndim == 0:
                    sa = np.full(m, float(sa))
                sigma_kind = (capi.SIGMA_PER_POINT if sa.ndim == 2 else
                              capi.SIGMA_SHARED if sa.shape == (m,) else capi.SIGMA_PER_CHAIN)
            want = {capi.SIGMA_SHARED: (m,), capi.SIGMA_PER_CHAIN: (n,), capi.SIGMA_PER_POINT: (n, m)}
            if sigma_kind not in want or sa.shape != want[sigma_kind]:
                raise ValueError("sigma must be [m], [n_chains] or [n_chains, m] by its sigma_kind")
            sa, sp = capi.as_f64(sa)
        ua, up = None, None
        if use is not None:
            ua = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
            if use_per_chain is None:
                use_per_chain = ua.ndim == 2
            if ua.shape != ((n, m) if use_per_chain else (m,)):
                raise ValueError("use must be [m] or [n_chains, m]")
            up = ua.ctypes.data_as(capi.u8p)
        out = {"lpd": np.zeros(n), "n_scored": np.zeros(n, dtype=np.int32),
               "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros(n, dtype=np.int32)}
        if pointwise:
            out["pw_lpd"] = np.zeros((n, m))
        if accumulators:
            out["pw_acc"] = np.zeros((n, m, 4))
        capi.check(self._summary("heldout")(
            self._h, int(fn), int(take), xp, n_cols, m, yp, int(bool(y_per_chain)), sp, int(sigma_kind),
            up, int(bool(use_per_chain)), out["lpd"].ctypes.data_as(capi.f64p),
            out["n_scored"].ctypes.data_as(capi.i32p),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None for k in ("pw_lpd", "pw_acc")),
            out["n_used"].ctypes.data_as(capi.i32p), out["status"].ctypes.data_as(capi.i32p)))
        return out

    def residuals(self, fn, theta=None, z_limit=3.0, pointwise=False):
        """Goodness of fit of every walker for function `fn` at one parameter vector each
        (mhx_get_residuals, which has the definition): theta [n_chains, d], None: every chain's
        most-likely parameters.  A dict of chi2, sum_z, dw (the sums of z^2, z and
        (z_i - z_{i-1})^2 of the standardized residuals z, fit minus data), max_abs_z and
        max_index (the greatest |z| and its point), n_pos, n_runs (the runs of equal sign), n_out
        (points with |z| > z_limit) and status (RESID_NONFINITE 1), all [n_chains].
        pointwise=True adds fit and z [n_chains, N]."""
        n = self.n_chains
        pts = getattr(self, "_datasets", {}).get(int(fn), (0, 1))[0]
        if pointwise and pts < 1:
            raise ValueError("residuals: function %d has no dataset set through this object" % int(fn))
        thp = None
        if theta is not None:
            th = np.ascontiguousarray(theta, dtype=np.float64)
            if th.shape != (n, self.d):
                raise ValueError("residuals: theta must be [n_chains, d] = [%d, %d]" % (n, self.d))
            thp = th.ctypes.data_as(capi.f64p)
        out = {k: np.zeros(n) for k in ("chi2", "sum_z", "dw", "max_abs_z")}
        out["max_index"] = np.zeros(n, dtype=np.int64)
        for k in ("n_pos", "n_runs", "n_out", "status"):
            out[k] = np.zeros(n, dtype=np.int32)
        if pointwise:
            out["fit"] = np.zeros((n, pts))
            out["z"] = np.zeros((n, pts))
        capi.check(self._summary("residuals")(
            self._h, int(fn), thp, float(z_limit),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None for k in ("fit", "z")),
            *(out[k].ctypes.data_as(capi.f64p) for k in ("chi2", "sum_z", "dw", "max_abs_z")),
            out["max_index"].ctypes.data_as(capi.i64p),
            *(out[k].ctypes.data_as(capi.i32p) for k in ("n_pos", "n_runs", "n_out", "status"))))
        return out

    def normal_equations(self, fn, theta=None, steps=None, pointwise=False):
        """The normal equations of every walker's least-squares problem for function `fn` at one
        parameter vector each (mhx_get_normal_equations, which has the definition): theta
        [n_chains, d], None: every chain's most-likely parameters; steps the half-widths of the
        central differences, [d] for all chains or [n_chains, d], None: normeq_steps(theta); a step
        of 0 leaves that parameter out (its row and column are +0.0).  A dict of jtj [n_chains, d,
        d] (g^T g of the scaled Jacobian g, the Fisher matrix), jtr [n_chains, d] (g^T u with u
        the weighted residual data minus fit: F delta = jtr is the Gauss-Newton step), chi2 (u^T u)
        and status (NORMEQ_NONFINITE 1) [n_chains].  pointwise=True adds g [n_chains, d, N]."""
        n, d = self.n_chains, self.d
        pts = getattr(self, "_datasets", {}).get(int(fn), (0, 1))[0]
        if pointwise and pts < 1:
            raise ValueError("normal_equations: function %d has no dataset set through this object" % int(fn))
        thp = None
        if theta is not None:
            th = np.ascontiguousarray(theta, dtype=np.float64)
            if th.shape != (n, d):
                raise ValueError("normal_equations: theta must be [n_chains, d] = [%d, %d]" % (n, d))
            thp = th.ctypes.data_as(capi.f64p)
        if steps is None:
            steps = normeq_steps(th if theta is not None else self.state()["best_theta"])
        hs = np.ascontiguousarray(steps, dtype=np.float64)
        if hs.shape not in ((d,), (n, d)):
            raise ValueError("normal_equations: steps must be [d] or [n_chains, d]")
        out = {"jtj": np.zeros((n, d, d)), "jtr": np.zeros((n, d)), "chi2": np.zeros(n),
               "status": np.zeros(n, dtype=np.int32)}
        if pointwise:
            out["g"] = np.zeros((n, d, pts))
        capi.check(self._summary("normal_equations")(
            self._h, int(fn), thp, hs.ctypes.data_as(capi.f64p), int(hs.ndim == 2),
            *(out[k].ctypes.data_as(capi.f64p) for k in ("jtj", "jtr", "chi2")),
            out["g"].ctypes.data_as(capi.f64p) if pointwise else None,
            out["status"].ctypes.data_as(capi.i32p)))
        return out

    def candidate_scores(self, cand, fn=-1, keep=1, scores=False):
        """The chi-square of many parameter vectors per walker, ranked on the device
        (mhx_get_candidate_scores, which has the definition): cand [m, d], tried by every chain,
        or [n_chains, m, d], each chain's own; fn a function, -1: the sum over all of them; keep in
        1 .. CAND_KEEP_MAX.  A dict of best_index, best_score [n_chains, keep] (ascending (score,
        index); index -1 and +inf where m < keep), n_bad [n_chains] (candidates whose score is not
        finite: they score +inf) and, with scores=True, score [n_chains, m]."""
        n, d = self.n_chains, self.d
        cd = np.ascontiguousarray(cand, dtype=np.float64)
        if not ((cd.ndim == 2 and cd.shape[1] == d) or (cd.ndim == 3 and cd.shape[0] == n and cd.shape[2] == d)):
            raise ValueError("candidate_scores: cand must be [m, d] or [n_chains, m, d] with n_chains = %d, d = %d"
                             % (n, d))
        m = cd.shape[-2]
        if m < 1:
            raise ValueError("candidate_scores: no candidates")
        keep = int(keep)
        if not 1 <= keep <= capi.CAND_KEEP_MAX:
            raise ValueError("candidate_scores: keep must be in 1 .. %d" % capi.CAND_KEEP_MAX)
        out = {"best_index": np.zeros((n, keep), dtype=np.int32), "best_score": np.zeros((n, keep)),
               "n_bad": np.zeros(n, dtype=np.int32)}
        if scores:
            out["score"] = np.zeros((n, m))
        capi.check(self._summary("candidate_scores")(
            self._h, int(fn), cd.ctypes.data_as(capi.f64p), m, int(cd.ndim == 3), keep,
            out["score"].ctypes.data_as(capi.f64p) if scores else None,
            out["best_index"].ctypes.data_as(capi.i32p), out["best_score"].ctypes.data_as(capi.f64p),
            out["n_bad"].ctypes.data_as(capi.i32p)))
        return out

    TRACE_FILTERS ={"steps": capi.TRACE_STEPS, "unique": capi.TRACE_UNIQUE, "forward": capi.TRACE_FORWARD}

    def traces(self, take, cols=None, filter="steps", stride=1, start=0, max_out=None, envelope=False):
        """every chain's steps, filtered and thinned on the device (mhx_get_traces, which has the
        definitions).  cols: parameter indices, capi.TRACE_PROB (-1) for a step's prob; None:
        [TRACE_PROB, 0 .. d-1].  filter: "steps", "unique" or "forward" (or a capi.TRACE_*);
        stride, start: every stride-th kept step from the start-th on, newest first; max_out: rows
        to return, None: trace_rows(take, stride, start), all there can be.  A dict of values
        [n_chains, max_out, n_cols] (rows from n_out on are zero), n_out, n_kept, n_used
        [n_chains] and, with envelope=True, lo and hi as values: the extremes of each row's
        bucket of `stride` kept steps."""
        cols = [capi.TRACE_PROB] + list(range(self.d)) if cols is None else [int(c) for c in cols]
        flt = self.TRACE_FILTERS.get(str(filter).lstrip(":").lower().replace("-steps", ""), filter)
        if max_out is None:  # (arguments the library will refuse are left for it to name)
            ok = int(take) >= 0 and int(stride) >= 1 and 0 <= int(start) < int(stride)
            max_out = max(trace_rows(int(take), stride, start), 1) if ok else 1
        ca, colp = capi.as_i32(cols or [0])
        n, nc, rows = self.n_chains, len(cols), max(int(max_out), 0)
        out = {"values": np.zeros((n, rows, nc))}
        if envelope:
            out["lo"], out["hi"] = np.zeros((n, rows, nc)), np.zeros((n, rows, nc))
        for k in ("n_out", "n_kept", "n_used"):
            out[k] = np.zeros(n, dtype=np.int32)
        capi.check(self._summary("traces")(
            self._h, int(take), int(flt), int(stride), int(start), colp, nc, int(max_out),
            *(out[k].ctypes.data_as(capi.f64p) if k in out else None for k in ("values", "lo", "hi")),
            *(out[k].ctypes.data_as(capi.i32p) for k in ("n_out", "n_kept", "n_used"))))
        return out


def trace_rows(n_kept, stride=1, start=0):
    """rows `thin` (M:149-157) leaves of a list of n_kept items: those at start, start + stride,
    ... (mhx_trace_rows: host arithmetic, no device).  ValueError, with the library's message,
    unless n_kept >= 0, stride >= 1 and 0 <= start < stride."""
    rows = C.c_int64(0)
    rc = capi.lib().mhx_trace_rows(int(n_kept), int(stride), int(start), C.byref(rows))
    if rc == capi.EINVAL:
        raise ValueError(capi.lib().mhx_last_error().decode())
    capi.check(rc)
    return rows.value


def hdi_span(n, mass):
    """the span g of a highest-density interval of `mass` per cent - a number or a (num, den) pair -
    among n sorted values: min(floor(n num / (100 den)), n - 1) (mhx_hdi_span: host arithmetic, no
    device).  ValueError, with the library's message, unless n >= 1, 1 <= den <= 10^6 and
    1 <= num <= 100 den."""
    num, den = mass if isinstance(mass, tuple) else percentile_ratio(mass)
    if not (-2 ** 31 <= int(num) < 2 ** 31 and -2 ** 31 <= int(den) < 2 ** 31):
        raise ValueError("the mass %r/%r does not fit the ABI's 32-bit integers" % (num, den))
    g = C.c_int64(0)
    rc = capi.lib().mhx_hdi_span(int(n), int(num), int(den), C.byref(g))
    if rc == capi.EINVAL:
        raise ValueError(capi.lib().mhx_last_error().decode())
    capi.check(rc)
    return g.value


def ensemble_pick(counts, rank):
    """(digit, rank in its bin, the bin's count) of `rank` among the bins `counts`
    (mhx_ensemble_pick: host arithmetic, no device): the smallest digit whose cumulative count
    exceeds rank.  ValueError, with the library's message, unless 0 <= rank < sum(counts)."""
    ca = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    digit, rb, bc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = capi.lib().mhx_ensemble_pick(ca.ctypes.data_as(capi.u64p), int(ca.size), int(rank),
                                      C.byref(digit), C.byref(rb), C.byref(bc))
    if rc == capi.EINVAL:
        raise ValueError(capi.lib().mhx_last_error().decode())
    capi.check(rc)
    return digit.value, rb.value, bc.value


def split_rhat(half_mean, half_var, n_used):
    """split R-hat of every column (mhx_split_rhat: host arithmetic, no device) from the half
    moments [n_chains, n_cols, 2] and n_used [n_chains] as Engine.autocorr returns them.
    ValueError, with the library's message, unless every chain's window has the same half length
    and that is at least 2."""
    hm = np.ascontiguousarray(half_mean, dtype=np.float64)
    hv = np.ascontiguousarray(half_var, dtype=np.float64)
    nu = np.ascontiguousarray(n_used, dtype=np.int32)
    if hm.ndim != 3 or hm.shape[2] != 2 or hv.shape != hm.shape or nu.shape != (hm.shape[0],):
        raise ValueError("half_mean and half_var must be [n_chains, n_cols, 2] and n_used [n_chains], "
                         "not %r, %r, %r" % (hm.shape, hv.shape, nu.shape))
    rhat = np.zeros(hm.shape[1])
    rc = capi.lib().mhx_split_rhat(hm.ctypes.data_as(capi.f64p), hv.ctypes.data_as(capi.f64p),
                                   nu.ctypes.data_as(capi.i32p), hm.shape[0], hm.shape[1],
                                   rhat.ctypes.data_as(capi.f64p))
    if rc == capi.EINVAL:
        raise ValueError(capi.lib().mhx_last_error().decode())
    capi.check(rc)
    return rhat


def band_count(take):
    """(ceiling (* 0.66 take)) M:1250 in the reference's single-float arithmetic (mhx_band_count)"""
    k = C.c_int64(0)
    capi.check(capi.lib().mhx_band_count(int(take), C.byref(k)))
    return k.value


def loo_tail_length(n, tail=0):
    """the tail PSIS-LOO fits in a window of n steps: min(n // 5, ceil(3 sqrt n)), or min(tail, n // 5)
    where tail > 0 shortens it; 0 below 25 steps (mhx_loo_tail_length)"""
    m = C.c_int32(0)
    capi.check(capi.lib().mhx_loo_tail_length(int(n), int(tail), C.byref(m)))
    return m.value


def _x_columns(owner, fn, x, m):
    """(array, pointer, n_cols, m) of the x argument of eval_function / fit_bands; x None: the
    dataset of function fn as set_dataset saw it"""
    if x is None:
        pts, cols = getattr(owner, "_datasets", {}).get(int(fn), (0, 1))
        return None, None, cols, int(pts if m is None else m)
    xa = np.ascontiguousarray(x, dtype=np.float64)
    if xa.ndim == 1:
        xa = xa[None, :]
    return xa, xa.ctypes.data_as(capi.f64p), int(xa.shape[0]), int(xa.shape[1])


def _planes_args(n_chains, x, y, sigma, sigma_kind):
    """the arrays of mhx_set_dataset_planes, checked: x [n], y [n_chains][n], sigma by its kind"""
    xa, xp = capi.as_f64(x)
    ya, yp = capi.as_f64(y)
    if xa.ndim != 1 or ya.shape != (n_chains, xa.size):
        raise ValueError("x must be [n] and y [n_chains][n]")
    want = {capi.SIGMA_NONE: None, capi.SIGMA_SHARED: (xa.size,), capi.SIGMA_PER_CHAIN: (n_chains,),
            capi.SIGMA_PER_POINT: (n_chains, xa.size)}
    if sigma_kind not in want:
        raise ValueError("sigma_kind must be one of SIGMA_NONE, _SHARED, _PER_CHAIN, _PER_POINT")
    sa, sp = None, None
    if (sigma is None) != (want[sigma_kind] is None):
        raise ValueError("sigma is None exactly with SIGMA_NONE")
    if sigma is not None:
        sa, sp = capi.as_f64(sigma)
        if sa.shape != want[sigma_kind]:
            raise ValueError("sigma must be %r for this sigma_kind" % (want[sigma_kind],))
    return (xa, ya, sa), (xp, yp, sp)


class Engine(_Summaries):
    def __init__(self, n_chains, n_params, n_functions=1, device=0, seed=0, chain_offset=0,
                 adapt_mode=capi.ADAPT_FAITHFUL, history_capacity=0, poisson_logfact_double=False):
        cfg = capi.Config()
        cfg.n_chains, cfg.n_params, cfg.n_functions = int(n_chains), int(n_params), int(n_functions)
        cfg.device, cfg.adapt_mode, cfg.seed = int(device), int(adapt_mode), int(seed)
        cfg.chain_offset, cfg.history_capacity = int(chain_offset), int(history_capacity)
        cfg.poisson_logfact_double = int(bool(poisson_logfact_double))
        self.n_chains, self.d, self.K = int(n_chains), int(n_params), int(n_functions)
        self._h = C.c_void_p()
        self._cb = None
        capi.check(capi.lib().mhx_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            capi.lib().mhx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- problem definition (walker-create) -------------------------------
    def set_function(self, k, model, shape=(), param_index=()):
        sh, shp = capi.as_i32(list(shape) if len(shape) else [0])
        ix, ixp = capi.as_i32(list(param_index))
        capi.check(capi.lib().mhx_set_function(self._h, k, model, shp, len(shape), ixp, len(ix)))

    @staticmethod
    def _names(names):
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        return arr

    def set_function_expr(self, k, expr, names, param_index):
        """function k as a C-syntax expression over x and `names` (see include/mhx.h)"""
        ix, ixp = capi.as_i32(list(param_index))
        capi.check(capi.lib().mhx_set_function_expr(self._h, k, expr.encode(), self._names(names),
                                                    ixp, len(ix)))

    def set_expr_recognition(self, on):
        """on=False: every expression of this engine is compiled exactly as written (libmhx
        otherwise serves polynomial + Gaussian / Lorentzian peak bodies with the enumerated
        models' kernels: include/mhx.h, mhx_set_function_expr)"""
        capi.check(capi.lib().mhx_set_expr_recognition(self._h, 1 if on else 0))

    def set_prior_expr(self, k, expr, names, index):
        """body of function k's prior over bounds_total and `names` (global parameter indices)"""
        ix, ixp = capi.as_i32(list(index))
        capi.check(capi.lib().mhx_set_prior_expr(self._h, k, (expr or "").encode(),
                                                 self._names(names), ixp, len(ix)))

    def set_likelihood_expr(self, k, expr):
        """per-point log-likelihood term of function k over y, model, error (dataset k must use
        LIK_EXPR, function k an expression model)"""
        capi.check(capi.lib().mhx_set_likelihood_expr(self._h, k, expr.encode()))

    def set_dataset(self, k, x, y, sigma=None, likelihood=capi.LIK_NORMAL):
        """x: [n], or [n][2] - a vector-valued x, one row per point, as the reference's x list holds
        it (mcmc-fitting.lisp:1136-1137): mhx_set_dataset_cols"""
        xa, xp = capi.as_f64(x)
        ya, yp = capi.as_f64(y)
        # (points, columns of x): what eval_function / fit_bands take for x=None
        self.__dict__.setdefault("_datasets", {})[int(k)] = (int(ya.size), xa.shape[1] if xa.ndim == 2 else 1)
        if xa.ndim == 2 and xa.shape[0] == ya.shape[0] and ya.ndim == 1:
            cols = [np.ascontiguousarray(xa[:, j]) for j in range(xa.shape[1])]
            ptrs = (capi.f64p * len(cols))(*[c.ctypes.data_as(capi.f64p) for c in cols])
            sp = None
            if sigma is not None:
                sa, sp = capi.as_f64(np.broadcast_to(np.asarray(sigma, dtype=np.float64), ya.shape))
            capi.check(capi.lib().mhx_set_dataset_cols(self._h, k, ptrs, len(cols), yp, sp, ya.size,
                                                       likelihood))
            return
        if xa.shape != ya.shape or xa.ndim != 1:
            raise ValueError("x and y must be 1-d and of equal length (or x [n][2])")
        if sigma is None:
            sp = None
        else:
            sa, sp = capi.as_f64(np.broadcast_to(np.asarray(sigma, dtype=np.float64), xa.shape))
        capi.check(capi.lib().mhx_set_dataset(self._h, k, xp, yp, sp, xa.size, likelihood))

    def set_dataset_planes(self, k, x, y, sigma=None, sigma_kind=capi.SIGMA_NONE,
                           likelihood=capi.LIK_NORMAL):
        """a dataset per walker (mhx_set_dataset_planes): x [n] shared, y [n_chains][n], sigma None,
        [n], [n_chains] or [n_chains][n] as sigma_kind says"""
        keep, (xp, yp, sp) = _planes_args(self.n_chains, x, y, sigma, sigma_kind)
        self.__dict__.setdefault("_datasets", {})[int(k)] = (int(keep[0].size), 1)
        capi.check(capi.lib().mhx_set_dataset_planes(self._h, k, xp, yp, sp, sigma_kind, keep[0].size,
                                                     likelihood))

    def set_bounds(self, k, idx, lo, hi):
        ix, ixp = capi.as_i32(list(idx))
        la, lp = capi.as_f64(lo)
        ha, hp = capi.as_f64(hi)
        capi.check(capi.lib().mhx_set_bounds(self._h, k, ixp, lp, hp, len(ix)))

    def init_chains(self, theta0):
        th = np.ascontiguousarray(theta0, dtype=np.float64)
        if th.shape == (self.d,):
            bc = 1
        elif th.shape == (self.n_chains, self.d):
            bc = 0
        else:
            raise ValueError("theta0 must be [d] or [n_chains, d]")
        capi.check(capi.lib().mhx_init_chains(self._h, th.ctypes.data_as(capi.f64p), bc))

    # ---- evaluation / parity hooks ------------------------------------------
    def logpost(self, theta, parts=False):
        th = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, self.d)
        out = np.zeros(th.shape[0])
        pr = np.zeros((th.shape[0], 2))
        capi.check(capi.lib().mhx_logpost(self._h, th.ctypes.data_as(capi.f64p), th.shape[0],
                                          out.ctypes.data_as(capi.f64p),
                                          pr.ctypes.data_as(capi.f64p)))
        return (out, pr) if parts else out

    def step_injected(self, L, z, u, T=None):
        La = np.ascontiguousarray(L, dtype=np.float64)
        per_chain = 1 if La.ndim == 3 else 0
        za = np.ascontiguousarray(z, dtype=np.float64).reshape(self.n_chains, self.d)
        ua = np.ascontiguousarray(u, dtype=np.float64).reshape(self.n_chains)
        Ta = np.ascontiguousarray(np.ones(self.n_chains) if T is None else
                                  np.broadcast_to(np.asarray(T, dtype=np.float64), (self.n_chains,)))
        acc = np.zeros(self.n_chains, dtype=np.uint8)
        capi.check(capi.lib().mhx_step_injected(
            self._h, La.ctypes.data_as(capi.f64p), per_chain, za.ctypes.data_as(capi.f64p),
            ua.ctypes.data_as(capi.f64p), Ta.ctypes.data_as(capi.f64p),
            acc.ctypes.data_as(capi.u8p)))
        return acc

    # ---- controller -----------------------------------------------------------
    def _opts(self, n, temperature, auto, max_walker_length, l_matrix):
        o = capi.RunOpts()
        capi.lib().mhx_run_opts_default(C.byref(o))
        o.n, o.temperature, o.auto_mode = int(n), float(temperature), int(auto)
        o.max_walker_length = int(max_walker_length or 0)
        if l_matrix is not None:
            self._L_keep = np.ascontiguousarray(l_matrix, dtype=np.float64)
            o.l_matrix = self._L_keep.ctypes.data_as(capi.f64p)
            o.l_matrix_per_chain = 1 if self._L_keep.ndim == 3 else 0
        return o

    def adaptive_begin(self, n=100000, temperature=1e3, auto=1, max_walker_length=0,
                       l_matrix=None):
        o = self._opts(n, temperature, auto, max_walker_length, l_matrix)
        capi.check(capi.lib().mhx_adaptive_begin(self._h, C.byref(o)))

    def adaptive_advance(self, max_iters, count=True):
        n = C.c_int64(-1)
        capi.check(capi.lib().mhx_adaptive_advance(self._h, int(max_iters),
                                                   C.byref(n) if count else None))
        return n.value

    def adaptive_steps_full(self, n=100000, temperature=1e3, auto=1, max_walker_length=0,
                            l_matrix=None):
        o = self._opts(n, temperature, auto, max_walker_length, l_matrix)
        capi.check(capi.lib().mhx_adaptive_steps_full(self._h, C.byref(o)))

    def adaptive_steps(self, n=30000):
        capi.check(capi.lib().mhx_adaptive_steps(self._h, int(n)))

    def many_steps(self, n, L):
        La = np.ascontiguousarray(L, dtype=np.float64)
        capi.check(capi.lib().mhx_many_steps(self._h, int(n), La.ctypes.data_as(capi.f64p),
                                             1 if La.ndim == 3 else 0))

    def take_step(self, L, temperature=1.0):
        """(walker-take-step w :l-matrix L :temperature T) for every chain, device randomness"""
        La = np.ascontiguousarray(L, dtype=np.float64)
        capi.check(capi.lib().mhx_take_step(self._h, La.ctypes.data_as(capi.f64p),
                                            1 if La.ndim == 3 else 0, float(temperature)))

    def request_stop(self):
        capi.check(capi.lib().mhx_request_stop(self._h))

    def comm_init_rank(self, unique_id, rank, n_ranks):
        """join the RCCL communicator of a one-process-per-GPU job (collective); unique_id: the
        128 bytes rank 0 got from comm_unique_id()"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        capi.check(capi.lib().mhx_comm_init_rank(self._h, buf, int(rank), int(n_ranks)))

    def set_allreduce(self, fn, device_buffer=False):
        """fn(ptr, n, device_buffer) -> 0; sums n doubles at ptr over all ranks in place."""
        if fn is None:
            self._cb = None
            capi.check(capi.lib().mhx_set_allreduce(self._h, capi.ALLREDUCE_FN(), None, 0))
            return

        def tramp(ctx, buf, n, dev):
            try:
                return int(fn(buf, n, dev) or 0)
            except Exception:  # never let an exception cross the C ABI
                import traceback
                traceback.print_exc()
                return 1
        self._cb = capi.ALLREDUCE_FN(tramp)
        capi.check(capi.lib().mhx_set_allreduce(self._h, self._cb, None, int(device_buffer)))

    # ---- read-back (walker-get) ----------------------------------------------------
    def state(self):
        C_, d = self.n_chains, self.d
        th, bt = np.zeros((C_, d)), np.zeros((C_, d))
        lp, bl = np.zeros(C_), np.zeros(C_)
        ln, ag = np.zeros(C_, dtype=np.int64), np.zeros(C_, dtype=np.int64)
        capi.check(capi.lib().mhx_get_state(
            self._h, th.ctypes.data_as(capi.f64p), lp.ctypes.data_as(capi.f64p),
            bt.ctypes.data_as(capi.f64p), bl.ctypes.data_as(capi.f64p),
            ln.ctypes.data_as(capi.i64p), ag.ctypes.data_as(capi.i64p)))
        return dict(theta=th, logpost=lp, best_theta=bt, best_logpost=bl, length=ln, age=ag)

    def chain(self, c):
        """one chain's state (mhx_get_chain): what the accessors of one walker read"""
        d = self.d
        th, bt = np.zeros(d), np.zeros(d)
        lp, bl = C.c_double(0), C.c_double(0)
        ln, ag = C.c_int64(0), C.c_int64(0)
        capi.check(capi.lib().mhx_get_chain(
            self._h, int(c), th.ctypes.data_as(capi.f64p), C.byref(lp),
            bt.ctypes.data_as(capi.f64p), C.byref(bl), C.byref(ln), C.byref(ag)))
        return dict(theta=th, logpost=lp.value, best_theta=bt, best_logpost=bl.value,
                    length=ln.value, age=ag.value)

    def chain_status(self):
        st = np.zeros(self.n_chains, dtype=np.int32)
        li = np.zeros(self.n_chains, dtype=np.int64)
        capi.check(capi.lib().mhx_get_chain_status(self._h, st.ctypes.data_as(capi.i32p),
                                                   li.ctypes.data_as(capi.i64p)))
        return st, li

    def lmatrix(self):
        L = np.zeros((self.n_chains, self.d, self.d))
        capi.check(capi.lib().mhx_get_lmatrix(self._h, L.ctypes.data_as(capi.f64p)))
        return L

    def temperature(self):
        T = np.zeros(self.n_chains)
        capi.check(capi.lib().mhx_get_temperature(self._h, T.ctypes.data_as(capi.f64p)))
        return T

    def acceptance(self, take):
        out = np.zeros(self.n_chains)
        capi.check(capi.lib().mhx_get_acceptance(self._h, int(take), out.ctypes.data_as(capi.f64p)))
        return out

    def trace(self, chain, take):
        take = int(take)
        prob = np.zeros(max(take, 1))
        th = np.zeros((max(take, 1), self.d))
        n = C.c_int(0)
        capi.check(capi.lib().mhx_get_trace(self._h, int(chain), take,
                                            prob.ctypes.data_as(capi.f64p),
                                            th.ctypes.data_as(capi.f64p), C.byref(n)))
        return prob[:n.value], th[:n.value]

    def proposal_factor(self, chain, take):
        L = np.zeros((self.d, self.d))
        st, nf = C.c_int(0), C.c_int(0)
        capi.check(capi.lib().mhx_get_proposal_factor(self._h, int(chain), int(take),
                                                      L.ctypes.data_as(capi.f64p), C.byref(st),
                                                      C.byref(nf)))
        return st.value, L, nf.value

    def eval_function(self, fn, theta, x=None, m=None, n_cols=None):
        """function `fn` of the problem at the points x ([m] or [n_cols, m]; None: the function's
        own dataset x, `m` its point count) for the full parameter vectors theta [n, d] or [d]:
        [n, m] (or [m]) model values (mhx_eval_function)"""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        one = th.ndim == 1
        th = th.reshape(-1, self.d)
        xa, xp, nc, m = _x_columns(self, fn, x, m)
        out = np.zeros((th.shape[0], m))
        capi.check(capi.lib().mhx_eval_function(self._h, int(fn), th.ctypes.data_as(capi.f64p),
                                                th.shape[0], xp, nc if n_cols is None else n_cols,
                                                m, out.ctypes.data_as(capi.f64p)))
        return out[0] if one else out

    def history_capacity(self):
        """steps the device ring of every chain holds: the greatest `take`"""
        n = C.c_int32(0)
        capi.check(capi.lib().mhx_get_history_capacity(self._h, C.byref(n)))
        return n.value

    def summary_timing(self):
        """HIP-event milliseconds of the kernels of the last batched summary call"""
        ms = C.c_double(0)
        capi.check(capi.lib().mhx_get_summary_timing(self._h, C.byref(ms)))
        return ms.value

    def set_history(self, chain, prob, theta):
        """restore a walk, newest first (walker-load)"""
        pa, pp = capi.as_f64(prob)
        ta, tp = capi.as_f64(np.asarray(theta, dtype=np.float64).reshape(len(pa), self.d))
        capi.check(capi.lib().mhx_set_history(self._h, int(chain), pp, tp, len(pa)))

    MODIFY = {"burn-walks": 0, "keep-walks": 1, "reset": 2, "reset-to-most-likely": 3}

    def modify(self, action, n=0):
        """walker-modify's :burn-walks / :keep-walks / :reset / :reset-to-most-likely (M:566-578)"""
        capi.check(capi.lib().mhx_walker_modify(self._h, self.MODIFY[action], int(n)))

    def pooled(self):
        d = self.d
        stats, L = np.zeros(1 + d + d * d), np.zeros((d, d))
        valid, n = C.c_int32(0), C.c_uint64(0)
        capi.check(capi.lib().mhx_get_pooled(self._h, stats.ctypes.data_as(capi.f64p),
                                             L.ctypes.data_as(capi.f64p), C.byref(valid),
                                             C.byref(n)))
        return dict(stats=stats, L=L, valid=bool(valid.value), refreshes=n.value)

    def counters(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib().mhx_get_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_name(self):
        """which kernels serve the problem: 'w16/gauss22_normal', 'w8/rtc[expr:normal]', ..."""
        r = capi.lib().mhx_kernel_name(self._h)
        if r is None:
            raise capi.MhxError(capi.ESTATE, capi.lib().mhx_last_error().decode("utf-8", "replace"))
        return r.decode()

    def kernel_timing(self, reset=False):
        avg, tot, n = C.c_double(0), C.c_double(0), C.c_uint64(0)
        capi.check(capi.lib().mhx_kernel_timing(self._h, int(reset), C.byref(avg), C.byref(n),
                                                C.byref(tot)))
        return dict(avg_ms=avg.value, launches=n.value, total_ms=tot.value)


def comm_unique_id():
    """128 bytes identifying a new RCCL communicator (rank 0 calls this and passes them on)"""
    buf = (C.c_uint8 * 128)()
    capi.check(capi.lib().mhx_comm_get_unique_id(buf))
    return bytes(buf)


def partition(n_chains, n_parts, part):
    """(first, count) of part's contiguous chain range (mhx_group_partition; no device needed)"""
    a, b = C.c_int64(0), C.c_int64(0)
    capi.check(capi.lib().mhx_group_partition(int(n_chains), int(n_parts), int(part),
                                              C.byref(a), C.byref(b)))
    return a.value, b.value


class _GroupEngine(Engine):
    """engine i of a group, seen through the per-engine entry points (owned by the group)"""

    def __init__(self, handle, n_chains, d, K):  # noqa: super().__init__ creates; this borrows
        self._h = C.c_void_p(handle)
        self._cb = None
        self.n_chains, self.d, self.K = int(n_chains), int(d), int(K)

    def close(self):
        self._h = C.c_void_p()


class Group(_Summaries):
    """ONE host process, several GPUs (include/mhx.h, mhx_group_*): n_chains walkers in all,
    contiguous global id ranges per device, launches enqueued on every device before any is
    waited for, the pooled tick's all-reduce through RCCL."""
    _summary_prefix = "mhx_group_get_"

    def __init__(self, n_chains, n_params, n_functions=1, devices=(0,), seed=0, chain_offset=0,
                 adapt_mode=capi.ADAPT_FAITHFUL, history_capacity=0, poisson_logfact_double=False):
        cfg = capi.Config()
        cfg.n_chains, cfg.n_params, cfg.n_functions = int(n_chains), int(n_params), int(n_functions)
        cfg.adapt_mode, cfg.seed = int(adapt_mode), int(seed)
        cfg.chain_offset, cfg.history_capacity = int(chain_offset), int(history_capacity)
        cfg.poisson_logfact_double = int(bool(poisson_logfact_double))
        self.n_chains, self.d, self.K = int(n_chains), int(n_params), int(n_functions)
        dev, devp = capi.as_i32(list(devices))
        self._h = C.c_void_p()
        capi.check(capi.lib().mhx_group_create(C.byref(cfg), devp, len(dev), C.byref(self._h)))
        self.ranges = []
        self.engines = []
        for i in range(capi.lib().mhx_group_size(self._h)):
            a, b = C.c_int64(0), C.c_int64(0)
            capi.check(capi.lib().mhx_group_chain_range(self._h, i, C.byref(a), C.byref(b)))
            self.ranges.append((a.value, b.value))
            self.engines.append(_GroupEngine(capi.lib().mhx_group_engine(self._h, i), b.value,
                                             self.d, self.K))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            for e in self.engines:
                e.close()
            capi.lib().mhx_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # problem definition: the same calls as Engine, applied to every device
    def set_function(self, k, model, shape=(), param_index=()):
        sh, shp = capi.as_i32(list(shape) if len(shape) else [0])
        ix, ixp = capi.as_i32(list(param_index))
        capi.check(capi.lib().mhx_group_set_function(self._h, k, model, shp, len(shape), ixp, len(ix)))

    def set_dataset(self, k, x, y, sigma=None, likelihood=capi.LIK_NORMAL):
        xa, xp = capi.as_f64(x)
        ya, yp = capi.as_f64(y)
        for owner in [self] + self.engines:      # (what waic / eval_function / fit_bands size x=None by)
            owner.__dict__.setdefault("_datasets", {})[int(k)] = (int(ya.size), 1)
        sp = None
        if sigma is not None:
            sa, sp = capi.as_f64(np.broadcast_to(np.asarray(sigma, dtype=np.float64), xa.shape))
        capi.check(capi.lib().mhx_group_set_dataset(self._h, k, xp, yp, sp, xa.size, likelihood))

    def set_dataset_planes(self, k, x, y, sigma=None, sigma_kind=capi.SIGMA_NONE,
                           likelihood=capi.LIK_NORMAL):
        """mhx_group_set_dataset_planes: y (and a per-walker sigma) cover all chains of the group"""
        keep, (xp, yp, sp) = _planes_args(self.n_chains, x, y, sigma, sigma_kind)
        for owner in [self] + self.engines:
            owner.__dict__.setdefault("_datasets", {})[int(k)] = (int(keep[0].size), 1)
        capi.check(capi.lib().mhx_group_set_dataset_planes(self._h, k, xp, yp, sp, sigma_kind,
                                                           keep[0].size, likelihood))

    def set_bounds(self, k, idx, lo, hi):
        ix, ixp = capi.as_i32(list(idx))
        la, lp = capi.as_f64(lo)
        ha, hp = capi.as_f64(hi)
        capi.check(capi.lib().mhx_group_set_bounds(self._h, k, ixp, lp, hp, len(ix)))

    def init_chains(self, theta0):
        th = np.ascontiguousarray(theta0, dtype=np.float64)
        bc = 1 if th.ndim == 1 else 0
        capi.check(capi.lib().mhx_group_init_chains(self._h, th.ctypes.data_as(capi.f64p), bc))

    def adaptive_begin(self, n=100000, temperature=1e3, auto=1, max_walker_length=0, l_matrix=None):
        o = Engine._opts(self, n, temperature, auto, max_walker_length, l_matrix)
        capi.check(capi.lib().mhx_group_adaptive_begin(self._h, C.byref(o)))

    def adaptive_advance(self, max_iters, count=True):
        n = C.c_int64(-1)
        capi.check(capi.lib().mhx_group_adaptive_advance(self._h, int(max_iters),
                                                         C.byref(n) if count else None))
        return n.value

    def adaptive_steps_full(self, n=100000, temperature=1e3, auto=1, max_walker_length=0,
                            l_matrix=None):
        o = Engine._opts(self, n, temperature, auto, max_walker_length, l_matrix)
        capi.check(capi.lib().mhx_group_adaptive_steps_full(self._h, C.byref(o)))

    def request_stop(self):
        capi.check(capi.lib().mhx_group_request_stop(self._h))

    def state(self):
        C_, d = self.n_chains, self.d
        th, bt = np.zeros((C_, d)), np.zeros((C_, d))
        lp, bl = np.zeros(C_), np.zeros(C_)
        ln, ag = np.zeros(C_, dtype=np.int64), np.zeros(C_, dtype=np.int64)
        capi.check(capi.lib().mhx_group_get_state(
            self._h, th.ctypes.data_as(capi.f64p), lp.ctypes.data_as(capi.f64p),
            bt.ctypes.data_as(capi.f64p), bl.ctypes.data_as(capi.f64p),
            ln.ctypes.data_as(capi.i64p), ag.ctypes.data_as(capi.i64p)))
        return dict(theta=th, logpost=lp, best_theta=bt, best_logpost=bl, length=ln, age=ag)

    def history_capacity(self):
        return self.engines[0].history_capacity()

    def counters(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib().mhx_group_get_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
