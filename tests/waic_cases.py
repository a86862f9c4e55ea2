"""The yardstick of mhx_get_waic: include/mhx.h's definition restated in numpy, elementwise over
the points and stepping serially over the window's steps.  numpy's float64 multiply, add, subtract
and divide round once each and never fuse, which is what the definition asks for.  The engine's
exp comes from oraclelib.mirror_gexp and the Poisson sweep's table logarithm from
oraclelib.mirror_tlog (the device's own values for positive normal arguments outside
[0.9375, 1.0625): the tests keep every rate above 1.0625).  The per-point constants come from
math.log - the libm std::log that libmhx calls when the dataset is set - never from np.log.

Input everywhere: the model VALUES v [n, N] at the window's steps, newest first: what
e.eval_function(fn, theta_steps) returns for the theta of e.trace(c, ring)."""
import ctypes
import ctypes.util
import math

import numpy as np

NORMAL, CUTOFF, POISSON, EXPR = 0, 1, 2, 3
NONFINITE, ONE_STEP = 1, 2
BLOCK = 256
HALF_LOG_2PI = -0.5 * math.log(2.0 * math.pi)       # (* -1/2 (log (* 2 pi)))


def normal_constants(sigma):
    """c_i = -1/2 log 2 pi + (-1 * log sigma_i), as set_dataset_impl forms it"""
    return np.array([HALF_LOG_2PI + (-1.0 * math.log(float(s))) for s in sigma])


def poisson_constants(y, in_double=False):
    """c_i = -log-factorial(y_i): a running sum of SINGLE-float logs (mcmc-fitting.lisp:379-380),
    or lgamma(y + 1) with poisson_logfact_double"""
    if in_double:       # (libm's lgamma, which libmhx calls: math.lgamma is CPython's own)
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.lgamma.restype, libm.lgamma.argtypes = ctypes.c_double, [ctypes.c_double]
        return np.array([-libm.lgamma(float(k) + 1.0) for k in y])
    top = int(max(y)) if len(y) else 0
    cache = np.zeros(top + 1, dtype=np.float32)
    for m in range(1, top + 1):
        cache[m] = np.float32(cache[m - 1] + np.float32(math.log(float(m))))
    return np.array([-float(cache[int(k)]) for k in y])


def terms(lik, v, y, sigma=None, lik_term=None, logfact_double=False):
    """l [n, N] from the values v [n, N] and the dataset (y, sigma) of the function.  lik_term:
    the expression likelihood as a callable (y, model, error) of numpy arrays, every operation
    its own rounding"""
    import oraclelib
    v = np.asarray(v, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        if lik == POISSON:
            c = poisson_constants(y, logfact_double)
            a = y[None, :] * oraclelib.mirror_tlog(v)
            return (a - v) + c[None, :]
        s = np.ones_like(y) if sigma is None else np.broadcast_to(np.asarray(sigma, float), y.shape)
        if lik == EXPR:
            return np.asarray(lik_term(y[None, :], v, s[None, :]), dtype=np.float64)
        w = 1.0 / s
        ys = y * w
        c = normal_constants(s)
        a = v * w[None, :]
        r = ys[None, :] - a
        h = 0.5 * r
        q = h * r
        ell = c[None, :] - q
        if lik == CUTOFF:
            ell = np.where(ell > -5000.0, ell, -5000.0)
        return ell


def accumulate(ell):
    """(M, S, mean, M2) [N] each of the terms ell [n, N], newest first: Welford and the running
    log-sum-exp of the definition, step after step"""
    import oraclelib
    ell = np.asarray(ell, dtype=np.float64)
    n, N = ell.shape
    mean, m2 = np.zeros(N), np.zeros(N)
    M, S = np.zeros(N), np.zeros(N)
    with np.errstate(all="ignore"):
        for s in range(n):
            e = ell[s]
            qk = 1.0 / float(s + 1)
            delta = e - mean
            mean = mean + delta * qk
            m2 = m2 + delta * (e - mean)
            if s == 0:
                M, S = e.copy(), np.ones(N)
                continue
            up = e > M
            g = oraclelib.mirror_gexp(np.where(up, M - e, e - M))
            S = np.where(up, S * g + 1.0, S + g)
            M = np.where(up, e, M)
    return M, S, mean, m2


def pointwise(acc, n):
    """pw_p = M2 / (n - 1) (n = 1: the IEEE 0/0) and the quotient S / n whose log pw_lppd adds to M"""
    M, S, mean, m2 = acc
    with np.errstate(all="ignore"):
        return m2 / np.float64(n - 1), S / np.float64(n)


def yardstick(ell):
    """everything but the device's own log: a dict of acc [N, 4], pw_p, quot = S / n, pw_lppd with
    numpy's log (within an ulp of the device's: for host-side comparisons), the totals by fsum, n_high
    and the status bits"""
    ell = np.asarray(ell, dtype=np.float64)
    n = ell.shape[0]
    acc = accumulate(ell)
    pw_p, quot = pointwise(acc, n)
    with np.errstate(all="ignore"):
        pw_lppd = acc[0] + np.log(quot)
    status = (0 if np.isfinite(ell).all() else NONFINITE) | (ONE_STEP if n == 1 else 0)
    return {"acc": np.column_stack(acc), "pw_p": pw_p, "quot": quot, "pw_lppd": pw_lppd,
            "lppd": math.fsum(pw_lppd) if np.isfinite(pw_lppd).all() else float("nan"),
            "p_waic": math.fsum(pw_p) if np.isfinite(pw_p).all() else float("nan"),
            "n_high": int((np.nan_to_num(pw_p, nan=0.0) > 0.4).sum()), "status": status}


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
