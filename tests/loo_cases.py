"""The yardstick of mhx_get_loo: include/mhx.h's definition restated in numpy, in the same operation
order.  numpy's float64 multiply, add, subtract, divide and sqrt round once each and never fuse, which
is what the definition asks for.  The terms come from waic_cases.terms, the engine's exp from
oraclelib.mirror_gexp; np.log stands where the definition says tlog (both below one ulp: what the
logarithm feeds is compared within a tolerance, never bit for bit).

Input everywhere: the terms ell [n, N] of a window, newest first (waic_cases.terms of the values
e.eval_function(fn, theta_steps) returns for the theta of e.trace(c, take)).

estimate_mp is the same formulas in mpmath from the same (tail, l_cut, S_b): what the fit, the
smoothing and the estimate are held to."""
import math

import numpy as np

NONFINITE, SHORT, FLAT, EMPTY = 1, 2, 4, 8
BLOCK = 256
MAX_TAIL = 1024
# The yardstick's distance from the same formulas at 200 bits on the same (tail, l_cut, S_b), the largest
# over tests/test_loo_host.py's crafted windows of 25, 64, 300 and 1024 steps, 48 points each: measured
# 6.153e-14 for khat, 7.085e-14 for sigma (relative) and 4.378e-14 for pw_elpd, recorded here rounded up
# to two digits.  Nearly all of it is the cancellation in x_k = r_k - r_cut next to the cut, where
# binary64 ratios a rounding apart give an x_k with few good digits; the device forms the same x_k bit
# for bit.  tests/test_gpu_loo.py takes the device's tolerance from these: 8 times, plus 8 ulp.
DEV_KHAT, DEV_SIGMA, DEV_ELPD = 6.2e-14, 7.1e-14, 4.4e-14
C_FACT = [1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 1.0 / 2.0, 1.0]


def gexp(x):
    import oraclelib
    return oraclelib.mirror_gexp(np.asarray(x, dtype=np.float64))


def tail_length(n, tail_len=0):
    """M of a window of n steps: min(n // 5, R), R the least integer with R R >= 9 n, or
    min(tail_len, n // 5); never above MAX_TAIL; below 5: none"""
    m = n // 5
    if tail_len > 0:
        m = min(m, tail_len)
    else:
        r = math.isqrt(9 * n)
        m = min(m, r if r * r == 9 * n else r + 1)
    m = min(m, MAX_TAIL)
    return m if m >= 5 else 0


def order_key(v):
    """the order of mhx_get_percentiles as unsigned integers: -0 before +0, every NaN last"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | top)
    return np.where(np.isnan(v), np.uint64(0xFFFFFFFFFFFFFFFF), k)


def split(ell, tail_len=0):
    """the order and the body sum: a dict of M, tail [N, M] = T_1 .. T_M ascending, T1, l_cut, S_b [N]"""
    ell = np.asarray(ell, dtype=np.float64)
    n, N = ell.shape
    M = tail_length(n, tail_len)
    idx = np.argsort(order_key(ell), axis=0, kind="stable")       # (ties: ascending s)
    T = np.take_along_axis(ell, idx[:M], axis=0)
    T1 = np.take_along_axis(ell, idx[:1], axis=0)[0]
    l_cut = np.take_along_axis(ell, idx[M:M + 1], axis=0)[0]
    body = np.ones((n, N), dtype=bool)
    np.put_along_axis(body, idx[:M], False, axis=0)
    with np.errstate(all="ignore"):
        g = gexp(T1[None, :] - ell)
        S_b = np.zeros(N)
        for s in range(n):
            S_b = S_b + np.where(body[s], g[s], 0.0)
    return {"M": M, "tail": T.T.copy(), "T1": T1, "l_cut": l_cut, "S_b": S_b}


def expm1_def(y):
    """E(y) of the smoothing: the degree-8 Taylor polynomial in Horner form below 2^-5, else gexp(y) - 1"""
    y = np.asarray(y, dtype=np.float64)
    p = np.full_like(y, C_FACT[0])
    for c in C_FACT[1:]:
        p = c + y * p
    return np.where(np.abs(y) < 2.0 ** -5, y * p, gexp(y) - 1.0)


def fit_np(x):
    """Zhang and Stephens' fit of x_1 <= ... <= x_M (the exceedances), in the definition's order:
    (k_raw, sigma, khat, fitted)"""
    x = np.asarray(x, dtype=np.float64)
    M = x.size
    Md, Mg = np.float64(M), 30 + math.isqrt(M)
    xq, xM = x[(M + 2) // 4 - 1], x[M - 1]
    with np.errstate(all="ignore"):
        if not (xq > 0.0 and xM > 0.0):
            return np.nan, 0.0, np.inf, False
        j = np.arange(1, Mg + 1, dtype=np.float64)
        theta = 1.0 / xM + ((1.0 - np.sqrt(np.float64(Mg) / (j - 0.5))) / 3.0) / xq
        acc = np.zeros(Mg)
        for k in range(M):
            acc = acc + np.log(1.0 - theta * x[k])
        kj = acc / Md
        L = Md * ((np.log((-theta) / kj) - kj) - 1.0)
        den = np.zeros(Mg)
        for i in range(Mg):
            den = den + gexp(L[i] - L)
        w = 1.0 / den
        that = np.float64(0.0)
        for v in theta * w:
            that = that + v
        ks = np.float64(0.0)
        for v in np.log(1.0 - that * x):
            ks = ks + v
        kraw = ks / Md
        sg = (-kraw) / that
        kh = (Md * kraw + 5.0) / np.float64(M + 10)
    if all(np.isfinite(v) for v in (that, kraw, sg, kh)) and sg > 0.0:
        return float(kraw), float(sg), float(kh), True
    return float(kraw), 0.0, np.inf, False


def estimate_np(n, tail, l_cut, S_b):
    """one point, from its tail T_1 .. T_M (ascending), l_cut and S_b: (khat, sigma, elpd, fitted)"""
    T = np.asarray(tail, dtype=np.float64)
    M = T.size
    T1 = T[0] if M else np.float64(l_cut)
    with np.errstate(all="ignore"):
        u = T[::-1]
        rcut = gexp(T1 - np.float64(l_cut))[()]
        khat, sigma, fitted = np.inf, 0.0, False
        if M > 0:
            _, sigma, khat, fitted = fit_np(gexp(T1 - u) - rcut)
        lw = T1 - u
        if fitted:
            p = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / np.float64(M)
            t = np.log(1.0 - p)
            q = (-sigma) * t if khat == 0.0 else (sigma * expm1_def((-khat) * t)) / khat
            lw = np.minimum(np.log(q + rcut), 0.0)
        W = V = np.float64(0.0)
        if M > 0:
            for a, b in zip(gexp(lw + (u - T1)), gexp(lw)):
                W, V = W + a, V + b
        A, D = np.float64(n - M) + W, np.float64(S_b) + V
        elpd = T1 + np.log(A / D)
    return khat, sigma, float(elpd), fitted


def estimate_mp(n, tail, l_cut, S_b):
    """the same formulas in mpmath at the precision the caller set, from the same inputs:
    (khat, sigma, elpd, fitted) as mpf"""
    import mpmath as mp
    T = [mp.mpf(float(v)) for v in tail]
    M = len(T)
    l_cut, S_b = mp.mpf(float(l_cut)), mp.mpf(float(S_b))
    T1 = T[0] if M else l_cut
    u = T[::-1]
    rcut = mp.exp(T1 - l_cut)
    khat, sigma, fitted = mp.inf, mp.mpf(0), False
    if M > 0:
        x = [mp.exp(T1 - v) - rcut for v in u]
        Mg = 30 + math.isqrt(M)
        xq, xM = x[(M + 2) // 4 - 1], x[M - 1]
        if xq > 0 and xM > 0:
            theta = [1 / xM + ((1 - mp.sqrt(mp.mpf(Mg) / (j - mp.mpf(0.5)))) / 3) / xq for j in range(1, Mg + 1)]
            kj = [mp.fsum(mp.log(1 - th * v) for v in x) / M for th in theta]
            L = [M * (mp.log(-th / k) - k - 1) for th, k in zip(theta, kj)]
            w = [1 / mp.fsum(mp.exp(Li - Lj) for Li in L) for Lj in L]
            that = mp.fsum(th * wj for th, wj in zip(theta, w))
            kraw = mp.fsum(mp.log(1 - that * v) for v in x) / M
            sg = -kraw / that
            kh = (M * kraw + 5) / (M + 10)
            if sg > 0:
                khat, sigma, fitted = kh, sg, True
    lw = [T1 - v for v in u]
    if fitted:
        lw = []
        for k in range(1, M + 1):
            t = mp.log(1 - (k - mp.mpf(0.5)) / M)
            q = -sigma * t if khat == 0 else sigma * mp.expm1(-khat * t) / khat
            lw.append(min(mp.log(q + rcut), mp.mpf(0)))
    W = mp.fsum(mp.exp(a + (v - T1)) for a, v in zip(lw, u))
    V = mp.fsum(mp.exp(a) for a in lw)
    elpd = T1 + mp.log(((n - M) + W) / (S_b + V))
    return khat, sigma, elpd, fitted


def yardstick(ell, tail_len=0, k_limit=0.7):
    """everything of the definition for the points of ell [n, N]: a dict of M, tail [N, M], acc [N, 4] =
    (T_1, l_cut, S_b, sigma), pw_khat, pw_elpd [N], fitted [N], n_high and the status bits (the
    lppd side is waic_cases.yardstick's)"""
    ell = np.asarray(ell, dtype=np.float64)
    n, N = ell.shape
    if n == 0:
        return {"M": 0, "tail": np.zeros((N, 0)), "acc": np.full((N, 4), np.nan), "pw_khat": np.full(N, np.inf),
                "pw_elpd": np.full(N, np.nan), "fitted": np.zeros(N, bool), "n_high": N if k_limit < np.inf else 0,
                "status": SHORT | EMPTY}
    s = split(ell, tail_len)
    M = s["M"]
    khat, sigma, elpd, fitted = np.empty(N), np.empty(N), np.empty(N), np.zeros(N, dtype=bool)
    for i in range(N):
        khat[i], sigma[i], elpd[i], fitted[i] = estimate_np(n, s["tail"][i], s["l_cut"][i], s["S_b"][i])
    status = (0 if np.isfinite(ell).all() else NONFINITE) | (SHORT if n < 25 else 0) | \
        (FLAT if M > 0 and not fitted.all() else 0)
    return {"M": M, "tail": s["tail"], "acc": np.column_stack([s["T1"], s["l_cut"], s["S_b"], sigma]),
            "pw_khat": khat, "pw_elpd": elpd, "fitted": fitted, "n_high": int((khat > k_limit).sum()),
            "status": status}


def block_sum(t):
    """the chain's sum of a pointwise quantity by mhx_get_waic's rule: blocks of 256 points, lane
    j = i mod 64 serially from 0.0, then pairwise over the lanes 32, 16, .. 1 apart, the blocks serially"""
    t = np.asarray(t, dtype=np.float64)
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for b0 in range(0, t.size, BLOCK):
            blk = np.zeros(BLOCK)
            blk[:min(BLOCK, t.size - b0)] = t[b0:b0 + BLOCK]
            lanes = np.zeros(64)
            for j in range(BLOCK // 64):
                lanes = lanes + blk[64 * j:64 * (j + 1)]
            m = 32
            while m >= 1:
                lanes = lanes + lanes[np.arange(64) ^ m]
                m >>= 1
            total = total + lanes[0]
    return float(total)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
