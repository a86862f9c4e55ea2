"""The yardstick of mhx_get_residuals: include/mhx.h's definition restated in numpy.  numpy's
float64 multiply, add, subtract, divide and square root round once each and never fuse, which is
what the definition asks for.

Input: the model VALUES v [N] of one walker - what e.eval_function(fn, theta_c) returns at the
dataset's own x - and the walker's data: y and sigma (None: 1.0) for the normal forms, the counts y
for Poisson."""
import numpy as np

NORMAL, CUTOFF, POISSON, EXPR = 0, 1, 2, 3
NONFINITE = 1
BLOCK = 256
LANES = 64


def standardized(lik, v, y, sigma=None):
    """z [N]: a = v w, z = a - ys with w = 1 / sigma, ys = y w as the engine forms them when the
    dataset is set (the normal forms); dl = v - y, rt = sqrt(v), z = dl / rt (Poisson, Pearson)"""
    v = np.asarray(v, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        if lik == POISSON:
            dl = v - y
            rt = np.sqrt(v)
            return dl / rt
        s = np.ones_like(y) if sigma is None else np.broadcast_to(np.asarray(sigma, float), y.shape)
        w = 1.0 / s
        ys = y * w
        a = v * w
        return a - ys


def block_sum(t):
    """the sum of the terms t [N] by the definition's rule: blocks of BLOCK points; lane i mod 64
    of a block adds its points serially in ascending i from 0.0 (a point beyond N adds 0.0); the
    64 lane sums are added by the butterfly u_j = u_j + u_{j xor m}, m = 32, 16, 8, 4, 2, 1; the
    blocks' sums are added serially in ascending block order from 0.0"""
    t = np.asarray(t, dtype=np.float64)
    N = t.size
    nb = (N + BLOCK - 1) // BLOCK
    padded = np.zeros(nb * BLOCK)
    padded[:N] = t
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for b in range(nb):
            rows = padded[b * BLOCK:(b + 1) * BLOCK].reshape(BLOCK // LANES, LANES)
            u = np.zeros(LANES)
            for row in rows:
                u = u + row
            m = LANES // 2
            while m >= 1:
                u = u + u[np.arange(LANES) ^ m]
                m //= 2
            total = total + u[0]
    return float(total)


def reduce(z, z_limit=3.0):
    """the statistics of the residuals z [N]: the three sums, the counts, the extreme"""
    z = np.asarray(z, dtype=np.float64)
    N = z.size
    with np.errstate(all="ignore"):
        t_chi = z * z
        t_dw = np.zeros(N)
        if N > 1:
            dd = z[1:] - z[:-1]
            t_dw[1:] = dd * dd
        s = z > 0.0
        az = np.abs(z)
        n_out = int((az > z_limit).sum())
    # from (-1.0, -1), where |z_i| > m take (|z_i|, i): the first of the greatest |z|, NaNs passed
    # over (|z| >= 0 > -1, so any number beats the start; argmax gives the first of equals)
    m, idx = -1.0, -1
    seen = np.where(np.isnan(az), -2.0, az)
    if N and seen.max() > m:
        idx = int(np.argmax(seen))
        m = float(az[idx])
    return {"chi2": block_sum(t_chi), "sum_z": block_sum(z), "dw": block_sum(t_dw),
            "n_pos": int(s.sum()), "n_runs": 1 + int((s[1:] != s[:-1]).sum()), "n_out": n_out,
            "max_abs_z": m, "max_index": idx}


def yardstick(lik, v, y, sigma=None, z_limit=3.0):
    """everything mhx_get_residuals returns for one walker but fit (which is v itself): a dict of z,
    chi2, sum_z, dw, n_pos, n_runs, n_out, max_abs_z, max_index and status"""
    v = np.asarray(v, dtype=np.float64)
    z = standardized(lik, v, y, sigma)
    out = reduce(z, z_limit)
    out["z"] = z
    out["status"] = 0 if (np.isfinite(v).all() and np.isfinite(z).all()) else NONFINITE
    return out


def same_bits(a, b):
    """the same bits, element by element; a NaN stands for any NaN (the definition fixes no payload)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | both_nan))
