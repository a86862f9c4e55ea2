"""The yardstick of mhx_get_normal_equations: include/mhx.h's definition restated in numpy.  numpy's
float64 multiply, add, subtract, divide and square root round once each and never fuse, which is
what the definition asks for; np.cumsum adds in sequence, which is the definition's serial sum.

Input: a callable values(theta) -> v [N], the model of ONE walker at the dataset's own x - on the
GPU what e.eval_function(fn, theta) returns, on the CPU numpy - the walker's vector theta [d], the
steps h [d], the places of theta the function reads, and the walker's data: y and sigma (None: 1.0)
for the normal forms, the counts y for Poisson."""
import numpy as np

NORMAL, CUTOFF, POISSON, EXPR = 0, 1, 2, 3
NONFINITE = 1
BLOCK = 1024


def serial_sum(t):
    """from 0.0, the terms added one after the other along the last axis"""
    t = np.asarray(t, dtype=np.float64)
    lead = np.zeros(t.shape[:-1] + (1,))
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([lead, t], axis=-1), axis=-1)[..., -1]


def block_sums(rows):
    """rows [q, N] -> S [q, q]: S[a, b] = the sum over the points of rows[a] * rows[b], by the
    definition's rule: within each block of BLOCK points serially in ascending i from 0.0, then the
    blocks' sums serially in ascending block order from 0.0"""
    rows = np.asarray(rows, dtype=np.float64)
    q, N = rows.shape
    parts = []
    with np.errstate(all="ignore"):
        for b0 in range(0, N, BLOCK):
            r = rows[:, b0:b0 + BLOCK]
            parts.append(serial_sum(r[:, None, :] * r[None, :, :]))
    return serial_sum(np.stack(parts, axis=-1))


def columns(values, theta, steps, reads):
    """v [N], and for every place t the function reads with a step h != 0 the central difference
    J[t] [N] with its vp, vm: {t: (J, vp, vm)}"""
    theta = np.asarray(theta, dtype=np.float64)
    v = np.asarray(values(theta), dtype=np.float64)
    cols = {}
    with np.errstate(all="ignore"):
        for t in sorted(set(int(t) for t in reads)):
            h = np.float64(steps[t])
            if h == 0.0:
                continue
            tp = theta[t] + h
            tm = theta[t] - h
            dh = tp - tm
            up, dn = theta.copy(), theta.copy()
            up[t], dn[t] = tp, tm
            vp = np.asarray(values(up), dtype=np.float64)
            vm = np.asarray(values(dn), dtype=np.float64)
            df = vp - vm
            cols[t] = (df / dh, vp, vm)
    return v, cols


def yardstick(values, lik, theta, steps, reads, y, sigma=None):
    """everything mhx_get_normal_equations returns for one walker: a dict of jtj [d, d], jtr [d],
    chi2, g [d, N], status - and u [N]"""
    theta = np.asarray(theta, dtype=np.float64)
    d = theta.size
    y = np.asarray(y, dtype=np.float64)
    v, cols = columns(values, theta, steps, reads)
    N = v.size
    g = np.zeros((d, N))
    ok = bool(np.isfinite(v).all())
    with np.errstate(all="ignore"):
        if lik == POISSON:
            rt = np.sqrt(v)
            dl = y - v
            u = dl / rt
            for t, (J, vp, vm) in cols.items():
                g[t] = J / rt
        else:
            s = np.ones_like(y) if sigma is None else np.broadcast_to(np.asarray(sigma, float), y.shape)
            w = 1.0 / s
            ys = y * w
            a = v * w
            u = ys - a
            for t, (J, vp, vm) in cols.items():
                g[t] = J * w
    for t, (J, vp, vm) in cols.items():
        ok = ok and bool(np.isfinite(vp).all() and np.isfinite(vm).all() and np.isfinite(g[t]).all())
    ok = ok and bool(np.isfinite(u).all())
    active = sorted(cols)
    S = block_sums(np.vstack([g[active], u[None, :]])) if N else np.zeros((len(active) + 1,) * 2)
    jtj, jtr = np.zeros((d, d)), np.zeros(d)
    for a, t in enumerate(active):
        jtr[t] = S[a, len(active)]
        for b, s_ in enumerate(active):
            jtj[t, s_] = S[min(a, b), max(a, b)]
    return {"jtj": jtj, "jtr": jtr, "chi2": float(S[-1, -1]), "g": g, "u": u,
            "status": 0 if ok else NONFINITE}


def same_bits(a, b):
    """the same bits, element by element; a NaN stands for any NaN (the definition fixes no payload)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | both_nan))
