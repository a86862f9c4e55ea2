#!/usr/bin/env python3
"""Times the normal equations of every walker, batched on the device and per chain on the host.

Two shapes, at the walkers' starting points (no walk: this is what runs BEFORE one):

  shared   --chains walkers on BASELINE config 2's two-peak model (d = 8) and its 1e5 points, one
           shared dataset
  planes   --chains spectra of 334 points, a dataset per walker (tools/planes_timing.py's ODMR
           sweeps, one stddev per spectrum, d = 7)

For each:

  (a) one Engine.normal_equations call (mhx_get_normal_equations): wall time and the HIP-event
      time of its kernels (mhx_get_summary_timing), the median and the least and greatest of
      --repeats warm runs after one warm-up;
  (b) the per-chain host route: 2 p + 1 mhx_eval_function calls for one walker and the scaling and
      contraction in numpy - timed on the first --sample chains and scaled to all of them
      ("extrapolated"); its F must agree with the device's to 1e-9 of the greatest entry.

and, on the second shape, one walker_set_least_squares (25 iterations) of the whole set.

Prints one JSON line.

    python tools/normeq_timing.py --chains 4096
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, e, repeats):
    fn()  # warm-up
    wall, kms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
        kms.append(e.summary_timing())
    return out, {"wall_s": statistics.median(wall), "wall_s_min_max": [min(wall), max(wall)],
                 "kernel_ms": statistics.median(kms), "kernel_ms_min_max": [min(kms), max(kms)]}


def host_route(e, th, hs, y, sigma):
    """F of one walker from 2 p + 1 mhx_eval_function calls and a numpy contraction"""
    d = th.size
    vecs = [th]
    for t in range(d):
        up, dn = th.copy(), th.copy()
        up[t], dn[t] = th[t] + hs[t], th[t] - hs[t]
        vecs += [up, dn]
    v = [e.eval_function(0, q) for q in vecs]
    w = 1.0 / sigma
    g = np.array([(v[1 + 2 * t] - v[2 + 2 * t]) / ((th[t] + hs[t]) - (th[t] - hs[t])) * w for t in range(d)])
    u = y * w - v[0] * w
    return g @ g.T, g @ u, float(u @ u)


def measure(mhx, e, theta, y_of, sigma_of, repeats, sample):
    n, pts = e.n_chains, e._datasets[0][0]
    hs = mhx.normeq_steps(theta)
    r, t = timed(lambda: e.normal_equations(0, theta, hs), e, repeats)
    evals = n * pts * (2 * e.d + 1)
    t.update({"model_values": evals, "model_values_per_s": evals / (t["kernel_ms"] * 1e-3),
              "chains_flagged": int((r["status"] != 0).sum())})
    out = {"normal_equations": t}
    n_s = min(sample, n)
    host_route(e, theta[0], hs[0], y_of(0), sigma_of(0))  # warm-up
    t_0 = time.perf_counter()
    for c in range(n_s):
        F, _, _ = host_route(e, theta[c], hs[c], y_of(c), sigma_of(c))
        assert np.abs(F - r["jtj"][c]).max() <= 1e-9 * np.abs(F).max(), (c, np.abs(F - r["jtj"][c]).max())
    t_s = time.perf_counter() - t_0
    out["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s, "all_chains_s": t_s * n / n_s,
                                   "extrapolated": n_s < n}
    out["speedup"] = out["per_chain_host_route"]["all_chains_s"] / t["wall_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--plane-points", type=int, default=334)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--only", choices=["shared", "planes"], default=None)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from planes_timing import spectra, KEYS

    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "chains": a.chains, "repeats": a.repeats}
    if a.only != "planes":
        s = pb.two_peak(n=a.points, seed=12)
        x, y, sig, _ = s.data[0]
        e = s.engine(mhx, a.chains, seed=41)
        theta = pb.perturbed(s.theta_star, a.chains, 0.01, seed=5)
        e.init_chains(theta)
        out = measure(mhx, e, theta, lambda c: y, lambda c: sig, a.repeats, a.sample)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.points, "d": e.d})
        res["shared"] = out
        e.close()
    if a.only != "shared":
        x, y, sigma, start = spectra(a.chains, a.plane_points)
        w = mhx.walker_set_create(function=mhx.models.lorentz_peaks(KEYS[:1], [KEYS[1:4], KEYS[4:7]]),
                                  datasets=[[x, y[c]] for c in range(a.chains)],
                                  params=[dict(zip(KEYS, start[c])) for c in range(a.chains)],
                                  data_error=[float(v) for v in sigma], seed=5)
        e = w.engine
        out = measure(mhx, e, start, lambda c: y[c], lambda c: np.full(a.plane_points, sigma[c]), a.repeats,
                      a.sample)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.plane_points, "d": e.d})
        t0 = time.perf_counter()
        r = mhx.walker_set_least_squares(w, iterations=a.iterations)
        dt = time.perf_counter() - t0
        dec = np.array([s_["newton-decrement"] if s_["status"] == 0 else np.nan for s_ in r["laplace"]])
        out["least_squares"] = {"wall_s": dt, "iterations": a.iterations,
                                "walkers_not_positive_or_finite": int(np.isnan(dec).sum()),
                                "median_newton_decrement": float(np.nanmedian(dec)),
                                "greatest_newton_decrement": float(np.nanmax(dec)),
                                "median_last_moving_iteration": float(np.median(r["iterations"]))}
        res["planes"] = out
        e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
