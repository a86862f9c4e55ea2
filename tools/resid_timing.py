#!/usr/bin/env python3
"""Times the residual read-out of a finished fit, batched on the device and per chain on the host.

Two shapes, each after a short real walk (the medians are taken over its newest --take steps):

  shared   --chains walkers on BASELINE config 2's two-peak model and its 1e5 points, one shared
           dataset; the batched call returns the totals only
  planes   --chains spectra of 334 points, a dataset per walker (tools/planes_timing.py's ODMR
           sweeps, one stddev per spectrum); the batched call returns fit and z as well

For each:

  (a) one Engine.residuals call at the medians (mhx_get_residuals): wall time and the HIP-event
      time of its kernels (mhx_get_summary_timing), the median and the least and greatest of
      --repeats warm runs after one warm-up; and the same with the Engine.percentiles call that
      makes the medians in front of it (the whole batched route);
  (b) the per-chain host route, what walker_get_residuals does for one walker: one mhx_get_trace
      of the window and its median, one mhx_eval_function, the subtraction, division and sums in
      numpy - timed on the first --sample chains and scaled to all of them ("extrapolated"); its
      chi-square must agree with the device's to 1e-9 relative.

Prints one JSON line.

    python tools/resid_timing.py --chains 4096
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


def host_route(e, c, take, y, sigma):
    """chi-square of chain c the way walker_get_residuals reaches its numbers"""
    _, th = e.trace(c, take)
    fit = e.eval_function(0, np.median(th, axis=0))
    z = (fit - y) / sigma
    return float(np.sum(z * z)), z


def measure(e, take, y_of, sigma_of, pointwise, repeats, sample):
    n, pts = e.n_chains, e._datasets[0][0]
    med, _ = e.percentiles(take, [(50, 1)])
    med = np.ascontiguousarray(med[:, 0, :])
    r, t = timed(lambda: e.residuals(0, med, pointwise=pointwise), e, repeats)
    t.update({"points": n * pts, "points_per_s": n * pts / (t["kernel_ms"] * 1e-3),
              "chains_flagged": int((r["status"] != 0).sum()), "pointwise": pointwise})
    out = {"residuals": t}

    def route():
        m, _ = e.percentiles(take, [(50, 1)])
        return e.residuals(0, np.ascontiguousarray(m[:, 0, :]), pointwise=pointwise)
    walls = []
    route()  # warm-up
    for _ in range(repeats):
        t0 = time.perf_counter()
        route()
        walls.append(time.perf_counter() - t0)
    out["medians_and_residuals"] = {"wall_s": statistics.median(walls), "wall_s_min_max": [min(walls), max(walls)]}
    n_s = min(sample, n)
    host_route(e, 0, take, y_of(0), sigma_of(0))  # warm-up
    t_0 = time.perf_counter()
    for c in range(n_s):
        got, _ = host_route(e, c, take, y_of(c), sigma_of(c))
        assert abs(got - r["chi2"][c]) <= 1e-9 * abs(got), (c, got, r["chi2"][c])
    t_s = time.perf_counter() - t_0
    out["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s, "all_chains_s": t_s * n / n_s,
                                   "extrapolated": n_s < n}
    out["speedup"] = out["per_chain_host_route"]["all_chains_s"] / out["medians_and_residuals"]["wall_s"]
    out["median_reduced_chi2"] = float(np.median(r["chi2"]) / (pts - e.d))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--take", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--plane-points", type=int, default=334)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--only", choices=["shared", "planes"], default=None)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from planes_timing import spectra

    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "chains": a.chains, "repeats": a.repeats,
           "iters": a.iters}
    if a.only != "planes":
        s = pb.two_peak(n=a.points, seed=12)
        x, y, sig, _ = s.data[0]
        e = s.engine(mhx, a.chains, seed=41)
        e.init_chains(pb.perturbed(s.theta_star, a.chains, 0.01, seed=5))
        e.adaptive_steps(a.iters)
        take = min(a.take, e.history_capacity())
        out = measure(e, take, lambda c: y, lambda c: sig, False, a.repeats, a.sample)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.points, "d": e.d})
        res["shared"] = out
        e.close()
    if a.only != "shared":
        x, y, sigma, start = spectra(a.chains, a.plane_points)
        e = mhx.Engine(a.chains, 7, 1, seed=5)
        e.set_function(0, mhx.capi.MODEL_LORENTZ_PEAKS, (1, 2), list(range(7)))
        e.set_dataset_planes(0, x, y, sigma, mhx.capi.SIGMA_PER_CHAIN)
        e.set_bounds(0, [], [], [])
        e.init_chains(start)
        e.adaptive_steps(a.iters)
        take = min(a.take, e.history_capacity())
        out = measure(e, take, lambda c: y[c], lambda c: sigma[c], True, a.repeats, a.sample)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.plane_points, "d": e.d})
        res["planes"] = out
        e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
