#!/usr/bin/env python3
"""Times walker-get-data-and-fit's envelopes of a finished fit, batched and per chain.

On BASELINE config 2's shape (d = 8, ring 1024, a 3000-iteration walk), take 1000, m = 1000 points:

  (a) one Engine.fit_bands call for every chain (mhx_get_fit_bands): wall time and the HIP-event
      time of its kernels (mhx_get_summary_timing), median of --repeats runs after one warm-up;
  (b) the per-chain host route: one mhx_get_trace of the ring, the selection of the
      ceiling(0.66 take) most probable steps on the host, one mhx_eval_function of them and numpy
      max / min - timed on the first --sample chains and scaled to all of them ("extrapolated").

Also one eval_function call of one parameter vector per chain (the fit curves of the whole set).
Prints one JSON line.

    python tools/band_timing.py --chains 4096
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAKE, M = 1000, 1000


def host_route(mhx, e, c, ring, xs):
    prob, th = e.trace(c, ring)
    k = min(mhx.band_count(min(TAKE, len(prob))), len(prob))
    order = np.argsort(-np.where(np.isnan(prob), -np.inf, prob), kind="stable")[:k]
    vals = e.eval_function(0, th[order], xs)
    return vals.max(axis=0), vals.min(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    ring = e.history_capacity()
    xs = mhx.fit_linspace(0.0, 1.0, M)
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": ring, "take": TAKE, "m": M, "repeats": a.repeats}
    e.fit_bands(0, TAKE, xs)  # warm-up
    wall, kms = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ymax, ymin, nsel, status = e.fit_bands(0, TAKE, xs)
        wall.append(time.perf_counter() - t0)
        kms.append(e.summary_timing())
    evals = float(nsel.astype(np.int64).sum()) * M
    res["batched"] = {"wall_s": statistics.median(wall), "kernel_ms": statistics.median(kms),
                      "model_values": evals,
                      "values_per_s": evals / (statistics.median(kms) * 1e-3),
                      "chains_flagged": int(status.sum())}
    n_s = min(a.sample, a.chains)
    host_route(mhx, e, 0, ring, xs)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        hmax, hmin = host_route(mhx, e, c, ring, xs)
        assert np.array_equal(hmax, ymax[c]) and np.array_equal(hmin, ymin[c]), c
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s,
                                   "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / res["batched"]["wall_s"]
    th = e.state()["best_theta"]
    e.eval_function(0, th, xs)
    fw, fk = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        e.eval_function(0, th, xs)
        fw.append(time.perf_counter() - t0)
        fk.append(e.summary_timing())
    res["fit_curves"] = {"wall_s": statistics.median(fw), "kernel_ms": statistics.median(fk)}
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
