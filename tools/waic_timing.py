#!/usr/bin/env python3
"""Times WAIC of a finished fit, batched on the device and per chain on the host.

On BASELINE config 2's two-peak model (d = 8, ring 1024, a 3000-iteration walk), take 1000, the
dataset's own 1000 points:

  (a) one Engine.waic call for every chain (mhx_get_waic), totals only: wall time and the
      HIP-event time of its kernels (mhx_get_summary_timing), the median and the least and
      greatest of --repeats warm runs after one warm-up; the same with the pointwise outputs;
  (b) mhx_get_fit_bands on the same engine and the same x, the same way: the kernel whose shape
      k_waic shares (its model values per second beside k_waic's point-steps per second);
  (c) the per-chain host route: one mhx_get_trace of the window, one mhx_eval_function of its
      steps and the definition in numpy (exp and log by numpy: what a user without the device
      call would write) - timed on the first --sample chains and scaled to all of them
      ("extrapolated"); its elpd must agree with the device's to 1e-9 relative.

Prints one JSON line.

    python tools/waic_timing.py --chains 4096
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

TAKE = 1000


def host_route(e, c, y, sig):
    """elpd of chain c from its trace: the definition with numpy's exp and log"""
    _, th = e.trace(c, TAKE)
    v = e.eval_function(0, th)
    w = 1.0 / sig
    r = y * w - v * w
    ell = (-0.5 * np.log(2.0 * np.pi) - np.log(sig)) - 0.5 * r * r
    top = ell.max(axis=0)
    lppd = top + np.log(np.exp(ell - top).sum(axis=0) / len(ell))
    return float(lppd.sum() - ell.var(axis=0, ddof=1).sum())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    s = pb.two_peak(n=a.points, seed=12)          # (make_walker's dataset)
    x, y, sig, _ = s.data[0]
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "points": a.points,
           "repeats": a.repeats}
    r, t = timed(lambda: e.waic(0, TAKE), e, a.repeats)
    steps = float(r["n_used"].astype(np.int64).sum()) * a.points
    t.update({"point_steps": steps, "point_steps_per_s": steps / (t["kernel_ms"] * 1e-3),
              "chains_flagged": int((r["status"] != 0).sum())})
    res["waic_totals"] = t
    _, t = timed(lambda: e.waic(0, TAKE, pointwise=True), e, a.repeats)
    t["point_steps_per_s"] = steps / (t["kernel_ms"] * 1e-3)
    res["waic_pointwise"] = t
    (_, _, nsel, _), t = timed(lambda: e.fit_bands(0, TAKE, x), e, a.repeats)
    values = float(nsel.astype(np.int64).sum()) * a.points
    t.update({"model_values": values, "values_per_s": values / (t["kernel_ms"] * 1e-3)})
    res["fit_bands"] = t
    n_s = min(a.sample, a.chains)
    host_route(e, 0, y, sig)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        got = host_route(e, c, y, sig)
        assert abs(got - r["elpd"][c]) <= 1e-9 * abs(got), (c, got, r["elpd"][c])
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / res["waic_totals"]["wall_s"]
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
