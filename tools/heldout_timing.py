#!/usr/bin/env python3
"""Times the held-out predictive density of a finished fit, batched on the device and per chain on
the host.

On BASELINE config 2's two-peak model (d = 8, ring 1024, a 3000-iteration walk), take 1000, 1000
points - the median and the least and greatest of --repeats warm runs after one warm-up, wall time
and the HIP-event time of the kernels (mhx_get_summary_timing):

  (1) one Engine.heldout call for every chain (mhx_get_heldout) given the engine's own (x, y, sigma):
      y shared by the chains, totals only; the same with the pointwise outputs;
  (2) the same call with a y and a `use` mask per chain (about half the points each);
  (3) Engine.waic on the same engine in the same process: the yardstick - with shared y the
      held-out kernel does WAIC's arithmetic on WAIC's window, and its lpd must be WAIC's lppd bit
      for bit;
  (4) the per-chain host route: one mhx_get_trace of the window, one mhx_eval_function of its steps
      and the definition in numpy (exp and log by numpy: what a user without the device call would
      write) - timed on the first --sample chains and scaled to all of them ("extrapolated"); its
      lpd must agree with the device's to 1e-9 relative.

Prints one JSON line.

    python tools/heldout_timing.py --chains 4096
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


def host_route(e, c, x, y, sig):
    """lpd of chain c from its trace: the definition with numpy's exp and log"""
    _, th = e.trace(c, TAKE)
    v = e.eval_function(0, th, x)
    w = 1.0 / sig
    r = y * w - v * w
    ell = (-0.5 * np.log(2.0 * np.pi) - np.log(sig)) - 0.5 * r * r
    top = ell.max(axis=0)
    return float((top + np.log(np.exp(ell - top).sum(axis=0) / len(ell))).sum())


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
    rw, t = timed(lambda: e.waic(0, TAKE), e, a.repeats)
    steps = float(rw["n_used"].astype(np.int64).sum()) * a.points
    t["point_steps_per_s"] = steps / (t["kernel_ms"] * 1e-3)
    res["waic_totals"] = t
    r, t = timed(lambda: e.heldout(0, TAKE, x, y, sigma=sig), e, a.repeats)
    t.update({"point_steps": steps, "point_steps_per_s": steps / (t["kernel_ms"] * 1e-3),
              "chains_flagged": int((r["status"] != 0).sum()),
              "lpd_is_waic_lppd_bit_for_bit": bool(np.array_equal(r["lpd"].view(np.uint64),
                                                                  rw["lppd"].view(np.uint64)))})
    res["heldout_shared_y_totals"] = t
    _, t = timed(lambda: e.heldout(0, TAKE, x, y, sigma=sig, pointwise=True, accumulators=True), e, a.repeats)
    t["point_steps_per_s"] = steps / (t["kernel_ms"] * 1e-3)
    res["heldout_shared_y_pointwise"] = t
    rng = np.random.default_rng(3)
    y2 = y[None, :] + sig[None, :] * rng.standard_normal((a.chains, a.points))
    use = (rng.random((a.chains, a.points)) < 0.5).astype(np.uint8)
    r2, t = timed(lambda: e.heldout(0, TAKE, x, y2, sigma=sig, use=use), e, a.repeats)
    t.update({"point_steps_per_s": steps / (t["kernel_ms"] * 1e-3), "points_scored": int(r2["n_scored"].sum())})
    res["heldout_per_chain_y_and_use"] = t
    _, t = timed(lambda: e.waic(0, TAKE), e, a.repeats)         # (once more, after the others: the same clocks)
    t["point_steps_per_s"] = steps / (t["kernel_ms"] * 1e-3)
    res["waic_totals_again"] = t
    n_s = min(a.sample, a.chains)
    host_route(e, 0, x, y, sig)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        got = host_route(e, c, x, y, sig)
        assert abs(got - r["lpd"][c]) <= 1e-9 * abs(got), (c, got, r["lpd"][c])
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / res["heldout_shared_y_totals"]["wall_s"]
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
