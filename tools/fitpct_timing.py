#!/usr/bin/env python3
"""Times the credible bands of a finished fit, batched on the device and per chain on the host.

On BASELINE config 2's two-peak model (d = 8, ring 1024, a 3000-iteration walk), take 1000, 1000
points between the data's least and greatest x, the 2.5 / 50 / 97.5 per cent points:

  (a) one Engine.fit_percentiles call for every chain (mhx_get_fit_percentiles): wall time and the
      HIP-event time of its kernels (mhx_get_summary_timing), the median and the least and greatest
      of --repeats warm runs after one warm-up; the same call with no percentile asked for, whose
      kernels are the values and moments alone - the difference is the selection's share;
  (b) the same call in fresh processes (the knobs are read when the problem is finalised) with
      MHX_FITPCT_NO_LDS=1 (every pass of the selection reads the staged values),
      MHX_FITPCT_SELECT_SINGLY=1 (select_percentile once per percentile: the straightforward form)
      and MHX_FITPCT_STEP_FASTEST=1 (the staged values laid a point's steps side by side);
  (c) mhx_get_fit_bands on the same engine and the same x, the same way;
  (d) the per-chain host route: one mhx_get_trace of the window, one mhx_eval_function of its
      take x m values and np.partition per column, np.mean and np.std - timed on the first
      --sample chains and scaled to all of them ("extrapolated"); its median curve must equal the
      device's.

Prints one JSON line.

    python tools/fitpct_timing.py --chains 4096
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAKE = 1000
PCTS = [(5, 2), (50, 1), (195, 2)]
KNOBS = ("MHX_FITPCT_NO_LDS", "MHX_FITPCT_SELECT_SINGLY", "MHX_FITPCT_STEP_FASTEST")


def host_route(mhx, e, c, xs):
    """(lo, median, hi, mean, stddev) of chain c from its trace, by numpy"""
    _, th = e.trace(c, TAKE)
    v = e.eval_function(0, th, xs)
    n = len(v)
    cut = []
    for num, den in PCTS:
        a, b = num * (n - 1), 100 * den
        cut += [a // b] + ([a // b + 1] if a % b else [])
    part = np.partition(v, sorted(set(cut)), axis=0)
    out = []
    for num, den in PCTS:
        a, b = num * (n - 1), 100 * den
        out.append((part[a // b] + part[a // b + 1]) / 2.0 if a % b else part[a // b])
    return out + [v.mean(axis=0), v.std(axis=0, ddof=1)]


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
    ap.add_argument("--device-call-only", action="store_true",
                    help="time (a) alone and print its entry: what the children of (b) run")
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    x = pb.two_peak(n=a.points, seed=12).data[0][0]          # (make_walker's dataset)
    xs = mhx.fit_linspace(x.min(), x.max(), a.points)
    got, t = timed(lambda: e.fit_percentiles(0, TAKE, xs, PCTS), e, a.repeats)
    values = float(got[3].astype(np.int64).sum()) * a.points
    _, t0 = timed(lambda: e.fit_percentiles(0, TAKE, xs, ()), e, a.repeats)
    t.update({"model_values": values, "values_kernel_ms": t0["kernel_ms"],
              "selection_kernel_ms": t["kernel_ms"] - t0["kernel_ms"], "moments_only_wall_s": t0["wall_s"],
              "values_per_s_of_the_values_kernels": values / (t0["kernel_ms"] * 1e-3),
              "chains_flagged": int((got[4] != 0).sum())})
    if a.device_call_only:
        e.close()
        print(json.dumps(t))
        return
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "points": a.points,
           "percentiles": [n / d for n, d in PCTS], "repeats": a.repeats, "fit_percentiles": t}
    (_, _, nsel, _), tb = timed(lambda: e.fit_bands(0, TAKE, xs), e, a.repeats)
    vb = float(nsel.astype(np.int64).sum()) * a.points
    tb.update({"model_values": vb, "values_per_s": vb / (tb["kernel_ms"] * 1e-3)})
    res["fit_bands"] = tb
    n_s = min(a.sample, a.chains)
    host_route(mhx, e, 0, xs)  # warm-up
    t_0 = time.perf_counter()
    for c in range(n_s):
        ref = host_route(mhx, e, c, xs)
        assert np.array_equal(ref[1], got[0][c, 1]), c
    t_s = time.perf_counter() - t_0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / t["wall_s"]
    e.close()
    for knob in KNOBS:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-call-only", "--chains",
                                str(a.chains), "--iters", str(a.iters), "--points", str(a.points), "--repeats",
                                str(a.repeats)], capture_output=True, text=True, env=dict(os.environ, **{knob: "1"}))
        if child.returncode != 0:
            sys.exit("the %s=1 run failed:\n" % knob + child.stderr[-3000:])
        res[knob.lower()[4:]] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
