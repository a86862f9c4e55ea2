#!/usr/bin/env python3
"""Times the posterior summaries of a finished fit, per chain and batched, on one engine.

On BASELINE config 2's shape (d = 8, default ring of 1024, a 3000-iteration walk at a small N):

  (a) the per-chain route: walker_get(w, get=..., chain=c) for every chain - the only way to
      these numbers before walker_set_get existed;
  (b) one walker_set_get of the same selector,

for :median-params, :covariance-matrix and :stddev-params; median of `--repeats` runs after one
warm-up, wall time, and beside (b) the HIP-event time of its kernels (mhx_get_summary_timing).
For --chains above --per-chain-limit, (a) is timed on the first --per-chain-limit chains and
scaled, and marked "extrapolated".  Also: the percentile kernel alone (one percentile, then the
eight of the tests) with its columns in LDS and read from memory (MHX_SUMMARY_NO_LDS=1, a child
process), with the window bytes it read per second.  Prints one JSON line.

    python tools/summary_timing.py --chains 4096
    python tools/summary_timing.py --chains 65536 --per-chain-limit 4096
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
PCTS8 = [50, 2.5, 97.5, 25, 75, 84.1, 0, 100]
TAKE = 1000


def make_walker(mhx, pb, chains, iters, n_points):
    s = pb.two_peak(n=n_points, seed=12)
    x, y, sig, _ = s.data[0]
    idx, lo, hi = s.bounds[0]
    params = []
    for k, v in zip(KEYS, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(
        function=mhx.models.gauss_peaks(KEYS[:2], [tuple(KEYS[2:5]), tuple(KEYS[5:8])]),
        data=[x, y], params=params, data_error=sig,
        log_prior=mhx.prior_bounds({KEYS[i]: (lo[i], hi[i]) for i in idx}),
        n_chains=chains, theta0=pb.perturbed(s.theta_star, chains, 0.01, seed=5), seed=41)
    mhx.walker_adaptive_steps(w, iters)
    return w


def median_time(fn, repeats):
    fn()  # warm-up
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def kernel_figures(w, repeats):
    """the percentile kernel alone: HIP-event ms and window bytes read per second"""
    e = w.engine
    fig = {}
    for name, pcts in (("median", [50]), ("eight_percentiles", PCTS8)):
        e.percentiles(TAKE, pcts)
        ms = []
        for _ in range(repeats):
            _, used = e.percentiles(TAKE, pcts)
            ms.append(e.summary_timing())
        m = statistics.median(ms)
        window_bytes = float(used.astype(np.int64).sum()) * e.d * 8
        fig[name] = {"kernel_ms": m, "window_GB_per_s": window_bytes / (m * 1e-3) / 1e9}
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--per-chain-limit", type=int, default=4096)
    ap.add_argument("--kernel-only", action="store_true",
                    help="only the percentile kernel's figures (what the MHX_SUMMARY_NO_LDS child runs)")
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    if a.kernel_only:
        print(json.dumps(kernel_figures(w, a.repeats)))
        return
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE,
           "repeats": a.repeats, "selectors": {}}
    n_pc = min(a.chains, a.per_chain_limit)
    for get in (":median-params", ":covariance-matrix", ":stddev-params"):
        def per_chain():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return [mhx.walker_get(w, get=get, take=TAKE, chain=c) for c in range(n_pc)]

        kms = []

        def batched():
            out = mhx.walker_set_get(w, get=get, take=TAKE)
            kms.append(e.summary_timing())
            return out

        # (a) is minutes of synchronising round trips: one warm-up chain, then `repeats` full passes
        mhx.walker_get(w, get=get, take=TAKE, chain=0)
        ta = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            per_chain()
            ta.append(time.perf_counter() - t0)
        t_a = statistics.median(ta) * (a.chains / n_pc)
        t_b = median_time(batched, a.repeats)
        res["selectors"][get] = {
            "per_chain_s": t_a, "per_chain_extrapolated": n_pc < a.chains,
            "batched_s": t_b, "batched_kernel_ms": statistics.median(kms[1:]),
            "speedup": t_a / t_b}
    res["percentile_kernel_lds"] = kernel_figures(w, a.repeats)
    env = dict(os.environ, MHX_SUMMARY_NO_LDS="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only",
                            "--chains", str(a.chains), "--iters", str(a.iters),
                            "--points", str(a.points), "--repeats", str(a.repeats)],
                           env=env, capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit("the MHX_SUMMARY_NO_LDS child failed:\n" + child.stdout + child.stderr)
    res["percentile_kernel_memory"] = json.loads(child.stdout.strip().splitlines()[-1])
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
