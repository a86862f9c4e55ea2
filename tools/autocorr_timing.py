#!/usr/bin/env python3
"""Times the autocorrelation read-out of a finished fit.

On BASELINE config 2's shape (4096 chains, d = 8, ring 1024, a 3000-iteration walk), take 1000,
all 8 columns, max_lag 255:

  (a) one Engine.autocorr call for every chain (mhx_get_autocorr): wall time and the HIP-event
      time of the kernel (mhx_get_summary_timing), the median and the spread of --repeats warm
      calls;
  (b) the same call in a fresh process with MHX_AUTOCORR_NO_LDS=1: every value read from memory;
  (c) Engine.percentiles (mhx_get_percentiles, two points) on the same engine in the same
      process: the kernel that reads the same window and selects;
  (d) the per-chain host route: one mhx_get_trace of the window plus autocorr() per column -
      timed on the first --sample chains, compared bit for bit with (a), and scaled to all of them
      ("extrapolated").

Prints one JSON line.

    python tools/autocorr_timing.py --chains 4096
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

TAKE, MAX_LAG = 1000, 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--device-call-only", action="store_true",
                    help="time (a) alone and print its entry: what the MHX_AUTOCORR_NO_LDS=1 child runs")
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    cols = list(range(e.d))

    def timed(fn, repeats):
        wall, kms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = fn()
            wall.append(time.perf_counter() - t0)
            kms.append(e.summary_timing())
        return out, {"wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall),
                     "kernel_ms": statistics.median(kms), "kernel_ms_min": min(kms), "kernel_ms_max": max(kms)}

    e.autocorr(TAKE, cols, MAX_LAG)  # warm-up
    r, device = timed(lambda: e.autocorr(TAKE, cols, MAX_LAG), a.repeats)
    device["median_tau"] = float(np.nanmedian(r["tau"]))
    device["open"] = int((r["status"] & mhx.capi.AUTOCORR_OPEN != 0).sum())
    if a.device_call_only:
        e.close()
        print(json.dumps(device))
        return
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "max_lag": MAX_LAG,
           "columns": len(cols), "repeats": a.repeats, "window_bytes": a.chains * TAKE * e.d * 8,
           "multiply_add_pairs": int(sum((int(t) - k) * len(cols) for t in r["n_used"] for k in range(MAX_LAG + 1))),
           "autocorr": device}
    e.percentiles(TAKE, [(0, 1), (100, 1)])  # warm-up
    _, res["get_percentiles_same_engine"] = timed(lambda: e.percentiles(TAKE, [(0, 1), (100, 1)]), a.repeats)
    r = e.autocorr(TAKE, cols, MAX_LAG, acf=True)
    n_s = min(a.sample, a.chains)
    mhx.autocorr(e.trace(0, TAKE)[1][:, 0], MAX_LAG)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        _, th = e.trace(c, TAKE)
        for j in cols:
            rho, tau, ess, status = mhx.autocorr(th[:, j], MAX_LAG)
            assert np.array_equal(rho, r["acf"][c, j, :len(rho)], equal_nan=True), (c, j)
            assert (tau == r["tau"][c, j] or tau != tau) and status == r["status"][c, j], (c, j)
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / device["wall_s"]
    e.close()
    # (b): knobs are read when an engine is created, so the other path needs a process of its own
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-call-only", "--chains", str(a.chains),
                            "--iters", str(a.iters), "--points", str(a.points), "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, MHX_AUTOCORR_NO_LDS="1"))
    if child.returncode != 0:
        sys.exit("the MHX_AUTOCORR_NO_LDS=1 run failed:\n" + child.stderr[-3000:])
    res["autocorr_no_lds"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
