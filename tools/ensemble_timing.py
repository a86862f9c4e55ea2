#!/usr/bin/env python3
"""Times the ensemble percentiles of a finished fit: one posterior from all chains.

On BASELINE config 2's shape (4096 chains, d = 8, ring 1024, a walk that fills the ring), take
1000, all 8 columns, the 2.5 / 50 / 97.5 per cent points:

  (a) one Engine.ensemble_percentiles call (mhx_get_ensemble_percentiles): wall time and the
      HIP-event time of the kernels of all its passes (mhx_get_summary_timing), the median and the
      spread of --repeats warm calls;
  (b) the same call in a fresh process with MHX_ENSEMBLE_NO_LDS=1: every pass reads its columns
      from memory;
  (c) Engine.percentiles (mhx_get_percentiles, the same three points, per chain) on the same
      engine in the same process: the kernel that reads the same windows once and selects;
  (d) the host route: one mhx_get_trace of the window per chain, the traces concatenated, numpy's
      selection (np.partition) per column and point - timed on the first --sample chains, compared
      bit for bit with the device's answer for those chains (an include mask), and scaled to all
      of them ("extrapolated").

Prints one JSON line.

    python tools/ensemble_timing.py --chains 4096
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

TAKE, PCTS = 1000, [2.5, 50, 97.5]


def host_points(mhx, pool):
    """nth-percentile of every point on every column of pool [N, nc] by selection, not a sort"""
    n = len(pool)
    out = np.empty((len(PCTS), pool.shape[1]))
    for q, p in enumerate(PCTS):
        num, den = mhx.engine.percentile_ratio(p)
        a, b = num * (n - 1), 100 * den
        pos = a // b
        for j in range(pool.shape[1]):
            if a % b:
                part = np.partition(pool[:, j], [pos, pos + 1])
                out[q, j] = (part[pos] + part[pos + 1]) / 2
            else:
                out[q, j] = np.partition(pool[:, j], pos)[pos]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--device-call-only", action="store_true",
                    help="time (a) alone and print its entry: what the MHX_ENSEMBLE_NO_LDS=1 child runs")
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

    e.ensemble_percentiles(TAKE, PCTS, cols)  # warm-up
    r, device = timed(lambda: e.ensemble_percentiles(TAKE, PCTS, cols), a.repeats)
    device["n_pooled"] = int(r["n_pooled"])
    device["median_of_column_0"] = float(r["out"][1, 0])
    if a.device_call_only:
        e.close()
        print(json.dumps(device))
        return
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "percentiles": PCTS,
           "columns": len(cols), "repeats": a.repeats, "window_bytes": a.chains * TAKE * e.d * 8,
           "ensemble": device}
    e.percentiles(TAKE, PCTS)  # warm-up
    _, res["get_percentiles_same_engine"] = timed(lambda: e.percentiles(TAKE, PCTS), a.repeats)
    # (d) on the first chains, against the device's answer for exactly those chains
    n_s = min(a.sample, a.chains)
    mask = np.arange(a.chains) < n_s
    part = e.ensemble_percentiles(TAKE, PCTS, cols, mask)
    e.trace(0, TAKE)  # warm-up
    t0 = time.perf_counter()
    traces = [e.trace(c, TAKE)[1] for c in range(n_s)]
    t_fetch = time.perf_counter() - t0
    t0 = time.perf_counter()
    pool = np.concatenate(traces, axis=0)
    host = host_points(mhx, pool)
    t_select = time.perf_counter() - t0
    assert np.array_equal(host, part["out"]) and part["n_pooled"] == len(pool), "the device and the host route differ"
    scale = a.chains / n_s
    res["host_route"] = {"sampled_chains": n_s, "fetch_s": t_fetch, "select_s": t_select,
                         "all_chains_s": (t_fetch + t_select) * scale, "extrapolated": n_s < a.chains}
    res["speedup"] = res["host_route"]["all_chains_s"] / device["wall_s"]
    e.close()
    # (b): knobs are read when an engine is created, so the other path needs a process of its own
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-call-only", "--chains", str(a.chains),
                            "--iters", str(a.iters), "--points", str(a.points), "--repeats", str(a.repeats)],
                           capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, MHX_ENSEMBLE_NO_LDS="1"))
    if child.returncode != 0:
        sys.exit("the MHX_ENSEMBLE_NO_LDS=1 run failed:\n" + child.stderr[-3000:])
    res["ensemble_no_lds"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
