#!/usr/bin/env python3
"""Times derived quantities (walker-with-exp and its posterior) of a finished fit.

On BASELINE config 2's shape (4096 chains, d = 8, ring 1024, a 3000-iteration walk), take 1000,
four bodies - the two peak areas, the amplitude ratio and the first peak's FWHM, 2 sqrt(log 2) |w1|
(one sqrt and one log per step) - and the percentiles 50 / 2.5 / 97.5:

  (a) one Engine.derived call for every chain (mhx_get_derived): wall time and the HIP-event time
      of its two kernels (mhx_get_summary_timing).  COLD: the first call of the process with an
      empty on-disk cache, which compiles the expressions' module with hiprtc; WARM: the median of
      --repeats further calls.
  (b) the per-chain host route: one mhx_get_trace of the window plus numpy - timed on the first
      --sample chains and scaled to all of them ("extrapolated");
  (c) Engine.percentiles (mhx_get_percentiles) with the same percentiles on the same engine in the
      same process: the nearest existing kernel - 8 columns, the same selection.

Prints one JSON line.

    python tools/derived_timing.py --chains 4096
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAKE, PCTS = 1000, [50, 2.5, 97.5]
NAMES, INDEX = ["a1", "w1", "a2", "w2"], [2, 4, 5, 7]   # b0 b1 A1 mu1 w1 A2 mu2 w2
SQRT_PI = "sqrt(3.14159265358979323846)"
BODIES = ["a1 * w1 * " + SQRT_PI, "a2 * w2 * " + SQRT_PI, "a2 / a1", "2.0 * sqrt(log(2.0)) * abs(w1)"]


def host_route(e, c):
    prob, th = e.trace(c, TAKE)
    a1, w1, a2, w2 = (th[:, j] for j in INDEX)
    vals = np.stack([a1 * w1 * np.sqrt(np.pi), a2 * w2 * np.sqrt(np.pi), a2 / a1,
                     2.0 * np.sqrt(np.log(2.0)) * np.abs(w1)])
    return np.percentile(vals, PCTS, axis=1), vals.mean(axis=1), vals.std(axis=1, ddof=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    # an empty on-disk cache of compiled modules: the cold call compiles
    os.environ["MHX_RTC_CACHE_DIR"] = tempfile.mkdtemp(prefix="mhx_derived_timing_")
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE,
           "bodies": BODIES, "percentiles": PCTS, "repeats": a.repeats,
           "window_bytes": a.chains * TAKE * e.d * 8}

    def timed(fn, repeats):
        wall, kms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = fn()
            wall.append(time.perf_counter() - t0)
            kms.append(e.summary_timing())
        return out, statistics.median(wall), statistics.median(kms), min(kms), max(kms)

    call = lambda: e.derived(BODIES, NAMES, INDEX, TAKE, PCTS)  # noqa: E731
    _, cw, ck, _, _ = timed(call, 1)
    res["cold"] = {"wall_s": cw, "kernel_ms": ck}
    r, ww, wk, wlo, whi = timed(call, a.repeats)
    res["warm"] = {"wall_s": ww, "kernel_ms": wk, "kernel_ms_min": wlo, "kernel_ms_max": whi,
                   "values": float(r["n_used"].astype(np.int64).sum()) * len(BODIES),
                   "flagged": int(r["status"].sum())}
    e.percentiles(TAKE, PCTS)  # warm-up
    _, pw, pk, plo, phi = timed(lambda: e.percentiles(TAKE, PCTS), a.repeats)
    res["get_percentiles_same_engine"] = {"columns": e.d, "wall_s": pw, "kernel_ms": pk,
                                          "kernel_ms_min": plo, "kernel_ms_max": phi}
    n_s = min(a.sample, a.chains)
    host_route(e, 0)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        hp, hm, _ = host_route(e, c)
        # (numpy's percentile interpolates and its mean sums pairwise: a sanity check, not the test)
        assert np.allclose(hm, r["mean"][c], rtol=1e-12), c
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s,
                                   "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / ww
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
