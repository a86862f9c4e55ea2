#!/usr/bin/env python3
"""Times the posterior histograms and pair-count grids of a finished fit.

On BASELINE config 2's shape (4096 chains, d = 8, ring 1024, a 3000-iteration walk), take 1000,
20 bins, all 8 columns and all 28 pairs, make-histo's own edges per chain:

  (a) one Engine.histograms call and one Engine.pair_grids call for every chain
      (mhx_get_histograms, mhx_get_pair_grids): wall time and the HIP-event time of the kernel
      (mhx_get_summary_timing), the median and the spread of --repeats warm calls; the edges are
      formed before the clock starts (their cost on the host is reported apart);
  (b) the per-chain host route: one mhx_get_trace of the window plus numpy's searchsorted and
      bincount - timed on the first --sample chains and scaled to all of them ("extrapolated");
  (c) Engine.percentiles (mhx_get_percentiles) for the 0 and 100 per cent points on the same
      engine in the same process: the kernel that reads the same window and selects.

Prints one JSON line.

    python tools/histo_timing.py --chains 4096
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

TAKE, BINS = 1000, 20


def host_route(e, c, edges, pairs):
    """the histograms and grids of chain c from its trace"""
    _, th = e.trace(c, TAKE)
    d = th.shape[1]
    k = np.stack([np.searchsorted(edges[c, j, 1:], th[:, j], side="left") for j in range(d)])
    histo = np.stack([np.bincount(k[j][k[j] < BINS], minlength=BINS) for j in range(d)])
    grids = []
    for a, b in pairs:
        ok = (k[a] < BINS) & (k[b] < BINS)
        grids.append(np.bincount(k[a][ok] * BINS + k[b][ok], minlength=BINS * BINS).reshape(BINS, BINS))
    return histo, np.stack(grids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    cols = list(range(e.d))
    pairs = [(i, j) for i in range(e.d) for j in range(i + 1, e.d)]
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "bins": BINS,
           "columns": len(cols), "pairs": len(pairs), "repeats": a.repeats,
           "window_bytes": a.chains * TAKE * e.d * 8}

    def timed(fn, repeats):
        wall, kms = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = fn()
            wall.append(time.perf_counter() - t0)
            kms.append(e.summary_timing())
        return out, {"wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall),
                     "kernel_ms": statistics.median(kms), "kernel_ms_min": min(kms), "kernel_ms_max": max(kms)}

    e.percentiles(TAKE, [(0, 1), (100, 1)])  # warm-up
    (pct, _), res["get_percentiles_same_engine"] = timed(lambda: e.percentiles(TAKE, [(0, 1), (100, 1)]),
                                                         a.repeats)
    t0 = time.perf_counter()
    edges = np.array([[mhx.histo_edges(pct[c, 0, j], pct[c, 1, j], BINS) for j in cols]
                      for c in range(a.chains)])
    res["edges_on_the_host_s"] = time.perf_counter() - t0
    e.histograms(TAKE, cols, edges)  # warm-up
    h, res["histograms"] = timed(lambda: e.histograms(TAKE, cols, edges), a.repeats)
    e.pair_grids(TAKE, cols, pairs, edges)  # warm-up
    g, res["pair_grids"] = timed(lambda: e.pair_grids(TAKE, cols, pairs, edges), a.repeats)
    res["histograms"]["counted"] = int(h["counts"].astype(np.int64).sum())
    res["pair_grids"]["counted"] = int(g["counts"].astype(np.int64).sum())
    n_s = min(a.sample, a.chains)
    host_route(e, 0, edges, pairs)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        hh, gg = host_route(e, c, edges, pairs)
        assert np.array_equal(hh, h["counts"][c]) and np.array_equal(gg, g["counts"][c]), c
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / \
        (res["histograms"]["wall_s"] + res["pair_grids"]["wall_s"])
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
