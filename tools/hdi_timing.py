#!/usr/bin/env python3
"""Times the highest-density intervals of a finished fit on one engine.

On the house shape (d = 8, default ring of 1024, a 3000-iteration walk, take 1000, all 8 columns,
masses 95 and 50, a ladder of 101 ranks):

  (a) one Engine.hdi call on the path the library picks (a chain's columns in one workgroup's LDS
      where their keys take 20 KiB at most, else one workgroup per (chain, column)), wall time and
      the HIP-event time of its kernel (mhx_get_summary_timing);
  (b) the same with MHX_HDI_NO_LDS=1 (a child process): one workgroup per (chain, column) whatever
      the shape - at the house shape that is (a)'s path, at --take 100 it is not;
  (c) mhx_get_percentiles with two points on the same engine: what the equal-tailed interval costs;
  (d) the host route, the only way to these numbers before: one Engine.traces call for the set,
      np.sort of every column and the definition's scan in numpy.

Medians of `--repeats` warm calls with the least and the greatest, and the build id.  Prints one
JSON line.

    python tools/hdi_timing.py --chains 4096
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
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAKE, MASSES, LADDER = 1000, [(95, 1), (50, 1)], 101
LDS_BUDGET = 20 << 10       # kHdiLdsBudget (csrc/mhx_plan.hpp)


def default_path(take, n_cols):
    pad = 2
    while pad < take:
        pad *= 2
    return "lds" if 8 * n_cols * (pad + 1) <= LDS_BUDGET else "memory"


def spread(v):
    return {"median": statistics.median(v), "least": min(v), "greatest": max(v)}


def timed(e, fn, repeats):
    """wall and kernel ms of `repeats` calls of fn after one warm-up"""
    fn()
    wall, kernel = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(e.summary_timing())
    return {"wall_ms": spread(wall), "kernel_ms": spread(kernel)}


def host_route(e, repeats):
    """one trace call for the set, a sort of every column, the scan of the definition"""
    cols = list(range(e.d))
    out = {"traces_ms": [], "sort_ms": [], "scan_ms": [], "total_ms": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        tr = e.traces(TAKE, cols)
        t1 = time.perf_counter()
        n = int(tr["n_out"].min())
        s = np.sort(tr["values"][:, :n, :], axis=1)
        t2 = time.perf_counter()
        for num, den in MASSES:
            g = min(n * num // (100 * den), n - 1)
            j = np.argmin(s[:, g:, :] - s[:, :n - g, :], axis=1)
            lo = np.take_along_axis(s, j[:, None, :], axis=1)
            hi = np.take_along_axis(s, j[:, None, :] + g, axis=1)
        ranks = np.arange(LADDER) * (n - 1) // (LADDER - 1)
        ladder = s[:, ranks, :]
        t3 = time.perf_counter()
        for k, v in (("traces_ms", t1 - t0), ("sort_ms", t2 - t1), ("scan_ms", t3 - t2), ("total_ms", t3 - t0)):
            out[k].append(v * 1e3)
    assert lo.shape == hi.shape and ladder.shape[1] == LADDER
    return {k: spread(v) for k, v in out.items()}


def device_figures(e, repeats):
    cols = list(range(e.d))
    return {"hdi": timed(e, lambda: e.hdi(TAKE, MASSES, cols, LADDER), repeats),
            "percentiles_two_points": timed(e, lambda: e.percentiles(TAKE, [(5, 2), (195, 2)]), repeats)}


def main():
    global TAKE
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=700)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--take", type=int, default=TAKE)
    ap.add_argument("--device-only", action="store_true",
                    help="only the device calls' figures (what the MHX_HDI_NO_LDS child runs)")
    a = ap.parse_args()
    TAKE = a.take
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    if a.device_only:
        print(json.dumps(device_figures(e, a.repeats)))
        return
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "chains": a.chains, "d": e.d,
           "ring": e.history_capacity(), "take": TAKE, "masses": MASSES, "ladder": LADDER, "repeats": a.repeats,
           "default_path": default_path(TAKE, e.d)}
    res["default"] = device_figures(e, a.repeats)
    res["host_route"] = host_route(e, min(a.repeats, 3))
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-only", "--chains", str(a.chains),
                            "--iters", str(a.iters), "--points", str(a.points), "--repeats", str(a.repeats), "--take", str(a.take)],
                           env=dict(os.environ, MHX_HDI_NO_LDS="1"), capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit("the MHX_HDI_NO_LDS child failed:\n" + child.stdout + child.stderr)
    res["no_lds"] = json.loads(child.stdout.strip().splitlines()[-1])
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
