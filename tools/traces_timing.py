#!/usr/bin/env python3
"""Times the batched traces of a finished fit (mhx_get_traces, Engine.traces).

On BASELINE config 2's shape (4096 chains, d = 8, ring 1024, a 3000-iteration walk), take 1000:

  (a) every column (prob and the 8 parameters), every step: what comes back is the whole window,
      chains x take x 9 doubles;
  (b) one column, every step;
  (c) every column, every 16th step with the envelope of the 16 (three arrays of 63 rows);
  (d) every column of the :unique-steps;
  (e) the per-chain host route for each of them: one mhx_get_trace of the window plus numpy's
      filter, thinning and extremes - timed on the first --sample chains and scaled to all of them
      ("extrapolated"), and compared with what the batched call returned for those chains.

For (a)-(d): wall time and the HIP-event time of the kernel (mhx_get_summary_timing), the median
and the spread of --repeats warm calls.  Prints one JSON line.

    python tools/traces_timing.py --chains 4096
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

TAKE, STRIDE = 1000, 16


def host_route(e, c, cols, filt, stride, envelope):
    """(values, lo, hi) of chain c from its trace: [rows, n_cols] each (lo, hi None without envelope)"""
    prob, th = e.trace(c, TAKE)
    table = np.column_stack([prob if j < 0 else th[:, j] for j in cols])
    if filt == "unique":
        bits = prob.view(np.uint64)
        table = table[np.r_[bits[:-1] != bits[1:], True]]
    values = table[::stride]
    if not envelope:
        return values, None, None
    at = np.arange(0, len(table), stride)
    return values, np.minimum.reduceat(table, at, axis=0), np.maximum.reduceat(table, at, axis=0)


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
    every = [mhx.capi.TRACE_PROB] + list(range(e.d))
    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
           "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "stride": STRIDE,
           "repeats": a.repeats}
    cases = {"a_all_columns": dict(cols=every, filt="steps", stride=1, envelope=False),
             "b_one_column": dict(cols=[3], filt="steps", stride=1, envelope=False),
             "c_stride_16_envelope": dict(cols=every, filt="steps", stride=STRIDE, envelope=True),
             "d_unique_all_columns": dict(cols=every, filt="unique", stride=1, envelope=False)}
    n_s = min(a.sample, a.chains)
    host_route(e, 0, every, "steps", 1, False)  # warm-up
    for name, k in cases.items():
        def call():
            return e.traces(TAKE, k["cols"], filter=k["filt"], stride=k["stride"], envelope=k["envelope"])
        call()  # warm-up
        wall, kms = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = call()
            wall.append(time.perf_counter() - t0)
            kms.append(e.summary_timing())
        row = {"wall_s": statistics.median(wall), "wall_s_min": min(wall), "wall_s_max": max(wall),
               "kernel_ms": statistics.median(kms), "kernel_ms_min": min(kms), "kernel_ms_max": max(kms),
               "bytes_back": int(sum(v.nbytes for v in r.values())), "rows": int(r["n_out"].sum())}
        same = True
        t0 = time.perf_counter()
        for c in range(n_s):
            got = host_route(e, c, k["cols"], k["filt"], k["stride"], k["envelope"])
            for side, v in zip(("values", "lo", "hi"), got):
                if v is not None:
                    same = same and np.array_equal(v, r[side][c, :int(r["n_out"][c])])
        t_s = time.perf_counter() - t0
        row["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s, "all_chains_s": t_s * a.chains / n_s,
                                       "extrapolated": n_s < a.chains, "same_as_the_batched_call": bool(same)}
        row["speedup"] = row["per_chain_host_route"]["all_chains_s"] / row["wall_s"]
        res[name] = row
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
