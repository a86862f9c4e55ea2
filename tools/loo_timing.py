#!/usr/bin/env python3
"""Times PSIS-LOO of a finished fit, batched on the device and per chain on the host.

On BASELINE config 2's two-peak model (d = 8, ring 1024, a 3000-iteration walk), take 1000, the
dataset's own 1000 points:

  (a) one Engine.loo call for every chain (mhx_get_loo), totals only: wall time and the HIP-event
      time of its kernels (mhx_get_summary_timing), the median and the least and greatest of
      --repeats warm runs after one warm-up; the same with the pointwise outputs;
  (b) the same call in a child process under MHX_LOO_NO_LDS=1 (every pass of the fit's selection
      reads the staged terms), and in a child under `rocprofv3 --kernel-trace --stats`, whose
      per-kernel totals divide the kernel time into values (k_loo_values), fit (k_loo_fit) and
      totals (k_loo_block_sums, k_loo_totals); --no-split leaves the second child out.  Both
      children run before this process opens the device;
  (c) mhx_get_waic and mhx_get_fit_percentiles (2.5 / 50 / 97.5 per cent) on the same engine, the
      same way;
  (d) the per-chain host route: one mhx_get_trace of the window, one mhx_eval_function of its steps
      and the definition in numpy (tests/loo_cases.py, the yardstick) - timed on the first --sample
      chains and scaled to all of them ("extrapolated"); its elpd_loo must agree with the device's to
      1e-9 relative.

Prints one JSON line.

    python tools/loo_timing.py --chains 4096
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAKE = 1000
PCTS = [(5, 2), (50, 1), (195, 2)]
GROUPS = (("values", ("k_loo_values", "mhx_user_loo")), ("fit", ("k_loo_fit",)),
          ("totals", ("k_loo_block_sums", "k_loo_totals")))


def host_route(e, c, y, sig):
    """elpd_loo of chain c from its trace: the yardstick of the definition"""
    import loo_cases as lc
    import waic_cases as wc
    _, th = e.trace(c, TAKE)
    ell = wc.terms(wc.NORMAL, e.eval_function(0, th), y, sig)
    return float(lc.yardstick(ell)["pw_elpd"].sum())


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


def say(what):
    print("loo_timing: " + what, file=sys.stderr, flush=True)


def child(a, env=None, under=()):
    cmd = list(under) + [sys.executable, os.path.abspath(__file__), "--device-call-only", "--chains",
                         str(a.chains), "--iters", str(a.iters), "--points", str(a.points), "--repeats", str(a.repeats)]
    run = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    if run.returncode != 0:
        sys.exit("%r failed:\n" % (cmd,) + run.stderr[-3000:])
    return json.loads(run.stdout.strip().splitlines()[-1])


def kernel_split(a):
    """per call of the totals-only form, from rocprofv3's kernel statistics of a child's 1 + repeats calls"""
    d = tempfile.mkdtemp(prefix="mhx_loo_split_")
    try:
        got = child(a, under=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
        ms = {name: 0.0 for name, _ in GROUPS}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for name, keys in GROUPS:
                    if any(k in row["Name"] for k in keys):
                        ms[name] += float(row["TotalDurationNs"]) * 1e-6 / (1 + a.repeats)
        return {"per_call_kernel_ms": ms, "the_profiled_calls": got}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--no-split", action="store_true", help="no child under rocprofv3")
    ap.add_argument("--device-call-only", action="store_true",
                    help="time the totals-only call alone and print its entry: what the children of (b) run")
    a = ap.parse_args()
    res = {}
    if not a.device_call_only:      # (before this process opens the device)
        say("the child with MHX_LOO_NO_LDS=1")
        res["loo_no_lds"] = child(a, env={"MHX_LOO_NO_LDS": "1"})
        if not a.no_split:
            say("the child under rocprofv3")
            res["kernel_split"] = kernel_split(a)
    import lisp_mcmc_amd as mhx
    import problems as pb
    from summary_timing import make_walker

    w = make_walker(mhx, pb, a.chains, a.iters, a.points)
    e = w.engine
    s = pb.two_peak(n=a.points, seed=12)          # (make_walker's dataset)
    x, y, sig, _ = s.data[0]
    r, t = timed(lambda: e.loo(0, TAKE), e, a.repeats)
    terms = float(r["n_used"].astype(np.int64).sum()) * a.points
    t.update({"terms": terms, "terms_per_s": terms / (t["kernel_ms"] * 1e-3), "tail": mhx.loo_tail_length(TAKE),
              "chains_flagged": int((r["status"] != 0).sum()), "points_above_0.7": int(r["n_high"].sum())})
    if a.device_call_only:
        e.close()
        print(json.dumps(t))
        return
    res.update({"build_id": mhx.capi.lib().mhx_build_id().decode(), "kernel": e.kernel_name(),
                "chains": a.chains, "d": e.d, "ring": e.history_capacity(), "take": TAKE, "points": a.points,
                "repeats": a.repeats, "loo_totals": t})
    say("totals only: %r" % (t,))
    _, res["loo_pointwise"] = timed(lambda: e.loo(0, TAKE, pointwise=True), e, a.repeats)
    _, res["waic_totals"] = timed(lambda: e.waic(0, TAKE), e, a.repeats)
    _, res["fit_percentiles"] = timed(lambda: e.fit_percentiles(0, TAKE, x, PCTS), e, a.repeats)
    n_s = min(a.sample, a.chains)
    host_route(e, 0, y, sig)  # warm-up
    t0 = time.perf_counter()
    for c in range(n_s):
        if c % 8 == 0:
            say("host route, chain %d of %d" % (c, n_s))
        got = host_route(e, c, y, sig)
        assert abs(got - r["elpd_loo"][c]) <= 1e-9 * abs(got), (c, got, r["elpd_loo"][c])
    t_s = time.perf_counter() - t0
    res["per_chain_host_route"] = {"sampled_chains": n_s, "sample_s": t_s,
                                   "all_chains_s": t_s * a.chains / n_s, "extrapolated": n_s < a.chains}
    res["speedup"] = res["per_chain_host_route"]["all_chains_s"] / res["loo_totals"]["wall_s"]
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
