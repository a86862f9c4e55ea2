#!/usr/bin/env python3
"""Times the candidate search: many starts per walker in ONE device call, against the routes there
were before it.

Two shapes, at the walkers' starting points (no walk: this is what runs BEFORE one):

  planes   --chains spectra of 334 points, a dataset per walker (tools/planes_timing.py's ODMR
           sweeps, one stddev per spectrum, d = 7), and a shared 17 x 17 grid over the two centres
  shared   --chains walkers on BASELINE config 2's two-peak model (d = 8) and its 1e5 points, one
           shared dataset, and 64 shared candidates

For each:

  (a) one Engine.candidate_scores call (mhx_get_candidate_scores): wall time and the HIP-event time
      of its kernels (mhx_get_summary_timing), the median and the least and greatest of --repeats
      warm runs after one warm-up;
  (b) m Engine.residuals calls, one per candidate with the candidate in every row - the route there
      was: wall time and the sum of the calls' kernel times, the same statistics.  The device's
      scores must equal their chi2 BIT FOR BIT on the first --sample chains, and (a) must not take
      longer than (b) in wall time: that is the call's reason to exist;
  (c) on the shared dataset only, one Engine.logpost of n_chains x m rows: another sum (the walk's
      own sweep, with the prior), timed for the ratio alone.

and, on the first shape, walker_set_search(apply=True) followed by walker_set_least_squares (25
iterations) of the whole set: how many walkers end without a Cholesky factor and the median Newton
decrement - beside the same polish without the search.

Prints one JSON line.

    python tools/cand_timing.py --chains 4096
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(wall, kms):
    return {"wall_s": statistics.median(wall), "wall_s_min_max": [min(wall), max(wall)],
            "kernel_ms": statistics.median(kms), "kernel_ms_min_max": [min(kms), max(kms)]}


def timed(fn, repeats):
    """fn() -> (result, kernel ms); one warm-up, then `repeats` timed runs"""
    fn()
    wall, kms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out, k = fn()
        wall.append(time.perf_counter() - t0)
        kms.append(k)
    return out, stats(wall, kms)


def measure(e, cand, repeats, sample, with_logpost):
    n, m = e.n_chains, cand.shape[0]
    pts = e._datasets[0][0]
    rows = [np.ascontiguousarray(np.tile(cand[j], (n, 1))) for j in range(m)]

    def one_call():
        r = e.candidate_scores(cand, fn=0, keep=4, scores=True)
        return r, e.summary_timing()

    def residual_calls():
        chi, k = np.empty((n, m)), 0.0
        for j in range(m):
            chi[:, j] = e.residuals(0, rows[j])["chi2"]
            k += e.summary_timing()
        return chi, k
    r, t_one = timed(one_call, repeats)
    chi, t_res = timed(residual_calls, repeats)
    s = min(sample, n)
    same = (r["score"][:s].view(np.uint64) == (0.0 + chi[:s]).view(np.uint64)) | ~np.isfinite(r["score"][:s])
    assert same.all(), "the device's scores are not the residual calls' chi2: %s" % np.argwhere(~same)[:4].tolist()
    assert (r["best_index"][:s, 0] == np.argmin(r["score"][:s], axis=1)).all()
    evals = n * m * pts
    t_one.update({"model_values": evals, "model_values_per_s": evals / (t_one["kernel_ms"] * 1e-3),
                  "candidates_not_finite": int(r["n_bad"].sum())})
    out = {"candidates": m, "one_call": t_one, "residual_calls": t_res,
           "wall_ratio_residual_calls_to_one_call": t_res["wall_s"] / t_one["wall_s"],
           "kernel_ratio_residual_calls_to_one_call": t_res["kernel_ms"] / t_one["kernel_ms"],
           "bits_checked_on_chains": s}
    assert t_one["wall_s"] <= t_res["wall_s"], ("one call took longer than the residual calls", t_one, t_res)
    if with_logpost:
        every = np.ascontiguousarray(np.repeat(cand[None, :, :], n, axis=0).reshape(n * m, -1))
        e.logpost(every)
        wall = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            e.logpost(every)
            wall.append(time.perf_counter() - t0)
        out["one_logpost_of_all_rows"] = {"rows": n * m, "wall_s": statistics.median(wall),
                                          "wall_s_min_max": [min(wall), max(wall)]}
        out["wall_ratio_logpost_to_one_call"] = statistics.median(wall) / t_one["wall_s"]
    return out


def polish_report(mhx, w, iterations, theta0=None):
    t0 = time.perf_counter()
    r = mhx.walker_set_least_squares(w, iterations=iterations, theta0=theta0)
    dt = time.perf_counter() - t0
    dec = np.array([s["newton-decrement"] if s["status"] == 0 else np.nan for s in r["laplace"]])
    red = np.array([s["reduced-chi2"] if s["reduced-chi2"] is not None else np.nan for s in r["laplace"]])
    return {"wall_s": dt, "iterations": iterations,
            "walkers_not_positive_or_finite": int(np.isnan(dec).sum()),
            "median_newton_decrement": float(np.nanmedian(dec)),
            "walkers_with_decrement_below_1e-8": int((dec <= 1e-8).sum()),
            "median_reduced_chi2": float(np.nanmedian(red)),
            "walkers_with_reduced_chi2_above_1.5": int((red > 1.5).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--plane-points", type=int, default=334)
    ap.add_argument("--grid", type=int, default=17)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--only", choices=["shared", "planes"], default=None)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    import problems as pb
    from planes_timing import spectra, KEYS, THETA

    res = {"build_id": mhx.capi.lib().mhx_build_id().decode(), "chains": a.chains, "repeats": a.repeats}
    if a.only != "shared":
        x, y, sigma, start = spectra(a.chains, a.plane_points)
        w = mhx.walker_set_create(function=mhx.models.lorentz_peaks(KEYS[:1], [KEYS[1:4], KEYS[4:7]]),
                                  datasets=[[x, y[c]] for c in range(a.chains)],
                                  params=[dict(zip(KEYS, start[c])) for c in range(a.chains)],
                                  data_error=[float(v) for v in sigma], seed=5)
        e = w.engine
        # the two centres over the sweep: ten widths either way of where the dips usually are
        axes = {"mu1": np.linspace(2.70, 2.94, a.grid), "mu2": np.linspace(2.80, 3.04, a.grid)}
        cand, shape = mhx.candidate_grid(dict(zip(KEYS, THETA)), axes)
        out = measure(e, cand, a.repeats, a.sample, False)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.plane_points, "d": e.d, "grid": list(shape)})
        out["least_squares_alone"] = polish_report(mhx, w, a.iterations)
        t0 = time.perf_counter()
        found = mhx.walker_set_search(w, candidates=cand, keep=4, apply=True)
        out["search"] = {"wall_s": time.perf_counter() - t0, "keep": 4,
                         "walkers_without_a_finite_candidate": sum(1 for s in found if s["index"] < 0)}
        out["search_then_least_squares"] = polish_report(mhx, w, a.iterations)
        res["planes"] = out
        e.close()
    if a.only != "planes":
        s = pb.two_peak(n=a.points, seed=12)
        e = s.engine(mhx, a.chains, seed=41)
        e.init_chains(pb.perturbed(s.theta_star, a.chains, 0.01, seed=5))
        cand = pb.perturbed(s.theta_star, a.candidates, 0.05, seed=6)
        out = measure(e, cand, a.repeats, a.sample, True)
        out.update({"kernel": e.kernel_name(), "points_per_chain": a.points, "d": e.d})
        res["shared"] = out
        e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
