#!/usr/bin/env python3
"""Times a walker set with a dataset per walker (walker_set_create, mhx_set_dataset_planes).

The shape of nv-specific.lisp's maps: --walkers spectra of --points points on one frequency
sweep, two Lorentzian dips on a constant background (MHX_MODEL_LORENTZ_PEAKS {1, 2}, d = 7), one
stddev per spectrum (MHX_SIGMA_PER_CHAIN), walker-adaptive-steps with n = --n for every walker:

  (a) the planes engine, resident form: wall time of init + walk and the kernels' HIP-event time
      (mhx_kernel_timing), at --walkers and at half of them;
  (b) the same with MHX_PLANES_NO_LDS=1 (streamed form; knobs are read when a problem is
      finalised, so a new engine in the same process takes it);
  (c) today's route: one single-walker engine per spectrum, one after another - timed on the
      first --sample spectra and scaled to all of them ("extrapolated");
  (d) a shared-data engine of --walkers walkers on ONE of the spectra: what the walk costs when
      nothing is per walker.

Medians of --repeats warm runs with their least and greatest; the first creation of each kind of
engine (hiprtc, or its on-disk cache) is reported apart as cold_create_s.  Prints one JSON line.

    python tools/planes_timing.py --walkers 4096
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

KEYS = ["bg", "a1", "mu1", "w1", "a2", "mu2", "w2"]
THETA = np.array([1.0, -0.3, 2.82, 0.012, -0.25, 2.92, 0.012])   # two dips of an ODMR sweep (GHz)


def spectra(walkers, points, seed=1):
    rng = np.random.default_rng(seed)
    x = np.linspace(2.7, 3.04, points)
    truth = THETA[None, :] * (1.0 + 0.02 * rng.standard_normal((walkers, THETA.size)))
    sigma = rng.uniform(0.01, 0.02, walkers)
    y = np.empty((walkers, points))
    for c in range(walkers):
        bg, a1, m1, w1, a2, m2, w2 = truth[c]
        y[c] = bg + a1 / (1 + ((x - m1) / w1) ** 2) + a2 / (1 + ((x - m2) / w2) ** 2)
    y += sigma[:, None] * rng.standard_normal((walkers, points))
    start = THETA[None, :] * (1.0 + 0.01 * rng.standard_normal((walkers, THETA.size)))
    return x, y, sigma, start


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--points", type=int, default=334)
    ap.add_argument("--n", type=int, default=30000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16)
    a = ap.parse_args()
    import lisp_mcmc_amd as mhx
    capi = mhx.capi
    x, y, sigma, start = spectra(a.walkers, a.points)

    def define(e, planes, rows):
        e.set_function(0, capi.MODEL_LORENTZ_PEAKS, (1, 2), list(range(7)))
        if planes:
            e.set_dataset_planes(0, x, np.ascontiguousarray(y[rows]), np.ascontiguousarray(sigma[rows]),
                                 capi.SIGMA_PER_CHAIN)
        else:  # every walker on the first spectrum of `rows`
            e.set_dataset(0, x, y[rows][0], np.full(a.points, sigma[rows][0]))
        e.set_bounds(0, [], [], [])
        return e

    def walk(e, th0):
        """one warm run: first steps and walker-adaptive-steps; wall seconds and kernel ms"""
        e.kernel_timing(reset=True)
        steps0 = e.counters()[0]
        t0 = time.perf_counter()
        e.init_chains(th0)
        e.adaptive_steps(a.n)
        wall = time.perf_counter() - t0
        return wall, e.kernel_timing()["total_ms"], e.counters()[0] - steps0

    def measure(planes, rows, no_lds=False):
        os.environ["MHX_PLANES_NO_LDS"] = "1" if no_lds else "0"
        n = len(y[rows])
        t0 = time.perf_counter()
        e = define(mhx.Engine(n, 7, 1, seed=5), planes, rows)
        e.logpost(start[rows][:1])                      # (finalises: compiles or loads the kernels)
        cold = time.perf_counter() - t0
        th0 = start[rows]
        walk(e, th0)                                    # warm-up
        runs = [walk(e, th0) for _ in range(a.repeats)]
        out = {"walkers": n, "kernel": e.kernel_name(), "cold_create_s": cold,
               "wall_s": summary([r[0] for r in runs]), "kernel_ms": summary([r[1] for r in runs]),
               "chain_steps_per_run": int(runs[-1][2])}
        # kernel time per step of the whole set (every walker takes one)
        out["kernel_us_per_set_step"] = out["kernel_ms"]["median"] * 1e3 * n / max(out["chain_steps_per_run"], 1)
        e.close()
        os.environ.pop("MHX_PLANES_NO_LDS", None)
        return out

    res = {"build_id": capi.lib().mhx_build_id().decode(), "points": a.points, "n": a.n,
           "repeats": a.repeats, "model": "lorentz_peaks{1,2}", "sigma_kind": "per_chain"}
    everyone, half = slice(0, a.walkers), slice(0, a.walkers // 2)
    res["a_planes_resident"] = measure(True, everyone)
    res["b_planes_streamed"] = measure(True, everyone, no_lds=True)
    res["a_planes_resident_half"] = measure(True, half)
    res["b_planes_streamed_half"] = measure(True, half, no_lds=True)
    res["d_shared_one_spectrum"] = measure(False, everyone)
    # (c) one single-walker engine per spectrum, sequentially
    n_s = min(a.sample, a.walkers)
    walls, kms = [], []
    warm = define(mhx.Engine(1, 7, 1, seed=5), False, slice(0, 1))
    walk(warm, start[:1])                               # (the kernels are loaded once per process)
    warm.close()
    for c in range(n_s):
        t0 = time.perf_counter()
        e = define(mhx.Engine(1, 7, 1, seed=5, chain_offset=c), False, slice(c, c + 1))
        _, km, _ = walk(e, start[c:c + 1])
        e.close()
        walls.append(time.perf_counter() - t0)
        kms.append(km)
    res["c_one_engine_per_spectrum"] = {
        "sampled_spectra": n_s, "wall_s_per_spectrum": summary(walls), "kernel_ms_per_spectrum": summary(kms),
        "all_spectra_wall_s": statistics.median(walls) * a.walkers, "extrapolated": n_s < a.walkers}
    res["speedup_a_over_c_extrapolated"] = (res["c_one_engine_per_spectrum"]["all_spectra_wall_s"]
                                            / res["a_planes_resident"]["wall_s"]["median"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
