"""What the histogram and pair-grid GPU tests share: engines with injected histories, the host
yardstick - a chain's trace plus the bin rule (a value falls in bin n = the smallest n in 1..B with
v <= edge n: bisect_left from index 1) - and the cases that are run a second time in a child
process with MHX_HISTO_NO_LDS=1."""
import os
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
LENGTHS = [1, 2, 3, 9, 10, 64, 65, 1023, 1024, 2047, 2048]
LF_X, LF_Y = [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0]


def line_engine(mhx, n_chains, d=2, used=(0, 1), **kw):
    """the five-point line fit over the parameters `used` of a vector of d (the histories are
    injected: the model does not matter)"""
    e = mhx.Engine(n_chains, d, 1, **kw)
    e.set_function(0, mhx.capi.MODEL_POLY, (), list(used))
    e.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    return e


def crafted_walk(rng, n, d, kind):
    """a walk of n steps, NEWEST FIRST (prob [n], theta [n][d]):
    0 a Metropolis-like walk: runs of repeated steps, negative values
    1 the same over a handful of parameter values that recur, some of them neighbours in the last
      bit: the extremes recur, values sit exactly on the first and last edges and next to them
    2 a drifting walk that moves at every step"""
    prob, theta = np.empty(n), np.empty((n, d))
    base = np.array([1.0, -2.5, 1e-3, -1e5, 0.0, 7.0, -0.125])
    pool = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)])
    p, th = rng.normal(-50.0, 3.0), rng.normal(0.0, 2.0, d)
    for i in range(n):
        if kind == 2 or i == 0 or rng.random() < 0.4:
            p = rng.normal(-50.0, 3.0)
            th = rng.choice(pool, d) if kind == 1 else th + rng.normal(0.0, 0.3, d)
        prob[i], theta[i] = p, th
    return prob[::-1].copy(), theta[::-1].copy()


def inject(e, rng, lengths):
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted_walk(rng, int(n), e.d, c % 3))


def crafted_d2(mhx):
    """300 chains of d = 2, ring 2048, walks of every length that matters and random ones"""
    rng = np.random.default_rng(1361)
    e = line_engine(mhx, 300, history_capacity=2048)
    e.init_chains([-1.0, 2.0])
    assert e.history_capacity() == 2048
    inject(e, rng, LENGTHS * 6 + list(rng.integers(1, 2049, 300 - 6 * len(LENGTHS))))
    return e


def crafted_d33(mhx):
    """40 chains of d = 33, ring 2048"""
    rng = np.random.default_rng(33)
    e = line_engine(mhx, 40, d=33, used=range(0, 32, 4), history_capacity=2048)
    e.init_chains(np.linspace(-1.0, 2.0, 33))
    inject(e, rng, LENGTHS + list(rng.integers(1, 2049, 40 - len(LENGTHS))))
    return e


COLS33 = [32, 0, 7]
PAIRS = [(0, 1), (2, 0), (1, 2)]


def narrow_edges(n_cols, bins):
    """one set of edges for every chain, narrower than the data of the crafted walks"""
    return np.array([np.linspace(-1.5 - 0.1 * j, 1.25 + 0.2 * j, bins + 1) for j in range(n_cols)])


def reference_edges(mhx, e, take, cols, bins):
    """make-histo's own boundaries for every chain and column, from the device's 0 and 100 per
    cent points of the window"""
    pct, _ = e.percentiles(take, [(0, 1), (100, 1)])
    return np.array([[mhx.histo_edges(pct[c, 0, p], pct[c, 1, p], bins) for p in cols]
                     for c in range(e.n_chains)])


def places(edges, v):
    """the bin rule on a column v: below (bool), the bin index 0..B-1 or B for above; NaN apart"""
    edges = np.asarray(edges)
    nan = np.isnan(v)
    k = np.searchsorted(edges[1:], v, side="left")     # bisect_left from index 1
    return (v < edges[0]) & ~nan, k, nan


def traces(e, take):
    """theta [t, d] newest first of every chain's window: e.trace(c, take)"""
    return [e.trace(c, take)[1] for c in range(e.n_chains)]


def want_histograms(windows, cols, edges):
    """the yardstick for every chain: counts, outside, n_used, status from traces(e, take)"""
    n, nc, nb = len(windows), len(cols), np.asarray(edges).shape[-1] - 1
    out = {"counts": np.zeros((n, nc, nb), dtype=np.int32), "outside": np.zeros((n, nc, 2), dtype=np.int32),
           "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, nc), dtype=np.int32)}
    for c, th in enumerate(windows):
        out["n_used"][c] = len(th)
        for j, p in enumerate(cols):
            b = edges[c, j] if np.asarray(edges).ndim == 3 else edges[j]
            below, k, nan = places(b, th[:, p])
            ok = ~below & ~nan
            out["counts"][c, j] = np.bincount(k[ok & (k < nb)], minlength=nb)
            out["outside"][c, j] = below.sum(), (ok & (k == nb)).sum()
            out["status"][c, j] = nan.any()
    return out


def want_pair_grids(windows, cols, pairs, edges):
    n, nb = len(windows), np.asarray(edges).shape[-1] - 1
    out = {"counts": np.zeros((n, len(pairs), nb, nb), dtype=np.int32),
           "n_inside": np.zeros((n, len(pairs)), dtype=np.int32),
           "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, len(pairs)), dtype=np.int32)}
    for c, th in enumerate(windows):
        out["n_used"][c] = len(th)
        col = []
        for j, p in enumerate(cols):
            b = edges[c, j] if np.asarray(edges).ndim == 3 else edges[j]
            below, k, nan = places(b, th[:, p])
            col.append((k, ~below & ~nan & (k < nb), nan.any()))
        for q, (a, b) in enumerate(pairs):
            both = col[a][1] & col[b][1]
            np.add.at(out["counts"][c, q], (col[a][0][both], col[b][0][both]), 1)
            out["n_inside"][c, q] = both.sum()
            out["status"][c, q] = col[a][2] or col[b][2]
    return out


def same(got, want):
    return list(got) == list(want) and all(
        got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in want)


def both_paths_cases(mhx):
    """the calls whose counts must not depend on where they are accumulated: {name: result dict}"""
    out = {}
    e = crafted_d2(mhx)
    for bins in (1, 20, 1024):
        out["h2_%d" % bins] = e.histograms(1000, [0, 1], reference_edges(mhx, e, 1000, [0, 1], bins))
    out["g2"] = e.pair_grids(1000, [0, 1], [(0, 1), (1, 0)], reference_edges(mhx, e, 1000, [0, 1], 20))
    e.close()
    e = crafted_d33(mhx)
    for take in (57, 2048):
        out["h33_%d" % take] = e.histograms(take, COLS33, narrow_edges(3, 20))
        out["g33_%d" % take] = e.pair_grids(take, COLS33, PAIRS, narrow_edges(3, 7))
    e.close()
    return out


_memo = {}


def lds_results(mhx):
    """both_paths_cases() of this process, once"""
    if "here" not in _memo:
        _memo["here"] = both_paths_cases(mhx)
    return _memo["here"]


def no_lds_results(tmp_path_factory):
    """... and of the child, once"""
    if "child" not in _memo:
        _memo["child"] = in_child_without_lds(str(tmp_path_factory.mktemp("histo") / "no_lds.npz"))
    return _memo["child"]


def in_child_without_lds(path):
    """both_paths_cases() in a fresh process with MHX_HISTO_NO_LDS=1 (knobs are read when an engine
    is created), saved to `path` and loaded back"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, lisp_mcmc_amd as mhx, histo_cases\n"
            "r = histo_cases.both_paths_cases(mhx)\n"
            "np.savez(%r, **{n + '.' + k: v for n, d in r.items() for k, v in d.items()})\n"
            "print('ok')\n" % (ROOT, TESTS, path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, MHX_HISTO_NO_LDS="1"))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-3000:]
    flat = np.load(path)
    got = {}
    for key in flat.files:
        name, k = key.split(".")
        got.setdefault(name, {})[k] = flat[key]
    return got
