"""What the ensemble-percentile tests share: the yardstick - walker._percentile (nth-percentile
M:1495-1506) on the concatenation of the chains' windows - a Python model of the eight-pass radix
selection over order keys that asks the library's mhx_ensemble_pick for every digit, a small C++
program that runs csrc/mhx_ensemble.hpp's own bookkeeping over a pool, and the GPU cases that are
run a second time in a child process with MHX_ENSEMBLE_NO_LDS=1."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

import histo_cases as hc

PCTS = [50, 2.5, 97.5, 25, 75, 84.1, 0, 100]
TAKES = (1, 7, 64, 1000, 2048)
ALL_ONES = (1 << 64) - 1
TOP = 1 << 63


def ratio(p):
    from fractions import Fraction
    f = Fraction(p).limit_denominator(1000)
    return f.numerator, f.denominator


def order_keys(v):
    """the order-preserving 64-bit key of every double (csrc/mhx_readout_kernels.hpp, order_key): all bits
    of a negative flipped, the sign bit of the others set, every NaN the greatest key"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.uint64)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(TOP))
    return np.where(np.isnan(v), np.uint64(ALL_ONES), k)


def key_value(k):
    k = int(k)
    b = (k ^ TOP) if k >> 63 else (~k & ALL_ONES)
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def yardstick(mhx, pool, pcts=PCTS):
    """walker._percentile of every percentile on every column of pool [N, nc]: [len(pcts), nc]"""
    pool = np.asarray(pool, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.array([[mhx.walker._percentile(p, pool[:, j]) for j in range(pool.shape[1])] for p in pcts])


def pooled(windows, include=None):
    """the concatenation of the included chains' windows [t_c, d]"""
    keep = [th for c, th in enumerate(windows) if include is None or include[c]]
    return np.concatenate(keep, axis=0)


def same(a, b):
    """np.array_equal, a NaN equal to a NaN (-0 equals +0: either may stand for the other)"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def model_select(mhx, values, pcts=PCTS, log=None):
    """the device's selection on one multiset of doubles, in Python: eight passes over the keys,
    each digit from mhx.ensemble_pick on the 256 counts of the keys that share the prefix, then
    the successor rule.  log (a list) receives (pass, counts occupied) of every pick."""
    keys = order_keys(values)
    n = len(keys)
    out = []
    for p in pcts:
        num, den = ratio(p)
        a, b = num * (n - 1), 100 * den
        rank, between = a // b, a % b != 0
        prefix, run = 0, n
        for ps in range(8):
            shift = 56 - 8 * ps
            mask = 0 if shift == 56 else (ALL_ONES << (shift + 8)) & ALL_ONES
            cand = keys[(keys & np.uint64(mask)) == np.uint64(prefix)]
            assert len(cand) == run
            counts = np.bincount(((cand >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
            digit, rank, run = mhx.ensemble_pick(counts.astype(np.uint64), rank)
            prefix |= digit << shift
            if log is not None:
                log.append((ps, int((counts > 0).sum())))
        lo = key_value(prefix)
        if not between:
            out.append(lo)
            continue
        nxt = prefix if rank + 1 < run else int(keys[keys > np.uint64(prefix)].min())
        with np.errstate(all="ignore"):
            out.append(float((np.float64(lo) + np.float64(key_value(nxt))) / 2))
    return np.array(out)


def special_values():
    """the doubles that try an order: negatives, both zeros, subnormals, infinities, neighbours in
    the last bit"""
    tiny = np.float64(5e-324)
    base = np.array([0.0, -0.0, tiny, -tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 1.5,
                     -2.5, 1e-3, -1e5, 7.0, -0.125, 1e308, -1e308, np.inf, -np.inf])
    finite = base[np.isfinite(base)]
    return np.concatenate([base, np.nextafter(finite, np.inf), np.nextafter(finite, -np.inf)])


def multisets():
    """{name: doubles} for the host model"""
    rng = np.random.default_rng(1495)
    sp = special_values()
    out = {
        "one": np.array([3.25]),
        "two": np.array([2.0, -1.0]),
        "special": sp,
        "special_runs": np.repeat(sp, rng.integers(1, 40, len(sp))),
        "equal": np.full(257, -0.75),
        "zeros": np.array([0.0, -0.0] * 33 + [0.0]),
        "normal": rng.normal(0.0, 2.0, 1001),
        "runs": np.repeat(rng.normal(1.0, 1e-9, 40), rng.integers(1, 60, 40)),
        "last_bit": 1.0 + np.arange(300) * np.finfo(np.float64).eps,
        "nan_one": np.concatenate([rng.normal(0.0, 1.0, 99), [np.nan]]),
        "nan_many": np.concatenate([sp, [np.nan, -np.nan, np.nan]]),
        "wide": np.concatenate([rng.normal(0, 1, 200) * 10.0 ** rng.integers(-300, 300, 200), sp]),
    }
    for k in out:
        out[k] = rng.permutation(out[k])
    return out


# ---- csrc/mhx_ensemble.hpp through a small compiled program: "nc npct N chains" on one line, the
# percentiles (num den) on the next, then the pool column by column as hex bit patterns.  It runs
# the header's own bookkeeping - first tasks, targets, tasks, advance, successor tasks - with a CPU
# loop in the kernel's place, and prints the tasks of every pass, the values as bits, the carving.
DRIVER = r'''
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "mhx_ensemble.hpp"
using namespace mhx;
int main() {
  static_assert(kEnsMaxTasks == 1008 && kEnsBins == 256 && kEnsPasses == 8, "the shapes of the call");
  int nc, npct;
  long long N, chains;
  while (scanf("%d %d %lld %lld", &nc, &npct, &N, &chains) == 4) {
    PctList pc{};
    pc.n = npct;
    for (int q = 0; q < npct; ++q)
      if (scanf("%d %d", &pc.num[q], &pc.den[q]) != 2) return 1;
    std::vector<std::vector<uint64_t>> key(nc, std::vector<uint64_t>(N));
    for (int c = 0; c < nc; ++c)
      for (long long i = 0; i < N; ++i) {
        uint64_t bits;
        if (scanf("%" SCNx64, &bits) != 1) return 1;
        double v;
        memcpy(&v, &bits, 8);
        key[c][i] = ensemble_order_key(v);
        if (ensemble_order_key(ensemble_key_value(key[c][i])) != key[c][i]) return 2;
      }
    const int max_tasks = ensemble_max_tasks(nc, npct), nt_all = nc * npct;
    std::vector<EnsTask> tasks(max_tasks);
    std::vector<EnsTarget> t(nt_all);
    std::vector<uint64_t> counts;
    auto count = [&](int nt) {
      counts.assign((size_t)nt * kEnsBins, 0);
      for (int k = 0; k < nt; ++k)
        for (uint64_t x : key[tasks[k].col])
          if ((x & ensemble_mask(tasks[k].shift)) == tasks[k].prefix)
            ++counts[(size_t)k * kEnsBins + ((x >> tasks[k].shift) & 255)];
    };
    int nt = ensemble_first_tasks(nc, tasks.data());
    printf("tasks %d", nt);
    count(nt);
    long long pooled = 0;
    for (int b = 0; b < kEnsBins; ++b) pooled += (long long)counts[b];
    ensemble_targets(pooled, pc, nc, t.data());
    for (int p = 0; p < kEnsPasses && nt_all > 0; ++p) {
      if (p > 0) {
        nt = ensemble_tasks(t.data(), nt_all, ensemble_shift(p), tasks.data());
        if (nt > max_tasks) return 3;
        printf(" %d", nt);
        count(nt);
      }
      if (!ensemble_advance(t.data(), nt_all, ensemble_shift(p), counts.data())) return 4;
    }
    nt = ensemble_successor_tasks(t.data(), nt_all, tasks.data());
    printf(" succ %d", nt);
    std::vector<uint64_t> least(nt > 0 ? nt : 1, ~(uint64_t)0);
    for (int k = 0; k < nt; ++k)
      for (uint64_t x : key[tasks[k].col])
        if (x > tasks[k].prefix && x < least[k]) least[k] = x;
    ensemble_take_successors(t.data(), nt_all, least.data());
    printf(" pooled %lld values", pooled);
    for (int k = 0; k < nt_all; ++k) {
      const double v = ensemble_value(t[k]);
      uint64_t bits;
      memcpy(&bits, &v, 8);
      printf(" %016" PRIx64, bits);
    }
    Carver cv;
    const EnsemblePieces s = carve_ensemble(cv, max_tasks, nc, chains);
    printf(" carve %d %zu %zu %zu %zu %zu %zu %d\n", max_tasks, s.counters, s.tasks, s.include, s.n_used, s.status,
           cv.bytes(), cv.bytes() <= kStageBudget ? 1 : 0);
  }
  return 0;
}
'''


def bookkeeping_answers(cases):
    """the driver's answer lines for cases [(pool [N, nc], pcts, n_chains)]; None without g++"""
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    lines = []
    for pool, pcts, chains in cases:
        pool = np.ascontiguousarray(pool, dtype=np.float64)
        lines.append("%d %d %d %d" % (pool.shape[1], len(pcts), pool.shape[0], chains))
        lines.append(" ".join("%d %d" % ratio(p) for p in pcts))
        for j in range(pool.shape[1]):
            lines.append(" ".join("%x" % b for b in pool[:, j].copy().view(np.uint64)))
    d = tempfile.mkdtemp(prefix="mhx_ensemble_")
    try:
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                               os.path.join(hc.ROOT, "lisp-mcmc_amd", "csrc"), "-o", exe, src])
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = out.split("\n")
    assert len(out) == len(cases) + 1 and out[-1] == ""
    return out[:-1]


def distinct_prefixes(pool, pcts, n_pass):
    """how many distinct (column, leading n_pass bytes of the key at pos) the percentiles have"""
    pool = np.asarray(pool, dtype=np.float64)
    n = pool.shape[0]
    seen = set()
    for j in range(pool.shape[1]):
        keys = np.sort(order_keys(pool[:, j]))
        for p in pcts:
            num, den = ratio(p)
            k = int(keys[num * (n - 1) // (100 * den)])
            seen.add((j, k >> (64 - 8 * n_pass) if n_pass else 0))
    return len(seen)


# ---- the GPU cases

def crafted_d3(mhx):
    """11 chains of d = 3, ring 2048, one walk of every length that matters: repeated steps, ties,
    neighbours in the last bit (hc.crafted_walk)"""
    rng = np.random.default_rng(1506)
    e = hc.line_engine(mhx, len(hc.LENGTHS), d=3, used=(0, 2), history_capacity=2048)
    e.init_chains([-1.0, 0.5, 2.0])
    assert e.history_capacity() == 2048
    hc.inject(e, rng, hc.LENGTHS)
    return e


def wide_engine(mhx):
    """3 chains of d = 63, 2048 steps each: 63 columns of 2048 keys are beyond a workgroup's LDS"""
    rng = np.random.default_rng(63)
    e = hc.line_engine(mhx, 3, d=63, used=range(0, 32, 4), history_capacity=2048)
    e.init_chains(np.linspace(-1.0, 2.0, 63))
    hc.inject(e, rng, [2048, 2048, 2048])
    return e


def call(e, take, cols=None, include=None, pcts=PCTS):
    return e.ensemble_percentiles(take, pcts, cols, include)


def both_paths_cases(mhx):
    """the calls whose bits must not depend on where the keys are read from: {name: result}.
    "*_windows": theta of every chain newest first, for the yardstick of that process's walks."""
    out = {}
    e = crafted_d3(mhx)
    for take in TAKES:
        out["d3_%d" % take] = call(e, take)
    out["d3_cols"] = call(e, 1000, [2, 0])
    out["d3_mask"] = call(e, 1000, None, [c % 3 != 1 for c in range(e.n_chains)])
    e.close()
    e = wide_engine(mhx)
    out["wide"] = call(e, 2048)
    out["wide_few"] = call(e, 2048, [62, 0, 31])      # three columns of 2048 keys do fit
    e.close()
    return {k: {n: np.asarray(v) for n, v in r.items()} for k, r in out.items()}


_memo = {}


def lds_results(mhx):
    if "here" not in _memo:
        _memo["here"] = both_paths_cases(mhx)
    return _memo["here"]


def no_lds_results(tmp_path_factory):
    """both_paths_cases() of a fresh child process with MHX_ENSEMBLE_NO_LDS=1 (knobs are read when
    an engine is created), once"""
    if "child" not in _memo:
        path = str(tmp_path_factory.mktemp("ensemble") / "no_lds.npz")
        code = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import numpy as np, lisp_mcmc_amd as mhx, ensemble_cases\n"
                "r = ensemble_cases.both_paths_cases(mhx)\n"
                "np.savez(%r, **{n + '.' + k: v for n, d in r.items() for k, v in d.items()})\n"
                "print('ok')\n" % (hc.ROOT, hc.TESTS, path))
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, MHX_ENSEMBLE_NO_LDS="1"))
        assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-3000:]
        flat = np.load(path)
        got = {}
        for key in flat.files:
            name, k = key.split(".")
            got.setdefault(name, {})[k] = flat[key]
        _memo["child"] = got
    return _memo["child"]
