"""What the highest-density-interval tests share: the numpy yardstick of mhx_get_hdi's definition
(include/mhx.h) - a sort by order key, one subtraction per width, the first argmin - the engines with
injected histories, and the cases that are run a second time in a child process with
MHX_HDI_NO_LDS=1.  Everything is compared on the float bits."""
import os
import subprocess
import sys

import numpy as np

import histo_cases as hc
from test_gpu_walker_set_get import LENGTHS, crafted_walk

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
NAN_KEY = np.uint64(2 ** 64 - 1)
NAN_BITS = np.uint64(0x7FFFFFFFFFFFFFFF)     # the NaN mhx_get_percentiles returns for any NaN
TAKES = (1, 2, 57, 1000, 2048)
ISSUE_MASSES = [(95, 1), (50, 1), (10, 1), (100, 1), (1365, 20)]
MASSES = ISSUE_MASSES + [(1, 1000)]          # the last one: g = 0 at these window lengths
LADDERS = (2, 101, 4096)
COLS33 = [32, 0, 7]


def span(n, num, den):
    """g of a mass of num/den per cent among n values, in Python's integers"""
    return min(n * num // (100 * den), n - 1)


def order_keys(x):
    """the device's 64-bit order keys: negatives with every bit flipped, the others with the sign
    bit set, any NaN the greatest key"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(x), NAN_KEY, k)


def ascending(x):
    """x in ascending order of its keys, as bits: -0 before +0, every NaN last and canonical"""
    k = np.sort(order_keys(x))
    return np.where(k >> np.uint64(63) != 0, k ^ np.uint64(1 << 63), ~k)


def column(x, masses, ladder):
    """the definition on one column's window x (any order of its steps): lo, hi as bits and pos
    [n_mass], the ladder as bits [ladder], the status, and per mass how many positions share the
    least width"""
    n = len(x)
    s = ascending(x)
    v = s.view(np.float64)
    lo, hi = np.zeros(len(masses), dtype=np.uint64), np.zeros(len(masses), dtype=np.uint64)
    pos, ties = np.zeros(len(masses), dtype=np.int32), np.zeros(len(masses), dtype=np.int64)
    for q, (num, den) in enumerate(masses):
        g = span(n, num, den)
        with np.errstate(all="ignore"):
            w = v[g:] - v[:n - g]
        j = int(np.argmin(w))
        lo[q], hi[q], pos[q], ties[q] = s[j], s[j + g], j, int((w == w[j]).sum())
    rungs = s[np.arange(ladder, dtype=np.int64) * (n - 1) // max(ladder - 1, 1)]    # floor(i (n - 1) / (L - 1))
    return lo, hi, pos, rungs, int(not np.isfinite(x).all()), ties


def want_hdi(windows, cols, masses, ladder=0):
    """the yardstick for every chain: a dict shaped like Engine.hdi's with lo, hi and ladder as
    uint64 bits, and `ties` [n, n_mass, n_cols].  windows: theta [t, d] of every chain's window, or
    with cols None the staged values [n_cols, t] of every chain"""
    n, nm = len(windows), len(masses)
    nc = len(cols) if cols is not None else len(windows[0])
    out = {"lo": np.zeros((n, nm, nc), dtype=np.uint64), "hi": np.zeros((n, nm, nc), dtype=np.uint64),
           "pos": np.zeros((n, nm, nc), dtype=np.int32), "ladder": np.zeros((n, nc, ladder), dtype=np.uint64),
           "n_used": np.zeros(n, dtype=np.int32), "status": np.zeros((n, nc), dtype=np.int32),
           "ties": np.zeros((n, nm, nc), dtype=np.int64)}
    for c, th in enumerate(windows):
        for j in range(nc):
            x = th[:, cols[j]] if cols is not None else th[j]
            out["n_used"][c] = len(x)
            (out["lo"][c, :, j], out["hi"][c, :, j], out["pos"][c, :, j], out["ladder"][c, j],
             out["status"][c, j], out["ties"][c, :, j]) = column(np.ascontiguousarray(x), masses, ladder)
    return out


def bits(got):
    """Engine.hdi's dict with its doubles as bits"""
    return {k: (np.ascontiguousarray(v).view(np.uint64) if v.dtype == np.float64 else v) for k, v in got.items()}


def same(got, want):
    """None, or where Engine.hdi's result differs from the yardstick (or from another result):
    every output of every chain and column, but lo, hi and pos of a column whose status is set"""
    got, want = bits(got), bits(want)
    for k in ("n_used", "status", "ladder", "lo", "hi", "pos"):
        a, b = got[k], want[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            return k, a.shape, b.shape, a.dtype, b.dtype
        if k in ("lo", "hi", "pos"):
            keep = np.broadcast_to((want["status"] == 0)[:, None, :], a.shape)
            a, b = a[keep], b[keep]
        if not np.array_equal(a, b):
            return k, np.argwhere(a != b)[:5].tolist()
    return None


def d2_walks():
    """the 300 crafted histories of tests/test_gpu_walker_set_get.py's d = 2 test: kinds 0-5, its
    LENGTHS six times over and random lengths"""
    rng = np.random.default_rng(2024)
    lengths = LENGTHS * 6 + list(rng.integers(1, 2049, 300 - 6 * len(LENGTHS)))
    return [crafted_walk(rng, int(n), 2, c % 6) for c, n in enumerate(lengths)]


def d33_walks():
    rng = np.random.default_rng(33)
    lengths = LENGTHS + list(rng.integers(1, 2049, 40 - len(LENGTHS)))
    return [crafted_walk(rng, int(n), 33, c % 6) for c, n in enumerate(lengths)]


def engine_of(mhx, walks, **kw):
    d = walks[0][1].shape[1]
    e = hc.line_engine(mhx, len(walks), d=d, used=(0, 1) if d == 2 else range(0, 32, 4), **kw)
    e.init_chains(np.linspace(-1.0, 2.0, d))
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
    return e


def windows_of(walks, take):
    return [th[:take] for _, th in walks]


def nonfinite_walks():
    """5 chains of 40 steps, d = 3; NONFINITE_HIT marks the columns that hold a NaN or an infinity"""
    rng = np.random.default_rng(3)
    walks = [rng.normal(0.0, 2.0, (40, 3)) for _ in range(5)]
    walks[1][3, 0] = np.nan
    walks[2][0, 1] = -np.inf
    walks[3][39, 2] = np.inf
    walks[4][7, 0], walks[4][8, 0], walks[4][20, 2] = -np.nan, np.inf, -np.inf
    return [(rng.normal(-5.0, 1.0, 40), th) for th in walks]


NONFINITE_HIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1]], dtype=bool)


def both_paths_cases(mhx):
    """the calls of the crafted d = 2 and d = 33 tests, whose bits must not depend on where the
    window is sorted: {name: Engine.hdi's result}"""
    out = {}
    e = engine_of(mhx, d2_walks(), history_capacity=2048)
    for take in TAKES:
        for ladder in LADDERS:
            out["d2_%d_%d" % (take, ladder)] = e.hdi(take, MASSES, [0, 1], ladder)
    e.close()
    e = engine_of(mhx, d33_walks(), history_capacity=2048)
    for take in TAKES:
        out["d33_%d" % take] = e.hdi(take, MASSES, COLS33, 101)
    out["d33_all_57"] = e.hdi(57, MASSES, None, 2)      # 33 columns of 64 keys: every wave sorts eight or nine
    e.close()
    return out


_memo = {}


def lds_results(mhx):
    """both_paths_cases() of this process, once"""
    if "here" not in _memo:
        _memo["here"] = both_paths_cases(mhx)
    return _memo["here"]


def no_lds_results(tmp_path_factory):
    """... and of a fresh child process with MHX_HDI_NO_LDS=1 (knobs are read when an engine is
    created), once"""
    if "child" not in _memo:
        path = str(tmp_path_factory.mktemp("hdi") / "no_lds.npz")
        code = ("import sys; sys.path[:0] = [%r, %r]\n"
                "import numpy as np, lisp_mcmc_amd as mhx, hdi_cases\n"
                "r = hdi_cases.both_paths_cases(mhx)\n"
                "np.savez(%r, **{n + '.' + k: v for n, d in r.items() for k, v in d.items()})\n"
                "print('ok')\n" % (ROOT, TESTS, path))
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, MHX_HDI_NO_LDS="1"))
        assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-3000:]
        flat = np.load(path)
        got = {}
        for key in flat.files:
            name, k = key.split(".")
            got.setdefault(name, {})[k] = flat[key]
        _memo["child"] = got
    return _memo["child"]


# "nc n_mass n_ladder take with_values key_pitch" answers "P fits|bytes off...|bytes off..."; "p take
# nc no_lds" answers "use_lds lds_bytes pad": carve_hdi's portion and carving, and the path rule
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_plan.hpp"
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26, "the budget");
  static_assert(kHdiLdsBudget == (size_t)20 << 10, "an eighth of a CU's LDS");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    if (line[0] == 'p') {
      int take, nc, off;
      if (sscanf(line + 1, "%d %d %d", &take, &nc, &off) != 3) return 1;
      EngineKnobs k;
      k.hdi_no_lds = off != 0;
      printf("%d %zu %lld\n", hdi_use_lds(take, nc, k) ? 1 : 0, hdi_lds_bytes(take, nc), (long long)hdi_pad(take));
      continue;
    }
    int nc, nm, nl, take, wv;
    long long kp;
    if (sscanf(line, "%d %d %d %d %d %lld", &nc, &nm, &nl, &take, &wv, &kp) != 6) return 1;
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n) {
      const HdiPieces s = carve_hdi(c, nc, nm, nl, take, wv, kp, n);
      off = {s.values, s.lo, s.hi, s.pos, s.ladder, s.n_used, s.status, s.keys};
    };
    const long long P = portion_of(carve);
    printf("%lld %d", P, one_item_fits(carve) ? 1 : 0);
    for (long long n : {1LL, P}) {
      Carver c;
      carve(c, n);
      if ((size_t)c.pieces() != off.size()) printf(" PIECES");
      printf("|%zu", c.bytes());
      for (size_t o : off) printf(" %zu", o);
    }
    printf("\n");
  }
  return 0;
}
'''


def carve_need(nc, nm, nl, take, with_values, key_pitch):
    """bytes per chain of every piece of carve_hdi, in the buffer's order"""
    return [8 * nc * take if with_values else 0, 8 * nm * nc, 8 * nm * nc, 4 * nm * nc, 8 * nc * nl, 4, 4 * nc,
            8 * nc * key_pitch]


def pad(take):
    p = 2
    while p < take:
        p *= 2
    return p


def driver_answers(queries):
    """the answers of csrc/mhx_stage.hpp and mhx_plan.hpp to `queries`, from a small program
    compiled against the headers; None without a C++ compiler"""
    import shutil
    import tempfile
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    d = tempfile.mkdtemp(prefix="mhx_hdi_stage_")
    try:
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                               os.path.join(ROOT, "lisp-mcmc_amd", "csrc"), "-o", exe, src])
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True,
                             text=True, check=True).stdout.split("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert len(out) == len(queries) + 1 and out[-1] == ""
    return out[:-1]


def portion(nc, nm, nl, take, with_values, key_pitch):
    """the chains of one portion by carve_hdi's own answer"""
    answer = driver_answers(["%d %d %d %d %d %d" % (nc, nm, nl, take, with_values, key_pitch)])
    assert answer is not None, "a C++ compiler is needed to ask csrc/mhx_stage.hpp"
    return int(answer[0].split()[0])
