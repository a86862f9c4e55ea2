"""The yardstick of mhx_get_heldout: include/mhx.h's definition restated in numpy on top of
tests/waic_cases.py - the same terms and the same log-sum-exp recurrence - with what the held-out
read-out adds: Welford's moments of the model VALUES, the use mask, and the block-ordered total.
And a small C++ program over csrc/mhx_heldout.hpp, the host-pure half of the call: what it refuses,
the arrays it prepares and the pieces it carves, asked on the CPU.

Input everywhere: the model VALUES v [n, m] at the window's steps, newest first: what
e.eval_function(fn, theta_steps, x) returns for the theta of e.trace(c, ring)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import waic_cases as wc

NONFINITE, NO_POINTS = 1, 2
BLOCK = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_NONE, SIGMA_SHARED, SIGMA_PER_CHAIN, SIGMA_PER_POINT = 0, 1, 2, 3
NONE, ONE, SHARED, SCALAR, PLANE = 0, 1, 2, 3, 4      # how a prepared array varies (kHo*)


def value_moments(v):
    """(mean_v, M2_v) [m] of the values v [n, m], newest first: Welford with q_k = 1.0 / k"""
    v = np.asarray(v, dtype=np.float64)
    mean, m2 = np.zeros(v.shape[1]), np.zeros(v.shape[1])
    with np.errstate(all="ignore"):
        for s in range(v.shape[0]):
            qk = 1.0 / float(s + 1)
            delta = v[s] - mean
            mean = mean + delta * qk
            m2 = m2 + delta * (v[s] - mean)
    return mean, m2


def block_sum(pw):
    """the total of a pointwise quantity in mhx_get_waic's order: per block of 256 points lane
    j = i mod 64 adds its points serially from 0.0 (a point beyond the end adds 0.0), the 64 lane
    sums are added pairwise, lanes 32 apart first, then the blocks serially from 0.0"""
    pw = np.asarray(pw, dtype=np.float64)
    nb = (pw.size + BLOCK - 1) // BLOCK
    padded = np.zeros(nb * BLOCK)
    padded[:pw.size] = pw
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        for b in range(nb):
            rows = padded[b * BLOCK:(b + 1) * BLOCK].reshape(BLOCK // 64, 64)
            u = np.zeros(64)
            for row in rows:
                u = u + row
            for m in (32, 16, 8, 4, 2, 1):
                u = u + u[np.arange(64) ^ m]
            total = total + u[0]
    return float(total)


def yardstick(ell, v, use=None):
    """everything but the device's own log: acc [m, 4] = (M, S, mean_v, M2_v), quot = S / n, pw_lpd
    with numpy's log (within an ulp of the device's), n_scored and the status bits; a point that is
    not used is 0.0 everywhere and what it evaluates to flags nothing"""
    ell = np.asarray(ell, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    n, m = ell.shape
    used = np.ones(m, dtype=bool) if use is None else np.asarray(use) != 0
    M, S, _, _ = wc.accumulate(ell)
    mean_v, m2_v = value_moments(v)
    with np.errstate(all="ignore"):
        quot = S / np.float64(n)
        pw = M + np.log(quot)
    acc = np.column_stack([M, S, mean_v, m2_v])
    acc[~used] = 0.0
    finite = np.isfinite(ell[:, used]).all() and np.isfinite(v[:, used]).all()
    status = (0 if finite and n > 0 else NONFINITE) | (0 if used.any() else NO_POINTS)
    return {"acc": acc, "quot": quot, "pw_lpd": np.where(used, pw, 0.0), "used": used,
            "n_scored": int(used.sum()), "status": status}


def sigma_rows(sigma, kind, n_chains, m):
    """sigma per (chain, point) [n_chains, m] of a sigma array of its kind (none: 1)"""
    if kind == SIGMA_NONE:
        return np.ones((n_chains, m))
    s = np.asarray(sigma, dtype=np.float64)
    if kind == SIGMA_SHARED:
        return np.repeat(s[None, :], n_chains, axis=0)
    if kind == SIGMA_PER_CHAIN:
        return np.repeat(s[:, None], m, axis=1)
    return s.reshape(n_chains, m)


# ---- the host-pure half, asked through a small program -----------------------------------------------
# Every query is a line of integers followed by the lines of data it needs (hexadecimal doubles; use
# bytes as integers):
#   "V lik ypc sk C m" + y + sigma                        ->  "0", or "-1 <the refusal>"
#   "F lik lfd ypc sk with_use upc C m c0 n m0 mc" + y + sigma + use
#                                                          ->  "Lys Lw Lc Luse" then ys, w, c, use
#   "C nb want Lys Lw Lc Luse m"                           ->  "P fits|bytes off...|bytes off..." for 1
#                                                              chain and for the P of one portion
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "mhx_heldout.hpp"
using namespace mhx;
static std::vector<double> doubles(const std::string& line) {
  std::vector<double> v;
  std::istringstream in(line);
  std::string w;
  while (in >> w) v.push_back(strtod(w.c_str(), nullptr));
  return v;
}
static void show(const std::vector<double>& v) {
  for (double d : v) printf("%a ", d);
  printf("\n");
}
int main() {
  static_assert(kStageBudget == (size_t)1 << 26, "the budget");
  std::string line, ly, ls, lu;
  while (std::getline(std::cin, line)) {
    std::istringstream q(line);
    char what;
    q >> what;
    if (what == 'V') {
      int lik, ypc, sk;
      long long C, m;
      q >> lik >> ypc >> sk >> C >> m;
      std::getline(std::cin, ly), std::getline(std::cin, ls);
      const std::vector<double> y = doubles(ly), s = doubles(ls);
      char msg[160] = "";
      const int rc = heldout_validate(lik, y.data(), ypc, s.empty() ? nullptr : s.data(), sk, C, m, msg, sizeof msg);
      printf("%d %s\n", rc, msg);
    } else if (what == 'F') {
      int lik, lfd, ypc, sk, wu, upc;
      long long C, m, c0, n, m0, mc;
      q >> lik >> lfd >> ypc >> sk >> wu >> upc >> C >> m >> c0 >> n >> m0 >> mc;
      std::getline(std::cin, ly), std::getline(std::cin, ls), std::getline(std::cin, lu);
      const std::vector<double> y = doubles(ly), s = doubles(ls), ud = doubles(lu);
      std::vector<uint8_t> use(ud.begin(), ud.end());
      HeldoutData D;
      D.y = y.data(), D.sigma = s.empty() ? nullptr : s.data(), D.use = wu ? use.data() : nullptr;
      D.y_per_chain = ypc, D.sigma_kind = sk, D.use_per_chain = upc, D.m = m;
      const HeldoutLayout L = heldout_layout(lik, ypc, sk, wu != 0, upc);
      // (exactly as large as the kinds say: a write past an end is the sanitizer's to find)
      std::vector<double> ys(heldout_elems(L.ys, n, mc)), w(heldout_elems(L.w, n, mc)), c(heldout_elems(L.c, n, mc));
      std::vector<uint8_t> us(heldout_elems(L.use, n, mc));
      std::vector<float> cache;
      heldout_fill(lik, lfd != 0, L, D, c0, n, m0, mc, ys.data(), w.data(), c.data(), us.data(), cache);
      printf("%d %d %d %d %lld %d %lld %d\n", L.ys, L.w, L.c, L.use, (long long)heldout_pitch(L.w, mc),
             heldout_step(L.w), (long long)heldout_pitch(L.ys, mc), heldout_step(L.c));
      show(ys), show(w), show(c);
      for (uint8_t b : us) printf("%d ", (int)b);
      printf("\n");
    } else if (what == 'C') {
      long long nb, m;
      int want;
      HeldoutLayout L;
      q >> nb >> want >> L.ys >> L.w >> L.c >> L.use >> m;
      std::vector<size_t> off;
      auto carve = [&](Carver& cv, int64_t n) {
        const HeldoutPieces s = carve_heldout(cv, nb, want, L, n, m);
        off = {s.status, s.n_used, s.n_scored, s.lpd, s.part_lpd, s.part_scored, s.x0, s.x1, s.ys, s.w, s.c, s.use,
               s.pw_lpd, s.pw_acc};
      };
      const long long P = portion_of(carve);
      printf("%lld %d", P, one_item_fits(carve) ? 1 : 0);
      for (long long n : {1LL, P}) {
        Carver cv;
        carve(cv, n);
        if ((size_t)cv.pieces() != off.size()) printf(" PIECES");
        printf("|%zu", cv.bytes());
        for (size_t o : off) printf(" %zu", o);
      }
      printf("\n");
    } else {
      return 1;
    }
  }
  return 0;
}
'''

_exe = {}


def _driver(sanitize):
    if sanitize not in _exe:
        gxx = shutil.which("g++")
        assert gxx is not None, "a C++ compiler is needed to ask csrc/mhx_heldout.hpp"
        d = tempfile.mkdtemp(prefix="mhx_heldout_")
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I",
                               os.path.join(ROOT, "lisp-mcmc_amd", "csrc"), "-o", exe, src])
        _exe[sanitize] = (d, exe)
    return _exe[sanitize][1]


def cleanup():
    for d, _ in _exe.values():
        shutil.rmtree(d, ignore_errors=True)
    _exe.clear()


def hexes(a):
    return " ".join(float(v).hex() for v in np.asarray(a, dtype=np.float64).reshape(-1))


def ask(text, sanitize=False):
    """the program's answer lines to the query text"""
    out = subprocess.run([_driver(sanitize)], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def ask_validate(lik, y, sigma, kind, n_chains, m):
    ya = np.asarray(y, dtype=np.float64)
    line = "V %d %d %d %d %d\n%s\n%s\n" % (lik, int(ya.ndim == 2), kind, n_chains, m, hexes(ya),
                                            "" if sigma is None else hexes(sigma))
    rc, _, msg = ask(line)[0].partition(" ")
    return int(rc), msg


def ask_fill(lik, logfact_double, y, sigma, kind, use, n_chains, m, c0, n, m0, mc, sanitize=False):
    """(kinds, extras, ys, w, c, use) of chains [c0, c0 + n) at points [m0, m0 + mc)"""
    ya = np.asarray(y, dtype=np.float64)
    ua = None if use is None else np.asarray(use, dtype=np.uint8)
    text = "F %d %d %d %d %d %d %d %d %d %d %d %d\n%s\n%s\n%s\n" % (
        lik, int(logfact_double), int(ya.ndim == 2), kind, int(ua is not None), int(ua is not None and ua.ndim == 2),
        n_chains, m, c0, n, m0, mc, hexes(ya), "" if sigma is None else hexes(sigma),
        "" if ua is None else " ".join(str(int(b)) for b in ua.reshape(-1)))
    head, ys, w, c, us = ask(text, sanitize)
    nums = [int(t) for t in head.split()]
    arr = [np.array([float.fromhex(t) for t in line.split()], dtype=np.float64) for line in (ys, w, c)]
    return nums[:4], nums[4:], arr[0], arr[1], arr[2], np.array([int(t) for t in us.split()], dtype=np.uint8)


def elems(kind, n, m):
    return {NONE: 0, ONE: 1, SHARED: m, SCALAR: n, PLANE: n * m}[kind]


def carve_need(nb, want, kinds, m):
    """(bytes fixed, bytes per chain) of every piece of carve_heldout, in the buffer's order"""
    per_kind = [(elems(k, 0, m), elems(k, 1, m) - elems(k, 0, m)) for k in kinds]
    fixed = [0, 0, 0, 0, 0, 0, 8 * m, 8 * m] + [8 * f for f, _ in per_kind[:3]] + [per_kind[3][0], 0, 0]
    per = [4, 4, 4, 8, 8 * nb, 4 * nb, 0, 0] + [8 * p for _, p in per_kind[:3]] + [
        per_kind[3][1], 8 * m if want & 1 else 0, 32 * m if want & 2 else 0]
    return fixed, per
