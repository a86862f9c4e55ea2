"""CPU checks around mhx_get_waic: the numpy yardstick (tests/waic_cases.py) against mpmath, the
hand case of include/mhx.h's definition, the host-side waic_merge and waic_compare, and carve_waic
(csrc/mhx_stage.hpp) compiled on the CPU.  No device is touched."""
import math
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest

import waic_cases as wc

mpmath.mp.prec = 200

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
U = 2.0 ** -53
B = 1 << 26
CHUNK = 1 << 17


@pytest.fixture(scope="module")
def mirror():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def exact(ell):
    """(lppd_i, M2_i, mean_i) of the columns of ell in 200-bit arithmetic"""
    n, N = ell.shape
    out = []
    for i in range(N):
        col = [mpmath.mpf(float(v)) for v in ell[:, i]]
        top = max(col)
        lse = top + mpmath.log(mpmath.fsum(mpmath.exp(v - top) for v in col) / n)
        mean = mpmath.fsum(col) / n
        out.append((lse, mpmath.fsum((v - mean) ** 2 for v in col), mean))
    return out


# Bounds, from the operation counts of the definition (u = 2^-53):
#   S    n - 1 additions, n - 1 exponentials below one ulp (2 u relative) and, where the maximum
#        moves, a multiplication: every term of S carries at most (3 n) u relative error, all terms
#        are positive, so |dS| <= 3 n u S; the quotient adds u.  log turns that into an ABSOLUTE
#        error of (3 n + 1) u, numpy's log adds u |L|, the final addition u |lppd|.
#   M2   Welford's update is backward stable: Chan, Golub and LeVeque (1983) bound the relative
#        error by n u kappa with kappa = sqrt(1 + n mean^2 / M2); a factor 4 covers the constants
#        of the three operations per step.
def check_against_mpmath(ell):
    n = ell.shape[0]
    y = wc.yardstick(ell)
    for i, (lse, m2, mean) in enumerate(exact(ell)):
        L = abs(float(lse - mpmath.mpf(float(y["acc"][i, 0]))))
        tol = (3 * n + 1) * U + U * L + U * abs(float(lse))
        assert abs(float(mpmath.mpf(float(y["pw_lppd"][i])) - lse)) <= tol, (i, n)
        if n > 1:
            m2f = float(m2)
            kappa = math.sqrt(1.0 + n * float(mean) ** 2 / m2f) if m2f > 0 else 1.0
            assert abs(float(mpmath.mpf(float(y["acc"][i, 3])) - m2)) <= 4 * n * U * kappa * m2f, (i, n)
            assert abs(float(mpmath.mpf(float(y["pw_p"][i])) - m2 / (n - 1))) <= \
                (4 * n * kappa + 1) * U * m2f / (n - 1), (i, n)


def test_the_yardstick_against_mpmath_on_random_terms():
    rng = np.random.default_rng(1)
    for n, N, centre, spread in ((1, 5, -3.0, 1.0), (2, 7, -3.0, 1.0), (3, 7, 0.5, 2.0), (64, 9, -40.0, 5.0),
                                 (300, 6, -900.0, 30.0)):
        check_against_mpmath(centre + spread * rng.standard_normal((n, N)))


def test_a_spread_of_1e4_where_the_naive_mean_of_exp_underflows():
    rng = np.random.default_rng(2)
    ell = -800.0 - 1e4 * rng.random((40, 8))                  # terms in [-10800, -800]
    ell[:, 0] = np.sort(ell[:, 0])                            # the maximum moves at every step
    ell[:, 1] = np.sort(ell[:, 1])[::-1]                      # ... and never
    with np.errstate(all="ignore"):
        naive = np.log(np.mean(np.exp(ell), axis=0))
    assert (ell.max(axis=0) < -750).all() and np.isinf(naive).all()
    assert (ell.max(axis=0) - ell.min(axis=0) > 9000).all()
    y = wc.yardstick(ell)
    assert np.isfinite(y["pw_lppd"]).all() and y["status"] == 0
    check_against_mpmath(ell)


def test_the_hand_case_of_the_definition(mirror):
    """one point, y = 0, sigma = 1, the values 0 (newest) and 2; the status bits and the block are
    the library's, and the two one-step halves pooled by waic_merge give the same point"""
    capi = mirror.capi
    assert (capi.WAIC_NONFINITE, capi.WAIC_ONE_STEP, capi.WAIC_BLOCK) == (wc.NONFINITE, wc.ONE_STEP, wc.BLOCK)
    c = wc.normal_constants([1.0])[0]
    assert c == -0.9189385332046727
    ell = wc.terms(wc.NORMAL, np.array([[0.0], [2.0]]), [0.0], [1.0])
    assert ell[0, 0] == c and ell[1, 0] == c - 2.0
    y = wc.yardstick(ell)
    M, S, mean, m2 = y["acc"][0]
    import oraclelib
    assert M == c and S == 1.0 + float(oraclelib.mirror_gexp(np.array([-2.0]))[0])
    assert mean == c - 1.0 and m2 == 2.0 and y["pw_p"][0] == 2.0
    assert abs(y["pw_lppd"][0] - -1.4851577027216454) <= 2 * U * 1.5
    assert y["n_high"] == 1 and y["status"] == 0
    one = wc.yardstick(ell[:1])
    assert one["status"] == wc.ONE_STEP and np.isnan(one["pw_p"][0]) and one["pw_lppd"][0] == c
    # (delta = -2, one half each: mean and M2 = 4 * 1 * 1 / 2 are exact; S goes through numpy's exp)
    pooled = mirror.waic_merge(np.stack([one["acc"], wc.yardstick(ell[1:])["acc"]]), [1, 1])
    assert pooled["pw_p"][0] == 2.0 and pooled["n"] == 2
    assert abs(pooled["pw_lppd"][0] - -1.4851577027216454) <= 4 * U * 1.5


def test_the_likelihoods_terms(mirror):
    """the yardstick's four term forms, numbered as the library numbers its likelihoods"""
    capi = mirror.capi
    assert (capi.LIK_NORMAL, capi.LIK_NORMAL_CUTOFF, capi.LIK_POISSON, capi.LIK_EXPR) == \
        (wc.NORMAL, wc.CUTOFF, wc.POISSON, wc.EXPR)
    assert "mhx_get_waic" in capi.SIGNATURES and "mhx_group_get_waic" in capi.SIGNATURES
    v = np.array([[2.0, 3.0], [2.5, 200.0]])
    y, s = np.array([2.0, 3.0]), np.array([0.5, 0.25])
    cut = wc.terms(wc.CUTOFF, v, y, s)
    nor = wc.terms(wc.NORMAL, v, y, s)
    assert cut[1, 1] == -5000.0 and nor[1, 1] < -5000.0 and np.array_equal(cut[0], nor[0])
    assert nor[0, 0] == wc.normal_constants(s)[0] - 0.0
    # Poisson: y log(v) - v - log y!, the factorial from single-float logs or lgamma
    yp = np.array([3.0, 0.0])
    for dbl in (False, True):
        got = wc.terms(wc.POISSON, v, yp, logfact_double=dbl)
        want = yp * np.log(v) - v - np.array([math.log(6.0), 0.0])
        assert np.allclose(got, want, rtol=0, atol=1e-6)
    e = wc.terms(wc.EXPR, v, y, s, lik_term=lambda yy, m, err: 0.0 - ((yy - m) / err) * ((yy - m) / err))
    assert e[0, 0] == 0.0 and e[1, 0] == -1.0


def test_waic_merge_of_split_windows(mirror):
    """the accumulators of the parts of a window, pooled, against the yardstick over the whole.
    Tolerances from the merge's operation count with k parts (u = 2^-53): (mean, M2) take 8
    operations per part on top of Welford's n u kappa per part - 4 (n + 8 k) u kappa M2 in all;
    S takes an exp (numpy: 1 ulp), a product and a sum per part on top of the parts' own 3 n u:
    an absolute (3 n + 3 k + 2) u on the log, plus the log's and the addition's ulp."""
    rng = np.random.default_rng(3)
    n, N = 90, 11
    ell = -20.0 + 4.0 * rng.standard_normal((n, N))
    ell[:, 0] += np.linspace(0.0, 300.0, n)                # (the parts' maxima differ widely)
    whole = wc.yardstick(ell)
    for cuts in ([0, 90], [0, 45, 90], [0, 1, 2, 30, 90], [0, 89, 90]):
        k = len(cuts) - 1
        parts = [wc.yardstick(ell[a:b]) for a, b in zip(cuts, cuts[1:])]
        got = mirror.waic_merge(np.stack([p["acc"] for p in parts]), np.diff(cuts))
        assert got["n"] == n
        tols = []
        for i in range(N):
            m2 = whole["acc"][i, 3]
            kappa = math.sqrt(1.0 + n * whole["acc"][i, 2] ** 2 / m2)
            tol_p = 2 * 4 * (n + 8 * k) * U * kappa * m2 / (n - 1)
            assert abs(got["pw_p"][i] - whole["pw_p"][i]) <= tol_p, (cuts, i)
            tol = 2 * (3 * n + 3 * k + 2) * U + 2 * U * (abs(math.log(whole["quot"][i])) + abs(whole["pw_lppd"][i]))
            assert abs(got["pw_lppd"][i] - whole["pw_lppd"][i]) <= tol, (cuts, i)
            tols += [tol_p, tol]
        # elpd: the per-point tolerances above, summed, plus the roundings of the sums themselves -
        # numpy's pairwise sums here and fsum in the yardstick, N u sum |term| at the most each - and
        # of the one subtraction
        total = sum(tols) + 2 * N * U * (np.abs(whole["pw_lppd"]).sum() + np.abs(whole["pw_p"]).sum()) + \
            U * (abs(whole["lppd"]) + abs(whole["p_waic"]))
        assert abs(got["elpd"] - (whole["lppd"] - whole["p_waic"])) <= total, cuts
    with pytest.raises(ValueError):
        mirror.waic_merge(np.zeros((2, 3, 3)), [1, 1])
    with pytest.raises(ValueError):
        mirror.waic_merge(np.zeros((2, 3, 4)), [1, 0])


def test_waic_compare(mirror):
    rng = np.random.default_rng(4)
    a, b = rng.normal(-1.0, 0.3, 50), rng.normal(-1.2, 0.3, 50)
    r = mirror.waic_compare({"pointwise": a}, {"pointwise": b})
    d = a - b
    assert r["elpd-diff"] == float(np.sum(d))
    assert r["se"] == float(np.sqrt(50 * np.var(d, ddof=1)))
    assert mirror.waic_compare(a, a) == {"elpd-diff": 0.0, "se": 0.0}
    with pytest.raises(ValueError):
        mirror.waic_compare(a, b[:49])


# ---- carve_waic on the CPU ---------------------------------------------------------------------------
# "nb_total want m" answers "P chunk|bytes off...|bytes off...": the cursor's portion and chunk, the
# carving of 1 and of P chains at a chunk of points
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17, "the budget and the chunk");
  long long nb, want, m;
  while (scanf("%lld %lld %lld", &nb, &want, &m) == 3) {
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n, int64_t mm) {
      const WaicPieces s = carve_waic(c, nb, (int)want, n, mm);
      off = {s.status, s.n_used, s.n_high, s.elpd, s.lppd, s.p_waic, s.part_lppd, s.part_p, s.part_high,
             s.cst, s.pw_lppd, s.pw_p, s.pw_acc};
    };
    const PortionCursor at = portion_cursor(1, m, carve);
    printf("%lld %lld", (long long)at.per_portion, (long long)at.chunk);
    for (long long n : {1LL, (long long)at.per_portion}) {
      Carver c;
      carve(c, n, at.chunk);
      if ((size_t)c.pieces() != off.size()) printf(" PIECES");
      printf("|%zu", c.bytes());
      for (size_t o : off) printf(" %zu", o);
    }
    printf("\n");
  }
  return 0;
}
'''


def test_carve_waic_alignment_budget_and_a_chunk_of_points():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_waic_stage_")
    try:
        src, exe = os.path.join(d, "waic_driver.cpp"), os.path.join(d, "waic_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
        cases = [(m, want) for m in (1, 255, 256, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 300, 1 << 20)
                 for want in (0, 1, 3, 4, 7)]
        queries = ["%d %d %d" % ((m + 255) // 256, want, m) for m, want in cases]
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")[:-1]
        assert len(out) == len(cases)
        for (m, want), line in zip(cases, out):
            nb, mc = (m + 255) // 256, min(m, CHUNK)
            head, *carvings = line.split("|")
            # per chain: three ints, three doubles, the partials; per point of the chunk what is asked for
            need = [(0, 4), (0, 4), (0, 4), (0, 8), (0, 8), (0, 8), (0, 8 * nb), (0, 8 * nb), (0, 4 * nb),
                    (8 * mc, 0), (0, 8 * mc if want & 1 else 0), (0, 8 * mc if want & 2 else 0),
                    (0, 32 * mc if want & 4 else 0)]
            fixed, per = sum(f for f, _ in need), sum(v for _, v in need)
            want_p = max(1, (B - (fixed + len(need) * 256)) // per)
            assert [int(w) for w in head.split()] == [want_p, mc], (m, want, line)
            for n, carving in zip((1, want_p), carvings):
                total, *off = (int(w) for w in carving.split())
                size = [f + n * v for f, v in need]
                assert len(off) == len(need) and off[0] == 0 and all(o % 256 == 0 for o in off)
                for k in range(len(off)):
                    assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (m, want, n, k)
                assert total <= B, (m, want, n, total)
            # what depends on the chains alone keeps its place whatever the chunk of points is
            first = [int(w) for w in carvings[0].split()][1:10]
            assert first == [256 * k for k in range(6)] + [1536, 1536 + 256 * ((8 * nb + 255) // 256),
                                                           1536 + 512 * ((8 * nb + 255) // 256)]
        assert CHUNK % wc.BLOCK == 0        # a chunk of points is whole blocks of the sums
    finally:
        shutil.rmtree(d, ignore_errors=True)
