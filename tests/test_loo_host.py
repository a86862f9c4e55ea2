"""CPU checks around mhx_get_loo: mhx_loo_tail_length against its rule, the numpy yardstick
(tests/loo_cases.py) against exact generalised-Pareto samples, a closed-form leave-one-out density and
200-bit mpmath, the hand cases of include/mhx.h's definition, carve_loo (csrc/mhx_stage.hpp) compiled
on the CPU, and the constants and signatures of the binding.  No device is touched."""
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np
import pytest

import loo_cases as lc
import waic_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
U = 2.0 ** -53
B = 1 << 26
CHUNK = 1 << 17


@pytest.fixture(scope="module")
def mirror():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


# ---- the tail length ---------------------------------------------------------------------------------
RULE = {1: 0, 24: 0, 25: 5, 64: 12, 300: 52, 1000: 95, 1024: 96, 8192: 272, 65536: 768}


def test_tail_length_rule_overrides_and_clamp(mirror):
    capi, lib = mirror.capi, mirror.capi.lib()

    def M(n, tail=0):
        out = C.c_int32(-7)
        assert lib.mhx_loo_tail_length(n, tail, C.byref(out)) == capi.OK
        assert out.value == lc.tail_length(n, tail) == mirror.loo_tail_length(n, tail)
        return out.value
    for n, want in RULE.items():
        assert M(n) == want, n
    for n in list(range(0, 200)) + [4999, 5000, 5119, 5120, 5121, 10 ** 6, 2 ** 31, 2 ** 62]:
        r = math.isqrt(9 * n)
        r += r * r < 9 * n
        want = min(n // 5, r, capi.LOO_MAX_TAIL)
        assert M(n) == (want if want >= 5 else 0), n
    # the caller's tail: never longer than a fifth of the window, never below 5, never above the limit
    assert [M(1000, t) for t in (1, 4, 5, 40, 200, 201, 1024)] == [0, 0, 5, 40, 200, 200, 200]
    assert M(24, 5) == 0 and M(25, 5) == 5 and M(29, 6) == 5 and M(30, 6) == 6
    assert M(65536, 1024) == 1024 and M(5120, 1024) == 1024 and M(5119, 1024) == 1023
    assert M(10 ** 9) == capi.LOO_MAX_TAIL == lc.MAX_TAIL
    out = C.c_int32(-7)
    for n, tail in ((-1, 0), (100, -1), (100, capi.LOO_MAX_TAIL + 1)):
        assert lib.mhx_loo_tail_length(n, tail, C.byref(out)) == capi.EINVAL and out.value == -7
    assert lib.mhx_loo_tail_length(100, 0, None) == capi.OK               # (a NULL output is allowed)


def test_constants_and_signatures(mirror):
    capi = mirror.capi
    assert (capi.LOO_NONFINITE, capi.LOO_SHORT, capi.LOO_FLAT, capi.LOO_EMPTY) == \
        (lc.NONFINITE, lc.SHORT, lc.FLAT, lc.EMPTY) == (1, 2, 4, 8)
    assert capi.LOO_BLOCK == lc.BLOCK == wc.BLOCK and capi.LOO_MAX_TAIL == 1024
    for name in ("mhx_get_loo", "mhx_group_get_loo", "mhx_loo_tail_length"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    assert len(capi.SIGNATURES["mhx_get_loo"][1]) == len(capi.SIGNATURES["mhx_group_get_loo"][1]) == 16
    assert mirror.loo_compare is mirror.waic_compare
    for name in ("walker_set_loo", "walker_loo", "loo_compare", "loo_tail_length"):
        assert name in mirror.__all__ and callable(getattr(mirror, name))
    assert callable(mirror.Engine.loo) and callable(mirror.Group.loo)


# ---- the fit against exact generalised-Pareto samples ---------------------------------------------------
def test_the_fit_recovers_the_shape_of_generalised_pareto_samples():
    """200 exceedances from scipy.stats.genpareto(k), 200 draws each, seed 2017: the mean k_raw is
    within 0.05 of k.  Measured with this yardstick: -0.2967, 0.1228, 0.5081, 0.9007 for k = -0.3, 0.1,
    0.5, 0.9."""
    from scipy.stats import genpareto
    rng = np.random.default_rng(2017)
    for k in (-0.3, 0.1, 0.5, 0.9):
        got = []
        for _ in range(200):
            kraw, sigma, khat, fitted = lc.fit_np(np.sort(genpareto.rvs(k, size=200, random_state=rng)))
            assert fitted and khat == (200.0 * kraw + 5.0) / 210.0 and sigma > 0.0
            got.append(kraw)
        print("genpareto k = %+.1f: mean k_raw %.4f" % (k, np.mean(got)))
        assert abs(np.mean(got) - k) <= 0.05, (k, np.mean(got))


# ---- a closed form ----------------------------------------------------------------------------------------
def line_posterior(seed):
    """a 20-point line with known sigma and a flat prior: the data, the posterior's mean and covariance
    and the analytic leave-one-out predictive log densities"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 2.0, 20)
    sig = 0.3
    y = 0.5 + 1.5 * x + sig * rng.standard_normal(x.size)
    X = np.column_stack([np.ones_like(x), x])
    cov = sig * sig * np.linalg.inv(X.T @ X)
    mean = np.linalg.solve(X.T @ X, X.T @ y)
    exact = np.empty(x.size)
    for i in range(x.size):
        keep = np.arange(x.size) != i
        Xi, yi = X[keep], y[keep]
        G = np.linalg.inv(Xi.T @ Xi)
        mu = X[i] @ (G @ (Xi.T @ yi))
        var = sig * sig * (1.0 + X[i] @ G @ X[i])
        exact[i] = -0.5 * math.log(2.0 * math.pi * var) - 0.5 * (y[i] - mu) ** 2 / var
    return rng, x, y, sig, X, mean, cov, exact


def test_the_yardstick_against_the_analytic_leave_one_out_density():
    """max |elpd_i - exact_i| <= 0.05 with 4000 independent draws of the exact posterior and <= 0.15
    with 1000 draws each repeated four times (a chain's runs of rejected proposals).  Measured with
    this yardstick, seed 7: 0.0162 and 0.0376."""
    rng, x, y, sig, X, mean, cov, exact = line_posterior(7)
    draws = rng.multivariate_normal(mean, cov, size=4000)
    for name, th, bound in (("4000 independent", draws, 0.05),
                            ("1000 repeated four times", np.repeat(draws[:1000], 4, axis=0), 0.15)):
        ell = wc.terms(wc.NORMAL, th @ X.T, y, np.full(x.size, sig))
        r = lc.yardstick(ell)
        err = np.abs(r["pw_elpd"] - exact).max()
        print("closed form, %s draws: max |elpd_i - exact_i| = %.4f, max khat %.3f" % (name, err, r["pw_khat"].max()))
        assert r["status"] == 0 and r["fitted"].all() and r["M"] == lc.tail_length(len(th))
        assert err <= bound, (name, err)


# ---- the yardstick against mpmath -------------------------------------------------------------------------
def crafted_terms(rng, n, N):
    """the terms of a Metropolis-like window of a line model (test_gpu_waic.crafted's recipe)"""
    from test_gpu_waic import crafted
    x = np.linspace(-4.0, 10.0, N)
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    _, th = crafted(rng, n, [-1.0, 2.0], 0.05)
    return wc.terms(wc.NORMAL, th[:, :1] + th[:, 1:] * x[None, :], y, sig)


def deviations(ell, tail_len=0):
    """the greatest distance of the yardstick from mpmath at 200 bits fed the same (tail, l_cut, S_b):
    (|khat|, |sigma| relative, |elpd|)"""
    mpmath.mp.prec = 200
    n = ell.shape[0]
    r = lc.yardstick(ell, tail_len)
    dk = ds = de = 0.0
    for i in range(ell.shape[1]):
        khat, sigma, elpd, fitted = lc.estimate_mp(n, r["tail"][i], r["acc"][i, 1], r["acc"][i, 2])
        assert fitted == bool(r["fitted"][i]), i
        if fitted:
            dk = max(dk, abs(float(mpmath.mpf(float(r["pw_khat"][i])) - khat)))
            ds = max(ds, abs(float((mpmath.mpf(float(r["acc"][i, 3])) - sigma) / sigma)))
        de = max(de, abs(float(mpmath.mpf(float(r["pw_elpd"][i])) - elpd)))
    return dk, ds, de


def test_the_yardstick_against_mpmath_on_crafted_windows():
    """The fit, the smoothing and the estimate in binary64 against the same formulas at 200 bits on
    the same (tail, l_cut, S_b): crafted Metropolis-like windows of n = 25, 64, 300, 1024 steps (M = 5,
    12, 52, 96), 48 points each.  The largest deviations are what loo_cases.DEV_KHAT, DEV_SIGMA and
    DEV_ELPD record, and the device's tolerance is taken from those (tests/test_gpu_loo.py).
    Measured: khat 3.5e-15, 6.2e-15, 2.8e-14, 6.2e-14 for the four windows, sigma (relative) 1.6e-14,
    1.1e-14, 3.7e-14, 7.1e-14, pw_elpd 4.4e-15, 1.2e-14, 2.5e-14, 4.4e-14; the largest 6.153e-14,
    7.085e-14 and 4.378e-14 (over six points a window they were a tenth of that: the deviation is the
    cancellation in x_k = r_k - r_cut, and it takes a sample to meet a column where it bites)."""
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0, 0.0]
    for n in (25, 64, 300, 1024):
        d = deviations(crafted_terms(rng, n, 48))
        print("n = %4d: khat %.3e, sigma (relative) %.3e, elpd %.3e" % ((n,) + d))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print("largest: khat %.3e, sigma (relative) %.3e, elpd %.3e" % tuple(worst))
    assert worst[0] <= lc.DEV_KHAT and worst[1] <= lc.DEV_SIGMA and worst[2] <= lc.DEV_ELPD


# ---- hand cases ---------------------------------------------------------------------------------------------
def test_a_window_of_24_steps_has_no_tail():
    """n = 24: M = 0, SHORT; elpd = T_1 + log(n / sum exp(T_1 - l_s)), the raw importance-sampling
    estimate, by hand"""
    rng = np.random.default_rng(3)
    ell = -3.0 + rng.standard_normal((24, 4))
    r = lc.yardstick(ell)
    assert r["M"] == 0 and r["status"] == lc.SHORT and not r["fitted"].any()
    assert np.isinf(r["pw_khat"]).all() and r["n_high"] == 4 and r["tail"].shape == (4, 0)
    for i in range(4):
        T1 = ell[:, i].min()
        assert r["acc"][i, 0] == T1 and r["acc"][i, 1] == T1 and r["acc"][i, 3] == 0.0
        S = math.fsum(math.exp(T1 - v) for v in ell[:, i])
        assert abs(r["acc"][i, 2] - S) <= 24 * 4 * U * S
        want = -math.log(math.fsum(math.exp(-v) for v in ell[:, i]) / 24.0)      # the harmonic mean
        assert abs(r["pw_elpd"][i] - want) <= 1e-13
    assert lc.yardstick(ell, k_limit=np.inf)["n_high"] == 0


def test_a_window_of_identical_steps_is_flat():
    """a chain that never moved: every ratio is 1, x = 0, FLAT; khat = +inf and elpd is the term itself"""
    for n in (25, 300):
        ell = np.tile(np.array([[-1.25, -700.0, 0.0, 3.5]]), (n, 1))
        r = lc.yardstick(ell)
        assert r["M"] == lc.tail_length(n) > 0 and r["status"] == lc.FLAT and not r["fitted"].any()
        assert np.isinf(r["pw_khat"]).all() and r["n_high"] == 4
        assert lc.same_bits(r["pw_elpd"], ell[0])
        assert lc.same_bits(r["acc"], np.column_stack([ell[0], ell[0], np.full(4, float(n - r["M"])), np.zeros(4)]))
        assert lc.same_bits(r["tail"], np.tile(ell[0][:, None], (1, r["M"])))


def test_ties_straddling_the_cut_go_to_the_newer_steps():
    """n = 30, M = 6: four distinct small terms, then a run of five equal terms of which two are tail -
    the two newest (smallest s) - and three are body"""
    n = 30
    col = np.linspace(-1.0, -2.0, n)                 # (all above the planted ones)
    small = {3: -9.0, 17: -8.0, 11: -7.5, 29: -7.0}
    run = [2, 8, 9, 20, 25]
    for s, v in small.items():
        col[s] = v
    col[run] = -5.0
    s = lc.split(col[:, None])
    assert s["M"] == 6 and list(s["tail"][0]) == [-9.0, -8.0, -7.5, -7.0, -5.0, -5.0]
    assert s["T1"][0] == -9.0 and s["l_cut"][0] == -5.0
    body = [k for k in range(n) if k not in small and k not in run[:2]]      # steps 9, 20, 25 are body
    want = np.float64(0.0)
    for k in body:
        want = want + lc.gexp(np.float64(-9.0) - col[k])[()]
    assert lc.same_bits(s["S_b"][0], want)
    # -0.0 sorts before +0.0, and a NaN last
    z = lc.split(np.array([0.0, -0.0, np.nan, 1.0, -0.0] + [2.0] * 25)[:, None], tail_len=5)
    assert lc.same_bits(z["tail"][0], [-0.0, -0.0, 0.0, 1.0, 2.0])


# ---- carve_loo on the CPU ----------------------------------------------------------------------------------
# "take P want m" answers "maxtake|P chunk|bytes off...|bytes off...": loo_max_take, the cursor's portion
# and chunk, the carving of 1 and of P chains at a chunk of points
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17 && kLooBlock == 256, "the budget");
  long long take, P, want, m;
  while (scanf("%lld %lld %lld %lld", &take, &P, &want, &m) == 4) {
    const long long nb = (m + 255) / 256;
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n, int64_t mm) {
      const LooPieces s = carve_loo(c, nb, (int)take, (int)P, (int)want, n, mm);
      off = {s.status, s.n_used, s.n_high, s.elpd, s.p_loo, s.lppd, s.part_elpd, s.part_lppd, s.part_high,
             s.cst, s.terms, s.pw_elpd, s.pw_khat, s.pw_lppd, s.pw_acc, s.tail};
    };
    const PortionCursor at = loo_cursor(1000, m, (int)take, (int)P, (int)want);
    printf("%d|%lld %lld", loo_max_take(m, (int)P, (int)want), (long long)at.per_portion, (long long)at.chunk);
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


def test_carve_loo_alignment_budget_and_a_chunk_of_points():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_loo_stage_")
    try:
        src, exe = os.path.join(d, "loo_driver.cpp"), os.path.join(d, "loo_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                               "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        cases = [(take, m, want) for take in (1, 64, 1000, 8192, 65536) for m in (1, 256, 257, 1000, 9000, CHUNK + 300)
                 for want in (0, 1, 3)]
        queries = ["%d %d %d %d" % (take, lc.tail_length(take), want, m) for take, m, want in cases]
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")[:-1]
        assert len(out) == len(cases)
        for (take, m, want), line in zip(cases, out):
            P, nb = lc.tail_length(take), (m + 255) // 256
            max_take, head, *carvings = line.split("|")
            per_portion, chunk = (int(w) for w in head.split())

            def need(mc):       # (fixed bytes, bytes per chain) of every piece at a chunk of mc points
                return [(0, 4), (0, 4), (0, 4), (0, 8), (0, 8), (0, 8), (0, 8 * nb), (0, 8 * nb), (0, 4 * nb),
                        (8 * mc, 0), (0, 8 * mc * take), (0, 8 * mc), (0, 8 * mc), (0, 8 * mc),
                        (0, 32 * mc if want & 1 else 0), (0, 8 * P * mc if want & 2 else 0)]

            def fits(mc):       # one chain, by one_item_fits' accounting
                nd = need(mc)
                return sum(f + v for f, v in nd) + 256 * len(nd) <= B
            # the chunk: every point where one chain fits with them, else the most whole blocks that fit
            if m <= CHUNK and fits(m):
                assert chunk == m, (take, m, want, line)
            else:
                assert chunk % 256 == 0 and chunk < m and chunk <= CHUNK, (take, m, want, line)
                assert (chunk == 0 or fits(chunk)) and (chunk + 256 > min(m, CHUNK) or not fits(chunk + 256))
            # the greatest take whose smallest chunk fits: the refusal names it
            m1 = min(m, 256)
            assert (chunk > 0) == (take <= int(max_take)), (take, m, want, line)
            nd = need(m1)
            rest = sum(f + v for i, (f, v) in enumerate(nd) if i != 10) + 256 * len(nd)
            assert int(max_take) == (B - rest) // (8 * m1), (take, m, want, line)
            if chunk == 0:
                continue
            nd = need(chunk)
            fixed, per = sum(f for f, _ in nd), sum(v for _, v in nd)
            assert per_portion == max(1, (B - (fixed + len(nd) * 256)) // per), (take, m, want, line)
            for n, carving in zip((1, per_portion), carvings):
                total, *off = (int(w) for w in carving.split())
                size = [f + n * v for f, v in nd]
                assert len(off) == len(nd) and off[0] == 0 and all(o % 256 == 0 for o in off)
                for k in range(len(off)):
                    assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (take, m, want, n, k)
                assert total <= B, (take, m, want, n, total)
            # what depends on the chains alone keeps its place whatever the chunk of points is
            first = [int(w) for w in carvings[0].split()][1:10]
            assert first == [256 * k for k in range(6)] + [1536, 1536 + 256 * ((8 * nb + 255) // 256),
                                                           1536 + 512 * ((8 * nb + 255) // 256)]
        assert CHUNK % lc.BLOCK == 0        # a chunk of points is whole blocks of the sums
    finally:
        shutil.rmtree(d, ignore_errors=True)
