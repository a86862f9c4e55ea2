"""CPU checks around mhx_get_residuals: the numpy yardstick (tests/resid_cases.py) against hand
cases of include/mhx.h's definition and against math.fsum, the host-side runs_z, and carve_resid
(csrc/mhx_stage.hpp) compiled on the CPU.  No device is touched."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import resid_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
U = 2.0 ** -53
B = 1 << 26
CHUNK = 1 << 17


@pytest.fixture(scope="module")
def mirror():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def test_the_librarys_constants_and_prototypes(mirror):
    capi = mirror.capi
    assert (capi.RESID_NONFINITE, capi.RESID_BLOCK) == (rc.NONFINITE, rc.BLOCK)
    assert (capi.LIK_NORMAL, capi.LIK_NORMAL_CUTOFF, capi.LIK_POISSON, capi.LIK_EXPR) == \
        (rc.NORMAL, rc.CUTOFF, rc.POISSON, rc.EXPR)
    a = capi.SIGNATURES["mhx_get_residuals"]
    assert a == capi.SIGNATURES["mhx_group_get_residuals"] and len(a[1]) == 15
    with open(os.path.join(ROOT, "include", "mhx.h")) as f:
        header = f.read()
    assert "#define MHX_RESID_BLOCK %d " % rc.BLOCK in header and "MHX_RESID_NONFINITE = 1" in header


def test_hand_cases_of_the_definition():
    one = rc.reduce([0.5])
    assert one["dw"] == 0.0 and one["n_runs"] == 1 and one["chi2"] == 0.25 and one["sum_z"] == 0.5
    assert (one["n_pos"], one["n_out"], one["max_abs_z"], one["max_index"]) == (1, 0, 0.5, 0)
    alt = rc.reduce([1.0, -1.0, 1.0])
    assert alt["n_runs"] == 3 and alt["dw"] == 8.0 and alt["chi2"] == 3.0 and alt["sum_z"] == 1.0
    assert alt["n_pos"] == 2 and alt["max_index"] == 0          # ties keep the earliest point
    # a zero and a -0 are "not positive": one run with the negative neighbour, no count
    zeros = rc.reduce([-1.0, 0.0, -0.0, -2.0, 3.0], z_limit=3.0)
    assert zeros["n_pos"] == 1 and zeros["n_runs"] == 2
    assert zeros["n_out"] == 0                                   # |z| = z_limit exactly is not counted
    assert (zeros["max_abs_z"], zeros["max_index"]) == (3.0, 4)
    assert rc.reduce([-1.0, 0.0, -0.0, -2.0, 3.0], z_limit=2.5)["n_out"] == 1
    # NaN: never positive, never counted, passed over by the extreme
    nan = float("nan")
    none = rc.reduce([nan, nan, nan])
    assert (none["max_abs_z"], none["max_index"]) == (-1.0, -1)
    assert (none["n_pos"], none["n_runs"], none["n_out"]) == (0, 1, 0)
    some = rc.reduce([nan, -4.0, nan, 4.0, 1.0])
    assert (some["max_abs_z"], some["max_index"]) == (4.0, 1) and some["n_out"] == 2
    assert some["n_pos"] == 2 and some["n_runs"] == 2
    # a z of exactly 0 as the only point: the extreme is 0 at point 0, not the start value
    z0 = rc.reduce([0.0])
    assert (z0["max_abs_z"], z0["max_index"]) == (0.0, 0)


def test_the_standardized_residual_forms():
    v = np.array([2.0, 3.5, 9.0])
    y = np.array([1.0, 4.0, 9.0])
    s = np.array([0.5, 0.25, 3.0])
    z = rc.standardized(rc.NORMAL, v, y, s)
    w = 1.0 / s
    assert rc.same_bits(z, v * w - y * w) and list(z) == [2.0, -2.0, 0.0]
    assert rc.same_bits(rc.standardized(rc.CUTOFF, v, y, s), z)
    assert rc.same_bits(rc.standardized(rc.NORMAL, v, y), v - y)          # no sigma: w = 1
    p = rc.standardized(rc.POISSON, np.array([4.0, 9.0, 0.0, -1.0]), np.array([2.0, 12.0, 0.0, 1.0]))
    assert list(p[:2]) == [1.0, -1.0] and np.isnan(p[2]) and np.isnan(p[3])
    out = rc.yardstick(rc.POISSON, [4.0, 0.0], [2.0, 3.0])
    assert out["status"] == rc.NONFINITE and out["z"][1] == -np.inf
    assert (out["max_abs_z"], out["max_index"], out["n_pos"], out["n_runs"]) == (np.inf, 1, 1, 2)
    assert rc.yardstick(rc.NORMAL, [1.0, np.inf], [1.0, 1.0])["status"] == rc.NONFINITE
    assert rc.yardstick(rc.NORMAL, v, y, s)["status"] == 0


def test_the_block_sums_order_and_accuracy():
    """the lanes, the butterfly and the blocks in the stated order; within N 2^-53 sum |term| of
    math.fsum, the bound of any order of N - 1 additions"""
    # 64 lanes of one block, a term only in lanes 0 and 32: they meet in the butterfly's first stage
    t = np.zeros(64)
    t[0], t[32], t[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    # (1 + 2^-53 rounds to 1 in stage one; lane 1's 2^-53 meets lane 33's 0, then 1 again: lost too)
    assert rc.block_sum(t) == 1.0
    t2 = np.zeros(64)
    t2[1], t2[33], t2[0] = 2.0 ** -53, 2.0 ** -53, 1.0       # the two small ones meet first: kept
    assert rc.block_sum(t2) == 1.0 + 2.0 ** -52
    # a lane adds its rows serially before any lane meets another
    t3 = np.zeros(256)
    t3[0], t3[64], t3[128] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert rc.block_sum(t3) == 1.0
    # blocks are added serially from 0.0
    t4 = np.zeros(3 * 256)
    t4[0], t4[256], t4[512] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert rc.block_sum(t4) == 1.0
    rng = np.random.default_rng(1)
    for N in (1, 2, 63, 64, 65, 255, 256, 257, 515, 5000):
        for scale in (1.0, 1e6):
            t = scale * rng.standard_normal(N) ** 3
            got = rc.block_sum(t)
            assert abs(got - math.fsum(t)) <= N * U * math.fsum(np.abs(t)), (N, scale)
        z = rng.standard_normal(N)
        r = rc.reduce(z)
        assert abs(r["chi2"] - math.fsum(z * z)) <= N * U * math.fsum(z * z), N
        d = np.diff(z)
        assert abs(r["dw"] - math.fsum(d * d)) <= N * U * math.fsum(d * d), N


def test_runs_z_against_its_formula(mirror):
    f = mirror.runs_z
    for n_pos, n_neg, runs in ((5, 5, 6), (5, 5, 2), (10, 3, 7), (2, 1, 2), (200, 134, 12)):
        N = n_pos + n_neg
        mu = 2.0 * n_pos * n_neg / N + 1.0
        var = (mu - 1.0) * (mu - 2.0) / (N - 1.0)
        assert f(n_pos, n_neg, runs) == (runs - mu) / math.sqrt(var)
    assert f(5, 5, 6) == 0.0                      # mu = 6: as many runs as chance gives
    assert f(200, 134, 12) < -10.0                # long runs: structured residuals
    for undefined in ((0, 0, 1), (1, 0, 1), (7, 0, 1), (0, 9, 1), (1, 1, 2)):   # (the last: var = 0)
        assert math.isnan(f(*undefined)), undefined


# ---- carve_resid on the CPU -------------------------------------------------------------------------
# "nb_total d with_theta want m" answers "P chunk|bytes off...|bytes off...": the cursor's portion
# and chunk, the carving of 1 and of P chains at a chunk of points
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17, "the budget and the chunk");
  long long nb, d, with_theta, want, m;
  while (scanf("%lld %lld %lld %lld %lld", &nb, &d, &with_theta, &want, &m) == 5) {
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n, int64_t mm) {
      const ResidPieces s = carve_resid(c, nb, (int)d, (int)with_theta, (int)want, n, mm);
      off = {s.status, s.n_pos, s.n_runs, s.n_out, s.max_index, s.chi2, s.sum_z, s.dw, s.max_abs_z, s.theta,
             s.part_chi2, s.part_sumz, s.part_dw, s.part_max, s.part_idx, s.part_cnt, s.fit, s.z};
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


def test_carve_resid_alignment_budget_and_a_chunk_of_points():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    tmp = tempfile.mkdtemp(prefix="mhx_resid_stage_")
    try:
        src, exe = os.path.join(tmp, "resid_driver.cpp"), os.path.join(tmp, "resid_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
        cases = [(m, want, d, wt) for m in (1, 255, 256, 257, 334, CHUNK - 1, CHUNK, CHUNK + 5, 100000, 1 << 20)
                 for want in (0, 1, 2, 3) for d, wt in ((8, 1), (8, 0), (63, 1))]
        queries = ["%d %d %d %d %d" % ((m + 255) // 256, d, wt, want, m) for m, want, d, wt in cases]
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")[:-1]
        assert len(out) == len(cases)
        for (m, want, d, wt), line in zip(cases, out):
            nb, mc = (m + 255) // 256, min(m, CHUNK)
            head, *carvings = line.split("|")
            # bytes per chain of each piece: four ints, an index, four doubles, theta, the partials,
            # and per point of the chunk what is asked for
            per = [4, 4, 4, 4, 8, 8, 8, 8, 8, 8 * d * wt, 8 * nb, 8 * nb, 8 * nb, 8 * nb, 8 * nb, 12 * nb,
                   8 * mc if want & 1 else 0, 8 * mc if want & 2 else 0]
            want_p = max(1, (B - len(per) * 256) // sum(per))
            assert [int(w) for w in head.split()] == [want_p, mc], (m, want, line)
            assert mc == m or mc % rc.BLOCK == 0               # a chunk of points is whole blocks
            for n, carving in zip((1, want_p), carvings):
                total, *off = (int(w) for w in carving.split())
                assert "PIECES" not in carving
                assert len(off) == len(per) and off[0] == 0 and all(o % 256 == 0 for o in off)
                for k in range(len(off)):                      # the pieces do not overlap
                    assert off[k] + n * per[k] <= (off[k + 1] if k + 1 < len(off) else total), (m, want, n, k)
                assert total <= B, (m, want, n, total)         # the stage stays under 64 MiB
            # what depends on the chains alone keeps its place whatever the chunk of points is
            first = [int(w) for w in carvings[0].split()][1:10]
            assert first == [256 * k for k in range(9)]
        assert CHUNK % rc.BLOCK == 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
