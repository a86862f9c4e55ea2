"""The numpy yardstick of mhx_get_normal_equations (tests/normeq_cases.py) against closed forms and
analytic derivatives, and the host layer on top of the device call - least_squares, laplace_summary,
walker_set_laplace - driven by numpy.  No GPU.

Bounds and where they come from:
  line model, F and b against X^T W X          1e-8 relative.  The model is linear in theta, so a
      central difference has no truncation error: what is left is the rounding of vp - vm,
      <= 4 * 2^-53 * max|v| / dh per derivative, about 7e-10 here.
  two_peak(334), g against analytic            1e-7 * max|g|.  Measured: 1.1e-9 (2.9e-9 on F); the
      bound is 100 times that - it checks that the definition IS a derivative, not its accuracy.
  least_squares, Newton decrement              <= 1e-8 after 25 iterations from 5 % starts
      (measured <= 1.3e-14, at most 11 iterations to 1e-10); the objective never falls."""
import numpy as np
import pytest

import normeq_cases as nc
import problems as pb


def line_values(x):
    return lambda th: th[0] + th[1] * x


# ---- hand cases ---------------------------------------------------------------------------------
def test_one_point():
    x, y, sig = np.array([2.0]), np.array([3.5]), np.array([0.5])
    r = nc.yardstick(line_values(x), nc.NORMAL, [1.0, 1.0], [0.5, 0.25], [0, 1], y, sig)
    # v = 3, u = (3.5 - 3) / 0.5 = 1; dv/db = 1, dv/dm = 2, both exact with these steps; w = 2
    assert r["status"] == 0 and r["chi2"] == 1.0
    assert r["g"].tolist() == [[2.0], [4.0]] and r["u"].tolist() == [1.0]
    assert r["jtj"].tolist() == [[4.0, 8.0], [8.0, 16.0]] and r["jtr"].tolist() == [2.0, 4.0]


def test_a_zero_step_and_an_unread_place_are_exact_zeros():
    x = np.array([1.0, 2.0, 4.0])
    y, sig = np.array([0.0, 1.0, 2.0]), np.ones(3)
    # d = 3, the function reads places 0 and 2; the step of place 0 is 0
    vals = lambda th: th[0] + th[2] * x
    r = nc.yardstick(vals, nc.NORMAL, [0.5, 9.0, 0.5], [0.0, 0.5, 0.25], [0, 2], y, sig)
    assert r["status"] == 0
    for t in (0, 1):
        assert not r["g"][t].any() and not np.signbit(r["g"][t]).any()
        assert r["jtr"][t] == 0.0 and not r["jtj"][t].any() and not r["jtj"][:, t].any()
    assert r["jtj"][2, 2] == 1.0 + 4.0 + 16.0
    assert r["jtr"][2] == float(np.cumsum(x * (y - (0.5 + 0.5 * x)))[-1])


def test_a_point_that_is_not_a_number_and_a_step_below_the_spacing():
    x = np.array([1.0, np.nan, 3.0])
    r = nc.yardstick(line_values(x), nc.NORMAL, [0.0, 1.0], [0.5, 0.5], [0, 1], np.zeros(3), None)
    assert r["status"] == nc.NONFINITE and np.isnan(r["chi2"])
    x = np.array([1.0, 2.0])
    r = nc.yardstick(line_values(x), nc.NORMAL, [1.0, 1.0], [1e-20, 0.5], [0, 1], np.zeros(2), None)
    assert r["status"] == nc.NONFINITE and np.isnan(r["g"][0]).all()      # dh == 0: 0 / 0
    r = nc.yardstick(line_values(x), nc.POISSON, [-5.0, 1.0], [0.5, 0.5], [0, 1], np.ones(2), None)
    assert r["status"] == nc.NONFINITE                                    # sqrt of a negative rate


def test_blocks_are_summed_in_order():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((2, 2 * nc.BLOCK + 3))
    S = nc.block_sums(rows)
    want = 0.0
    for b0 in range(0, rows.shape[1], nc.BLOCK):
        part = 0.0
        for v in rows[0, b0:b0 + nc.BLOCK] * rows[1, b0:b0 + nc.BLOCK]:
            part = part + v
        want = want + part
    assert S[0, 1] == S[1, 0] == want
    assert nc.block_sums(np.array([[-0.0, 0.0], [1.0, 1.0]]))[0, 1] == 0.0
    assert not np.signbit(nc.block_sums(np.array([[-0.0], [1.0]]))[0, 1])  # from +0.0, not from the first term


# ---- the line against X^T W X ---------------------------------------------------------------------
def test_line_against_the_closed_form():
    import lisp_mcmc_amd as mhx
    rng = np.random.default_rng(1)
    N = 1500
    x = np.linspace(-4.0, 10.0, N)
    sig = rng.uniform(0.2, 0.5, N)
    y = -1.0 + 2.0 * x + sig * rng.standard_normal(N)
    th = np.array([-1.0, 2.0])
    r = nc.yardstick(line_values(x), nc.NORMAL, th, mhx.normeq_steps(th), [0, 1], y, sig)
    X = np.column_stack([np.ones(N), x])
    W = 1.0 / (sig * sig)
    F = X.T @ (X * W[:, None])
    b = X.T @ (W * (y - X @ th))
    assert r["status"] == 0
    assert np.abs(r["jtj"] - F).max() <= 1e-8 * np.abs(F).max()
    assert np.abs(r["jtr"] - b).max() <= 1e-8 * np.abs(F).max() * np.abs(th).max()
    assert abs(r["chi2"] - float((W * (y - X @ th) ** 2).sum())) <= 1e-12 * r["chi2"]


# ---- two peaks against analytic derivatives ----------------------------------------------------------
def two_peak_jacobian(th, x):
    """d model / d theta [8, N] of problems.two_peak's model: b0 + b1 x + sum A exp(-((x - mu) / w)^2)"""
    J = [np.ones_like(x), x]
    for k in range(2):
        A, mu, w = th[2 + 3 * k: 5 + 3 * k]
        t = (x - mu) / w
        e = np.exp(-t * t)
        J += [e, A * e * 2.0 * t / w, A * e * 2.0 * t * t / w]
    return np.array(J)


def two_peak_values(x):
    return lambda th: pb.model_eval_np(pb.GAUSS, (2, 2), th, x)


def analytic(s, th):
    """(F, b, decrement) of two_peak problem s at th from the analytic Jacobian"""
    x, y, sig, _ = s.data[0]
    g = two_peak_jacobian(th, x) / sig
    u = (y - pb.model_eval_np(pb.GAUSS, (2, 2), th, x)) / sig
    F, b = g @ g.T, g @ u
    return F, b, float(b @ np.linalg.solve(F, b))


def test_two_peak_is_a_derivative():
    import lisp_mcmc_amd as mhx
    s = pb.two_peak(n=334)
    x, y, sig, _ = s.data[0]
    th = pb.perturbed(s.theta_star, 1, 0.02, seed=4)[0]
    r = nc.yardstick(two_peak_values(x), nc.NORMAL, th, mhx.normeq_steps(th), range(8), y, sig)
    g = two_peak_jacobian(th, x) / sig
    F, b, _ = analytic(s, th)
    err_g, err_F = np.abs(r["g"] - g).max() / np.abs(g).max(), np.abs(r["jtj"] - F).max() / np.abs(F).max()
    print("two_peak(334): g differs by %.2g of max|g|, F by %.2g of max|F|" % (err_g, err_F))
    assert r["status"] == 0
    assert err_g <= 1e-7 and err_F <= 1e-7
    assert np.abs(r["jtr"] - b).max() <= 1e-7 * np.abs(g).max() * np.abs(r["u"]).sum()


# ---- least_squares over numpy ------------------------------------------------------------------------
def numpy_equations(s):
    import lisp_mcmc_amd as mhx
    x, y, sig, _ = s.data[0]

    def equations(theta):
        rs = [nc.yardstick(two_peak_values(x), nc.NORMAL, th, mhx.normeq_steps(th), range(8), y, sig)
              for th in theta]
        return np.array([r["jtj"] for r in rs]), np.array([r["jtr"] for r in rs])

    def objective(theta):
        lo, hi = np.minimum(s.theta_star * 0.5, s.theta_star * 1.5), np.maximum(s.theta_star * 0.5, s.theta_star * 1.5)
        out = []
        for th in theta:
            u = (y - pb.model_eval_np(pb.GAUSS, (2, 2), th, x)) / sig
            out.append(-0.5 * float(u @ u) if ((th >= lo) & (th <= hi)).all() else -np.inf)
        return np.array(out)
    return equations, objective


@pytest.mark.parametrize("n", [334, 1500])
def test_least_squares_reaches_the_least_squares_point(n):
    import lisp_mcmc_amd as mhx
    s = pb.two_peak(n=n)
    equations, objective = numpy_equations(s)
    start = pb.perturbed(s.theta_star, 11, 0.05, seed=3)
    r = mhx.least_squares(equations, objective, start, iterations=25, damping=1e-3)
    dec = [analytic(s, th)[2] for th in r["theta"]]
    print("two_peak(%d): greatest Newton decrement %.3g, iterations %s" % (n, max(dec), r["iterations"].tolist()))
    assert max(dec) <= 1e-8
    assert r["history"].shape == (26, 11) and (np.diff(r["history"], axis=0) >= 0.0).all()
    assert np.array_equal(r["history"][-1], r["objective"]) and np.array_equal(objective(r["theta"]), r["objective"])
    assert (r["objective"] > objective(start)).all() and (r["iterations"] >= 1).all()


def test_least_squares_leaves_a_fixed_place_and_a_walker_at_its_optimum_alone():
    F0 = np.array([[2.0, 0.0, 0.5], [0.0, 0.0, 0.0], [0.5, 0.0, 1.0]])
    opt = np.array([1.0, 7.0, -2.0])

    def equations(theta):       # a quadratic: b = F (opt - theta) over the live places
        return np.array([F0] * len(theta)), np.array([F0 @ (opt - th) for th in theta])

    def objective(theta):
        return np.array([-0.5 * (opt - th) @ F0 @ (opt - th) for th in theta])
    start = np.array([[0.0, 3.0, 0.0], [1.0, 3.0, -2.0]])
    r = mhx_least_squares()(equations, objective, start, iterations=12)
    assert r["theta"][:, 1].tolist() == [3.0, 3.0]                       # the zero row never moves
    assert np.allclose(r["theta"][0, [0, 2]], opt[[0, 2]], atol=1e-9)
    assert np.array_equal(r["theta"][1], start[1]) and r["iterations"].tolist()[1] == 0


def mhx_least_squares():
    import lisp_mcmc_amd as mhx
    return mhx.least_squares


# ---- laplace_summary and walker_set_laplace on a planted F ----------------------------------------
class PlantedEngine:
    """what walker_set_laplace asks of an engine, answered from planted numbers"""

    def __init__(self, theta, F, b, chi2, status):
        self.theta, self.F, self.b, self.chi2, self.status = theta, F, b, chi2, status
        self.n_chains, self.d, self.K = theta.shape[0], theta.shape[1], len(F)
        self.asked = []

    def state(self):
        return {"best_theta": self.theta}

    def normal_equations(self, fn, theta=None, steps=None, pointwise=False):
        self.asked.append((fn, np.array(theta), np.array(steps)))
        return {"jtj": self.F[fn].copy(), "jtr": self.b[fn].copy(), "chi2": self.chi2[fn].copy(),
                "status": self.status[fn].copy()}


def test_walker_set_laplace_on_a_planted_matrix():
    import lisp_mcmc_amd as mhx
    from importlib import import_module
    walker = import_module("lisp-mcmc_amd.walker")
    theta = np.array([[1.0, 2.0, 0.0], [1.5, 2.5, 3.0]])
    A = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 0.0]])   # function 0 reads places 0, 1
    B = np.array([[1.0, 0.0, 0.5], [0.0, 0.0, 0.0], [0.5, 0.0, 2.0]])   # function 1 reads places 0, 2
    F = [np.array([A, 2.0 * A]), np.array([B, B])]
    b = [np.array([[1.0, -1.0, 0.0], [0.0, 0.0, 0.0]]), np.array([[0.5, 0.0, 0.25], [0.0, 0.0, 0.0]])]
    chi2 = [np.array([10.0, 20.0]), np.array([5.0, 6.0])]
    status = [np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)]
    e = PlantedEngine(theta, F, b, chi2, status)
    data = [[np.zeros(40), np.zeros(40)], [np.zeros(30), np.zeros(30)]]
    w = walker.Walker(e, None, ["a", "b", "c"], data, [None, None], None, None)
    out = mhx.walker_set_laplace(w)
    assert [k for k, _, _ in e.asked] == [0, 1]
    assert np.array_equal(e.asked[0][2], mhx.normeq_steps(theta)) and e.asked[0][2][0, 2] == np.cbrt(2.0 ** -52)
    Fs, bs = A + B, b[0][0] + b[1][0]
    cov = np.linalg.inv(Fs)
    s = out[0]
    assert s["params"] == {"a": 1.0, "b": 2.0, "c": 0.0} and s["varied-keys"] == ["a", "b", "c"]
    assert (s["chi2"], s["dof"], s["status"]) == (15.0, 70 - 3, 0) and s["reduced-chi2"] == 15.0 / 67.0
    assert np.array_equal(s["gradient"], bs)
    assert np.allclose(s["covariance-matrix"], cov, rtol=1e-13, atol=0)
    assert np.allclose(s["stddev-params"], np.sqrt(np.diag(cov)), rtol=1e-13)
    assert np.allclose(np.diag(s["correlation"]), 1.0, rtol=1e-14)
    assert np.allclose(s["correlation"][0, 1], cov[0, 1] / np.sqrt(cov[0, 0] * cov[1, 1]), rtol=1e-13)
    assert abs(s["newton-decrement"] - bs @ cov @ bs) <= 1e-13 * s["newton-decrement"]
    L = s["l-matrix"]
    assert np.allclose(L @ L.T, cov * 2.38 ** 2 / 3.0, rtol=1e-13) and np.array_equal(L, np.tril(L))
    assert out[1]["newton-decrement"] == 0.0 and out[1]["chi2"] == 26.0
    assert mhx.walker_laplace(w, chain=1)["params"] == out[1]["params"]
    # a fixed key: its step is 0, its row and column of the l-matrix are zero, p is one less
    e.asked.clear()
    hold = mhx.walker_set_laplace(w, fixed=[":b"], steps={"a": 0.125})[0]
    assert (e.asked[0][2][:, 1] == 0.0).all() and (e.asked[0][2][:, 0] == 0.125).all()
    keep = [0, 2]
    cov2 = np.linalg.inv(Fs[np.ix_(keep, keep)])
    assert hold["varied-keys"] == ["a", "c"] and hold["dof"] == 70 - 2
    assert np.allclose(hold["covariance-matrix"], cov2, rtol=1e-13)
    L = hold["l-matrix"]
    assert not L[1].any() and not L[:, 1].any() and hold["stddev-params"][1] == 0.0
    assert np.allclose((L @ L.T)[np.ix_(keep, keep)], cov2 * 2.38 ** 2 / 2.0, rtol=1e-13)
    # what is not positive definite, and what is not finite, is said and not inverted
    status[0][1] = 1
    F[1][0][2, 2] = -2.0
    bad = mhx.walker_set_laplace(w)
    assert bad[0]["status"] == walker.LAPLACE_NOT_POSITIVE and bad[0]["l-matrix"] is None
    assert bad[1]["status"] == walker.LAPLACE_NONFINITE and bad[1]["covariance-matrix"] is None
    assert bad[0]["chi2"] == 15.0 and np.array_equal(bad[0]["gradient"], bs)


def test_normeq_steps():
    import lisp_mcmc_amd as mhx
    h = mhx.normeq_steps([[0.0, -2.0], [4.0, 1e-300]])
    c = np.cbrt(2.0 ** -52)
    assert h.tolist() == [[c, c * 2.0], [c * 4.0, c * 1e-300]]


# ---- carve_normeq on the CPU ------------------------------------------------------------------------
# "nb_total n_tasks d per_chain with_theta want_g m" answers "P chunk|bytes off...|bytes off...": the
# cursor's portion and chunk, the carving of 1 and of P chains at a chunk of points
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17, "the budget and the chunk");
  long long nb, nt, d, pc, wt, wg, m;
  while (scanf("%lld %lld %lld %lld %lld %lld %lld", &nb, &nt, &d, &pc, &wt, &wg, &m) == 7) {
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n, int64_t mm) {
      const NormEqPieces s = carve_normeq(c, nb, (int)nt, (int)d, (int)pc, (int)wt, (int)wg, n, mm);
      off = {s.steps, s.status, s.chi2, s.jtr, s.jtj, s.chain_steps, s.theta, s.part, s.g};
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


def test_carve_normeq_alignment_budget_and_a_chunk_of_points():
    import os
    import shutil
    import subprocess
    import tempfile
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lisp-mcmc_amd", "csrc")
    chunk, budget = 1 << 17, 1 << 26
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    tmp = tempfile.mkdtemp(prefix="mhx_normeq_stage_")
    try:
        src, exe = os.path.join(tmp, "normeq_driver.cpp"), os.path.join(tmp, "normeq_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", csrc, "-o", exe, src])
        cases = [(m, wg, d, p, pc, wt) for m in (1, 1023, 1024, 1025, 334, chunk, chunk + 1029, 100000)
                 for wg in (0, 1) for d, p in ((2, 2), (8, 8), (63, 32)) for pc, wt in ((0, 0), (1, 1))]
        queries = ["%d %d %d %d %d %d %d" % ((m + nc.BLOCK - 1) // nc.BLOCK, (p + 1) * (p + 2) // 2, d, pc, wt, wg, m)
                   for m, wg, d, p, pc, wt in cases]
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")[:-1]
        assert len(out) == len(cases)
        places = {}
        for (m, wg, d, p, pc, wt), line in zip(cases, out):
            nb, nt, mc = (m + nc.BLOCK - 1) // nc.BLOCK, (p + 1) * (p + 2) // 2, min(m, chunk)
            head, *carvings = line.split("|")
            fixed = 0 if pc else 8 * d                          # the shared steps do not grow with the chains
            per = [0, 4, 8, 8 * d, 8 * d * d, 8 * d * pc, 8 * d * wt, 8 * nb * nt, 8 * d * mc * wg]
            want_p = max(1, (budget - fixed - len(per) * 256) // sum(per))
            assert [int(w) for w in head.split()] == [want_p, mc], (m, wg, d, line)
            assert mc == m or mc % nc.BLOCK == 0                 # a chunk of points is whole blocks
            for n, carving in zip((1, want_p), carvings):
                total, *off = (int(w) for w in carving.split())
                assert "PIECES" not in carving
                assert len(off) == len(per) and off[0] == 0 and all(o % 256 == 0 for o in off)
                size = [fixed] + [n * b for b in per[1:]]
                for k in range(len(off)):                        # the pieces do not overlap
                    assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (m, wg, n, k)
                # under 64 MiB, unless one chain alone is more (g of a wide problem at a whole chunk)
                assert total <= budget or n == 1, (m, wg, d, n, total)
            # what depends on the chains alone keeps its place whatever the chunk of points is
            one = [int(w) for w in carvings[0].split()][1:8]
            assert places.setdefault((d, pc, wt), one) == one
        assert chunk % nc.BLOCK == 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
