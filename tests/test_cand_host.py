"""CPU checks of the candidate search (mhx_get_candidate_scores and its Python mirror): the order
and shape of candidate_grid, the ranking rule of tests/cand_cases.py on planted ties, infinities and
m < keep, the argument checks of the Python layer that need no device, the winner walker_set_search
takes from a planted engine's answers, and the stage arithmetic (carve_cand in csrc/mhx_stage.hpp)
against the header, as tests/test_histo_stage_plan.py drives the histograms': a portion stays within
the budget and one more chain would not fit."""
import itertools
import math
import os
import shutil
import subprocess
import tempfile
from importlib import import_module

import numpy as np
import pytest

import cand_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
B = 1 << 26
INF = math.inf


# ---- candidate_grid ------------------------------------------------------------------------------
def test_candidate_grid_is_row_major_with_the_first_axis_slowest():
    import lisp_mcmc_amd as mhx
    base = [":a", 1.0, ":mu", 2.0, ":w", 3.0, ":c", 4.0]
    cand, shape = mhx.candidate_grid(base, {":mu": [0.1, 0.2, 0.3], "c": [7.0, 8.0]})
    assert shape == (3, 2) and cand.shape == (6, 4) and cand.dtype == np.float64
    want, wshape = cc.grid([1.0, 2.0, 3.0, 4.0], [(1, [0.1, 0.2, 0.3]), (3, [7.0, 8.0])])
    assert wshape == shape and np.array_equal(cand, want)
    assert cand[:, 1].tolist() == [0.1, 0.1, 0.2, 0.2, 0.3, 0.3]      # the first axis is the slowest
    assert cand[:, 3].tolist() == [7.0, 8.0] * 3
    assert (cand[:, 0] == 1.0).all() and (cand[:, 2] == 3.0).all()     # the rest is the base
    assert np.array_equal(cand[:, 3].reshape(shape)[0], [7.0, 8.0])   # scores.reshape(shape) is the map
    # a dict base, a plist of axes, one axis, one value
    one, shape1 = mhx.candidate_grid({"a": 1.0, "b": 2.0}, [":b", [5.0]])
    assert shape1 == (1,) and np.array_equal(one, [[1.0, 5.0]])
    # the axes' order decides, not the parameters'
    swapped, sshape = mhx.candidate_grid(base, [":c", [7.0, 8.0], ":mu", [0.1, 0.2, 0.3]])
    assert sshape == (2, 3) and swapped[:, 3].tolist() == [7.0] * 3 + [8.0] * 3


def test_candidate_grid_refuses_what_it_cannot_place():
    import lisp_mcmc_amd as mhx
    base = {"a": 1.0, "b": 2.0}
    for axes in ({"z": [1.0]}, {"a": []}, {}, [":a", [1.0], ":a", [2.0]], [":a"]):
        with pytest.raises(ValueError):
            mhx.candidate_grid(base, axes)


# ---- the score and the ranking ---------------------------------------------------------------------
def test_total_adds_in_ascending_k_from_zero_and_is_infinite_where_not_finite():
    a, b, c = 0.1, 0.2, 0.3
    assert cc.total([a, b, c]) == (0.0 + a + b) + c != a + (b + c)
    assert cc.total([a]) == a and cc.total([]) == 0.0
    assert cc.total([1e308, 1e308]) == INF                       # the total overflows
    assert cc.total([1.0, float("nan")]) == INF and cc.total([INF]) == INF
    assert cc.total([1.0, 2.0], bad=True) == INF                 # a value or residual was not finite


def test_rank_on_planted_ties_infinities_and_fewer_candidates_than_kept():
    idx, val, bad = cc.rank([3.0, 1.0, 2.0, 1.0, INF, 0.5], 4)
    assert idx.tolist() == [5, 1, 3, 2] and val.tolist() == [0.5, 1.0, 1.0, 2.0] and bad == 1
    assert idx.dtype == np.int32
    # equal scores go to the smaller index - the infinite ones too, which rank last
    idx, val, bad = cc.rank([INF, 7.0, INF, 7.0], 4)
    assert idx.tolist() == [1, 3, 0, 2] and val.tolist() == [7.0, 7.0, INF, INF] and bad == 2
    # m < keep: the rest is (-1, +inf); an infinite candidate is still a candidate
    idx, val, bad = cc.rank([INF, 2.0], 5)
    assert idx.tolist() == [1, 0, -1, -1, -1] and val.tolist() == [2.0, INF, INF, INF, INF] and bad == 1
    idx, val, bad = cc.rank([4.0], 1)
    assert idx.tolist() == [0] and val.tolist() == [4.0] and bad == 0
    # +0.0 and -0.0 are equal scores; keep 16 of 70 with every score the same is 0 .. 15
    assert cc.rank([0.0, -0.0], 2)[0].tolist() == [0, 1]
    assert cc.rank([1.0] * 70, cc.KEEP_MAX)[0].tolist() == list(range(16))
    with pytest.raises(AssertionError):
        cc.rank([float("nan")], 1)


# ---- the Python layer without a device ---------------------------------------------------------------
class StubSummaries:
    """an engine's shape and nothing behind it: a call that reaches the library fails the test"""
    n_chains, d, _h = 3, 2, None

    def _summary(self, name):
        raise AssertionError("the library was called")


def stub():
    engine = import_module("lisp-mcmc_amd.engine")
    return type("Stub", (StubSummaries, engine._Summaries), {})()


def test_candidate_scores_checks_its_arguments_before_the_library():
    capi = import_module("lisp-mcmc_amd._capi")
    assert capi.CAND_KEEP_MAX == cc.KEEP_MAX == 16
    s = stub()
    ok = np.zeros((4, 2))
    for cand in (np.zeros((4, 3)), np.zeros(2), np.zeros((2, 4, 2)), np.zeros((3, 4, 3)), np.zeros((0, 2)),
                 np.zeros((3, 0, 2))):
        with pytest.raises(ValueError):
            s.candidate_scores(cand)
    for keep in (0, 17, -1):
        with pytest.raises(ValueError):
            s.candidate_scores(ok, keep=keep)
    with pytest.raises(AssertionError):      # good arguments do reach it
        s.candidate_scores(ok, keep=16)
    with pytest.raises(AssertionError):
        s.candidate_scores(np.zeros((3, 5, 2)), fn=0, keep=1, scores=True)


class PlantedEngine:
    """what the search asks of an engine, answered from planted numbers: the score of candidate j of
    chain c is score[c][j]; logpost(rows) = -score/2 of the row's first place minus a prior"""

    def __init__(self, best, score, prior=None):
        self.best = np.array(best, dtype=np.float64)
        self.n_chains, self.d, self.K = self.best.shape[0], self.best.shape[1], 1
        self.score, self.prior = score, prior or (lambda row: 0.0)
        self.calls, self.init = [], None

    def state(self):
        return {"best_theta": self.best}

    def candidate_scores(self, cand, fn=-1, keep=1, scores=False):
        cand = np.asarray(cand)
        self.calls.append((cand.copy(), fn, keep, scores))
        n, m = self.n_chains, cand.shape[-2]
        rows = cand if cand.ndim == 3 else np.broadcast_to(cand, (n,) + cand.shape)
        sc = np.array([[self.score(c, rows[c, j]) for j in range(m)] for c in range(n)])
        out = {"best_index": np.zeros((n, keep), dtype=np.int32), "best_score": np.zeros((n, keep)),
               "n_bad": np.zeros(n, dtype=np.int32)}
        for c in range(n):
            out["best_index"][c], out["best_score"][c], out["n_bad"][c] = cc.rank(sc[c], keep)
        if scores:
            out["score"] = sc
        return out

    def logpost(self, rows):
        assert rows.shape == (self.n_chains, self.d)
        return np.array([-0.5 * self.score(c, rows[c]) + self.prior(rows[c]) for c in range(self.n_chains)])

    def init_chains(self, theta):
        self.init = np.array(theta)


def planted_walker(e, keys):
    walker = import_module("lisp-mcmc_amd.walker")
    return walker.Walker(e, None, keys, [[np.zeros(4), np.zeros(4)]], [None], None, None)


def test_walker_set_search_takes_the_winner_under_the_prior():
    import lisp_mcmc_amd as mhx
    centre = [0.3, 0.7, 0.5]                       # walker c's dip
    e = PlantedEngine([[0.5, 9.0]] * 3, lambda c, row: INF if row[0] < 0 else (row[0] - centre[c]) ** 2 * 100.0,
                      prior=lambda row: -1e3 if row[0] > 0.65 else 0.0)
    w = planted_walker(e, ["mu", "c"])
    cand, _ = mhx.candidate_grid({"mu": 0.0, "c": 1.0}, {"mu": [-1.0, 0.1, 0.3, 0.5, 0.7, 0.9]})
    out = mhx.walker_set_search(w, candidates=cand, keep=3)
    assert len(e.calls) == 1 and e.calls[0][1:] == (-1, 3, False)      # one device call, all functions
    assert [o["index"] for o in out] == [2, 3, 3]                      # walker 1's best, 0.7, is beyond the prior
    assert out[0]["params"] == {"mu": 0.3, "c": 1.0} and out[0]["chi2"] == 0.0 and out[0]["logpost"] == 0.0
    assert out[1]["params"]["mu"] == 0.5 and out[1]["chi2"] == (0.5 - 0.7) ** 2 * 100.0
    assert [o["n-bad"] for o in out] == [1, 1, 1]
    assert e.init is None
    # without the prior the least chi-square wins; apply stands the walkers there
    out = mhx.walker_set_search(w, candidates=cand, keep=3, with_prior=False, apply=True)
    assert [o["index"] for o in out] == [2, 4, 3] and out[1]["logpost"] is None
    assert np.array_equal(e.init, cand[[2, 4, 3]])
    assert mhx.walker_search(w, chain=1, candidates=cand, keep=3, with_prior=False) == out[1]
    # axes: each walker's own most-likely vector with the key replaced (the per-chain form)
    e.best = np.array([[0.5, 9.0], [0.5, 8.0], [0.5, 7.0]])
    e.calls.clear()
    out = mhx.walker_set_search(w, axes={"mu": [0.3, 0.5]}, keep=2, with_prior=False)
    sent = e.calls[0][0]
    assert sent.shape == (3, 2, 2) and sent[:, :, 1].tolist() == [[9.0, 9.0], [8.0, 8.0], [7.0, 7.0]]
    assert [o["index"] for o in out] == [0, 1, 1] and out[1]["params"] == {"mu": 0.5, "c": 8.0}
    # no finite candidate: index -1 and the walker's most-likely parameters, which apply leaves it at
    out = mhx.walker_set_search(w, candidates=[[-1.0, 0.0], [-2.0, 0.0]], keep=4, apply=True)
    assert all(o["index"] == -1 and o["chi2"] == INF and o["n-bad"] == 2 for o in out)
    assert out[2]["params"] == {"mu": 0.5, "c": 7.0} and np.array_equal(e.init, e.best)
    for kw in ({}, {"candidates": cand, "axes": {"mu": [0.1]}}):
        with pytest.raises(ValueError):
            mhx.walker_set_search(w, **kw)


def test_walker_set_chi2_map_and_theta0_check_their_arguments():
    import lisp_mcmc_amd as mhx
    e = PlantedEngine([[0.5, 9.0], [0.25, 8.0]], lambda c, row: INF if row[1] < 0 else row[0] * 10.0 + row[1] + c)
    w = planted_walker(e, ["mu", "c"])
    r = mhx.walker_set_chi2_map(w, {"c": [1.0, -1.0, 3.0], "mu": [0.0, 1.0]})
    assert e.calls[0][0].shape == (2, 6, 2) and e.calls[0][1:] == (-1, 1, True)
    assert r["chi2"].shape == (2, 3, 2) and list(r["axes"]) == ["c", "mu"]
    assert r["chi2"][1].tolist() == [[2.0, 12.0], [INF, INF], [4.0, 14.0]]
    assert r["delta-chi2"][1].tolist() == [[0.0, 10.0], [INF, INF], [2.0, 12.0]]
    one = mhx.walker_set_chi2_map(w, [":mu", [0.0, 0.5]])
    assert one["chi2"].tolist() == [[9.0, 14.0], [9.0, 14.0]]           # the walker's own c stays
    with pytest.raises(ValueError):
        mhx.walker_set_chi2_map(w, {"mu": [0.0], "c": [1.0], "x": [2.0]})
    with pytest.raises(ValueError):
        mhx.walker_set_chi2_map(w, {"nu": [0.0]})
    with pytest.raises(ValueError):
        mhx.walker_set_least_squares(w, theta0=np.zeros((3, 2)))


# ---- the stage arithmetic ----------------------------------------------------------------------------
# "nb d per_chain keep m" answers "P fits|bytes off...|bytes off...": the portion, whether one chain
# fits at all, then the carving of 1 and of P chains
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26, "the budget");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    long long nb, m;
    int d, per_chain, keep;
    if (sscanf(line, "%lld %d %d %d %lld", &nb, &d, &per_chain, &keep, &m) != 5) return 1;
    std::vector<size_t> off;
    auto carve = [&](Carver& c, int64_t n) {
      const CandPieces s = carve_cand(c, nb, d, per_chain, keep, m, n);
      off = {s.cand, s.n_bad, s.best_index, s.best_score, s.score, s.part};
    };
    const bool fits = one_item_fits(carve);
    const long long P = fits ? portion_of(carve) : 0;
    printf("%lld %d", P, fits ? 1 : 0);
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


@pytest.fixture(scope="module")
def ask():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_cand_stage_")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])

    def run(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True,
                             text=True, check=True).stdout.split("\n")
        assert len(out) == len(queries) + 1 and out[-1] == ""
        return out[:-1]

    yield run
    shutil.rmtree(d, ignore_errors=True)


def cand_need(nb, d, per_chain, keep, m):
    """(fixed bytes, bytes per chain) of every piece, in the buffer's order: the header's outputs
    score [n][m], best_index and best_score [n][keep], n_bad [n], the candidates and the blocks' sums"""
    c = 8 * m * d
    return [(0, c) if per_chain else (c, 0), (0, 4), (0, 4 * keep), (0, 8 * keep), (0, 8 * m), (0, 8 * m * nb)]


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit(ask):
    shapes = list(itertools.product((1, 2, 391, 4000), (1, 7, 63), (0, 1), (1, 16), (1, 64, 289, 100000)))
    refused = 0
    for (nb, d, per_chain, keep, m), line in zip(shapes, ask(["%d %d %d %d %d" % s for s in shapes])):
        need = cand_need(nb, d, per_chain, keep, m)
        head, *carvings = line.split("|")
        P, fits = (int(w) for w in head.split())
        fixed, per = sum(f for f, _ in need), sum(v for _, v in need)
        slack = 256 * len(need)
        assert fits == (fixed + per + slack <= B), (nb, d, per_chain, keep, m, line)
        if not fits:
            refused += 1
            continue
        assert P == (B - fixed - slack) // per >= 1, (line,)
        assert fixed + (P + 1) * per + slack > B, (line,)              # one more chain would not fit
        for n, carving in zip((1, P), carvings):
            total, *off = (int(w) for w in carving.split())
            size = [f + n * v for f, v in need]
            assert len(off) == len(need)
            assert all(o % 256 == 0 for o in off) and off[0] == 0
            for k in range(len(off)):
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (line, n, k)
            assert total <= B, (line, n, total)
    # 1e5 candidates over 391 blocks are 313 MB of block sums a chain: such a call is refused
    assert refused > 0 and not (8 * 100000 * 391 <= B)
    # the timing tool's shapes: 289 shared candidates on two blocks, 64 on config 2's 391 blocks
    two = ask(["2 7 0 1 289", "391 8 0 1 64"])
    assert int(two[0].split()[0]) >= 4096 and 300 <= int(two[1].split()[0]) < 4096
