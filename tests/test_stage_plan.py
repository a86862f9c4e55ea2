"""CPU checks of the batched read-outs' stage arithmetic (csrc/mhx_stage.hpp): how many items a
portion holds, how its pieces are carved, and the order of the portions.  A small driver compiled
against the header answers for a grid of shapes.  The portion sizes are compared with the formulas
the three read-outs had when each kept its own (restated here in Python integers: the slack
literals 5, 8 and 7 times 256 were the piece counts of carvers written elsewhere); the carving is
checked against the bytes every piece needs, in the order the engine lays them out."""
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
B = 1 << 26
CHUNK = 1 << 17
DS, TAKES, NPCTS, NES = (1, 2, 33, 63), (1, 8, 1000, 1024, 65536), (1, 16), (1, 16)
MS = (1, 5, CHUNK - 1, CHUNK, CHUNK + 1000, 1 << 20)
PERCENTILES, COVARIANCES, FACTORS, BEST = range(4)

# One query per line on stdin.  "s kind d n_pct take", "f d take m" (m: all the points of the call)
# and "d ne take n_pct" answer "P chunk|bytes off...|bytes off..." - the portion and the chunk of
# points of the call's cursor, then the carving of 1 and of P items at a chunk of points (a piece
# count that is not the carver's own spoils the line); "c items per_portion points chunk" answers
# a cursor's portions "i0,n,m0,m ...".
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
typedef std::vector<size_t> Offsets;
template <class Carve>
static void answer(long long points, Carve carve) {  // carve(carver, n, m, &offsets)
  Offsets off;
  const PortionCursor at =
      portion_cursor(1, points, [&](Carver& c, int64_t n, int64_t m) { carve(c, n, m, off); });
  printf("%lld %lld", (long long)at.per_portion, (long long)at.chunk);
  for (long long n : {1LL, (long long)at.per_portion}) {
    Carver c;
    carve(c, n, at.chunk, off);
    if ((size_t)c.pieces() != off.size()) printf(" PIECES");
    printf("|%zu", c.bytes());
    for (size_t o : off) printf(" %zu", o);
  }
  printf("\n");
}
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17, "the budget and the chunk");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    long long a, b, c, d = 0;
    if (sscanf(line + 1, "%lld %lld %lld %lld", &a, &b, &c, &d) < 3) return 1;
    if (line[0] == 's') {
      const SummaryShape y = summary_shape((int)a, (int)b, (int)c, (int)d);
      answer(1, [&](Carver& cv, int64_t n, int64_t, Offsets& off) {
        const SummaryPieces s = carve_summary(cv, y, n);
        off = {s.dv[0], s.dv[1], s.iv[0], s.iv[1], s.scratch};
      });
    } else if (line[0] == 'f') {
      answer(c, [&](Carver& cv, int64_t n, int64_t m, Offsets& off) {
        const FitPieces s = carve_fit(cv, (int)a, (int)b, n, m);
        off = {s.sel, s.n_sel, s.status, s.theta, s.x0, s.x1, s.ymax, s.ymin};
      });
    } else if (line[0] == 'd') {
      answer(1, [&](Carver& cv, int64_t n, int64_t, Offsets& off) {
        const DerivedPieces s = carve_derived(cv, (int)a, (int)b, (int)c, n);
        off = {s.values, s.at_best, s.pct, s.mean, s.stddev, s.n_used, s.status};
      });
    } else {
      PortionCursor at;
      at.items = a, at.per_portion = b, at.points = c, at.chunk = d;
      for (; !at.done(); at.advance()) {
        const Portion p = at.now();
        printf("%lld,%lld,%lld,%lld ", (long long)p.i0, (long long)p.n, (long long)p.m0, (long long)p.m);
      }
      printf("\n");
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def ask():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_stage_")
    src, exe = os.path.join(d, "stage_driver.cpp"), os.path.join(d, "stage_driver")
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


def summary_case(kind, d, n_pct, take):
    """the query, the portion of the read-out's own formula, the points of a chunk, and the bytes
    per item that each piece needs, in the order the pieces lie in the buffer (fixed bytes: none)"""
    nd0, nd1, ni, scratch = {PERCENTILES: (n_pct * d, 0, 1, False), COVARIANCES: (d * d, 0, 2, True),
                             FACTORS: (d * d, d * d, 2, True), BEST: (1, d, 0, False)}[kind]
    per = 8 * (nd0 + nd1) + 4 * ni + (4 * take if scratch else 0)
    need = [8 * nd0, 8 * nd1, 4 if ni > 0 else 0, 4 if ni > 1 else 0, 4 * take if scratch else 0]
    return "s %d %d %d %d" % (kind, d, n_pct, take), max(1, (B - 5 * 256) // per), 1, [(0, v) for v in need]


def fit_case(d, take, m):
    mc = min(m, CHUNK)
    P = max(1, (B - (16 * mc + 8 * 256)) // (16 * mc + 8 * d + 4 * take + 8))
    need = [(0, 4 * take), (0, 4), (0, 4), (0, 8 * d if take == 0 else 0), (8 * mc, 0), (8 * mc, 0),
            (0, 8 * mc), (0, 8 * mc)]
    return "f %d %d %d" % (d, take, m), P, mc, need


def derived_case(ne, take, n_pct):
    P = max(1, (B - 7 * 256) // (8 * (ne * take + ne * (3 + n_pct)) + 4 * (1 + ne)))
    need = [8 * ne * take, 8 * ne, 8 * ne * n_pct, 8 * ne, 8 * ne, 4, 4 * ne]
    return "d %d %d %d" % (ne, take, n_pct), P, 1, [(0, v) for v in need]


def all_cases():
    cases = [summary_case(*a) for a in itertools.product(range(4), DS, NPCTS, TAKES)]
    cases += [fit_case(*a) for a in itertools.product(DS, (0,) + TAKES, MS)]
    cases += [derived_case(*a) for a in itertools.product(NES, TAKES, NPCTS)]
    return cases


def test_portions_and_carving_over_the_grid(ask):
    cases = all_cases()
    assert len(cases) == 4 * 4 * 2 * 5 + 4 * 6 * 6 + 2 * 5 * 2
    assert len({c[0] for c in cases}) == len(cases)    # every grid point is a query of its own
    for (query, want_p, want_chunk, need), line in zip(cases, ask([c[0] for c in cases])):
        head, *carvings = line.split("|")
        assert [int(w) for w in head.split()] == [want_p, want_chunk], (query, line)
        fixed, per = sum(f for f, _ in need), sum(v for _, v in need)
        for n, carving in zip((1, want_p), carvings):
            total, *off = (int(w) for w in carving.split())
            size = [f + n * v for f, v in need]
            assert len(off) == len(need), (query, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (query, n, off)
            # in the engine's order, no piece reaching into the next or past the end
            for k in range(len(off)):
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (query, n, k, off)
            if fixed + len(need) * 256 + per <= B:    # (one item fits at all)
                assert total <= B, (query, n, total)


def test_the_cursor_covers_items_and_points_once_points_first(ask):
    tuples = [(10, 4, 1, 1), (8, 4, 1, 1), (1, 1, 1, 1), (0, 3, 5, 2), (7, 3, 10, 4), (7, 3, 3, 4), (6, 3, 8, 4),
              (5, 7, 9, 2), (3, 1, CHUNK + 1000, CHUNK), (4000, 3842, 1, 1)]
    for (items, per, m, chunk), line in zip(tuples, ask(["c %d %d %d %d" % t for t in tuples])):
        got = [tuple(int(v) for v in w.split(",")) for w in line.split()]
        want = [(i0, min(per, items - i0), m0, min(chunk, m - m0))
                for i0 in range(0, items, per) for m0 in range(0, m, chunk)]
        assert got == want, (items, per, m, chunk)
        if items * m <= 1000:
            cells = [(i, j) for i0, n, m0, mm in got for i in range(i0, i0 + n) for j in range(m0, m0 + mm)]
            assert sorted(cells) == [(i, j) for i in range(items) for j in range(m)]
