"""CPU checks of the stage arithmetic of the histogram and pair-grid read-outs (carve_histo,
carve_grid, one_item_fits in csrc/mhx_stage.hpp), driven as tests/test_stage_plan.py drives the
other read-outs: a small program compiled against the header answers for a grid of shapes.  A
portion's carved bytes stay within the budget, its pieces lie in the engine's order without
reaching into each other, and by the planner's accounting (the bytes asked for plus one alignment
unit per piece) one more chain would not fit."""
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
B = 1 << 26
NCS, HISTO_BINS, GRID_BINS, NPS = (1, 2, 8, 33, 63), (1, 2, 20, 1024), (1, 20, 64), (0, 1, 28, 1953, 4096)

# "h nc nb per_chain" / "g nc nb np per_chain" answer "P fits|bytes off...|bytes off...": the
# portion, whether one chain fits at all, then the carving of 1 and of P chains
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
typedef std::vector<size_t> Offsets;
template <class Carve>
static void answer(Carve carve) {  // carve(carver, n, &offsets)
  Offsets off;
  const long long P = portion_of([&](Carver& c, int64_t n) { carve(c, n, off); });
  printf("%lld %d", P, one_item_fits([&](Carver& c, int64_t n) { carve(c, n, off); }) ? 1 : 0);
  for (long long n : {1LL, P}) {
    Carver c;
    carve(c, n, off);
    if ((size_t)c.pieces() != off.size()) printf(" PIECES");
    printf("|%zu", c.bytes());
    for (size_t o : off) printf(" %zu", o);
  }
  printf("\n");
}
int main() {
  static_assert(kStageBudget == (size_t)1 << 26, "the budget");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    int a, b, c, d = 0;
    if (sscanf(line + 1, "%d %d %d %d", &a, &b, &c, &d) < 3) return 1;
    if (line[0] == 'h') {
      answer([&](Carver& cv, int64_t n, Offsets& off) {
        const HistoPieces s = carve_histo(cv, a, b, c, n);
        off = {s.edges, s.counts, s.outside, s.n_used, s.status};
      });
    } else {
      answer([&](Carver& cv, int64_t n, Offsets& off) {
        const GridPieces s = carve_grid(cv, a, b, c, d, n);
        off = {s.edges, s.pairs, s.counts, s.n_inside, s.n_used, s.status};
      });
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
    d = tempfile.mkdtemp(prefix="mhx_histo_stage_")
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


def histo_case(nc, nb, per_chain):
    """the query and (fixed bytes, bytes per chain) of every piece, in the buffer's order"""
    e = 8 * nc * (nb + 1)
    need = [(0, e) if per_chain else (e, 0), (0, 4 * nc * nb), (0, 8 * nc), (0, 4), (0, 4 * nc)]
    return "h %d %d %d" % (nc, nb, per_chain), need


def grid_case(nc, nb, np_, per_chain):
    e = 8 * nc * (nb + 1)
    need = [(0, e) if per_chain else (e, 0), (8 * np_, 0), (0, 4 * np_ * nb * nb), (0, 4 * np_), (0, 4),
            (0, 4 * np_)]
    return "g %d %d %d %d" % (nc, nb, np_, per_chain), need


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit(ask):
    cases = [histo_case(*a) for a in itertools.product(NCS, HISTO_BINS, (0, 1))]
    cases += [grid_case(*a) for a in itertools.product(NCS, GRID_BINS, NPS, (0, 1))]
    assert len(cases) == 5 * 4 * 2 + 5 * 3 * 5 * 2
    refused = 0
    for (query, need), line in zip(cases, ask([c[0] for c in cases])):
        head, *carvings = line.split("|")
        P, fits = (int(w) for w in head.split())
        fixed, per = sum(f for f, _ in need), sum(v for _, v in need)
        slack = 256 * len(need)
        assert fits == (fixed + per + slack <= B), (query, line)
        if not fits:
            refused += 1
            continue
        assert P == (B - fixed - slack) // per >= 1, (query, line)
        assert fixed + (P + 1) * per + slack > B, (query, line)    # one more chain would not fit
        for n, carving in zip((1, P), carvings):
            total, *off = (int(w) for w in carving.split())
            size = [f + n * v for f, v in need]
            assert len(off) == len(need), (query, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (query, n, off)
            for k in range(len(off)):
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (query, n, k, off)
            assert total <= B, (query, n, total)
        # the edges come first, and shared edges leave the chains' pieces where one chain has them
        assert carvings[0].split()[1] == carvings[1].split()[1] == "0"
    # 4096 pairs of 64 x 64 cells are 64 MiB by themselves: no chain fits, whatever the rest
    assert refused == 5 * 2
