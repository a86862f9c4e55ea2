"""CPU checks of mhx_get_fit_percentiles' stage arithmetic (csrc/mhx_stage.hpp: carve_fitpct,
fitpct_cursor, fitpct_max_take), in the way test_stage_plan.py checks the other read-outs': a small
driver compiled against the header answers for a grid of shapes, and the answers are compared
with the bytes every piece needs, restated here in Python integers.

The call stages `take` doubles per chain and point, so the chunk of points cannot be
portion_cursor's fixed 2^17: it is all of m where one chain fits the 64 MiB budget with them, else
the largest whole number of blocks of the value kernel (128 points) with which one chain fits."""
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
BLOCK = 128
TAKES = (1, 8, 1000, 1024, 65536)
MS = (1, 5, BLOCK - 1, BLOCK, BLOCK + 1, 1000, CHUNK + 1000)
NPCTS = (0, 3, 16)
N_PIECES = 8

# "q take n_pct m items" answers "chunk per_portion max_take|bytes off...|bytes off...|portions":
# the cursor, the carving of 1 and of per_portion chains at the chunk, and the cursor's portions
# "i0,n,m0,m" (the first and last 40 when there are more; their count and the cells they cover lead).
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26 && kFitChunkPoints == 1 << 17 && kFitPctBlock == 128,
                "the budget, the chunk and the block");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    long long take, n_pct, m, items;
    if (sscanf(line + 1, "%lld %lld %lld %lld", &take, &n_pct, &m, &items) != 4) return 1;
    PortionCursor at = fitpct_cursor(items, m, (int)take, (int)n_pct);
    printf("%lld %lld %d", (long long)at.chunk, (long long)at.per_portion, fitpct_max_take(m, (int)n_pct));
    for (long long n : {1LL, (long long)at.per_portion}) {
      Carver c;
      const FitPctPieces s = carve_fitpct(c, (int)take, (int)n_pct, n, at.chunk);
      printf("|%zu %d %zu %zu %zu %zu %zu %zu %zu %zu", c.bytes(), c.pieces(), s.status, s.n_used, s.x0, s.x1,
             s.values, s.pct, s.mean, s.stddev);
    }
    printf("|");
    if (at.chunk > 0) {
      std::vector<Portion> all;
      long long cells = 0;
      for (; !at.done(); at.advance()) {
        all.push_back(at.now());
        cells += (long long)at.now().n * at.now().m;
      }
      printf("%zu %lld", all.size(), cells);
      for (size_t k = 0; k < all.size(); ++k)
        if (k < 40 || k + 40 >= all.size())
          printf(" %lld,%lld,%lld,%lld", (long long)all[k].i0, (long long)all[k].n, (long long)all[k].m0,
                 (long long)all[k].m);
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
    d = tempfile.mkdtemp(prefix="mhx_fitpct_stage_")
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


def need(take, n_pct, n, m):
    """the bytes of every piece, in the order they lie in the buffer"""
    return [4 * n, 4 * n, 8 * m, 8 * m, 8 * n * m * take, 8 * n * n_pct * m, 8 * n * m, 8 * n * m]


def one_fits(take, n_pct, m):
    """one chain's pieces and a piece's worth of alignment each within the budget"""
    return sum(need(take, n_pct, 1, m)) + N_PIECES * 256 <= B


def want_chunk(take, n_pct, m):
    if m <= CHUNK and one_fits(take, n_pct, m):
        return m
    blocks = [k for k in range(1, min(m, CHUNK) // BLOCK + 1) if one_fits(take, n_pct, k * BLOCK)]
    return blocks[-1] * BLOCK if blocks else 0


GRID = list(itertools.product(TAKES, MS, NPCTS))


def test_the_chunk_of_points_and_the_carving_over_the_grid(ask):
    lines = ask(["q %d %d %d 3" % (take, n_pct, m) for take, m, n_pct in GRID])
    refused = 0
    for (take, m, n_pct), line in zip(GRID, lines):
        head, one, many, _ = line.split("|")
        chunk, per, max_take = (int(w) for w in head.split())
        # whole blocks and at most kFitChunkPoints, or all of m
        assert chunk == want_chunk(take, n_pct, m), (take, m, n_pct, line)
        assert chunk <= CHUNK and (chunk == m or chunk % BLOCK == 0)
        # the greatest take whose smallest chunk, min(m, block) points, one chain can stage
        small = min(m, BLOCK)
        assert one_fits(max_take, n_pct, small) and not one_fits(max_take + 1, n_pct, small)
        if chunk == 0:      # not even the smallest chunk fits: the call is refused
            refused += 1
            assert not one_fits(take, n_pct, small) and max_take < take
            continue
        assert one_fits(take, n_pct, chunk)
        # ... and the next larger chunk would not fit, or the chunk is all of m
        if chunk != m:
            assert chunk + BLOCK > CHUNK or not one_fits(take, n_pct, chunk + BLOCK), (take, m, n_pct)
        fixed, per_item = sum(need(take, n_pct, 0, chunk)), sum(need(take, n_pct, 1, chunk)) - sum(need(take, n_pct, 0, chunk))
        assert per == max(1, (B - fixed - N_PIECES * 256) // per_item), (take, m, n_pct, per)
        for n, carving in ((1, one), (per, many)):
            total, pieces, *off = (int(w) for w in carving.split())
            size = need(take, n_pct, n, chunk)
            assert pieces == N_PIECES == len(off)
            assert all(o % 256 == 0 for o in off) and off[0] == 0
            for k in range(N_PIECES):   # in order, no piece reaching into the next or past the end
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < N_PIECES else total), (take, m, n_pct, n, k)
            assert total <= B, (take, m, n_pct, n, total)
    # take 65536 with a whole block or more of points is what does not fit (127 points still do)
    assert refused == sum(1 for take, m, _ in GRID if take == 65536 and m >= BLOCK) == 12


def test_the_cursor_covers_items_and_points_exactly_once(ask):
    cases = [(take, n_pct, m, items) for take, m, n_pct in GRID for items in (1, 3, 4099)
             if want_chunk(take, n_pct, m) > 0]
    for (take, n_pct, m, items), line in zip(cases, ask(["q %d %d %d %d" % c for c in cases])):
        head, _, _, tail = line.split("|")
        chunk, per, _ = (int(w) for w in head.split())
        count, cells, *shown = tail.split()
        want = [(i0, min(per, items - i0), m0, min(chunk, m - m0))
                for i0 in range(0, items, per) for m0 in range(0, m, chunk)]
        assert int(count) == len(want) and int(cells) == items * m, (take, n_pct, m, items)
        got = [tuple(int(v) for v in w.split(",")) for w in shown]
        assert got == (want if len(want) <= 80 else want[:40] + want[-40:]), (take, n_pct, m, items)
        if items * m <= 5000 and len(want) <= 80:
            seen = [(i, j) for i0, n, m0, mm in got for i in range(i0, i0 + n) for j in range(m0, m0 + mm)]
            assert sorted(seen) == [(i, j) for i in range(items) for j in range(m)]


def test_take_1000_at_1000_points_is_what_the_issue_sized(ask):
    """4096 chains, take 1000, 1000 points, three percentiles: all 1000 points in one chunk, eight
    chains a portion (8 MB of values each)"""
    head = ask(["q 1000 3 1000 4096"])[0].split("|")[0].split()
    assert [int(head[0]), int(head[1])] == [1000, (B - 16000 - 8 * 256) // (8 + 8000 * 1000 + 8 * 5 * 1000)]
    assert int(head[1]) == 8
