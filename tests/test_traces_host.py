"""CPU checks of the batched traces (mhx_get_traces): the thinning rule mhx_trace_rows against a
transliteration of the reference's `thin` (mcmc-fitting.lisp:149-157), the stage arithmetic of
carve_traces (csrc/mhx_stage.hpp) driven as tests/test_histo_stage_plan.py drives carve_histo, and
the argument check that needs no device."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
B = 1 << 26


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def thin(lst, n, start=0):
    """(thin list n start) M:149-157: the elements at the indices i with (i - start) mod n == 0"""
    if n == 1:
        return list(lst)
    return [lst[i] for i in range(len(lst)) if (i - start) % n == 0]


def test_trace_rows_is_the_length_of_thin(mhx):
    lib, capi = mhx.capi.lib(), mhx.capi
    checked = 0
    for length, stride in itertools.product(range(41), range(1, 10)):
        for start in range(stride):
            want = thin(list(range(length)), stride, start)
            # ... whose elements are the kept items start, start + stride, ...
            assert want == list(range(start, length, stride))
            rows = C.c_int64(-1)
            assert lib.mhx_trace_rows(length, stride, start, C.byref(rows)) == capi.OK
            assert rows.value == len(want), (length, stride, start)
            assert mhx.trace_rows(length, stride, start) == len(want)
            checked += 1
    assert checked == 41 * sum(range(1, 10))
    assert lib.mhx_trace_rows(5, 2, 0, None) == capi.OK      # the output may be NULL


def test_trace_rows_refuses_what_thin_cannot_mean(mhx):
    lib, capi = mhx.capi.lib(), mhx.capi
    rows = C.c_int64(-1)
    for n_kept, stride, start in ((5, 0, 0), (5, -1, 0), (5, 3, -1), (5, 3, 3), (5, 3, 4), (5, 1, 1), (-1, 1, 0)):
        assert lib.mhx_trace_rows(n_kept, stride, start, C.byref(rows)) == capi.EINVAL, (n_kept, stride, start)
        assert lib.mhx_last_error()
        with pytest.raises(ValueError):
            mhx.trace_rows(n_kept, stride, start)
    assert rows.value == -1


def test_a_null_engine_or_group_is_refused(mhx):
    lib, capi = mhx.capi.lib(), mhx.capi
    _c, cols = capi.as_i32([capi.TRACE_PROB, 0])
    for fn in (lib.mhx_get_traces, lib.mhx_group_get_traces):
        assert fn(None, 10, capi.TRACE_STEPS, 1, 0, cols, 2, 10, None, None, None, None, None, None) == capi.EINVAL
        assert b"NULL" in lib.mhx_last_error()


# "n_cols max_out take envelope" answers "P fits|bytes off...|bytes off...": the portion, whether
# one chain fits at all, then the carving of 1 and of P chains
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mhx_stage.hpp"
using namespace mhx;
typedef std::vector<size_t> Offsets;
int main() {
  static_assert(kStageBudget == (size_t)1 << 26, "the budget");
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    int nc, mo, take, env;
    if (sscanf(line, "%d %d %d %d", &nc, &mo, &take, &env) != 4) return 1;
    Offsets off;
    auto carve = [&](Carver& c, int64_t n) {
      const TracePieces s = carve_traces(c, nc, mo, take, env, n);
      off = {s.cols, s.values, s.lo, s.hi, s.n_out, s.n_kept, s.n_used, s.kept};
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


@pytest.fixture(scope="module")
def ask():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_traces_stage_")
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


def pieces(n_cols, max_out, take, envelope):
    """(fixed bytes, bytes per chain) of every piece, in the buffer's order: the column list, the
    rows, their envelopes, the three counts, the kept-index scratch"""
    rows = 8 * max_out * n_cols
    env = rows if envelope else 0
    return [(4 * n_cols, 0), (0, rows), (0, env), (0, env), (0, 4), (0, 4), (0, 4), (0, 4 * take)]


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit(ask):
    shapes = list(itertools.product((1, 9, 34), (1, 64, 2048, 32768), (1, 2048, 32768), (0, 1)))
    assert len(shapes) == 3 * 4 * 3 * 2
    lines = ask(["%d %d %d %d" % s for s in shapes])
    several = 0
    for shape, line in zip(shapes, lines):
        need = pieces(*shape)
        head, *carvings = line.split("|")
        P, fits = (int(w) for w in head.split())
        fixed, per = sum(f for f, _ in need), sum(v for _, v in need)
        slack = 256 * len(need)
        assert fits == (fixed + per + slack <= B) == 1, (shape, line)     # every shape here fits
        assert P == (B - fixed - slack) // per >= 1, (shape, line)
        assert fixed + (P + 1) * per + slack > B, (shape, line)           # one more chain would not fit
        several += P > 1
        for n, carving in zip((1, P), carvings):
            total, *off = (int(w) for w in carving.split())
            size = [f + n * v for f, v in need]
            assert len(off) == len(need), (shape, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (shape, n, off)
            for k in range(len(off)):
                assert off[k] + size[k] <= (off[k + 1] if k + 1 < len(off) else total), (shape, n, k, off)
            assert total <= B, (shape, n, total)
            if not shape[3]:    # without an envelope lo and hi take no bytes: three offsets coincide
                assert off[2] == off[3] == off[4], (shape, n, off)
            else:
                assert off[3] - off[2] >= size[2] > 0 and off[4] - off[3] >= size[3] > 0
    assert several > len(shapes) // 2
    # the widest shape: three arrays of 32768 x 34 doubles are 26.7 MB of a chain's 64 MiB
    assert lines[-1].split("|")[0] == "2 1"
