"""CPU checks of the planner's rules for a dataset per walker (csrc/mhx_plan.hpp): such a problem
always takes the batch kernels, and whether its planes stay in LDS is a pure function of lengths,
sigma kinds, the number of functions and the kernel family.  A small driver compiled against the
header, as tests/test_launch_plan.py has one."""
import csv
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
CASES = os.path.join(ROOT, "tests", "golden", "launch_plan_cases.csv")
ENV_COLS = ["MHX_FAMILY_WPG", "MHX_SPLIT", "MHX_TSPLIT", "MHX_NO_PERSIST", "MHX_PERSIST_TS",
            "MHX_PERSIST_FILL", "MHX_COMPACT_ALWAYS", "MHX_NO_COMPACT"]
OUT_COLS = ["family", "want_split", "tsplit", "split_slices", "persist", "ts_initial",
            "reslice_3q", "reslice_1q", "reslice_1", "deal_initial", "deal_3q", "deal_1q", "deal_1"]
NONE, SHARED, PER_CHAIN, PER_POINT = 0, 1, 2, 3

# "plan": rows of the golden table on stdin, planned with ProblemShape::planes set -> want_split,
#         tsplit, split_slices, persist.
# "resident wpg K n kind [n kind ...]": planes_resident of those functions in a problem of K.
# "knob": planes_no_lds of the environment as it is, and the defaults of the new fields.
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mhx_plan.hpp"
using namespace mhx;
int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "knob")) {
    printf("%d %d %d\n", (int)read_knobs().planes_no_lds, (int)EngineKnobs().planes_no_lds,
           (int)ProblemShape().planes);
    return 0;
  }
  if (argc > 3 && !strcmp(argv[1], "resident")) {
    int64_t n[MHX_MAX_FUNCTIONS];
    int kind[MHX_MAX_FUNCTIONS], np = 0;
    for (int i = 4; i + 1 < argc; i += 2) {
      n[np] = atoll(argv[i]);
      kind[np++] = atoi(argv[i + 1]);
    }
    printf("%d %lld\n", (int)planes_resident(n, kind, np, atoi(argv[3]), atoi(argv[2]), read_knobs()),
           (long long)planes_lds_capacity(atoi(argv[2])));
    return 0;
  }
  static const char* names[8] = {"MHX_FAMILY_WPG", "MHX_SPLIT", "MHX_TSPLIT", "MHX_NO_PERSIST", "MHX_PERSIST_TS",
                                 "MHX_PERSIST_FILL", "MHX_COMPACT_ALWAYS", "MHX_NO_COMPACT"};
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    long long longest, K, d, heavy, chains, pooled, capable, poff, cus, pc, pcts;
    char env[8][32];
    if (sscanf(line, "%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%31[^,],%31[^,],%31[^,],%31[^,],"
               "%31[^,],%31[^,],%31[^,],%31[^,\n]", &longest, &K, &d, &heavy, &chains, &pooled, &capable, &poff,
               &cus, &pc, &pcts, env[0], env[1], env[2], env[3], env[4], env[5], env[6], env[7]) != 19)
      return 1;
    for (int i = 0; i < 8; ++i) {
      if (!strcmp(env[i], "-")) unsetenv(names[i]);
      else setenv(names[i], strcmp(env[i], "_") ? env[i] : "", 1);
    }
    const EngineKnobs kn = read_knobs();
    ProblemShape s;
    s.longest = longest;
    s.nwin = ceil_div(longest, kPadPoints);
    s.K = (int)K;
    s.d = (int)d;
    s.heavy = heavy != 0;
    s.chains = chains;
    s.pooled = pooled != 0;
    s.persist_off = poff != 0;
    s.cus = (int)cus;
    s.waves_per_group = choose_family(s, kn);
    s.tile_points = tile_points_of(s.waves_per_group);
    s.per_cu = (int)pc;
    s.per_cu_ts = (int)pcts;
    s.planes = true;
    const bool want = want_split(s, kn, capable != 0);
    s.capable = capable != 0;
    const LaunchPlan p = plan_modes(s, kn);
    printf("%d,%d,%d,%d,%d\n", (int)want, (int)p.tsplit, p.split_slices, (int)p.persist, p.ts_initial);
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_planes_plan_")
    src, exe = os.path.join(d, "planes_driver.cpp"), os.path.join(d, "planes_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
    yield exe
    shutil.rmtree(d, ignore_errors=True)


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("MHX_")}


def test_a_problem_with_planes_takes_the_batch_kernels(driver):
    """every row of the recorded table whose plan is a split or persistent form - whatever
    MHX_SPLIT, MHX_TSPLIT or MHX_PERSIST_TS say - is the batch form once a function has planes"""
    with open(CASES) as f:
        rows = [r for r in csv.DictReader(f) if r["split_slices"] != "0" or r["persist"] != "0"]
    assert len(rows) >= 50
    assert {r["tsplit"] for r in rows} == {"0", "1"} and {r["persist"] for r in rows} == {"0", "1"}
    assert any(r[c] not in ("-", "0") for r in rows for c in ("MHX_SPLIT",))
    assert any(r[c] not in ("-", "0") for r in rows for c in ("MHX_TSPLIT",))
    assert any(r["MHX_PERSIST_TS"] == "1" for r in rows)
    in_cols = [c for c in rows[0] if c not in OUT_COLS]
    feed = "".join(",".join(r[c] for c in in_cols) + "\n" for r in rows)
    out = subprocess.run([driver], input=feed, capture_output=True, text=True, env=clean_env(), check=True)
    got = out.stdout.strip().split("\n")
    assert len(got) == len(rows)
    bad = [(",".join(r[c] for c in in_cols), g) for r, g in zip(rows, got) if g != "0,0,0,0,0"]
    assert not bad, "%d of %d rows are not the batch form, first: %s" % (len(bad), len(rows), bad[:3])


def resident(driver, wpg, K, fns, env=None):
    e = clean_env()
    e.update(env or {})
    args = [driver, "resident", str(wpg), str(K)] + [str(v) for f in fns for v in f]
    r, cap = subprocess.run(args, capture_output=True, text=True, env=e, check=True).stdout.split()
    return int(r), int(cap)


def pad(n):
    return max((n + 127) // 128, 1) * 128


def longest_that_fits(wpg, shared_arrays, wave_arrays):
    """from the rule as DESIGN.md states it: pad(n) * (shared + wpg * per wave) <= the doubles
    of the tile buffers (2 buffers x 4 arrays x 128 wpg points)"""
    cap = 2 * 4 * 2 * 64 * wpg
    return cap // (shared_arrays + wpg * wave_arrays) // 128 * 128


@pytest.mark.parametrize("wpg", [8, 16])
@pytest.mark.parametrize("kind,shared,wave", [(PER_CHAIN, 1, 1), (NONE, 1, 1), (SHARED, 2, 1),
                                              (PER_POINT, 1, 2)])
def test_the_resident_rule_at_its_boundaries(driver, wpg, kind, shared, wave):
    cap = resident(driver, wpg, 1, [(1, kind)])[1]
    assert cap == {8: 8192, 16: 16384}[wpg]
    n = longest_that_fits(wpg, shared, wave)
    assert n > 0 and pad(n) == n
    assert resident(driver, wpg, 1, [(n, kind)])[0] == 1
    assert resident(driver, wpg, 1, [(n - 127, kind)])[0] == 1      # (the same padded length)
    assert resident(driver, wpg, 1, [(n + 1, kind)])[0] == 0
    assert resident(driver, wpg, 1, [(n + 64, kind)])[0] == 0
    # the sizes the GPU tests use: 334 points resident, 1500 streamed, in every kind and family
    assert resident(driver, wpg, 1, [(334, kind)])[0] == 1
    assert resident(driver, wpg, 1, [(1500, kind)])[0] == 0


def test_without_a_per_wave_sigma_plane_nearly_twice_the_length_fits():
    for wpg in (8, 16):
        assert longest_that_fits(wpg, 1, 1) >= 2 * longest_that_fits(wpg, 1, 2)
    assert (longest_that_fits(8, 1, 1), longest_that_fits(8, 1, 2)) == (896, 384)
    assert (longest_that_fits(16, 1, 1), longest_that_fits(16, 1, 2)) == (896, 384)


def test_resident_needs_the_tile_buffers_for_itself(driver):
    # two functions on planes share the space ...
    assert resident(driver, 8, 2, [(384, PER_CHAIN), (384, PER_CHAIN)])[0] == 1
    assert resident(driver, 8, 2, [(512, PER_CHAIN), (512, PER_CHAIN)])[0] == 0
    # ... a function on a shared dataset beside them stages its tiles there: streamed
    assert resident(driver, 8, 2, [(128, PER_CHAIN)])[0] == 0
    assert resident(driver, 16, 3, [(128, NONE), (128, NONE)])[0] == 0


def test_the_knob_parses_like_the_other_flags(driver):
    def knob(env):
        e = clean_env()
        e.update(env)
        return subprocess.run([driver, "knob"], capture_output=True, text=True, env=e, check=True).stdout.split()
    assert knob({}) == ["0", "0", "0"]              # (the new fields default to "off")
    for val, on in (("0", "0"), ("1", "1"), ("", "0"), ("abc", "0"), ("7", "1")):
        assert knob({"MHX_PLANES_NO_LDS": val})[0] == on, val
    assert resident(driver, 8, 1, [(334, PER_CHAIN)], {"MHX_PLANES_NO_LDS": "1"})[0] == 0
    assert resident(driver, 8, 1, [(334, PER_CHAIN)], {"MHX_PLANES_NO_LDS": "0"})[0] == 1
