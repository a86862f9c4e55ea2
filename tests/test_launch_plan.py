"""CPU checks of the engine's launch-mode rules (csrc/mhx_plan.hpp): which kernel family, split
mode, slice count and persistent form a problem gets, how a tile-sliced run re-slices and how the
batch kernels deal their chains.  A small driver compiled against the header runs the planner over
tests/golden/launch_plan_cases.csv, whose expected columns were recorded from the engine's rules
before they moved into the header (every branch of them taken), and read_knobs() is checked
against a handful of environments."""
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

# One row per line on stdin: the problem's numbers, then the switches as environment values ("-":
# unset, "_": set to ""), which the driver sets before read_knobs().  Out: OUT_COLS; the re-slicing
# and the deals after 3/4, 1/4 of the chains and all but one have finished (-1: no repack due).
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mhx_plan.hpp"
using namespace mhx;
int main(int argc, char** argv) {
  if (argc > 1) {  // read_knobs() of the environment as it is
    const EngineKnobs k = read_knobs();
    printf("%d %d %d %d %d %d %d %d", k.family_wpg, k.split_set, k.split, k.tsplit_set, k.tsplit, k.no_persist,
           k.persist_ts, k.persist_fill);
    printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d\n", k.no_resident_slices, k.no_window_grids, k.no_tile_skip,
           k.no_recognise, k.no_yw, k.no_deal, k.force_generic, k.no_rtc_specialise, k.early_reject, k.no_compact,
           k.compact_always, k.no_graph, (int)sizeof(EngineKnobs));
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
    const bool want = want_split(s, kn, capable != 0);
    s.capable = capable != 0;
    const LaunchPlan p = plan_modes(s, kn);
    const int64_t W = s.waves_per_group, runs[3] = {chains * 3 / 4, chains / 4, 1};
    long long res[3], deal[3];
    const bool batch = !kn.no_compact && p.split_slices == 0;
    for (int i = 0; i < 3; ++i) {
      const bool due = !kn.no_compact && repack_due(runs[i], chains);
      res[i] = p.tsplit && due ? reslice_tsplit(s, kn, p.split_slices, p.persist, ceil_div(runs[i], W)) : -1;
      deal[i] = batch && due ? deal_target(s.cus, W, chains, runs[i], kn.compact_always) : -1;
    }
    printf("%d,%d,%d,%d,%d,%d,%lld,%lld,%lld,%lld,%lld,%lld,%lld\n", s.waves_per_group, (int)want, (int)p.tsplit,
           p.split_slices, (int)p.persist, p.ts_initial, res[0], res[1], res[2],
           batch ? (long long)deal_initial_target(s.cus, W, chains) : 0LL, deal[0], deal[1], deal[2]);
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_plan_")
    src, exe = os.path.join(d, "plan_driver.cpp"), os.path.join(d, "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])
    yield exe
    shutil.rmtree(d, ignore_errors=True)


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("MHX_")}


def test_launch_plan_matches_the_recorded_rules(driver):
    with open(CASES) as f:
        rows = list(csv.DictReader(f))
    assert 1000 <= len(rows) <= 5000
    in_cols = [c for c in rows[0] if c not in OUT_COLS]
    feed = "".join(",".join(r[c] for c in in_cols) + "\n" for r in rows)
    out = subprocess.run([driver], input=feed, capture_output=True, text=True, env=clean_env(), check=True)
    got = out.stdout.strip().split("\n")
    assert len(got) == len(rows)
    bad = []
    for r, g in zip(rows, got):
        want = ",".join(r[c] for c in OUT_COLS)
        if g != want:
            bad.append("%s: want %s got %s" % (",".join(r[c] for c in in_cols), want, g))
    assert not bad, "%d of %d rows differ, first: %s" % (len(bad), len(rows), bad[:5])
    # the table holds every form: batch kernels, per-chain and tile-sliced split, each persistent or not
    forms = {(r["tsplit"], r["split_slices"] != "0", r["persist"]) for r in rows}
    assert forms >= {("0", False, "0"), ("0", True, "0"), ("0", True, "1"), ("1", True, "0"), ("1", True, "1")}


def knobs(driver, env):
    e = clean_env()
    e.update(env)
    out = subprocess.run([driver, "knobs"], capture_output=True, text=True, env=e, check=True).stdout.split()
    names = ["family_wpg", "split_set", "split", "tsplit_set", "tsplit", "no_persist", "persist_ts",
             "persist_fill", "no_resident_slices", "no_window_grids", "no_tile_skip", "no_recognise", "no_yw",
             "no_deal", "force_generic", "no_rtc_specialise", "early_reject", "no_compact", "compact_always",
             "no_graph"]
    return dict(zip(names, (int(v) for v in out)))


FLAGS = {"MHX_NO_PERSIST": "no_persist", "MHX_NO_RESIDENT_SLICES": "no_resident_slices",
         "MHX_NO_WINDOW_GRIDS": "no_window_grids", "MHX_NO_TILE_SKIP": "no_tile_skip",
         "MHX_NO_RECOGNISE": "no_recognise", "MHX_NO_YW": "no_yw", "MHX_NO_DEAL": "no_deal",
         "MHX_FORCE_GENERIC": "force_generic", "MHX_NO_RTC_SPECIALISE": "no_rtc_specialise",
         "MHX_EARLY_REJECT": "early_reject", "MHX_NO_COMPACT": "no_compact",
         "MHX_COMPACT_ALWAYS": "compact_always", "MHX_NO_GRAPH": "no_graph"}


def test_read_knobs_parses_the_environment(driver):
    base = knobs(driver, {})
    assert base == dict(family_wpg=0, split_set=0, split=0, tsplit_set=0, tsplit=0, no_persist=0, persist_ts=-1,
                        persist_fill=100, **{v: 0 for v in FLAGS.values() if v != "no_persist"})
    # flags: on when set and atoi() != 0
    for var, field in FLAGS.items():
        for val, on in (("0", 0), ("1", 1), ("", 0), ("abc", 0), ("7", 1)):
            k = knobs(driver, {var: val})
            assert k[field] == on and {n: v for n, v in k.items() if n != field} == \
                {n: v for n, v in base.items() if n != field}, (var, val)
    # MHX_SPLIT / MHX_TSPLIT: set and value apart (empty or not a number: set, 0)
    for val, num in (("0", 0), ("1", 1), ("", 0), ("abc", 0), ("12", 12)):
        k = knobs(driver, {"MHX_SPLIT": val, "MHX_TSPLIT": val})
        assert (k["split_set"], k["split"], k["tsplit_set"], k["tsplit"]) == (1, num, 1, num), val
    # MHX_PERSIST_TS: unset -1, else 0 or 1
    for val, v in (("0", 0), ("1", 1), ("", 0), ("abc", 0), ("3", 1)):
        assert knobs(driver, {"MHX_PERSIST_TS": val})["persist_ts"] == v, val
    # MHX_PERSIST_FILL clamped to 10..100; MHX_FAMILY_WPG only 8 and 16
    assert [knobs(driver, {"MHX_PERSIST_FILL": v})["persist_fill"] for v in ("5", "500", "55", "")] == [10, 100, 55, 10]
    assert [knobs(driver, {"MHX_FAMILY_WPG": v})["family_wpg"] for v in ("12", "8", "16", "", "abc")] == [0, 8, 16, 0, 0]
