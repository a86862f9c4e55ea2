"""The case tables of tests/split_cases.py, checked on the CPU: the pair / slot / slice arithmetic
restated there is the kernels' and the planner's, every case reaches the place its comment names
(empty slots, the ragged last chunk, empty slices, resident windows or not, a slice of more than 64
windows, windows on another grid), and the faithful oracle lies within the stated tolerance
1e-12 * sum |term| of the high-precision reference at every short shape and vector the device
tests use - the reference alone must stay inside the cap.

A change of kPadPoints, of the slot rule or of build_ts_table fails here, loudly, instead of
leaving tests/test_gpu_split_values.py on shapes that no longer reach anything."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import problems as pb
import split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_and_rules_are_the_sources():
    types = source("mhx_types.hpp")
    assert re.search(r"constexpr int kWave = (\d+);", types).group(1) == str(sc.KWAVE)
    assert "constexpr int tile_points_of(int waves_per_group) { return 2 * kWave * waves_per_group; }" in types
    assert "constexpr int kPadPoints = tile_points_of(16);" in types
    assert sc.tile_points(16) == sc.WINDOW and sc.tile_points(8) * 2 == sc.WINDOW
    # the slot rule of the per-chain form, in k_split_sweep_body and in k_persist_body alike
    kernels = source("mhx_kernels.hpp")
    for line in ("const int64_t pairs = (f.n + 2 * kWave - 1) / (2 * kWave);",
                 "const int64_t per = (pairs + S.split_slots - 1) / S.split_slots;",
                 "const int64_t b0 = (int64_t)slot * per, b1 = b0 + per < pairs ? b0 + per : pairs;",
                 "if (b0 < b1) v = Spec::loglik_part(f, pf, b0 * 2 * kWave, b1 * 2 * kWave, sl.scr[w]);"):
        assert kernels.count(line) == 2, "the slot rule changed (restate it in split_cases.chain_slots): " + line
    # ... and the slice table of the tile-sliced form
    engine = source("mhx_engine.cpp")
    for line in ("const int64_t nwin = (f.n + kPadPoints - 1) / kPadPoints;",
                 "const int64_t per = (nwin + ts - 1) / ts;",
                 "const int64_t off = (int64_t)sl * per * kPadPoints;",
                 "g.n = std::min<int64_t>(per * kPadPoints, f.n - off);",
                 "bool resident = e->persist && e->P.K == 1 && kPadPoints <= 2 * e->fam->tile_points;",
                 "resident = resident && per == 1;"):
        assert engine.count(line) == 1, "build_ts_table changed (restate it in split_cases.ts_table): " + line
    assert "e->S.split_slots = e->tsplit ? e->split_slices : e->split_slices * e->fam->waves_per_group;" in engine


# longest, chains, then the knobs ("-": unset) -> tsplit, split_slices, persist of plan_modes for a
# problem whose kernels have the split forms, on 256 CUs that hold two persistent workgroups each
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mhx_plan.hpp"
using namespace mhx;
int main() {
  static const char* names[5] = {"MHX_FAMILY_WPG", "MHX_SPLIT", "MHX_TSPLIT", "MHX_NO_PERSIST", "MHX_PERSIST_TS"};
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    long long longest, chains, K, d;
    char env[5][32];
    if (sscanf(line, "%lld,%lld,%lld,%lld,%31[^,],%31[^,],%31[^,],%31[^,],%31[^,\n]", &longest, &chains, &K, &d,
               env[0], env[1], env[2], env[3], env[4]) != 9)
      return 1;
    for (int i = 0; i < 5; ++i) {
      if (!strcmp(env[i], "-")) unsetenv(names[i]);
      else setenv(names[i], env[i], 1);
    }
    const EngineKnobs kn = read_knobs();
    ProblemShape s;
    s.longest = longest;
    s.nwin = ceil_div(longest, kPadPoints);
    s.K = (int)K;
    s.d = (int)d;
    s.chains = chains;
    s.cus = 256;
    s.waves_per_group = choose_family(s, kn);
    s.tile_points = tile_points_of(s.waves_per_group);
    s.per_cu = 2;
    s.per_cu_ts = 2;
    s.capable = true;
    const LaunchPlan p = plan_modes(s, kn);
    printf("%d,%d,%d,%d\n", s.waves_per_group, (int)p.tsplit, p.split_slices, (int)p.persist);
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def planner():
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++: the planner's rules cannot be compared"
    d = tempfile.mkdtemp(prefix="mhx_split_cases_")
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, src])

    def plan(rows):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MHX_")}
        feed = "".join(",".join(str(v) for v in r) + "\n" for r in rows)
        out = subprocess.run([exe], input=feed, capture_output=True, text=True, env=env, check=True)
        return [tuple(int(v) for v in line.split(",")) for line in out.stdout.strip().split("\n")]

    yield plan
    shutil.rmtree(d, ignore_errors=True)


def test_forms_and_slice_counts_are_the_planners(planner):
    """every case under every form's knobs: the planner gives the form, the family and the slice
    count the tables state (what the device tests then assert through kernel_name())"""
    rows, want = [], []
    for c in sc.PER_CHAIN_CASES:
        s = sc.problem(c.kind, c.lens)
        assert sc.forced_split_slices(max(c.lens), c.k) == c.slices, c.id
        for f in sc.per_chain_forms(c.k):
            rows.append((max(c.lens), c.chains, s.K, s.d, "-", f.env.get("MHX_SPLIT", "-"), "-",
                         f.env.get("MHX_NO_PERSIST", "-"), "-"))
            want.append((8, 0, c.slices, int(f.persistent)))
    for c in sc.TILE_SLICED_CASES:
        s = sc.problem(c.kind, c.lens)
        assert sc.forced_ts_slices(max(c.lens), c.k) == c.slices, c.id
        for wpg, chains in ((8, 9), (16, 17)):
            for f in sc.tile_sliced_forms(c.k, wpg, extras=False):
                rows.append((max(c.lens), chains, s.K, s.d, wpg, "-", c.k, "-", f.env["MHX_PERSIST_TS"]))
                want.append((wpg, 1, c.slices, int(f.persistent)))
    got = planner(rows)
    bad = [(r, w, g) for r, w, g in zip(rows, want, got) if w != g]
    assert not bad, bad[:5]


@pytest.mark.parametrize("case", sc.PER_CHAIN_CASES, ids=[c.id for c in sc.PER_CHAIN_CASES])
def test_per_chain_case_reaches_its_place(case):
    slots = case.slices * 8
    assert len(case.lens) == len(case.per) == len(case.used) == len(case.last) == len(case.tail)
    for n, per, used, last, tail in zip(case.lens, case.per, case.used, case.last, case.tail):
        tab = sc.chain_slots(n, case.slices)
        assert len(tab) == slots
        pairs = sc.ceil_div(n, sc.PAIR)
        assert sc.ceil_div(pairs, slots) == per
        full = [s for s, (b0, b1) in enumerate(tab) if b0 < b1]
        assert full == list(range(used)), (case.id, full)          # the slots past `used` are empty
        assert tab[used - 1][1] - tab[used - 1][0] == last
        assert sum(b1 - b0 for b0, b1 in tab) == pairs              # every pair once
        assert n - (pairs - 1) * sc.PAIR == tail
        # the chunk reads [b0, b1) * 128: past n by 128 - tail points, inside the padded window
        assert tab[used - 1][1] * sc.PAIR - n == sc.PAIR - tail < sc.WINDOW
    th = sc.case_vectors(case)
    assert th.shape == (case.chains, sc.problem(case.kind, case.lens).d)
    assert case.chains in (1, 3, 7)


def test_per_chain_cases_cover_what_the_issue_names():
    by = {c.id: c for c in sc.PER_CHAIN_CASES}
    # one pair, then two, all but the first slots empty; eight pairs, one per slot; nine pairs:
    # slots 5 to 7 empty, slot 4 half full; 24 slots, the last four beyond the data, a ragged chunk
    assert [by["grid-%d" % n].used[0] for n in (1, 127, 128, 129, 1024, 1025)] == [1, 1, 1, 2, 8, 5]
    c = by["grid-1025"]
    assert (c.per[0], c.used[0], c.last[0]) == (2, 5, 1)
    c = by["grid-12289-x3"]
    assert (c.slices * 8, c.per[0], c.used[0], c.last[0]) == (24, 5, 20, 2)
    assert by["grid-12289-x99"].slices == 3
    c = by["pvoigt-1+12289"]
    assert c.used == (1, 20) and sc.problem(c.kind, c.lens).K == 2
    assert {c.chains for c in sc.PER_CHAIN_CASES} == {1, 3, 7}
    assert {c.kind for c in sc.PER_CHAIN_CASES} == {"grid", "jitter", "cutoff", "poisson", "lorentz", "pvoigt"}
    # every odd vector is used somewhere in the per-chain form, per kind that has it
    for kind in ("grid", "cutoff", "poisson"):
        rows = set()
        for c in sc.PER_CHAIN_CASES:
            if c.kind == kind:
                rows |= set(c.rows if c.rows is not None else range(c.chains))
        assert rows >= set(sc.ODD_ROWS[:len(sc.ODD[kind])]), (kind, rows)


@pytest.mark.parametrize("case", sc.TILE_SLICED_CASES, ids=[c.id for c in sc.TILE_SLICED_CASES])
def test_tile_sliced_case_reaches_its_place(case):
    assert len(case.lens) == len(case.n)
    for n, want in zip(case.lens, case.n):
        per, tab = sc.ts_table(n, case.slices)
        assert tuple(m for _, m in tab) == want, (case.id, tab)
        assert sum(m for _, m in tab) == n
        for off, m in tab:
            assert off % sc.WINDOW == 0 and (m == 0 or off + m <= n)
    for wpg in (8, 16):
        assert sc.ts_resident(case.lens, case.slices, wpg) == case.resident, case.id
    assert case.vectors in (9, 17) and len(sc.case_vectors(case)) == case.vectors
    if case.sharp:
        assert case.kind == "grid" and len(case.lens) == 1 and case.ref == "hp"
    if case.ref == "hp":
        assert max(case.lens) <= 12289


def test_tile_sliced_cases_cover_what_the_issue_names():
    by = {c.id: c for c in sc.TILE_SLICED_CASES}
    assert by["grid-2049-ts2"].n == ((2048, 1),)                       # the second slice: one point
    assert by["grid-4096-ts2"].resident and by["grid-4097-ts3"].resident
    assert not by["grid-4097-ts2"].resident and by["grid-4097-ts3"].n[0][-1] == 1
    assert by["grid-6144-ts7"].k == 7 and by["grid-6144-ts7"].slices == 3
    g = by["pvoigt-2049+9000-ts4"]
    assert g.n[0][2:] == (0, 0) and g.n[1][3] == 0 and sc.problem(g.kind, g.lens).K == 2   # empty slices
    long_ = by["grid-270336-ts2"]
    per, tab = sc.ts_table(long_.lens[0], long_.slices)
    assert per == 66 > 64 and tab[1][0] == 66 * sc.WINDOW                # crosses its own 64th window
    assert {c.kind for c in sc.TILE_SLICED_CASES} == {"grid", "jitter", "cutoff", "poisson", "lorentz", "pvoigt",
                                                      "piecewise"}


def test_piecewise_slices_start_on_other_grids():
    """what the shifted tgh has to follow: the grid step of a slice's first window differs from
    window 0's - a window that is no grid at 12288 points; at 20480 points also windows on the
    steps 0.6 h and 1.7 h and the jittered window"""
    for c in sc.TILE_SLICED_CASES:
        if c.kind != "piecewise":
            continue
        x = sc.problem(c.kind, c.lens).data[0][0]
        steps = sc.window_steps(x)
        per, tab = sc.ts_table(c.lens[0], c.slices)
        first = [steps[off // sc.WINDOW] for off, m in tab if m]
        assert steps[0] != 0.0 and any(h != steps[0] for h in first[1:]), (c.id, steps)
        if c.lens[0] == 12288:
            assert [h != 0.0 for h in steps] == [True, True, False, False, False, True]
        else:
            h0 = steps[0]
            rel = [round(h / h0, 6) for h in steps]
            assert rel == [1.0, 0.0, 1.0, 0.0, 0.6, 0.6, 0.0, 1.7, 0.0, 1.0], rel
            assert any(h not in (0.0, h0) for h in first), (c.id, first)   # a slice starts on another step
    # ... and the jittered problem has no grid anywhere, the plain one is one grid
    assert not any(sc.window_steps(sc.problem("jitter", (4096,)).data[0][0]))
    assert len(set(sc.window_steps(sc.problem("grid", (4096,)).data[0][0]))) == 1


def test_vectors_are_what_the_tables_say(orc):
    for kind, lens in (("grid", (1025,)), ("cutoff", (1025,)), ("poisson", (1025,)), ("pvoigt", (1, 12289)),
                       ("lorentz", (1025,)), ("jitter", (1025,))):
        s = sc.problem(kind, lens)
        assert all(b is None for b in s.bounds)
        th = sc.all_vectors(kind, lens)
        assert th.shape == (17, s.d) and np.array_equal(th[0], s.theta_star)
        op = s.oracle(orc)
        for row, t in enumerate(th):
            finite = sc.rates_positive(s, t)
            assert np.isfinite(op.logpost(t)) == finite, (kind, row)
            assert finite == (not (kind == "poisson" and row == 6)), (kind, row)
    # the cutoff's own vector has terms on both sides of the clamp
    s = sc.problem("cutoff", (1025,))
    x, y, sig, _ = s.data[0]
    r = (y - pb.model_eval_np(pb.GAUSS, (2, 2), sc.all_vectors("cutoff", (1025,))[6], x)) / sig
    term = -0.5 * r * r - np.log(sig) - 0.5 * np.log(2 * np.pi)
    assert 50 < int((term < -5000).sum()) < len(x) - 50
    # the prior cases: 0, 1 and 3 bounds violated, by at most 0.1
    s = sc.problem("bounded", (4097,))
    twin = sc.problem("grid", (4097,))
    assert all(np.array_equal(a, b) for a, b in zip(s.data[0][:3], twin.data[0][:3]))
    idx, lo, hi = s.bounds[0]
    for t, want in zip(sc.prior_vectors(s), (0, 1, 3)):
        assert sc.violated(s, t) == want
        assert np.maximum(np.maximum(lo - t, t - hi), 0.0).max() <= 0.1


def test_reordering_depths():
    """n = 4096 in two slices: batch 2 x 16 points of a lane per accumulator, acc0 + acc1, the
    butterfly's 6, the finishing fma: 40; a slice 16 + 1 + 6, then one slot addition, the
    butterfly's 6 and the finishing fma: 31 - together 71 * 2^-53 = 7.9e-15 of sum r^2 / 2"""
    assert sc.reorder_depths(4096, 2) == (40, 31)
    assert sc.reorder_depths(2048 * 132, 2) == (16 * 132 + 8, 16 * 66 + 7 + 1 + 7)
    assert sc.reorder_depths(6144, 3) == (56, 31)


HP_CASES = [c for c in sc.PER_CHAIN_CASES + sc.TILE_SLICED_CASES if getattr(c, "ref", "hp") == "hp"]


@pytest.mark.slow
@pytest.mark.parametrize("case", HP_CASES, ids=[("pc-" if isinstance(c, sc.PerChain) else "ts-") + c.id for c in HP_CASES])
def test_faithful_oracle_is_within_the_tolerance_of_the_high_precision_reference(orc, case):
    """at every short shape and vector of the device tests: |oracle - mpmath| <= 1e-12 sum |term|,
    both references' sum |term| equal to 1e-9, and non-finite exactly together"""
    s = sc.problem(case.kind, case.lens)
    op = s.oracle(orc)
    ref, scale = sc.references(case)
    worst = 0.0
    for t, r, sc_ in zip(sc.case_vectors(case), ref, scale):
        got = op.logpost(t)
        if not np.isfinite(r):
            assert not np.isfinite(got)
            continue
        assert abs(op.abs_terms(t) - sc_) <= 1e-9 * sc_
        assert abs(got - r) <= sc.REL * sc_, (case.id, got, r, sc_)
        worst = max(worst, abs(got - r) / (sc.REL * sc_))
    print("%s: oracle against mpmath, worst ratio to 1e-12 sum |term|: %.3g" % (case.id, worst))


def test_faithful_oracle_prior_cases(orc):
    """the prior cases' reference is the high-precision likelihood of the twin problem without
    bounds plus the oracle's prior: the oracle's own likelihood part within the tolerance of it"""
    s, twin = sc.problem("bounded", (4097,)), sc.problem("grid", (4097,))
    op = s.oracle(orc)
    for t in sc.prior_vectors(s):
        ll, scale = sc.hp_reference(twin, t)
        v, parts = op.logpost(t, parts=True)
        assert abs(parts[0] - ll) <= sc.REL * scale
        assert parts[1] <= 0.0 and (parts[1] < 0.0) == (sc.violated(s, t) > 0)
