"""CPU checks of what finalising a problem decides (csrc/mhx_finalize.hpp): the x ranges and grids
of a dataset's 2048-point windows against the rule restated in numpy, bit for bit; the LDS layout
of a dataset per walker against the arithmetic of DESIGN.md section 3.3; and the kernel choice and
its name over tests/golden/kernel_choice_cases.csv, whose expected names and refusals were recorded
on the MI355X from the engine before these rules moved into the header.  A small driver compiled
against the header with the plain host compiler does the computing."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import kernel_choice_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
WP = 2048  # kPadPoints

# stdin, one request per line:
#   W n x_0 .. x_(n-1)      (hex floats)  -> whole-dataset 64 h, windows, then lo / hi / table rows
#   P K wpg no_lds {planes n sigma_kind}  -> resident, then K rows of the layout
#   C / F chains pooled knob x 7 fn0 fn1  -> code|name or message|rtc fallback required|K x kind,wgrid,er,tgh,slot,prior
#                                            (F: after the fall-back to the generic kernels, note "no hiprtc")
DRIVER = r'''
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include "mhx_finalize.hpp"
using namespace mhx;
static void put(const std::vector<double>& v) {
  for (double d : v) { uint64_t b; memcpy(&b, &d, 8); printf(" %016" PRIx64, b); }
  printf("\n");
}
static std::vector<double> padded(const std::vector<double>& x) {  // as mhx_set_dataset pads
  std::vector<double> hx(windows_of(x.size()) * kPadPoints, x.empty() ? 0.0 : x.back());
  std::copy(x.begin(), x.end(), hx.begin());
  return hx;
}
static std::vector<double> x_of(const std::string& kind) {
  const size_t n = kind == "piecewise" ? 2 * 2048 + 5 : kind == "long" ? 4 * 2048 + 5 : 64;
  std::vector<double> x(n);
  for (size_t i = 0; i < n; ++i) {
    const double t = (double)i;
    x[i] = kind == "piecewise" ? (i < 2048 ? t * 0.01 : 20.48 + (t - 2048) * 0.02)
           : kind == "irregular" ? t * 0.25 + 0.01 * (double)((i * i) % 7)
           : kind == "grid" ? t * 0.25 : t * 0.002;
  }
  return x;
}
int main() {
  static const char* knob[7] = {"MHX_FORCE_GENERIC", "MHX_NO_RTC_SPECIALISE", "MHX_EARLY_REJECT", "MHX_NO_RECOGNISE",
                                "MHX_NO_WINDOW_GRIDS", "MHX_PLANES_NO_LDS", "MHX_FAMILY_WPG"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "W") {
      size_t n;
      in >> n;
      std::vector<double> x(n), lo, hi, gh;
      for (double& v : x) { std::string s; in >> s; v = strtod(s.c_str(), nullptr); }
      const std::vector<double> hx = padded(x);
      window_ranges(hx.data(), n, &lo, &hi);
      const bool any = window_grids(hx.data(), n, &gh);
      put({64.0 * grid_step(x.data(), n)});
      printf("%zu %d\n", windows_of(n), (int)any);
      put(lo), put(hi), put(gh);
    } else if (what == "P") {
      int K, wpg, no_lds;
      in >> K >> wpg >> no_lds;
      PlanesFn fn[MHX_MAX_FUNCTIONS];
      PlanesLayout pl[MHX_MAX_FUNCTIONS];
      for (int k = 0; k < K; ++k) { int p; in >> p >> fn[k].n >> fn[k].sigma_kind; fn[k].planes = p != 0; }
      EngineKnobs kn;
      kn.planes_no_lds = no_lds != 0;
      printf("%d\n", (int)planes_layout(fn, K, wpg, kn, pl));
      for (int k = 0; k < K; ++k)
        printf("%d %d %d %d %d %d\n", pl[k].resident, pl[k].bit, pl[k].off_x, pl[k].off_w, pl[k].off_rows, pl[k].row_stride);
    } else {
      long long chains;
      int pooled;
      in >> chains >> pooled;
      for (int i = 0; i < 7; ++i) {
        std::string v;
        in >> v;
        if (v == "-") unsetenv(knob[i]); else setenv(knob[i], v.c_str(), 1);
      }
      const EngineKnobs kn = read_knobs();
      ProblemDesc P{};
      FnInput fi[MHX_MAX_FUNCTIONS];
      PlanesFn pf[MHX_MAX_FUNCTIONS];
      UserExpr ux[MHX_MAX_FUNCTIONS];
      RecognisedModel rm[MHX_MAX_FUNCTIONS];
      const std::string lx[MHX_MAX_FUNCTIONS];
      bool has_tgh[MHX_MAX_FUNCTIONS] = {};
      ProblemShape sh;
      std::string tok;
      int first = 0;
      while (in >> tok && tok != "-") {
        char model[16], lik[16], form[16], data[32], xk[16];
        int s0, s1, n_idx, prior;
        if (sscanf(tok.c_str(), "%15[^/]/%d/%d/%d/%15[^/]/%15[^/]/%d/%31[^/]/%15s", model, &s0, &s1, &n_idx, lik, form,
                   &prior, data, xk) != 9)
          return 1;
        const int k = P.K++;
        FnDesc& f = P.fn[k];
        const int m = !strcmp(model, "poly") ? MHX_MODEL_POLY : !strcmp(model, "gauss") ? MHX_MODEL_GAUSS_PEAKS
                                                                                          : MHX_MODEL_LORENTZ_PEAKS;
        const bool is_expr = !strncmp(form, "expr", 4) || !strcmp(form, "rexpr");
        f.model = is_expr ? MHX_MODEL_EXPR : m;
        f.shape[0] = is_expr ? 0 : s0, f.shape[1] = is_expr ? 0 : s1;
        f.n_idx = n_idx;
        for (int j = 0; j < n_idx; ++j) f.idx[j] = first + j, ux[k].index.push_back(first + j);
        first += n_idx;
        f.lik = !strcmp(lik, "normal") ? MHX_LIK_NORMAL : !strcmp(lik, "cutoff") ? MHX_LIK_NORMAL_CUTOFF
                : !strcmp(lik, "poisson") ? MHX_LIK_POISSON : MHX_LIK_EXPR;
        if (is_expr) ux[k].expr = "text", ux[k].xcols = !strcmp(form, "expr2") ? 2 : 1;
        if (!strcmp(form, "rexpr")) {
          rm[k].model = m, rm[k].shape[0] = s0, rm[k].shape[1] = s1;
          for (int j = 0; j < n_idx; ++j) rm[k].order.push_back(j);
        }
        fi[k].fn_set = strcmp(form, "unset") != 0;
        fi[k].data_set = strcmp(data, "unset") != 0;
        fi[k].planes = !strncmp(data, "planes-", 7);
        fi[k].expr = &ux[k], fi[k].recog = &rm[k];
        fi[k].prior_expr = prior != 0;
        fi[k].lik_expr = !strcmp(lik, "expr");
        f.n_xcols = !strcmp(data, "cols2") ? 2 : 1;
        if (fi[k].data_set) {  // what mhx_set_dataset leaves, then the window table as finalisation gates it
          const std::vector<double> x = x_of(xk), hx = padded(x);
          std::vector<double> gh;
          f.n = (int64_t)x.size();
          f.grid_H = 64.0 * grid_step(x.data(), x.size());
          has_tgh[k] = f.grid_H == 0.0 && !kn.no_window_grids && window_grids(hx.data(), x.size(), &gh);
        }
        const char* sk = fi[k].planes ? data + 7 : "none";
        pf[k] = PlanesFn{fi[k].planes, f.n, !strcmp(sk, "shared") ? MHX_SIGMA_SHARED : !strcmp(sk, "chain") ? MHX_SIGMA_PER_CHAIN
                                            : !strcmp(sk, "point") ? MHX_SIGMA_PER_POINT : MHX_SIGMA_NONE};
        sh.longest = std::max<int64_t>(sh.longest, f.n);
        sh.planes = sh.planes || fi[k].planes;
      }
      P.d = first;
      Refusal r = validate_problem(P, fi, pooled != 0);
      if (!r) r = resolve_functions(P, fi, !kn.no_recognise);
      if (r) {
        printf("%d|%s|\n", r.code, r.msg.c_str());
        continue;
      }
      sh.chains = chains;
      PlanesLayout pl[MHX_MAX_FUNCTIONS];
      const int wpg = choose_family(sh, kn);
      const bool res = sh.planes && planes_layout(pf, P.K, wpg, kn, pl);
      KernelChoice c = choose_kernels(P, fi, has_tgh, pooled != 0, kn);
      const int was_rtc = c.rtc;
      if (what == "F") fall_back_to_generic(&c);
      apply_choice(c, &P);
      printf("0|%s|%d %d %d", kernel_name(c, wpg, res, LaunchPlan{}, what == "F" ? "no hiprtc" : "").c_str(), was_rtc,
             (int)c.builtin_fallback, (int)c.compile_required);
      const std::vector<UserExpr> models = program_models(c, ux, lx);
      for (int k = 0; k < P.K; ++k) {
        const FnChoice& fc = c.fn[k];
        if (P.fn[k].user_slot != fc.user_slot || P.fn[k].prior_slot != fc.prior_slot) return 2;
        if (fc.user_slot >= 0 && (models[fc.user_slot].builtin != fc.type || models[fc.user_slot].wgrid != fc.wgrid)) return 3;
        printf("|%d,%d,%d,%d,%d,%d", (int)fc.kind, (int)fc.wgrid, (int)fc.early_reject, (int)fc.keep_tgh, fc.user_slot,
               fc.prior_slot);
      }
      printf("\n");
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tempfile.mkdtemp(prefix="mhx_finalize_")
    src, exe = os.path.join(d, "finalize_driver.cpp"), os.path.join(d, "finalize_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    # (-ffp-contract=off: x_0 + i h rounds twice, as the library is built)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", exe, src])
    yield exe
    shutil.rmtree(d, ignore_errors=True)


def ask(driver, lines):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MHX_")}
    out = subprocess.run([driver], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, env=env,
                         check=True)
    return out.stdout.split("\n")


def bits(v):
    return [struct.pack("<d", float(x)).hex() for x in np.atleast_1d(v)]


def from_bits(words):
    return [struct.pack("<Q", int(w, 16)).hex() for w in words]


# ---- windows: the rule, stated here in numpy

def fits(xw, h):
    if h == 0.0 or not np.isfinite(h):
        return False
    tol = 8.0 * 2.0 ** -52 * max(abs(xw[0]), abs(xw[-1]))
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(xw - (xw[0] + np.arange(len(xw), dtype=np.float64) * h)) <= tol))


def grid_of(xw, h_prev=0.0):
    """the step of the grid the points are (h_prev tried first, then their own), or 0"""
    if len(xw) < 2 or not (np.isfinite(xw[0]) and np.isfinite(xw[-1])):
        return 0.0
    if fits(xw, h_prev):
        return h_prev
    h = (xw[-1] - xw[0]) / np.float64(len(xw) - 1)
    return h if fits(xw, h) else 0.0


def windows_expected(x):
    n = len(x)
    nw = max(-(-n // WP), 1)
    hx = np.full(nw * WP, x[-1] if n else 0.0)
    hx[:n] = x
    lo, hi, gh, h_prev = [], [], [], 0.0
    for t in range(nw):
        w = hx[t * WP:(t + 1) * WP]
        ok = bool(np.isfinite(w).all())
        lo.append(w.min() if ok else -np.inf)
        hi.append(w.max() if ok else np.inf)
        h = grid_of(x[t * WP:min((t + 1) * WP, n)], h_prev)
        gh.append(64.0 * h)
        if h != 0.0:
            h_prev = h
    return 64.0 * grid_of(x), nw, h_prev != 0.0, lo, hi, gh


def window_cases():
    rng = np.random.default_rng(5)
    i3 = np.arange(3 * WP, dtype=np.float64)
    c = {"n1": np.array([3.5]), "n2": np.array([1.0, 1.5]), "n2_equal": np.array([2.0, 2.0])}
    for n in (WP - 1, WP, WP + 1):
        c["grid_%d" % n] = 0.5 + 0.125 * np.arange(n)
        c["ragged_%d" % n] = np.sort(rng.uniform(-3, 7, n))
    c["three_windows_ragged"] = np.cumsum(rng.uniform(0.01, 0.02, 2 * WP + 100)) - 20.0   # the pads repeat the last x
    bad = 0.25 * np.arange(2 * WP + 7)
    bad[WP + 5], bad[WP + 900] = np.nan, np.inf
    c["nan_and_inf_in_window_1"] = bad
    c["constant"] = np.full(WP + 10, 4.25)
    c["one_grid_three_windows"] = 0.25 * i3
    c["one_grid_offset_1e6"] = 1e6 + i3 * 0.1             # the last window's own step is not the carried one
    c["descending"] = 10.0 - 0.01 * i3
    c["two_scans"] = np.concatenate([0.01 * np.arange(3000), 40.0 + 0.03 * np.arange(3000)])
    jit = 0.5 * i3
    jit[WP:2 * WP] += rng.uniform(0, 0.1, WP)
    c["jittered_between_grids"] = jit
    c["last_window_of_one"] = 0.125 * np.arange(WP + 1)
    c["nothing_fits"] = np.sort(rng.uniform(0, 100, 5000))
    c["unsorted_ends_non_finite"] = np.concatenate([[np.inf], rng.uniform(0, 1, 50), [np.nan]])
    return c


def test_window_ranges_and_grids_bit_for_bit(driver):
    cases = window_cases()
    out = ask(driver, ["W %d %s" % (len(x), " ".join(float(v).hex() for v in x)) for x in cases.values()])
    seen = set()
    for j, (name, x) in enumerate(cases.items()):
        H, nw, any_, lo, hi, gh = windows_expected(x)
        got = out[5 * j:5 * j + 5]
        assert from_bits(got[0].split()) == bits(H), name
        assert got[1].split() == [str(nw), str(int(any_))], name
        for g, want, what in zip(got[2:], (lo, hi, gh), ("lo", "hi", "grid")):
            assert from_bits(g.split()) == bits(want), (name, what)
        seen.add((nw, any_, H != 0.0))
    # whole grids, piecewise ones, none at all; one window and several
    assert seen >= {(1, True, True), (1, False, False), (3, True, True), (3, True, False), (3, False, False)}
    # what the cases are there for
    e = {name: windows_expected(x) for name, x in cases.items()}
    assert len(set(bits(e["one_grid_three_windows"][5]))) == 1 and len(set(bits(e["one_grid_offset_1e6"][5]))) == 1
    x = cases["one_grid_offset_1e6"]
    own = [(x[(t + 1) * WP - 1] - x[t * WP]) / (WP - 1.0) for t in range(3)]
    assert any(bits(64.0 * h) != bits(e["one_grid_offset_1e6"][5][0]) for h in own[1:])
    assert [g != 0.0 for g in e["two_scans"][5]] == [True, False, True] and e["two_scans"][5][0] != e["two_scans"][5][2]
    assert [g != 0.0 for g in e["jittered_between_grids"][5]] == [True, False, True]
    assert bits(e["jittered_between_grids"][5][0]) == bits(e["jittered_between_grids"][5][2])
    assert [g != 0.0 for g in e["last_window_of_one"][5]] == [True, False]
    assert e["nan_and_inf_in_window_1"][3][1] == -np.inf and e["nan_and_inf_in_window_1"][4][1] == np.inf
    assert np.isfinite(e["nan_and_inf_in_window_1"][3][0]) and e["three_windows_ragged"][3][2] <= cases["three_windows_ragged"][-1]
    assert not e["nothing_fits"][2] and not e["constant"][2] and not e["n1"][2] and e["n2"][2]


# ---- a dataset per walker: DESIGN.md section 3.3, "Two forms, one rule"

def planes_expected(fns, wpg, no_lds):
    """fns: (planes, n, sigma_kind); -> resident, [(resident, bit, off_x, off_w, off_rows, row_stride)]"""
    pad = lambda n: max(-(-n // 128), 1) * 128
    shared = lambda n, kind: pad(n) * (2 if kind == 1 else 1)      # x, and a shared 1/sigma
    per_wave = lambda n, kind: pad(n) * (2 if kind == 3 else 1)    # y/sigma, and a 1/sigma plane
    capacity = 2 * 4 * (128 * wpg)                                # the tile buffers: 2 x 4 arrays of a tile
    need = sum(shared(n, k) + wpg * per_wave(n, k) for p, n, k in fns if p)
    resident = (not no_lds) and all(p for p, _, _ in fns) and need <= capacity
    rows, off = [], 0
    for j, (p, n, k) in enumerate(fns):
        if not p:
            rows.append((0, 0, 0, 0, 0, 0))
        elif not resident:
            rows.append((0, 1 << j, 0, 0, 0, 0))
        else:
            rows.append((1, 1 << j, off, off + pad(n), off + shared(n, k), per_wave(n, k)))
            off += shared(n, k) + wpg * per_wave(n, k)
    return resident, rows


def test_planes_layout(driver):
    cases = []
    for wpg in (8, 16):
        for no_lds in (0, 1):
            for kind in range(4):
                for n in (64, 384, 385, 896, 897):
                    cases.append(([(1, n, kind)], wpg, no_lds))
                cases.append(([(1, 100, kind), (1, 200, 3 - kind)], wpg, no_lds))
                cases.append(([(1, 64, kind), (1, 64, 2), (1, 130, 0)], wpg, no_lds))      # three of K = 3
                cases.append(([(0, 64, 0), (1, 64, kind), (1, 64, 2)], wpg, no_lds))       # two of K = 3
                cases.append(([(0, 5000, 0), (1, 64, kind), (0, 64, 0)], wpg, no_lds))     # one of K = 3
    out = ask(driver, ["P %d %d %d %s" % (len(f), w, nl, " ".join("%d %d %d" % t for t in f)) for f, w, nl in cases])
    at, forms = 0, set()
    for fns, wpg, no_lds in cases:
        resident, rows = planes_expected(fns, wpg, no_lds)
        assert out[at] == str(int(resident)), (fns, wpg, no_lds)
        assert [tuple(int(v) for v in ln.split()) for ln in out[at + 1:at + 1 + len(fns)]] == rows, (fns, wpg, no_lds)
        at += 1 + len(fns)
        forms.add((resident, len(fns), sum(p for p, _, _ in fns)))
    assert forms >= {(True, 1, 1), (False, 1, 1), (True, 2, 2), (True, 3, 3), (False, 3, 2), (False, 3, 1)}
    # (section 3.3's figures: 896 points without a per-wave 1/sigma plane, 384 with one, in either family)
    for wpg in (8, 16):
        assert [planes_expected([(1, n, k)], wpg, 0)[0] for n, k in ((896, 2), (897, 2), (384, 3), (385, 3))] == \
            [True, False, True, False]


# ---- the kernel choice and its name

def choice_line(r, what="C"):
    return " ".join([what, r["chains"], str(int(r["adapt"] == "pooled"))] + [r[k] for k in kc.KNOBS] + [r["fn0"], r["fn1"], "-"])


def slots_of(name):
    """what a name says of its functions: (kind, wgrid, early reject) each"""
    m = re.search(r"/rtc\[(.*)\]", name)
    if not m:
        return None
    out = []
    for ent in re.split(r", (?![^<]*>)", m.group(1)):
        t = ent.rsplit(":", 1)[0]
        kind = 1 if t == "expr" else (3 if "+planes(" in ent else 0) if t == "generic" else 2
        out.append((kind, int("+wgrid" in t), int("+early-reject" in t)))
    return out


def test_kernel_choice_matches_the_recorded_engine(driver):
    rows = kc.rows()
    assert 35 <= len(rows) <= 60 and len({r["id"] for r in rows}) == len(rows)
    out = ask(driver, [choice_line(r) for r in rows])
    names = set()
    for r, got in zip(rows, out):
        code, text, *rest = got.split("|")
        assert int(code) == int(r["code"]), (r["id"], got)
        if int(code) != 0:
            assert text == r["expected"], r["id"]
            continue
        recorded = re.sub(r"( persistent)? t?split x\d+$", "", r["expected"])
        assert text == recorded, r["id"]
        names.add(recorded)
        rtc, fallback, required = (int(v) for v in rest[0].split())
        fns = [tuple(int(v) for v in f.split(",")) for f in rest[1:]]
        said = slots_of(recorded)
        assert (said is not None) == bool(rtc), r["id"]
        if said is None:
            assert all(f[:3] == (0, 0, 0) and f[4:] == (-1, -1) for f in fns) and not fallback, r["id"]
            continue
        assert [f[:3] for f in fns] == said, r["id"]
        assert all(f[3] == f[1] for f in fns), r["id"]                   # the table survives where a kernel follows it
        assert [f[4] for f in fns if f[0]] == list(range(sum(1 for f in fns if f[0]))), r["id"]
        assert fallback == int(any(f[0] == 0 for f in fns)), r["id"]
        assert required == int(any(f[0] in (1, 3) or "+planes(" in recorded or fn["prior"] for f, fn in zip(fns, r["fns"]))), r["id"]
    # every branch is among the rows
    for piece in ("/gauss22_normal", "/poly2_normal", "/gauss15_poisson", "w16/", "/generic", "rtc[PeaksModel<2, 3, false>:normal]",
                  "+wgrid:", "+early-reject:", "+wgrid+early-reject:", "rtc[expr:normal]", "rtc[expr:expr]",
                  "rtc[expr:normal, generic:normal]", "+planes(resident)", "+planes(streamed)",
                  "rtc[generic:normal+planes(", "rtc[PeaksModel<2, 2, true>:normal]"):
        assert any(piece in n for n in names), piece
    refused = {(int(r["code"]), r["expected"]) for r in rows if int(r["code"]) != 0}
    assert len(refused) >= 7, refused


def test_fall_back_to_the_generic_kernels_when_the_compile_fails(driver):
    """enumerated models only: the generic kernels serve, the name says why, the slots are given back -
    and the per-window grid table stays, as it always has"""
    rows = {r["id"]: r for r in kc.rows()}
    out = ask(driver, [choice_line(rows[i], "F") for i in ("builtin_gauss23", "wgrid_gauss22", "early_reject_gauss22")])
    for got, tgh in zip(out, (0, 1, 0)):
        code, text, flags, fn = got.split("|")
        assert (code, text) == ("0", "w8/generic [not specialised: no hiprtc]")
        assert flags.split() == ["1", "0", "0"]                           # was a run-time program, not a required one
        assert [int(v) for v in fn.split(",")][3:] == [tgh, -1, -1]
