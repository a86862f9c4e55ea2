// mhx_finalize.hpp -- what finalising a problem DECIDES, as pure functions of plain data (no HIP,
// no engine): the x ranges and grids of a dataset's windows, the LDS layout of a dataset per
// walker, what an expression runs as, which kernels serve the problem and what they are called.
// mhx_engine.cpp's finalize_problem calls these in order and does the allocating, uploading and
// compiling in between; tests/test_finalize_host.py pins every rule on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mhx_plan.hpp"
#include "mhx_types.hpp"

namespace mhx {

// ---- The kernels a problem can get.
// Compiled problem specialisations.  SPEC_GENERIC dispatches on (model, shape, likelihood) at
// run time; the others fix one model + likelihood for all K functions so that their
// parameters live in scalar registers and the kernel's register budget is its own.
enum SpecId {
  SPEC_GENERIC = 0,
  SPEC_GAUSS22_NORMAL = 1,   // 2 background terms + 2 Gaussian peaks, weighted normal (8 params)
  SPEC_GAUSS15_POISSON = 2,  // constant background + 5 Gaussian peaks, Poisson (16 params)
  SPEC_PVOIGT2_NORMAL = 3,   // 11-parameter two-peak pseudo-Voigt (global fits)
  SPEC_POLY2_NORMAL = 4,     // b + m x
  SPEC_POLY8_NORMAL = 5,     // degree-7 polynomial
  SPEC_LORDER_NORMAL = 6,    // test.lisp's 6-parameter lineshape
  SPEC_GAUSS22_CUTOFF = 7,
#ifdef MHX_AOT_G23
  SPEC__COUNT = 9
#else
  SPEC__COUNT = 8
#endif
};
constexpr int SPEC_USER = 100;  // the program compiled at run time (mhx_rtc.hpp)

inline const char* spec_name(int spec) {
  static const char* names[] = {"generic",      "gauss22_normal", "gauss15_poisson",
                                "pvoigt2_normal", "poly2_normal",   "poly8_normal",
                                "lorder_normal", "gauss22_cutoff"};
  if (spec == 8) return "gauss23_normal_aot_experiment";
  return spec >= 0 && spec < 8 ? names[spec] : "?";
}

inline bool all_fns(const ProblemDesc& P, int model, int lik, int n_idx, int s0, int s1) {
  for (int k = 0; k < P.K; ++k) {
    const FnDesc& f = P.fn[k];
    if (f.model != model || f.lik != lik || f.n_idx != n_idx) return false;
    if (s0 >= 0 && (f.shape[0] != s0 || f.shape[1] != s1)) return false;
  }
  return true;
}

inline int select_spec(const ProblemDesc& P) {
  if (all_fns(P, MHX_MODEL_GAUSS_PEAKS, MHX_LIK_NORMAL, 8, 2, 2)) return SPEC_GAUSS22_NORMAL;
  if (all_fns(P, MHX_MODEL_GAUSS_PEAKS, MHX_LIK_POISSON, 16, 1, 5)) return SPEC_GAUSS15_POISSON;
  if (all_fns(P, MHX_MODEL_PVOIGT2, MHX_LIK_NORMAL, 11, -1, -1)) return SPEC_PVOIGT2_NORMAL;
  if (all_fns(P, MHX_MODEL_POLY, MHX_LIK_NORMAL, 2, -1, -1)) return SPEC_POLY2_NORMAL;
  if (all_fns(P, MHX_MODEL_POLY, MHX_LIK_NORMAL, 8, -1, -1)) return SPEC_POLY8_NORMAL;
  if (all_fns(P, MHX_MODEL_LORDER_MIXED, MHX_LIK_NORMAL, 6, -1, -1)) return SPEC_LORDER_NORMAL;
  if (all_fns(P, MHX_MODEL_GAUSS_PEAKS, MHX_LIK_NORMAL_CUTOFF, 8, 2, 2)) return SPEC_GAUSS22_CUTOFF;
#ifdef MHX_AOT_G23
  if (all_fns(P, MHX_MODEL_GAUSS_PEAKS, MHX_LIK_NORMAL, 11, 2, 3)) return 8;
#endif
  return SPEC_GENERIC;
}

// The C++ type (csrc/mhx_device.hpp) that evaluates function f with everything about its shape
// known at compile time, or "" when the shape is too big for scalar registers.
inline std::string builtin_model_type(const FnDesc& f) {
  switch (f.model) {
    case MHX_MODEL_POLY:
      if (f.n_idx >= 1 && f.n_idx <= 16) return "PolyModel<" + std::to_string(f.n_idx) + ">";
      return "";
    case MHX_MODEL_GAUSS_PEAKS:
    case MHX_MODEL_LORENTZ_PEAKS: {
      const int nbg = f.shape[0], npk = f.shape[1];
      if (npk < 1 || npk > 6 || nbg < 0 || nbg > 4) return "";
      return "PeaksModel<" + std::to_string(nbg) + ", " + std::to_string(npk) + ", " +
             (f.model == MHX_MODEL_LORENTZ_PEAKS ? "true" : "false") + ">";
    }
    case MHX_MODEL_LORDER_MIXED: return "LorderModel";
    case MHX_MODEL_EXP_DECAY: return "ExpDecayModel";
    case MHX_MODEL_SINUSOID: return "SinusoidModel";
    case MHX_MODEL_PVOIGT2: return "PVoigt2Model";
    default: return "";
  }
}

// A model or prior body handed over as a C-syntax expression, or - models only - what a slot of
// the run-time compiled program is instead (mhx_rtc.hpp: rtc_get).
struct UserExpr {
  std::string expr;                // validated, identifiers already rewritten
  std::vector<std::string> names;  // as given by the caller
  std::vector<int> index;
  std::string builtin;   // models: non-empty = the C++ type of an ahead-of-time model struct
                         // ("PeaksModel<1, 3, false>"): no expression, the function is only
                         // given its own compile-time specialisation
  int xcols = 1;         // expression models: 2 when the text names xcol1 (a second column of x)
  bool wgrid = false;    // builtin peaks models: the function has a per-window grid table
                         // (FnDesc::tgh) - its kernel is FixedSpec<Model, LIK, true>
  bool early_reject = false;  // builtin models: compile the program with sweep()'s exact early
                              // rejection (-DMHX_EARLY_REJECT; mhx_kernels.hpp)
  bool planes = false;   // models: the function has a dataset per walker (mhx_set_dataset_planes):
                         // its likelihood is planes_loglik, and the program is compiled with
                         // MHX_PLANES (mhx_kernels.hpp)
  bool dispatch = false; // planes models: an enumerated model without a compile-time type - the
                         // slot goes through the run-time dispatch on FnDesc::model
  int lik = -1;          // models: the function's likelihood kind (-1: dispatch at run time)
  std::string lik_expr;  // models with MHX_LIK_EXPR: the per-point term over y, model, error
};

// What an expression IS (mhx_expr.cpp: rtc_recognise): a polynomial background plus Gaussian or
// Lorentzian peaks over distinct parameters is served by the enumerated model's kernels.
// order[j] = which of the expression's names is local parameter j of the enumerated model
// (bg_0 .., then A, mu, w per peak).
struct RecognisedModel {
  int model = -1;  // MHX_MODEL_POLY / _GAUSS_PEAKS / _LORENTZ_PEAKS, -1: not of the shape
  int shape[2] = {0, 0};
  std::vector<int> order;
};

// A problem that cannot be finalised: the code and message mhx_last_error reports.
struct Refusal {
  int code = MHX_OK;
  std::string msg;
  explicit operator bool() const { return code != MHX_OK; }
};
inline Refusal refuse(int code, const char* fmt, int a = 0, int b = 0) {
  char buf[512];
  snprintf(buf, sizeof buf, fmt, a, b);
  return Refusal{code, buf};
}

// ---- Grids.  A uniformly spaced x (spectra, histograms, time series: x_i = x_0 + i h) lets the
// Gaussian peaks advance by a two-multiply recurrence instead of an exp per point (PeaksModel,
// csrc/mhx_device.hpp).  n points are a grid of step h when every x_i is within 8 ulp of max |x|
// of x_0 + i h.
inline bool grid_fits(const double* x, size_t n, double h) {
  if (n < 2 || h == 0.0 || !std::isfinite(h) || !std::isfinite(x[0]) || !std::isfinite(x[n - 1])) return false;
  const double tol = 8.0 * 0x1p-52 * std::max(std::fabs(x[0]), std::fabs(x[n - 1]));
  for (size_t i = 0; i < n; ++i)
    if (!(std::fabs(x[i] - (x[0] + (double)i * h)) <= tol)) return false;
  return true;
}
// The step of the grid n points are - h_prev if that fits (0: nothing to try first), else their
// own (x_last - x_first) / (n - 1) - or 0 when they are none.
inline double grid_step(const double* x, size_t n, double h_prev = 0.0) {
  if (n < 2) return 0.0;
  if (grid_fits(x, n, h_prev)) return h_prev;
  const double h = (x[n - 1] - x[0]) / (double)(n - 1);
  return grid_fits(x, n, h) ? h : 0.0;
}

// ---- Windows: the kPadPoints-point stretches of a padded dataset (hx: windows_of(n) whole
// windows, the pads repeating the last x), whatever the kernel family.
inline size_t windows_of(size_t n) { return std::max<size_t>((n + kPadPoints - 1) / kPadPoints, 1); }

// The x range of every window, pads included: what tile-level peak skipping tests against
// (PeaksModel::tile_mask; sweep: one mask and one seeding of the recurrence per window).  A window
// that holds a non-finite x gets (-inf, +inf).
inline void window_ranges(const double* hx, size_t n, std::vector<double>* lo, std::vector<double>* hi) {
  const size_t nw = windows_of(n), wp = (size_t)kPadPoints;
  lo->assign(nw, 0.0);
  hi->assign(nw, 0.0);
  for (size_t t = 0; t < nw; ++t) {
    double l = INFINITY, h = -INFINITY;
    bool ok = true;
    for (size_t i = t * wp; i < (t + 1) * wp; ++i) {
      ok = ok && std::isfinite(hx[i]);
      l = std::min(l, hx[i]);
      h = std::max(h, hx[i]);
    }
    (*lo)[t] = ok ? l : -INFINITY;
    (*hi)[t] = ok ? h : INFINITY;
  }
}

// Per-window grids.  A dataset that is not ONE grid may still be a grid window by window -
// concatenated scans, a re-gridded stretch, one jittered region: window w gets H_w = 64 h when
// its data points are a grid of step h - first tried with the previous grid window's h, so that
// runs of windows on one grid carry the SAME bits (the kernel re-derives its constants only where
// H changes: PeaksModel::regrid), then with its own - and 0 otherwise (direct form there).
// False, and no table, when no window is a grid.
inline bool window_grids(const double* hx, size_t n, std::vector<double>* gh) {
  const size_t nw = windows_of(n), wp = (size_t)kPadPoints;
  gh->assign(nw, 0.0);
  double h_prev = 0.0;
  for (size_t t = 0; t < nw; ++t) {
    const size_t i0 = t * wp;
    const double h = grid_step(hx + i0, std::min(wp, n > i0 ? n - i0 : 0), h_prev);
    if (h == 0.0) continue;
    (*gh)[t] = 64.0 * h;
    h_prev = h;
  }
  return h_prev != 0.0;
}

// ---- A dataset per walker (mhx_set_dataset_planes): where function k's arrays lie in
// GroupLds::tiles when the problem is resident (mhx_plan.hpp: planes_resident, one decision for
// the problem) - the functions one after the other, of each its shared x, its shared 1/sigma
// `pitch` doubles on, then a row per wave.  Streamed: all zero but the function's bit.
struct PlanesFn {
  bool planes = false;  // the function has a dataset per walker
  int64_t n = 0;
  int sigma_kind = MHX_SIGMA_NONE;
};
struct PlanesLayout {
  int32_t resident = 0, bit = 0, off_x = 0, off_w = 0, off_rows = 0, row_stride = 0;
};
inline bool planes_layout(const PlanesFn* fn, int K, int waves_per_group, const EngineKnobs& kn,
                          PlanesLayout* out) {
  int64_t pn[MHX_MAX_FUNCTIONS];
  int pk[MHX_MAX_FUNCTIONS], np = 0;
  for (int k = 0; k < K; ++k)
    if (fn[k].planes) pn[np] = fn[k].n, pk[np++] = fn[k].sigma_kind;
  const bool resident = planes_resident(pn, pk, np, K, waves_per_group, kn);
  int64_t off = 0;
  for (int k = 0; k < K; ++k) {
    PlanesLayout& l = out[k] = PlanesLayout{};
    if (!fn[k].planes) continue;
    l.resident = resident ? 1 : 0;
    l.bit = 1 << k;
    if (!resident) continue;
    l.off_x = (int32_t)off;
    l.off_w = (int32_t)(off + planes_pad(fn[k].n));
    off += planes_shared_doubles(fn[k].n, fn[k].sigma_kind);
    l.off_rows = (int32_t)off;
    l.row_stride = (int32_t)planes_wave_doubles(fn[k].n, fn[k].sigma_kind);
    off += (int64_t)waves_per_group * l.row_stride;
  }
  return resident;
}

// ---- What the caller set, function by function, beside the FnDesc.
struct FnInput {
  bool fn_set = false, data_set = false;
  bool planes = false;               // a dataset per walker
  const UserExpr* expr = nullptr;    // the function as an expression (expr->expr empty: an enumerated model)
  const RecognisedModel* recog = nullptr;
  bool prior_expr = false;           // a prior-bounds-let body
  bool lik_expr = false;             // mhx_set_likelihood_expr was called
};

// Step 1: is everything there, and does a dataset per walker go with the rest
inline Refusal validate_problem(const ProblemDesc& P, const FnInput* in, bool pooled) {
  bool planes = false;
  for (int k = 0; k < P.K; ++k) {
    if (!in[k].fn_set) return refuse(MHX_ESTATE, "function %d was never set (mhx_set_function)", k);
    if (!in[k].data_set) return refuse(MHX_ESTATE, "dataset %d was never set (mhx_set_dataset)", k);
    planes = planes || in[k].planes;
  }
  if (!planes) return Refusal{};
  if (pooled)
    return refuse(MHX_EUNSUPPORTED, "a dataset per walker (mhx_set_dataset_planes) with "
                                    "MHX_ADAPT_POOLED: one pooled covariance assumes one posterior");
  for (int k = 0; k < P.K; ++k)
    if (P.fn[k].n_xcols > 1)
      return refuse(MHX_EUNSUPPORTED, "a dataset per walker (mhx_set_dataset_planes) in a problem "
                                      "whose dataset %d has two columns of x (mhx_set_dataset_cols)", k);
  return Refusal{};
}

// A function given as an expression: a body that IS polynomial background + Gaussian /
// Lorentzian peaks runs as that enumerated model (same gather map, permuted into the model's
// order), unless its likelihood is an expression too (which reads `model` from an expression
// model) or recognition is off (mhx_set_expr_recognition; MHX_NO_RECOGNISE=1: A/B runs, bench.py
// --workload c2expr).  Decided when the problem is finalised, not in mhx_set_function_expr: the
// dataset's likelihood may be set before or after.
inline Refusal resolve_functions(ProblemDesc& P, const FnInput* in, bool recognise) {
  for (int k = 0; k < P.K; ++k) {
    FnDesc& f = P.fn[k];
    if (in[k].expr && !in[k].expr->expr.empty()) {
      const UserExpr& u = *in[k].expr;
      const RecognisedModel& r = *in[k].recog;
      if (recognise && r.model >= 0 && f.lik != MHX_LIK_EXPR) {
        f.model = r.model;
        f.n_idx = (int)r.order.size();
        for (int j = 0; j < f.n_idx; ++j) f.idx[j] = u.index[(size_t)r.order[(size_t)j]];
        f.shape[0] = r.shape[0];
        f.shape[1] = r.shape[1];
      } else {
        f.model = MHX_MODEL_EXPR;
        f.n_idx = (int)u.index.size();
        for (int j = 0; j < f.n_idx; ++j) f.idx[j] = u.index[(size_t)j];
        f.shape[0] = f.shape[1] = 0;
      }
    }
    if (f.lik == MHX_LIK_EXPR) {
      if (!in[k].lik_expr)
        return refuse(MHX_ESTATE, "dataset %d uses MHX_LIK_EXPR but mhx_set_likelihood_expr was "
                                  "never called for it", k);
      if (f.model != MHX_MODEL_EXPR)
        return refuse(MHX_EUNSUPPORTED, "function %d: an expression likelihood needs an expression "
                                        "model (mhx_set_function_expr)", k);
    }
    if (f.model == MHX_MODEL_EXPR && in[k].expr->xcols > f.n_xcols)
      return refuse(MHX_ESTATE, "function %d reads xcol1 but dataset %d has one column of x "
                                "(mhx_set_dataset_cols)", k, k);
  }
  return Refusal{};
}

// a point costs 40 instructions and more (ProblemShape::heavy)
inline bool heavy_problem(const ProblemDesc& P) {
  for (int k = 0; k < P.K; ++k) {
    const FnDesc& f = P.fn[k];
    if (f.lik == MHX_LIK_POISSON || f.lik == MHX_LIK_EXPR || f.model == MHX_MODEL_PVOIGT2 ||
        f.model == MHX_MODEL_EXPR)
      return true;
  }
  return false;
}

// ---- Which kernels: an ahead-of-time specialisation if the problem matches one; otherwise
// kernels compiled at run time (hiprtc) in which EVERY function - expression or enumerated model -
// gets its own compile-time specialisation (parameters in SGPRs, fast exp path, tile-level peak
// skipping): 2.4-2.8x the run-time-dispatched generic kernels on configs 2 and 3.  The generic
// kernels remain for MHX_FORCE_GENERIC=1 / MHX_NO_RTC_SPECIALISE=1 and for machines without
// hiprtc.
enum SlotKind {
  SLOT_NONE = 0,  // no slot: an ahead-of-time kernel, or the generic dispatcher inside the program
  SLOT_EXPR,      // the expression as written
  SLOT_BUILTIN,   // an enumerated model under its compile-time type
  SLOT_DISPATCH   // an enumerated model without one, on planes: the run-time dispatch, in a slot
};
struct FnChoice {
  SlotKind kind = SLOT_NONE;
  std::string type;           // SLOT_BUILTIN: builtin_model_type
  int lik = MHX_LIK_NORMAL;
  bool planes = false;
  bool wgrid = false;         // the kernel instance that follows the per-window grid table
  bool early_reject = false;
  bool keep_tgh = false;      // FnDesc::tgh survives (nobody would read it otherwise: the direct form)
  int user_slot = -1, prior_slot = -1;  // FnDesc's
};
struct KernelChoice {
  int K = 0;
  bool rtc = false;               // a program compiled at run time; else the ahead-of-time `spec`
  int spec = SPEC_GENERIC;
  bool compile_required = false;  // rtc: a failed compile is an error (expressions, planes), not
                                  // a fall-back to the generic kernels
  bool builtin_fallback = false;  // rtc: a function stays with the generic dispatcher
  FnChoice fn[MHX_MAX_FUNCTIONS];
};

// has_tgh[k]: function k has a per-window grid table (window_grids), in.planes / .prior_expr as above
inline KernelChoice choose_kernels(const ProblemDesc& P, const FnInput* in, const bool* has_tgh, bool pooled,
                                   const EngineKnobs& kn) {
  KernelChoice c;
  c.K = P.K;
  const bool specialise = !kn.no_rtc_specialise && !kn.force_generic;
  bool any_expr = false, any_wgrid = false, any_planes = false;
  for (int k = 0; k < P.K; ++k) {
    const FnDesc& f = P.fn[k];
    c.fn[k].lik = f.lik;
    c.fn[k].planes = in[k].planes;
    any_expr = any_expr || f.model == MHX_MODEL_EXPR || in[k].prior_expr;
    // a dataset per walker has its sweep in programs compiled at run time only (MHX_PLANES)
    any_planes = any_planes || in[k].planes;
    // a function with a per-window grid table needs the kernel instance that follows it
    // (FixedSpec<Model, LIK, true>, mhx_kernels.hpp): compiled at run time, like every problem
    // without an ahead-of-time kernel - the ahead-of-time ones stay what they were
    c.fn[k].keep_tgh = specialise && !in[k].planes && has_tgh[k] && f.model == MHX_MODEL_GAUSS_PEAKS &&
                       f.shape[0] >= 1 && f.shape[0] <= 2 && f.shape[1] >= 1 && f.shape[1] <= 6 &&
                       f.lik != MHX_LIK_EXPR;
    any_wgrid = any_wgrid || c.fn[k].keep_tgh;
  }
  // MHX_EARLY_REJECT=1: sweep()'s exact early rejection (mhx_kernels.hpp) for a problem of ONE
  // function of a bounded enumerated model (peaks, polynomial: no term of theirs overflows at
  // finite parameters) with the weighted normal likelihood and no prior body - compiled at run
  // time too, so that the ahead-of-time kernels do not carry the test (4-5 % in a walk's first
  // iterations even when it never fires)
  const FnDesc& f0 = P.fn[0];
  const bool any_er = kn.early_reject && specialise && P.K == 1 && f0.lik == MHX_LIK_NORMAL &&
                      (f0.model == MHX_MODEL_GAUSS_PEAKS || f0.model == MHX_MODEL_LORENTZ_PEAKS ||
                       f0.model == MHX_MODEL_POLY) &&
                      !in[0].prior_expr && !builtin_model_type(f0).empty() && !pooled && !any_planes;
  const bool must_rtc = any_expr || any_wgrid || any_er || any_planes;
  const int aot = must_rtc ? SPEC_GENERIC : select_spec(P);
  if (!must_rtc && (aot != SPEC_GENERIC || !specialise)) {
    c.spec = kn.force_generic ? SPEC_GENERIC : aot;
    return c;
  }
  c.rtc = true;
  c.compile_required = any_expr || any_planes;
  int n_models = 0, n_priors = 0;
  for (int k = 0; k < P.K; ++k) {
    const FnDesc& f = P.fn[k];
    FnChoice& fc = c.fn[k];
    const std::string type = specialise && f.model != MHX_MODEL_EXPR ? builtin_model_type(f) : std::string();
    if (f.model == MHX_MODEL_EXPR) {
      fc.kind = SLOT_EXPR;
    } else if (!type.empty()) {
      fc.kind = SLOT_BUILTIN;
      fc.type = type;
      fc.wgrid = fc.keep_tgh;
      fc.early_reject = any_er;
    } else if (in[k].planes) {
      fc.kind = SLOT_DISPATCH;
    } else {
      c.builtin_fallback = true;
    }
    if (fc.kind != SLOT_NONE) fc.user_slot = n_models++;
    if (in[k].prior_expr) fc.prior_slot = n_priors++;
  }
  return c;
}

// the run-time compile failed on a problem of enumerated models only: the generic kernels serve
inline void fall_back_to_generic(KernelChoice* c) {
  c->rtc = false;
  c->spec = SPEC_GENERIC;
  for (int k = 0; k < c->K; ++k) c->fn[k].user_slot = -1;
}

// what the choice leaves in the problem description the kernels read
inline void apply_choice(const KernelChoice& c, ProblemDesc* P) {
  for (int k = 0; k < c.K; ++k) {
    FnDesc& f = P->fn[k];
    f.user_slot = c.fn[k].user_slot;
    f.prior_slot = c.fn[k].prior_slot;
    if (!c.fn[k].keep_tgh) f.tgh = nullptr;
  }
}

// the program's model slots (rtc_get's `models`), in slot order; expr[k], lik_expr[k]: the texts
inline std::vector<UserExpr> program_models(const KernelChoice& c, const UserExpr* expr, const std::string* lik_expr) {
  std::vector<UserExpr> models;
  for (int k = 0; k < c.K; ++k) {
    const FnChoice& fc = c.fn[k];
    if (fc.kind == SLOT_NONE) continue;
    UserExpr u = fc.kind == SLOT_EXPR ? expr[k] : UserExpr();
    u.builtin = fc.type;
    u.lik = fc.lik;
    u.wgrid = fc.wgrid;
    u.early_reject = fc.early_reject;
    u.planes = fc.planes;
    u.dispatch = fc.kind == SLOT_DISPATCH;
    if (fc.lik == MHX_LIK_EXPR) u.lik_expr = lik_expr[k];
    models.push_back(u);
  }
  return models;
}

// A name for what was chosen (mhx_kernel_name).  rtc_note: why a problem of enumerated models was
// not specialised (the first line of the compiler's message).
inline std::string kernel_name(const KernelChoice& c, int waves_per_group, bool planes_res, const LaunchPlan& plan,
                               const std::string& rtc_note) {
  static const char* kLik[] = {"normal", "normal_cutoff", "poisson", "expr"};
  std::string name = "w" + std::to_string(waves_per_group) + "/";
  if (c.rtc) {
    name += "rtc[";
    for (int k = 0; k < c.K; ++k) {
      const FnChoice& fc = c.fn[k];
      const std::string t = fc.kind == SLOT_EXPR ? std::string("expr")
                            : fc.kind == SLOT_BUILTIN
                                ? fc.type + (fc.wgrid ? "+wgrid" : "") + (fc.early_reject ? "+early-reject" : "")
                                : std::string("generic");
      name += (k ? ", " : "") + t + ":" + kLik[fc.lik & 3] +
              (fc.planes ? (planes_res ? "+planes(resident)" : "+planes(streamed)") : "");
    }
    name += "]";
  } else {
    name += spec_name(c.spec);
    if (!rtc_note.empty()) name += " [not specialised: " + rtc_note + "]";
  }
  if (plan.split_slices > 0)
    name += (plan.tsplit ? (plan.persist ? " persistent tsplit x" : " tsplit x")
                         : (plan.persist ? " persistent split x" : " split x")) +
            std::to_string(plan.split_slices);
  return name;
}

}  // namespace mhx
