// mhx_stage.hpp -- the arithmetic of the batched read-outs' stage buffer as pure functions of
// plain numbers (no HIP, no engine): how a portion of items is carved into 256-byte aligned
// pieces, how many items fit the budget, and the order in which portions are worked through.
// mhx_engine.cpp's portion runner launches what these describe; tests/test_stage_plan.py pins the
// portion sizes and the carving on the CPU.  With them, and as free of HIP: data_view, where a
// chain's own data lie for a launch (tests/test_dataview_host.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mhx_types.hpp"

namespace mhx {

constexpr size_t kStageAlign = 256;
inline size_t align256(size_t v) { return (v + kStageAlign - 1) & ~(kStageAlign - 1); }

// what a read-out's pieces may take of an engine's stage buffer, whatever the call's size
constexpr size_t kStageBudget = (size_t)64 << 20;
// points of x a fit launch works on at a time
constexpr int64_t kFitChunkPoints = (int64_t)1 << 17;

// hands out consecutive 256-byte aligned offsets
struct Carver {
  size_t take(size_t bytes) {
    const size_t o = end_;
    end_ += align256(bytes);
    asked_ += bytes;
    ++pieces_;
    return o;
  }
  size_t bytes() const { return end_; }    // the buffer the pieces need
  size_t asked() const { return asked_; }  // ... of which the pieces themselves
  int pieces() const { return pieces_; }

 private:
  size_t end_ = 0, asked_ = 0;
  int pieces_ = 0;
};

inline int64_t portion_items(size_t budget, size_t fixed_bytes, size_t per_item_bytes) {
  return std::max<int64_t>(1, (int64_t)((budget - fixed_bytes) / per_item_bytes));
}
// The items of one portion, from the piece list that carves it: carve(carver, n) takes the pieces
// of n items, each of a size linear in n.  What 0 items take is fixed, an item adds the
// difference, and every piece may lose up to kStageAlign bytes to its alignment.
template <class Carve>
int64_t portion_of(Carve&& carve) {
  Carver none, one;
  carve(none, 0);
  carve(one, 1);
  return portion_items(kStageBudget, none.asked() + (size_t)none.pieces() * kStageAlign, one.asked() - none.asked());
}

// ---- the pieces of each read-out, in the order they lie in the buffer

// walker-set-get: two double arrays [n][nd], two int arrays [n] (ni of them in use), the index
// scratch [n][take] of the covariance and factor kernels
enum { SUM_PERCENTILES = 0, SUM_COVARIANCES = 1, SUM_FACTORS = 2, SUM_BEST = 3 };
struct SummaryShape {
  size_t nd[2] = {0, 0};
  int ni = 0;
  size_t scratch = 0;  // ints per chain
};
inline SummaryShape summary_shape(int kind, int d_, int n_pct, int take) {
  const size_t d = (size_t)d_, dd = d * d;
  SummaryShape y;
  switch (kind) {
    case SUM_PERCENTILES: y.nd[0] = (size_t)n_pct * d; y.ni = 1; break;
    case SUM_COVARIANCES: y.nd[0] = dd; y.ni = 2; y.scratch = (size_t)take; break;
    case SUM_FACTORS: y.nd[0] = y.nd[1] = dd; y.ni = 2; y.scratch = (size_t)take; break;
    default: y.nd[0] = 1; y.nd[1] = d; break;
  }
  return y;
}
struct SummaryPieces {
  size_t dv[2], iv[2], scratch;
};
inline SummaryPieces carve_summary(Carver& c, const SummaryShape& y, int64_t n_) {
  const size_t n = (size_t)n_;
  SummaryPieces s;
  for (int k = 0; k < 2; ++k) s.dv[k] = c.take(n * y.nd[k] * sizeof(double));
  for (int k = 0; k < 2; ++k) s.iv[k] = c.take(k < y.ni ? n * sizeof(int32_t) : 0);
  s.scratch = c.take(n * y.scratch * sizeof(int32_t));
  return s;
}

// fit curves and bands, n items at m points (take 0: parameter vectors [n][d], else the selected
// steps' slots [n][take] of the chains).  The pieces whose size depends on the items alone come
// first: they keep their place from one chunk of points to the next.  theta is carved for the
// bands too, which leave it unused: an item has always been budgeted with it.
struct FitPieces {
  size_t sel, n_sel, status, theta, x0, x1, ymax, ymin;
};
inline FitPieces carve_fit(Carver& c, int d, int take, int64_t n_, int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_;
  FitPieces s;
  s.sel = c.take(n * (size_t)take * sizeof(int32_t));
  s.n_sel = c.take(n * sizeof(int32_t));
  s.status = c.take(n * sizeof(int32_t));
  s.theta = c.take(n * (size_t)d * sizeof(double));
  s.x0 = c.take(m * sizeof(double));
  s.x1 = c.take(m * sizeof(double));
  s.ymax = c.take(n * m * sizeof(double));
  s.ymin = c.take(n * m * sizeof(double));
  return s;
}

// derived quantities: the values [n][ne][take], the results [n][ne] (percentiles [n][ne][n_pct]),
// n_used [n], status [n][ne]
struct DerivedPieces {
  size_t values, at_best, pct, mean, stddev, n_used, status;
};
inline DerivedPieces carve_derived(Carver& c, int ne_, int take, int n_pct, int64_t n_) {
  const size_t n = (size_t)n_, ne = (size_t)ne_;
  DerivedPieces s;
  s.values = c.take(n * ne * (size_t)take * sizeof(double));
  s.at_best = c.take(n * ne * sizeof(double));
  s.pct = c.take(n * ne * (size_t)n_pct * sizeof(double));
  s.mean = c.take(n * ne * sizeof(double));
  s.stddev = c.take(n * ne * sizeof(double));
  s.n_used = c.take(n * sizeof(int32_t));
  s.status = c.take(n * ne * sizeof(int32_t));
  return s;
}

// posterior histograms: the caller's edges [nc][nb + 1] - one set for every chain (per_chain 0:
// the piece does not grow with n and comes first either way) or [n][nc][nb + 1] - the counts
// [n][nc][nb], (below, above) [n][nc][2], n_used [n], status [n][nc]
struct HistoPieces {
  size_t edges, counts, outside, n_used, status;
};
inline HistoPieces carve_histo(Carver& c, int nc_, int nb_, int per_chain, int64_t n_) {
  const size_t n = (size_t)n_, nc = (size_t)nc_, nb = (size_t)nb_;
  HistoPieces s;
  s.edges = c.take((per_chain ? n : 1) * nc * (nb + 1) * sizeof(double));
  s.counts = c.take(n * nc * nb * sizeof(int32_t));
  s.outside = c.take(n * nc * 2 * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.status = c.take(n * nc * sizeof(int32_t));
  return s;
}
// pair-count grids: the edges as above and the pair list (pair_a [np], pair_b [np]), neither
// growing with n unless the edges are per chain; the cells [n][np][nb][nb], n_inside [n][np],
// n_used [n], status [n][np]
struct GridPieces {
  size_t edges, pairs, counts, n_inside, n_used, status;
};
inline GridPieces carve_grid(Carver& c, int nc_, int nb_, int np_, int per_chain, int64_t n_) {
  const size_t n = (size_t)n_, nc = (size_t)nc_, nb = (size_t)nb_, np = (size_t)np_;
  GridPieces s;
  s.edges = c.take((per_chain ? n : 1) * nc * (nb + 1) * sizeof(double));
  s.pairs = c.take(2 * np * sizeof(int32_t));
  s.counts = c.take(n * np * nb * nb * sizeof(int32_t));
  s.n_inside = c.take(n * np * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.status = c.take(n * np * sizeof(int32_t));
  return s;
}
// autocorrelation read-out: rho [n][nc][max_lag + 1] - always carved: the kernel writes it and reads
// it back for Geyer's sum, whether the caller asks for it or not - tau, ess [n][nc], half_mean,
// half_var [n][nc][2], n_lags, n_used [n], status [n][nc].  One chain's pieces are about 0.5 MB at
// most (nc = 63, max_lag = 1023): they always fit the budget.
struct AutocorrPieces {
  size_t acf, tau, ess, half_mean, half_var, n_lags, n_used, status;
};
inline AutocorrPieces carve_autocorr(Carver& c, int nc_, int max_lag, int64_t n_) {
  const size_t n = (size_t)n_, nc = (size_t)nc_, nl = (size_t)max_lag + 1;
  AutocorrPieces s;
  s.acf = c.take(n * nc * nl * sizeof(double));
  s.tau = c.take(n * nc * sizeof(double));
  s.ess = c.take(n * nc * sizeof(double));
  s.half_mean = c.take(n * nc * 2 * sizeof(double));
  s.half_var = c.take(n * nc * 2 * sizeof(double));
  s.n_lags = c.take(n * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.status = c.take(n * nc * sizeof(int32_t));
  return s;
}
// WAIC of n chains at m points of a function of nb_total blocks: what depends on the chains alone
// comes first and keeps its place from one chunk of points to the next - status, n_used, n_high
// [n], the totals elpd, lppd, p_waic [n], the blocks' partial sums [n][nb_total] (two double
// arrays, one int) - then the chunk's per-point constants [m] and the pointwise results the caller
// asked for: pw_lppd, pw_p [n][m], pw_acc [n][m][4] (want bits 1, 2, 4; a piece not asked for is
// empty and the kernel does not write it).
enum { WAIC_WANT_LPPD = 1, WAIC_WANT_P = 2, WAIC_WANT_ACC = 4 };
struct WaicPieces {
  size_t status, n_used, n_high, elpd, lppd, p_waic, part_lppd, part_p, part_high, cst, pw_lppd, pw_p, pw_acc;
};
inline WaicPieces carve_waic(Carver& c, int64_t nb_total, int want, int64_t n_, int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_, nb = (size_t)nb_total;
  WaicPieces s;
  s.status = c.take(n * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.n_high = c.take(n * sizeof(int32_t));
  s.elpd = c.take(n * sizeof(double));
  s.lppd = c.take(n * sizeof(double));
  s.p_waic = c.take(n * sizeof(double));
  s.part_lppd = c.take(n * nb * sizeof(double));
  s.part_p = c.take(n * nb * sizeof(double));
  s.part_high = c.take(n * nb * sizeof(int32_t));
  s.cst = c.take(m * sizeof(double));
  s.pw_lppd = c.take((want & WAIC_WANT_LPPD) ? n * m * sizeof(double) : 0);
  s.pw_p = c.take((want & WAIC_WANT_P) ? n * m * sizeof(double) : 0);
  s.pw_acc = c.take((want & WAIC_WANT_ACC) ? n * m * 4 * sizeof(double) : 0);
  return s;
}
// Residuals of n chains at m points of a function of nb_total blocks: what depends on the chains
// alone comes first and keeps its place from one chunk of points to the next - status, the counts
// n_pos, n_runs, n_out [n], max_index [n], the totals chi2, sum_z, dw, max_abs_z [n], the caller's
// parameter vectors theta [n][d] (with_theta 0: empty, the device's most-likely ones are read), the
// blocks' partials [n][nb_total] (four double arrays, one of 64-bit indices, one of three ints) -
// then the pointwise results the caller asked for: fit, z [n][m] (want bits 1, 2; a piece not asked
// for is empty and the kernel does not write it).
enum { RESID_WANT_FIT = 1, RESID_WANT_Z = 2 };
struct ResidPieces {
  size_t status, n_pos, n_runs, n_out, max_index, chi2, sum_z, dw, max_abs_z, theta, part_chi2, part_sumz,
      part_dw, part_max, part_idx, part_cnt, fit, z;
};
inline ResidPieces carve_resid(Carver& c, int64_t nb_total, int d, int with_theta, int want, int64_t n_,
                               int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_, nb = (size_t)nb_total;
  ResidPieces s;
  s.status = c.take(n * sizeof(int32_t));
  s.n_pos = c.take(n * sizeof(int32_t));
  s.n_runs = c.take(n * sizeof(int32_t));
  s.n_out = c.take(n * sizeof(int32_t));
  s.max_index = c.take(n * sizeof(int64_t));
  s.chi2 = c.take(n * sizeof(double));
  s.sum_z = c.take(n * sizeof(double));
  s.dw = c.take(n * sizeof(double));
  s.max_abs_z = c.take(n * sizeof(double));
  s.theta = c.take(with_theta ? n * (size_t)d * sizeof(double) : 0);
  s.part_chi2 = c.take(n * nb * sizeof(double));
  s.part_sumz = c.take(n * nb * sizeof(double));
  s.part_dw = c.take(n * nb * sizeof(double));
  s.part_max = c.take(n * nb * sizeof(double));
  s.part_idx = c.take(n * nb * sizeof(int64_t));
  s.part_cnt = c.take(n * nb * 3 * sizeof(int32_t));
  s.fit = c.take((want & RESID_WANT_FIT) ? n * m * sizeof(double) : 0);
  s.z = c.take((want & RESID_WANT_Z) ? n * m * sizeof(double) : 0);
  return s;
}
// Normal equations of n chains at m points of a function of nb_total blocks and n_tasks tasks in a
// problem of d parameters: the shared steps [d] come first (per_chain_steps: empty here), then
// what depends on the chains alone and keeps its place from one chunk of points to the next -
// status, chi2 [n], jtr [n][d], jtj [n][d][d], the per-chain steps [n][d] (else empty), the
// caller's parameter vectors theta [n][d] (with_theta 0: empty), the blocks' partials
// [n][nb_total][n_tasks] - then the Jacobian g [n][d][m] where the caller asked for it.
struct NormEqPieces {
  size_t steps, status, chi2, jtr, jtj, chain_steps, theta, part, g;
};
inline NormEqPieces carve_normeq(Carver& c, int64_t nb_total, int n_tasks, int d_, int per_chain_steps,
                                 int with_theta, int want_g, int64_t n_, int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_, nb = (size_t)nb_total, d = (size_t)d_;
  NormEqPieces s;
  s.steps = c.take(per_chain_steps ? 0 : d * sizeof(double));
  s.status = c.take(n * sizeof(int32_t));
  s.chi2 = c.take(n * sizeof(double));
  s.jtr = c.take(n * d * sizeof(double));
  s.jtj = c.take(n * d * d * sizeof(double));
  s.chain_steps = c.take(per_chain_steps ? n * d * sizeof(double) : 0);
  s.theta = c.take(with_theta ? n * d * sizeof(double) : 0);
  s.part = c.take(n * nb * (size_t)n_tasks * sizeof(double));
  s.g = c.take(want_g ? n * d * m * sizeof(double) : 0);
  return s;
}
// Candidate scores of n chains, m_cand candidates each, over functions of nb_pitch blocks in all:
// the candidates [m_cand][d] - one set for every chain (per_chain 0: the piece does not grow with n
// and comes first either way) or [n][m_cand][d] - then n_bad [n], best_index, best_score [n][keep],
// the scores [n][m_cand] (always carved: the ranking reads them) and the blocks' sums
// [n][m_cand][nb_pitch].
struct CandPieces {
  size_t cand, n_bad, best_index, best_score, score, part;
};
inline CandPieces carve_cand(Carver& c, int64_t nb_pitch, int d_, int per_chain, int keep_, int64_t m_cand,
                             int64_t n_) {
  const size_t n = (size_t)n_, m = (size_t)m_cand, nb = (size_t)nb_pitch, d = (size_t)d_, keep = (size_t)keep_;
  CandPieces s;
  s.cand = c.take((per_chain ? n : 1) * m * d * sizeof(double));
  s.n_bad = c.take(n * sizeof(int32_t));
  s.best_index = c.take(n * keep * sizeof(int32_t));
  s.best_score = c.take(n * keep * sizeof(double));
  s.score = c.take(n * m * sizeof(double));
  s.part = c.take(n * m * nb * sizeof(double));
  return s;
}
// The DataView (mhx_types.hpp) of function f from point m0 of its dataset on: the shared arrays
// (pd NULL), or the planes of a dataset per walker, whose row c is the engine's chain c.  Every
// array a point indexes is offset by m0; the one 1/sigma per walker of kPlaneWScalar is not.
inline DataView data_view(const FnDesc& f, const PlaneDesc* pd, int64_t m0) {
  DataView v{};
  v.x0 = f.x + m0;
  v.x1 = f.n_xcols > 1 ? f.c + m0 : nullptr;
  if (pd) {
    v.y = pd->y + m0, v.y_pitch = pd->pitch;
    switch (pd->w_kind) {
      case kPlaneWShared: v.w = f.w + m0, v.w_pitch = 0, v.w_step = 1; break;
      case kPlaneWScalar: v.w = pd->w, v.w_pitch = 1, v.w_step = 0; break;
      default: v.w = pd->w + m0, v.w_pitch = pd->pitch, v.w_step = 1; break;
    }
  } else {
    v.y = f.y + m0, v.y_pitch = 0;
    v.w = f.w + m0, v.w_pitch = 0, v.w_step = 1;
  }
  return v;
}
// batched traces: the caller's column list [n_cols] - it does not grow with n and comes first -
// the rows values [n][max_out][n_cols], their envelopes lo and hi of the same shape (envelope 0:
// both empty, the kernel does not write them), n_out, n_kept, n_used [n], and the kept-index
// scratch [n][take]: the ring slots of the steps that passed the filter, newest first.  The
// outputs lie together, values .. n_used, so that one clear zeroes them.
struct TracePieces {
  size_t cols, values, lo, hi, n_out, n_kept, n_used, kept;
};
inline TracePieces carve_traces(Carver& c, int n_cols_, int max_out_, int take, int envelope, int64_t n_) {
  const size_t n = (size_t)n_, rows = (size_t)max_out_ * (size_t)n_cols_;
  TracePieces s;
  s.cols = c.take((size_t)n_cols_ * sizeof(int32_t));
  s.values = c.take(n * rows * sizeof(double));
  s.lo = c.take(envelope ? n * rows * sizeof(double) : 0);
  s.hi = c.take(envelope ? n * rows * sizeof(double) : 0);
  s.n_out = c.take(n * sizeof(int32_t));
  s.n_kept = c.take(n * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.kept = c.take(n * (size_t)take * sizeof(int32_t));
  return s;
}
// highest-density intervals and quantile ladders: the staged values [n][nc][take] of the derived
// form (with_values 0: empty, the ring's columns are read), lo, hi [n][n_mass][nc], pos of the same
// shape, the ladder [n][nc][n_ladder], n_used [n], status [n][nc], and on the memory path the keys
// [n][nc][key_pitch] (key_pitch 0, the LDS path: empty).  The keys of ONE chain may exceed the
// budget (63 columns of a window of 2^17 steps): the caller asks one_item_fits first.
struct HdiPieces {
  size_t values, lo, hi, pos, ladder, n_used, status, keys;
};
inline HdiPieces carve_hdi(Carver& c, int nc_, int n_mass, int n_ladder, int take, int with_values,
                           int64_t key_pitch, int64_t n_) {
  const size_t n = (size_t)n_, nc = (size_t)nc_, nm = (size_t)n_mass;
  HdiPieces s;
  s.values = c.take(with_values ? n * nc * (size_t)take * sizeof(double) : 0);
  s.lo = c.take(n * nm * nc * sizeof(double));
  s.hi = c.take(n * nm * nc * sizeof(double));
  s.pos = c.take(n * nm * nc * sizeof(int32_t));
  s.ladder = c.take(n * nc * (size_t)n_ladder * sizeof(double));
  s.n_used = c.take(n * sizeof(int32_t));
  s.status = c.take(n * nc * sizeof(int32_t));
  s.keys = c.take(n * nc * (size_t)key_pitch * sizeof(uint64_t));
  return s;
}
// Whether ONE item of a piece list fits the budget at all, by portion_of's own accounting
// (portion_of answers 1 either way: a read-out that must not outgrow the budget asks first).
template <class Carve>
bool one_item_fits(Carve&& carve) {
  Carver none, one;
  carve(none, 0);
  carve(one, 1);
  return one.asked() + (size_t)none.pieces() * kStageAlign <= kStageBudget;
}

// ---- the order of the portions: `items` in portions of at most `per_portion`, each worked
// through `points` in chunks of at most `chunk` - points first, then items.  The first portion
// is the largest in both.
struct Portion {
  int64_t i0, n, m0, m;
};
struct PortionCursor {
  int64_t items = 0, per_portion = 1, points = 1, chunk = 1;
  int64_t i0 = 0, m0 = 0;
  bool done() const { return i0 >= items; }
  Portion now() const {
    return {i0, std::min(items - i0, per_portion), m0, std::min(points - m0, chunk)};
  }
  void advance() {
    const Portion p = now();
    m0 += p.m;
    if (m0 >= points) {
      m0 = 0;
      i0 += p.n;
    }
  }
};
// The cursor of a call over `items` and `points` (1 unless x goes in chunks): at most
// kFitChunkPoints points at a time, and the items per portion that carve(carver, n, m) gives at
// that many points.
template <class Carve>
PortionCursor portion_cursor(int64_t items, int64_t points, Carve&& carve) {
  PortionCursor at;
  at.items = items;
  at.points = points;
  at.chunk = std::min(points, kFitChunkPoints);
  at.per_portion = portion_of([&](Carver& c, int64_t n) { carve(c, n, at.chunk); });
  return at;
}

// The cursor of a call whose values are staged per item, step and point (mhx_get_fit_percentiles,
// mhx_get_loo).  portion_cursor's fixed chunk would ask 1 GB of one chain at take 1000: here the
// chunk of points is all of `points` where one item fits the budget with them (fits(m); and they
// are at most kFitChunkPoints), else the largest whole number of blocks of `block` points, at most
// kFitChunkPoints, with which one item fits.  chunk == 0: not even one block fits - the caller
// refuses the call.
template <class Fits, class Carve>
PortionCursor block_cursor(int64_t items, int64_t points, int64_t block, Fits&& fits, Carve&& carve) {
  PortionCursor at;
  at.items = items;
  at.points = points;
  if (points <= kFitChunkPoints && fits(points)) {
    at.chunk = points;
  } else {
    int64_t lo = 0, hi = std::min(points, kFitChunkPoints) / block;  // blocks: lo fits, hi + 1 does not
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) / 2;
      if (fits(mid * block)) lo = mid; else hi = mid - 1;
    }
    at.chunk = lo * block;
  }
  at.per_portion = at.chunk > 0 ? portion_of([&](Carver& c, int64_t n) { carve(c, n, at.chunk); }) : 1;
  return at;
}
// the greatest take for which fits(take) holds (0: none does); fits is monotone in take
template <class Fits>
int max_take_that_fits(Fits&& fits) {
  int lo = 0, hi = 1 << 30;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (fits(mid)) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- pointwise percentiles of the fit (mhx_get_fit_percentiles): n chains at m points.  What
// depends on the chains alone comes first and keeps its place from one chunk of points to the
// next - status, n_used [n] - then x0, x1 [m], the staged values [n][take][m] (a chain's window
// step by step, the points of a step side by side) and the results pct [n][n_pct][m], mean,
// stddev [n][m].
constexpr int64_t kFitPctBlock = 128;  // points of a block of the value kernel (MHX_FITPCT_BLOCK)
static_assert(kFitChunkPoints % kFitPctBlock == 0, "a chunk of points is whole blocks");
struct FitPctPieces {
  size_t status, n_used, x0, x1, values, pct, mean, stddev;
};
inline FitPctPieces carve_fitpct(Carver& c, int take, int n_pct, int64_t n_, int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_;
  FitPctPieces s;
  s.status = c.take(n * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.x0 = c.take(m * sizeof(double));
  s.x1 = c.take(m * sizeof(double));
  s.values = c.take(n * m * (size_t)take * sizeof(double));
  s.pct = c.take(n * (size_t)n_pct * m * sizeof(double));
  s.mean = c.take(n * m * sizeof(double));
  s.stddev = c.take(n * m * sizeof(double));
  return s;
}
// whether ONE chain's pieces at m points fit the budget
inline bool fitpct_fits(int take, int n_pct, int64_t m) {
  return one_item_fits([&](Carver& c, int64_t n) { carve_fitpct(c, take, n_pct, n, m); });
}
// The cursor of mhx_get_fit_percentiles: block_cursor over blocks of kFitPctBlock points.
inline PortionCursor fitpct_cursor(int64_t items, int64_t points, int take, int n_pct) {
  return block_cursor(items, points, kFitPctBlock, [&](int64_t m) { return fitpct_fits(take, n_pct, m); },
                      [&](Carver& c, int64_t n, int64_t m) { carve_fitpct(c, take, n_pct, n, m); });
}
// the greatest take at which one chain's smallest chunk of `points` fits (0: none does)
inline int fitpct_max_take(int64_t points, int n_pct) {
  const int64_t m = std::min(points, kFitPctBlock);
  return max_take_that_fits([&](int take) { return fitpct_fits(take, n_pct, m); });
}

// ---- PSIS-LOO (mhx_get_loo): n chains at m points of a function of nb_total blocks.  What depends
// on the chains alone comes first and keeps its place from one chunk of points to the next - status,
// n_used, n_high [n], the totals elpd, p_loo, lppd [n], the blocks' partial sums [n][nb_total] (two
// double arrays, one int) - then the chunk's per-point constants [m], the staged terms [n][take][m]
// (a chain's window step by step, the points of a step side by side), the pointwise results pw_elpd,
// pw_khat, pw_lppd [n][m] (always carved: the block sums read them) and, where the caller asked for
// them (want bits 1, 2), pw_acc [n][m][4] and tail [n][m][P].
constexpr int64_t kLooBlock = 256;  // points of a block of the sums (MHX_LOO_BLOCK)
static_assert(kFitChunkPoints % kLooBlock == 0, "a chunk of points is whole blocks");
enum { LOO_WANT_ACC = 1, LOO_WANT_TAIL = 2 };
struct LooPieces {
  size_t status, n_used, n_high, elpd, p_loo, lppd, part_elpd, part_lppd, part_high, cst, terms, pw_elpd, pw_khat,
      pw_lppd, pw_acc, tail;
};
inline LooPieces carve_loo(Carver& c, int64_t nb_total, int take, int P, int want, int64_t n_, int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_, nb = (size_t)nb_total;
  LooPieces s;
  s.status = c.take(n * sizeof(int32_t));
  s.n_used = c.take(n * sizeof(int32_t));
  s.n_high = c.take(n * sizeof(int32_t));
  s.elpd = c.take(n * sizeof(double));
  s.p_loo = c.take(n * sizeof(double));
  s.lppd = c.take(n * sizeof(double));
  s.part_elpd = c.take(n * nb * sizeof(double));
  s.part_lppd = c.take(n * nb * sizeof(double));
  s.part_high = c.take(n * nb * sizeof(int32_t));
  s.cst = c.take(m * sizeof(double));
  s.terms = c.take(n * m * (size_t)take * sizeof(double));
  s.pw_elpd = c.take(n * m * sizeof(double));
  s.pw_khat = c.take(n * m * sizeof(double));
  s.pw_lppd = c.take(n * m * sizeof(double));
  s.pw_acc = c.take((want & LOO_WANT_ACC) ? n * m * 4 * sizeof(double) : 0);
  s.tail = c.take((want & LOO_WANT_TAIL) ? n * m * (size_t)P * sizeof(double) : 0);
  return s;
}
// whether ONE chain's pieces at m points fit the budget
inline bool loo_fits(int64_t nb_total, int take, int P, int want, int64_t m) {
  return one_item_fits([&](Carver& c, int64_t n) { carve_loo(c, nb_total, take, P, want, n, m); });
}
// The cursor of mhx_get_loo: block_cursor over blocks of kLooBlock points.
inline PortionCursor loo_cursor(int64_t items, int64_t points, int take, int P, int want) {
  const int64_t nb_total = (points + kLooBlock - 1) / kLooBlock;
  return block_cursor(items, points, kLooBlock, [&](int64_t m) { return loo_fits(nb_total, take, P, want, m); },
                      [&](Carver& c, int64_t n, int64_t m) { carve_loo(c, nb_total, take, P, want, n, m); });
}
// the greatest take at which one chain's smallest chunk of `points` fits, with the tail of P slots
// the call asked for (0: none does)
inline int loo_max_take(int64_t points, int P, int want) {
  const int64_t nb_total = (points + kLooBlock - 1) / kLooBlock, m = std::min(points, kLooBlock);
  return max_take_that_fits([&](int take) { return loo_fits(nb_total, take, P, want, m); });
}

}  // namespace mhx
