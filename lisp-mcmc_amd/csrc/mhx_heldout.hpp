// mhx_heldout.hpp -- the host half of mhx_get_heldout as pure functions of plain numbers and the
// caller's arrays (no HIP, no engine): what mhx_set_dataset would refuse of them, which of the
// prepared arrays (ys, w, c and the use bytes) vary by chain and which by point, their numbers for
// a chunk of points and a range of chains - formed exactly as mhx_set_dataset forms a dataset's -
// and the pieces of a portion in the stage buffer.  mhx_engine.cpp's HeldoutCall uploads and
// launches what these describe; tests/test_heldout_stage_plan.py drives them on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mhx.h"
#include "mhx_stage.hpp"

namespace mhx {

// M:379-380: (reduce (lambda (x y) (+ x (log y))) (up-to n)) sums SINGLE-float logs
inline double log_factorial_ref(long n, bool in_double, std::vector<float>& cache) {
  if (in_double) return std::lgamma((double)n + 1.0);
  if (n <= 0) return 0.0;
  if ((long)cache.size() <= n) {
    size_t old = cache.size();
    if (old == 0) {
      cache.push_back(0.0f);
      old = 1;
    }
    cache.resize((size_t)n + 1);
    for (size_t m = old; m <= (size_t)n; ++m) cache[m] = cache[m - 1] + (float)std::log((double)m);
  }
  return (double)cache[(size_t)n];
}

// How a prepared array varies: not there at all, one number for every chain and point, a row [m]
// shared by the chains, a scalar per chain [n], a plane [n][m].  The kernel indexes all of them as
// a[i * pitch + p * step] (HeldoutArgs, mhx_types.hpp).
enum { kHoNone = 0, kHoOne = 1, kHoShared = 2, kHoScalar = 3, kHoPlane = 4 };
inline size_t heldout_elems(int kind, int64_t n, int64_t m) {
  switch (kind) {
    case kHoOne: return 1;
    case kHoShared: return (size_t)m;
    case kHoScalar: return (size_t)n;
    case kHoPlane: return (size_t)n * (size_t)m;
    default: return 0;
  }
}
inline int64_t heldout_pitch(int kind, int64_t m) { return kind == kHoPlane ? m : kind == kHoScalar ? 1 : 0; }
inline int heldout_step(int kind) { return kind == kHoShared || kind == kHoPlane ? 1 : 0; }

// The kinds of ys, w, c and the use bytes for a likelihood and the shapes of the caller's arrays.
//   normal forms  w = 1/sigma and c follow sigma; ys = y * w is a plane as soon as either factor is
//                 the chain's own
//   Poisson       ys = y and c = -log-factorial(y) follow y; w is one 0.0, as the dataset's
//   expression    ys = y; w = sigma, handed over as `error` untouched (none: one 1.0); no constant
struct HeldoutLayout {
  int ys = kHoShared, w = kHoOne, c = kHoNone, use = kHoNone;
};
inline HeldoutLayout heldout_layout(int lik, int y_per_chain, int sigma_kind, bool with_use, int use_per_chain) {
  const int by_y = y_per_chain ? kHoPlane : kHoShared;
  const int by_sigma = sigma_kind == MHX_SIGMA_SHARED      ? kHoShared
                       : sigma_kind == MHX_SIGMA_PER_CHAIN ? kHoScalar
                       : sigma_kind == MHX_SIGMA_PER_POINT ? kHoPlane
                                                           : kHoOne;
  HeldoutLayout L;
  L.use = !with_use ? kHoNone : use_per_chain ? kHoPlane : kHoShared;
  if (lik == MHX_LIK_POISSON) {
    L.ys = L.c = by_y, L.w = kHoOne;
  } else if (lik == MHX_LIK_EXPR) {
    L.ys = by_y, L.w = by_sigma, L.c = kHoNone;
  } else {
    L.w = L.c = by_sigma;
    L.ys = (y_per_chain || by_sigma == kHoScalar || by_sigma == kHoPlane) ? kHoPlane : kHoShared;
  }
  return L;
}

// What mhx_set_dataset refuses of a dataset of this likelihood, over all of the caller's arrays
// (n_chains chains, m points), naming the index in the caller's own array.  0, or -1 with msg filled.
inline int heldout_validate(int lik, const double* y, int y_per_chain, const double* sigma, int sigma_kind,
                            int64_t n_chains, int64_t m, char* msg, size_t cap) {
  const size_t C = (size_t)n_chains, M = (size_t)m;
  if (lik == MHX_LIK_POISSON) {
    const size_t ny = y_per_chain ? C * M : M;
    for (size_t i = 0; i < ny; ++i)
      if (!(y[i] >= 0.0) || y[i] != std::floor(y[i]) || y[i] > 1e9) {
        snprintf(msg, cap, "poisson count y[%zu] = %g is not a non-negative integer", i, y[i]);
        return -1;
      }
    return 0;
  }
  if (lik == MHX_LIK_EXPR) return 0;
  const size_t ns = sigma_kind == MHX_SIGMA_SHARED      ? M
                    : sigma_kind == MHX_SIGMA_PER_CHAIN ? C
                    : sigma_kind == MHX_SIGMA_PER_POINT ? C * M
                                                        : 0;
  for (size_t i = 0; i < ns; ++i)
    if (!(sigma[i] > 0.0) || !std::isfinite(sigma[i])) {
      snprintf(msg, cap, "sigma[%zu] = %g must be finite and > 0 (M:376)", i, sigma[i]);
      return -1;
    }
  return 0;
}

// The caller's arrays, read by (chain, point)
struct HeldoutData {
  const double* y = nullptr;
  const double* sigma = nullptr;
  const uint8_t* use = nullptr;
  int y_per_chain = 0, sigma_kind = MHX_SIGMA_NONE, use_per_chain = 0;
  int64_t m = 0;  // points of a row
  double y_at(int64_t c, int64_t i) const { return y[(y_per_chain ? c * m : 0) + i]; }
  double sigma_at(int64_t c, int64_t i) const {
    switch (sigma_kind) {
      case MHX_SIGMA_SHARED: return sigma[i];
      case MHX_SIGMA_PER_CHAIN: return sigma[c];
      case MHX_SIGMA_PER_POINT: return sigma[c * m + i];
      default: return 1.0;  // (if data-error data-error 1) M:1144
    }
  }
  uint8_t use_at(int64_t c, int64_t i) const { return use[(use_per_chain ? c * m : 0) + i]; }
};

// every element of an array of `kind` for n chains from c0 and mc points from m0: at(chain, point)
template <class T, class At>
void heldout_each(int kind, int64_t c0, int64_t n, int64_t m0, int64_t mc, T* out, At&& at) {
  const int64_t rows = kind == kHoScalar || kind == kHoPlane ? n : kind == kHoNone ? 0 : 1;
  const int64_t cols = kind == kHoShared || kind == kHoPlane ? mc : 1;
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t p = 0; p < cols; ++p) out[r * cols + p] = at(c0 + r, m0 + p);
}

// The prepared arrays of chains [c0, c0 + n) at points [m0, m0 + mc), each of heldout_elems(kind,
// n, mc) elements: the arithmetic of mhx_set_dataset, element by element (one division, one
// product; libm's log; the log-factorial in the form the engine was configured with).
inline void heldout_fill(int lik, bool logfact_double, const HeldoutLayout& L, const HeldoutData& D, int64_t c0,
                         int64_t n, int64_t m0, int64_t mc, double* ys, double* w, double* c, uint8_t* use,
                         std::vector<float>& lf_cache) {
  const double half_log_2pi = -0.5 * std::log(2.0 * M_PI);  // (* -1/2 (log (* 2 pi))) M:377
  if (lik == MHX_LIK_POISSON) {
    heldout_each(L.ys, c0, n, m0, mc, ys, [&](int64_t ch, int64_t i) { return D.y_at(ch, i); });
    heldout_each(L.w, c0, n, m0, mc, w, [&](int64_t, int64_t) { return 0.0; });
    heldout_each(L.c, c0, n, m0, mc, c, [&](int64_t ch, int64_t i) {
      return -log_factorial_ref((long)D.y_at(ch, i), logfact_double, lf_cache);
    });
  } else if (lik == MHX_LIK_EXPR) {
    heldout_each(L.ys, c0, n, m0, mc, ys, [&](int64_t ch, int64_t i) { return D.y_at(ch, i); });
    heldout_each(L.w, c0, n, m0, mc, w, [&](int64_t ch, int64_t i) { return D.sigma_at(ch, i); });
  } else {
    heldout_each(L.ys, c0, n, m0, mc, ys, [&](int64_t ch, int64_t i) {
      const double wi = 1.0 / D.sigma_at(ch, i);
      return D.y_at(ch, i) * wi;
    });
    heldout_each(L.w, c0, n, m0, mc, w, [&](int64_t ch, int64_t i) { return 1.0 / D.sigma_at(ch, i); });
    heldout_each(L.c, c0, n, m0, mc, c, [&](int64_t ch, int64_t i) {
      return half_log_2pi + (-1.0 * std::log(D.sigma_at(ch, i)));
    });
  }
  heldout_each(L.use, c0, n, m0, mc, use,
               [&](int64_t ch, int64_t i) { return (uint8_t)(D.use_at(ch, i) != 0 ? 1 : 0); });
}

// Held-out scores of n chains at m points of a call of nb_total blocks: what depends on the chains
// alone comes first and keeps its place from one chunk of points to the next - status, n_used,
// n_scored [n], the total lpd [n], the blocks' partial sums and counts [n][nb_total] - then the
// chunk's x0, x1 [m], the prepared ys, w, c (doubles) and use (bytes), each of its kind's size, and
// the pointwise results the caller asked for: pw_lpd [n][m], pw_acc [n][m][4] (want bits 1, 2; a
// piece not asked for is empty and the kernel does not write it).
enum { HELDOUT_WANT_LPD = 1, HELDOUT_WANT_ACC = 2 };
struct HeldoutPieces {
  size_t status, n_used, n_scored, lpd, part_lpd, part_scored, x0, x1, ys, w, c, use, pw_lpd, pw_acc;
};
inline HeldoutPieces carve_heldout(Carver& cv, int64_t nb_total, int want, const HeldoutLayout& L, int64_t n_,
                                   int64_t m_) {
  const size_t n = (size_t)n_, m = (size_t)m_, nb = (size_t)nb_total;
  HeldoutPieces s;
  s.status = cv.take(n * sizeof(int32_t));
  s.n_used = cv.take(n * sizeof(int32_t));
  s.n_scored = cv.take(n * sizeof(int32_t));
  s.lpd = cv.take(n * sizeof(double));
  s.part_lpd = cv.take(n * nb * sizeof(double));
  s.part_scored = cv.take(n * nb * sizeof(int32_t));
  s.x0 = cv.take(m * sizeof(double));
  s.x1 = cv.take(m * sizeof(double));
  s.ys = cv.take(heldout_elems(L.ys, n_, m_) * sizeof(double));
  s.w = cv.take(heldout_elems(L.w, n_, m_) * sizeof(double));
  s.c = cv.take(heldout_elems(L.c, n_, m_) * sizeof(double));
  s.use = cv.take(heldout_elems(L.use, n_, m_));
  s.pw_lpd = cv.take((want & HELDOUT_WANT_LPD) ? n * m * sizeof(double) : 0);
  s.pw_acc = cv.take((want & HELDOUT_WANT_ACC) ? n * m * 4 * sizeof(double) : 0);
  return s;
}

}  // namespace mhx
