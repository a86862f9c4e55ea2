// mhx_derived.hpp -- the device half of mhx_get_derived that depends on the user's expressions:
// walker-with-exp (M:1052-1064) for every step of every chain's window.  Included only by the
// run-time compiled module mhx_user_derived (mhx_rtc.cpp: generate_derived), never by the
// stepping programs and never by the ahead-of-time units; the summaries of the values are
// k_derived_summary's (mhx_readout_kernels.hpp), which needs no expression.
#pragma once
#include "mhx_kernels.hpp"

namespace mhx {
inline namespace MHX_FAMILY {

// One workgroup of kDerivedThreads per chain (as k_percentiles).  Thread j takes the WHOLE steps
// j, j + kDerivedThreads, ... of the window, newest first: neighbouring lanes read neighbouring
// rows of the ring, so the window's t x d doubles - one contiguous run, two where the ring has
// wrapped - come in once, line by line; a lane loads only the parameters the module names
// (Exprs::kP, their places in theta in A.idx), evaluates all Exprs::kN expressions and stores
// the values at [q][s] of the chain's staging block: unit stride across the lanes.
// The step behind the window's last, s == t, stands for the chain's most-likely step
// (:most-likely-params M:511-515: best_theta / best_prob, the walker's own, whatever take is).
// gexp / tlog read their tables at LDS address 0: dynamic LDS = LdsHead, no static LDS.
static_assert(sizeof(LdsHead) == kDerivedLdsBytes, "kDerivedLdsBytes (mhx_types.hpp)");
template <class Exprs>
__device__ __forceinline__ void k_derived_body(const ChainState& S, const DerivedArgs& A) {
  lds_tables_begin();
  __syncthreads();
  const int64_t i = blockIdx.x;
  if (i >= A.n) return;
  const int64_t c = A.c0 + i;
  const int d = S.d;
  Ring r;
  r.prob = S.hist_prob + c * S.R;
  r.theta = S.hist_theta + c * S.R * d;
  r.mask = S.R - 1;
  r.d = d;
  r.nh = uniform_i64(S.n_hist[c]);
  r.length = uniform_i64(S.length[c]);
  int64_t held = r.length < r.nh ? r.length : r.nh;
  if (held > (int64_t)A.take) held = A.take;
  const int t = (int)(held < 0 ? 0 : held);
  constexpr int kP = Exprs::kP > 0 ? Exprs::kP : 1;
  for (int s = threadIdx.x; s <= t; s += kDerivedThreads) {
    const bool best = s == t;
    const int slot = r.slot(best ? 0 : s);
    const double* row = best ? S.best_theta + c * d : r.theta + (int64_t)slot * d;
    const double prob = best ? S.best_prob[c] : r.prob[slot];
    double p[kP], g[Exprs::kN];
#pragma unroll
    for (int j = 0; j < Exprs::kP; ++j) p[j] = row[A.idx[j]];
    Exprs::eval(p, prob, g);
    if (best) {
      if (A.at_best) {
#pragma unroll
        for (int q = 0; q < Exprs::kN; ++q) A.at_best[i * Exprs::kN + q] = g[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < Exprs::kN; ++q)
        A.values[(i * Exprs::kN + q) * (int64_t)A.pitch + s] = g[q];
    }
  }
}

}  // inline namespace MHX_FAMILY
}  // namespace mhx
