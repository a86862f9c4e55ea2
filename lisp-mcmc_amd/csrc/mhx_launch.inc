// mhx_launch.inc -- included at the end of mhx_kernels.hip: spec table + launchers.
#include "mhx_launch.hpp"

#define MHX_CAT2(a, b) a##b
#define MHX_CAT(a, b) MHX_CAT2(a, b)

namespace mhx {
inline namespace MHX_FAMILY {

using Spec0 = GenericSpec;
using Spec1 = FixedSpec<PeaksModel<2, 2, false>, MHX_LIK_NORMAL>;
using Spec2 = FixedSpec<PeaksModel<1, 5, false>, MHX_LIK_POISSON>;
using Spec3 = FixedSpec<PVoigt2Model, MHX_LIK_NORMAL>;
using Spec4 = FixedSpec<PolyModel<2>, MHX_LIK_NORMAL>;
using Spec5 = FixedSpec<PolyModel<8>, MHX_LIK_NORMAL>;
using Spec6 = FixedSpec<LorderModel, MHX_LIK_NORMAL>;
using Spec7 = FixedSpec<PeaksModel<2, 2, false>, MHX_LIK_NORMAL_CUTOFF>;
#ifdef MHX_AOT_G23
using Spec8 = FixedSpec<PeaksModel<2, 3, false>, MHX_LIK_NORMAL>;  // (experiment: g23 ahead of time)
#endif

template <class F>
static inline void for_spec(int spec, F&& f) {
  switch (spec) {
    case 1: f(Spec1{}); break;
    case 2: f(Spec2{}); break;
    case 3: f(Spec3{}); break;
    case 4: f(Spec4{}); break;
    case 5: f(Spec5{}); break;
    case 6: f(Spec6{}); break;
    case 7: f(Spec7{}); break;
#ifdef MHX_AOT_G23
    case 8: f(Spec8{}); break;
#endif
    default: f(Spec0{}); break;
  }
}


static inline dim3 grid_for(int64_t n) {
  return dim3((unsigned)((n + kWavesPerGroup - 1) / kWavesPerGroup));
}

// the device math reads its tables at absolute LDS addresses (mhx_device.hpp): a kernel that
// sweeps must not have static LDS in front of its dynamic LDS
template <class F>
static hipError_t no_static_lds(F* fn) {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(fn));
  if (e == hipSuccess && a.sharedSizeBytes != 0) e = hipErrorInvalidKernelFile;
  return e;
}
template <class F>
static hipError_t set_lds(F* fn) {
  hipError_t e = no_static_lds(fn);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GroupLds));
}

static hipError_t configure_kernels() {
  hipError_t e = hipSuccess;
  for (int s = 0; s < SPEC__COUNT; ++s) {
    for_spec(s, [&](auto sp) {
      using SpecT = decltype(sp);
      if (e == hipSuccess) e = set_lds(&k_logpost<SpecT>);
      if (e == hipSuccess) e = set_lds(&k_init<SpecT>);
      if (e == hipSuccess) e = set_lds(&k_step_injected<SpecT>);
      if (e == hipSuccess) e = set_lds(&k_adaptive<SpecT>);
      if (e == hipSuccess) e = set_lds(&k_split_step<SpecT>);
      if (e == hipSuccess) e = no_static_lds(&k_split_sweep<SpecT>);
      if (e == hipSuccess) e = set_lds(&k_split_tsweep<SpecT>);
      if constexpr (SpecT::kSplit) {
        if (e == hipSuccess) e = set_lds(&k_persist<SpecT>);
        if (e == hipSuccess) e = set_lds(&k_persist_ts<SpecT>);
      }
    });
  }
  if (e == hipSuccess) e = set_lds(&k_initial_l);
  return e;
}

static hipError_t launch_logpost(int spec, hipStream_t st, const ProblemDesc* P, const double* theta,
                          int64_t n, double* out, double* parts) {
  if (n <= 0) return hipSuccess;
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_logpost<SpecT><<<grid_for(n), dim3(kThreads), sizeof(GroupLds), st>>>(P, theta, n, out, parts);
  });
  return hipGetLastError();
}

static hipError_t launch_init(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_init<SpecT><<<grid_for(S.n_chains), dim3(kThreads), sizeof(GroupLds), st>>>(P, S);
  });
  return hipGetLastError();
}

static hipError_t launch_step_injected(int spec, hipStream_t st, const ProblemDesc* P,
                                const ChainState& S, const double* L, int per_chain_l,
                                const double* z, const double* u, const double* T,
                                unsigned char* accepted) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_step_injected<SpecT><<<grid_for(S.n_chains), dim3(kThreads), sizeof(GroupLds), st>>>(
        P, S, L, per_chain_l, z, u, T, accepted);
  });
  return hipGetLastError();
}

static hipError_t launch_adaptive(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                           const RunDesc& R, int64_t max_iters, int plain) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_adaptive<SpecT><<<grid_for(S.slot_chain ? S.n_slots : S.n_chains), dim3(kThreads),
                        sizeof(GroupLds), st>>>(
        P, S, R, max_iters, plain);
  });
  return hipGetLastError();
}

static hipError_t launch_initial_l(hipStream_t st, const ChainState& S, const RunDesc& R, int have_l,
                            double T0) {
  k_initial_l<<<grid_for(S.n_chains), dim3(kThreads), sizeof(GroupLds), st>>>(S, R, have_l, T0);
  return hipGetLastError();
}

static hipError_t launch_l_matrix(hipStream_t st, const ChainState& S, int64_t chain, int take, int* fwd,
                           double* cov, double* out, int* info) {
  k_l_matrix<<<dim3(1), dim3(kWave), 0, st>>>(S, chain, take, fwd, cov, out, info);
  return hipGetLastError();
}

static hipError_t launch_acceptance(hipStream_t st, const ChainState& S, int take, double* out) {
  k_acceptance<<<grid_for(S.n_chains), dim3(kThreads), 0, st>>>(S, take, out);
  return hipGetLastError();
}

static hipError_t launch_pool_stats(hipStream_t st, const ChainState& S, const RunDesc& R) {
  k_pool_stats<<<grid_for(S.n_chains), dim3(kThreads), 0, st>>>(S, R);
  return hipGetLastError();
}
static hipError_t launch_pool_reduce(hipStream_t st, const ChainState& S) {
  k_pool_reduce<<<dim3(1 + S.d + S.d * S.d), dim3(256), 0, st>>>(S);
  return hipGetLastError();
}
static hipError_t launch_modify(hipStream_t st, const ChainState& S, int action, int64_t n) {
  k_modify<<<grid_for(S.n_chains), dim3(kThreads), 0, st>>>(S, action, n);
  return hipGetLastError();
}
static hipError_t launch_pool_factor(hipStream_t st, const ChainState& S) {
  k_pool_factor<<<dim3(1), dim3(kWave), 0, st>>>(S);
  return hipGetLastError();
}
static bool split_capable(int spec) {
  bool ok = false;
  for_spec(spec, [&](auto sp) { ok = decltype(sp)::kSplit; });
  return ok;
}
static hipError_t launch_split_sweep(int spec, hipStream_t st, const ProblemDesc* P,
                                     const ChainState& S, int slices) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_split_sweep<SpecT><<<dim3((unsigned)slices, (unsigned)S.n_chains), dim3(kThreads),
                           kSweepLdsBytes, st>>>(P, S);
  });
  return hipGetLastError();
}
static hipError_t launch_split_tsweep(int spec, hipStream_t st, const ProblemDesc* P,
                                      const FnDesc* slices, const ChainState& S, int n_slices) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_split_tsweep<SpecT><<<dim3((unsigned)n_slices,
                                 grid_for(S.slot_chain ? S.n_slots : S.n_chains).x), dim3(kThreads),
                            sizeof(GroupLds), st>>>(P, slices, S, n_slices);
  });
  return hipGetLastError();
}
static hipError_t launch_split_step(int spec, hipStream_t st, const ProblemDesc* P,
                                    const ChainState& S, const RunDesc& R, int mode, int plain) {
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    k_split_step<SpecT><<<grid_for(S.slot_chain ? S.n_slots : S.n_chains), dim3(kThreads),
                          sizeof(GroupLds), st>>>(
        P, S, R, mode, plain);
  });
  return hipGetLastError();
}
static hipError_t launch_persist(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                                 const RunDesc& R, int slices, int64_t max_iters, int plain) {
  hipError_t e = hipSuccess;
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    if constexpr (SpecT::kSplit) {
      k_persist<SpecT><<<dim3(1u + (unsigned)slices, (unsigned)S.n_chains), dim3(kThreads),
                         sizeof(GroupLds), st>>>(P, S, R, max_iters, plain);
    } else {
      e = hipErrorInvalidValue;
    }
  });
  return e != hipSuccess ? e : hipGetLastError();
}
static int persist_per_cu(int spec, int ts) {
  int n = 0;
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    if constexpr (SpecT::kSplit) {
      const hipError_t e =
          ts ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_persist_ts<SpecT>, kThreads, sizeof(GroupLds))
             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_persist<SpecT>, kThreads, sizeof(GroupLds));
      if (e != hipSuccess) n = 0;
    }
  });
  return n;
}
static hipError_t launch_persist_ts(int spec, hipStream_t st, const ProblemDesc* P,
                                    const FnDesc* slices, const ChainState& S, const RunDesc& R,
                                    int n_slices, int64_t max_iters, int plain) {
  hipError_t e = hipSuccess;
  for_spec(spec, [&](auto sp) {
    using SpecT = decltype(sp);
    if constexpr (SpecT::kSplit) {
      k_persist_ts<SpecT><<<dim3(1u + (unsigned)n_slices,
                                 grid_for(S.slot_chain ? S.n_slots : S.n_chains).x), dim3(kThreads),
                            sizeof(GroupLds), st>>>(P, slices, S, R, n_slices, max_iters, plain);
#ifdef MHX_PERSIST_TIMING
      static unsigned long long h[1024][8];
      (void)hipStreamSynchronize(st);
      (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_persist_trace), sizeof(h));
      const unsigned gx = 1u + (unsigned)n_slices, gy = grid_for(S.slot_chain ? S.n_slots : S.n_chains).x;
      for (unsigned y = 0; y < gy; ++y)
        for (unsigned x = 0; x < gx && y * gx + x < 1024; ++x) {
          const unsigned long long* r = h[y * gx + x];
          const unsigned long long n = r[6] ? r[6] : 1;
          fprintf(stderr, "trace wg %u %u xcc %llu se %llu cu %llu n %llu a %llu b %llu c %llu end %llu\n", x, y, r[0],
                  r[1], r[2], r[6], r[3] / n, r[4] / n, r[5] / n, r[7]);
        }
#endif
    } else {
      e = hipErrorInvalidValue;
    }
  });
  return e != hipSuccess ? e : hipGetLastError();
}
}  // inline namespace MHX_FAMILY

const Family& MHX_CAT(family_, MHX_FAMILY)() {
  static const Family f = {kWavesPerGroup,       kThreads,          kTilePoints,
                           sizeof(GroupLds),     kSweepLdsBytes,    configure_kernels, launch_logpost,
                           launch_init,          launch_step_injected, launch_adaptive,
                           launch_initial_l,     launch_l_matrix,   launch_acceptance,
                           launch_pool_stats,    launch_pool_reduce, launch_pool_factor,
                           launch_modify,        split_capable,     launch_split_sweep,
                           launch_split_tsweep,  launch_split_step, launch_persist, persist_per_cu, launch_persist_ts};
  return f;
}

#ifdef MHX_FAMILY_PRIMARY  // family-independent helpers: defined by one unit only
hipError_t summary_configure() {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_percentiles),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_derived_summary),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_histograms),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pair_grids),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_autocorr),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ensemble_digits),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fitpct_select),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  if (e == hipSuccess) e = no_static_lds(&k_loo_fit);  // (gexp and tlog read their tables at LDS address 0)
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_loo_fit),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPctLdsBudget);
  return e;
}
hipError_t launch_percentiles(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              const PctList& pc, bool use_lds, double* out, int32_t* n_used) {
  if (n <= 0) return hipSuccess;
  const size_t lds = use_lds ? pct_lds_bytes(take, S.d) : 0;
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_percentiles<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, c0, take, pc, use_lds ? 1 : 0, pct_column_pitch(take, S.d), out, n_used);
  return hipGetLastError();
}
hipError_t launch_derived_summary(hipStream_t st, const ChainState& S, int64_t c0, int64_t n,
                                  int take, int ne, const PctList& pc, bool use_lds,
                                  const double* vals, double* pct, double* mean, double* stddev,
                                  int32_t* n_used, int32_t* status) {
  if (n <= 0) return hipSuccess;
  const size_t lds = use_lds ? pct_lds_bytes(take, ne) : 0;
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_derived_summary<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, c0, take, ne, take, pc, use_lds ? 1 : 0, pct_column_pitch(take, ne), vals, pct, mean,
      stddev, n_used, status);
  return hipGetLastError();
}
hipError_t launch_histograms(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             const ColList& cl, int nb, const double* edges, int64_t edge_stride,
                             bool use_lds, int32_t* counts, int32_t* outside, int32_t* n_used,
                             int32_t* status) {
  if (n <= 0) return hipSuccess;
  const size_t lds = use_lds ? histo_lds_bytes(cl.n, nb) : 0;
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_histograms<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, c0, take, cl, nb, edges, edge_stride, use_lds ? 1 : 0, histo_count_pitch(nb), counts,
      outside, n_used, status);
  return hipGetLastError();
}
hipError_t launch_pair_grids(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             const ColList& cl, int nb, int np, const double* edges,
                             int64_t edge_stride, const int32_t* pairs, bool use_lds,
                             int32_t* counts, int32_t* n_inside, int32_t* n_used, int32_t* status) {
  if (n <= 0) return hipSuccess;
  const size_t lds = use_lds ? grid_lds_bytes(take, cl.n, nb, np) : 0;
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_pair_grids<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, c0, take, cl, nb, np, edges, edge_stride, pairs, use_lds ? 1 : 0, grid_place_pitch(take),
      counts, n_inside, n_used, status);
  return hipGetLastError();
}
hipError_t launch_autocorr(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                           const ColList& cl, int max_lag, bool use_lds, double* acf, double* tau,
                           double* ess, double* half_mean, double* half_var, int32_t* n_lags,
                           int32_t* n_used, int32_t* status) {
  static_assert(kAcTail == 256, "autocorr_lds_bytes leaves 256 doubles after the last column");
  if (n <= 0) return hipSuccess;
  const size_t lds = autocorr_lds_bytes(take, cl.n, use_lds);
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_autocorr<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, c0, take, cl, max_lag, use_lds ? 1 : 0, pct_column_pitch(take, cl.n), acf, tau, ess,
      half_mean, half_var, n_lags, n_used, status);
  return hipGetLastError();
}
hipError_t launch_ensemble_digits(hipStream_t st, const ChainState& S, int64_t n, int take,
                                  const ColList& cl, const uint8_t* include, const EnsTask* tasks,
                                  int n_tasks, int mode, bool use_lds, uint64_t* counters,
                                  int32_t* n_used, int32_t* nan_flag) {
  static_assert(kPctWaves == 4, "ensemble_lds_bytes counts four histograms");
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
  if (n <= 0 || n_tasks <= 0) return hipSuccess;
  const size_t lds = ensemble_lds_bytes(take, cl.n, use_lds);
  if (lds > kPctLdsBudget) return hipErrorInvalidValue;
  k_ensemble_digits<<<dim3((unsigned)n), dim3(kPctThreads), lds, st>>>(
      S, take, cl, include, tasks, n_tasks, mode, use_lds ? 1 : 0, pct_column_pitch(take, cl.n),
      reinterpret_cast<unsigned long long*>(counters), n_used, nan_flag);
  return hipGetLastError();
}
hipError_t launch_hdi(hipStream_t st, const ChainState& S, int64_t n, const HdiArgs& A) {
  if (n <= 0 || A.cl.n <= 0) return hipSuccess;
  if (A.tpad != hdi_pad(A.take)) return hipErrorInvalidValue;
  const size_t lds = A.use_lds ? hdi_lds_bytes(A.take, A.cl.n) : (size_t)std::min(A.tpad, kHdiChunk) * sizeof(uint64_t);
  const int64_t groups = A.use_lds ? n : n * A.cl.n;
  static_assert(kHdiLdsBudget <= 64 * 1024 && kHdiChunk * sizeof(uint64_t) <= 64 * 1024, "no more LDS than a kernel has unasked");
  if ((A.use_lds && lds > kHdiLdsBudget) || groups > 0x7fffffff || (!A.use_lds && !A.keys)) return hipErrorInvalidValue;
  k_hdi<<<dim3((unsigned)groups), dim3(kPctThreads), lds, st>>>(S, A);
  return hipGetLastError();
}
hipError_t launch_covariances(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int* uniq, double* cov, int32_t* n_unique, int32_t* status) {
  if (n <= 0) return hipSuccess;
  k_covariances<<<grid_for(n), dim3(kThreads), 0, st>>>(S, c0, n, take, uniq, cov, n_unique, status);
  return hipGetLastError();
}
hipError_t launch_traces(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                         int filter, int stride, int start, int n_cols, int max_out,
                         const int32_t* cols, int* kept, double* values, double* lo, double* hi,
                         int32_t* n_out, int32_t* n_kept, int32_t* n_used) {
  if (n <= 0) return hipSuccess;
  k_traces<<<grid_for(n), dim3(kThreads), 0, st>>>(S, c0, n, take, filter, stride, start, n_cols,
                                                  max_out, cols, kept, values, lo, hi, n_out, n_kept,
                                                  n_used);
  return hipGetLastError();
}
hipError_t launch_l_matrices(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             int* fwd, double* cov, double* out, int32_t* status,
                             int32_t* n_forward) {
  if (n <= 0) return hipSuccess;
  k_l_matrices<<<grid_for(n), dim3(kThreads), 0, st>>>(S, c0, n, take, fwd, cov, out, status,
                                                      n_forward);
  return hipGetLastError();
}
hipError_t launch_window_best(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              double* prob, double* theta) {
  if (n <= 0) return hipSuccess;
  k_window_best<<<grid_for(n), dim3(kThreads), 0, st>>>(S, c0, n, take, prob, theta);
  return hipGetLastError();
}

// ---- the model read-outs (MHX_MODEL_READOUTS, mhx_launch.hpp): one configure and one launcher
template <class Spec, class Args>
struct ModelKernel;
#define MHX_X(ID, ARGS, KERNEL, ...)                    \
  template <class Spec>                                 \
  struct ModelKernel<Spec, ARGS> {                      \
    static constexpr auto* fn = &KERNEL<Spec>;          \
  };
MHX_MODEL_READOUTS(MHX_X)
#undef MHX_X
template <class Spec, class Args>
static hipError_t configure_model() {
  constexpr auto* fn = ModelKernel<Spec, Args>::fn;
  hipError_t e = no_static_lds(fn);
  if (e == hipSuccess && ModelReadout<Args>::kMaxLds != 0)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)ModelReadout<Args>::kMaxLds);
  return e;
}
hipError_t model_readouts_configure() {
  hipError_t e = hipSuccess;
  for (int s = 0; s < SPEC__COUNT; ++s)
    for_spec(s, [&](auto sp) {
      using SpecT = decltype(sp);
#define MHX_X(ID, ARGS, ...) \
  if (e == hipSuccess) e = configure_model<SpecT, ARGS>();
      MHX_MODEL_READOUTS(MHX_X)
#undef MHX_X
    });
  return e;
}
template <class Args>
hipError_t launch_model(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S, const Args& A) {
  using R = ModelReadout<Args>;
  const int64_t waves = R::waves(A);
  if (waves <= 0) return hipSuccess;
  Args a = A;
  R::fix_up(kWavesPerGroup, a);
  for_spec(spec, [&](auto sp) {
    constexpr auto* fn = ModelKernel<decltype(sp), Args>::fn;
    if constexpr (R::kState)
      fn<<<grid_for(waves), dim3(kThreads), R::lds(kWavesPerGroup, a), st>>>(P, S, a);
    else
      fn<<<grid_for(waves), dim3(kThreads), R::lds(kWavesPerGroup, a), st>>>(P, a);
  });
  return hipGetLastError();
}
#define MHX_X(ID, ARGS, ...) \
  template hipError_t launch_model<ARGS>(int, hipStream_t, const ProblemDesc*, const ChainState&, const ARGS&);
MHX_MODEL_READOUTS(MHX_X)
#undef MHX_X

// mhx_eval_function / mhx_get_fit_bands: the steps every chain's band envelopes (k_band_select)
hipError_t launch_band_select(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int32_t* sel, int32_t* n_sel) {
  if (n <= 0) return hipSuccess;
  k_band_select<<<grid_for(n), dim3(kThreads), 0, st>>>(S, c0, n, take, sel, n_sel);
  return hipGetLastError();
}

// mhx_get_waic: the totals (k_waic_totals)
hipError_t launch_waic_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int64_t nb_total, const double* part_lppd, const double* part_p,
                              const int32_t* part_high, double* elpd, double* lppd, double* p_waic,
                              int32_t* n_high, int32_t* n_used, int32_t* status) {
  if (n <= 0) return hipSuccess;
  k_waic_totals<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
      S, c0, n, take, nb_total, part_lppd, part_p, part_high, elpd, lppd, p_waic, n_high, n_used, status);
  return hipGetLastError();
}

// mhx_get_heldout: the totals (k_heldout_totals)
hipError_t launch_heldout_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                                 int64_t nb_total, const double* part_lpd, const int32_t* part_scored,
                                 double* lpd, int32_t* n_scored, int32_t* n_used, int32_t* status) {
  if (n <= 0) return hipSuccess;
  k_heldout_totals<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
      S, c0, n, take, nb_total, part_lpd, part_scored, lpd, n_scored, n_used, status);
  return hipGetLastError();
}

// mhx_get_residuals: the totals (k_resid_totals)
hipError_t launch_resid_totals(hipStream_t st, int64_t n, int64_t nb_total, const ResidArgs& A,
                               double* chi2, double* sum_z, double* dw, double* max_abs_z,
                               int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out) {
  if (n <= 0) return hipSuccess;
  k_resid_totals<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
      n, nb_total, A.part_chi2, A.part_sumz, A.part_dw, A.part_max, A.part_idx, A.part_cnt, chi2, sum_z, dw,
      max_abs_z, max_index, n_pos, n_runs, n_out);
  return hipGetLastError();
}

// mhx_get_normal_equations: the totals (k_normeq_totals)
hipError_t launch_normeq_totals(hipStream_t st, const NormEqArgs& A, int d, double* jtj, double* jtr,
                                double* chi2) {
  if (A.n <= 0) return hipSuccess;
  const int64_t threads = A.n * A.n_tasks;
  k_normeq_totals<<<dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(A, d, jtj, jtr,
                                                                                                   chi2);
  return hipGetLastError();
}

// mhx_get_candidate_scores: the totals and the ranking (k_cand_totals)
hipError_t launch_cand_totals(hipStream_t st, const ProblemDesc* P, int fn, int64_t n, int64_t m_cand,
                              int64_t nb_pitch, int keep, const double* part, double* score,
                              int32_t* best_index, double* best_score, int32_t* n_bad) {
  if (n <= 0) return hipSuccess;
  k_cand_totals<<<dim3((unsigned)n), dim3(kWave), 0, st>>>(P, fn, n, m_cand, nb_pitch, keep, part, score,
                                                           best_index, best_score, n_bad);
  return hipGetLastError();
}

// mhx_get_fit_percentiles: the model-free selection (k_fitpct_select)
hipError_t launch_fitpct_select(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                                int64_t m, int64_t vs_step, int64_t vs_point, const PctList& pc,
                                bool use_lds, bool together, const double* vals, double* pct,
                                int32_t* n_used, int32_t* status) {
  if (n <= 0 || m <= 0) return hipSuccess;
  const int cols = use_lds ? fitpct_cols(take) : kFitPctMemCols;
  if (cols <= 0) return hipErrorInvalidValue;
  const size_t lds = use_lds ? pct_lds_bytes(take, cols) : 0;
  const int64_t n_groups = (m + cols - 1) / cols;
  if (lds > kPctLdsBudget || n * n_groups > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  k_fitpct_select<<<dim3((unsigned)(n * n_groups)), dim3(kPctThreads), lds, st>>>(
      S, c0, take, m, cols, (int)n_groups, vs_step, vs_point, pc, use_lds ? 1 : 0, together ? 1 : 0,
      pct_column_pitch(take, cols), vals, pct, n_used, status);
  return hipGetLastError();
}


// mhx_get_loo: the model-free fit (k_loo_fit), the block sums and the totals
hipError_t launch_loo_fit(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take, int tail_len,
                          int64_t m, bool use_lds, const double* terms, double* pw_elpd, double* pw_khat,
                          double* pw_acc, double* tail, int32_t* status) {
  static_assert(kLooCols == kLooColsPerGroup && sizeof(LdsHead) == 6144, "loo_lds_bytes (mhx_launch.hpp)");
  if (n <= 0 || m <= 0) return hipSuccess;
  const int P = loo_tail_length_of(take, tail_len);
  const size_t lds = loo_lds_bytes(take, P, use_lds);
  const int64_t n_groups = (m + kLooCols - 1) / kLooCols;
  if (lds > kPctLdsBudget || n * n_groups > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  k_loo_fit<<<dim3((unsigned)(n * n_groups)), dim3(kPctThreads), lds, st>>>(
      S, c0, take, tail_len, m, (int)n_groups, P, loo_p2(P), use_lds ? 1 : 0, pct_column_pitch(take, kLooCols),
      terms, pw_elpd, pw_khat, pw_acc, tail, status);
  return hipGetLastError();
}
hipError_t launch_loo_block_sums(hipStream_t st, int64_t n, int64_t m, int64_t blk0, int64_t nb_total,
                                 double k_limit, const double* pw_elpd, const double* pw_lppd,
                                 const double* pw_khat, double* part_elpd, double* part_lppd,
                                 int32_t* part_high) {
  if (n <= 0 || m <= 0) return hipSuccess;
  const int64_t nb = loo_blocks(m), groups = (n * nb + kPctWaves - 1) / kPctWaves;
  if (groups > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  k_loo_block_sums<<<dim3((unsigned)groups), dim3(kPctThreads), 0, st>>>(
      n, m, (int)nb, blk0, nb_total, k_limit, pw_elpd, pw_lppd, pw_khat, part_elpd, part_lppd, part_high);
  return hipGetLastError();
}
hipError_t launch_loo_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             int64_t nb_total, const double* part_elpd, const double* part_lppd,
                             const int32_t* part_high, double* elpd, double* p_loo, double* lppd,
                             int32_t* n_high, int32_t* n_used, int32_t* status) {
  if (n <= 0) return hipSuccess;
  k_loo_totals<<<dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(
      S, c0, n, take, nb_total, part_elpd, part_lppd, part_high, elpd, p_loo, lppd, n_high, n_used, status);
  return hipGetLastError();
}

#endif

}  // namespace mhx
