// mhx_launch.hpp -- host-callable launchers of the gfx950 kernels (defined in mhx_kernels.hip,
// once per kernel family: see mhx_types.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "mhx_finalize.hpp"
#include "mhx_plan.hpp"
#include "mhx_types.hpp"

namespace mhx {

// (the compiled problem specialisations, SpecId, and their choice: mhx_finalize.hpp)

// One family of kernels: everything that depends on the workgroup shape goes through this table.
struct Family {
  int waves_per_group;  // chains per workgroup
  int threads;          // 64 * waves_per_group
  int tile_points;      // data points per LDS tile and array
  size_t lds_bytes;     // dynamic LDS of the stepping kernels
  size_t sweep_lds_bytes;  // dynamic LDS of the split-mode sweep kernel (the math tables)
  hipError_t (*configure)();
  hipError_t (*logpost)(int spec, hipStream_t st, const ProblemDesc* P, const double* theta,
                        int64_t n, double* out, double* parts);
  hipError_t (*init)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S);
  hipError_t (*step_injected)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                              const double* L, int per_chain_l, const double* z, const double* u,
                              const double* T, unsigned char* accepted);
  hipError_t (*adaptive)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                         const RunDesc& R, int64_t max_iters, int plain);
  hipError_t (*initial_l)(hipStream_t st, const ChainState& S, const RunDesc& R, int have_l,
                          double T0);
  hipError_t (*l_matrix)(hipStream_t st, const ChainState& S, int64_t chain, int take, int* fwd,
                         double* cov, double* out, int* info);
  hipError_t (*acceptance)(hipStream_t st, const ChainState& S, int take, double* out);
  hipError_t (*pool_stats)(hipStream_t st, const ChainState& S, const RunDesc& R);
  hipError_t (*pool_reduce)(hipStream_t st, const ChainState& S);
  hipError_t (*pool_factor)(hipStream_t st, const ChainState& S);
  hipError_t (*modify)(hipStream_t st, const ChainState& S, int action, int64_t n);
  // split mode (mhx_kernels.hpp): the partial sums of every pending proposal over `slices`
  // workgroups per chain, and the two halves of the loop iteration around them
  bool (*split_capable)(int spec);
  hipError_t (*split_sweep)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                            int slices);
  // ... or, tile-sliced (k_split_tsweep): groups of chains on slices of whole windows, `slices` =
  // the device copy of the slice table [K][n_slices]
  hipError_t (*split_tsweep)(int spec, hipStream_t st, const ProblemDesc* P, const FnDesc* slices,
                             const ChainState& S, int n_slices);
  hipError_t (*split_step)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                           const RunDesc& R, int mode, int plain);
  // ... or ONE launch for many iterations of a handful of chains (k_persist): grid (1 + slices,
  // chains), every workgroup resident at once (the caller checks)
  hipError_t (*persist)(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S,
                        const RunDesc& R, int slices, int64_t max_iters, int plain);
  // workgroups of the persistent kernel (ts: the tile-sliced one) a CU holds at once, as the
  // runtime's occupancy calculator sees the compiled kernel (0: not compiled for this spec)
  int (*persist_per_cu)(int spec, int ts);
  // ... the same for the tile-sliced mode (k_persist_ts): grid (1 + n_slices, chain groups)
  hipError_t (*persist_ts)(int spec, hipStream_t st, const ProblemDesc* P, const FnDesc* slices,
                           const ChainState& S, const RunDesc& R, int n_slices, int64_t max_iters,
                           int plain);
};

const Family& family_w8();
const Family& family_w16();

// walker-set-get: summaries of the `n` chains from `c0` on (mhx_readout_kernels.hpp; family-independent,
// compiled once).  Outputs and scratch are indexed by the chain's place in [c0, c0 + n).
// The LDS a percentile workgroup needs for a window of `take` steps of d parameters, and the
// column pitch that goes with it; above kPctLdsBudget the kernel reads its columns from memory.
constexpr size_t kPctLdsBudget = 80 * 1024;  // two workgroups per CU (160 KiB)
inline int pct_column_pitch(int take, int d) {
  return ((take + 15) & ~15) + (d >= 16 ? 1 : 16 / d);
}
inline size_t pct_lds_bytes(int take, int d) {
  return (size_t)d * pct_column_pitch(take, d) * sizeof(double);
}
hipError_t summary_configure();
hipError_t launch_percentiles(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              const PctList& pc, bool use_lds, double* out, int32_t* n_used);
// mhx_get_derived, the summaries (k_derived_summary): vals [n][ne][take] as mhx_user_derived
// left them; the keys of a chain go to LDS where pct_lds_bytes(take, ne) fits kPctLdsBudget
hipError_t launch_derived_summary(hipStream_t st, const ChainState& S, int64_t c0, int64_t n,
                                  int take, int ne, const PctList& pc, bool use_lds,
                                  const double* vals, double* pct, double* mean, double* stddev,
                                  int32_t* n_used, int32_t* status);
// mhx_get_histograms / mhx_get_pair_grids (k_histograms, k_pair_grids): the pitch of a column's
// counts (below, the bins, above; odd) and of a column's 16-bit places (an odd count of 32-bit
// words), and the LDS a workgroup needs for edges + counts (+ places).  Where that exceeds
// kPctLdsBudget the caller passes use_lds = false and zeroed outputs: the counts then go straight
// to memory.  edges: one set [nc][nb + 1] (edge_stride 0) or one per chain of the launch.
inline int histo_count_pitch(int nb) { return (nb + 2) | 1; }
inline int grid_place_pitch(int take) { return 2 * (((take + 1) / 2) | 1); }
inline size_t histo_lds_bytes(int nc, int nb) {
  return (size_t)nc * (nb + 1) * sizeof(double) + ((size_t)nc * histo_count_pitch(nb) + nc) * sizeof(int32_t);
}
inline size_t grid_lds_bytes(int take, int nc, int nb, int np) {
  return (size_t)nc * (nb + 1) * sizeof(double) + ((size_t)np * nb * nb + np + nc) * sizeof(int32_t) +
         (size_t)nc * grid_place_pitch(take) * sizeof(uint16_t);
}
hipError_t launch_histograms(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             const ColList& cl, int nb, const double* edges, int64_t edge_stride,
                             bool use_lds, int32_t* counts, int32_t* outside, int32_t* n_used,
                             int32_t* status);
hipError_t launch_pair_grids(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             const ColList& cl, int nb, int np, const double* edges,
                             int64_t edge_stride, const int32_t* pairs, bool use_lds,
                             int32_t* counts, int32_t* n_inside, int32_t* n_used, int32_t* status);
// mhx_get_autocorr (k_autocorr): the LDS a workgroup needs for nc columns of a window of `take`
// steps - the pitch of k_percentiles, 256 doubles a lane may read past the last column, and a
// mean, a c_0 and a flag per column.  Above kPctLdsBudget, or with use_lds = false, the columns
// stay in memory.  acf [n][nc][max_lag + 1] is written AND read back by the kernel.
inline size_t autocorr_lds_bytes(int take, int nc, bool use_lds) {
  return (use_lds ? ((size_t)nc * pct_column_pitch(take, nc) + 256) * sizeof(double) : 0) +
         (size_t)nc * (2 * sizeof(double) + sizeof(int32_t));
}
hipError_t launch_autocorr(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                           const ColList& cl, int max_lag, bool use_lds, double* acf, double* tau,
                           double* ess, double* half_mean, double* half_var, int32_t* n_lags,
                           int32_t* n_used, int32_t* status);
// mhx_get_ensemble_percentiles (k_ensemble_digits): one pass over ALL the engine's chains.  The
// LDS a workgroup needs: nc columns of keys at the pitch of k_percentiles where use_lds, and a
// 256-bin uint32 histogram for each of its four waves.  Above kPctLdsBudget, or with use_lds =
// false, the columns stay in memory.
inline size_t ensemble_lds_bytes(int take, int nc, bool use_lds) {
  return (use_lds ? (size_t)nc * pct_column_pitch(take, nc) * sizeof(uint64_t) : 0) +
         (size_t)4 * kEnsBins * sizeof(uint32_t);
}
hipError_t launch_ensemble_digits(hipStream_t st, const ChainState& S, int64_t n, int take,
                                  const ColList& cl, const uint8_t* include, const EnsTask* tasks,
                                  int n_tasks, int mode, bool use_lds, uint64_t* counters,
                                  int32_t* n_used, int32_t* nan_flag);
// mhx_get_hdi / mhx_get_derived_hdi (k_hdi) over the n chains from A.c0 on.  The caller chose the
// path (hdi_use_lds, mhx_plan.hpp) and set A.tpad = hdi_pad(A.take); the LDS path takes
// hdi_lds_bytes of LDS, the memory path a sub-sequence of up to kHdiChunk keys.
hipError_t launch_hdi(hipStream_t st, const ChainState& S, int64_t n, const HdiArgs& A);
hipError_t launch_covariances(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int* uniq, double* cov, int32_t* n_unique, int32_t* status);
// mhx_get_traces (k_traces): cols [n_cols] on the device, kept [n][take] scratch, values / lo / hi
// [n][max_out][n_cols] zeroed by the caller (lo, hi: nullptr where not asked for)
hipError_t launch_traces(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                         int filter, int stride, int start, int n_cols, int max_out,
                         const int32_t* cols, int* kept, double* values, double* lo, double* hi,
                         int32_t* n_out, int32_t* n_kept, int32_t* n_used);
hipError_t launch_l_matrices(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             int* fwd, double* cov, double* out, int32_t* status,
                             int32_t* n_forward);
hipError_t launch_window_best(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              double* prob, double* theta);

// ---- The model read-outs: the kernels that evaluate a model for a batched read-out
// (mhx_kernels.hpp).  Each is compiled ahead of time as KERNEL<Spec> for every spec - in the
// primary family only, whichever family steps the problem: a wave is an item and a block of
// points in either - and at run time as the twin mhx_user_ID over the same KERNEL_body.  A wave is
// a unit of work, a workgroup is the family's, and no kernel may have static LDS (the device math
// reads its tables at absolute LDS addresses).  What differs from kernel to kernel is stated here,
// once, and everything that configures, generates, looks up or launches them goes by this list:
//   ID       names the twin, and MR_ID is its handle's place in UserProgram::f_model
//   ARGS     the argument struct (mhx_types.hpp); launch_model(.., A) finds the kernel by its type
//   KERNEL   the kernel template; KERNEL(P, A), or KERNEL(P, S, A) where STATE says it takes ChainState
//   WAVES    the waves a launch needs, of its arguments A (<= 0: nothing to launch)
//   LDS      its dynamic LDS, of the waves per workgroup wpg and A
//   MAX_LDS  what hipFuncAttributeMaxDynamicSharedMemorySize must be raised to (0: the 64 KiB a
//            kernel has unasked are enough)
//   FIX_UP   what the launcher completes in its copy of A, because it depends on wpg
#define MHX_MODEL_READOUTS(X)                                                                                  \
  /* ID      ARGS        KERNEL           STATE  WAVES                             LDS  MAX_LDS  FIX_UP */     \
  X(fit,    FitArgs,    k_fit,           false, A.m <= 0 ? 0 : A.n * A.n_chunks, fit_lds_bytes(wpg), 0, (void)0)    \
  X(waic,   WaicArgs,   k_waic,          true,  A.m <= 0 ? 0 : A.n * A.n_blocks, fit_lds_bytes(wpg), 0, (void)0)    \
  X(resid,  ResidArgs,  k_resid,         true,  A.m <= 0 ? 0 : A.n * A.n_blocks, fit_lds_bytes(wpg), 0, (void)0)    \
  /* (the tile of the widest function takes the LDS past 64 KiB; sub, lanes: normeq_sub says why) */          \
  X(normeq, NormEqArgs, k_normeq,        true,  A.m <= 0 ? 0 : A.n * A.n_blocks, normeq_lds_bytes(wpg, A.p),        \
    kNormEqLdsBudget, (A.lanes = normeq_lanes(wpg, A.p), A.sub = normeq_sub(wpg, A.p)))                        \
  X(cand,   CandArgs,   k_cand,          false, A.m <= 0 || A.m_cand <= 0 ? 0 : A.n * A.n_blocks,              \
    fit_lds_bytes(wpg), 0, (void)0)                                                                            \
  X(fitpct, FitPctArgs, k_fitpct_values, true,  A.m <= 0 ? 0 : A.n * A.n_blocks, fit_lds_bytes(wpg), 0, (void)0)    \
  X(loo,    LooArgs,    k_loo_values,    true,  A.m <= 0 ? 0 : A.n * A.n_blocks, fit_lds_bytes(wpg), 0, (void)0)    \
  X(heldout, HeldoutArgs, k_heldout,     true,  A.m <= 0 ? 0 : A.n * A.n_blocks, fit_lds_bytes(wpg), 0, (void)0)

enum ModelReadoutId {
#define MHX_X(ID, ...) MR_##ID,
  MHX_MODEL_READOUTS(MHX_X)
#undef MHX_X
  MR__COUNT
};
// the list's line of an argument type, for the templated launch paths
template <class Args>
struct ModelReadout;
#define MHX_X(ID, ARGS, KERNEL, STATE, WAVES, LDS, MAX_LDS, FIX_UP)                   \
  template <>                                                                         \
  struct ModelReadout<ARGS> {                                                         \
    static constexpr int kId = MR_##ID;                                               \
    static constexpr bool kState = STATE;                                             \
    static constexpr unsigned kMaxLds = MAX_LDS;                                      \
    static int64_t waves(const ARGS& A) { return WAVES; }                             \
    static unsigned lds(int wpg, const ARGS& A) { return (void)A, LDS; }              \
    static void fix_up(int wpg, ARGS& A) { (void)wpg, (void)A, FIX_UP; }              \
  };
MHX_MODEL_READOUTS(MHX_X)
#undef MHX_X
// The ahead-of-time kernel of A's type for `spec` (S: what a kernel without ChainState leaves
// unread); run-time compiled problems go through rtc_launch_model (mhx_rtc.hpp).
hipError_t model_readouts_configure();
template <class Args>
hipError_t launch_model(int spec, hipStream_t st, const ProblemDesc* P, const ChainState& S, const Args& A);

// mhx_eval_function / mhx_get_fit_bands: the steps every chain's band envelopes (sel [n][take]
// ring slots, n_sel [n]), and the model values / envelopes themselves (FitArgs, mhx_types.hpp)
// through launch_model.
inline int fit_chunks(int64_t m) { return (int)((m + kWave * kFitPts - 1) / (kWave * kFitPts)); }
hipError_t launch_band_select(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int32_t* sel, int32_t* n_sel);

// mhx_get_waic: the pointwise accumulation and the blocks' partial sums (WaicArgs, mhx_types.hpp)
// through launch_model, and the totals of n chains from the partials of all nb_total blocks.
inline int64_t waic_blocks(int64_t m) { return (m + MHX_WAIC_BLOCK - 1) / MHX_WAIC_BLOCK; }
hipError_t launch_waic_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                              int64_t nb_total, const double* part_lppd, const double* part_p,
                              const int32_t* part_high, double* elpd, double* lppd, double* p_waic,
                              int32_t* n_high, int32_t* n_used, int32_t* status);

// mhx_get_heldout: the pointwise accumulation over the caller's data and the blocks' partial sums
// (HeldoutArgs, mhx_types.hpp) through launch_model, and the totals of n chains from the partials
// of all nb_total blocks (blocks of MHX_HELDOUT_BLOCK = MHX_WAIC_BLOCK points: waic_blocks counts them).
hipError_t launch_heldout_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                                 int64_t nb_total, const double* part_lpd, const int32_t* part_scored,
                                 double* lpd, int32_t* n_scored, int32_t* n_used, int32_t* status);

// mhx_get_fit_percentiles: the values and moments (FitPctArgs, mhx_types.hpp) through launch_model,
// and the model-free selection over the staged values.  fitpct_cols: the neighbouring points one
// selection workgroup takes - the most of 8, 4, 2, 1 whose key columns fit kPctLdsBudget (two
// workgroups a CU), 0 where not even one column does: the selection then reads the stage.
// together: a column's percentiles share their passes (select_percentiles_together).
inline int64_t fitpct_blocks(int64_t m) { return (m + MHX_FITPCT_BLOCK - 1) / MHX_FITPCT_BLOCK; }
inline int fitpct_cols(int take) {
  for (int c = 8; c >= 1; c >>= 1)
    if (pct_lds_bytes(take, c) <= kPctLdsBudget) return c;
  return 0;
}
constexpr int kFitPctMemCols = 4;  // ... a workgroup's points on the memory path: one per wave
hipError_t launch_fitpct_select(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                                int64_t m, int64_t vs_step, int64_t vs_point, const PctList& pc,
                                bool use_lds, bool together, const double* vals, double* pct,
                                int32_t* n_used, int32_t* status);

// mhx_get_loo: the staged terms and pw_lppd (LooArgs, mhx_types.hpp) through launch_model, the
// model-free fit of every (chain, point) column, the block sums of a chunk of points and the totals.
// A fit workgroup takes kLooCols = 4 neighbouring points, a wave each.  Its LDS: the math tables,
// per wave the tail's keys and x (two arrays of loo_p2(P) slots), and - where that still fits
// kPctLdsBudget - the four columns' keys (loo_use_lds); else the selection reads the stage.
constexpr int kLooColsPerGroup = 4;
inline int64_t loo_blocks(int64_t m) { return (m + MHX_LOO_BLOCK - 1) / MHX_LOO_BLOCK; }
inline int64_t loo_value_blocks(int64_t m) { return (m + kLooValBlock - 1) / kLooValBlock; }
inline int loo_p2(int P) {
  int p2 = 64;
  while (p2 < P) p2 <<= 1;
  return p2;
}
inline size_t loo_lds_bytes(int take, int P, bool use_lds) {
  return 6144 + (size_t)kLooColsPerGroup * 2 * loo_p2(P) * sizeof(double) +
         (use_lds ? pct_lds_bytes(take, kLooColsPerGroup) : 0);
}
inline bool loo_use_lds(int take, int P) { return loo_lds_bytes(take, P, true) <= kPctLdsBudget; }
hipError_t launch_loo_fit(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take, int tail_len,
                          int64_t m, bool use_lds, const double* terms, double* pw_elpd, double* pw_khat,
                          double* pw_acc, double* tail, int32_t* status);
hipError_t launch_loo_block_sums(hipStream_t st, int64_t n, int64_t m, int64_t blk0, int64_t nb_total,
                                 double k_limit, const double* pw_elpd, const double* pw_lppd,
                                 const double* pw_khat, double* part_elpd, double* part_lppd,
                                 int32_t* part_high);
hipError_t launch_loo_totals(hipStream_t st, const ChainState& S, int64_t c0, int64_t n, int take,
                             int64_t nb_total, const double* part_elpd, const double* part_lppd,
                             const int32_t* part_high, double* elpd, double* p_loo, double* lppd,
                             int32_t* n_high, int32_t* n_used, int32_t* status);

// mhx_get_residuals: the residuals' block sums, counts and extremes (ResidArgs, mhx_types.hpp)
// through launch_model - every engine with a dataset per walker is run-time compiled - and the
// totals of n chains from the partials of all nb_total blocks.
inline int64_t resid_blocks(int64_t m) { return (m + MHX_RESID_BLOCK - 1) / MHX_RESID_BLOCK; }
hipError_t launch_resid_totals(hipStream_t st, int64_t n, int64_t nb_total, const ResidArgs& A,
                               double* chi2, double* sum_z, double* dw, double* max_abs_z,
                               int64_t* max_index, int32_t* n_pos, int32_t* n_runs, int32_t* n_out);

// mhx_get_normal_equations: the block sums of the products of the scaled Jacobian and the residual
// (NormEqArgs, mhx_types.hpp) through launch_model, and the totals of A.n chains from the partials
// of all A.nb_total blocks, scattered into jtj [n][d][d], jtr [n][d] (both zeroed by the caller) and
// chi2 [n].
inline int64_t normeq_blocks(int64_t m) { return (m + MHX_NORMEQ_BLOCK - 1) / MHX_NORMEQ_BLOCK; }
hipError_t launch_normeq_totals(hipStream_t st, const NormEqArgs& A, int d, double* jtj, double* jtr,
                                double* chi2);

// mhx_get_candidate_scores: the blocks' chi-square of every candidate of every chain for one
// function (CandArgs, mhx_types.hpp) through launch_model and, once all selected functions (fn, or
// all of them at -1) have written their blocks, the scores [n][m_cand], the `keep` best of each
// chain and its count of candidates that are not finite.
hipError_t launch_cand_totals(hipStream_t st, const ProblemDesc* P, int fn, int64_t n, int64_t m_cand,
                              int64_t nb_pitch, int keep, const double* part, double* score,
                              int32_t* best_index, double* best_score, int32_t* n_bad);

}  // namespace mhx
