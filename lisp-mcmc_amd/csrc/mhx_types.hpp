// mhx_types.hpp -- structures shared by the host engine and the gfx950 kernels.
//
// Data layout in HBM (all IEEE binary64 unless noted):
//   dataset k      x[n_pad] y[n_pad] (= y/sigma for the normal likelihoods) w[n_pad] (c[n_pad] for the cutoff likelihood), each a
//                  separate 256-B aligned array padded to a whole number of tiles; w = 1/sigma;
//                  pads are (x_last, 0, 0) so a padded point adds exactly +0 to the sum.
//   chain state    theta[C][d], prob[C], best_theta[C][d], best_prob[C], length/age/draw[C]
//   history ring   hist_prob[C][R], hist_theta[C][R][d]; n_hist[C] = entries ever pushed,
//                  entry e lives in slot e % R; the walk of the reference (M:471, newest first)
//                  is entries n_hist-1, n_hist-2, ...
//   controller     L[C][d][d] row-major, temperature[C], loop_i[C], flags
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#include "../../include/mhx.h"

namespace mhx {

constexpr int kWave = 64;
// The device code is compiled in two FAMILIES that differ in the chains (= waves) per workgroup,
// and with it in the LDS tile (2 * 64 * waves points: one 16-B LDS-DMA element per thread and
// array):
//   w8   8 waves, 1024-point tiles, two workgroups per CU: short datasets, few chains
//   w16 16 waves, 2048-point tiles, one workgroup per CU: half the per-tile fixed cost (barrier,
//        pipeline prologue), +9 % on BASELINE config 2, -17 % on test.lisp's 334 points
// The engine picks one per problem (mhx_engine.cpp: choose_family).  Datasets are padded to
// kPadPoints, a whole number of tiles of either family.
constexpr int tile_points_of(int waves_per_group) { return 2 * kWave * waves_per_group; }
constexpr int kPadPoints = tile_points_of(16);
constexpr int kMaxArrays = 4;               // x, y, w, c

struct FnDesc {
  int32_t model, lik, n_idx, n_bounds;
  int32_t shape[4];
  int32_t idx[MHX_MAX_FN_PARAMS];
  int32_t bidx[MHX_MAX_BOUNDS];
  double blo[MHX_MAX_BOUNDS];
  double bhi[MHX_MAX_BOUNDS];
  const double* x;
  const double* y;
  const double* w;  // 1/sigma (normal), unused (poisson)
  const double* c;  // -1/2 log(2 pi) - log sigma_i (cutoff only)
  int64_t n;        // points
  int64_t n_tiles;  // ceil(n / tile points of the family in use)
  double lik_const; // normal: sum_i(-1/2 log 2pi - log sigma_i); poisson: -sum_i logfact(k_i)
  double xmin, xmax; // range of x over the n points (fast-path preconditions of the models)
  double grid_H;     // 64 h when x is a uniform grid x_0 + i h (to 8 ulp of max |x|), else 0: the
                     // distance between two successive points of one lane (Gaussian recurrence)
  const double* txlo;  // [ceil(n / kPadPoints)] smallest / largest x of each 2048-point window (-inf /
  const double* txhi;  // +inf when it holds a non-finite x): what tile-level peak skipping tests against
  int32_t tile_skip;   // 0: evaluate every peak for every point (MHX_NO_TILE_SKIP=1)
  int32_t solo;        // 1: the problem's only function and a single tile - it stays in LDS
                       // 2: a dataset per walker (mhx_set_dataset_planes): c points to a PlaneDesc
  int32_t user_slot;  // >= 0: index of the run-time compiled expression model (MHX_MODEL_EXPR)
  int32_t prior_slot; // >= 0: index of the run-time compiled prior body, else -1
  int32_t no_yw;      // 1: never take the two-array "yw" tiles of the all-recurrence steps (MHX_NO_YW=1)
  int32_t n_xcols;    // columns of x the dataset brought (mhx_set_dataset_cols): with 2, c holds x1
  // per-window grids: [ceil(n / kPadPoints)] 64 h of every 2048-point window whose x are a grid
  // x_w + i h (to 8 ulp of its max |x|), 0 where they are not; nullptr when the WHOLE dataset is
  // one grid (grid_H != 0) or no window is.  Runs of windows on one grid carry the same bits.
  const double* tgh;
};

// A dataset per walker (mhx_set_dataset_planes; include/mhx.h states the sum).  x is the
// function's own, shared array (FnDesc::x, padded as ever); every walker brings
//   y          [n_rows][pitch]  y/sigma of walker r in row r, pads 0; pitch = n padded to 128
//   w          kPlaneWPlane: [n_rows][pitch] 1/sigma, pads 0;  kPlaneWScalar: [n_rows], one
//              1/sigma per walker (MHX_SIGMA_PER_CHAIN; MHX_SIGMA_NONE: 1.0);  kPlaneWShared:
//              unused - the function's shared FnDesc::w serves every walker
//   lik_const  [n_rows]  sum_i(-1/2 log 2pi - log sigma_i) of walker r
// FnDesc::c of such a function (FnDesc::solo == 2) points to this, in device memory.  Only
// programs compiled at run time with MHX_PLANES read it (mhx_kernels.hpp: planes_loglik).
// resident != 0: the arrays fit GroupLds::tiles (mhx_plan.hpp: planes_resident) - the shared ones
// at off_x / off_w, wave s of the workgroup's own at off_rows + s * row_stride (y, then w when it
// is a plane), all counted in doubles.  bit: the function's flag in GroupLds::resident.
enum { kPlaneWShared = 0, kPlaneWScalar = 1, kPlaneWPlane = 2 };
constexpr int kPlanePad = 2 * kWave;  // a lane takes two points per iteration of the sum
struct PlaneDesc {
  const double* y;
  const double* w;
  const double* lik_const;
  int64_t n_rows, pitch;
  int32_t w_kind, resident, bit;
  int32_t off_x, off_w, off_rows, row_stride;
};

struct ProblemDesc {
  int32_t d, K;
  int32_t no_deal;  // 1: wave w judges the proposal of its own chain (MHX_NO_DEAL=1; group_logpost)
  int32_t test_lose_sweepers;  // 1 (test library only): k_persist's sweep workgroups leave at once,
                               // as if they had never got onto the GPU
  FnDesc fn[MHX_MAX_FUNCTIONS];
};

// per-chain state, structure of arrays
struct ChainState {
  int64_t n_chains;
  int64_t chain_offset;  // global id of local chain 0
  int32_t d, R;          // R = history ring capacity
  uint64_t seed;
  double* theta;
  double* prob;
  double* best_theta;
  double* best_prob;
  int64_t* length;  // (walker-length w)
  int64_t* age;     // (walker-age w)
  uint64_t* draw;   // proposals drawn so far: Philox counter
  int64_t* n_hist;
  double* hist_prob;
  double* hist_theta;
  // controller
  double* L;
  double* temperature;
  int64_t* loop_i;
  int64_t* reset_index;
  int32_t* shutting;
  int32_t* status;
  // scratch for the adaptation tick
  int32_t* fwd_idx;  // [C][sts]
  double* mat_tmp;   // [C][2][d][d]
  // pooled-mode statistics [C][1 + d + d*d]: (n, sum delta, sum delta delta^T) of the chain's
  // forward-step displacements; pool_vec [1 + d + d*d] = their sum over chains (and ranks);
  // L_pool [d][d] = (2.38^2/d) * chol(pooled covariance); pool_valid = 1 when usable
  double* pool_stats;
  double* pool_vec;
  double* L_pool;
  int32_t* pool_valid;
  unsigned long long* step_counter;  // chain-steps taken by all chains (device atomic)
  // split mode (few chains, long datasets: one chain's likelihood sum is spread over many
  // workgroups, mhx_kernels.hpp "split mode"): the outstanding proposal of every chain and the
  // partial sums of its functions, one per (slice, wave) slot
  double* split_prop;      // [C][d]
  double* split_u;         // [C] the accept uniform drawn with the proposal
  int32_t* split_pending;  // [C] 1: split_prop / split_u hold a proposal to be judged
  double* split_part;      // [C][K][split_slots]
  int32_t split_slots;
  // the stepping kernel's wave slots -> chains (batch mode, per-walker adaptation): chains that
  // have finished give their slots up (mhx_engine.cpp, compact_slots): entry -1 = empty slot.
  // nullptr: slot s is chain s
  const int32_t* slot_chain;
  int64_t n_slots;  // entries of slot_chain
  int32_t split_pad_;
  // persistent split mode (k_persist: ONE launch runs many iterations of a handful of chains
  // spread over the GPU); both zeroed by the host before every launch
  // persist_msg [C][64] 64-bit words: the chain's proposal as four 128-byte lines of 15
  // parameters and one generation tag each (element j at word (j / 15) * 16 + j % 15, tags at
  // words 15, 31, 47, 63); persist_part [C][K][split_slots] 16-byte pairs {partial sum,
  // generation}.  A 128-byte line / a 16-byte pair is written and read by ONE memory
  // instruction that goes to the level every XCD sees (sc1): who finds the tag finds the data.
  unsigned long long* persist_msg;
  void* persist_part;
  // set by a master whose sweep workgroups did not answer within its patience (they were not all
  // on the GPU - another kernel held it): the iteration is taken back, the launch ends, the host
  // reports it (MHX_EDEVICE) and goes back to the two-launch form
  int32_t* persist_error;
};

// nth-percentile's position rule (M:1495-1506, include/mhx.h: mhx_percentile_rank) for the
// n = num/den per cent point of `len` sorted values: q = num (len-1) / (100 den) exactly;
// pos = floor(q), between = q has a fractional part.  The caller has checked len >= 1,
// den >= 1, 0 <= num <= 100 den (all products then fit 64 bits).
#ifndef __HIPCC_RTC__
#ifdef __HIPCC__
__host__ __device__
#endif
inline void percentile_rank_of(int64_t len, int32_t num, int32_t den,
                        int64_t* pos, int32_t* between) {
  const int64_t a = (int64_t)num * (len - 1), b = (int64_t)100 * den;
  *pos = a / b;
  *between = a % b != 0 ? 1 : 0;
}
#endif

// the percentiles one mhx_get_percentiles call asks for (a kernel argument)
struct PctList {
  int32_t n;
  int32_t num[MHX_MAX_PERCENTILES], den[MHX_MAX_PERCENTILES];
};

// the parameters one mhx_get_histograms / mhx_get_pair_grids call bins (a kernel argument):
// idx[c] = the parameter of column c, of_param[p] = the column of parameter p or -1
struct ColList {
  int32_t n;
  int32_t idx[MHX_MAX_PARAMS + 1], of_param[MHX_MAX_PARAMS + 1];
};

// one task of a pass of mhx_get_ensemble_percentiles (k_ensemble_digits reads a list of them):
// count, by their 8-bit digit at `shift`, the keys of column `col` (a place in the call's
// ColList) whose bits above the digit equal `prefix`; in the successor pass `prefix` is a whole
// key and the task asks for the least key above it
struct EnsTask {
  uint64_t prefix;
  int32_t col, shift;
};
constexpr int kEnsBins = 256;  // counters of a task: one per value of a digit
enum { ENS_COUNT_FIRST = 0, ENS_COUNT = 1, ENS_SUCCESSOR = 2 };  // k_ensemble_digits' modes

// walker-get-data-and-fit's count of enveloped steps, (ceiling (* 0.66 take)) M:1250
// (include/mhx.h: mhx_band_count): 0.66 is a single float and so is the product.
#ifndef __HIPCC_RTC__
#ifdef __HIPCC__
__host__ __device__
#endif
inline int64_t band_count_of(int64_t take) {
  const float p = 0.66f * (float)take;
  return (int64_t)__builtin_ceilf(p);
}
#endif

// The data of one function as each chain reads its own, from the first point of a launch on: what
// k_resid, k_normeq and k_cand are given (data_view, mhx_stage.hpp, builds it on the host).  x0, x1,
// y, w come offset to the launch's first point, and the data are on the device in full: index -1 is
// the point before it.  Chain c, counted from the engine's chain 0 as the planes' rows are, reads
//   ys_i = y[c * y_pitch + i]               y_pitch 0: the shared dataset; a plane's pitch else
//   w_i  = w[c * w_pitch + i * w_step]      (0, 1) the shared 1/sigma - the shared dataset's and
//                                           kPlaneWShared's; (1, 0) one per walker, kPlaneWScalar:
//                                           w is NOT offset to the first point; (pitch, 1) a plane
//                                           of them, kPlaneWPlane
// so that one kernel serves shared datasets and all three PlaneDesc::w_kinds.  y_row(c), w_row(c):
// the rows these index.  The three kernel bodies write the two products out, member by member, as
// they did before there was a view: through the accessors three k_resid instances and one k_cand
// came out of the compiler with other VGPR counts (poly2, poly8: 56 -> 50; generic 106 -> 108;
// k_cand pvoigt2 107 -> 100), the same as ever without them.
#ifdef __HIPCC__
#define MHX_HOST_DEVICE __host__ __device__
#else
#define MHX_HOST_DEVICE
#endif
struct DataView {
  const double* x0;
  const double* x1;  // the second column of x, or nullptr
  const double* y;
  const double* w;
  int64_t y_pitch, w_pitch;
  int32_t w_step, pad_;
  MHX_HOST_DEVICE const double* y_row(int64_t c) const { return y + c * y_pitch; }
  MHX_HOST_DEVICE const double* w_row(int64_t c) const { return w + c * w_pitch; }
};

// k_fit (mhx_eval_function, mhx_get_fit_bands): the model of function `fn` at m points for n
// items.  An item is ONE parameter vector (sel == nullptr: row row0 + i of theta; ymax receives
// the values) or a chain's selected steps (rows row0 + i rows_per_item + sel[i sel_pitch + k],
// k < n_sel[i]; ymax / ymin receive the envelope).  A wave serves one item and one chunk of
// kWave x kFitPts points; n_chunks chunks cover m.
constexpr int kFitPts = 8;  // x a lane keeps in registers, with a running max and min each
struct FitArgs {
  const double* theta;
  const int32_t* sel;
  const int32_t* n_sel;
  int64_t row0, n;
  int32_t rows_per_item, sel_pitch, fn, n_chunks;
  const double* x0;  // [m]
  const double* x1;  // [m] the second column of x, or nullptr
  int64_t m;
  double* ymax;      // [n][m]
  double* ymin;      // [n][m] or nullptr
  int32_t* status;   // [n] set to 1 where a value is not finite (zeroed by the host), or nullptr
};
// dynamic LDS of k_fit for a family of `wpg` waves per workgroup: the math tables, then per wave
// the parameter vector and the model's scratch (FitLds, mhx_kernels.hpp)
constexpr unsigned fit_lds_bytes(int wpg) {
  return 6144u + (unsigned)wpg * (MHX_MAX_PARAMS + 1 + MHX_MAX_FN_PARAMS + 4) * 8u;
}

// k_waic (mhx_get_waic): per data point of function `fn`, the log-sum-exp and the Welford moments
// of the log-likelihood terms over the window of each of n chains from c0 on.  A wave serves one
// chain and one block of MHX_WAIC_BLOCK = kWave x kWaicPts points; n_blocks blocks cover the m
// points of this launch, which are blocks blk0 .. of the function's nb_total.  The dataset's
// arrays come offset to the launch's first point: y and w as the sweep reads them (y/sigma and
// 1/sigma for the normal forms), c the per-point constants (nullptr: none, MHX_LIK_EXPR).
// kWaicPts = 4: a lane keeps nine doubles per point (x0, x1, ys, w, c, M, S, mean, M2) where
// k_fit keeps four: 72 VGPRs before the model has one.  The kernel runs in workgroups of 8 waves
// (two per SIMD), so what counts is how many WHOLE workgroups the registers leave a CU: two up to
// 128 VGPRs (4 waves per SIMD), one above (2 waves per SIMD, whatever the compiler's "3" says).
// As compiled for gfx950 with 4 points no instance uses scratch; config 2's two-peak kernel takes
// 117 VGPRs and the polynomials 114: two workgroups a CU, as their k_fit.  The five-peak Poisson,
// pvoigt2 and lorder instances take 139 to 145 and the generic kernel 185: one workgroup a CU
// (pvoigt2's and the generic k_fit are there already; Poisson's and lorder's k_fit, at 123 and
// 124, still fit two).  With 8 points the arrays alone are 144 VGPRs: EVERY instance, the flagship
// included, would fall to one workgroup a CU, for the sake of halving a per-step prepare that
// 256 points share already.  MHX_WAIC_BLOCK must divide kFitChunkPoints, so the choice is among
// powers of two.
constexpr int kWaicPts = MHX_WAIC_BLOCK / kWave;
static_assert(kWaicPts * kWave == MHX_WAIC_BLOCK && kWaicPts == 4, "MHX_WAIC_BLOCK (include/mhx.h)");
struct WaicArgs {
  int64_t c0, n;
  int32_t take, fn, n_blocks, pad_;
  int64_t blk0, nb_total, m;
  const double* x0;
  const double* x1;  // the second column of x, or nullptr
  const double* y;
  const double* w;
  const double* c;
  double* pw_lppd;     // [n][m] or nullptr
  double* pw_p;        // [n][m] or nullptr
  double* pw_acc;      // [n][m][4] or nullptr
  double* part_lppd;   // [n][nb_total] the blocks' sums of pw_lppd
  double* part_p;      // [n][nb_total] ... of pw_p
  int32_t* part_high;  // [n][nb_total] points of the block with pw_p > 0.4
  int32_t* status;     // [n] MHX_WAIC_NONFINITE is stored where a value or a term is not finite
};

// k_heldout (mhx_get_heldout): k_waic over data the caller handed in.  Per point of the launch's m,
// the log-sum-exp of the log-likelihood terms and the Welford moments of the model VALUES over the
// window of each of n chains from c0 on; a wave serves one chain and one block of MHX_HELDOUT_BLOCK
// = kWave x kWaicPts points, blocks blk0 .. of the call's nb_total.  The host prepares ys, w and c
// (mhx_heldout.hpp) and uploads them per portion, so a row is counted from the LAUNCH's first chain
// and the arrays begin at the launch's first point.  Item i reads, in DataView's manner,
//   ys_p  = ys[i * y_pitch + p]                y_pitch 0: one y for every chain
//   w_p   = w[i * w_pitch + p * w_step]        (0, 1) shared; (1, 0) a scalar per chain; (pitch, 1)
//                                              a plane; (0, 0) one number for all (no sigma)
//   c_p   = c[i * c_pitch + p * c_step]        the same; c nullptr: none (MHX_LIK_EXPR)
//   use_p = use[i * use_pitch + p] != 0        use nullptr: every point
// so one instance serves shared and per-chain data.  Four accumulators a point, as k_waic (the
// value moments take the place of the term moments, and there is no pw_p), and one byte for the use
// flags (bits of one register): the register budget of kWaicPts above applies.  As compiled for
// gfx950: config 2's two-peak instance 113 VGPRs and the polynomials 110 and 111 (two workgroups a
// CU, as their k_waic), five-peak Poisson 143, pvoigt2 145, lorder 139, the generic kernel 185 (one
// workgroup a CU, as their k_waic); no instance uses scratch.  The value moments are taken right
// behind Spec::values, ahead of the term: with them in the log-sum-exp's loop, where k_waic has
// its term moments, a value lived across the exponentials and every instance took 20 VGPRs more
// (two-peak 137: one workgroup a CU).
static_assert(MHX_HELDOUT_BLOCK == MHX_WAIC_BLOCK, "mhx_get_heldout's sums follow mhx_get_waic's rule");
struct HeldoutArgs {
  int64_t c0, n;
  int32_t take, fn, n_blocks, w_step;
  int64_t blk0, nb_total, m;
  const double* x0;
  const double* x1;  // the second column of x, or nullptr
  const double* ys;
  const double* w;
  const double* c;       // or nullptr
  const unsigned char* use;  // or nullptr
  int64_t y_pitch, w_pitch, c_pitch, use_pitch;
  int32_t c_step, pad_;
  double* pw_lpd;        // [n][m] or nullptr
  double* pw_acc;        // [n][m][4] or nullptr
  double* part_lpd;      // [n][nb_total] the blocks' sums of pw_lpd
  int32_t* part_scored;  // [n][nb_total] the blocks' counts of used points
  int32_t* status;       // [n] MHX_HELDOUT_NONFINITE is stored where a used value or term is not finite
};

// k_fitpct_values (mhx_get_fit_percentiles): the model of function `fn` at m points for every step
// of the window of each of n chains from c0 on, and the Welford moments of those values per point.
// A wave serves one chain and one block of MHX_FITPCT_BLOCK = kWave x kFitPctPts points; n_blocks
// blocks cover m.  The value of point p at the step s-th from newest goes to
// values[i * take * m + s * vs_step + p * vs_point]: vs_step = m, vs_point = 1 lays a step's
// points side by side (the stores of a wave are whole lines; the selection transposes on its way
// into LDS), vs_step = 1, vs_point = take lays a point's steps side by side.
// kFitPctPts = 2.  Registers would allow k_fit's 8: a lane keeps four doubles per point (x0, x1,
// mean, M2), what k_fit keeps (x0, x1, max, min), and as compiled for gfx950 with 8 points the
// two-peak instance took 118 VGPRs and none used scratch.  But the values are staged, `take`
// doubles per chain and point, and the stage budget (mhx_stage.hpp: 64 MiB) bounds the points in
// flight, not the registers: at take 1000 a portion is 8 388 (chain, point) pairs, which is 16
// waves of 512 points - two workgroups on a GPU of 256 CUs - or 66 waves of 128.  A wave's time
// is its window's steps, one after the other, whatever it holds; fewer points per lane shorten
// the step and spread the portion over more CUs.  Below 2 a step is shorter than the latency of
// the next step's parameter row, which is the only load in flight.  MHX_FITPCT_BLOCK must divide
// kFitChunkPoints, so the choice is among powers of two.
constexpr int kFitPctPts = MHX_FITPCT_BLOCK / kWave;
static_assert(kFitPctPts * kWave == MHX_FITPCT_BLOCK && kFitPctPts == 2, "MHX_FITPCT_BLOCK (include/mhx.h)");
struct FitPctArgs {
  int64_t c0, n;
  int32_t take, fn, n_blocks, pad_;
  int64_t m, vs_step, vs_point;
  const double* x0;  // [m]
  const double* x1;  // [m] the second column of x, or nullptr
  double* values;    // [n][take * m]
  double* mean;      // [n][m]
  double* stddev;    // [n][m]
  int32_t* status;   // [n] MHX_FITPCT_NONFINITE is or-ed in where a value is not finite
};

// mhx_get_loo's tail length M for a window of n steps (include/mhx.h: mhx_loo_tail_length), in
// integer arithmetic: min(n / 5, R) with R the least integer whose square reaches 9 n, or
// min(tail_len, n / 5) where the caller shortens the tail; below 5 there is no tail.
#ifndef __HIPCC_RTC__
#ifdef __HIPCC__
__host__ __device__
#endif
inline int32_t loo_tail_length_of(int64_t n, int32_t tail_len) {
  if (n < 0) n = 0;
  if (n > ((int64_t)1 << 40)) n = (int64_t)1 << 40;  // (far beyond where MHX_LOO_MAX_TAIL decides)
  int64_t m = n / 5;
  if (tail_len > 0) {
    m = m < (int64_t)tail_len ? m : (int64_t)tail_len;
  } else {
    int64_t r = 0;
    while (r < MHX_LOO_MAX_TAIL && r * r < 9 * n) ++r;
    m = m < r ? m : r;
  }
  if (m > MHX_LOO_MAX_TAIL) m = MHX_LOO_MAX_TAIL;
  return m < 5 ? 0 : (int32_t)m;
}
#endif

// k_loo_values (mhx_get_loo): k_waic's walk with the log-sum-exp pair alone in registers; every
// step's likelihood term of every point goes to the portion's stage piece for k_loo_fit, laid out
// as k_fitpct_values lays its values: the term of point p at the step s-th from newest at
// terms[i * take * m + s * m + p], a step's points side by side.  A wave serves one chain and one
// block of kLooValBlock = kWave x kLooValPts points; n_blocks such blocks cover m.
// kLooValPts = 2, k_fitpct_values' choice and for its reason: the terms are staged, `take` doubles
// per chain and point, so the 64 MiB of a portion bound the points in flight (8 chains of 1000
// points at take 1000), a wave's time is its window's steps one after the other whatever it holds,
// and fewer points per lane spread the portion over more waves.  Measured at that shape with 4
// points per lane (k_waic's): 888 ms of k_loo_values against k_fitpct_values' 505 ms.  The sums'
// block, MHX_LOO_BLOCK = kWave x kLooPts, is k_loo_block_sums' alone; a chunk of points is whole
// blocks of either.
constexpr int kLooPts = MHX_LOO_BLOCK / kWave;
static_assert(kLooPts * kWave == MHX_LOO_BLOCK && kLooPts == 4, "MHX_LOO_BLOCK (include/mhx.h)");
static_assert(MHX_LOO_BLOCK == MHX_WAIC_BLOCK, "mhx_get_loo's sums follow mhx_get_waic's rule");
constexpr int kLooValPts = 2;
constexpr int kLooValBlock = kWave * kLooValPts;
static_assert(MHX_LOO_BLOCK % kLooValBlock == 0, "a chunk of points is whole blocks of the value kernel too");
struct LooArgs {
  int64_t c0, n;
  int32_t take, fn, n_blocks, pad_;
  int64_t m;
  const double* x0;
  const double* x1;  // the second column of x, or nullptr
  const double* y;
  const double* w;
  const double* c;
  double* terms;     // [n][take * m]
  double* pw_lppd;   // [n][m]
  int32_t* status;   // [n] MHX_LOO_NONFINITE is or-ed in where a value or a term is not finite
};

// k_resid (mhx_get_residuals): function `fn` at ONE parameter vector per chain over the chain's own
// data, for each of n chains from c0 on, and the block sums, counts and extreme of the standardized
// residuals.  A wave serves one chain and one block of MHX_RESID_BLOCK = kWave x kResidPts points;
// n_blocks blocks cover the m points of this launch, which are blocks blk0 .. of the function's
// nb_total and begin at point p_first of the dataset.  The chain's data come as a DataView; its
// index -1 is what the first block of a later chunk reads for its neighbour.  theta [n][d] is the
// launch's (nullptr: ChainState::best_theta).  A lane keeps five points - its four and, in a fifth
// slot, the block's neighbour (the last point of the block before, recomputed from the same inputs:
// the same bits) - so that ONE Spec::values with one prepare serves both.
constexpr int kResidPts = MHX_RESID_BLOCK / kWave;
static_assert(kResidPts * kWave == MHX_RESID_BLOCK && kResidPts == 4, "MHX_RESID_BLOCK (include/mhx.h)");
static_assert(MHX_RESID_BLOCK == MHX_WAIC_BLOCK, "mhx_get_residuals' sums follow mhx_get_waic's rule");
struct ResidArgs {
  int64_t c0, n;
  int32_t fn, n_blocks;
  int64_t blk0, nb_total, m, p_first;
  double z_limit;
  const double* theta;  // [n][d] or nullptr
  DataView data;
  double* fit;          // [n][m] or nullptr
  double* z;            // [n][m] or nullptr
  double* part_chi2;    // [n][nb_total] the blocks' sums of z^2
  double* part_sumz;    // [n][nb_total] ... of z
  double* part_dw;      // [n][nb_total] ... of (z_i - z_{i-1})^2
  double* part_max;     // [n][nb_total] the blocks' greatest |z| (-1.0: none)
  int64_t* part_idx;    // [n][nb_total] ... and its place in the dataset (-1: none)
  int32_t* part_cnt;    // [n][nb_total][3] z > 0, changes of sign, |z| > z_limit
  int32_t* status;      // [n] MHX_RESID_NONFINITE is stored where a value or a residual is not finite
};

// k_normeq (mhx_get_normal_equations): the scaled Jacobian g by central differences, the weighted
// residual u and the block sums of their products, for function `fn` at ONE parameter vector per
// chain over the chain's own data (read through a DataView).  A wave serves one chain
// and one block of MHX_NORMEQ_BLOCK points, in sub-steps of `sub` = kNormEqPts * `lanes` <= 256
// points (a lane evaluates kNormEqPts = 4 of them, as k_waic: k_normeq_body says why) whose rows
// {g_i0 .. g_i,p-1, u_i} lie point-major in the wave's LDS tile, `pitch` doubles apart.  The p
// columns are the distinct places of theta the function reads, col[] ascending; a TASK is a pair
// (a <= b) of the p + 1 columns of a row - a, b < p an entry of jtj, b == p one of jtr, a == b == p
// chi2 - in the order k = b (b + 1) / 2 + a.  Lane l keeps tasks l, l + 64, ... in registers.
// part [n][nb_total][n_tasks] receives the blocks' sums; k_normeq_totals adds them in block order.
//   pitch  odd, >= p + 1: the 16 lanes of a ds_write_b64 group, `pitch` doubles apart, fall on 16
//          different pairs of the 32 write banks; a phase-2 ds_read_b64 has all lanes in ONE row of
//          at most 33 doubles (66 dwords of the 64 read banks): equal addresses broadcast, and only
//          columns 0 and 32 of the widest tile share a bank
//   sub    what keeps the workgroup's LDS inside kNormEqLdsBudget, a CU's 160 KiB: all 64 lanes
//          have points up to p = 8 in the family of 8 waves, one workgroup a CU
constexpr int kNormEqCols = MHX_MAX_FN_PARAMS + 1;
constexpr int kNormEqMaxTasks = kNormEqCols * (kNormEqCols + 1) / 2;  // 561
constexpr int kNormEqLaneTasks = (kNormEqMaxTasks + kWave - 1) / kWave;  // 9
constexpr unsigned kNormEqLdsBudget = 160u * 1024u;
constexpr int kNormEqPts = 4;  // points a lane evaluates in one Spec::values
static_assert(kNormEqLaneTasks == 9, "nine tasks a lane at MHX_MAX_FN_PARAMS columns");
constexpr int normeq_tasks(int p) { return (p + 1) * (p + 2) / 2; }
constexpr int normeq_pitch(int p) { return (p + 1) | 1; }
constexpr int normeq_lanes(int wpg, int p) {  // lanes of a wave that have points in a sub-step
  const unsigned per_point = (unsigned)wpg * (unsigned)normeq_pitch(p) * 8u;
  const unsigned fit = (kNormEqLdsBudget - fit_lds_bytes(wpg)) / per_point / (unsigned)kNormEqPts;
  return fit >= (unsigned)kWave ? kWave : (int)fit;
}
constexpr int normeq_sub(int wpg, int p) { return kNormEqPts * normeq_lanes(wpg, p); }
constexpr unsigned normeq_lds_bytes(int wpg, int p) {
  return fit_lds_bytes(wpg) + (unsigned)wpg * (unsigned)normeq_sub(wpg, p) * (unsigned)normeq_pitch(p) * 8u;
}
static_assert(normeq_lanes(16, MHX_MAX_FN_PARAMS) >= 8 && normeq_lanes(8, 8) == kWave, "normeq_lanes");
static_assert(MHX_NORMEQ_BLOCK % (kNormEqPts * kWave) == 0, "whole sub-steps at the widest");
struct NormEqArgs {
  int64_t c0, n;
  int32_t fn, n_blocks, p, n_tasks;
  int32_t pitch, steps_pitch;  // steps_pitch 0: one [d] for all chains; d: [n][d]
  int32_t sub, lanes;          // (the launcher's: they depend on the kernel's family)
  int64_t blk0, nb_total, m;
  int32_t col[MHX_MAX_FN_PARAMS];  // [p] the places of theta the function reads, ascending
  const double* theta;  // [n][d] or nullptr
  const double* steps;  // [d] or [n][d]
  DataView data;
  double* g;            // [n][d][m] or nullptr (zeroed by the host: the kernel writes active columns)
  double* part;         // [n][nb_total][n_tasks]
  int32_t* status;      // [n] MHX_NORMEQ_NONFINITE is stored where a value is not finite
};

// k_cand (mhx_get_candidate_scores): function `fn` at m_cand parameter vectors per chain over the
// chain's own data (read through a DataView), for each of n chains from c0 on.
// A wave serves one chain and one block of MHX_RESID_BLOCK points: it loads the block's points
// once, kResidPts per lane, and walks the candidates - cand[j] (cand_pitch 0: one [m_cand][d] for
// every chain) or cand[i * cand_pitch + j] of the launch's chain i - each through the wave's LDS row,
// the next one's load in flight.  The block's sum of z^2 goes to
//   part[(i * m_cand + j) * nb_pitch + blk0 + block]
// where nb_pitch is the blocks of ALL the call's functions and blk0 this function's first; a block
// with a value or residual that is not finite stores a NaN.  k_cand_totals adds a candidate's
// blocks function by function and ranks the chain's candidates.
struct CandArgs {
  int64_t c0, n;
  int32_t fn, n_blocks;
  int64_t m_cand, cand_pitch;  // cand_pitch in candidates: 0 or m_cand
  int64_t blk0, nb_pitch, m;
  const double* cand;  // [m_cand][d] or [n][m_cand][d]
  DataView data;
  double* part;        // [n][m_cand][nb_pitch]
};

// mhx_user_derived (mhx_get_derived, mhx_derived.hpp): the expressions of one run-time compiled
// module over the windows of the n chains from c0 on.  idx[j] = the place in theta of the j-th
// name; values [n][n_expr][pitch] newest first, at_best [n][n_expr] (the most-likely step).
struct DerivedArgs {
  int64_t c0, n;
  int32_t take, pitch;
  int32_t idx[MHX_MAX_PARAMS + 1];
  double* values;
  double* at_best;
};
constexpr int kDerivedThreads = 256;  // one workgroup of four waves per chain, as k_percentiles
constexpr unsigned kDerivedLdsBytes = 6144u;  // its dynamic LDS: LdsHead, the math tables

// The span of a highest-density interval (include/mhx.h: mhx_hdi_span): of n sorted values, a mass
// of num/den per cent reaches from s_j to s_{j+g}, g = min(floor(n num / (100 den)), n - 1), in
// exact integers.  n = a D + b with D = 100 den and b < D gives a num + floor(b num / D): no
// product leaves 64 bits.  The caller has checked n >= 1, 1 <= den <= 10^6, 1 <= num <= 100 den.
#ifndef __HIPCC_RTC__
#ifdef __HIPCC__
__host__ __device__
#endif
inline int64_t hdi_span_of(int64_t n, int32_t num, int32_t den) {
  const int64_t D = (int64_t)100 * den, a = n / D, b = n % D;
  const int64_t g = a * num + b * num / D;
  return g < n - 1 ? g : n - 1;
}
#endif
// k_hdi (mhx_get_hdi, mhx_get_derived_hdi): the windows of the chains from c0 on, nc columns each.
// The source of the columns: the ring's parameters cl.idx[c] (vals NULL), or a staged array - the
// value of step s (newest first) of column c of the launch's chain i is
// vals[i * vals_chain + c * vals_col + s * vals_step] (cl then only counts the columns).
//   use_lds = 1: one workgroup per chain, a column's keys in `tpad` slots of LDS, `tpad + 1` apart
//   use_lds = 0: one workgroup per (chain, column), the keys in keys [n][nc][tpad]
// tpad is a power of two >= 2 and >= take.  lo, hi, pos [n][n_mass][nc], ladder [n][nc][n_ladder],
// n_used [n], status [n][nc].
struct HdiArgs {
  int64_t c0;
  int32_t take, n_mass, n_ladder, use_lds, tpad;
  int32_t mass_num[MHX_MAX_HDI_MASSES], mass_den[MHX_MAX_HDI_MASSES];
  ColList cl;
  const double* vals;
  int64_t vals_chain, vals_col, vals_step;
  unsigned long long* keys;
  double *lo, *hi;
  int32_t* pos;
  double* ladder;
  int32_t *n_used, *status;
};
constexpr int kHdiChunk = 4096;  // keys of a sub-sequence that k_hdi's memory path finishes in LDS

struct RunDesc {
  int64_t n, sts, temp_steps, mwl, tail;
  int32_t auto_mode, has_mwl, adapt_mode;
  const double* temps;  // entries [temps_first, temps_first + window) of the schedule: the host
  int64_t temps_first;  // keeps the window over the loop indices of the launch (mhx_engine.cpp)
  const int32_t* stop_flag;
};

}  // namespace mhx
