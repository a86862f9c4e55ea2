// mhx_plan.hpp -- which launch form the engine picks for a problem: the environment switches,
// read in one place, and the mode rules as pure functions of plain numbers (no HIP, no engine).
// mhx_engine.cpp fills a ProblemShape when it finalises a problem and allocates for the answer;
// tests/test_launch_plan.py pins every branch of these rules on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "mhx_types.hpp"

namespace mhx {

// The switches that steer finalisation, compaction and launching (README: "Environment knobs").
// A flag is on when the variable is set and atoi() of it is not 0.
struct EngineKnobs {
  int family_wpg = 0;        // MHX_FAMILY_WPG=8|16: pins the kernel family (any other value: ignored, 0)
  bool split_set = false;    // MHX_SPLIT set (even empty): the caller has decided between batch and per-chain split
  int split = 0;             // MHX_SPLIT=<n>: 0 keeps the batch kernels, n caps the per-chain split mode's slices
  bool tsplit_set = false;   // MHX_TSPLIT set (even empty): the tile-sliced slicing is forced, never re-cut
  int tsplit = 0;            // MHX_TSPLIT=<n>: 0 switches the tile-sliced split mode off, n asks for n slices
  bool no_persist = false;   // MHX_NO_PERSIST: never the persistent kernels (k_persist, k_persist_ts)
  int persist_ts = -1;       // MHX_PERSIST_TS: 1 tile-sliced persistent wherever two slices fit, 0 never, -1 unset
  int persist_fill = 100;    // MHX_PERSIST_FILL: per cent of the persistent workgroup slots used (10..100)
  bool no_resident_slices = false;  // MHX_NO_RESIDENT_SLICES: persistent slices fetch their window every round
  bool no_window_grids = false;     // MHX_NO_WINDOW_GRIDS: no per-window grids (one grid or none)
  bool no_tile_skip = false;        // MHX_NO_TILE_SKIP: every Gaussian peak at every point
  bool no_recognise = false;        // MHX_NO_RECOGNISE: every expression compiled as written
  bool no_yw = false;               // MHX_NO_YW: never the two-array "yw" tiles
  bool no_deal = false;             // MHX_NO_DEAL: every wave judges its own chain's proposal
  bool force_generic = false;       // MHX_FORCE_GENERIC: the run-time dispatched generic kernels
  bool no_rtc_specialise = false;   // MHX_NO_RTC_SPECIALISE: no hiprtc kernels for problems without an AOT one
  bool early_reject = false;        // MHX_EARLY_REJECT: sweep()'s exact early rejection where it applies
  bool no_compact = false;          // MHX_NO_COMPACT: never repack or deal the chains over workgroups
  bool compact_always = false;      // MHX_COMPACT_ALWAYS: repack small launches too (tests)
  bool no_graph = false;            // MHX_NO_GRAPH: split-mode kernels issued one by one, no captured graph
  bool summary_no_lds = false;      // MHX_SUMMARY_NO_LDS: k_percentiles reads its columns from memory even where they fit LDS
  bool histo_no_lds = false;        // MHX_HISTO_NO_LDS: k_histograms / k_pair_grids count straight into memory even where LDS would hold them
  bool autocorr_no_lds = false;     // MHX_AUTOCORR_NO_LDS: k_autocorr reads the window from memory even where its columns fit LDS
  bool ensemble_no_lds = false;     // MHX_ENSEMBLE_NO_LDS: k_ensemble_digits reads its columns from memory in every pass even where they fit LDS
  bool fitpct_no_lds = false;       // MHX_FITPCT_NO_LDS: k_fitpct_select reads its columns from the stage in every pass even where they fit LDS
  bool fitpct_select_singly = false;  // MHX_FITPCT_SELECT_SINGLY: k_fitpct_select runs select_percentile once per percentile (the form it was measured against)
  bool fitpct_step_fastest = false; // MHX_FITPCT_STEP_FASTEST: the staged values lie a point's steps side by side (measurement: DESIGN 4.9)
  bool loo_no_lds = false;          // MHX_LOO_NO_LDS: k_loo_fit reads its columns from the staged terms in every pass even where they fit LDS
  bool hdi_no_lds = false;          // MHX_HDI_NO_LDS: k_hdi sorts every window in memory, one workgroup per (chain, column), even where a chain's keys fit LDS
  bool planes_no_lds = false;       // MHX_PLANES_NO_LDS: a dataset per walker is streamed from memory even where it fits LDS
#ifdef MHX_DEBUG_HOOKS
  bool test_lose_sweepers = false;  // MHX_TEST_LOSE_SWEEPERS: k_persist's sweep workgroups never come (test library)
#endif
};

inline EngineKnobs read_knobs() {
  EngineKnobs k;
  const struct { const char* name; bool EngineKnobs::*on; } flags[] = {
      {"MHX_NO_PERSIST", &EngineKnobs::no_persist}, {"MHX_NO_RESIDENT_SLICES", &EngineKnobs::no_resident_slices},
      {"MHX_NO_WINDOW_GRIDS", &EngineKnobs::no_window_grids}, {"MHX_NO_TILE_SKIP", &EngineKnobs::no_tile_skip},
      {"MHX_NO_RECOGNISE", &EngineKnobs::no_recognise}, {"MHX_NO_YW", &EngineKnobs::no_yw},
      {"MHX_NO_DEAL", &EngineKnobs::no_deal}, {"MHX_FORCE_GENERIC", &EngineKnobs::force_generic},
      {"MHX_NO_RTC_SPECIALISE", &EngineKnobs::no_rtc_specialise}, {"MHX_EARLY_REJECT", &EngineKnobs::early_reject},
      {"MHX_NO_COMPACT", &EngineKnobs::no_compact}, {"MHX_COMPACT_ALWAYS", &EngineKnobs::compact_always},
      {"MHX_NO_GRAPH", &EngineKnobs::no_graph}, {"MHX_SUMMARY_NO_LDS", &EngineKnobs::summary_no_lds},
      {"MHX_HISTO_NO_LDS", &EngineKnobs::histo_no_lds}, {"MHX_AUTOCORR_NO_LDS", &EngineKnobs::autocorr_no_lds},
      {"MHX_FITPCT_NO_LDS", &EngineKnobs::fitpct_no_lds}, {"MHX_FITPCT_STEP_FASTEST", &EngineKnobs::fitpct_step_fastest},
      {"MHX_FITPCT_SELECT_SINGLY", &EngineKnobs::fitpct_select_singly}, {"MHX_LOO_NO_LDS", &EngineKnobs::loo_no_lds},
      {"MHX_PLANES_NO_LDS", &EngineKnobs::planes_no_lds}, {"MHX_ENSEMBLE_NO_LDS", &EngineKnobs::ensemble_no_lds},
      {"MHX_HDI_NO_LDS", &EngineKnobs::hdi_no_lds},
#ifdef MHX_DEBUG_HOOKS
      {"MHX_TEST_LOSE_SWEEPERS", &EngineKnobs::test_lose_sweepers},
#endif
  };
  for (const auto& f : flags) {
    const char* v = getenv(f.name);
    k.*f.on = v && atoi(v) != 0;
  }
  if (const char* s = getenv("MHX_FAMILY_WPG")) k.family_wpg = atoi(s) == 16 ? 16 : atoi(s) == 8 ? 8 : 0;
  if (const char* s = getenv("MHX_SPLIT")) k.split_set = true, k.split = atoi(s);
  if (const char* s = getenv("MHX_TSPLIT")) k.tsplit_set = true, k.tsplit = atoi(s);
  if (const char* s = getenv("MHX_PERSIST_TS")) k.persist_ts = atoi(s) != 0 ? 1 : 0;
  if (const char* s = getenv("MHX_PERSIST_FILL")) k.persist_fill = std::max(10, std::min(100, atoi(s)));
  return k;
}

// What the rules read of a problem, worked out once per finalisation.
struct ProblemShape {
  int64_t longest = 0;      // points of the longest dataset
  int64_t nwin = 0;         // its windows of kPadPoints points
  int K = 1, d = 1;         // functions, parameters
  bool heavy = false;       // a point costs 40 instructions and more (Poisson, pseudo-Voigt, expressions)
  int64_t chains = 0;
  bool pooled = false;      // MHX_ADAPT_POOLED: the batch kernels only
  int waves_per_group = 8;  // the kernel family (choose_family) ...
  int tile_points = tile_points_of(8);  // ... and its LDS tile
  bool capable = false;     // the problem's kernels have the split-mode forms
  bool persist_off = false; // a persistent launch of this engine once failed
  int cus = 256;            // compute units of the device
  int per_cu = 0;           // k_persist workgroups a CU holds at once
  int per_cu_ts = 0;        // k_persist_ts workgroups a CU holds at once
  bool planes = false;      // a function has a dataset per walker (mhx_set_dataset_planes): the batch kernels only
};

// the launch form: the batch kernels (split_slices == 0), the per-chain split mode (split_slices
// workgroups per chain) or the tile-sliced one (tsplit: split_slices slices per function), each as
// two launches per iteration or one persistent launch per portion
struct LaunchPlan {
  bool tsplit = false;
  int split_slices = 0;
  bool persist = false;
  int ts_initial = 0;  // slices a run starts with (reslice_tsplit may cut finer as chains finish)
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Which workgroup shape serves this problem (mhx_types.hpp), as waves per group.  16 chains per
// workgroup and 2048-point tiles pay off when the datasets are long (>= 4 such tiles) and there
// are enough chains to give every CU its one workgroup; otherwise 8 chains per workgroup (more,
// smaller workgroups; less barrier and pad overhead on short datasets).  MHX_FAMILY_WPG pins it.
inline int choose_family(const ProblemShape& s, const EngineKnobs& k) {
  if (k.family_wpg) return k.family_wpg;
  return s.longest >= 4 * (int64_t)tile_points_of(16) && s.chains >= 16 * 256 ? 16 : 8;
}

// May this engine use the persistent kernels at all (MHX_NO_PERSIST=1: never; persist_off: a
// launch of theirs once lost its sweep workgroups; their handshake blocks carry 60 parameters)
inline bool persist_allowed(const ProblemShape& s, const EngineKnobs& k) {
  return !s.persist_off && !k.no_persist && s.d <= 60;
}

// Workgroups of a persistent launch (k_persist, k_persist_ts: they wait for one another) the GPU
// holds at once: CUs times what the occupancy calculator gives the COMPILED kernel (registers,
// LDS and waves - an assumed "two per CU" was wrong for a kernel of 132 VGPRs and cost half the
// speed, see k_persist_ts).  Every slot: what the calculator promises is what the dispatcher
// gives - 128 groups x (1 + 3) = 512 workgroups on 256 CUs ran in one shift, 55.9 us per
// iteration against 72.0 of two launches - and a workgroup that finds its slot taken for a
// while by another kernel of the process arrives late, within the masters' patience
// (MHX_PERSIST_FILL=<per cent>: measurements).
inline int64_t persist_capacity(const ProblemShape& s, const EngineKnobs& k, bool ts) {
  return (int64_t)s.cus * (ts ? s.per_cu_ts : s.per_cu) * k.persist_fill / 100;
}

// nwin windows cut into ts slices are ceil(nwin / ts) windows per slice - which may fill fewer
// slices than ts: 49 windows in 16 slices are 13 slices of 4 (the last one of 1) and three empty
// ones, whose workgroups would be launched (or, persistent, sit on a CU and poll) for nothing.
// The sums are the same bits either way: an empty slice's partial sum is +0.
inline int64_t trim_slices(int64_t nwin, int64_t ts) {
  if (ts <= 0 || nwin <= 0) return ts;
  return ceil_div(nwin, ceil_div(nwin, ts));
}

// Split mode (mhx_kernels.hpp): how many workgroups share one chain's likelihood sums, or 0 for
// the batch kernels.  Worth it when the batch launch would leave most CUs without a workgroup
// and every (slice, wave) slot still gets at least 512 points of the longest dataset.
// MHX_SPLIT=0 switches it off, MHX_SPLIT=<n> forces n slices.
// cap_pc > 0: the per-chain persistent form (k_persist: one launch per portion of iterations) is
// allowed and the GPU holds that many of its workgroups at once - where C (1 + slices) of them
// fit, split mode costs 7.6 us per iteration instead of the two launches' 14 and pays off on
// shorter datasets (4096 points: 13.4 us in the batch kernel).
inline int choose_split(const ProblemShape& s, const EngineKnobs& k, int64_t cap_pc) {
  if (!s.capable || s.pooled || s.planes) return 0;
  const int64_t C = s.chains;
  const int W = s.waves_per_group;
  const int64_t by_data = s.longest / (512 * (int64_t)W);
  if (k.split_set) return k.split <= 0 ? 0 : (int)std::min<int64_t>(std::max<int64_t>(by_data, 1), k.split);
  // measured (tools/debug/split_sweep.sh, round 2; chain-steps/s batch | best split):
  //   config 2's problem   64 chains 6.6e5 | 2.4e6 (x4)    256: 2.6e6 | 4.5e6 (x4)
  //                        512: 5.3e6 | 5.4e6 (x2)         1024: 1.05e7 | 5.9e6    2048: 2.1e7 | 6.3e6
  //   config 3's problem   16: 4.2e3 | 1.5e5 (x24)    256: 6.7e4 | 2.9e5 (x8)    1024: 2.7e5 | 3.1e5
  // (round 2, with the recurrence in the split sweep as well:  config 3  16: 2.3e5 (x24)
  //  256: 4.6e5 (x4)    1024: 2.7e5 | 5.4e5 (x4);  config 2 unchanged: its split sweep is bound by
  //  the L2, every chain reading the dataset for itself)
  // The batch kernels (peak skipping, LDS tiles shared by 8 chains) win from about 128
  // workgroups on when a point is cheap; a point that costs 40 instructions and more (a log per
  // point, a pseudo-Voigt, an expression compiled as written) keeps the whole GPU busy in split
  // mode until the batch kernels have a workgroup for every CU.  Below that about 1024
  // workgroups in the sweep launch are best.
  if (ceil_div(C, W) >= (s.heavy ? 256 : 128)) return 0;
  // two launches cost about 14 us per iteration: the fused batch kernel is quicker than that up
  // to roughly a dozen 1024-point tiles; one persistent launch is quicker from one slice's worth
  // of points on (the batch kernel: 13.4 us on 4096 points)
  if (by_data < 4) {
    if (by_data >= 1 && !s.heavy && C * (1 + by_data) <= cap_pc) return (int)by_data;
    return 0;
  }
  // (cheap points: beyond 8 slices the partial sums and the extra blocks cost more than they
  // bring once there are 32 chains and more - 64 chains: x16 2.2e6, x8 2.4e6, x4 2.4e6)
  const int64_t want = s.heavy ? std::max<int64_t>(4, 2048 / C)
                               : std::max<int64_t>(2, std::min<int64_t>(1024 / C, C < 32 ? 24 : 8));
  const int64_t slices = std::min<int64_t>(std::min<int64_t>(want, 24), by_data);
  return slices >= 2 ? (int)slices : 0;
}

// Tile-sliced split mode (k_split_tsweep): into how many slices of whole windows every function is
// cut, each walked by the workgroups of ALL chain groups, or 0.  For batches too small to give
// every CU a workgroup of the batch kernels and big enough to fill workgroups of their own:
// about two workgroups per CU in the sweep launch.  MHX_TSPLIT=0 switches it off (the per-chain
// split mode or the batch kernels then), MHX_TSPLIT=<n> asks for n slices; MHX_SPLIT=0 means the
// batch kernels here too, MHX_SPLIT=<n> alone the per-chain split mode.
// cap_pc, cap_ts > 0: the persistent forms are allowed (workgroups of k_persist / k_persist_ts the
// GPU holds at once).  One persistent launch costs about 10.3 us per iteration where the two
// launches cost 20 (measured round 4, two-peak problem, us per iteration, persistent | default
// of round 3):  8192 points  32 chains 12.4 | 18.2 (batch kernel)    256: 12.4 | 18.5
//   20000 points  128: 11.1 | 22.1 (per-chain split)    256: 13.2 | 28.9
//   50000 points  8: 10.4 | 20.4 (two launches)    128: 11.9 | 23.5
// so it serves from 4 windows on - unless the per-chain persistent form fits, which is quicker
// still on short datasets (20000 points, 8 ... 64 chains: 7.7 ... 8.7 us).
inline int choose_tsplit(const ProblemShape& s, const EngineKnobs& k, int64_t cap_pc, int64_t cap_ts) {
  if (!s.capable || s.pooled || s.planes) return 0;
  const int64_t nwin = s.nwin;
  const int64_t C = s.chains;
  const int W = s.waves_per_group;
  const int64_t groups = ceil_div(C, W);
  int64_t want = 0;
  // (MHX_SPLIT set: the caller has decided - the batch kernels, or the per-chain split mode)
  if (k.split_set && (!k.tsplit_set || k.split <= 0)) return 0;
  if (k.tsplit_set) {
    want = k.tsplit;
    if (want <= 0) return 0;
  } else {
    // two launches and the step kernel cost about 17 us per iteration (64 chains of config 2's
    // problem: 20.7 us with one window per workgroup): the fused batch kernel, 0.6-0.8 us per
    // 1024-point tile when points are cheap, is quicker than that up to about two dozen tiles
    if (groups >= 256) return 0;
    // fewer walkers than a workgroup has waves: the per-chain split mode - unless the persistent
    // form is allowed, whose sweep workgroups walk LDS tiles with peak skipping and the
    // recurrence, one window per wave however long the dataset (a single walker on 1e5 points
    // 7.6 -> 6.4 us per step, on 1e6 points 25.4 -> 11.1; 20000 points: 6.2 against 6.7, left alone)
    if (C < W && (cap_ts <= 0 || nwin < 12)) return 0;
    if (nwin < (s.heavy ? 4 : 12)) {
      // too short for two launches per iteration: as one persistent launch, or not at all
      // (a window per slice, or fewer slices of up to 4 windows where the GPU does not hold that
      // many workgroups at once: 20000 points, 512 walkers x7 instead of the per-chain split
      // mode's two launches)
      const int64_t fit = std::min<int64_t>(nwin, cap_ts / groups - 1);
      if (nwin < (s.heavy ? 2 : 4) || fit < 2 || ceil_div(nwin, fit) > 4) return 0;
      const int pc = choose_split(s, k, cap_pc);
      if (pc > 0 && C * (1 + pc) <= cap_pc) return 0;  // (the per-chain persistent form)
      return (int)trim_slices(nwin, fit);
    }
    // measured (config 2's problem, chain-steps/s; slices 4 | 8 | 16 | 32 | 49):
    //   64 chains 1.5e6 | 2.1e6 | 2.6e6 | 3.1e6 | 3.1e6     256: 6.0e6 | 7.9e6 | 8.0e6 | 7.0e6 | 6.3e6
    //   1024: 1.47e7 | 1.33e7 | 1.13e7 | 9.2e6 | 8.8e6       (per-chain split mode: 2.4e6, 4.7e6; batch
    //   kernels at 1024: 1.31e7) - about 512 workgroups in the sweep launch
    want = 512 / groups;
  }
  want = std::min<int64_t>(want, nwin);
  if (!k.tsplit_set) {
    want = trim_slices(nwin, want);
    // two or three slices as TWO LAUNCHES per iteration lose to the batch kernels on datasets
    // that are not long (measured round 4, us per iteration, two launches | batch kernels:
    //   1536 walkers x2: 5e4 points 76.5 | 56.7, 1e5: 102 | 90.8, 1e6: 690 | 846;
    //   1100 walkers x3: 5e4 points 58.6 | 55.2, 1e5: 75.9 | 89.9) - unless the persistent
    // form will take them (1024 walkers x3, 5e4 points: 35.5 | 49.1)
    const int64_t pfit = cap_ts > 0 ? std::min<int64_t>(want, cap_ts / groups - 1) : 0;
    const bool persistable = pfit >= std::max<int64_t>(2, (3 * want + 3) / 4) && k.persist_ts != 0;
    if (!persistable && ((want == 2 && nwin < 128) || (want == 3 && nwin < 32))) return 0;
  }
  return want >= 2 ? (int)want : 0;
}

// Whether the kernels compiled at run time need the split-mode forms (rtc_get's want_split), for
// a problem whose kernels would have them (`capable`): before the kernels exist their occupancy
// is not known, so the persistent forms are assumed to fit as well as they could.
inline bool want_split(ProblemShape s, const EngineKnobs& k, bool capable) {
  s.capable = capable;
  const int64_t cap_guess = persist_allowed(s, k) ? 2 * 256 : 0;
  return choose_split(s, k, cap_guess) > 0 || choose_tsplit(s, k, cap_guess, cap_guess) > 0;
}

// The launch form of a finalised problem, the persistent forms' reduced slicing included.
inline LaunchPlan plan_modes(const ProblemShape& s, const EngineKnobs& k) {
  LaunchPlan p;
  const bool pa = s.capable && persist_allowed(s, k);
  const int64_t cap_pc = pa ? persist_capacity(s, k, false) : 0;
  const int64_t cap_ts = pa && k.persist_ts != 0 ? persist_capacity(s, k, true) : 0;
  const int ts = choose_tsplit(s, k, cap_pc, cap_ts);
  p.tsplit = ts > 0;
  p.split_slices = p.tsplit ? ts : choose_split(s, k, cap_pc);
  p.ts_initial = p.tsplit ? ts : 0;
  if (p.split_slices == 0) return p;
  // the split modes as ONE launch per portion of iterations (k_persist, k_persist_ts): the chain's
  // master wave and its sweep workgroups hand each other the proposal and the partial sums
  // through memory, which needs every workgroup of the launch on the GPU at once
  // (MHX_NO_PERSIST=1: the two launches per iteration of rounds 1-3).
  // tile-sliced: (1 + slices) workgroups per chain GROUP - with fewer slices, down to 2,
  // where the default slicing would not fit the GPU at once (a run's re-slicing keeps to the
  // same bound: reslice_tsplit)
  const int64_t units = p.tsplit ? ceil_div(s.chains, s.waves_per_group) : s.chains;
  const int64_t cap = persist_capacity(s, k, p.tsplit);
  int64_t slices = p.split_slices;
  // The tile-sliced form runs with fewer slices where the default slicing does not fit the
  // GPU at once - down to three quarters of it (MHX_PERSIST_TS=1: down to 2; =0: never the
  // persistent form).  Measured round 4 (two-peak problem, 1e5 points, us per iteration,
  // persistent | two launches):  8 chains x49 10.1 | 20.0    64: x49 12.2 | 23.0
  //   128: x27 14.3 | x32 26.5    256: x13 19.6 | x16 33.6    512: x6 31.2 | x8 46.6
  //   1024: x2 68.9 | x4 71.7;   1e6 points  8: 15.4 | 23.8    64: 34.5 | 45.8
  //   256: 120 | 121    1024: x2 611 | x4 429 (half the slices: not taken).
  // (Round 3 had measured the persistent form no faster and left it behind a switch: its
  // kernel took 132 VGPRs, one workgroup fitted a CU, and the launch ran in two shifts.)
  if (p.tsplit && !k.tsplit_set) {
    const int64_t fit = trim_slices(s.nwin, std::min<int64_t>(slices, cap / units - 1));
    const int64_t least = k.persist_ts > 0 ? 2 : std::max<int64_t>(2, (3 * slices + 3) / 4);
    // (fewer slices only where an iteration is short enough for the saved launches to
    // matter: up to 48 windows per slice - 1e6 points, 1024 walkers: x3, 163 windows each,
    // 500 us against the two launches' x4 424; 512: x7, 70 each, 226 against x8 223;
    // 256: x15, 33 each, 106 against x16 121; 1e5 points, 1024 walkers: x3 55.9 against x4 72.0)
    const bool short_rounds = fit > 0 && ceil_div(s.nwin, fit) <= 48;
    slices = fit >= least && (fit == slices || short_rounds || k.persist_ts > 0) ? fit : 0;
  }
  const bool want = p.tsplit ? k.persist_ts != 0 : true;
  p.persist = want && persist_allowed(s, k) && slices >= (p.tsplit ? 2 : 1) && units * (1 + slices) <= cap;
  if (p.persist && p.tsplit) p.split_slices = p.ts_initial = (int)slices;
  return p;
}

// A dataset per walker (mhx_set_dataset_planes): resident in LDS or streamed from memory.
// The resident form keeps, in the space the tile buffers occupy (GroupLds::tiles: 2 * kMaxArrays
// tiles - 8192 doubles in the 8-wave family, 16384 in the 16-wave family), of every function its
// shared x, its shared 1/sigma where there is one (MHX_SIGMA_SHARED), and for each wave of the
// workgroup the walker's y/sigma and - MHX_SIGMA_PER_POINT only - its 1/sigma, each padded to
// kPlanePad points.  It needs the tile buffers for itself: a problem that also has a function on
// a shared dataset (whose sweep stages tiles there) is streamed.  MHX_PLANES_NO_LDS=1: streamed.
inline int64_t planes_pad(int64_t n) { return std::max<int64_t>(ceil_div(n, kPlanePad), 1) * kPlanePad; }
inline int64_t planes_lds_capacity(int waves_per_group) {
  return 2 * (int64_t)kMaxArrays * tile_points_of(waves_per_group);
}
// doubles of function k: shared ones and those of each wave
inline int64_t planes_shared_doubles(int64_t n, int sigma_kind) {
  return planes_pad(n) * (sigma_kind == MHX_SIGMA_SHARED ? 2 : 1);
}
inline int64_t planes_wave_doubles(int64_t n, int sigma_kind) {
  return planes_pad(n) * (sigma_kind == MHX_SIGMA_PER_POINT ? 2 : 1);
}
// n[k], sigma_kind[k]: the K_planes functions with a dataset per walker; K: all functions
inline bool planes_resident(const int64_t* n, const int* sigma_kind, int K_planes, int K,
                            int waves_per_group, const EngineKnobs& k) {
  if (k.planes_no_lds || K_planes < 1 || K_planes != K) return false;
  int64_t need = 0;
  for (int i = 0; i < K_planes; ++i)
    need += planes_shared_doubles(n[i], sigma_kind[i]) +
            (int64_t)waves_per_group * planes_wave_doubles(n[i], sigma_kind[i]);
  return need <= planes_lds_capacity(waves_per_group);
}

// Highest-density intervals (k_hdi): a column's window is sorted as keys in a power of two of
// slots, hdi_pad(take) of them.  The LDS path lays a chain's nc columns down hdi_pad + 1 slots apart
// (neighbouring columns then start two banks apart for the transposing store) and needs them all in
// one workgroup's LDS; otherwise, or with MHX_HDI_NO_LDS=1, the memory path: the keys in a piece of
// the stage buffer, one workgroup per (chain, column), which sorts a window of up to kHdiChunk keys
// in 8 bytes of LDS a key.  kHdiLdsBudget is a CU's 160 KiB over eight: with more, fewer than eight
// workgroups of four waves fit a CU, wave slots stay empty, and the LDS path was measured the slower
// one (64 KiB a workgroup, 1.6 times; level at 16 KiB; 2.1 times the quicker at 8 KiB).
constexpr size_t kHdiLdsBudget = (size_t)20 * 1024;
inline int64_t hdi_pad(int64_t take) {
  int64_t p = 2;
  while (p < take) p <<= 1;
  return p;
}
inline size_t hdi_lds_bytes(int take, int nc) { return (size_t)nc * (size_t)(hdi_pad(take) + 1) * sizeof(uint64_t); }
inline bool hdi_use_lds(int take, int nc, const EngineKnobs& k) {
  return !k.hdi_no_lds && hdi_lds_bytes(take, nc) <= kHdiLdsBudget;
}

// A repack of the chains still walking is due when a quarter of those dealt at the last deal
// (all of them before the first) has finished since.
inline bool repack_due(int64_t running, int64_t mapped) { return running > 0 && running * 4 <= mapped * 3; }

// Tile-sliced split mode, chains packed into `groups` groups: the slices the functions are cut
// into again, so that the sweep launch keeps about 512 workgroups (MHX_TSPLIT set: as they are).
inline int64_t reslice_tsplit(const ProblemShape& s, const EngineKnobs& k, int64_t slices, bool persist,
                              int64_t groups) {
  if (k.tsplit_set) return slices;
  int64_t ts = std::max<int64_t>(slices, std::min<int64_t>(std::min<int64_t>(512 / groups, s.nwin), 512));
  if (persist)  // (every workgroup of a persistent launch on the GPU at once)
    ts = std::max<int64_t>(2, std::min<int64_t>(ts, persist_capacity(s, k, true) / groups - 1));
  return std::max<int64_t>(2, trim_slices(s.nwin, ts));
}

// Workgroups of W waves the batch kernels' GPU holds at once: two per CU in the 8-wave family.
inline int64_t resident_groups(int cus, int64_t W) { return (int64_t)cus * (W <= 8 ? 2 : 1); }

// Batch kernels: the workgroups `running` chains are dealt over when a launch had `in_use` slots -
// max(what they need, min(what the launch had, what the GPU holds)); MHX_COMPACT_ALWAYS=1 lets
// the launch shrink below what the GPU holds.
inline int64_t deal_target(int cus, int64_t W, int64_t in_use, int64_t running, bool always) {
  const int64_t floor_groups = always ? 1 : resident_groups(cus, W);
  return std::max<int64_t>(ceil_div(running, W), std::min<int64_t>(ceil_div(in_use, W), floor_groups));
}

// ... and at the start of a run of C chains: up to one workgroup per CU, workgroups of 4; between
// one and two per CU (8-wave family), two on EVERY CU instead of two on some and one on the
// others.  0: the chains stay where they are.
inline int64_t deal_initial_target(int cus, int64_t W, int64_t C) {
  const int64_t groups = ceil_div(C, W);
  const int64_t resident = resident_groups(cus, W);
  const int64_t target = groups <= cus ? std::min<int64_t>(cus, std::max<int64_t>(groups, (C + 3) / 4))
                                       : (groups < resident ? resident : groups);
  return target <= groups || C <= W ? 0 : target;
}

}  // namespace mhx
