// mhx_ensemble.hpp -- the host half of mhx_get_ensemble_percentiles as pure functions of plain
// numbers (no HIP, no engine): which bin of a pass's counters holds a rank, which distinct tasks
// the next pass needs, what a found key is worth as a double, and how the call's scratch is
// carved.  mhx_engine.cpp launches what these describe (k_ensemble_digits); tests/
// test_ensemble_host.py drives them on the CPU.
//
// The selection: the order keys of the pool are 64-bit integers; pass p = 0 .. 7 looks at the
// 8-bit digit at shift 56 - 8 p.  A TARGET is one (percentile, column) of the call: it carries
// the digits found so far (`prefix`), its rank among the keys that share them and how many those
// are.  A pass counts, per distinct (column, prefix), the sharing keys by their next digit; the
// target's rank falls in exactly one bin, whose digit joins the prefix.  After eight passes the
// prefix is the key itself and `run` the number of pool elements equal to it.
#pragma once
#include <cstdint>
#include <cstring>

#include "mhx_stage.hpp"
#include "mhx_types.hpp"

namespace mhx {

constexpr int kEnsPasses = 8;
constexpr int kEnsMaxTasks = MHX_MAX_PARAMS * MHX_MAX_PERCENTILES;
static_assert(kEnsPasses * 8 == 64 && kEnsBins == 256, "eight 8-bit digits make a key");

// The smallest digit whose cumulative count exceeds `rank`, the rank within that bin and the
// bin's count; false unless n_bins >= 1 and 0 <= rank < the sum of the counts.
inline bool ensemble_pick(const uint64_t* counts, int n_bins, int64_t rank, int32_t* digit,
                          int64_t* rank_in_bin, int64_t* bin_count) {
  if (!counts || n_bins < 1 || rank < 0) return false;
  uint64_t left = (uint64_t)rank;  // the rank among the bins not yet passed
  for (int b = 0; b < n_bins; ++b) {
    if (left < counts[b]) {
      if (digit) *digit = b;
      if (rank_in_bin) *rank_in_bin = (int64_t)left;
      if (bin_count) *bin_count = (int64_t)counts[b];
      return true;
    }
    left -= counts[b];
  }
  return false;
}

struct EnsTarget {
  int32_t col = 0;      // its column of the call
  int32_t task = -1;    // its task in the pass at hand (-1: none)
  int32_t between = 0;  // the percentile is the mean of elements pos and pos + 1
  uint64_t prefix = 0;  // the digits found so far, in place
  int64_t rank = 0;     // its rank among the keys that share the prefix
  int64_t run = 0;      // how many keys share the prefix
  uint64_t next = 0;    // the key of element pos + 1 (between only; after the successor pass)
};

inline int ensemble_shift(int pass) { return 56 - 8 * pass; }
// the bits of a key above the digit at `shift`
inline uint64_t ensemble_mask(int shift) { return shift >= 56 ? 0 : ~(uint64_t)0 << (shift + 8); }

// pass 0 knows no rank yet (the pool's size is what it counts): one task per column
inline int ensemble_first_tasks(int n_cols, EnsTask* tasks) {
  for (int c = 0; c < n_cols; ++c) tasks[c] = EnsTask{0, c, ensemble_shift(0)};
  return n_cols;
}
// the targets [n_pct][n_cols] of a pool of n_pooled >= 1 elements, ahead of pass 0's pick
inline void ensemble_targets(int64_t n_pooled, const PctList& pc, int n_cols, EnsTarget* t) {
  for (int q = 0; q < pc.n; ++q) {
    int64_t pos;
    int32_t between;
    percentile_rank_of(n_pooled, pc.num[q], pc.den[q], &pos, &between);
    for (int c = 0; c < n_cols; ++c) {
      EnsTarget& g = t[q * n_cols + c];
      g = EnsTarget{};
      g.col = c, g.task = c, g.between = between, g.rank = pos, g.run = n_pooled;
    }
  }
}
// The distinct (column, prefix) of the targets as the tasks of the pass at `shift`, in the order
// the targets first name them; every target learns its task.  Returns their number (at most n).
inline int ensemble_tasks(EnsTarget* t, int n, int shift, EnsTask* tasks) {
  int nt = 0;
  for (int i = 0; i < n; ++i) {
    int k = 0;
    while (k < nt && !(tasks[k].col == t[i].col && tasks[k].prefix == t[i].prefix)) ++k;
    if (k == nt) tasks[nt++] = EnsTask{t[i].prefix, t[i].col, shift};
    t[i].task = k;
  }
  return nt;
}
// every target picks its bin of counts [n_tasks][kEnsBins]; false when a rank lies outside its
// task's counts (the counters do not belong to these targets)
inline bool ensemble_advance(EnsTarget* t, int n, int shift, const uint64_t* counts) {
  for (int i = 0; i < n; ++i) {
    int32_t digit = 0;
    if (t[i].task < 0 ||
        !ensemble_pick(counts + (size_t)t[i].task * kEnsBins, kEnsBins, t[i].rank, &digit, &t[i].rank, &t[i].run))
      return false;
    t[i].prefix |= (uint64_t)digit << shift;
  }
  return true;
}
// After the last pass: element pos + 1 of a `between` target is the same key unless pos is the
// last of its run of equal keys; those targets get a successor task - the distinct (column, key)
// among them - and the others task -1 and next = their own key.  Returns the number of tasks.
inline int ensemble_successor_tasks(EnsTarget* t, int n, EnsTask* tasks) {
  int nt = 0;
  for (int i = 0; i < n; ++i) {
    t[i].task = -1, t[i].next = t[i].prefix;
    if (!t[i].between || t[i].rank + 1 < t[i].run) continue;
    int k = 0;
    while (k < nt && !(tasks[k].col == t[i].col && tasks[k].prefix == t[i].prefix)) ++k;
    if (k == nt) tasks[nt++] = EnsTask{t[i].prefix, t[i].col, 0};
    t[i].task = k;
  }
  return nt;
}
inline void ensemble_take_successors(EnsTarget* t, int n, const uint64_t* least) {
  for (int i = 0; i < n; ++i)
    if (t[i].task >= 0) t[i].next = least[t[i].task];
}

// the double of an order key (order_key of mhx_readout_kernels.hpp, inverted; the NaN key gives a NaN)
inline double ensemble_key_value(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k ^ ((uint64_t)1 << 63)) : ~k;
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}
inline uint64_t ensemble_order_key(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  if (v != v) return ~(uint64_t)0;
  return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}
inline double ensemble_value(const EnsTarget& g) {
  const double lo = ensemble_key_value(g.prefix);
  return g.between ? (lo + ensemble_key_value(g.next)) / 2.0 : lo;
}

// The scratch of a call on one engine: the counters of at most max_tasks tasks, the task list,
// the include mask, n_used [n_chains] and the columns' NaN flags.  Nothing depends on `take`;
// the counters are at most kEnsMaxTasks x 2 KiB.
struct EnsemblePieces {
  size_t counters, tasks, include, n_used, status;
};
inline int ensemble_max_tasks(int n_cols, int n_pct) { return n_cols * (n_pct > 1 ? n_pct : 1); }
inline EnsemblePieces carve_ensemble(Carver& c, int max_tasks, int n_cols, int64_t n_chains) {
  EnsemblePieces s;
  s.counters = c.take((size_t)max_tasks * kEnsBins * sizeof(uint64_t));
  s.tasks = c.take((size_t)max_tasks * sizeof(EnsTask));
  s.include = c.take((size_t)n_chains);
  s.n_used = c.take((size_t)n_chains * sizeof(int32_t));
  s.status = c.take((size_t)n_cols * sizeof(int32_t));
  return s;
}

}  // namespace mhx
