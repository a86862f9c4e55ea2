// mhx_readout_kernels.hpp -- the model-free read-out kernels of the history ring: walker-set-get
// (k_percentiles .. k_band_select) and the second halves of the model read-outs (k_waic_totals ..
// k_loo_totals).  No model Spec is involved, so they are compiled ONCE: mhx_kernels.hip includes
// this file in the primary family's unit only, after mhx_kernels.hpp and ahead of mhx_launch.inc,
// whose primary half holds their launchers.  Never embedded, never handed to hiprtc.
#pragma once
#include "mhx_kernels.hpp"

namespace mhx {
inline namespace MHX_FAMILY {

// ------------------------------------------------------------------------------------------
// walker-set-get (M:1029-1030): the summarising selectors of walker-get for EVERY chain in one
// launch, on the device ring.  No model Spec is involved: compiled once (the primary family's
// unit), never through hiprtc.  Each launch covers the `n` chains from `c0` on (the host works
// through the chains in portions so that the scratch stays bounded); outputs and scratch are
// indexed by the chain's place in the portion.
// ------------------------------------------------------------------------------------------

// order-preserving 64-bit key of a double: all bits of a negative flipped, the sign bit of the
// others set.  -0 < +0 as keys (they compare equal as numbers: either may stand for the other);
// every NaN gets the greatest key, so it sorts last whatever its sign.
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long b = bits_of(v);
  if (v != v) return ~0ULL;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

// nth-percentile (M:1495-1506) of the n keys key_at(0 .. n-1) by one wavefront: the key of rank
// `pos` of the ascending order by most-significant-bit-first radix selection (one bit a pass:
// count the still-candidate keys whose bit is 0; the rank falls among them or among the others),
// 64 passes whatever n is, nothing sorted, nothing stored.  `between`: the mean with the next
// element - the same key when the rank is not the last of its run of equal keys, else the
// smallest key above it (one masked min-reduction).  All lanes return the same value.
template <class KeyAt>
__device__ __forceinline__ double select_percentile(KeyAt key_at, int n, int pos, bool between) {
  const int l = lane_id();
  unsigned long long prefix = 0, mask = 0;
  int k = pos, cand = n;
  for (int b = 63; b >= 0; --b) {
    const unsigned long long bit = 1ULL << b;
    int cnt = 0;
    for (int s = l; s < n; s += kWave) {
      const unsigned long long key = key_at(s);
      cnt += ((key & mask) == prefix && (key & bit) == 0) ? 1 : 0;
    }
    const int c0 = __builtin_amdgcn_readfirstlane(wave_sum_i(cnt));
    if (k < c0) {
      cand = c0;
    } else {
      k -= c0;
      cand -= c0;
      prefix |= bit;
    }
    mask |= bit;
  }
  const double lo = key_value(prefix);
  if (!between) return lo;
  unsigned long long up = prefix;
  if (k + 1 >= cand) {
    unsigned long long m = ~0ULL;
    for (int s = l; s < n; s += kWave) {
      const unsigned long long key = key_at(s);
      if (key > prefix && key < m) m = key;
    }
    up = wave_min_u64(m);
  }
  return (lo + key_value(up)) / 2.0;
}

// mhx_get_percentiles.  One workgroup of kPctWaves wavefronts per chain; wave w serves the
// parameters w, w + kPctWaves, ...; every percentile reruns the selection (64 cheap passes over
// a column that is already in LDS, against one pass to bring it there).
//   use_lds = 1: the window's rows - t x d contiguous doubles, two runs when the ring has
//     wrapped - are read ONCE, coalesced, by the whole workgroup and laid down as keys, one
//     column of `tpad` slots per parameter (tpad staggers the columns over the banks for the
//     transposing store; the selection reads a column with unit stride, conflict-free)
//   use_lds = 0: a window that does not fit (d * tpad * 8 bytes of LDS): every pass reads the
//     column from global memory / L2 with stride d
constexpr int kPctWaves = 4;
constexpr int kPctThreads = kWave * kPctWaves;
__global__ __launch_bounds__(kPctThreads) void k_percentiles(ChainState S, int64_t c0, int take,
                                                            PctList pc, int use_lds, int tpad,
                                                            double* __restrict__ out,
                                                            int32_t* __restrict__ n_used) {
  unsigned long long* col = reinterpret_cast<unsigned long long*>(mhx_lds_raw);
  const int w = wave_in_group(), l = lane_id(), d = S.d;
  const int64_t i = blockIdx.x;
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  if (threadIdx.x == 0) n_used[i] = t;
  if (use_lds) {
    const int64_t oldest = ring.nh - t;
    for (int f = threadIdx.x; f < t * d; f += kPctThreads) {
      const int s = f / d, p = f - s * d;
      const int64_t slot = (oldest + s) & (int64_t)ring.mask;
      col[(size_t)p * tpad + s] = order_key(ring.theta[slot * d + p]);
    }
    __syncthreads();
  }
  for (int p = w; p < d; p += kPctWaves)
    for (int q = 0; q < pc.n; ++q) {
      double v = 0.0;
      if (t > 0) {
        int64_t pos;
        int32_t between;
        percentile_rank_of(t, pc.num[q], pc.den[q], &pos, &between);
        if (use_lds) {
          const unsigned long long* cp = col + (size_t)p * tpad;
          v = select_percentile([&](int s) { return cp[s]; }, t, (int)pos, between != 0);
        } else {
          v = select_percentile(
              [&](int s) { return order_key(ring.theta[(int64_t)ring.slot(s) * d + p]); }, t,
              (int)pos, between != 0);
        }
      }
      if (l == 0) out[(i * pc.n + q) * d + p] = v;
    }
}

// The place of v among the ascending edges b[0 .. nb] (make-histo M:1548-1557 as a bin rule: v
// falls in bin n = the smallest n in 1..nb with v <= b[n]): 0 below b[0], n, nb + 1 above b[nb],
// -1 a NaN.  A lower-bound search over b[1 .. nb]: at most 11 probes at nb = 1024.
__device__ __forceinline__ int histo_slot(const double* b, int nb, double v) {
  if (v != v) return -1;
  if (v < b[0]) return 0;
  int lo = 1, n = nb;
  while (n > 0) {
    const int half = n >> 1;
    if (b[lo + half] < v) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

// mhx_get_histograms.  One workgroup of kPctThreads per chain.  The window's rows - t x d
// contiguous doubles, two runs when the ring has wrapped - are read ONCE, coalesced, as
// k_percentiles reads them; an element of a column that is asked for finds its place among that
// column's edges and adds 1 to an int32 count.  Integer additions only: any order of the threads
// gives the same counts.
//   use_lds = 1: the chain's edge rows [nc][nb + 1] are copied to LDS, the counts live there
//     ([nc][cpitch]: below, the nb bins, above; cpitch is odd, which spreads equal bins of
//     neighbouring columns over the banks) and are written out once at the end
//   use_lds = 0: edges and counts do not fit: the edges are read from the stage buffer and the
//     counts go straight into the portion's pieces (zeroed by the host) with global atomics
// edges + i * edge_stride: chain i's rows (edge_stride 0: one set for all).  counts [n][nc][nb],
// outside [n][nc][2] = (below, above), n_used [n], status [n][nc] (1: the column held a NaN).
__global__ __launch_bounds__(kPctThreads) void k_histograms(
    ChainState S, int64_t c0, int take, ColList cl, int nb, const double* __restrict__ edges,
    int64_t edge_stride, int use_lds, int cpitch, int32_t* __restrict__ counts,
    int32_t* __restrict__ outside, int32_t* __restrict__ n_used, int32_t* __restrict__ status) {
  const int d = S.d, nc = cl.n, ne = nb + 1, tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  if (tid == 0) n_used[i] = t;
  const double* ge = edges + i * edge_stride;
  double* le = reinterpret_cast<double*>(mhx_lds_raw);
  int32_t* cnt = reinterpret_cast<int32_t*>(le + nc * ne);
  int32_t* nan = cnt + nc * cpitch;
  if (use_lds) {
    for (int f = tid; f < nc * ne; f += kPctThreads) le[f] = ge[f];
    for (int f = tid; f < nc * cpitch + nc; f += kPctThreads) cnt[f] = 0;
    __syncthreads();
  }
  // element f = s d + p of the window, oldest row first; (s, p) follow f without a division
  const int64_t oldest = ring.nh - t;
  const int ds = kPctThreads / d, dp = kPctThreads - ds * d;
  int s = tid / d, p = tid - s * d;
  for (int f = tid; f < t * d; f += kPctThreads) {
    const int c = cl.of_param[p];
    if (c >= 0) {
      const int64_t slot = (oldest + s) & (int64_t)ring.mask;
      const double v = ring.theta[slot * d + p];
      if (use_lds) {
        const int k = histo_slot(le + c * ne, nb, v);
        if (k < 0)
          nan[c] = 1;
        else
          atomicAdd(&cnt[c * cpitch + k], 1);
      } else {
        const int k = histo_slot(ge + c * ne, nb, v);
        const int64_t col = i * nc + c;
        if (k < 0)
          status[col] = 1;
        else if (k == 0 || k > nb)
          atomicAdd(&outside[col * 2 + (k > nb ? 1 : 0)], 1);
        else
          atomicAdd(&counts[col * nb + (k - 1)], 1);
      }
    }
    s += ds;
    p += dp;
    if (p >= d) {
      p -= d;
      ++s;
    }
  }
  if (!use_lds) return;
  __syncthreads();
  for (int f = tid; f < nc * nb; f += kPctThreads) {
    const int c = f / nb, k = f - c * nb;
    counts[i * nc * nb + f] = cnt[c * cpitch + 1 + k];
  }
  for (int c = tid; c < nc; c += kPctThreads) {
    outside[(i * nc + c) * 2] = cnt[c * cpitch];
    outside[(i * nc + c) * 2 + 1] = cnt[c * cpitch + nb + 1];
    status[i * nc + c] = nan[c];
  }
}

// mhx_get_pair_grids.  One workgroup of kPctThreads per chain; pairs [2][np]: pair q counts the
// steps by (bin of column pair_a[q], bin of column pair_b[q]) in counts [n][np][nb][nb];
// n_inside [n][np] the steps with both values in a bin, status [n][np] (1: either column held a
// NaN), n_used [n].  Integer additions only, as k_histograms.
//   use_lds = 1: the window is read ONCE, coalesced, and the place of every (column, step) laid
//     down in LDS as a 16-bit value (0xffff a NaN), one row of `ipitch` values per column - an
//     odd count of 32-bit words, so that the columns of one step fall on different banks for the
//     transposing store.  Every pair is then counted from two unit-stride rows into its cells
//     in LDS; cells, n_inside and status are written out once at the end
//   use_lds = 0: edges + cells + places do not fit: a step's two values are read and placed per
//     pair, and the counts go straight into the portion's pieces (zeroed by the host)
__global__ __launch_bounds__(kPctThreads) void k_pair_grids(
    ChainState S, int64_t c0, int take, ColList cl, int nb, int np,
    const double* __restrict__ edges, int64_t edge_stride, const int32_t* __restrict__ pairs,
    int use_lds, int ipitch, int32_t* __restrict__ counts, int32_t* __restrict__ n_inside,
    int32_t* __restrict__ n_used, int32_t* __restrict__ status) {
  const int d = S.d, nc = cl.n, ne = nb + 1, cells = nb * nb, tid = threadIdx.x;
  const int64_t i = blockIdx.x;
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  if (tid == 0) n_used[i] = t;
  const double* ge = edges + i * edge_stride;
  const int64_t oldest = ring.nh - t;
  double* le = reinterpret_cast<double*>(mhx_lds_raw);
  int32_t* cnt = reinterpret_cast<int32_t*>(le + nc * ne);
  int32_t* inside = cnt + np * cells;
  int32_t* nan = inside + np;
  unsigned short* place = reinterpret_cast<unsigned short*>(nan + nc);
  if (use_lds) {
    for (int f = tid; f < nc * ne; f += kPctThreads) le[f] = ge[f];
    for (int f = tid; f < np * cells + np + nc; f += kPctThreads) cnt[f] = 0;
    __syncthreads();
    const int ds = kPctThreads / d, dp = kPctThreads - ds * d;
    int s = tid / d, p = tid - s * d;
    for (int f = tid; f < t * d; f += kPctThreads) {
      const int c = cl.of_param[p];
      if (c >= 0) {
        const int64_t slot = (oldest + s) & (int64_t)ring.mask;
        const int k = histo_slot(le + c * ne, nb, ring.theta[slot * d + p]);
        if (k < 0) nan[c] = 1;
        place[c * ipitch + s] = (unsigned short)k;
      }
      s += ds;
      p += dp;
      if (p >= d) {
        p -= d;
        ++s;
      }
    }
    __syncthreads();
  }
  for (int q = 0; q < np; ++q) {
    const int a = pairs[q], b = pairs[np + q];
    int local = 0, bad = 0;
    for (int s = tid; s < t; s += kPctThreads) {
      int ka, kb;
      if (use_lds) {
        ka = place[a * ipitch + s];
        kb = place[b * ipitch + s];
      } else {
        const double* row = ring.theta + ((oldest + s) & (int64_t)ring.mask) * d;
        ka = histo_slot(ge + a * ne, nb, row[cl.idx[a]]);
        kb = histo_slot(ge + b * ne, nb, row[cl.idx[b]]);
        bad |= (ka < 0 || kb < 0) ? 1 : 0;
      }
      if (ka >= 1 && ka <= nb && kb >= 1 && kb <= nb) {
        const int cell = (ka - 1) * nb + (kb - 1);
        if (use_lds)
          atomicAdd(&cnt[q * cells + cell], 1);
        else
          atomicAdd(&counts[(i * np + q) * cells + cell], 1);
        ++local;
      }
    }
    const int total = wave_sum_i(local);
    if (lane_id() == 0 && total > 0) {
      if (use_lds)
        atomicAdd(&inside[q], total);
      else
        atomicAdd(&n_inside[i * np + q], total);
    }
    if (bad) status[i * np + q] = 1;
  }
  if (!use_lds) return;
  __syncthreads();
  for (int f = tid; f < np * cells; f += kPctThreads) counts[i * np * cells + f] = cnt[f];
  for (int q = tid; q < np; q += kPctThreads) {
    n_inside[i * np + q] = inside[q];
    status[i * np + q] = (nan[pairs[q]] | nan[pairs[np + q]]) != 0 ? 1 : 0;
  }
}

// mhx_get_autocorr (include/mhx.h has the definitions; they fix every bit).  One workgroup of
// kPctThreads per chain; x_0 is the NEWEST step of the window.
//   1 the window's rows - t x d contiguous doubles, two runs when the ring has wrapped - are read
//     ONCE, coalesced, as k_percentiles reads them; the requested columns are laid down in LDS
//     newest first, one column of `tpad` doubles each; a value that is not finite marks its column
//   2 the serial sums ahead of the lags: column c belongs to wave c % kPctWaves, and three lanes
//     of that wave walk it at once - the mean, the newer half's mean and then variance, the older
//     half's - in one loop of uniform length, so a wave keeps 3 x (its columns) chains in flight;
//     the column is then rewritten in place as dev_s = x_s - m
//   3 a task is (column, 256 lags), dealt over the waves: lane l runs the serial sums of the lags
//     256 g + 64 j + l, j = 0..3 - four independent chains of adds - over s.  dev_s is one address
//     for the whole wave (a broadcast), dev_{s + k} consecutive addresses across the lanes (free
//     of bank conflicts): the defined order is the fast one, and no sum crosses lanes.  The loop
//     runs unpredicated while every lane's s + k stays below t, the rest under a select (what a
//     lane reads past its column - at most 255 doubles, kAcTail - is never added)
//   4 c_k goes to the portion's acf piece, c_0 to LDS besides; the thread that wrote c_k then
//     replaces it by rho_k = c_k / c_0
//   5 one thread per column forms Geyer's sum from the written rho, tau, ess and the status
// use_lds = 0 (the columns do not fit, or MHX_AUTOCORR_NO_LDS): the same arithmetic, every x read
// from ring.theta and dev formed as it is used - x_s - m rounds the same wherever it is done.
constexpr int kAcLagsPerTask = 4 * kWave;
constexpr int kAcTail = kAcLagsPerTask;  // doubles after the last column that a lane may read
template <bool kLds>
__device__ __forceinline__ void autocorr_body(const Ring& ring, const ColList& cl, int t, int L,
                                              int nl, int tpad, int64_t i, double* acf, double* tau,
                                              double* ess, double* half_mean, double* half_var,
                                              int32_t* status) {
  const int d = ring.d, nc = cl.n, tid = threadIdx.x, w = wave_in_group(), l = lane_id();
  double* col = reinterpret_cast<double*>(mhx_lds_raw);
  double* mean_of = col + (kLds ? (size_t)nc * tpad + kAcTail : 0);
  double* c0_of = mean_of + nc;
  int32_t* bad_of = reinterpret_cast<int32_t*>(c0_of + nc);
  for (int c = tid; c < nc; c += kPctThreads) mean_of[c] = 0.0, c0_of[c] = 0.0, bad_of[c] = 0;
  __syncthreads();
  {  // 1: element f = s d + p of the window, oldest row first
    const int64_t oldest = ring.nh - t;
    const int ds = kPctThreads / d, dp = kPctThreads - ds * d;
    int s = tid / d, p = tid - s * d;
    for (int f = tid; f < t * d; f += kPctThreads) {
      const int c = cl.of_param[p];
      if (c >= 0) {
        const int64_t slot = (oldest + s) & (int64_t)ring.mask;
        const double v = ring.theta[slot * d + p];
        if (!finite_f64(v)) bad_of[c] = 1;
        if (kLds) col[(size_t)c * tpad + (t - 1 - s)] = v;
      }
      s += ds;
      p += dp;
      if (p >= d) {
        p -= d;
        ++s;
      }
    }
  }
  __syncthreads();
  auto x_at = [&](int c, int s) -> double {
    return kLds ? col[(size_t)c * tpad + s] : ring.theta[(int64_t)ring.slot(s) * d + cl.idx[c]];
  };
  const int h = t / 2;
  {  // 2: lane 3 q + j of wave w, column w + kPctWaves q: j = 0 the window, 1 and 2 its halves
    const int q = l / 3, j = l - 3 * q, c = w + kPctWaves * q;
    const bool mine = l < 48 && c < nc;
    const int cc = mine ? c : 0, start = j == 2 ? t - h : 0, len = mine ? (j == 0 ? t : h) : 0;
    const int last = t > 0 ? t - 1 : 0;
    double sum = x_at(cc, start < last ? start : last);
#pragma unroll 8
    for (int s = 1; s < t; ++s) {
      const int u = start + s;
      const double x = x_at(cc, u < last ? u : last);
      sum = s < len ? sum + x : sum;
    }
    const double m = sum / (double)len;
    if (mine && j == 0 && t > 0) mean_of[c] = m;
    if (mine && j > 0 && h > 0) {
      const double u0 = x_at(cc, start) - m;
      double sq = u0 * u0;
#pragma unroll 8
      for (int s = 1; s < h; ++s) {
        const double u = x_at(cc, start + s) - m;
        sq = sq + u * u;
      }
      half_mean[(i * nc + c) * 2 + (j - 1)] = m;
      half_var[(i * nc + c) * 2 + (j - 1)] = sq / (double)(h - 1);
    }
  }
  __syncthreads();
  if (kLds) {
    for (int f = tid; f < nc * t; f += kPctThreads) {
      const int c = f / t, s = f - c * t;
      col[(size_t)c * tpad + s] = col[(size_t)c * tpad + s] - mean_of[c];
    }
    __syncthreads();
  }
  // 3, 4: the lags
  const int ngrp = (L + kAcLagsPerTask) / kAcLagsPerTask;  // L = -1 (no step): none
  for (int T = w; T < nc * ngrp; T += kPctWaves) {
    const int c = T / ngrp, g = T - c * ngrp, k0 = kAcLagsPerTask * g + l;
    const double m = mean_of[c];
    auto dev = [&](int s) -> double { return kLds ? col[(size_t)c * tpad + s] : x_at(c, s) - m; };
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    // s + k < t for every lag of the task while s < t - 256 g - 255
    const int s_all = t - kAcLagsPerTask * g - (kAcLagsPerTask - 1), s_end = t - kAcLagsPerTask * g;
    int s = 0;
#pragma unroll 4
    for (; s < s_all; ++s) {
      const double a = dev(s);
      const int u = s + k0;
      a0 = a0 + a * dev(u);
      a1 = a1 + a * dev(u + kWave);
      a2 = a2 + a * dev(u + 2 * kWave);
      a3 = a3 + a * dev(u + 3 * kWave);
    }
    for (; s < s_end; ++s) {
      const double a = dev(s);
      const int u = s + k0;
      if (kLds) {
        const double b0 = dev(u), b1 = dev(u + kWave), b2 = dev(u + 2 * kWave), b3 = dev(u + 3 * kWave);
        a0 = u < t ? a0 + a * b0 : a0;
        a1 = u + kWave < t ? a1 + a * b1 : a1;
        a2 = u + 2 * kWave < t ? a2 + a * b2 : a2;
        a3 = u + 3 * kWave < t ? a3 + a * b3 : a3;
      } else {
        if (u < t) a0 = a0 + a * dev(u);
        if (u + kWave < t) a1 = a1 + a * dev(u + kWave);
        if (u + 2 * kWave < t) a2 = a2 + a * dev(u + 2 * kWave);
        if (u + 3 * kWave < t) a3 = a3 + a * dev(u + 3 * kWave);
      }
    }
    double* out = acf + (i * nc + c) * nl;
    const double av[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + j * kWave;
      if (k <= L) {
        const double ck = av[j] / (double)t;
        out[k] = ck;
        if (k == 0) c0_of[c] = ck;
      }
    }
  }
  __syncthreads();
  for (int T = w; T < nc * ngrp; T += kPctWaves) {
    const int c = T / ngrp, g = T - c * ngrp, k0 = kAcLagsPerTask * g + l;
    double* out = acf + (i * nc + c) * nl;
    const double c0v = c0_of[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + j * kWave;
      if (k <= L) out[k] = out[k] / c0v;
    }
  }
  __threadfence_block();
  __syncthreads();
  // 5: column 4 l + w, so that the columns spread over the waves
  const int c = kPctWaves * l + w;
  if (c < nc) {
    const double* rho = acf + (i * nc + c) * nl;
    double sum = 0.0;
    bool open = true;
    for (int j = 0; 2 * j + 1 <= L; ++j) {
      const double pj = rho[2 * j] + rho[2 * j + 1];
      if (!(pj > 0.0)) {
        open = false;
        break;
      }
      sum = sum + pj;
    }
    const double c0v = c0_of[c];
    const bool constant = c0v == 0.0;
    const double tv = constant ? c0v / c0v : 2.0 * sum - 1.0;
    tau[i * nc + c] = tv;
    ess[i * nc + c] = (double)t / tv;
    status[i * nc + c] = (bad_of[c] ? MHX_AUTOCORR_NONFINITE : 0) | (constant ? MHX_AUTOCORR_CONSTANT : 0) |
                         (open ? MHX_AUTOCORR_OPEN : 0);
  }
}
// acf [n][nc][max_lag + 1], tau / ess / status [n][nc], half_mean / half_var [n][nc][2], n_lags /
// n_used [n]
__global__ __launch_bounds__(kPctThreads) void k_autocorr(
    ChainState S, int64_t c0, int take, ColList cl, int max_lag, int use_lds, int tpad, double* acf,
    double* __restrict__ tau, double* __restrict__ ess, double* __restrict__ half_mean,
    double* __restrict__ half_var, int32_t* __restrict__ n_lags, int32_t* __restrict__ n_used,
    int32_t* __restrict__ status) {
  const int64_t i = blockIdx.x;
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  const int L = max_lag < t - 1 ? max_lag : t - 1;
  if (threadIdx.x == 0) n_used[i] = t, n_lags[i] = L;
  if (use_lds)
    autocorr_body<true>(ring, cl, t, L, max_lag + 1, tpad, i, acf, tau, ess, half_mean, half_var, status);
  else
    autocorr_body<false>(ring, cl, t, L, max_lag + 1, tpad, i, acf, tau, ess, half_mean, half_var, status);
}

// mhx_get_ensemble_percentiles: one pass of the radix selection over the POOL of all included
// chains' windows (include/mhx.h has the definitions, mhx_ensemble.hpp the host's half).  One
// workgroup of kPctThreads per chain of the engine; an excluded chain's workgroup returns at once.
//   1 the window's rows - t x d contiguous doubles, two runs when the ring has wrapped - are read
//     ONCE, coalesced, as k_percentiles and k_autocorr read them; the requested columns are laid
//     down in LDS as order keys, one column of `tpad` keys each
//   2 wave w takes the tasks w, w + kPctWaves, ...: it walks the task's column, keeps the keys
//     whose bits above the task's digit equal the task's prefix, and adds 1 to the digit's bin of
//     its own 256-bin uint32 histogram in LDS (a window holds at most ring-capacity steps)
//   3 every non-zero bin goes to the task's uint64 counters in memory with one integer atomic add
// ENS_COUNT_FIRST (pass 0, whose tasks are one per column with no prefix) also writes n_used and
// flags the columns that hold a NaN (the only value whose key is all ones).
// ENS_SUCCESSOR: a task's prefix is a whole key; the wave finds the least key of the column above
// it (one masked min-reduction, as select_percentile's) and hands it to the task's counter with
// one integer atomic min.
// Integer additions and minima only: thread order, workgroup order and the split of the chains
// over devices cannot change a bit.  No workgroup waits for another.
// use_lds = 0 (the columns do not fit, or MHX_ENSEMBLE_NO_LDS): every pass reads the column from
// ring.theta with stride d; only the histograms are in LDS.
template <bool kLds>
__device__ __forceinline__ void ensemble_body(const Ring& ring, const ColList& cl, int t, int tpad,
                                              const EnsTask* __restrict__ tasks, int n_tasks, int mode,
                                              unsigned long long* counters, int32_t* nan_flag) {
  const int d = ring.d, nc = cl.n, tid = threadIdx.x, w = wave_in_group(), l = lane_id();
  unsigned long long* col = reinterpret_cast<unsigned long long*>(mhx_lds_raw);
  unsigned int* hist = reinterpret_cast<unsigned int*>(col + (kLds ? (size_t)nc * tpad : 0)) + w * kEnsBins;
  if (kLds) {  // 1: element f = s d + p of the window, oldest row first
    const int64_t oldest = ring.nh - t;
    const int ds = kPctThreads / d, dp = kPctThreads - ds * d;
    int s = tid / d, p = tid - s * d;
    for (int f = tid; f < t * d; f += kPctThreads) {
      const int c = cl.of_param[p];
      if (c >= 0) {
        const int64_t slot = (oldest + s) & (int64_t)ring.mask;
        col[(size_t)c * tpad + s] = order_key(ring.theta[slot * d + p]);
      }
      s += ds;
      p += dp;
      if (p >= d) {
        p -= d;
        ++s;
      }
    }
    __syncthreads();
  }
  auto key_at = [&](int c, int s) -> unsigned long long {
    return kLds ? col[(size_t)c * tpad + s] : order_key(ring.theta[(int64_t)ring.slot(s) * d + cl.idx[c]]);
  };
  // every wave goes round as often as the busiest, so that the barriers are the workgroup's
  for (int T0 = 0; T0 < n_tasks; T0 += kPctWaves) {
    const int T = T0 + w;
    const bool mine = T < n_tasks;
    const EnsTask tk = tasks[mine ? T : 0];
    const int c = tk.col;
    if (mode == ENS_SUCCESSOR) {
      if (!mine) continue;
      unsigned long long m = ~0ULL;
      for (int s = l; s < t; s += kWave) {
        const unsigned long long key = key_at(c, s);
        if (key > tk.prefix && key < m) m = key;
      }
      m = wave_min_u64(m);
      // the counter only ever falls: a chain whose least key is not below what it reads there has
      // nothing to hand in (a stale read only costs a minimum that changes nothing), which spares
      // most of the workgroups an atomic on an address they all share
      if (l == 0 && m < __hip_atomic_load(&counters[T], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&counters[T], m);
      continue;
    }
    for (int b = l; b < kEnsBins; b += kWave) hist[b] = 0;
    __syncthreads();
    if (mine) {
      const unsigned long long mask = tk.shift >= 56 ? 0ULL : ~0ULL << (tk.shift + 8);
      bool nan = false;
      for (int s = l; s < t; s += kWave) {
        const unsigned long long key = key_at(c, s);
        if ((key & mask) == tk.prefix) atomicAdd(&hist[(unsigned)(key >> tk.shift) & (kEnsBins - 1)], 1u);
        nan = nan || key == ~0ULL;
      }
      if (mode == ENS_COUNT_FIRST && nan) atomicOr(&nan_flag[c], 1);
    }
    __syncthreads();
    if (mine)
      for (int b = l; b < kEnsBins; b += kWave) {
        const unsigned int h = hist[b];
        if (h != 0) atomicAdd(&counters[(size_t)T * kEnsBins + b], (unsigned long long)h);
      }
  }
}
// tasks [n_tasks]; counters [n_tasks][kEnsBins] zeroed (ENS_SUCCESSOR: [n_tasks], all ones);
// include [chains] or NULL; n_used [chains] and nan_flag [cl.n] zeroed ahead of ENS_COUNT_FIRST
__global__ __launch_bounds__(kPctThreads) void k_ensemble_digits(
    ChainState S, int take, ColList cl, const uint8_t* __restrict__ include,
    const EnsTask* __restrict__ tasks, int n_tasks, int mode, int use_lds, int tpad,
    unsigned long long* counters, int32_t* __restrict__ n_used, int32_t* nan_flag) {
  const int64_t i = blockIdx.x;
  if (include && include[i] == 0) return;
  const Ring ring = ring_of(S, i);
  const int t = ring_held(ring, take);
  if (mode == ENS_COUNT_FIRST && threadIdx.x == 0) n_used[i] = t;
  if (use_lds)
    ensemble_body<true>(ring, cl, t, tpad, tasks, n_tasks, mode, counters, nan_flag);
  else
    ensemble_body<false>(ring, cl, t, tpad, tasks, n_tasks, mode, counters, nan_flag);
}

// mhx_get_derived, second half: the posterior summaries of the values mhx_user_derived left in
// the portion's staging buffer, vals [n][ne][pitch] newest first.  One workgroup of kPctWaves
// wavefronts per chain, as k_percentiles, the expressions in the parameters' place.
//   use_lds = 1: the t values of every expression are laid down as keys, one column of `tpad`
//     slots each (read once, unit stride); the selections and the sums run from there
//   use_lds = 0 (ne * tpad * 8 bytes do not fit): both read the staging buffer
// mean M:1518-1519 and standard-deviation M:1521-1527: lane q of the LAST wave walks expression
// q's column newest first - the serial sum, one division; then the serial sum of
// (v - mean) * (v - mean), / (n - 1), sqrt (n = 1: 0/0, a NaN) - and notes a value that is not
// finite (status).  A NaN read back from a key is the canonical one: any NaN makes both sums NaN.
// pct [n][n_pct][ne], mean / stddev / status [n][ne], n_used [n].
__global__ __launch_bounds__(kPctThreads) void k_derived_summary(
    ChainState S, int64_t c0, int take, int ne, int pitch, PctList pc, int use_lds, int tpad,
    const double* __restrict__ vals, double* __restrict__ pct, double* __restrict__ mean,
    double* __restrict__ stddev, int32_t* __restrict__ n_used, int32_t* __restrict__ status) {
  unsigned long long* col = reinterpret_cast<unsigned long long*>(mhx_lds_raw);
  const int w = wave_in_group(), l = lane_id();
  const int64_t i = blockIdx.x;
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  const double* v = vals + i * (int64_t)ne * pitch;
  if (threadIdx.x == 0) n_used[i] = t;
  if (use_lds) {
    for (int q = 0; q < ne; ++q)
      for (int s = threadIdx.x; s < t; s += kPctThreads)
        col[(size_t)q * tpad + s] = order_key(v[(int64_t)q * pitch + s]);
    __syncthreads();
  }
  if (w == kPctWaves - 1 && l < ne) {
    const unsigned long long* cp = col + (size_t)l * tpad;
    const double* vp = v + (int64_t)l * pitch;
    auto at = [&](int s) -> double { return use_lds ? key_value(cp[s]) : vp[s]; };
    double m = 0.0, sd = 0.0;
    bool bad = false;
    if (t > 0) {
      double sum = at(0);
      bad = !finite_f64(sum);
      for (int s = 1; s < t; ++s) {
        const double x = at(s);
        bad = bad || !finite_f64(x);
        sum = sum + x;
      }
      m = sum / (double)t;
      double sq = (at(0) - m) * (at(0) - m);
      for (int s = 1; s < t; ++s) {
        const double u = at(s) - m;
        sq = sq + u * u;
      }
      sd = __builtin_sqrt(sq / (double)(t - 1));
    }
    mean[i * ne + l] = m;
    stddev[i * ne + l] = sd;
    status[i * ne + l] = bad ? 1 : 0;
  }
  for (int q = w; q < ne; q += kPctWaves)
    for (int k = 0; k < pc.n; ++k) {
      double r = 0.0;
      if (t > 0) {
        int64_t pos;
        int32_t between;
        percentile_rank_of(t, pc.num[k], pc.den[k], &pos, &between);
        if (use_lds) {
          const unsigned long long* cp = col + (size_t)q * tpad;
          r = select_percentile([&](int s) { return cp[s]; }, t, (int)pos, between != 0);
        } else {
          const double* vp = v + (int64_t)q * pitch;
          r = select_percentile([&](int s) { return order_key(vp[s]); }, t, (int)pos, between != 0);
        }
      }
      if (l == 0) pct[(i * pc.n + k) * ne + q] = r;
    }
}

// mhx_get_hdi / mhx_get_derived_hdi (include/mhx.h has the definition): the only read-out that
// ORDERS a window.  A column's values are laid down as order keys in n = the least power of two
// >= max(t, 2) slots, the slots past t holding the greatest key (a NaN's: both sort last), and
// sorted by a bitonic network: the merges of size k = 2, 4, .. n, each the passes of stride k/2
// .. 1, a pass n/2 independent compare-exchanges.  The trip counts depend on n alone; the sorted
// order of keys is unique, so any schedule of the network gives the same bits.
//
// hdi_network runs, on the n keys a[0 .. n) that stand at places base .. base + n of their
// sequence, the passes of the merges k0 .. k1 whose stride is below n.  kWaveOnly: one wavefront
// owns the keys and a pass ends at a wave barrier; else the workgroup, at __syncthreads.
template <bool kWaveOnly>
__device__ __forceinline__ void hdi_pass_end() {
  if (kWaveOnly) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}
template <bool kWaveOnly>
__device__ __forceinline__ void hdi_network(unsigned long long* a, int n, int base, int k0, int k1) {
  const int me = kWaveOnly ? lane_id() : (int)threadIdx.x, nt = kWaveOnly ? kWave : kPctThreads;
  const int half = n >> 1;
  for (int k = k0; k <= k1; k <<= 1)
    for (int j = k >> 1 < half ? k >> 1 : half; j >= 1; j >>= 1) {
      for (int p = me; p < half; p += nt) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const bool up = ((base + i) & k) == 0;
        const unsigned long long x = a[i], y = a[i + j];
        if ((x > y) == up) {
          a[i] = y;
          a[i + j] = x;
        }
      }
      hdi_pass_end<kWaveOnly>();
    }
}
// The narrowest interval of span g among the sorted keys key_at(0 .. t), by one wavefront: lanes
// stride over j, each keeps its least width w_j = s_{j+g} - s_j (one IEEE subtraction; finite
// widths are non-negative, so their bits order as integers) at its lowest j; the wave's least
// width, then the least j among the lanes that hold it.  All lanes return the same j; where a
// width is a NaN (a column that is not finite) any j in range.
template <class KeyAt>
__device__ __forceinline__ int hdi_narrowest(KeyAt key_at, int t, int g) {
  unsigned long long best = ~0ULL, at = ~0ULL;
  for (int j = lane_id(); j + g < t; j += kWave) {
    const unsigned long long b = bits_of(key_value(key_at(j + g)) - key_value(key_at(j)));
    if (b < best || at == ~0ULL) best = b, at = (unsigned long long)j;
  }
  const unsigned long long least = wave_min_u64(best);
  const unsigned long long j = wave_min_u64(best == least ? at : ~0ULL);
  return j > (unsigned long long)(t - 1 - g) ? 0 : (int)j;
}
// What one sorted column gives, written by `parts` wavefronts of which this is wave `part`: the
// intervals (a mass to a wave), the ladder (its ranks over all lanes) and the status.
template <class KeyAt>
__device__ __forceinline__ void hdi_outputs(KeyAt key_at, int t, const HdiArgs& A, int64_t i, int c, int part,
                                            int parts) {
  const int l = lane_id(), nc = A.cl.n;
  for (int q = part; q < A.n_mass; q += parts) {
    const int g = (int)hdi_span_of(t, A.mass_num[q], A.mass_den[q]);
    const int j = hdi_narrowest(key_at, t, g);
    if (l == 0) {
      const int64_t o = (i * A.n_mass + q) * nc + c;
      A.lo[o] = key_value(key_at(j));
      A.hi[o] = key_value(key_at(j + g));
      A.pos[o] = j;
    }
  }
  const int L = A.n_ladder;
  for (int k = part * kWave + l; k < L; k += parts * kWave)
    A.ladder[(i * nc + c) * L + k] = key_value(key_at((int)((int64_t)k * (t - 1) / (L - 1))));
  if (part == 0 && l == 0) {
    // -inf has the least key a value can have, +inf the greatest below the NaNs'
    const bool bad = key_at(0) == 0x000fffffffffffffULL || key_at(t - 1) >= 0xfff0000000000000ULL;
    A.status[i * nc + c] = bad ? 1 : 0;
  }
}
// value s (any order of s within the window) of column c of chain i
__device__ __forceinline__ double hdi_value(const HdiArgs& A, const Ring& ring, int64_t i, int c, int s) {
  if (A.vals) return A.vals[i * A.vals_chain + c * A.vals_col + s * A.vals_step];
  return ring.theta[(int64_t)ring.slot(s) * ring.d + A.cl.idx[c]];
}
__global__ __launch_bounds__(kPctThreads) void k_hdi(ChainState S, HdiArgs A) {
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(mhx_lds_raw);
  const int w = wave_in_group(), tid = threadIdx.x, nc = A.cl.n, d = S.d;
  const int64_t i = A.use_lds ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / nc;
  const Ring ring = ring_of(S, A.c0 + i);
  const int t = ring_held(ring, A.take);
  int n = 2;
  while (n < t) n <<= 1;
  if (t == 0) {  // (no step held: nothing to order)
    if (A.use_lds || blockIdx.x % nc == 0) {
      if (tid == 0) A.n_used[i] = 0;
      for (int f = tid; f < A.n_mass * nc; f += kPctThreads)
        A.lo[i * A.n_mass * nc + f] = A.hi[i * A.n_mass * nc + f] = 0.0, A.pos[i * A.n_mass * nc + f] = 0;
      for (int f = tid; f < nc * A.n_ladder; f += kPctThreads) A.ladder[i * nc * A.n_ladder + f] = 0.0;
      for (int f = tid; f < nc; f += kPctThreads) A.status[i * nc + f] = 0;
    }
    return;
  }
  if (A.use_lds) {
    // one workgroup per chain: the window is read once, coalesced, by the whole workgroup; then
    // wave w sorts and reads out the columns w, w + kPctWaves, .. on its own
    const int cp = A.tpad + 1;
    if (tid == 0) A.n_used[i] = t;
    if (A.vals) {
      for (int c = 0; c < nc; ++c)
        for (int s = tid; s < n; s += kPctThreads)
          lds[(size_t)c * cp + s] = s < t ? order_key(hdi_value(A, ring, i, c, s)) : ~0ULL;
    } else {
      const int64_t oldest = ring.nh - t;
      const int ds = kPctThreads / d, dp = kPctThreads - ds * d;
      int s = tid / d, p = tid - s * d;
      for (int f = tid; f < t * d; f += kPctThreads) {
        const int c = A.cl.of_param[p];
        if (c >= 0) {
          const int64_t slot = (oldest + s) & (int64_t)ring.mask;
          lds[(size_t)c * cp + s] = order_key(ring.theta[slot * d + p]);
        }
        s += ds;
        p += dp;
        if (p >= d) {
          p -= d;
          ++s;
        }
      }
      for (int c = 0; c < nc; ++c)
        for (int s2 = t + tid; s2 < n; s2 += kPctThreads) lds[(size_t)c * cp + s2] = ~0ULL;
    }
    __syncthreads();
    for (int c = w; c < nc; c += kPctWaves) {
      unsigned long long* a = lds + (size_t)c * cp;
      hdi_network<true>(a, n, 0, 2, n);
      hdi_outputs([&](int s) { return a[s]; }, t, A, i, c, 0, 1);
    }
    return;
  }
  // one workgroup per (chain, column): the keys in the stage piece, sub-sequences of kHdiChunk
  // keys finished in LDS, the passes of a greater stride in memory
  const int c = (int)(blockIdx.x - i * nc);
  unsigned long long* g = A.keys + (i * nc + c) * (int64_t)A.tpad;
  if (c == 0 && tid == 0) A.n_used[i] = t;
  const int ch = n < kHdiChunk ? n : kHdiChunk;
  // the sub-sequence from `base` on through the merges k0 .. k1 in LDS; from_src: the keys are
  // formed from the column's values, not read back
  auto in_lds = [&](int base, int k0, int k1, bool from_src) {
    for (int s = tid; s < ch; s += kPctThreads)
      lds[s] = !from_src ? g[base + s] : base + s < t ? order_key(hdi_value(A, ring, i, c, base + s)) : ~0ULL;
    __syncthreads();
    hdi_network<false>(lds, ch, base, k0, k1);
    if (n > ch) {
      for (int s = tid; s < ch; s += kPctThreads) g[base + s] = lds[s];
      __syncthreads();
    }
  };
  for (int base = 0; base < n; base += ch) in_lds(base, 2, ch, true);
  for (int k = ch << 1; k <= n; k <<= 1) {
    for (int j = k >> 1; j >= ch; j >>= 1) {
      for (int p = tid; p < (n >> 1); p += kPctThreads) {
        const int e = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const bool up = (e & k) == 0;
        const unsigned long long x = g[e], y = g[e + j];
        if ((x > y) == up) {
          g[e] = y;
          g[e + j] = x;
        }
      }
      __syncthreads();
    }
    for (int base = 0; base < n; base += ch) in_lds(base, k, k, false);
  }
  // (a window of one chunk is still in LDS; a longer one is read from its piece)
  if (n > ch)
    hdi_outputs([&](int s) { return g[s]; }, t, A, i, c, w, kPctWaves);
  else
    hdi_outputs([&](int s) { return lds[s]; }, t, A, i, c, w, kPctWaves);
}

// mhx_get_covariances: :covariance-matrix M:541 = lplist-covariance (M:614-643) of :unique-steps
// (M:492-496), one wavefront per chain.  uniq: [n][take] ring slots of the unique steps, newest
// first (compacted in order like ring_forward_list); cov [n][d][d].
__global__ __launch_bounds__(kThreads) void k_covariances(ChainState S, int64_t c0, int64_t n,
                                                         int take, int* __restrict__ uniq_all,
                                                         double* __restrict__ cov_all,
                                                         int32_t* __restrict__ n_unique,
                                                         int32_t* __restrict__ status) {
  __shared__ double avg_all[kWavesPerGroup][MHX_MAX_PARAMS + 1];
  const int w = wave_in_group(), l = lane_id(), d = S.d;
  const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + w;
  if (i >= n) return;
  const Ring r = ring_of(S, c0 + i);
  const int t = ring_held(r, take);
  int* uniq = uniq_all + i * take;
  double* cov = cov_all + i * d * d;
  double* avg = avg_all[w];
  int nu = 0;
  for (int base = 0; base < t; base += kWave) {
    const int s = base + l;
    bool f = false;
    if (s < t) {
      const bool last = s == t - 1;
      const double a = r.prob[r.slot(s)];
      const double b = last ? 0.0 : r.prob[r.slot(s + 1)];
      f = last || bits_of(a) != bits_of(b);
    }
    const unsigned long long m = __ballot(f);
    const int pos = nu + __popcll(m & ((1ULL << l) - 1ULL));
    if (f) uniq[pos] = r.slot(s);
    nu += __popcll(m);
  }
  __threadfence();
  int st = L_OK;
  if (nu == 0) {  // (no history at all: nothing the reference could be asked about)
    for (int e = l; e < d * d; e += kWave) cov[e] = 0.0;
    st = L_CAUGHT;
  } else {
    const double dn = (double)nu;
    auto x = [&](int k, int p) -> double { return r.theta[(int64_t)uniq[k] * d + p]; };
    // averages M:626: (/ (reduce #'+ x) n)
    if (l < d) {
      double s = x(0, l);
      for (int k = 1; k < nu; ++k) s = s + x(k, l);
      const double a = s / dn;
      avg[l] = a;
      st = trap_of(a);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // covariance M:636-643 (the /n sits inside the accumulation; multiply, divide, add)
    for (int e = l; e < d * d; e += kWave) {
      const int a = e / d, b = e - a * d;
      const double aa = avg[a], ab = avg[b];
      double mini = 0.0;
      for (int k = 0; k < nu; ++k) {
        const double u = x(k, a) - aa, v = x(k, b) - ab;
        mini = mini + (u * v) / dn;
      }
      cov[e] = mini;
      if (st == L_OK) st = trap_of(mini);
    }
  }
  const bool bad = __ballot(st != L_OK) != 0ULL;
  if (l == 0) {
    n_unique[i] = nu;
    status[i] = bad ? L_CAUGHT : L_OK;
  }
}

// mhx_get_traces: the steps of every chain's window, filtered (MHX_TRACE_*: :steps, :unique-steps
// M:492-496, :forward-steps M:497-502) and thinned (`thin` M:149-157), one wavefront per chain.
// 1. compact: blocks of 64 steps, newest first; a ballot and a prefix count give every kept step
//    its place in kept [n][take] (ring slots), as in ring_forward_list.  MHX_TRACE_STEPS keeps
//    every step: item i is slot(i) and the list is not written.
// 2. gather: (row r, column j) is flattened over the lanes, so a row's n_cols values are written
//    side by side and read from one theta[slot][0 .. d) line.  The lane that owns (r, j) walks its
//    bucket - kept items start + r stride .. - in order and carries lo / hi in registers: the
//    sequential definition of include/mhx.h, no reduction.  lo / hi may be nullptr, each alone.
// cols [n_cols]: a parameter, or MHX_TRACE_PROB.  values, lo, hi [n][max_out][n_cols] and the
// counts come zeroed from the host: rows from n_out on are left as they are.
__global__ __launch_bounds__(kThreads) void k_traces(ChainState S, int64_t c0, int64_t n, int take,
                                                    int filter, int stride, int start, int n_cols,
                                                    int max_out, const int32_t* __restrict__ cols,
                                                    int* __restrict__ kept_all,
                                                    double* __restrict__ values_all,
                                                    double* __restrict__ lo_all,
                                                    double* __restrict__ hi_all,
                                                    int32_t* __restrict__ n_out,
                                                    int32_t* __restrict__ n_kept,
                                                    int32_t* __restrict__ n_used) {
  const int w = wave_in_group(), l = lane_id(), d = S.d;
  const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + w;
  if (i >= n) return;
  const Ring r = ring_of(S, c0 + i);
  const int t = ring_held(r, take);
  int* kept = kept_all + i * take;
  int nk = t;
  if (filter != MHX_TRACE_STEPS) {
    const bool uniq = filter == MHX_TRACE_UNIQUE;
    nk = 0;
    for (int base = 0; base < t; base += kWave) {
      const int s = base + l;
      bool f = false;
      if (s < t) {
        const bool last = s == t - 1;
        const double a = r.prob[r.slot(s)];
        const double b = last ? 0.0 : r.prob[r.slot(s + 1)];
        f = uniq ? (last || bits_of(a) != bits_of(b)) : (!last && !(a <= b));
      }
      const unsigned long long m = __ballot(f);
      const int pos = nk + __popcll(m & ((1ULL << l) - 1ULL));
      if (f) kept[pos] = r.slot(s);
      nk += __popcll(m);
    }
    __threadfence();
  }
  const int rows = nk <= start ? 0 : (nk - start + stride - 1) / stride;
  const int no = rows < max_out ? rows : max_out;
  if (l == 0) {
    n_out[i] = no;
    n_kept[i] = nk;
    n_used[i] = t;
  }
  const bool envelope = lo_all != nullptr || hi_all != nullptr;
  const int64_t at = i * (int64_t)max_out * n_cols;
  auto slot_of = [&](int k) { return filter == MHX_TRACE_STEPS ? r.slot(k) : kept[k]; };
  for (int e = l; e < no * n_cols; e += kWave) {
    const int row = e / n_cols, j = e - row * n_cols, col = cols[j];
    auto value_of = [&](int k) {
      const int slot = slot_of(k);
      return col < 0 ? r.prob[slot] : r.theta[(int64_t)slot * d + col];
    };
    const int k0 = start + row * stride;
    const double first = value_of(k0);
    values_all[at + e] = first;
    if (envelope) {
      const int k1 = k0 + stride < nk ? k0 + stride : nk;
      double lo = first, hi = first;
      for (int k = k0 + 1; k < k1; ++k) {
        const double v = value_of(k);
        if (v < lo) lo = v;
        if (v > hi) hi = v;
      }
      if (lo_all) lo_all[at + e] = lo;
      if (hi_all) hi_all[at + e] = hi;
    }
  }
}

// mhx_get_proposal_factors: ring_l_matrix - the code k_l_matrix and the controller run - for
// every chain.  fwd [n][take], cov / out [n][d][d] (zeroed by the host, as for k_l_matrix).
__global__ __launch_bounds__(kThreads) void k_l_matrices(ChainState S, int64_t c0, int64_t n,
                                                        int take, int* __restrict__ fwd,
                                                        double* __restrict__ cov,
                                                        double* __restrict__ out,
                                                        int32_t* __restrict__ status,
                                                        int32_t* __restrict__ n_forward) {
  __shared__ double avg_all[kWavesPerGroup][MHX_MAX_PARAMS + 1];
  const int w = wave_in_group(), d = S.d;
  const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + w;
  if (i >= n) return;
  const Ring ring = ring_of(S, c0 + i);
  int nf = 0;
  const int st = ring_l_matrix(ring, take, fwd + i * take, cov + i * d * d, out + i * d * d,
                               (lds_dptr_t)avg_all[w], &nf);
  if (lane_id() == 0) {
    status[i] = st;
    n_forward[i] = nf;
  }
}

// mhx_get_window_best: :most-likely-step M:503-505 over the window.  The reference's reduce goes
// from the newest step to the oldest and keeps the step it holds only while that one is STRICTLY
// greater: of equal greatest probs the oldest wins.  Per lane over its strided share in that
// order, then a butterfly that carries the step index.
__global__ __launch_bounds__(kThreads) void k_window_best(ChainState S, int64_t c0, int64_t n,
                                                         int take, double* __restrict__ prob,
                                                         double* __restrict__ theta) {
  const int w = wave_in_group(), l = lane_id(), d = S.d;
  const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + w;
  if (i >= n) return;
  const Ring r = ring_of(S, c0 + i);
  const int t = ring_held(r, take);
  double bv = 0.0;
  int bs = -1;
  for (int s = l; s < t; s += kWave) {
    const double v = r.prob[r.slot(s)];
    if (bs < 0 || !(bv > v)) {
      bv = v;
      bs = s;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(bv, m, 64);
    const int os = __shfl_xor(bs, m, 64);
    const bool take_other = os >= 0 && (bs < 0 || ov > bv || (ov == bv && os > bs));
    if (take_other) {
      bv = ov;
      bs = os;
    }
  }
  if (l == 0) prob[i] = bv;
  if (l < d) theta[i * d + l] = bs < 0 ? 0.0 : r.theta[(int64_t)r.slot(bs) * d + l];
}

// mhx_get_fit_bands, first half: which steps walker-get-data-and-fit envelopes (M:1249-1251).
// One wavefront per chain.  Candidates: ALL the steps the ring holds (the reference sorts the
// whole walk); k = min(ceiling(0.66 take_c), held) of them, take_c = min(take, walker-length),
// are selected - those of greatest prob, among equal probs the newer first, a NaN last.  A rank
// problem on the prob column: the radix selection of select_percentile on the descending key
// gives the threshold and how many steps AT the threshold belong, then one pass newest first
// compacts the slots of the selected steps into sel[i][0 .. k) (ballot + prefix count, the
// ties counted off as they come).  No sort.
__device__ __forceinline__ unsigned long long band_key(double v) {
  if (v != v) return ~0ULL;
  if (v == 0.0) v = 0.0;  // (-0 and +0 are one prob)
  return ~order_key(v);
}
__global__ __launch_bounds__(kThreads) void k_band_select(ChainState S, int64_t c0, int64_t n,
                                                         int take, int32_t* __restrict__ sel_all,
                                                         int32_t* __restrict__ n_sel) {
  const int w = wave_in_group(), l = lane_id();
  const int64_t i = (int64_t)blockIdx.x * kWavesPerGroup + w;
  if (i >= n) return;
  const Ring r = ring_of(S, c0 + i);
  const int held = ring_held(r, S.R);
  const int64_t take_c = r.length < (int64_t)take ? r.length : (int64_t)take;
  int64_t want = take_c >= 1 ? band_count_of(take_c) : 0;
  const int k = (int)(want < (int64_t)held ? want : (int64_t)held);
  if (l == 0) n_sel[i] = k;
  if (k <= 0) return;
  int32_t* sel = sel_all + i * take;
  auto key_at = [&](int s) { return band_key(r.prob[r.slot(s)]); };
  // the key of rank k - 1 and that rank's place among the steps that share it
  unsigned long long prefix = 0, mask = 0;
  int rank = k - 1;
  for (int b = 63; b >= 0; --b) {
    const unsigned long long bit = 1ULL << b;
    int cnt = 0;
    for (int s = l; s < held; s += kWave) {
      const unsigned long long key = key_at(s);
      cnt += ((key & mask) == prefix && (key & bit) == 0) ? 1 : 0;
    }
    const int z = __builtin_amdgcn_readfirstlane(wave_sum_i(cnt));
    if (rank >= z) {
      rank -= z;
      prefix |= bit;
    }
    mask |= bit;
  }
  const int ties = rank + 1;  // steps at the threshold that belong: the newest `ties` of them
  int pos = 0, seen = 0;
  for (int base = 0; base < held; base += kWave) {
    const int s = base + l;
    const unsigned long long key = s < held ? key_at(s) : ~0ULL;
    const bool in = s < held;
    const bool eq = in && key == prefix;
    const unsigned long long me = __ballot(eq);
    const unsigned long long below = (1ULL << l) - 1ULL;
    const bool f = in && (key < prefix || (eq && seen + __popcll(me & below) < ties));
    const unsigned long long mf = __ballot(f);
    if (f) sel[pos + __popcll(mf & below)] = r.slot(s);
    pos += __popcll(mf);
    seen += __popcll(me);
  }
}

// mhx_get_waic, the totals: one thread per chain adds the blocks' partial sums in block order
// (whatever launches wrote them), takes the one subtraction and completes n_used and the status
// (a one-step window; an empty one, whose 0/0 quotient is flagged as not finite).
__global__ __launch_bounds__(kThreads) void k_waic_totals(ChainState S, int64_t c0, int64_t n, int take,
                                                          int64_t nb_total,
                                                          const double* __restrict__ part_lppd,
                                                          const double* __restrict__ part_p,
                                                          const int32_t* __restrict__ part_high,
                                                          double* __restrict__ elpd,
                                                          double* __restrict__ lppd,
                                                          double* __restrict__ p_waic,
                                                          int32_t* __restrict__ n_high,
                                                          int32_t* __restrict__ n_used,
                                                          int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t c = c0 + i;
  int64_t t = S.length[c] < S.n_hist[c] ? S.length[c] : S.n_hist[c];
  if (t > (int64_t)take) t = take;
  if (t < 0) t = 0;
  double sl = 0.0, sp = 0.0;
  int nh = 0;
  for (int64_t b = 0; b < nb_total; ++b) {
    sl = sl + part_lppd[i * nb_total + b];
    sp = sp + part_p[i * nb_total + b];
    nh += part_high[i * nb_total + b];
  }
  lppd[i] = sl;
  p_waic[i] = sp;
  elpd[i] = sl - sp;
  n_high[i] = nh;
  n_used[i] = (int32_t)t;
  if (t == 1) status[i] = status[i] | MHX_WAIC_ONE_STEP;
  if (t == 0) status[i] = status[i] | MHX_WAIC_NONFINITE;  // (an empty walk: nothing to average)
}

// mhx_get_heldout, the totals: one thread per chain adds the blocks' partial sums in block order
// (whatever launches wrote them) and completes n_used and the status (no point used; an empty
// window, whose 0/0 quotient is flagged as not finite).
__global__ __launch_bounds__(kThreads) void k_heldout_totals(ChainState S, int64_t c0, int64_t n, int take,
                                                             int64_t nb_total,
                                                             const double* __restrict__ part_lpd,
                                                             const int32_t* __restrict__ part_scored,
                                                             double* __restrict__ lpd,
                                                             int32_t* __restrict__ n_scored,
                                                             int32_t* __restrict__ n_used,
                                                             int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t c = c0 + i;
  int64_t t = S.length[c] < S.n_hist[c] ? S.length[c] : S.n_hist[c];
  if (t > (int64_t)take) t = take;
  if (t < 0) t = 0;
  double sl = 0.0;
  int ns = 0;
  for (int64_t b = 0; b < nb_total; ++b) {
    sl = sl + part_lpd[i * nb_total + b];
    ns += part_scored[i * nb_total + b];
  }
  lpd[i] = sl;
  n_scored[i] = ns;
  n_used[i] = (int32_t)t;
  if (t == 0) status[i] = status[i] | MHX_HELDOUT_NONFINITE;  // (an empty walk: nothing to average)
  if (ns == 0) status[i] = status[i] | MHX_HELDOUT_NO_POINTS;
}

// mhx_get_residuals, the totals: one thread per chain adds the blocks' partial sums and counts in
// block order (whatever launches wrote them) and keeps the first of the blocks' greatest |z|.
__global__ __launch_bounds__(kThreads) void k_resid_totals(
    int64_t n, int64_t nb_total, const double* __restrict__ part_chi2, const double* __restrict__ part_sumz,
    const double* __restrict__ part_dw, const double* __restrict__ part_max,
    const int64_t* __restrict__ part_idx, const int32_t* __restrict__ part_cnt, double* __restrict__ chi2,
    double* __restrict__ sum_z, double* __restrict__ dw, double* __restrict__ max_abs_z,
    int64_t* __restrict__ max_index, int32_t* __restrict__ n_pos, int32_t* __restrict__ n_runs,
    int32_t* __restrict__ n_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double sc = 0.0, sz = 0.0, sd = 0.0, mx = -1.0;
  int64_t mi = -1;
  int np = 0, nc = 0, no = 0;
  for (int64_t b = 0; b < nb_total; ++b) {
    const int64_t o = i * nb_total + b;
    sc = sc + part_chi2[o];
    sz = sz + part_sumz[o];
    sd = sd + part_dw[o];
    np += part_cnt[o * 3 + 0];
    nc += part_cnt[o * 3 + 1];
    no += part_cnt[o * 3 + 2];
    if (part_max[o] > mx) mx = part_max[o], mi = part_idx[o];
  }
  chi2[i] = sc;
  sum_z[i] = sz;
  dw[i] = sd;
  max_abs_z[i] = mx;
  max_index[i] = mi;
  n_pos[i] = np;
  n_runs[i] = 1 + nc;
  n_out[i] = no;
}

// mhx_get_normal_equations, the totals: one thread per chain and task adds the blocks' partial sums
// in block order (whatever launches wrote them) and scatters the total through the function's gather
// map: task (a, b) to jtj[col a][col b] and its mirror, (a, p) to jtr[col a], (p, p) to chi2.  A
// column whose step is 0 is +0.0 exactly; what the function does not read was zeroed by the host.
__global__ __launch_bounds__(kThreads) void k_normeq_totals(NormEqArgs A, int d,
                                                            double* __restrict__ jtj,
                                                            double* __restrict__ jtr,
                                                            double* __restrict__ chi2) {
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (tid >= A.n * A.n_tasks) return;
  const int64_t i = tid / A.n_tasks;
  const int k = (int)(tid - i * A.n_tasks);
  int b = 0;
  while ((b + 1) * (b + 2) / 2 <= k) ++b;
  const int a = k - b * (b + 1) / 2;
  const double* part = A.part + i * A.nb_total * (int64_t)A.n_tasks + k;
  double s = 0.0;
  for (int64_t blk = 0; blk < A.nb_total; ++blk) s = s + part[blk * (int64_t)A.n_tasks];
  const double* hs = A.steps + i * A.steps_pitch;
  const int p = A.p;
  if (b == p) {
    if (a == p) {
      chi2[i] = s;
    } else {
      const int t = A.col[a];
      jtr[i * d + t] = hs[t] == 0.0 ? 0.0 : s;
    }
  } else {
    const int t = A.col[a], u = A.col[b];
    const double v = (hs[t] == 0.0 || hs[u] == 0.0) ? 0.0 : s;
    jtj[(i * d + t) * d + u] = v;
    jtj[(i * d + u) * d + t] = v;
  }
}

// mhx_get_candidate_scores, totals and ranking: one wave per chain.  Lane l takes candidates l,
// l + 64, ...: a function's blocks are added in block order to a sum that starts at 0.0 (chi2_k,
// the bits of mhx_get_residuals), the functions' sums in ascending k to a total that starts at 0.0;
// a total that is not finite - a NaN block is one of its terms where a value or residual was not -
// becomes +infinity and counts in n_bad.  Then `keep` passes, each the wave's lexicographic minimum
// of (score, index) over the candidates above the one taken last: no flags are kept.  No score is a
// NaN, so every comparison is decided; index INT32_MAX stands for "none left" and is stored as -1.
__global__ __launch_bounds__(kWave) void k_cand_totals(const ProblemDesc* __restrict__ Pp, int fn,
                                                       int64_t n, int64_t m_cand, int64_t nb_pitch,
                                                       int keep, const double* __restrict__ part,
                                                       double* __restrict__ score,
                                                       int32_t* __restrict__ best_index,
                                                       double* __restrict__ best_score,
                                                       int32_t* __restrict__ n_bad) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int l = threadIdx.x;
  const int k0 = fn >= 0 ? fn : 0, k1 = fn >= 0 ? fn + 1 : Pp->K;
  const double inf = __builtin_inf();
  double* sr = score + i * m_cand;
  int bad = 0;
  for (int64_t j = l; j < m_cand; j += kWave) {
    const double* pj = part + (i * m_cand + j) * nb_pitch;
    double total = 0.0;
    for (int k = k0; k < k1; ++k) {
      const int64_t nb = (Pp->fn[k].n + MHX_RESID_BLOCK - 1) / MHX_RESID_BLOCK;
      double c = 0.0;
      for (int64_t b = 0; b < nb; ++b) c = c + pj[b];
      pj += nb;
      total = total + c;
    }
    const bool fin = finite_f64(total);
    bad += fin ? 0 : 1;
    sr[j] = fin ? total : inf;
  }
  bad = wave_sum_i(bad);
  if (l == 0) n_bad[i] = bad;
  // (a lane reads back below only the scores it stored above: candidates l, l + 64, ...)
  double ls = -inf;  // the candidate taken last: every (score, index) lies above (-inf, -1)
  int32_t lj = -1;
  for (int r = 0; r < keep; ++r) {
    double bs = inf;
    int32_t bj = INT32_MAX;
    for (int64_t j = l; j < m_cand; j += kWave) {
      const double s = sr[j];
      const bool above = s > ls || (s == ls && (int32_t)j > lj);
      const bool less = s < bs || (s == bs && (int32_t)j < bj);
      if (above && less) bs = s, bj = (int32_t)j;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(bs, m, kWave);
      const int32_t oj = __shfl_xor(bj, m, kWave);
      const bool take = os < bs || (os == bs && oj < bj);
      bs = take ? os : bs;
      bj = take ? oj : bj;
    }
    if (l == 0) {
      best_index[i * keep + r] = bj == INT32_MAX ? -1 : bj;
      best_score[i * keep + r] = bs;
    }
    ls = bs, lj = bj;  // (none left: (inf, INT32_MAX), above which nothing lies)
  }
}

// select_percentile for up to kSelTogether ranks of ONE column in the same 64 passes: a pass reads
// every key once and tests it against each rank's prefix; a rank's count is the popcount of the
// wave's ballot, kept in scalar registers - no per-lane counter, no reduction.  The passes a
// column costs no longer grow with the percentiles asked for.  Each rank follows
// select_percentile's own decisions bit by bit, so the results are its bits.  pos, between, out
// [nq], nq <= kSelTogether; all lanes hold the same out.
constexpr int kSelTogether = 4;
template <class KeyAt>
__device__ __forceinline__ void select_percentiles_together(KeyAt key_at, int n, int nq, const int* pos,
                                                            const bool* between, double* out) {
  const int l = lane_id();
  unsigned long long prefix[kSelTogether], mask = 0;
  int k[kSelTogether], cand[kSelTogether];
#pragma unroll
  for (int q = 0; q < kSelTogether; ++q) prefix[q] = 0, k[q] = q < nq ? pos[q] : 0, cand[q] = n;
  for (int b = 63; b >= 0; --b) {
    const unsigned long long bit = 1ULL << b, upto = mask | bit;
    int cnt[kSelTogether] = {0, 0, 0, 0};
    for (int s0 = 0; s0 < n; s0 += kWave) {
      const bool in = s0 + l < n;
      const unsigned long long key = in ? key_at(s0 + l) & upto : 0ULL;
#pragma unroll
      for (int q = 0; q < kSelTogether; ++q)  // (a candidate whose bit is 0: its bits down to b are the prefix)
        if (q < nq) cnt[q] += (int)__popcll(__ballot(in && key == prefix[q]));
    }
#pragma unroll
    for (int q = 0; q < kSelTogether; ++q) {
      if (k[q] < cnt[q]) {
        cand[q] = cnt[q];
      } else {
        k[q] -= cnt[q];
        cand[q] -= cnt[q];
        prefix[q] |= bit;
      }
    }
    mask |= bit;
  }
#pragma unroll
  for (int q = 0; q < kSelTogether; ++q) {
    if (q >= nq) continue;
    const double lo = key_value(prefix[q]);
    if (!between[q]) {
      out[q] = lo;
      continue;
    }
    unsigned long long up = prefix[q];
    if (k[q] + 1 >= cand[q]) {  // (the last of its run of equal keys: the smallest key above it)
      unsigned long long m = ~0ULL;
      for (int s = l; s < n; s += kWave) {
        const unsigned long long key = key_at(s);
        if (key > prefix[q] && key < m) m = key;
      }
      up = wave_min_u64(m);
    }
    out[q] = (lo + key_value(up)) / 2.0;
  }
}

// mhx_get_fit_percentiles, second half: the percentiles of the staged values, model-free.  One
// workgroup of kPctWaves wavefronts serves chain i and `cols` neighbouring points; wave w takes
// the points w, w + kPctWaves, ... of them and reruns the selection for every percentile.
//   use_lds = 1: the t values of each of the workgroup's points are laid down as keys, one column
//     of `tpad` slots a point - read once; with a step's points side by side in memory the read is
//     the transposing one of k_percentiles (tpad staggers the columns over the banks)
//   use_lds = 0 (not even one column fits, or MHX_FITPCT_NO_LDS=1): every pass reads the stage
// together = 1: a column's percentiles share their passes, kSelTogether at a time
// (select_percentiles_together); 0 (MHX_FITPCT_SELECT_SINGLY=1): select_percentile once for each.
// The workgroup of a chain's first points also completes the chain's n_used and status.
// pct [n][n_pct][m].
__global__ __launch_bounds__(kPctThreads) void k_fitpct_select(
    ChainState S, int64_t c0, int take, int64_t m, int cols, int n_groups, int64_t vs_step,
    int64_t vs_point, PctList pc, int use_lds, int together, int tpad, const double* __restrict__ vals,
    double* __restrict__ pct, int32_t* __restrict__ n_used, int32_t* __restrict__ status) {
  unsigned long long* col = reinterpret_cast<unsigned long long*>(mhx_lds_raw);
  const int w = wave_in_group(), l = lane_id();
  const int64_t i = blockIdx.x / n_groups;
  const int64_t p0 = (int64_t)(blockIdx.x - i * n_groups) * cols;
  const int nc = (int)(m - p0 < cols ? m - p0 : cols);
  const Ring ring = ring_of(S, c0 + i);
  const int t = ring_held(ring, take);
  const double* v = vals + i * ((int64_t)take * m) + p0 * vs_point;
  if (p0 == 0 && threadIdx.x == 0) {
    n_used[i] = t;
    if (t == 1) atomicOr(&status[i], (int32_t)MHX_FITPCT_ONE_STEP);
    if (t == 0) atomicOr(&status[i], (int32_t)MHX_FITPCT_EMPTY);
  }
  if (use_lds) {
    if (vs_point == 1) {
      for (int f = threadIdx.x; f < t * cols; f += kPctThreads) {
        const int s = f / cols, q = f - s * cols;
        if (q < nc) col[(size_t)q * tpad + s] = order_key(v[(int64_t)s * vs_step + q]);
      }
    } else {
      for (int q = 0; q < nc; ++q)
        for (int s = threadIdx.x; s < t; s += kPctThreads)
          col[(size_t)q * tpad + s] = order_key(v[(int64_t)s * vs_step + (int64_t)q * vs_point]);
    }
    __syncthreads();
  }
  for (int q = w; q < nc; q += kPctWaves) {
    const unsigned long long* cp = col + (size_t)q * tpad;
    const double* vp = v + (int64_t)q * vs_point;
    for (int k0 = 0; k0 < pc.n; k0 += together ? kSelTogether : 1) {
      const int nq = together ? (pc.n - k0 < kSelTogether ? pc.n - k0 : kSelTogether) : 1;
      double r[kSelTogether] = {0.0, 0.0, 0.0, 0.0};
      if (t > 0) {
        int pos[kSelTogether] = {0, 0, 0, 0};
        bool between[kSelTogether] = {false, false, false, false};
#pragma unroll
        for (int j = 0; j < kSelTogether; ++j)
          if (j < nq) {
            int64_t at;
            int32_t half;
            percentile_rank_of(t, pc.num[k0 + j], pc.den[k0 + j], &at, &half);
            pos[j] = (int)at, between[j] = half != 0;
          }
        if (!together) {
          r[0] = use_lds ? select_percentile([&](int s) { return cp[s]; }, t, pos[0], between[0])
                         : select_percentile([&](int s) { return order_key(vp[(int64_t)s * vs_step]); }, t,
                                             pos[0], between[0]);
        } else if (use_lds) {
          select_percentiles_together([&](int s) { return cp[s]; }, t, nq, pos, between, r);
        } else {
          select_percentiles_together([&](int s) { return order_key(vp[(int64_t)s * vs_step]); }, t, nq, pos,
                                      between, r);
        }
      }
#pragma unroll
      for (int j = 0; j < kSelTogether; ++j)
        if (j < nq && l == 0) pct[(i * pc.n + k0 + j) * m + p0 + q] = r[j];
    }
  }
}

// The key of rank `pos` (from 0) of the n keys key_at(0 .. n-1) in ascending order, by
// select_percentile's radix selection bit by bit, and *within = its place in its run of equal keys
// (pos minus the number of keys below it).  All lanes return the same values.
template <class KeyAt>
__device__ __forceinline__ unsigned long long select_key(KeyAt key_at, int n, int pos, int* within) {
  const int l = lane_id();
  unsigned long long prefix = 0, mask = 0;
  int k = pos;
  for (int b = 63; b >= 0; --b) {
    const unsigned long long bit = 1ULL << b, upto = mask | bit;
    int c0 = 0;
    for (int s0 = 0; s0 < n; s0 += kWave) {
      const bool in = s0 + l < n;
      const unsigned long long key = in ? key_at(s0 + l) & upto : 0ULL;
      c0 += (int)__popcll(__ballot(in && key == prefix));  // (still a candidate, and its bit is 0)
    }
    if (k >= c0) {
      k -= c0;
      prefix |= bit;
    }
    mask |= bit;
  }
  *within = k;
  return prefix;
}
// exp(y) - 1 of mhx_get_loo's smoothing: the Taylor polynomial of degree 8 below 2^-5, every product
// and sum rounded on its own (this unit is compiled without contraction), else gexp(y) - 1
__device__ __forceinline__ double loo_expm1(double y) {
  if (fabs(y) < 0x1p-5) {
    double p = 1.0 / 40320.0;
    p = 1.0 / 5040.0 + y * p;
    p = 1.0 / 720.0 + y * p;
    p = 1.0 / 120.0 + y * p;
    p = 1.0 / 24.0 + y * p;
    p = 1.0 / 6.0 + y * p;
    p = 1.0 / 2.0 + y * p;
    p = 1.0 + y * p;
    return y * p;
  }
  return gexp(y) - 1.0;
}
// the sum of the first `cnt` lanes' v, serially from acc in lane order: every lane ends with the
// same bits.  cnt is wave-uniform.
__device__ __forceinline__ double lanes_serial_sum(double acc, double v, int cnt) {
  for (int j = 0; j < cnt; ++j) acc = acc + readlane_f64(v, j);
  return acc;
}

// mhx_get_loo, second half (include/mhx.h has the definition): the Pareto-smoothed estimate of the
// staged terms, model-free.  One workgroup of kPctWaves wavefronts serves chain i and kLooCols
// neighbouring points, ONE WAVE A COLUMN: everything between the column and its three numbers is
// serial in the definition's order, or as wide as a tail (M of about 3 sqrt n) or as the fit's grid
// (Mg <= 62 values of theta: one lane each), so a wave is the widest unit that has work throughout,
// and no barrier separates the phases.  For its column a wave
//   1 finds the key of rank M by radix selection (select_key), and T_1 by one min-reduction
//   2 walks the steps in ascending s: a step below the cut key, or among the first `within` of the
//     cut key's run, goes to the wave's tail buffer in LDS; every other adds gexp(T_1 - l_s) to
//     S_b, the exponentials 64 at a time and the sum in lane order (lanes_serial_sum)
//   3 sorts the tail's keys in LDS (bitonic over the next power of two, padded with the greatest key)
//   4 lays down x_k, runs the fit with theta_j in lane j - 1, each lane summing its tlog serially
//     over the tail (x_k is one LDS broadcast for all lanes), then the weights and theta^ from
//     readlane loops; k_raw's terms 64 at a time, summed in lane order
//   5 smooths (a lane per k) and takes the two final sums in lane order.
// LDS: the math tables (LdsHead, at address 0: gexp and tlog read them there), per wave its tail
// keys [p2] and x [p2], then - use_lds - the four columns' keys at `tpad` slots each, transposed on
// the way in as k_fitpct_select does.  use_lds = 0 (the columns do not fit, or MHX_LOO_NO_LDS=1):
// passes 1 and 2 read the stage.  p2: the power of two that holds the call's P.
constexpr int kLooCols = kPctWaves;
__global__ __launch_bounds__(kPctThreads) void k_loo_fit(
    ChainState S, int64_t c0, int take, int tail_len, int64_t m, int n_groups, int P, int p2, int use_lds,
    int tpad, const double* __restrict__ terms, double* __restrict__ pw_elpd, double* __restrict__ pw_khat,
    double* __restrict__ pw_acc, double* __restrict__ tail, int32_t* __restrict__ status) {
  lds_tables_begin();
  unsigned long long* const work = reinterpret_cast<unsigned long long*>(mhx_lds_raw + sizeof(LdsHead));
  unsigned long long* const col = work + (size_t)kPctWaves * 2 * p2;
  const int w = wave_in_group(), l = lane_id();
  const int64_t i = blockIdx.x / n_groups;
  const int64_t pg = (int64_t)(blockIdx.x - i * n_groups) * kLooCols;
  const int nc = (int)(m - pg < kLooCols ? m - pg : kLooCols);
  const Ring ring = ring_of(S, c0 + i);
  const int n = ring_held(ring, take);
  const double* v = terms + i * ((int64_t)take * m) + pg;
  if (use_lds) {
    for (int f = threadIdx.x; f < n * kLooCols; f += kPctThreads) {
      const int s = f / kLooCols, q = f - s * kLooCols;
      if (q < nc) col[(size_t)q * tpad + s] = order_key(v[(int64_t)s * m + q]);
    }
  }
  __syncthreads();  // (the tables and the columns; the only barrier)
  if (w >= nc) return;
  const unsigned long long* cp = col + (size_t)w * tpad;
  const double* vp = v + w;
  auto key_at = [&](int s) -> unsigned long long {
    return use_lds ? cp[s] : order_key(vp[(int64_t)s * m]);
  };
  unsigned long long* const tk = work + (size_t)w * 2 * p2;  // the tail's keys, then T ascending
  double* const xs = reinterpret_cast<double*>(tk + p2);     // x_k, then lw_k
  const int64_t o = i * m + pg + w;
  const int M = n > 0 ? loo_tail_length_of(n, tail_len) : 0;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  double T1 = nan, lcut = nan, Sb = 0.0, sigma = 0.0, khat = inf, elpd = nan;
  bool flat = false;
  if (n > 0) {
    // 1: the cut key and the smallest key
    int within = 0;
    const unsigned long long kcut = select_key(key_at, n, M, &within);
    unsigned long long mn = ~0ULL;
    for (int s = l; s < n; s += kWave) {
      const unsigned long long k = key_at(s);
      mn = k < mn ? k : mn;
    }
    mn = wave_min_u64(mn);
    T1 = key_value(mn), lcut = key_value(kcut);
    // 2: the tail to LDS, the body into S_b in step order
    int n_eq = 0, n_tail = 0;
    for (int s0 = 0; s0 < n; s0 += kWave) {
      const bool in = s0 + l < n;
      const unsigned long long k = in ? key_at(s0 + l) : ~0ULL;
      const bool eq = in && k == kcut;
      const unsigned long long beq = __ballot(eq), below = (1ULL << l) - 1ULL;
      const bool tl = in && (k < kcut || (eq && n_eq + (int)__popcll(beq & below) < within));
      const unsigned long long btl = __ballot(tl);
      const int at = n_tail + (int)__popcll(btl & below);
      if (tl && at < M) tk[at] = k;  // (at < M always: M steps are tail by the selection's count)
      const double ge = (in && !tl) ? gexp(T1 - key_value(k)) : 0.0;
      Sb = lanes_serial_sum(Sb, ge, n - s0 < kWave ? n - s0 : kWave);
      n_eq += (int)__popcll(beq);
      n_tail += (int)__popcll(btl);
    }
    // 3: T_1 .. T_M ascending
    for (int f = M + l; f < p2; f += kWave) tk[f] = ~0ULL;
    __builtin_amdgcn_wave_barrier();
    if (M > 1) {
      for (int kk = 2; kk <= p2; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
          for (int t = l; t < p2 / 2; t += kWave) {
            const int a = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), b = a | jj;
            const unsigned long long ka = tk[a], kb = tk[b];
            const bool asc = (a & kk) == 0;
            if ((ka > kb) == asc) tk[a] = kb, tk[b] = ka;
          }
          __builtin_amdgcn_wave_barrier();
        }
    }
    // 4: x_k = r_k - r_cut for k = 1 .. M, u_k = T_{M+1-k}; xs[k - 1]
    const double rcut = gexp(T1 - lcut);
    for (int k = l; k < M; k += kWave) {
      const double u = key_value(tk[M - 1 - k]);
      xs[k] = gexp(T1 - u) - rcut;
    }
    __builtin_amdgcn_wave_barrier();
    bool fitted = false;
    if (M > 0) {
      const double Md = (double)M;
      const int Mg = 30 + (int)__builtin_sqrt(Md);  // (sqrt is correctly rounded: the floor is exact for M <= 1024)
      const double xq = xs[(M + 2) / 4 - 1], xM = xs[M - 1];
      if (xq > 0.0 && xM > 0.0) {
        const double G = (double)Mg;
        const int j = l < Mg ? l + 1 : Mg;  // (lanes beyond the grid repeat its last value, unread)
        const double a0 = G / ((double)j - 0.5);
        const double a1 = 1.0 - __builtin_sqrt(a0);
        const double a2 = a1 / 3.0;
        const double th = 1.0 / xM + a2 / xq;
        double sum = 0.0;
        for (int k = 0; k < M; ++k) sum = sum + tlog(1.0 - th * xs[k]);
        const double kj = sum / Md;
        const double Lj = Md * ((tlog((-th) / kj) - kj) - 1.0);
        double den = 0.0;
        for (int q = 0; q < Mg; ++q) den = den + gexp(readlane_f64(Lj, q) - Lj);
        const double wj = 1.0 / den;
        const double that = uniform_f64(lanes_serial_sum(0.0, th * wj, Mg));
        double ks = 0.0;
        for (int k0 = 0; k0 < M; k0 += kWave) {
          const double t = k0 + l < M ? tlog(1.0 - that * xs[k0 + l]) : 0.0;
          ks = lanes_serial_sum(ks, t, M - k0 < kWave ? M - k0 : kWave);
        }
        const double kraw = uniform_f64(ks) / Md;
        const double sg = (-kraw) / that;
        const double kh = (Md * kraw + 5.0) / (double)(M + 10);
        if (finite_f64(that) && finite_f64(kraw) && finite_f64(sg) && finite_f64(kh) && sg > 0.0) {
          fitted = true;
          sigma = sg, khat = kh;
        }
      }
      flat = !fitted;
    }
    // 5: lw_k over xs, then the two sums in ascending k
    __builtin_amdgcn_wave_barrier();
    double W = 0.0, V = 0.0;
    for (int k0 = 0; k0 < M; k0 += kWave) {
      const int k = k0 + l;
      double e1 = 0.0, e2 = 0.0;
      if (k < M) {
        const double u = key_value(tk[M - 1 - k]);
        double lw = T1 - u;
        if (fitted) {
          const double p = ((double)(k + 1) - 0.5) / (double)M;
          const double t = tlog(1.0 - p);
          const double q = khat == 0.0 ? (-sigma) * t : (sigma * loo_expm1((-khat) * t)) / khat;
          const double lq = tlog(q + rcut);
          lw = lq < 0.0 ? lq : 0.0;
        }
        e1 = gexp(lw + (u - T1));
        e2 = gexp(lw);
      }
      const int cnt = M - k0 < kWave ? M - k0 : kWave;
      W = lanes_serial_sum(W, e1, cnt);
      V = lanes_serial_sum(V, e2, cnt);
    }
    const double A = (double)(n - M) + W, D = Sb + V;
    elpd = T1 + tlog(A / D);
  }
  if (l == 0) {
    pw_elpd[o] = elpd;
    pw_khat[o] = khat;
    if (pw_acc) {
      pw_acc[o * 4 + 0] = T1;
      pw_acc[o * 4 + 1] = lcut;
      pw_acc[o * 4 + 2] = Sb;
      pw_acc[o * 4 + 3] = sigma;
    }
    if (flat) atomicOr(&status[i], (int32_t)MHX_LOO_FLAT);
  }
  if (tail)
    for (int k = l; k < P; k += kWave) tail[o * P + k] = k < M ? key_value(tk[k]) : nan;
}

// mhx_get_loo: the block sums of a chunk of points, by mhx_get_waic's rule.  Wave g serves chain
// g / n_blocks of the launch and block g % n_blocks of the chunk, which is block blk0 + that of the
// function's nb_total: lane j adds its kLooPts points serially from 0.0 (a point beyond m adds 0.0),
// then the butterfly.  part_* [n][nb_total].
__global__ __launch_bounds__(kPctThreads) void k_loo_block_sums(
    int64_t n, int64_t m, int n_blocks, int64_t blk0, int64_t nb_total, double k_limit,
    const double* __restrict__ pw_elpd, const double* __restrict__ pw_lppd, const double* __restrict__ pw_khat,
    double* __restrict__ part_elpd, double* __restrict__ part_lppd, int32_t* __restrict__ part_high) {
  const int w = wave_in_group(), l = lane_id();
  const int64_t g = (int64_t)blockIdx.x * kPctWaves + w;
  if (g >= n * n_blocks) return;
  const int64_t i = g / n_blocks, blk = g - i * n_blocks;
  const int64_t p0 = blk * (int64_t)MHX_LOO_BLOCK + l;
  double se = 0.0, sl = 0.0;
  int nh = 0;
#pragma unroll
  for (int j = 0; j < kLooPts; ++j) {
    const int64_t p = p0 + (int64_t)j * kWave;
    const bool in = p < m;
    const int64_t q = i * m + (in ? p : 0);
    const double e = pw_elpd[q], lp = pw_lppd[q], kh = pw_khat[q];
    se = se + (in ? e : 0.0);
    sl = sl + (in ? lp : 0.0);
    nh += (in && kh > k_limit) ? 1 : 0;
  }
  se = wave_sum(se);
  sl = wave_sum(sl);
  nh = wave_sum_i(nh);
  if (l == 0) {
    const int64_t o = i * nb_total + blk0 + blk;
    part_elpd[o] = se;
    part_lppd[o] = sl;
    part_high[o] = nh;
  }
}

// mhx_get_loo, the totals: one thread per chain adds the blocks' partial sums in block order
// (whatever launches wrote them), takes the one subtraction and completes n_used and the status
// (a window without a tail; an empty one).
__global__ __launch_bounds__(kThreads) void k_loo_totals(ChainState S, int64_t c0, int64_t n, int take,
                                                         int64_t nb_total,
                                                         const double* __restrict__ part_elpd,
                                                         const double* __restrict__ part_lppd,
                                                         const int32_t* __restrict__ part_high,
                                                         double* __restrict__ elpd,
                                                         double* __restrict__ p_loo,
                                                         double* __restrict__ lppd,
                                                         int32_t* __restrict__ n_high,
                                                         int32_t* __restrict__ n_used,
                                                         int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t c = c0 + i;
  int64_t t = S.length[c] < S.n_hist[c] ? S.length[c] : S.n_hist[c];
  if (t > (int64_t)take) t = take;
  if (t < 0) t = 0;
  double se = 0.0, sl = 0.0;
  int nh = 0;
  for (int64_t b = 0; b < nb_total; ++b) {
    se = se + part_elpd[i * nb_total + b];
    sl = sl + part_lppd[i * nb_total + b];
    nh += part_high[i * nb_total + b];
  }
  elpd[i] = se;
  lppd[i] = sl;
  p_loo[i] = sl - se;
  n_high[i] = nh;
  n_used[i] = (int32_t)t;
  if (t < 25) status[i] = status[i] | MHX_LOO_SHORT;
  if (t == 0) status[i] = status[i] | MHX_LOO_EMPTY;
}

}  // inline namespace MHX_FAMILY
}  // namespace mhx
