// insite_wavestats.h — the one definition of the order statistics and moments one wave takes over the bootstrap
// replicates it holds in registers (lane l, slot s = replicate s 64 + l; V = R_pad / 64 slots per lane): the lane
// exchanges, the fixed-order wave sums, the in-register bitonic sort, the read of a sorted rank, the vote count and,
// built on them, ef_series_stats: the point value, moments, quantiles and NaN rule of include/insite_effect.h.  effect_bands_kernel
// (insite_effect.hip) and regimen_choice_kernel (insite_regimen.hip, §9j) both call ef_series_stats
// and differ only in the stride of the staging writes, so the regimen statistics are the effect bands' by
// construction.  The quantile interpolation is insite_affine.h's quantile_interp, shared with the cohort finalize.
// insite_common.h's convention: an anonymous namespace, each translation unit gets its own internal copy.
#pragma once
#include <limits>

#include "insite_affine.h"

namespace {

// ---------------------------------------------------------------------------------------------
// wave helpers
// ---------------------------------------------------------------------------------------------
// the value of the lane whose byte address is `addr` (= 4 x lane)
__device__ __forceinline__ double ef_permute(double v, int addr) {
  const u32x2 w = __builtin_bit_cast(u32x2, v);
  u32x2 r;
  r.x = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)w.x);
  r.y = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)w.y);
  return __builtin_bit_cast(double, r);
}

// the value of lane (lane ^ M).  Inside a row of 16 lanes the masks 1, 2, 3, 7, 8 and 15 are DPP moves on the VALU
// (quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0], row_half_mirror, row_ror:8, row_mirror); the others go through the LDS
// crossbar (ds_bpermute_b32, no LDS storage).  Every lane is active wherever this is called.
template <int M>
__device__ __forceinline__ double ef_xor_lane(double v, int lane) {
  constexpr int ctrl = M == 1 ? 0xB1 : M == 2 ? 0x4E : M == 3 ? 0x1B : M == 7 ? 0x141 : M == 8 ? 0x128 : M == 15 ? 0x140 : -1;
  if constexpr (ctrl >= 0) {
    const u32x2 w = __builtin_bit_cast(u32x2, v);
    u32x2 r;
    r.x = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w.x, ctrl, 0xF, 0xF, true);
    r.y = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w.y, ctrl, 0xF, 0xF, true);
    return __builtin_bit_cast(double, r);
  } else {
    return ef_permute(v, (lane ^ M) << 2);
  }
}

// sums over the wave in a fixed order (xor butterfly: every lane adds the same pairs, so every lane holds the same
// bits), NB independent sums at a time
template <int NB, int OFF>
__device__ __forceinline__ void ef_wave_sum_from(double (&v)[NB], int lane) {
  if constexpr (OFF < kWave) {
    double o[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) o[b] = ef_xor_lane<OFF>(v[b], lane);
#pragma unroll
    for (int b = 0; b < NB; ++b) v[b] += o[b];
    ef_wave_sum_from<NB, 2 * OFF>(v, lane);
  }
}
template <int NB>
__device__ __forceinline__ void ef_wave_sum(double (&v)[NB], int lane) {
  ef_wave_sum_from<NB, 1>(v, lane);
}

// Ascending bitonic sort of the 64 V keys of a wave; the key of lane l, slot s has index i = l V + s.  The merge of
// size k starts with the mirror exchange i <-> i ^ (k - 1) and goes on with i <-> i ^ j, j = k / 4 .. 1, so every
// compare-exchange puts the minimum at the lower index (no descending runs).  Exchanges inside a lane (j < V) are
// min / max pairs; an exchange between lanes fetches the partner's key and keeps one of the two.  Keys must not be
// NaN (the caller replaces NaN by +Inf).
template <int V>
constexpr int ef_log2v() { return V == 1 ? 0 : (V == 2 ? 1 : (V == 4 ? 2 : 3)); }

// one compare-exchange i <-> i ^ (1 << JB) of every key of NB independent key sets (every index a template
// constant: the keys stay in registers; the sets' exchanges are issued together, so the NB dependent chains overlap)
template <int NB, int V, int JB>
__device__ __forceinline__ void ef_exchange(double (&key)[NB][V], int lane) {
  constexpr int LV = ef_log2v<V>();
  if constexpr (JB < LV) {
    constexpr int j = 1 << JB;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) {
        if ((s & j) == 0) {
          const double lo = __builtin_fmin(key[b][s], key[b][s | j]), hi = __builtin_fmax(key[b][s], key[b][s | j]);
          key[b][s] = lo;
          key[b][s | j] = hi;
        }
      }
  } else {
    constexpr int jl = 1 << (JB - LV);
    const bool upper = (lane & jl) != 0;
    double o[NB][V];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) o[b][s] = ef_xor_lane<jl>(key[b][s], lane);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) key[b][s] = ((o[b][s] < key[b][s]) != upper) ? o[b][s] : key[b][s];
  }
}

template <int NB, int V, int JB>
__device__ __forceinline__ void ef_exchanges_down(double (&key)[NB][V], int lane) {
  if constexpr (JB >= 0) {
    ef_exchange<NB, V, JB>(key, lane);
    ef_exchanges_down<NB, V, JB - 1>(key, lane);
  }
}

// the merge of size 1 << KB: the mirror exchange, then i <-> i ^ j for j = (1 << KB) / 4 .. 1
template <int NB, int V, int KB>
__device__ __forceinline__ void ef_merge(double (&key)[NB][V], int lane) {
  constexpr int LV = ef_log2v<V>();
  if constexpr (KB <= LV) {
    constexpr int m = (1 << KB) - 1;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) {
        if (s < (s ^ m)) {
          const double lo = __builtin_fmin(key[b][s], key[b][s ^ m]), hi = __builtin_fmax(key[b][s], key[b][s ^ m]);
          key[b][s] = lo;
          key[b][s ^ m] = hi;
        }
      }
  } else {
    constexpr int lm = (1 << (KB - LV)) - 1;  // partner lane = lane ^ lm, partner slot = V - 1 - s
    const bool upper = (lane & (1 << (KB - LV - 1))) != 0;
    double o[NB][V];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) o[b][s] = ef_xor_lane<lm>(key[b][V - 1 - s], lane);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int s = 0; s < V; ++s) key[b][s] = ((o[b][s] < key[b][s]) != upper) ? o[b][s] : key[b][s];
  }
  ef_exchanges_down<NB, V, KB - 2>(key, lane);
}

template <int NB, int V, int KB>
__device__ __forceinline__ void ef_merges_up(double (&key)[NB][V], int lane) {
  if constexpr (KB <= ef_log2v<V>() + 6) {
    ef_merge<NB, V, KB>(key, lane);
    ef_merges_up<NB, V, KB + 1>(key, lane);
  }
}

template <int NB, int V>
__device__ __forceinline__ void ef_sort(double (&key)[NB][V], int lane) {
  ef_merges_up<NB, V, 1>(key, lane);
}

// the sorted key of index i (wave-uniform), in every lane
template <int V>
__device__ __forceinline__ double ef_rank_value(const double (&key)[V], int i) {
  constexpr int LV = ef_log2v<V>();
  // the slot by a select tree over the bits of i (a chain of slot == s selects, and with V = 2 the one select
  // between the two keys, is turned into an indexed scratch array: V = 2 selects between the two lane values instead)
  if constexpr (V == 2) {
    const double x0 = readlane_f64(key[0], i >> 1), x1 = readlane_f64(key[1], i >> 1);
    return (i & 1) ? x1 : x0;
  }
  double x[V];
#pragma unroll
  for (int s = 0; s < V; ++s) x[s] = key[s];
#pragma unroll
  for (int b = 0; b < LV; ++b) {
    const bool odd = ((i >> b) & 1) != 0;
#pragma unroll
    for (int s = 0; s < (V >> (b + 1)); ++s) x[s] = odd ? x[2 * s + 1] : x[2 * s];
  }
  return readlane_f64(x[0], i >> LV);
}

// The votes of the valid slots (regimen_choice_kernel, feedback_rules_kernel): lane j < K returns the number of valid
// slots of the wave whose best[s] is j (an exact count: ballot + popcount per candidate), the other lanes 0.
template <int V>
__device__ __forceinline__ int ef_vote_counts(const bool (&valid)[V], const int (&best)[V], int K, int lane) {
  int mine = 0;
  for (int j = 0; j < K; ++j) {
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < V; ++s) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid[s] && best[s] == j));
    mine = lane == j ? cnt : mine;
  }
  return mine;
}

// The statistics of NB series over the replicates 1..R-1 = the valid slots (insite_effect.h: the point model's value,
// the mean shifted by replicate 1's value, the two-pass standard deviation with ddof 1, the Q quantiles of ranks qr
// over the n = R - 1 keys, and the NaN rule: one NaN among the valid values makes everything but the point NaN).
// Lane 0 writes statistic t of series b to stage[(b (3 + Q) + t) stride]; the NB sorts and reductions are independent
// chains issued together.
template <int NB, int V>
__device__ __forceinline__ void ef_series_stats(const double (&v)[NB][V], const bool (&valid)[V], int lane, int n,
                                                int Q, const QuantileRank* qr, double* stage, int stride) {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double key[NB][V];
  bool any_nan[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    bool bad = false;
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const bool isn = v[b][s] != v[b][s];
      bad = bad || (valid[s] && isn);
      key[b][s] = (valid[s] && !isn) ? v[b][s] : inf;
    }
    any_nan[b] = __builtin_amdgcn_ballot_w64(bad) != 0;
  }
  // mean, shifted by c = v[1] (lane 1, slot 0), and the two-pass standard deviation; fixed order: the lane's slots
  // ascending, then the wave butterfly
  double acc[NB], c[NB], mean[NB], sd[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    c[b] = readlane_f64(v[b][0], 1);
    c[b] = fabs(c[b]) < inf ? c[b] : 0.0;
    acc[b] = 0.0;
#pragma unroll
    for (int s = 0; s < V; ++s) acc[b] += valid[s] ? v[b][s] - c[b] : 0.0;
  }
  ef_wave_sum<NB>(acc, lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    mean[b] = c[b] + acc[b] / (double)n;
    acc[b] = 0.0;
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const double d = v[b][s] - mean[b];
      acc[b] += valid[s] ? d * d : 0.0;
    }
  }
  ef_wave_sum<NB>(acc, lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) sd[b] = sqrt(acc[b] / (double)(n - 1));
  ef_sort<NB, V>(key, lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    double* st = stage + b * (3 + Q) * stride;
    const double point = readlane_f64(v[b][0], 0);
    if (lane == 0) {
      st[0] = point;
      st[stride] = any_nan[b] ? nan : mean[b];
      st[2 * stride] = any_nan[b] ? nan : sd[b];
    }
    for (int j = 0; j < Q; ++j) {
      const int i = (int)qr[j].i;
      const double lo = ef_rank_value<V>(key[b], i);
      const double hi = ef_rank_value<V>(key[b], i + 1 < n ? i + 1 : n - 1);
      double qv = quantile_interp(lo, hi, qr[j].g);
      qv = any_nan[b] ? nan : qv;
      if (lane == 0) st[(3 + j) * stride] = qv;
    }
  }
}

// The sort and the moments of one series whose valid values are all finite, about a reference y (score_sums_kernel,
// insite_score.hip): key = the ascending sort of the n valid values (the padding +Inf behind them), mean = the shifted
// mean of ef_series_stats, and in every lane the wave totals m2 = sum (v - mean)^2, abs_dev = sum |v - y| and
// gini = sum_i (2 i - n + 1) (key_i - mean) over the sorted index i = lane V + slot < n.  Two wave reductions of two
// sums each, in ef_series_stats' fixed order: the lane's slots ascending, then the butterfly.
template <int V>
__device__ __forceinline__ void ef_sorted_moments(const double (&v)[V], const bool (&valid)[V], int lane, int n,
                                                  double y, double (&key)[1][V], double& mean, double& m2,
                                                  double& abs_dev, double& gini) {
  const double inf = std::numeric_limits<double>::infinity();
  const double c = readlane_f64(v[0], 1);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int s = 0; s < V; ++s) {
    key[0][s] = valid[s] ? v[s] : inf;
    acc[0] += valid[s] ? v[s] - c : 0.0;
    acc[1] += valid[s] ? fabs(v[s] - y) : 0.0;
  }
  ef_wave_sum<2>(acc, lane);
  mean = c + acc[0] / (double)n;
  abs_dev = acc[1];
  ef_sort<1, V>(key, lane);
  acc[0] = acc[1] = 0.0;
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const double d = v[s] - mean;
    acc[0] += valid[s] ? d * d : 0.0;
    const int i = lane * V + s;
    acc[1] += i < n ? (double)(2 * i - n + 1) * (key[0][s] - mean) : 0.0;
  }
  ef_wave_sum<2>(acc, lane);
  m2 = acc[0];
  gini = acc[1];
}

}  // namespace
