// insite_blockstats.h — the one definition of what the two cohort-level consumers of the bootstrap ensemble share
// (insite_cohort.hip; insite_policy.hip, §9k): the arms of a 64-step window as ballot masks (lane =
// replicate kernels: the step's arm is a scalar bit test) and the statistics one block takes over the R values of a
// series held in LDS (thread = replicate): the point value, the mean shifted by replicate 1's value, the two-pass
// deviation by a fixed tree, the padding to +Inf, the bitonic sort and the quantile pick of include/insite_effect.h.
// cohort_finalize_kernel and policy_finalize_kernel both call co_block_series_stats, so the policy statistics are the
// cohort statistics by construction.  The quantile interpolation is insite_affine.h's quantile_interp.
// insite_common.h's convention: an anonymous namespace, each translation unit gets its own internal copy.
#pragma once
#include <limits>

#include "insite_affine.h"

namespace {

// ---------------------------------------------------------------------------------------------
// arms as ballot masks
// ---------------------------------------------------------------------------------------------
// the arms of one 64-step window as bit masks: bit k of m[a - 1] = (the arm of step k is a); no bit: arm 0
template <int NARM>
struct CoArmMask {
  uint64_t m[NARM > 1 ? NARM - 1 : 1];
};

template <int NARM>
__device__ __forceinline__ CoArmMask<NARM> co_arm_mask(int v, int n_arms) {
  CoArmMask<NARM> r;
  r.m[0] = 0;
#pragma unroll
  for (int a = 1; a < NARM; ++a) r.m[a - 1] = __builtin_amdgcn_ballot_w64(v == a && a < n_arms);
  return r;
}

// ---------------------------------------------------------------------------------------------
// block statistics
// ---------------------------------------------------------------------------------------------
// the sum of the threads' values in a fixed order (a tree over red[BLOCK]); every thread gets it
template <int BLOCK>
__device__ __forceinline__ double co_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int o = BLOCK / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}

// The statistics of one series over the replicates.  key[0..rpad): key[r] = v[r] for r < R, +Inf past it (rpad: the
// power of two >= max(R, 2)), written by the block's threads in the stride of the block; bad: this thread saw a NaN
// among v[1..R-1].  Every thread of the block calls.  store(i, x) writes statistic i: thread 0 stores the point, the
// mean and the deviation (0..2), thread t < Q quantile t (3 + t).  key is sorted on return.
template <int BLOCK, class Store>
__device__ __forceinline__ void co_block_series_stats(double* key, double* red, int R, int rpad, int Q,
                                                      const QuantileRank* qr, int bad, Store store) {
  const int t = threadIdx.x;
  const int n = R - 1;
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const bool any_nan = __syncthreads_or(bad) != 0;
  const double point = key[0];
  double c = key[1];
  c = fabs(c) < inf ? c : 0.0;
  // mean, shifted by c, and the two-pass deviation; fixed order: the thread's replicates ascending, then the tree
  double a = 0.0;
  for (int r = t; r < R; r += BLOCK) a += r >= 1 ? key[r] - c : 0.0;
  const double mean = c + co_block_sum<BLOCK>(a, red) / (double)n;
  a = 0.0;
  for (int r = t; r < R; r += BLOCK) {
    const double d = key[r] - mean;
    a += r >= 1 ? d * d : 0.0;
  }
  const double sd = sqrt(co_block_sum<BLOCK>(a, red) / (double)(n - 1));
  __syncthreads();
  // the keys: the point model and NaN go to +Inf (with a NaN every quantile is NaN anyway)
  for (int r = t; r < R; r += BLOCK) {
    const double v = key[r];
    key[r] = (r >= 1 && v == v) ? v : inf;
  }
  __syncthreads();
  for (int kk = 2; kk <= rpad; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = t; i < rpad; i += BLOCK) {
        const int l = i ^ j;
        if (l > i) {
          const double x = key[i], y = key[l];
          const bool up = (i & kk) == 0;
          if ((x > y) == up) {
            key[i] = y;
            key[l] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  if (t == 0) {
    store(0, point);
    store(1, any_nan ? nan : mean);
    store(2, any_nan ? nan : sd);
  }
  if (t < Q) {
    const int i = (int)qr[t].i;
    const double qv = quantile_interp(key[i], key[i + 1 < n ? i + 1 : n - 1], qr[t].g);
    store(3 + t, any_nan ? nan : qv);
  }
}

}  // namespace
