// insite_score.hip — scoring the bootstrap ensemble against observed outcomes on MI355X (gfx950):
// include/insite_score.h, DESIGN.md §9p.
//
// Kernels:
//   score_sums_kernel     block = one wave = one contiguous chunk of rows, taken one after the other.  Lane l holds
//                         V = R_pad / 64 replicates (replicate s 64 + l in slot s), as effect_bands_kernel.  Prologue
//                         per row: insite_affine.h's ensemble_maps.  Per step one FMA per replicate; then, for an
//                         observed cell, insite_wavestats.h's ef_sorted_moments (one bitonic sort in registers, two
//                         fixed-order wave reductions), the rank counts by ballot + popcount, and the 2 L band ends by
//                         ef_rank_value + quantile_interp.  Lane j < S then holds statistic j of the cell and adds it
//                         to element [group][step][j] of the wave's private slab in the workspace: one coalesced
//                         read-add-write per cell, no atomics, the order is the row order.  The wave zeroes its slab
//                         first (a lane only ever reads what it wrote itself).
//   score_reduce_kernel   thread = one (group, step, statistic): the chunks' slabs in chunk order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "insite_affine.h"
#include "insite_score.h"
#include "insite_wavestats.h"

namespace {

// ---------------------------------------------------------------------------------------------
// launch plan
// ---------------------------------------------------------------------------------------------
// chunks a launch aims at.  More is not better: the reduction walks the chunks one after the other, and 16384 chunks
// took 15.9 ms where 4096 take 12.8 ms (100k rows, R = 256: measured)
constexpr int kScWaves = 4096;
constexpr size_t kScMaxWs = ((size_t)1 << 30) - 4096;  // the workspace bound of the ABI
constexpr int kScWin = 64;                // steps whose arm, observation and mask one load brings in (one per lane)
constexpr int kScRedBlock = 256;
constexpr int kScFixed = 6;               // the rows of sums before the histogram

struct ScPlan {
  int64_t n_chunks, rpc;  // chunks of rows and rows per chunk
  int64_t slab;           // doubles of one chunk's slab: G T 64
  size_t bytes;           // 0: the shape does not fit the workspace bound
};

inline ScPlan sc_plan(int64_t N, int T, int G) {
  ScPlan p;
  std::memset(&p, 0, sizeof(p));
  const double slab_d = (double)G * (double)T * kWave * 8.0;
  if (N < 1 || slab_d > (double)kScMaxWs) return p;
  p.slab = (int64_t)G * T * kWave;
  int64_t chunks = kScWaves;
  const int64_t fit = (int64_t)kScMaxWs / (p.slab * 8);
  if (chunks > fit) chunks = fit;
  if (chunks > N) chunks = N;
  p.rpc = (N + chunks - 1) / chunks;
  p.n_chunks = (N + p.rpc - 1) / p.rpc;
  p.bytes = (size_t)(p.n_chunks * p.slab * 8);
  return p;
}

// ---------------------------------------------------------------------------------------------
// score_sums_kernel
// ---------------------------------------------------------------------------------------------
// one level: the ranks of its two band ends and the penalty factor, from the host
struct ScLevel {
  QuantileRank lo, hi;
  double c, pad;
};

struct ScArgs {
  const double* y0;
  const double* u;
  const int8_t* arm;
  const double* coef;
  const double* y_obs;
  const int8_t* active;   // nullptr: every cell active
  const int32_t* group;   // nullptr: every row in group 0
  double* slabs;
  int64_t lda, ldy, ldm, N, rpc;
  int32_t T, A, substeps, method, R, G, L, B;
  double dt, drop;
  ScLevel lv[INSITE_SCORE_MAX_LEVELS];
};

template <int V, int NARM>
__global__ void __launch_bounds__(kWave) score_sums_kernel(ScArgs sa, AffineLib lib) {
  const int lane = threadIdx.x;
  const int n = sa.R - 1;
  const double h = sa.dt / (double)sa.substeps;
  const int64_t p_lo = (int64_t)blockIdx.x * sa.rpc;
  const int64_t p_hi = p_lo + sa.rpc < sa.N ? p_lo + sa.rpc : sa.N;
  const int64_t n_slab = (int64_t)sa.G * sa.T * kWave;
  double* slab = sa.slabs + (int64_t)blockIdx.x * n_slab;
  for (int64_t e = lane; e < n_slab; e += kWave) slab[e] = 0.0;

  bool valid[V];  // the slot holds a resampled replicate (1..R-1); replicate 0 is lane 0, slot 0
  bool held[V];   // the slot holds a replicate at all
#pragma unroll
  for (int s = 0; s < V; ++s) {
    held[s] = s * kWave + lane < sa.R;
    valid[s] = held[s] && s * kWave + lane >= 1;
  }
  const int lv_base = kScFixed + sa.B;

  for (int64_t p = p_lo; p < p_hi; ++p) {
    // the row's group: the range test comes before any index is formed from the id
    const int g = sa.group ? __builtin_amdgcn_readfirstlane(sa.group[p]) : 0;
    if (g < 0 || g >= sa.G) continue;
    double* grow = slab + (int64_t)g * sa.T * kWave + lane;

    // ---- prologue: the interval maps of the lane's replicates (insite_affine.h) ------------------------------
    double PA[V][NARM], PB[V][NARM];
    ensemble_maps<V, NARM>(lib, sa.coef, sa.u + p * lib.U, sa.R, sa.A, sa.drop, sa.method, sa.substeps, h, lane, PA,
                           PB);
    const double y0 = sa.y0[p];
    double v[V];
#pragma unroll
    for (int s = 0; s < V; ++s) v[s] = y0;

    for (int k0 = 0; k0 < sa.T; k0 += kScWin) {
      const int nk = sa.T - k0 < kScWin ? sa.T - k0 : kScWin;
      // the window's arms, observations and mask: lane i < nk reads step k0 + i (nothing past column T - 1)
      int wa = 0, wm = 0;
      double wy = 0.0;
      if (lane < nk) {
        wa = sa.arm[p * sa.lda + k0 + lane];
        wy = sa.y_obs[p * sa.ldy + k0 + lane];
        wm = sa.active ? sa.active[p * sa.ldm + k0 + lane] : 1;
      }
      const uint64_t seen = __builtin_amdgcn_ballot_w64(wm != 0 && fabs(wy) < __builtin_inf());  // observed cells
      for (int kk = 0; kk < nk; ++kk) {
        const int aa = __builtin_amdgcn_readlane(wa, kk);
#pragma unroll
        for (int s = 0; s < V; ++s) {
          double A = PA[s][0], B = PB[s][0];
#pragma unroll
          for (int a = 1; a < NARM; ++a) {
            A = aa == a ? PA[s][a] : A;
            B = aa == a ? PB[s][a] : B;
          }
          v[s] = fma(A, v[s], B);
        }
        if (((seen >> kk) & 1) == 0) continue;  // (uniform) an unobserved cell reaches nothing
        double* cell = grow + (int64_t)(k0 + kk) * kWave;
        const double cur = *cell;
        bool nonfinite = false;
#pragma unroll
        for (int s = 0; s < V; ++s) nonfinite = nonfinite || (held[s] && !(fabs(v[s]) < __builtin_inf()));
        if (__builtin_amdgcn_ballot_w64(nonfinite) != 0) {  // (uniform) a bad cell: its own count and nothing else
          *cell = cur + (lane == 1 ? 1.0 : 0.0);
          continue;
        }
        const double y = readlane_f64(wy, kk);
        const double point = readlane_f64(v[0], 0);
        double key[1][V], mean, m2, abs_dev, gini;
        ef_sorted_moments<V>(v, valid, lane, n, y, key, mean, m2, abs_dev, gini);
        const double e0 = point - y, em = mean - y;
        const double var = n > 1 ? m2 / (double)(n - 1) : 0.0;
        const double crps = abs_dev / (double)n - gini / ((double)n * (double)n);
        int c_lt = 0, c_eq = 0;
#pragma unroll
        for (int s = 0; s < V; ++s) {
          c_lt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid[s] && v[s] < y));
          c_eq += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid[s] && v[s] == y));
        }
        int bin = ((2 * c_lt + c_eq) * sa.B) / (2 * n);
        bin = bin < sa.B - 1 ? bin : sa.B - 1;
        // lane j: statistic j of the cell
        double mine = lane == 0 ? 1.0 : 0.0;
        mine = lane == 2 ? e0 * e0 : mine;
        mine = lane == 3 ? em * em : mine;
        mine = lane == 4 ? var : mine;
        mine = lane == 5 ? crps : mine;
        mine = lane == kScFixed + bin ? 1.0 : mine;
        for (int j = 0; j < sa.L; ++j) {
          const int il = (int)sa.lv[j].lo.i, ih = (int)sa.lv[j].hi.i;
          const double lo = quantile_interp(ef_rank_value<V>(key[0], il),
                                            ef_rank_value<V>(key[0], il + 1 < n ? il + 1 : n - 1), sa.lv[j].lo.g);
          const double hi = quantile_interp(ef_rank_value<V>(key[0], ih),
                                            ef_rank_value<V>(key[0], ih + 1 < n ? ih + 1 : n - 1), sa.lv[j].hi.g);
          const double width = hi - lo;
          const double below = lo - y > 0.0 ? lo - y : 0.0, above = y - hi > 0.0 ? y - hi : 0.0;
          const double iscore = width + sa.lv[j].c * below + sa.lv[j].c * above;
          const int l0 = lv_base + 3 * j;
          mine = lane == l0 ? ((lo <= y && y <= hi) ? 1.0 : 0.0) : mine;
          mine = lane == l0 + 1 ? width : mine;
          mine = lane == l0 + 2 ? iscore : mine;
        }
        *cell = cur + mine;
      }
    }
  }
}

// thread = (g, k, statistic j): the chunks in chunk order
__global__ void __launch_bounds__(kScRedBlock)
score_reduce_kernel(const double* __restrict__ slabs, int64_t n_chunks, int G, int T, int S, double* __restrict__ sums,
                    int64_t lds) {
  const int64_t idx = (int64_t)blockIdx.x * kScRedBlock + threadIdx.x;
  const int64_t n_slab = (int64_t)G * T * kWave;
  if (idx >= n_slab) return;
  const int j = (int)(idx % kWave);
  if (j >= S) return;
  const int64_t gk = idx / kWave;
  const int k = (int)(gk % T);
  const int g = (int)(gk / T);
  double acc = 0.0;
  for (int64_t c = 0; c < n_chunks; ++c) acc += slabs[c * n_slab + idx];
  sums[((int64_t)g * S + j) * lds + k] = acc;
}

bool sc_groups_ok(int32_t n_groups) { return n_groups >= 1 && n_groups <= INSITE_SCORE_MAX_GROUPS; }

}  // namespace

extern "C" {

int32_t insite_score_abi_version(void) { return INSITE_SCORE_ABI_VERSION; }

size_t insite_score_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms, int32_t n_replicates,
                                    int32_t n_groups) {
  // (no sub-steps and no dt here: 1 and 0 pass)
  if (!ensemble_shape_ok(n_rows, T, n_arms, 1, 0.0, n_replicates) || !sc_groups_ok(n_groups) || n_terms < 1 ||
      n_terms > INSITE_MAX_TERMS || n_replicates > INSITE_SCORE_MAX_REPLICATES || n_rows == 0)
    return 0;
  return sc_plan(n_rows, T, n_groups).bytes;
}

int32_t insite_score_sums_f64(const double* y0, const double* u, const int8_t* arm, int64_t ld_arm, const double* coef,
                              const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                              int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                              int32_t n_replicates, const double* y_obs, int64_t ld_obs, const int8_t* active,
                              int64_t ld_active, const int32_t* group, int32_t n_groups, const double* levels,
                              int32_t n_levels, int32_t n_bins, void* workspace, size_t workspace_bytes, double* sums,
                              int64_t ld_sums, void* stream) {
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) || !sc_groups_ok(n_groups) ||
      ld_arm < (int64_t)T || ld_obs < (int64_t)T || (active && ld_active < (int64_t)T) || ld_sums < (int64_t)T ||
      n_levels < 1 || n_levels > INSITE_SCORE_MAX_LEVELS || n_bins < 1 || n_bins > INSITE_SCORE_MAX_BINS || !levels)
    return INSITE_E_INVALID_ARG;
  for (int j = 0; j < n_levels; ++j)
    if (!(levels[j] > 0.0 && levels[j] < 1.0)) return INSITE_E_INVALID_ARG;  // NaN fails both comparisons
  AffineLib lib;
  const int32_t st = ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_SCORE_MAX_REPLICATES, &lib);
  if (st != INSITE_OK || n_rows == 0) return st;
  if (!y0 || !arm || !coef || !y_obs || !sums || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;
  const ScPlan plan = sc_plan(n_rows, T, n_groups);
  if (plan.bytes == 0) return INSITE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < plan.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return INSITE_E_INVALID_ARG;

  ScArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.y0 = y0;
  sa.u = n_statics > 0 ? u : y0;  // never read
  sa.arm = arm;
  sa.coef = coef;
  sa.y_obs = y_obs;
  sa.active = active;
  sa.group = group;
  sa.slabs = static_cast<double*>(workspace);
  sa.lda = ld_arm;
  sa.ldy = ld_obs;
  sa.ldm = active ? ld_active : 0;
  sa.N = n_rows;
  sa.rpc = plan.rpc;
  sa.T = T;
  sa.A = n_arms;
  sa.substeps = substeps;
  sa.method = method;
  sa.R = n_replicates;
  sa.G = n_groups;
  sa.L = n_levels;
  sa.B = n_bins;
  sa.dt = dt;
  sa.drop = drop_below;
  for (int j = 0; j < n_levels; ++j) {
    sa.lv[j].lo = quantile_rank(0.5 - 0.5 * levels[j], n_replicates - 1);
    sa.lv[j].hi = quantile_rank(0.5 + 0.5 * levels[j], n_replicates - 1);
    sa.lv[j].c = 2.0 / (1.0 - levels[j]);
  }
  const int S = kScFixed + n_bins + 3 * n_levels;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)plan.n_chunks);
  with_slots(n_replicates, n_arms,
             [&](auto v, auto narm) { score_sums_kernel<v(), narm()><<<grid, kWave, 0, hs>>>(sa, lib); });
  const int64_t n_el = plan.slab;
  score_reduce_kernel<<<(unsigned)((n_el + kScRedBlock - 1) / kScRedBlock), kScRedBlock, 0, hs>>>(
      sa.slabs, plan.n_chunks, n_groups, T, S, sums, ld_sums);
  return launch_status();
}

}  // extern "C"
