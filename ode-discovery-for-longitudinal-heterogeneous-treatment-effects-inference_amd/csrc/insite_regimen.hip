// insite_regimen.hip — regimen choice over the bootstrap ensemble on MI355X (gfx950): include/insite_regimen.h,
// DESIGN.md §9j.
//
// Kernel:
//   regimen_choice_kernel  wave = row.  Lane l holds V = R_pad / 64 replicates (replicate s 64 + l in slot s), as
//                          effect_bands_kernel.  Prologue per row, once for all K plans: the affine fold and the
//                          interval map (A_a, B_a) of every replicate and arm (insite_affine.h's ensemble_maps, as
//                          the effect bands; the host checks and the choice of V and NARM are shared too).  Phase 1,
//                          per plan: y = y0, J = cost[j]; the plan's arm bytes and the row's weights come in 16-step chunks (one load per lane, read
//                          back by v_readlane: both are wave-uniform), the step's arm is a scalar branch, and a step is
//                          two FMAs per replicate (y <- A y + B, J <- w y + J); the running strict minimum of s J and
//                          its index stay in registers, and J goes to a lane-private LDS column [K - 1][R_pad] (a lane
//                          reads only what it wrote: no barrier; the last plan's J stays in registers).  Then the
//                          votes: ballot + popcount per plan over the valid slots.  Phase 2, per plan, last plan first:
//                          J back from its column, the regret against the replicate's minimum, and the statistics of
//                          both series by insite_wavestats.h's ef_series_stats (sorted together at V <= 4); the plan's
//                          [2, 3 + Q] block is staged in LDS and flushed as one contiguous segment of the row's block.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_regimen.h"
#include "insite_wavestats.h"

namespace {

constexpr int kRgTc = 16;                                    // steps per chunk of arm bytes and weights
constexpr int kRgMaxStats = 3 + INSITE_REGIMEN_MAX_QUANTILES;
constexpr int kRgStage = 40;                                 // doubles of the staging block: >= 2 kRgMaxStats
static_assert(2 * kRgMaxStats <= kRgStage && kRgStage <= kWave, "one plan's block is flushed by one wave at once");

struct RgArgs {
  const double* y0;
  const double* u;
  const int8_t* plans;
  const double* w;
  const double* cost;  // nullptr: zeros
  const double* coef;
  int32_t* choice;
  double* win;
  double* out;
  int64_t ps, ldp, ldw, ldo, N, ppb;  // ppb: rows per block
  int32_t T, A, K, substeps, method, R, Q, Rpad;
  double dt, drop, sense;
  QuantileRank qr[INSITE_REGIMEN_MAX_QUANTILES];  // per quantile: i and g of the header's formula
};

// one interval under the wave-uniform arm `aa` (0..NARM-1): a scalar branch, then one FMA per replicate
template <int V, int NARM>
__device__ __forceinline__ void rg_step(int aa, const double (&PA)[V][NARM], const double (&PB)[V][NARM],
                                        double (&y)[V]) {
  if constexpr (NARM == 1) {
#pragma unroll
    for (int s = 0; s < V; ++s) y[s] = fma(PA[s][0], y[s], PB[s][0]);
  } else if constexpr (NARM == 2) {
    if (aa == 1) {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][1], y[s], PB[s][1]);
    } else {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][0], y[s], PB[s][0]);
    }
  } else {
    if (aa == 1) {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][1], y[s], PB[s][1]);
    } else if (aa == 2) {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][2], y[s], PB[s][2]);
    } else if (aa == 3) {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][3], y[s], PB[s][3]);
    } else {
#pragma unroll
      for (int s = 0; s < V; ++s) y[s] = fma(PA[s][0], y[s], PB[s][0]);
    }
  }
}

template <int V, int NARM>
__global__ void __launch_bounds__(kWave) regimen_choice_kernel(RgArgs ra, AffineLib lib) {
  extern __shared__ double rg_lds[];  // [kRgStage] staging, then the objective columns [K - 1][Rpad]
  double* stage = rg_lds;
  double* col = rg_lds + kRgStage;
  constexpr int NB = V <= 4 ? 2 : 1;
  const int lane = threadIdx.x;
  const int NS = 3 + ra.Q;
  const int n = ra.R - 1;
  const int K = ra.K;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double h = ra.dt / (double)ra.substeps;
  const int64_t p_lo = (int64_t)blockIdx.x * ra.ppb;
  const int64_t p_hi = p_lo + ra.ppb < ra.N ? p_lo + ra.ppb : ra.N;

  bool valid[V];  // the slot holds a resampled replicate (1..R-1); replicate 0 is lane 0, slot 0
#pragma unroll
  for (int s = 0; s < V; ++s) valid[s] = s * kWave + lane >= 1 && s * kWave + lane < ra.R;

  for (int64_t p = p_lo; p < p_hi; ++p) {
    // ---- prologue: the interval maps of the lane's replicates (insite_affine.h) ------------------------------
    double PA[V][NARM], PB[V][NARM];
    ensemble_maps<V, NARM>(lib, ra.coef, ra.u + p * lib.U, ra.R, ra.A, ra.drop, ra.method, ra.substeps, h, lane, PA,
                           PB);
    const double y0 = ra.y0[p];

    // ---- phase 1: the objectives of every plan, the running minimum inside each replicate -------------------
    double J[V], bestJ[V];
    int besti[V];
    bool abst[V];
#pragma unroll
    for (int s = 0; s < V; ++s) {
      bestJ[s] = 0.0;
      besti[s] = 0;
      abst[s] = false;
    }
    for (int j = 0; j < K; ++j) {
      const double cj = ra.cost ? ra.cost[j] : 0.0;
      double y[V];
#pragma unroll
      for (int s = 0; s < V; ++s) {
        y[s] = y0;
        J[s] = cj;
      }
      const int8_t* pl = ra.plans + (int64_t)j * ra.ps + p * ra.ldp;
      const double* wr = ra.w + p * ra.ldw;
      for (int k0 = 0; k0 < ra.T; k0 += kRgTc) {
        const int nk = ra.T - k0 < kRgTc ? ra.T - k0 : kRgTc;
        // the chunk: lane i < nk reads step k0 + i (nothing past column T - 1)
        int wa = 0;
        double ww = 0.0;
        if (lane < nk) {
          wa = pl[k0 + lane];
          ww = wr[k0 + lane];
        }
        for (int kk = 0; kk < nk; ++kk) {
          int aa = __builtin_amdgcn_readlane(wa, kk);
          aa = (aa >= 1 && aa < ra.A) ? aa : 0;
          const double wk = readlane_f64(ww, kk);
          rg_step<V, NARM>(aa, PA, PB, y);
#pragma unroll
          for (int s = 0; s < V; ++s) J[s] = fma(wk, y[s], J[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < V; ++s) {
        abst[s] = abst[s] || J[s] != J[s];
        const bool better = j == 0 || ra.sense * J[s] < ra.sense * bestJ[s];
        bestJ[s] = better ? J[s] : bestJ[s];
        besti[s] = better ? j : besti[s];
      }
      if (j < K - 1) {
#pragma unroll
        for (int s = 0; s < V; ++s) col[j * ra.Rpad + s * kWave + lane] = J[s];
      }
    }
#pragma unroll
    for (int s = 0; s < V; ++s) besti[s] = abst[s] ? -1 : besti[s];

    // ---- the point model's choice and the votes ----------------------------------------------------------------
    const int pick = __builtin_amdgcn_readlane(besti[0], 0);
    const int mine = ef_vote_counts<V>(valid, besti, K, lane);
    if (lane == 0) ra.choice[p] = pick;
    if (lane < K) ra.win[p * K + lane] = (double)mine / (double)n;

    // ---- phase 2: per plan (the last first: its J is still in registers) the statistics of J and of the regret ----
    for (int j = K - 1; j >= 0; --j) {
      if (j < K - 1) {
#pragma unroll
        for (int s = 0; s < V; ++s) J[s] = col[j * ra.Rpad + s * kWave + lane];
      }
      double g[V];
#pragma unroll
      for (int s = 0; s < V; ++s) g[s] = abst[s] ? nan : ra.sense * J[s] - ra.sense * bestJ[s];
      if constexpr (NB == 2) {
        double v[2][V];
#pragma unroll
        for (int s = 0; s < V; ++s) {
          v[0][s] = J[s];
          v[1][s] = g[s];
        }
        ef_series_stats<2, V>(v, valid, lane, n, ra.Q, ra.qr, stage, 1);
      } else {
#pragma unroll 1
        for (int sv = 0; sv < 2; ++sv) {
          double v[1][V];
#pragma unroll
          for (int s = 0; s < V; ++s) v[0][s] = sv == 0 ? J[s] : g[s];
          ef_series_stats<1, V>(v, valid, lane, n, ra.Q, ra.qr, stage + sv * NS, 1);
        }
      }
      // flush the plan's block: out[p, j, :, :], 2 (3 + Q) contiguous doubles
      wave_lds_sync();
      if (lane < 2 * NS) ra.out[p * ra.ldo + (int64_t)j * 2 * NS + lane] = stage[lane];
      wave_lds_sync();
    }
  }
}

// a + b c in int64, or false when it does not fit (a, b, c >= 0)
inline bool rg_mul_add(int64_t a, int64_t b, int64_t c, int64_t* out) {
  int64_t m;
  return !__builtin_mul_overflow(b, c, &m) && !__builtin_add_overflow(a, m, out);
}

}  // namespace

extern "C" {

int32_t insite_regimen_abi_version(void) { return INSITE_REGIMEN_ABI_VERSION; }

size_t insite_regimen_workspace_bytes(int64_t, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

int32_t insite_regimen_choice_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                                  int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w,
                                  const double* cost, int32_t sense, const double* coef, const int8_t* exps,
                                  int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                  double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const double* q, int32_t n_quantiles, int32_t* choice,
                                  double* win, double* out, int64_t ld_out, void* /*workspace*/,
                                  size_t /*workspace_bytes*/, void* stream) {
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) ||
      check_quantiles(q, n_quantiles, INSITE_REGIMEN_MAX_QUANTILES) != INSITE_OK || n_plans < 1 ||
      n_plans > INSITE_REGIMEN_MAX_PLANS ||
      (sense != INSITE_REGIMEN_MINIMIZE && sense != INSITE_REGIMEN_MAXIMIZE))
    return INSITE_E_INVALID_ARG;
  // the strides: their lower bounds, and the largest element offset of every array must fit int64 (the kernel's index
  // arithmetic is int64)
  const int64_t last_row = n_rows > 0 ? n_rows - 1 : 0;
  int64_t span, top;
  if (ld_plan < 0 || (ld_plan != 0 && ld_plan < (int64_t)T) || plan_stride < (int64_t)T ||
      !rg_mul_add(0, n_rows, ld_plan, &span) || plan_stride < span ||
      !rg_mul_add((int64_t)T, (int64_t)(n_plans - 1), plan_stride, &top) || !rg_mul_add(top, last_row, ld_plan, &top))
    return INSITE_E_INVALID_ARG;
  if (ld_w < 0 || (ld_w != 0 && ld_w < (int64_t)T) || !rg_mul_add((int64_t)T, last_row, ld_w, &top))
    return INSITE_E_INVALID_ARG;
  const int64_t block = (int64_t)n_plans * 2 * (3 + n_quantiles);
  if (ld_out < block || !rg_mul_add(block, last_row, ld_out, &top) || !rg_mul_add(0, n_rows, (int64_t)n_plans, &top))
    return INSITE_E_INVALID_ARG;
  AffineLib lib;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_REGIMEN_MAX_REPLICATES, &lib);
  if (st != INSITE_OK || n_rows == 0) return st;
  if (!y0 || !plans || !w || !coef || !choice || !win || !out || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;

  RgArgs ra;
  std::memset(&ra, 0, sizeof(ra));
  ra.y0 = y0;
  ra.u = n_statics > 0 ? u : y0;  // never read
  ra.plans = plans;
  ra.w = w;
  ra.cost = cost;
  ra.coef = coef;
  ra.choice = choice;
  ra.win = win;
  ra.out = out;
  ra.ps = plan_stride;
  ra.ldp = ld_plan;
  ra.ldw = ld_w;
  ra.ldo = ld_out;
  ra.N = n_rows;
  ra.T = T;
  ra.A = n_arms;
  ra.K = n_plans;
  ra.substeps = substeps;
  ra.method = method;
  ra.R = n_replicates;
  ra.Q = n_quantiles;
  ra.dt = dt;
  ra.drop = drop_below;
  ra.sense = (double)sense;
  for (int j = 0; j < n_quantiles; ++j) ra.qr[j] = quantile_rank(q[j], n_replicates - 1);
  ra.Rpad = replicate_slots(n_replicates) * kWave;
  // staging + K - 1 columns: at most 40 + 15 x 512 doubles = 61760 bytes, below the 64 KiB a launch may ask for
  const size_t lds = sizeof(double) * ((size_t)kRgStage + (size_t)(n_plans - 1) * (size_t)ra.Rpad);
  ra.ppb = rows_per_block(n_rows);
  const dim3 grid((unsigned)((n_rows + ra.ppb - 1) / ra.ppb));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  with_slots(n_replicates, n_arms, [&](auto v, auto narm) {
    regimen_choice_kernel<v(), narm()><<<grid, kWave, lds, hs>>>(ra, lib);
  });
  return launch_status();
}

}  // extern "C"
