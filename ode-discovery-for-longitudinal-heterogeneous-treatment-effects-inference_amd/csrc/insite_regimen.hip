// insite_regimen.hip — regimen choice over the bootstrap ensemble on MI355X (gfx950): include/insite_regimen.h,
// DESIGN.md §9j.
//
// Kernel:
//   regimen_choice_kernel  wave = row.  Lane l holds V = R_pad / 64 replicates (replicate s 64 + l in slot s), as
//                          effect_bands_kernel.  Prologue per row, once for all K plans: the affine fold and the
//                          interval map (A_a, B_a) of every replicate and arm.  Phase 1, per plan: y = y0, J = cost[j];
//                          the plan's arm bytes and the row's weights come in 16-step chunks (one load per lane, read
//                          back by v_readlane: both are wave-uniform), the step's arm is a scalar branch, and a step is
//                          two FMAs per replicate (y <- A y + B, J <- w y + J); the running strict minimum of s J and
//                          its index stay in registers, and J goes to a lane-private LDS column [K - 1][R_pad] (a lane
//                          reads only what it wrote: no barrier; the last plan's J stays in registers).  Then the
//                          votes: ballot + popcount per plan over the valid slots.  Phase 2, per plan, last plan first:
//                          J back from its column, the regret against the replicate's minimum, and the statistics of
//                          both series by insite_wavestats.h's network (sorted together at V <= 4); the plan's
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
constexpr int kRgMaxBlocks = 1 << 20;                        // blocks of one launch; past it a block walks a run of rows
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

// The statistics of NB series (insite_effect.h: point, shifted mean, two-pass standard deviation, quantiles, the NaN
// rule) into st[b (3 + Q) + stat], written by lane 0.  The arithmetic and its order are effect_bands_kernel's.
template <int NB, int V>
__device__ __forceinline__ void rg_stats(const double (&v)[NB][V], const bool (&valid)[V], int lane, int n,
                                         const RgArgs& ra, double* st) {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int NS = 3 + ra.Q;
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
    double* sb = st + b * NS;
    const double point = readlane_f64(v[b][0], 0);
    if (lane == 0) {
      sb[0] = point;
      sb[1] = any_nan[b] ? nan : mean[b];
      sb[2] = any_nan[b] ? nan : sd[b];
    }
    for (int j = 0; j < ra.Q; ++j) {
      const int i = (int)ra.qr[j].i;
      const double g = ra.qr[j].g;
      double qv = ef_quantile<V>(key[b], i, g, n);
      qv = any_nan[b] ? nan : qv;
      if (lane == 0) sb[3 + j] = qv;
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
    // ---- prologue: the interval maps of the lane's replicates (effect_bands_kernel's) ------------------------
    double uu[INSITE_MAX_STATICS];
#pragma unroll
    for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? ra.u[p * lib.U + t] : 0.0;
    double PA[V][NARM], PB[V][NARM];
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int r = s * kWave + lane;
      const double* cb = ra.coef + (int64_t)(r < ra.R ? r : 0) * ra.A * lib.F;
      double al[NARM], be[NARM];
#pragma unroll
      for (int a = 0; a < NARM; ++a) al[a] = be[a] = 0.0;
#pragma unroll
      for (int j = 0; j < INSITE_MAX_TERMS; ++j) {
        if (j < lib.F) {
          const int code = lib.ucode[j];
          const double m = monomial_code(code & 0xffffff, uu);
          const bool lin = (code >> 24) != 0;
#pragma unroll
          for (int a = 0; a < NARM; ++a) {
            if (a < ra.A) {
              const double c = cb[a * lib.F + j];
              // a dropped term adds 0; a NaN coefficient is kept (insite_effect.h)
              const double v = (fabs(c) > ra.drop || c != c) ? c * m : 0.0;
              if (lin) be[a] += v;
              else al[a] += v;
            }
          }
        }
      }
#pragma unroll
      for (int a = 0; a < NARM; ++a) interval_map(ra.method, ra.substeps, h, al[a], be[a], PA[s][a], PB[s][a]);
    }
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
    int mine = 0;
    for (int j = 0; j < K; ++j) {
      int cnt = 0;
#pragma unroll
      for (int s = 0; s < V; ++s) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid[s] && besti[s] == j));
      mine = lane == j ? cnt : mine;
    }
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
        rg_stats<2, V>(v, valid, lane, n, ra, stage);
      } else {
#pragma unroll 1
        for (int sv = 0; sv < 2; ++sv) {
          double v[1][V];
#pragma unroll
          for (int s = 0; s < V; ++s) v[0][s] = sv == 0 ? J[s] : g[s];
          rg_stats<1, V>(v, valid, lane, n, ra, stage + sv * NS);
        }
      }
      // flush the plan's block: out[p, j, :, :], 2 (3 + Q) contiguous doubles
      wave_lds_sync();
      if (lane < 2 * NS) ra.out[p * ra.ldo + (int64_t)j * 2 * NS + lane] = stage[lane];
      wave_lds_sync();
    }
  }
}

template <int V>
void rg_launch_v(int na, dim3 grid, size_t lds, hipStream_t hs, const RgArgs& ra, const AffineLib& lib) {
  if (na == 1) regimen_choice_kernel<V, 1><<<grid, kWave, lds, hs>>>(ra, lib);
  else if (na == 2) regimen_choice_kernel<V, 2><<<grid, kWave, lds, hs>>>(ra, lib);
  else regimen_choice_kernel<V, 4><<<grid, kWave, lds, hs>>>(ra, lib);
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
  if (n_rows < 0 || T < 1 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || substeps < 1 || !(dt >= 0.0) ||
      n_replicates < 2 || check_quantiles(q, n_quantiles, INSITE_REGIMEN_MAX_QUANTILES) != INSITE_OK ||
      n_plans < 1 || n_plans > INSITE_REGIMEN_MAX_PLANS ||
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
  if (method != INSITE_METHOD_EULER && method != INSITE_METHOD_RK4) return INSITE_E_UNSUPPORTED;
  AffineLib lib;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, &lib);
  if (st != INSITE_OK) return st;
  if (n_replicates > INSITE_REGIMEN_MAX_REPLICATES) return INSITE_E_UNSUPPORTED;
  if (n_rows == 0) return INSITE_OK;
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
  const int v = n_replicates <= 64 ? 1 : (n_replicates <= 128 ? 2 : (n_replicates <= 256 ? 4 : 8));
  ra.Rpad = v * kWave;
  // staging + K - 1 columns: at most 40 + 15 x 512 doubles = 61760 bytes, below the 64 KiB a launch may ask for
  const size_t lds = sizeof(double) * ((size_t)kRgStage + (size_t)(n_plans - 1) * (size_t)ra.Rpad);
  const int64_t blocks = n_rows < kRgMaxBlocks ? n_rows : kRgMaxBlocks;
  ra.ppb = (n_rows + blocks - 1) / blocks;
  const dim3 grid((unsigned)((n_rows + ra.ppb - 1) / ra.ppb));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const int na = n_arms <= 1 ? 1 : (n_arms <= 2 ? 2 : 4);
  if (v == 1) rg_launch_v<1>(na, grid, lds, hs, ra, lib);
  else if (v == 2) rg_launch_v<2>(na, grid, lds, hs, ra, lib);
  else if (v == 4) rg_launch_v<4>(na, grid, lds, hs, ra, lib);
  else rg_launch_v<8>(na, grid, lds, hs, ra, lib);
  return launch_status();
}

}  // extern "C"
