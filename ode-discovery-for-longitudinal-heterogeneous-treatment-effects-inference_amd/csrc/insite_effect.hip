// insite_effect.hip — paired treatment-effect bands over the bootstrap ensemble on MI355X (gfx950):
// include/insite_effect.h, DESIGN.md §9h.
//
// Kernel:
//   effect_bands_kernel   wave = patient.  Lane l holds V = R_pad / 64 replicates (replicate s 64 + l in slot s;
//                         R_pad = the power of two >= max(64, R)).  Prologue per patient: the affine fold (alpha, beta)
//                         and the interval map (A_a, B_a) of every replicate and arm, as rollout_tm_kernel.  Per step
//                         one FMA per replicate and plan (the step's arm is wave-uniform: scalar selects), then per
//                         series a bitonic network over the R_pad keys in registers -- the stages inside a lane are
//                         v_min_f64 / v_max_f64, the lane stages DPP moves inside a row of 16 lanes and ds_bpermute
//                         beyond (no LDS storage, no barrier) -- the order statistics by v_readlane, and mean / std
//                         by fixed-order wave reductions; a step's three series are sorted together at V <= 4.  The
//                         [n_series, 3 + Q] results of 16 steps are staged in LDS and flushed as row segments.
//                         The lane exchanges, sums, sort network and rank reads are insite_wavestats.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_effect.h"
#include "insite_wavestats.h"

namespace {

// ---------------------------------------------------------------------------------------------
// effect_bands_kernel
// ---------------------------------------------------------------------------------------------
constexpr int kEfTc = 16;                                   // steps staged in LDS between two flushes
constexpr int kEfMaxStats = 3 + INSITE_EFFECT_MAX_QUANTILES;
constexpr int kEfMaxBlocks = 1 << 20;                       // blocks of one launch; past it a block walks a run of patients

struct EfArgs {
  const double* y0;
  const double* u;
  const int8_t* arm_a;
  const int8_t* arm_b;  // nullptr: series A only
  const double* coef;
  double* out;
  int64_t lda, ldb, ldo, N, ppb;  // ppb: patients per block
  int32_t T, A, substeps, method, R, Q;
  double dt, drop;
  QuantileRank qr[INSITE_EFFECT_MAX_QUANTILES];  // per quantile: i and g of the header's formula
};

// NSER: 1 (plan A only) or 3 series.  The three series of a step are sorted together where the registers allow it
// (V <= 4: three independent chains of dependent exchanges in flight); V = 8 sorts them one after the other.
template <int V, int NARM, int NSER>
__global__ void __launch_bounds__(kWave) effect_bands_kernel(EfArgs ea, AffineLib lib) {
  __shared__ double stage[NSER * kEfMaxStats * kEfTc];
  constexpr int NB = V <= 4 ? NSER : 1;
  constexpr int nser = NSER;
  const int lane = threadIdx.x;
  const int NS = 3 + ea.Q;
  const int n = ea.R - 1;
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double h = ea.dt / (double)ea.substeps;
  const int64_t p_lo = (int64_t)blockIdx.x * ea.ppb;
  const int64_t p_hi = p_lo + ea.ppb < ea.N ? p_lo + ea.ppb : ea.N;

  bool valid[V];  // the slot holds a resampled replicate (1..R-1); replicate 0 is lane 0, slot 0
#pragma unroll
  for (int s = 0; s < V; ++s) valid[s] = s * kWave + lane >= 1 && s * kWave + lane < ea.R;

  for (int64_t p = p_lo; p < p_hi; ++p) {
    // ---- prologue: the interval maps of the lane's replicates -------------------------------------------
    double uu[INSITE_MAX_STATICS];
#pragma unroll
    for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? ea.u[p * lib.U + t] : 0.0;
    double PA[V][NARM], PB[V][NARM];
#pragma unroll
    for (int s = 0; s < V; ++s) {
      const int r = s * kWave + lane;
      const double* cb = ea.coef + (int64_t)(r < ea.R ? r : 0) * ea.A * lib.F;
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
            if (a < ea.A) {
              const double c = cb[a * lib.F + j];
              // a dropped term adds 0; a NaN coefficient is kept (insite_effect.h)
              const double v = (fabs(c) > ea.drop || c != c) ? c * m : 0.0;
              if (lin) be[a] += v;
              else al[a] += v;
            }
          }
        }
      }
#pragma unroll
      for (int a = 0; a < NARM; ++a) interval_map(ea.method, ea.substeps, h, al[a], be[a], PA[s][a], PB[s][a]);
    }
    const double y0 = ea.y0[p];
    double yA[V], yB[V];
#pragma unroll
    for (int s = 0; s < V; ++s) yA[s] = yB[s] = y0;

    // ---- time loop -----------------------------------------------------------------------------------------
    for (int k0 = 0; k0 < ea.T; k0 += kEfTc) {
      const int nk = ea.T - k0 < kEfTc ? ea.T - k0 : kEfTc;
      // the chunk's arms: lane i < nk reads step k0 + i (nothing past column T - 1)
      int wa = 0, wb = 0;
      if (lane < nk) {
        wa = ea.arm_a[p * ea.lda + k0 + lane];
        if (ea.arm_b) wb = ea.arm_b[p * ea.ldb + k0 + lane];
      }
      for (int kk = 0; kk < nk; ++kk) {
        const int aa = __builtin_amdgcn_readlane(wa, kk);
        const int ab = __builtin_amdgcn_readlane(wb, kk);
#pragma unroll
        for (int s = 0; s < V; ++s) {
          double A = PA[s][0], B = PB[s][0];
#pragma unroll
          for (int a = 1; a < NARM; ++a) {
            A = aa == a ? PA[s][a] : A;
            B = aa == a ? PB[s][a] : B;
          }
          yA[s] = fma(A, yA[s], B);
        }
        if (nser == 3) {
#pragma unroll
          for (int s = 0; s < V; ++s) {
            double A = PA[s][0], B = PB[s][0];
#pragma unroll
            for (int a = 1; a < NARM; ++a) {
              A = ab == a ? PA[s][a] : A;
              B = ab == a ? PB[s][a] : B;
            }
            yB[s] = fma(A, yB[s], B);
          }
        }
        // the series, NB at a time (the NB sorts and reductions are independent chains issued together)
#pragma unroll 1
        for (int sv0 = 0; sv0 < NSER; sv0 += NB) {
          double v[NB][V], key[NB][V];
          bool any_nan[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int sv = sv0 + b;
            bool bad = false;
#pragma unroll
            for (int s = 0; s < V; ++s) {
              v[b][s] = sv == 0 ? yA[s] : (sv == 1 ? yB[s] : yA[s] - yB[s]);
              const bool isn = v[b][s] != v[b][s];
              bad = bad || (valid[s] && isn);
              key[b][s] = (valid[s] && !isn) ? v[b][s] : inf;
            }
            any_nan[b] = __builtin_amdgcn_ballot_w64(bad) != 0;
          }
          // mean, shifted by c = v[1] (lane 1, slot 0), and the two-pass standard deviation; fixed order: the lane's
          // slots ascending, then the wave butterfly
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
            double* st = stage + ((sv0 + b) * NS) * kEfTc + kk;
            const double point = readlane_f64(v[b][0], 0);
            if (lane == 0) {
              st[0] = point;
              st[kEfTc] = any_nan[b] ? nan : mean[b];
              st[2 * kEfTc] = any_nan[b] ? nan : sd[b];
            }
            for (int j = 0; j < ea.Q; ++j) {
              const int i = (int)ea.qr[j].i;
              const double g = ea.qr[j].g;
              const double lo = ef_rank_value<V>(key[b], i);
              const double hi = ef_rank_value<V>(key[b], i + 1 < n ? i + 1 : n - 1);
              double qv = (g == 0.0 || lo == hi) ? lo : lo + g * (hi - lo);
              qv = any_nan[b] ? nan : qv;
              if (lane == 0) st[(3 + j) * kEfTc] = qv;
            }
          }
        }
      }
      // ---- flush the chunk: row (series, stat), columns k0 .. k0 + nk - 1 ------------------------------------
      wave_lds_sync();
      const int n_el = nser * NS * kEfTc;
      for (int e = lane; e < n_el; e += kWave) {
        const int row = e / kEfTc, col = e % kEfTc;
        if (col < nk) ea.out[((int64_t)row * ea.N + p) * ea.ldo + k0 + col] = stage[e];
      }
      wave_lds_sync();
    }
  }
}

template <int V, int NSER>
void ef_launch_vs(int na, dim3 grid, hipStream_t hs, const EfArgs& ea, const AffineLib& lib) {
  if (na == 1) effect_bands_kernel<V, 1, NSER><<<grid, kWave, 0, hs>>>(ea, lib);
  else if (na == 2) effect_bands_kernel<V, 2, NSER><<<grid, kWave, 0, hs>>>(ea, lib);
  else effect_bands_kernel<V, 4, NSER><<<grid, kWave, 0, hs>>>(ea, lib);
}

template <int V>
void ef_launch_v(int na, dim3 grid, hipStream_t hs, const EfArgs& ea, const AffineLib& lib) {
  if (ea.arm_b) ef_launch_vs<V, 3>(na, grid, hs, ea, lib);
  else ef_launch_vs<V, 1>(na, grid, hs, ea, lib);
}

}  // namespace

extern "C" {

int32_t insite_effect_abi_version(void) { return INSITE_EFFECT_ABI_VERSION; }

size_t insite_effect_workspace_bytes(int64_t, int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

int32_t insite_effect_bands_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                double dt, int32_t method, int32_t substeps, double drop_below,
                                int32_t n_replicates, const double* q, int32_t n_quantiles, double* out,
                                int64_t ld_out, void* /*workspace*/, size_t /*workspace_bytes*/, void* stream) {
  if (n_rows < 0 || T < 1 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || substeps < 1 || !(dt >= 0.0) ||
      ld_arm_a < (int64_t)T || (arm_b && ld_arm_b < (int64_t)T) || ld_out < (int64_t)T || n_replicates < 2 ||
      check_quantiles(q, n_quantiles, INSITE_EFFECT_MAX_QUANTILES) != INSITE_OK)
    return INSITE_E_INVALID_ARG;
  if (method != INSITE_METHOD_EULER && method != INSITE_METHOD_RK4) return INSITE_E_UNSUPPORTED;
  AffineLib lib;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, &lib);
  if (st != INSITE_OK) return st;
  if (n_replicates > INSITE_EFFECT_MAX_REPLICATES) return INSITE_E_UNSUPPORTED;
  if (n_rows == 0) return INSITE_OK;
  if (!y0 || !arm_a || !coef || !out || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;

  EfArgs ea;
  std::memset(&ea, 0, sizeof(ea));
  ea.y0 = y0;
  ea.u = n_statics > 0 ? u : y0;  // never read
  ea.arm_a = arm_a;
  ea.arm_b = arm_b;
  ea.coef = coef;
  ea.out = out;
  ea.lda = ld_arm_a;
  ea.ldb = arm_b ? ld_arm_b : 0;
  ea.ldo = ld_out;
  ea.N = n_rows;
  ea.T = T;
  ea.A = n_arms;
  ea.substeps = substeps;
  ea.method = method;
  ea.R = n_replicates;
  ea.Q = n_quantiles;
  ea.dt = dt;
  ea.drop = drop_below;
  for (int j = 0; j < n_quantiles; ++j) ea.qr[j] = quantile_rank(q[j], n_replicates - 1);
  const int64_t blocks = n_rows < kEfMaxBlocks ? n_rows : kEfMaxBlocks;
  ea.ppb = (n_rows + blocks - 1) / blocks;
  const dim3 grid((unsigned)((n_rows + ea.ppb - 1) / ea.ppb));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const int na = n_arms <= 1 ? 1 : (n_arms <= 2 ? 2 : 4);
  if (n_replicates <= 64) ef_launch_v<1>(na, grid, hs, ea, lib);
  else if (n_replicates <= 128) ef_launch_v<2>(na, grid, hs, ea, lib);
  else if (n_replicates <= 256) ef_launch_v<4>(na, grid, hs, ea, lib);
  else ef_launch_v<8>(na, grid, hs, ea, lib);
  return launch_status();
}

}  // extern "C"
