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
//                         The prologue is insite_affine.h's ensemble_maps (the replicate fold and its keep-NaN rule),
//                         a series' statistics insite_wavestats.h's ef_series_stats; the host checks, the rows per
//                         block and the choice of V and NARM are insite_affine.h's, shared with the other two units.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "insite_affine.h"
#include "insite_effect.h"
#include "insite_wavestats.h"

namespace {

// ---------------------------------------------------------------------------------------------
// effect_bands_kernel
// ---------------------------------------------------------------------------------------------
constexpr int kEfTc = 16;                                   // steps staged in LDS between two flushes
constexpr int kEfMaxStats = 3 + INSITE_EFFECT_MAX_QUANTILES;

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
  const double h = ea.dt / (double)ea.substeps;
  const int64_t p_lo = (int64_t)blockIdx.x * ea.ppb;
  const int64_t p_hi = p_lo + ea.ppb < ea.N ? p_lo + ea.ppb : ea.N;

  bool valid[V];  // the slot holds a resampled replicate (1..R-1); replicate 0 is lane 0, slot 0
#pragma unroll
  for (int s = 0; s < V; ++s) valid[s] = s * kWave + lane >= 1 && s * kWave + lane < ea.R;

  for (int64_t p = p_lo; p < p_hi; ++p) {
    // ---- prologue: the interval maps of the lane's replicates (insite_affine.h) ------------------------------
    double PA[V][NARM], PB[V][NARM];
    ensemble_maps<V, NARM>(lib, ea.coef, ea.u + p * lib.U, ea.R, ea.A, ea.drop, ea.method, ea.substeps, h, lane, PA,
                           PB);
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
          double v[NB][V];
#pragma unroll
          for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int s = 0; s < V; ++s) v[b][s] = sv0 + b == 0 ? yA[s] : (sv0 + b == 1 ? yB[s] : yA[s] - yB[s]);
          ef_series_stats<NB, V>(v, valid, lane, n, ea.Q, ea.qr, stage + sv0 * NS * kEfTc + kk, kEfTc);
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
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) || ld_arm_a < (int64_t)T ||
      (arm_b && ld_arm_b < (int64_t)T) || ld_out < (int64_t)T ||
      check_quantiles(q, n_quantiles, INSITE_EFFECT_MAX_QUANTILES) != INSITE_OK)
    return INSITE_E_INVALID_ARG;
  AffineLib lib;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_EFFECT_MAX_REPLICATES, &lib);
  if (st != INSITE_OK || n_rows == 0) return st;
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
  ea.ppb = rows_per_block(n_rows);
  const dim3 grid((unsigned)((n_rows + ea.ppb - 1) / ea.ppb));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  with_slots(n_replicates, n_arms, [&](auto v, auto narm) {
    if (arm_b) effect_bands_kernel<v(), narm(), 3><<<grid, kWave, 0, hs>>>(ea, lib);
    else effect_bands_kernel<v(), narm(), 1><<<grid, kWave, 0, hs>>>(ea, lib);
  });
  return launch_status();
}

}  // extern "C"
