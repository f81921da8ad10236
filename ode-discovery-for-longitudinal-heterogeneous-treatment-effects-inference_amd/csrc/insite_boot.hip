// insite_boot.hip — patient-level Poisson bootstrap of the discovery Gram systems on MI355X (gfx950):
// include/insite_bootstrap.h, DESIGN.md §9g.
//
// Kernels:
//   boot_gram_kernel      R replicates x N patients x (n_arms nE) entry columns as a GEMM on
//                         v_mfma_f64_16x16x4f64: M = 16 replicates, K = 4 patients, N = 16 entry columns.  The A
//                         operand (the Poisson weight of [replicate lane & 15][patient lane >> 4]) is made in
//                         registers, one Threefry-2x32-20 block per two patients; the B operand (a patient's Gram
//                         entries, arm-major columns) is expanded from mom, u and the table once per 8 patients and
//                         held while the wave walks its replicate tiles.  The weights never exist in memory.
//   boot_finalize_kernel  the waves' partials -> G | b in a fixed order; mirrors the triangle into the full G.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "insite_bootstrap.h"
#include "insite_affine.h"
#include "insite_bootplan.h"

namespace {

// ---------------------------------------------------------------------------------------------
// boot_gram_kernel
// ---------------------------------------------------------------------------------------------
// Block = one wave, independent of every other.  blockIdx.x: a contiguous run of 8-patient groups; blockIdx.y: a
// group of RT replicate tiles; blockIdx.z: a chunk of CT 16-column tiles of the n_arms nE entry columns (column
// c = a nE + e: entry e of arm a; a patient's B value is its entry where a is its arm, else 0 -- a select).
//
// Groups are aligned in the GLOBAL patient index g = patient_offset + p (base a multiple of 8; slots outside the
// shard are masked), so the Threefry pair q = g >> 1 of slot s is (base >> 1) + (s >> 1) whatever the offset.  The
// lane (replicate lane & 15, kq = lane >> 4) hashes pair (base >> 1) + kq once per replicate tile and gets the
// weights of slots 2 kq (word a) and 2 kq + 1 (word b): the K index of the first MFMA of the group runs over the
// even slots, that of the second over the odd ones, and the B operands are read in the same order -- no lane
// exchange.  Per group the wave first expands the 8 patients into LDS rows {m_0..m_8, mom_0..mom_4, arm, 1} (lane
// = slot x 8 + column; column 8 by the lanes of column 0), then every lane reads its 2 CT B values.
// The accumulators (RT x CT tiles of 4 f64) stay in registers over the wave's whole patient run; at the end they
// go to the wave's partial [rpad][cpad] (C/D layout of the f64 MFMA: register j = row (lane >> 4) + 4 j, column
// lane & 15).  Replicate tiles past R are skipped; the rows past R inside the last tile run on their own keys and are
// never read.
// (the tiling constants, BtPlan / bt_plan and the finalisation: insite_bootplan.h, shared with insite_segboot.hip)
constexpr int kBtPs = 17;              // LDS row of one patient (odd -> conflict free)

template <int RT, int CT>
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2)))
boot_gram_kernel(const double* __restrict__ mom, const double* __restrict__ u, const int8_t* __restrict__ arm,
                 const int32_t* __restrict__ rows, int min_rows, int64_t N, int64_t off, int n_arms, AffineGramLib lib,
                 uint32_t seed, int R, int ncol, int64_t g0, int64_t nG, int64_t gpw, int64_t rpad, int64_t cpad,
                 double* __restrict__ partial) {
  __shared__ double ps[8 * kBtPs];
  const int lane = threadIdx.x;
  const int col = lane & 15, kq = lane >> 4;
  const int rt0 = blockIdx.y * RT;
  const int ct0 = blockIdx.z * CT;

  // this lane's entry columns, packed: the LDS slots of m_i | m_k (15: the constant 1) << 8 | the moment << 16 |
  // (arm + 2) << 24 (0: no such column)
  int c_desc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) {
    const int c = (ct0 + t) * 16 + col;
    const bool ok = c < ncol;
    const int a = ok ? c / lib.nE : 0;
    const int e = ok ? c - a * lib.nE : 0;
    const int i = lib.ei[e], k = lib.ek[e];
    const int exi = (lib.ucode[i] >> 24) & 0xff;
    const int exk = k >= 0 ? (lib.ucode[k] >> 24) & 0xff : 0;
    c_desc[t] = i | (k >= 0 ? k : 15) << 8 | (k >= 0 ? 9 + exi + exk : 12 + exi) << 16 | (ok ? a + 2 : 0) << 24;
  }
  dbl4 acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[rt][t] = dbl4{0.0, 0.0, 0.0, 0.0};

  const int s1 = lane >> 3, j1 = lane & 7;  // expansion: slot and column of this lane
  const int64_t gi_lo = (int64_t)blockIdx.x * gpw;
  const int64_t gi_hi = gi_lo + gpw < nG ? gi_lo + gpw : nG;
  for (int64_t gi = gi_lo; gi < gi_hi; ++gi) {
    const int64_t base = g0 + 8 * gi;  // global index of slot 0 (a multiple of 8)
    {
      const int64_t p = base + s1 - off;
      const bool valid = p >= 0 && p < N;
      const int64_t pc = valid ? p : 0;
      const int arm_p = arm[pc];
      const bool on = valid && arm_p >= 0 && arm_p < n_arms && (rows == nullptr || rows[pc] >= min_rows);
      double uu[INSITE_MAX_STATICS];
#pragma unroll
      for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? u[pc * lib.U + t] : 0.0;
      double* row = ps + s1 * kBtPs;
      if (j1 < lib.F) row[j1] = monomial_code(lib.ucode[j1] & 0xffffff, uu);
      if (j1 == 0 && lib.F > 8) row[8] = monomial_code(lib.ucode[8] & 0xffffff, uu);
      if (j1 < 5) row[9 + j1] = mom[pc * 5 + j1];
      if (j1 == 5) row[14] = (double)(on ? arm_p : -1);
      if (j1 == 6) row[15] = 1.0;
    }
    wave_lds_sync();
    double bv[2][CT];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double* row = ps + (2 * kq + h) * kBtPs;
      const int a = (int)row[14] + 2;  // 1: contributes nothing
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int d = c_desc[t];
        const double v = row[d & 0xff] * row[(d >> 8) & 0xff] * row[(d >> 16) & 0xff];
        bv[h][t] = a == (d >> 24) ? v : 0.0;
      }
    }
    wave_lds_sync();
    const uint64_t q = (uint64_t)(base >> 1) + (uint64_t)kq;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      if ((rt0 + rt) * 16 < R) {  // (uniform)
        const uint32_t r = (uint32_t)((rt0 + rt) * 16 + col);
        uint32_t wa = (uint32_t)q, wb = (uint32_t)(q >> 32);
        threefry2x32_20(seed, r, wa, wb);
        const double w0 = r == 0u ? 1.0 : (double)poisson1_weight(wa);
        const double w1 = r == 0u ? 1.0 : (double)poisson1_weight(wb);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
          acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, bv[0][t], acc[rt][t], 0, 0, 0);
          acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1, bv[1][t], acc[rt][t], 0, 0, 0);
        }
      }
    }
  }
  // the wave's partial [rpad][cpad]: rows (rt0 + rt) 16 + kq + 4 j < rpad, columns (ct0 + t) 16 + col < cpad
  double* out = partial + (int64_t)blockIdx.x * rpad * cpad;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out[(int64_t)((rt0 + rt) * 16 + kq + 4 * j) * cpad + (ct0 + t) * 16 + col] = acc[rt][t][j];
}

int32_t run_boot_gram(const double* mom, const double* u, const int8_t* arm, const int32_t* rows, int32_t min_rows,
                      int64_t n_patients, int64_t patient_offset, int32_t n_statics, int32_t n_arms,
                      const int8_t* exps, int32_t n_terms, int32_t n_replicates, uint32_t seed, double* G_out,
                      double* b_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_patients < 0 || patient_offset < 0 || patient_offset > INT64_MAX - n_patients - 8 || !G_out || !b_out ||
      n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_replicates < 1)
    return INSITE_E_INVALID_ARG;
  if (n_patients > 0 && (!mom || !arm || (n_statics > 0 && !u))) return INSITE_E_INVALID_ARG;
  AffineGramLib lib;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, &lib);
  if (st != INSITE_OK) return st;
  if (n_replicates > INSITE_BOOT_MAX_REPLICATES) return INSITE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < insite_bootstrap_workspace_bytes(n_patients, n_arms, n_terms, n_replicates))
    return INSITE_E_WORKSPACE;
  if (n_patients == 0) return INSITE_OK;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const BtPlan pl = bt_plan(n_patients, n_arms, lib.nE, n_replicates);
  const int64_t g0 = patient_offset & ~(int64_t)7;
  const int64_t nG = (patient_offset + n_patients - g0 + 7) / 8;  // <= (N + 7) / 8 + 1
  const int64_t gpw = (nG + pl.n_px - 1) / pl.n_px;
  double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + kBtHeader);
  if (n_statics == 0) u = mom;  // never read
  const dim3 grid((unsigned)pl.n_px, (unsigned)pl.n_rg, (unsigned)pl.n_z);
#define INSITE_BOOT_LAUNCH(RT, CT)                                                                                     \
  boot_gram_kernel<RT, CT><<<grid, kWave, 0, hs>>>(mom, u, arm, rows, min_rows, n_patients, patient_offset, n_arms, lib, \
                                               seed, n_replicates, pl.ncol, g0, nG, gpw, pl.rpad, pl.cpad, part)
  switch (pl.ct) {
    case 1: INSITE_BOOT_LAUNCH(kBtRt, 1); break;
    case 2: INSITE_BOOT_LAUNCH(kBtRt, 2); break;
    case 3: INSITE_BOOT_LAUNCH(kBtRt, 3); break;
    case 4: INSITE_BOOT_LAUNCH(kBtRt, 4); break;
    default: INSITE_BOOT_LAUNCH(kBtRt - 1, 5); break;
  }
#undef INSITE_BOOT_LAUNCH
  const int64_t n_out = (int64_t)n_replicates * pl.ncol;
  boot_finalize_kernel<<<dim3((unsigned)((n_out + kBtFinBlock - 1) / kBtFinBlock)), kBtFinBlock, 0, hs>>>(
      part, pl.n_px, pl.rpad, pl.cpad, n_replicates, n_arms, lib, G_out, b_out);
  return launch_status();
}

}  // namespace

extern "C" {

int32_t insite_bootstrap_abi_version(void) { return INSITE_BOOTSTRAP_ABI_VERSION; }

size_t insite_bootstrap_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t n_replicates) {
  if (n_patients < 0 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_terms < 1 || n_terms > INSITE_MAX_TERMS ||
      n_replicates < 1 || n_replicates > INSITE_BOOT_MAX_REPLICATES)
    return 0;
  // one partial [rpad][cpad] per wave of the patient dimension
  const BtPlan pl = bt_plan(n_patients, n_arms, n_terms * (n_terms + 1) / 2 + n_terms, n_replicates);
  return kBtHeader + (size_t)pl.n_px * (size_t)pl.rpad * (size_t)pl.cpad * sizeof(double);
}

int32_t insite_bootstrap_gram_f64(const double* mom, const double* u, const int8_t* arm, const int32_t* rows,
                                  int32_t min_rows, int64_t n_patients, int64_t patient_offset, int32_t n_statics,
                                  int32_t n_arms, const int8_t* exps, int32_t n_terms, int32_t n_replicates,
                                  uint32_t seed, double* G_out, double* b_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return run_boot_gram(mom, u, arm, rows, min_rows, n_patients, patient_offset, n_statics, n_arms, exps, n_terms,
                       n_replicates, seed, G_out, b_out, workspace, workspace_bytes, stream);
}

int32_t insite_sindy_bootstrap_f64(const double* mom, const double* u, const int8_t* arm, const int32_t* rows,
                                   int32_t min_rows, int64_t n_patients, int64_t patient_offset, int32_t n_statics,
                                   int32_t n_arms, const int8_t* exps, int32_t n_terms, int32_t n_replicates,
                                   uint32_t seed, int32_t optimizer, double threshold, double alpha, double nu,
                                   double tol, int32_t max_iter, int32_t unbias, double* G_out, double* b_out,
                                   double* coef_out, int8_t* mask_out, int32_t* iters_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (optimizer != INSITE_OPT_SR3 && optimizer != INSITE_OPT_STLSQ) return INSITE_E_INVALID_ARG;
  if (!coef_out || !bt_solver_params_ok(threshold, alpha, nu, tol, max_iter)) return INSITE_E_INVALID_ARG;
  const int32_t st = run_boot_gram(mom, u, arm, rows, min_rows, n_patients, patient_offset, n_statics, n_arms, exps,
                                   n_terms, n_replicates, seed, G_out, b_out, workspace, workspace_bytes, stream);
  if (st != INSITE_OK || n_patients == 0) return st;
  const int64_t n_sys = (int64_t)n_replicates * n_arms;
  if (optimizer == INSITE_OPT_SR3)
    return insite_sr3_f64(G_out, b_out, n_sys, n_terms, threshold, nu, tol, max_iter, unbias, coef_out, mask_out,
                          iters_out, stream);
  return insite_stlsq_f64(G_out, b_out, n_sys, n_terms, threshold, alpha, max_iter, unbias, coef_out, mask_out,
                          iters_out, stream);
}

}  // extern "C"
