// insite_weak.hip — weak-form SINDy discovery on MI355X (gfx950): include/insite_weak.h, DESIGN.md §9f.
//
// Kernels:
//   weak_prep_kernel   row sums c_k and the nonzero column range of every 16-row tile of W | D.
//   gram_weak_kernel   projections a = W x, d = -D x of every patient's series onto the K test functions on
//                      v_mfma_f64_16x16x4f64 (inside the tiles' ranges only), the five per-patient moment sums over k
//                      straight from the
//                      accumulators, their per-arm expansion to Gram entries (one entry per lane, as the strong
//                      form's scalar path) and the block's partial.  a and d never leave the registers.
//   weak_finalize_kernel  the block partials -> G | b in a fixed order (groups of 16 blocks, then the groups).
//   sr3_kernel         thread = system: SR3 with the l1 prox on the column-normalised Gram system.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "insite_weak.h"
#include "insite_affine.h"

namespace {

// entries of one arm's system at F = INSITE_MAX_TERMS (AffineGramLib's entry list)
constexpr int kWkMaxEnt = INSITE_MAX_TERMS * (INSITE_MAX_TERMS + 1) / 2 + INSITE_MAX_TERMS;  // 54 <= one wave

// ---------------------------------------------------------------------------------------------
// weak_prep_kernel + gram_weak_kernel
// ---------------------------------------------------------------------------------------------
// A test function touches only the grid points of its subdomain (the default H = L / 20: a tenth of the grid), so
// W and D are mostly zeros.  weak_prep_kernel (one block per tile of 16 rows) finds each tile's nonzero column
// range [lo, hi) (rounded to multiples of 4) and every row's sum c_k = sum_i W[k,i] (lane-strided partial sums,
// then a butterfly: a fixed order).  gram_weak_kernel then multiplies only inside the ranges: with the rows sorted
// by centre (insite_amd.weak / SINDY.fit_weak sort them; the sum over k does not depend on the row order) a tile's
// range is its 16 subdomains' union, about a quarter of the grid at K = 100.  Unsorted or dense rows are handled
// the same way, only slower.
// Block = 4 waves = one 64-patient tile; wave = a 16-patient column group, independent of the other waves until
// the block's partial.  Per row tile kt and 4 steps the wave issues one B operand (x[t + (lane >> 4)][patient
// lane & 15]) against two A operands (W / D[16 kt + (lane & 15)][t + (lane >> 4)]) on v_mfma_f64_16x16x4f64:
//     aW (16 test functions x 16 patients) += W tile . x tile,   aD += D tile . x tile.
// The operands come straight from the caches: W and D are K T 16 B in all, read by every wave; a wave's x columns
// are re-read once per row tile whose range covers them.  Rows past K and steps past T enter as zeros (the loads
// are clamped and masked; nothing is read out of bounds).  After a tile's last step the lane holds a, d of rows
// (lane >> 4) + 4 j for patient lane & 15 (the f64 C/D layout): it adds c^2, c a, a^2, c d, a d into its five
// sums, and after the last tile two butterfly steps over lane >> 4 complete them.  a and d never leave the
// registers.
#ifndef INSITE_WEAK_UNROLL
#define INSITE_WEAK_UNROLL 2  // 4-step groups loaded ahead of their MFMAs (A/B 2 / 4 / 8: profiles/weak/unroll_ab.jsonl)
#endif
constexpr int kWkUnroll = INSITE_WEAK_UNROLL;
constexpr int kWkPs = 17;             // per-patient LDS row of the expansion (odd -> conflict free)
constexpr int kWkMaxBlocks = 8192;    // partials; larger cohorts loop over tiles
constexpr int kWkGroup = 16;          // blocks per group of the fixed-order reduction
constexpr size_t kWkHeader = 512;     // the ABI's zero header (this path keeps no counters in it)
constexpr int kWkMaxTiles = INSITE_WEAK_MAX_K / 16;
constexpr size_t kWkPrepBytes = INSITE_WEAK_MAX_K * sizeof(double) + 2 * kWkMaxTiles * sizeof(int32_t);

inline int64_t wk_grid(int64_t N) {
  int64_t g = (N + kWave - 1) / kWave;
  if (g > kWkMaxBlocks) g = kWkMaxBlocks;
  return g < 1 ? 1 : g;
}

__global__ void __launch_bounds__(kBlock)
weak_prep_kernel(const double* __restrict__ W, const double* __restrict__ D, int64_t ldw, int K, int T,
                 double* __restrict__ cvec, int32_t* __restrict__ rng) {
  __shared__ int slo[16], shi[16];
  const int kt = blockIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  for (int rr = wid; rr < 16; rr += kWavesPerBlock) {
    const int r = kt * 16 + rr;
    double s = 0.0;
    int lo = T, hi = 0;
    if (r < K) {
      for (int t = lane; t < T; t += kWave) {
        const double w = W[(int64_t)r * ldw + t];
        const double d = D[(int64_t)r * ldw + t];
        s += w;
        if (w != 0.0 || d != 0.0) {
          lo = min(lo, t);
          hi = max(hi, t + 1);
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, kWave);
      lo = min(lo, __shfl_xor(lo, off, kWave));
      hi = max(hi, __shfl_xor(hi, off, kWave));
    }
    if (lane == 0) {
      cvec[r] = s;
      slo[rr] = lo;
      shi[rr] = hi;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int lo = T, hi = 0;
    for (int rr = 0; rr < 16; ++rr) {
      lo = min(lo, slo[rr]);
      hi = max(hi, shi[rr]);
    }
    rng[2 * kt] = lo & ~3;
    rng[2 * kt + 1] = (hi + 3) & ~3;
  }
}

template <int NARM>
__global__ void __launch_bounds__(kBlock)
gram_weak_kernel(const double* __restrict__ x, int64_t xsp, int64_t xst, int T, const double* __restrict__ W,
                 const double* __restrict__ D, int64_t ldw, int K, const double* __restrict__ cvec,
                 const int32_t* __restrict__ rng, const double* __restrict__ u, const int8_t* __restrict__ arm,
                 const int32_t* __restrict__ rows, int64_t N, int n_arms, AffineGramLib lib,
                 double* __restrict__ partial, double* __restrict__ mom) {
  __shared__ double psm[kWavesPerBlock * 16 * kWkPs];
  __shared__ double red[kWavesPerBlock * INSITE_MAX_ARMS * kWave];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int col = lane & 15, kq = lane >> 4;
  double acc[NARM];
#pragma unroll
  for (int a = 0; a < NARM; ++a) acc[a] = 0.0;
  const int my_i = lane < lib.nE ? lib.ei[lane] : 0;
  const int my_k = lane < lib.nE ? lib.ek[lane] : 0;
  const int my_exi = (lib.ucode[my_i] >> 24) & 0xff;
  const int my_exk = my_k >= 0 ? (lib.ucode[my_k] >> 24) & 0xff : 0;
  const int moff = my_k >= 0 ? 9 + my_exi + my_exk : 12 + my_exi;
  double* ps = psm + wid * (16 * kWkPs);
  const int n_kt = (K + 15) / 16;

  const int64_t n_tiles = (N + kWave - 1) / kWave;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p = tile * kWave + wid * 16 + col;
    const int64_t pc = p < N ? p : N - 1;
    const int arm_p = arm[pc];
    const bool on = p < N && rows[pc] >= T && arm_p >= 0 && arm_p < n_arms;
    const double* xcol = x + pc * xsp;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0;

    for (int kt = 0; kt < n_kt; ++kt) {
      const int lo = __builtin_amdgcn_readfirstlane(rng[2 * kt]);
      const int hi = __builtin_amdgcn_readfirstlane(rng[2 * kt + 1]);
      if (lo >= hi) continue;  // (uniform) an all-zero tile: c = a = d = 0
      const int r = kt * 16 + col;
      const bool rok = r < K;
      const double* wp = W + (int64_t)(rok ? r : K - 1) * ldw;
      const double* dp = D + (int64_t)(rok ? r : K - 1) * ldw;
      dbl4 aW = {0.0, 0.0, 0.0, 0.0}, aD = {0.0, 0.0, 0.0, 0.0};
      // kWkUnroll 4-step groups per iteration: their 3 kWkUnroll operand loads are issued before the first MFMA
      for (int t = lo; t < hi; t += 4 * kWkUnroll) {
        double wa[kWkUnroll], da[kWkUnroll], xb[kWkUnroll];
#pragma unroll
        for (int q = 0; q < kWkUnroll; ++q) {
          const int tt = t + 4 * q + kq;
          const bool tok = tt < T;  // (past hi, inside T: the tile's own zeros)
          const int tc = tok ? tt : T - 1;
          const double wv = wp[tc];
          const double dv = dp[tc];
          const double xv = xcol[(int64_t)tc * xst];
          wa[q] = rok && tok ? wv : 0.0;
          da[q] = rok && tok ? dv : 0.0;
          xb[q] = tok ? xv : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kWkUnroll; ++q) {
          if (t + 4 * q < hi) {  // (uniform)
            aW = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[q], xb[q], aW, 0, 0, 0);
            aD = __builtin_amdgcn_mfma_f64_16x16x4f64(da[q], xb[q], aD, 0, 0, 0);
          }
        }
      }
      // C/D layout of the f64 MFMA: register j of the lane = row (lane >> 4) + 4 j, column lane & 15
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double c = cvec[kt * 16 + kq + 4 * j];
        const double a = aW[j];
        const double d = -aD[j];
        S0 = fma(c, c, S0);
        S1 = fma(c, a, S1);
        S2 = fma(a, a, S2);
        S3 = fma(c, d, S3);
        S4 = fma(a, d, S4);
      }
    }
    S0 += __shfl_xor(S0, 16, kWave);
    S1 += __shfl_xor(S1, 16, kWave);
    S2 += __shfl_xor(S2, 16, kWave);
    S3 += __shfl_xor(S3, 16, kWave);
    S4 += __shfl_xor(S4, 16, kWave);
    S0 += __shfl_xor(S0, 32, kWave);
    S1 += __shfl_xor(S1, 32, kWave);
    S2 += __shfl_xor(S2, 32, kWave);
    S3 += __shfl_xor(S3, 32, kWave);
    S4 += __shfl_xor(S4, 32, kWave);
    if (!on) S0 = S1 = S2 = S3 = S4 = 0.0;
    if (mom && kq == 0 && p < N) {
      double* mrow = mom + p * 5;
      mrow[0] = S0;
      mrow[1] = S1;
      mrow[2] = S2;
      mrow[3] = S3;
      mrow[4] = S4;
    }
    // ---- per-patient Gram block A(u) M A(u)^T, one entry per lane over the wave's 16 patients ----
    wave_lds_sync();
    if (kq == 0) {
      double uu[INSITE_MAX_STATICS];
#pragma unroll
      for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? u[pc * lib.U + t] : 0.0;
      double* row = ps + col * kWkPs;
      for (int j = 0; j < lib.F; ++j) row[j] = monomial_code(lib.ucode[j] & 0xffffff, uu);
      row[9] = S0;
      row[10] = S1;
      row[11] = S2;
      row[12] = S3;
      row[13] = S4;
      row[14] = (double)(on ? arm_p : -1);
    }
    wave_lds_sync();
    if (lane < lib.nE) {
      for (int q = 0; q < 16; ++q) {
        const double* row = ps + q * kWkPs;
        double wq = row[my_i] * row[moff];
        if (my_k >= 0) wq *= row[my_k];
        const int a = (int)row[14];
#pragma unroll
        for (int aa = 0; aa < NARM; ++aa) acc[aa] += (a == aa) ? wq : 0.0;
      }
    }
    wave_lds_sync();
  }
  // ---- the block's partial: waves 0..3 per entry, in order ----
#pragma unroll
  for (int a = 0; a < NARM; ++a) red[(wid * NARM + a) * kWave + lane] = acc[a];
  __syncthreads();
  const int n_ent = n_arms * lib.nE;
  for (int idx = tid; idx < n_ent; idx += kBlock) {
    const int a = idx / lib.nE, e = idx - a * lib.nE;
    double v = red[a * kWave + e];
#pragma unroll
    for (int ww = 1; ww < kWavesPerBlock; ++ww) v += red[(ww * NARM + a) * kWave + e];
    partial[(int64_t)blockIdx.x * n_ent + idx] = v;
  }
}

// One block: group sums (kWkGroup consecutive blocks, block order) -> gpart, then the groups in order -> G | b.
constexpr int kWkFinBlock = 1024;
__global__ void __launch_bounds__(kWkFinBlock)
weak_finalize_kernel(const double* __restrict__ part, int nblk, int n_arms, AffineGramLib lib,
                     double* __restrict__ gpart, double* __restrict__ G, double* __restrict__ b) {
  const int n_ent = n_arms * lib.nE;
  const int ng = (nblk + kWkGroup - 1) / kWkGroup;
  for (int pi = threadIdx.x; pi < ng * n_ent; pi += kWkFinBlock) {
    const int g = pi / n_ent, q = pi - g * n_ent;
    const int g0 = g * kWkGroup;
    const int gs = nblk - g0 < kWkGroup ? nblk - g0 : kWkGroup;
    double v[kWkGroup];
#pragma unroll
    for (int j = 0; j < kWkGroup; ++j) v[j] = part[(int64_t)(g0 + (j < gs ? j : 0)) * n_ent + q];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kWkGroup; ++j) s += j < gs ? v[j] : 0.0;
    gpart[pi] = s;
  }
  __threadfence_block();
  __syncthreads();
  const int64_t F = lib.F;
  for (int q = threadIdx.x; q < n_ent; q += kWkFinBlock) {
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += gpart[(int64_t)g * n_ent + q];
    const int a = q / lib.nE, e = q - a * lib.nE;
    const int i = lib.ei[e], k = lib.ek[e];
    if (k >= 0) {
      G[(a * F + i) * F + k] = s;
      G[(a * F + k) * F + i] = s;
    } else {
      b[a * F + i] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// SR3
// ---------------------------------------------------------------------------------------------
// Cholesky factor of (g + shift I) restricted to the support mask m (inactive rows / columns: identity);
// only the lower triangle of g is read.  False when a pivot is not positive.
template <int F>
__device__ bool wk_factor(const double (&g)[F][F], unsigned m, double shift, double (&l)[F][F], double (&rd)[F]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < F; ++i) {
    const bool ai = (m >> i) & 1u;
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const bool act = ai && ((m >> j) & 1u);
      double a = act ? g[i][j] : 0.0;
      if (i == j) a = ai ? a + shift : 1.0;
#pragma unroll
      for (int q = 0; q < j; ++q) a = fma(-l[i][q], l[j][q], a);
      if (i == j) {
        if (!(a > 0.0)) {
          ok = false;
          a = 1.0;
        }
        l[i][i] = sqrt(a);
        rd[i] = 1.0 / l[i][i];
      } else {
        l[i][j] = a * rd[j];
      }
    }
  }
  return ok;
}

template <int F>
__device__ void wk_solve(const double (&l)[F][F], const double (&rd)[F], unsigned m, const double (&rhs)[F],
                         double (&c)[F]) {
  double z[F];
#pragma unroll
  for (int i = 0; i < F; ++i) {
    double s = ((m >> i) & 1u) ? rhs[i] : 0.0;
#pragma unroll
    for (int q = 0; q < i; ++q) s = fma(-l[i][q], z[q], s);
    z[i] = s * rd[i];
  }
#pragma unroll
  for (int i = F - 1; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int q = i + 1; q < F; ++q) s = fma(-l[q][i], c[q], s);
    c[i] = ((m >> i) & 1u) ? s * rd[i] : 0.0;
  }
}

template <int F>
__global__ void __launch_bounds__(kBlock)
sr3_kernel(const double* __restrict__ G, const double* __restrict__ b, int64_t n_sys, double thr, double nu, double tol,
           int max_iter, int unbias, double* __restrict__ coef, int8_t* __restrict__ mask,
           int32_t* __restrict__ iters) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sys) return;
  constexpr unsigned all = (1u << F) - 1u;
  double g[F][F], gn[F][F], l[F][F], rd[F], rhs[F], bn[F], inv[F], v[F], w[F], r[F];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < F; ++i) {
    rhs[i] = b[s * F + i];
#pragma unroll
    for (int j = 0; j <= i; ++j) g[i][j] = G[(s * F + i) * F + j];
  }
#pragma unroll
  for (int i = 0; i < F; ++i) {
    if (!(g[i][i] > 0.0)) ok = false;
    inv[i] = 1.0 / sqrt(ok ? g[i][i] : 1.0);
  }
#pragma unroll
  for (int i = 0; i < F; ++i) {
    bn[i] = rhs[i] * inv[i];
#pragma unroll
    for (int j = 0; j <= i; ++j) gn[i][j] = g[i][j] * inv[i] * inv[j];
  }
  ok &= wk_factor<F>(gn, all, 0.0, l, rd);
  wk_solve<F>(l, rd, all, bn, v);
  const double inu = 1.0 / nu;
  ok &= wk_factor<F>(gn, all, inu, l, rd);
  int it = 0;
  if (ok) {
    for (int k = 0; k < max_iter; ++k) {
      it = k + 1;
#pragma unroll
      for (int i = 0; i < F; ++i) r[i] = bn[i] + v[i] * inu;
      wk_solve<F>(l, rd, all, r, w);
      double diff = 0.0;
#pragma unroll
      for (int i = 0; i < F; ++i) {
        const double mag = fabs(w[i]) - thr;
        const double vn = mag > 0.0 ? copysign(mag, w[i]) : 0.0;
        const double dv = vn - v[i];
        diff += dv * dv;
        v[i] = vn;
      }
      if (sqrt(diff) * inu < tol) break;
    }
  }
  unsigned sup = 0u;
#pragma unroll
  for (int i = 0; i < F; ++i)
    if (fabs(v[i]) > 1e-14) sup |= 1u << i;
  double c[F];
  if (unbias && sup) {
    ok &= wk_factor<F>(g, sup, 0.0, l, rd);
    wk_solve<F>(l, rd, sup, rhs, c);
  } else {
#pragma unroll
    for (int i = 0; i < F; ++i) c[i] = v[i] * inv[i];
  }
  if (!ok) {
    sup = 0u;
    it = -1;
#pragma unroll
    for (int i = 0; i < F; ++i) c[i] = __builtin_nan("");
  }
#pragma unroll
  for (int i = 0; i < F; ++i) {
    coef[s * F + i] = c[i];
    if (mask) mask[s * F + i] = (int8_t)((sup >> i) & 1u);
  }
  if (iters) iters[s] = it;
}

inline bool sr3_params_ok(double threshold, double nu, double tol, int32_t max_iter) {
  return threshold >= 0.0 && tol >= 0.0 && nu > 0.0 && max_iter >= 0;  // NaN fails every comparison
}

template <int NARM>
void launch_gram_weak(hipStream_t hs, int64_t grid, const double* x, int64_t xsp, int64_t xst, int T, const double* W,
                      const double* D, int64_t ldw, int K, const double* cvec, const int32_t* rng, const double* u,
                      const int8_t* arm, const int32_t* rows, int64_t N, int n_arms, const AffineGramLib& lib,
                      double* part, double* mom) {
  gram_weak_kernel<NARM><<<dim3((unsigned)grid), kBlock, 0, hs>>>(x, xsp, xst, T, W, D, ldw, K, cvec, rng, u, arm, rows,
                                                                  N, n_arms, lib, part, mom);
}

int32_t run_weak_gram(const double* x, int64_t ldx, int32_t layout, int32_t n_steps, const double* W, const double* D,
                      int64_t ldw, int32_t K, const double* u, const int8_t* arm, const int32_t* rows,
                      int64_t n_patients, int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms,
                      double* G_out, double* b_out, double* mom_out, void* workspace, size_t workspace_bytes,
                      void* stream) {
  const bool tm = layout == INSITE_LAYOUT_TIME_MAJOR;
  if (layout != INSITE_LAYOUT_PATIENT_MAJOR && !tm) return INSITE_E_INVALID_ARG;
  if (n_patients < 0 || !G_out || !b_out || n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_steps < 1 || K < 1 ||
      ldw < n_steps || (tm ? ldx < n_patients : ldx < n_steps) || ldx < 1)
    return INSITE_E_INVALID_ARG;
  if (n_patients > 0 && (!x || !W || !D || !arm || !rows || (n_statics > 0 && !u))) return INSITE_E_INVALID_ARG;
  AffineGramLib lib;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, &lib);
  if (st != INSITE_OK) return st;
  if (K > INSITE_WEAK_MAX_K) return INSITE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < insite_gram_weak_workspace_bytes(n_patients, n_arms, n_terms, K))
    return INSITE_E_WORKSPACE;
  if (n_patients == 0) return INSITE_OK;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const int64_t grid = wk_grid(n_patients);
  const int n_ent = n_arms * lib.nE;
  // workspace: header | c [INSITE_WEAK_MAX_K] | tile ranges [2 x 64] | block partials | group sums
  char* base = static_cast<char*>(workspace) + kWkHeader;
  double* cvec = reinterpret_cast<double*>(base);
  int32_t* rng = reinterpret_cast<int32_t*>(base + INSITE_WEAK_MAX_K * sizeof(double));
  double* part = reinterpret_cast<double*>(base + kWkPrepBytes);
  double* gpart = part + grid * n_ent;
  const int64_t xsp = tm ? 1 : ldx, xst = tm ? ldx : 1;
  if (n_statics == 0) u = x;
  weak_prep_kernel<<<dim3((unsigned)((K + 15) / 16)), kBlock, 0, hs>>>(W, D, ldw, K, n_steps, cvec, rng);
#define INSITE_WEAK_LAUNCH(NA)                                                                                    \
  launch_gram_weak<NA>(hs, grid, x, xsp, xst, n_steps, W, D, ldw, K, cvec, rng, u, arm, rows, n_patients, n_arms, \
                       lib, part, mom_out)
  if (n_arms == 1) INSITE_WEAK_LAUNCH(1);
  else if (n_arms == 2) INSITE_WEAK_LAUNCH(2);
  else INSITE_WEAK_LAUNCH(4);
#undef INSITE_WEAK_LAUNCH
  weak_finalize_kernel<<<1, kWkFinBlock, 0, hs>>>(part, (int)grid, n_arms, lib, gpart, G_out, b_out);
  return launch_status();
}

}  // namespace

extern "C" {

int32_t insite_weak_abi_version(void) { return INSITE_WEAK_ABI_VERSION; }

size_t insite_gram_weak_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t K) {
  if (n_patients < 0 || n_arms < 1 || n_arms > INSITE_MAX_ARMS || n_terms < 1 || n_terms > INSITE_MAX_TERMS || K < 1)
    return 0;
  // row sums and tile ranges (weak_prep_kernel), block partials [grid][n_arms * nE] and the group sums
  // [ceil(grid / 16)][n_arms * nE], nE <= 54
  const size_t grid = (size_t)wk_grid(n_patients);
  return kWkHeader + kWkPrepBytes + (grid + (grid + kWkGroup - 1) / kWkGroup) * (size_t)n_arms * kWkMaxEnt * sizeof(double);
}

int32_t insite_gram_weak_f64(const double* x, int64_t ldx, int32_t layout, int32_t n_steps, const double* W,
                             const double* D, int64_t ldw, int32_t K, const double* u, const int8_t* arm,
                             const int32_t* rows, int64_t n_patients, int32_t n_statics, int32_t n_arms,
                             const int8_t* exps, int32_t n_terms, double* G_out, double* b_out, double* mom_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  return run_weak_gram(x, ldx, layout, n_steps, W, D, ldw, K, u, arm, rows, n_patients, n_statics, n_arms, exps,
                       n_terms, G_out, b_out, mom_out, workspace, workspace_bytes, stream);
}

int32_t insite_sr3_f64(const double* G, const double* b, int64_t n_sys, int32_t n_terms, double threshold, double nu,
                       double tol, int32_t max_iter, int32_t unbias, double* coef_out, int8_t* mask_out,
                       int32_t* iters_out, void* stream) {
  if (n_sys < 0 || n_terms < 1 || !sr3_params_ok(threshold, nu, tol, max_iter)) return INSITE_E_INVALID_ARG;
  if (n_terms > INSITE_MAX_TERMS) return INSITE_E_UNSUPPORTED;
  if (n_sys == 0) return INSITE_OK;
  if (!G || !b || !coef_out) return INSITE_E_INVALID_ARG;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n_sys + kBlock - 1) / kBlock));
  switch (n_terms) {
#define INSITE_SR3_CASE(FF)                                                                                      \
  case FF:                                                                                                       \
    sr3_kernel<FF><<<grid, kBlock, 0, hs>>>(G, b, n_sys, threshold, nu, tol, max_iter, unbias, coef_out, mask_out, \
                                            iters_out);                                                          \
    break;
    INSITE_SR3_CASE(1)
    INSITE_SR3_CASE(2)
    INSITE_SR3_CASE(3)
    INSITE_SR3_CASE(4)
    INSITE_SR3_CASE(5)
    INSITE_SR3_CASE(6)
    INSITE_SR3_CASE(7)
    INSITE_SR3_CASE(8)
    INSITE_SR3_CASE(9)
#undef INSITE_SR3_CASE
    default:
      return INSITE_E_UNSUPPORTED;
  }
  return launch_status();
}

int32_t insite_sindy_fit_weak_f64(const double* x, int64_t ldx, int32_t layout, int32_t n_steps, const double* W,
                                  const double* D, int64_t ldw, int32_t K, const double* u, const int8_t* arm,
                                  const int32_t* rows, int64_t n_patients, int32_t n_statics, int32_t n_arms,
                                  const int8_t* exps, int32_t n_terms, int32_t optimizer, double threshold,
                                  double alpha, double nu, double tol, int32_t max_iter, int32_t unbias,
                                  double* G_out, double* b_out, double* coef_out, int8_t* mask_out,
                                  int32_t* iters_out, double* mom_out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (optimizer != INSITE_OPT_SR3 && optimizer != INSITE_OPT_STLSQ) return INSITE_E_INVALID_ARG;
  if (!coef_out || !sr3_params_ok(threshold, nu, tol, max_iter) || !(alpha >= 0.0)) return INSITE_E_INVALID_ARG;
  const int32_t st = run_weak_gram(x, ldx, layout, n_steps, W, D, ldw, K, u, arm, rows, n_patients, n_statics, n_arms,
                                   exps, n_terms, G_out, b_out, mom_out, workspace, workspace_bytes, stream);
  if (st != INSITE_OK || n_patients == 0) return st;
  if (optimizer == INSITE_OPT_SR3)
    return insite_sr3_f64(G_out, b_out, n_arms, n_terms, threshold, nu, tol, max_iter, unbias, coef_out, mask_out,
                          iters_out, stream);
  return insite_stlsq_f64(G_out, b_out, n_arms, n_terms, threshold, alpha, max_iter, unbias, coef_out, mask_out,
                          iters_out, stream);
}

}  // extern "C"
