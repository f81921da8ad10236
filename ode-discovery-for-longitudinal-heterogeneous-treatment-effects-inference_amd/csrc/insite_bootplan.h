// insite_bootplan.h — what the two bootstrap Gram translation units (insite_boot.hip: one arm per patient, DESIGN.md
// §9g; insite_segboot.hip: the treatment-segment path, §9o) share: the tiling of the R replicates x N patients x
// (n_arms nE) entry columns GEMM over waves, the layout of the waves' partials and their fixed-order finalisation.
// insite_common.h's convention: an anonymous namespace, each translation unit gets its own internal copy.
#pragma once
#include "insite_affine.h"

namespace {

constexpr int kBtRt = 4;               // replicate tiles per wave (3 with 5 column tiles: 256 VGPRs hold 2 waves per SIMD)
constexpr int kBtMaxCt = 5;            // column tiles per wave (n_arms nE <= 216: 14 tiles in <= 3 chunks)
constexpr int kBtWaves = 2048;         // waves the launch may have: what the machine holds (256 CUs x 4 SIMDs x 2)
constexpr size_t kBtHeader = 512;      // the ABI's zero header (this path keeps no counters in it)
constexpr int kBtFinBlock = 256;

struct BtPlan {
  int ncol, n_tiles, n_z, ct, rt, n_rg;
  int64_t n_px, rpad, cpad;
};

inline BtPlan bt_plan(int64_t N, int n_arms, int nE, int R) {
  BtPlan p;
  p.ncol = n_arms * nE;
  p.n_tiles = (p.ncol + 15) / 16;
  p.n_z = (p.n_tiles + kBtMaxCt - 1) / kBtMaxCt;
  p.ct = (p.n_tiles + p.n_z - 1) / p.n_z;
  p.rt = p.ct == kBtMaxCt ? kBtRt - 1 : kBtRt;
  p.n_rg = (R + 16 * p.rt - 1) / (16 * p.rt);
  const int64_t groups = (N + 7) / 8 + 1;  // an upper bound for every offset
  // rounded down: the launch then fits the machine in one round (1M x 1024, std7, 2 arms: 2068 waves 6.34 ms,
  // 2046 waves 5.49 ms)
  int64_t px = kBtWaves / ((int64_t)p.n_rg * p.n_z);
  if (px > groups) px = groups;
  p.n_px = px < 1 ? 1 : px;
  p.rpad = (int64_t)p.n_rg * 16 * p.rt;
  p.cpad = (int64_t)p.n_z * p.ct * 16;
  return p;
}

// thread = (replicate, entry column): the waves' partials in wave order, then the entry to G (both triangles) or b
__global__ void __launch_bounds__(kBtFinBlock)
boot_finalize_kernel(const double* __restrict__ partial, int64_t n_px, int64_t rpad, int64_t cpad, int R, int n_arms,
                     AffineGramLib lib, double* __restrict__ G, double* __restrict__ b) {
  const int ncol = n_arms * lib.nE;
  const int64_t idx = (int64_t)blockIdx.x * kBtFinBlock + threadIdx.x;
  if (idx >= (int64_t)R * ncol) return;
  const int64_t r = idx / ncol;
  const int c = (int)(idx - r * ncol);
  const double* src = partial + r * cpad + c;
  double s = 0.0;
  for (int64_t w = 0; w < n_px; ++w) s += src[w * rpad * cpad];
  const int a = c / lib.nE, e = c - a * lib.nE;
  const int i = lib.ei[e], k = lib.ek[e];
  const int64_t F = lib.F;
  const int64_t sys = r * n_arms + a;
  if (k >= 0) {
    G[(sys * F + i) * F + k] = s;
    G[(sys * F + k) * F + i] = s;
  } else {
    b[sys * F + i] = s;
  }
}

inline bool bt_solver_params_ok(double threshold, double alpha, double nu, double tol, int32_t max_iter) {
  return threshold >= 0.0 && alpha >= 0.0 && tol >= 0.0 && nu > 0.0 && max_iter >= 0;  // NaN fails every comparison
}

}  // namespace
