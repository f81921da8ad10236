// insite_affine.h — the one definition of what every translation unit of the affine libraries (state exponent
// <= INSITE_MAX_STATE_DEGREE) shares: the exponent-table checks and their packed codes, the Gram entry list, the
// quantile ranks and interpolation, the bootstrap weight stream (Threefry-2x32-20 + the Poisson(1) inverse CDF), the
// interval map of the rollout and, for the three consumers of the bootstrap ensemble, the
// replicate fold with its keep-NaN rule and the host entry points' common checks and launch plan.  Two contracts rest
// on there being one copy: DESIGN.md §9i (the cohort kernel's weight of (seed, replicate, global patient) is §9g's,
// bit for bit) and §9h (the effect and cohort trajectories are rollout's).
// insite_common.h's convention: an anonymous namespace, each translation unit gets its own internal copy.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "insite_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// library descriptors
// ---------------------------------------------------------------------------------------------
constexpr int kMaxEntries = 64;  // Gram + moment entries, one per lane
static_assert(INSITE_MAX_TERMS * (INSITE_MAX_TERMS + 1) / 2 + INSITE_MAX_TERMS <= kMaxEntries, "entry list");

struct AffineLib {
  int32_t F, U;
  int32_t ucode[INSITE_MAX_TERMS];  // column j: eu[j][0] | eu[j][1] << 8 | eu[j][2] << 16 | ex[j] << 24
};

struct AffineGramLib {
  int32_t F, U, nE;
  int32_t ucode[INSITE_MAX_TERMS];  // as AffineLib
  int8_t ei[kMaxEntries];
  int8_t ek[kMaxEntries];  // -1 => moment entry b[ei]
};

// The checks and status codes of every ABI that takes an exponent table exps[F][1 + U] (column 0: the state), and the
// table packed into ucode[F].
inline int32_t pack_exponents(const int8_t* exps, int32_t F, int32_t U, int32_t* ucode) {
  if (!exps || F < 1 || F > INSITE_MAX_TERMS || U < 0 || U > INSITE_MAX_STATICS) return INSITE_E_INVALID_ARG;
  for (int j = 0; j < F; ++j) {
    const int8_t ex = exps[j * (1 + U)];
    if (ex < 0) return INSITE_E_INVALID_ARG;
    if (ex > INSITE_MAX_STATE_DEGREE) return INSITE_E_UNSUPPORTED;
    int c = (int)ex << 24;
    for (int i = 0; i < U; ++i) {
      const int8_t e = exps[j * (1 + U) + 1 + i];
      if (e < 0 || e > 8) return INSITE_E_INVALID_ARG;
      c |= (int)e << (8 * i);
    }
    ucode[j] = c;
  }
  return INSITE_OK;
}

// The entries of one arm's system: G's upper triangle, row-major, then b.  Returns their count nE = F (F + 1) / 2 + F.
inline int32_t gram_entries(int32_t F, int8_t* ei, int8_t* ek) {
  int e = 0;
  for (int i = 0; i < F; ++i)
    for (int k = i; k < F; ++k) {
      ei[e] = (int8_t)i;
      ek[e] = (int8_t)k;
      ++e;
    }
  for (int i = 0; i < F; ++i) {
    ei[e] = (int8_t)i;
    ek[e] = -1;
    ++e;
  }
  return e;
}

inline int32_t build_affine_lib(const int8_t* exps, int32_t F, int32_t U, AffineLib* lib) {
  std::memset(lib, 0, sizeof(*lib));
  lib->F = F;
  lib->U = U;
  return pack_exponents(exps, F, U, lib->ucode);
}

inline int32_t build_affine_lib(const int8_t* exps, int32_t F, int32_t U, AffineGramLib* lib) {
  std::memset(lib, 0, sizeof(*lib));
  lib->F = F;
  lib->U = U;
  const int32_t st = pack_exponents(exps, F, U, lib->ucode);
  if (st == INSITE_OK) lib->nE = gram_entries(F, lib->ei, lib->ek);
  return st;
}

// prod_i u[i]^((code >> 8 i) & 0xff): the u-monomial of a packed column / atom code -- 1 times u[0] e0 times, then
// u[1], u[2]: every kernel multiplies in this order
__device__ __forceinline__ double monomial_code(int code, const double* u) {
  double m = 1.0;
#pragma unroll
  for (int i = 0; i < INSITE_MAX_STATICS; ++i) {
    const int e = (code >> (8 * i)) & 0xff;
    for (int k = 0; k < e; ++k) m *= u[i];
  }
  return m;
}

// ---------------------------------------------------------------------------------------------
// quantiles of n sorted keys: q -> the lower index i and the fraction g of pos = q (n - 1)
// ---------------------------------------------------------------------------------------------
// One 16-byte element: a run-time index into a separate int32 array of a kernel argument was copied to scratch.
struct QuantileRank {
  int64_t i;
  double g;
};

inline int32_t check_quantiles(const double* q, int32_t Q, int32_t max_q) {
  if (Q < 1 || Q > max_q || !q) return INSITE_E_INVALID_ARG;
  for (int j = 0; j < Q; ++j)
    if (!(q[j] >= 0.0 && q[j] <= 1.0)) return INSITE_E_INVALID_ARG;  // NaN fails both comparisons
  return INSITE_OK;
}

inline QuantileRank quantile_rank(double q, int n) {
  const double pos = q * (double)(n - 1);
  int i = (int)std::floor(pos);
  if (i > n - 1) i = n - 1;
  return QuantileRank{i, pos - (double)i};
}

// include/insite_effect.h's formula between the sorted keys lo = s[i] and hi = s[min(i + 1, n - 1)]
__device__ __forceinline__ double quantile_interp(double lo, double hi, double g) {
  return (g == 0.0 || lo == hi) ? lo : lo + g * (hi - lo);
}

// ---------------------------------------------------------------------------------------------
// weights: Threefry-2x32-20 (Salmon et al., SC'11; pinned by the Random123 known-answer vectors) and the Poisson(1)
// inverse CDF
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void threefry2x32_20(uint32_t k0, uint32_t k1, uint32_t& a, uint32_t& b) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  constexpr int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  a += ks[0];
  b += ks[1];
#pragma unroll
  for (int g = 0; g < 5; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a += b;
      b = __builtin_rotateleft32(b, R[g & 1][i]) ^ a;
    }
    a += ks[(g + 1) % 3];
    b += ks[(g + 2) % 3] + (uint32_t)(g + 1);
  }
}

// w = #{k : v >= T_k}, T_k = floor(2^32 sum_{i <= k} e^-1 / i!) (insite_bootstrap.h; tests/test_bootstrap_oracle.py
// recomputes the list)
__device__ __forceinline__ int poisson1_weight(uint32_t v) {
  constexpr uint32_t T[12] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u,
                              4294609777u, 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u};
  int w = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) w += v >= T[k] ? 1 : 0;
  return w;
}

// ---------------------------------------------------------------------------------------------
// interval map
// ---------------------------------------------------------------------------------------------
// Every library of this ABI is affine in the state (INSITE_MAX_STATE_DEGREE 1), so per arm the RHS is
// f(y) = al + be * y with al, be fixed per patient, and one observation interval of either integrator is an affine
// map y <- A y + B whose coefficients are loop invariants (the stage arithmetic of the reference scan, hoisted out
// of the time loop):
//   Euler, S substeps of h = dt/S (odeint, pkpd/utils.py:68-94): y <- (1 + h be) y + h al, S times;
//   RK4, S steps: k1..k4 of the linear RHS give y <- R(z) y + h al P(z), z = h be,
//     R = 1 + z + z^2/2 + z^3/6 + z^4/24,  P = 1 + z/2 + z^2/6 + z^3/24, composed S times.
// The time loop is then one dependent FMA per step instead of ~10 (the RK4 chain's latency, not HBM, bounded small
// cohorts: DESIGN.md §5).  Results agree with the stage-by-stage evaluation to fp64 rounding (tests: rtol 1e-11
// against the oracle's explicit stages).
__device__ __forceinline__ void interval_map(int method, int substeps, double h, double al, double be, double& A,
                                             double& B) {
  double a1, b1;
  if (method == INSITE_METHOD_EULER) {
    a1 = fma(h, be, 1.0);
    b1 = h * al;
  } else {
    const double z = h * be;
    const double P = fma(z, fma(z, fma(z, 1.0 / 24.0, 1.0 / 6.0), 0.5), 1.0);  // 1 + z/2 + z^2/6 + z^3/24
    a1 = fma(z, P, 1.0);                                                        // R = 1 + z P
    b1 = h * al * P;
  }
  A = 1.0;
  B = 0.0;
  for (int s = 0; s < substeps; ++s) {
    B = fma(a1, B, b1);
    A *= a1;
  }
}

// The same arithmetic, every arm in one pass over the sub-steps (the arms' chains interleave).  Written out, not
// built on the scalar map's single step: with a run-time method that factoring changed the register allocation of
// the kernels that call either.
template <int NARM>
__device__ __forceinline__ void interval_map(int method, int substeps, double h, const double (&al)[NARM],
                                             const double (&be)[NARM], double (&A)[NARM], double (&B)[NARM]) {
  double a1[NARM], b1[NARM];
#pragma unroll
  for (int a = 0; a < NARM; ++a) {
    if (method == INSITE_METHOD_EULER) {
      a1[a] = fma(h, be[a], 1.0);
      b1[a] = h * al[a];
    } else {
      const double z = h * be[a];
      const double P = fma(z, fma(z, fma(z, 1.0 / 24.0, 1.0 / 6.0), 0.5), 1.0);
      a1[a] = fma(z, P, 1.0);
      b1[a] = h * al[a] * P;
    }
    A[a] = 1.0;
    B[a] = 0.0;
  }
  for (int s = 0; s < substeps; ++s) {
#pragma unroll
    for (int a = 0; a < NARM; ++a) {
      B[a] = fma(a1[a], B[a], b1[a]);
      A[a] *= a1[a];
    }
  }
}

// the value of lane `src` (wave-uniform), in every lane
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const u32x2 w = __builtin_bit_cast(u32x2, v);
  u32x2 r;
  r.x = (unsigned)__builtin_amdgcn_readlane((int)w.x, src);
  r.y = (unsigned)__builtin_amdgcn_readlane((int)w.y, src);
  return __builtin_bit_cast(double, r);
}

// ---------------------------------------------------------------------------------------------
// the bootstrap ensemble (insite_effect.hip, insite_cohort.hip, insite_regimen.hip): replicate fold and maps
// ---------------------------------------------------------------------------------------------
// One replicate's RHS of every arm, f_a(y) = al[a] + be[a] y, folded over the library's terms in ascending order.
// coef(a, j): the replicate's coefficient of arm a < n_arms, term j; mono(j): the u-monomial of term j.  A dropped
// term (|c| <= drop) adds 0 and a NaN coefficient is kept (insite_effect.h); insite_hip.hip's affine_rates_regs
// drops it.
template <int NARM, class Coef, class Mono>
__device__ __forceinline__ void replicate_fold(const AffineLib& lib, int n_arms, double drop, Coef coef, Mono mono,
                                               double (&al)[NARM], double (&be)[NARM]) {
#pragma unroll
  for (int a = 0; a < NARM; ++a) al[a] = be[a] = 0.0;
#pragma unroll
  for (int j = 0; j < INSITE_MAX_TERMS; ++j) {
    if (j < lib.F) {
      const double m = mono(j);
      const bool lin = (lib.ucode[j] >> 24) != 0;
#pragma unroll
      for (int a = 0; a < NARM; ++a) {
        if (a < n_arms) {
          const double c = coef(a, j);
          const double v = (fabs(c) > drop || c != c) ? c * m : 0.0;
          if (lin) be[a] += v;
          else al[a] += v;
        }
      }
    }
  }
}

// The prologue of a wave that holds the ensemble in registers (lane l, slot s = replicate s 64 + l; a slot past R
// reads replicate 0 and is never used): the row's statics u_row, then per slot the fold and the interval map (PA, PB)
// of every arm.  coef: [R][n_arms][F].
template <int V, int NARM>
__device__ __forceinline__ void ensemble_maps(const AffineLib& lib, const double* coef, const double* u_row, int R,
                                              int n_arms, double drop, int method, int substeps, double h, int lane,
                                              double (&PA)[V][NARM], double (&PB)[V][NARM]) {
  double uu[INSITE_MAX_STATICS];
#pragma unroll
  for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? u_row[t] : 0.0;
#pragma unroll
  for (int s = 0; s < V; ++s) {
    const int r = s * kWave + lane;
    const double* cb = coef + (int64_t)(r < R ? r : 0) * n_arms * lib.F;
    double al[NARM], be[NARM];
    replicate_fold<NARM>(
        lib, n_arms, drop, [&](int a, int j) { return cb[a * lib.F + j]; },
        [&](int j) { return monomial_code(lib.ucode[j] & 0xffffff, uu); }, al, be);
#pragma unroll
    for (int a = 0; a < NARM; ++a) interval_map(method, substeps, h, al[a], be[a], PA[s][a], PB[s][a]);
  }
}

// ---------------------------------------------------------------------------------------------
// the bootstrap ensemble: what the three host entry points share
// ---------------------------------------------------------------------------------------------
inline bool ensemble_shape_ok(int64_t n_rows, int32_t T, int32_t n_arms, int32_t substeps, double dt,
                              int32_t n_replicates) {
  return n_rows >= 0 && T >= 1 && n_arms >= 1 && n_arms <= INSITE_MAX_ARMS && substeps >= 1 && dt >= 0.0 &&
         n_replicates >= 2;  // (a NaN dt fails its comparison)
}

// after the caller's INVALID_ARG checks, in the order the headers document: the method, the exponent table (packed
// into lib), the replicate cap
inline int32_t ensemble_lib(int32_t method, const int8_t* exps, int32_t n_terms, int32_t n_statics,
                            int32_t n_replicates, int32_t max_replicates, AffineLib* lib) {
  if (method != INSITE_METHOD_EULER && method != INSITE_METHOD_RK4) return INSITE_E_UNSUPPORTED;
  const int32_t st = build_affine_lib(exps, n_terms, n_statics, lib);
  if (st != INSITE_OK) return st;
  return n_replicates > max_replicates ? INSITE_E_UNSUPPORTED : INSITE_OK;
}

// wave = row: the rows one block walks, so that a launch has at most 2^20 blocks
inline int64_t rows_per_block(int64_t n_rows) {
  const int64_t blocks = n_rows < (1 << 20) ? n_rows : (1 << 20);
  return (n_rows + blocks - 1) / blocks;
}

// the register slots of a kernel instantiation: V = R_pad / 64 replicates per lane and NARM arms, handed to f as
// integral constants
inline int replicate_slots(int n_replicates) {
  return n_replicates <= 64 ? 1 : (n_replicates <= 128 ? 2 : (n_replicates <= 256 ? 4 : 8));
}
template <class F>
void with_arm_slots(int n_arms, F f) {
  if (n_arms <= 1) f(std::integral_constant<int, 1>());
  else if (n_arms <= 2) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 4>());
}
template <class F>
void with_slots(int n_replicates, int n_arms, F f) {
  with_arm_slots(n_arms, [&](auto narm) {
    const int v = replicate_slots(n_replicates);
    if (v == 1) f(std::integral_constant<int, 1>(), narm);
    else if (v == 2) f(std::integral_constant<int, 2>(), narm);
    else if (v == 4) f(std::integral_constant<int, 4>(), narm);
    else f(std::integral_constant<int, 8>(), narm);
  });
}

}  // namespace
