// insite_cohort.hip — cohort and subgroup average treatment effects over the bootstrap ensemble on MI355X (gfx950):
// include/insite_cohort.h, DESIGN.md §9i.
//
// Kernels:
//   cohort_sums_kernel     block = one wave, lane = replicate.  A block owns one 64-replicate tile, one group, one
//                          tile of 16 or 32 steps and a contiguous chunk of patients.  It reads 64 group ids at a time,
//                          takes the ballot of `group == g` and visits the set bits, so the group test is
//                          wave-uniform.  Per visited patient (its y0, u and arms loaded one patient ahead): the
//                          affine fold (insite_affine.h's replicate_fold, the one effect_bands_kernel uses, with the
//                          coefficients from LDS) and the interval maps, the lane's Poisson weight (one
//                          Threefry block per pair of global patient indices), the arms of 64 steps as ballot masks
//                          (the step's arm is a scalar bit test), then per plan and step one FMA per arm and a
//                          select; the steps of the block's tile add w y to lane-private register accumulators, the
//                          steps before it are rolled without accumulating.  No cross-lane traffic in the time
//                          loop, no atomics.  The block ends with plain vector stores of its partial [s][k][lane]
//                          to its workspace slot.
//   cohort_reduce_kernel   thread = one element of sums / wsum: the chunks' partials in chunk order.
//   cohort_finalize_kernel block = (group, step): the means of the 1 or 3 series, per series the fixed-order mean and
//                          two-pass deviation and a bitonic sort of the R_pad keys in LDS (insite_blockstats.h's
//                          co_block_series_stats, shared with policy_finalize_kernel); the host's common checks and
//                          NARM choice are insite_affine.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_blockstats.h"
#include "insite_cohort.h"

namespace {

// ---------------------------------------------------------------------------------------------
// launch plan
// ---------------------------------------------------------------------------------------------
// steps of one time tile (the register accumulators of one block): 16 where that holds every step (4 waves per SIMD),
// else 32 (2 waves per SIMD; at T = 60 a block then re-rolls 92 steps for its 60, against 156 with tiles of 16:
// DESIGN.md §9i)
#ifndef INSITE_COHORT_TT_LONG
#define INSITE_COHORT_TT_LONG 32          // A/B builds only (tools/bench_cohort_effect.py --kernel-only): 16 or 32
#endif
constexpr int kCoTtShort = 16, kCoTtLong = INSITE_COHORT_TT_LONG;
inline int co_tile(int T) { return T <= kCoTtShort ? kCoTtShort : kCoTtLong; }
constexpr int kCoArmBlock = 16;           // steps of one unrolled block of the time loop
constexpr int kCoWaves = 8192;            // waves a launch aims at: about two rounds of what the machine holds, the
                                          // long time tiles first (a tile's cost grows with its index)
constexpr size_t kCoMaxWs = ((size_t)1 << 30) - 4096;  // the workspace bound of the ABI
constexpr int kCoRedBlock = 256;
constexpr int kCoFinBlock = 256;

struct CoPlan {
  int n_rt, n_tt, tile;
  int64_t n_chunks, ppc;       // patient chunks and patients per chunk (a multiple of 64)
  int64_t slot;                // doubles of one (chunk, group, replicate tile) slot of sums: 2 T 64
  int64_t wpart_off;           // offset of the weight-sum partials, in doubles
  size_t bytes;                // 0: the shape does not fit the workspace bound
};

inline CoPlan co_plan(int64_t N, int T, int R, int G) {
  CoPlan p;
  std::memset(&p, 0, sizeof(p));
  p.n_rt = (R + kWave - 1) / kWave;
  p.tile = co_tile(T);
  p.n_tt = (int)(((int64_t)T + p.tile - 1) / p.tile);
  p.slot = (int64_t)2 * T * kWave;
  // one chunk: every (group, replicate tile) slot and its 64 weight sums
  const double per_chunk_d = (double)G * p.n_rt * (double)(p.slot + kWave) * 8.0;
  if (N < 1 || per_chunk_d > (double)kCoMaxWs) return p;
  const int64_t per_chunk = (int64_t)G * p.n_rt * (p.slot + kWave) * 8;
  const int64_t batches = (N + kWave - 1) / kWave;
  int64_t chunks = kCoWaves / ((int64_t)p.n_rt * G * p.n_tt);
  const int64_t fit = (int64_t)kCoMaxWs / per_chunk;
  if (chunks > fit) chunks = fit;
  if (chunks > batches) chunks = batches;
  if (chunks < 1) chunks = 1;
  const int64_t bpc = (batches + chunks - 1) / chunks;
  p.n_chunks = (batches + bpc - 1) / bpc;
  p.ppc = bpc * kWave;
  p.wpart_off = p.n_chunks * G * p.n_rt * p.slot;
  p.bytes = (size_t)(p.n_chunks * per_chunk);
  return p;
}

// ---------------------------------------------------------------------------------------------
// cohort_sums_kernel
// ---------------------------------------------------------------------------------------------
struct CoArgs {
  const double* y0;
  const double* u;
  const int8_t* arm_a;
  const int8_t* arm_b;  // nullptr: series A only
  const double* coef;
  const int32_t* group;  // nullptr: every row in group 0
  double* partial;
  double* wpart;
  int64_t lda, ldb, N, off, ppc, n_chunks;
  int32_t T, A, substeps, method, R, G, n_rt, poisson;
  uint32_t seed;
  double dt, drop;
};

constexpr int kCoWin = 64;  // steps whose arms one load brings in (one per lane)

// one step: the candidate of every arm, then the step's (wave-uniform) choice among the results -- NARM FMAs and
// NARM - 1 selects of one double, against 2 (NARM - 1) selects and one FMA when the map is selected first
template <int NARM>
__device__ __forceinline__ double co_step(const double (&PA)[NARM], const double (&PB)[NARM],
                                          const CoArmMask<NARM>& am, int k, double y) {
  double r = fma(PA[0], y, PB[0]);
#pragma unroll
  for (int a = 1; a < NARM; ++a) {
    const double c = fma(PA[a], y, PB[a]);
    r = ((am.m[a - 1] >> k) & 1) ? c : r;
  }
  return r;
}

// what a patient's pass reads from memory, loaded one patient ahead
struct CoRow {
  double y0, uu[INSITE_MAX_STATICS];
  int va, vb;  // lane l: the arms of step l (the first window), 0 past the steps the block rolls
};

// NSER: 1 (plan A only) or 2 plans.  Grid: x = chunk + n_chunks (rt + n_rt (g + G (n_tt - 1 - time tile))): blocks are
// dispatched in that order, the long time tiles first.
template <int TT, int NARM, int NSER>
__global__ void __launch_bounds__(kWave) cohort_sums_kernel(CoArgs ca, AffineLib lib) {
  constexpr int kCoTt = TT;
  // the replicate tile's coefficients, transposed: cs[a F + j][lane] (conflict-free column reads)
  __shared__ double cs[NARM * INSITE_MAX_TERMS * kWave];
  const int lane = threadIdx.x;
  int64_t bx = blockIdx.x;
  const int64_t chunk = bx % ca.n_chunks;
  bx /= ca.n_chunks;
  const int rt = (int)(bx % ca.n_rt);
  bx /= ca.n_rt;
  const int g = (int)(bx % ca.G);
  const int n_tt = (ca.T + kCoTt - 1) / kCoTt;
  const int tt = n_tt - 1 - (int)(bx / ca.G);
  const int r = rt * kWave + lane;
  const int t_lo = tt * kCoTt;
  const int t_hi = t_lo + kCoTt < ca.T ? t_lo + kCoTt : ca.T;  // the steps the block rolls: nothing past is read
  const double h = ca.dt / (double)ca.substeps;

  {
    const double* cb = ca.coef + (int64_t)(r < ca.R ? r : 0) * ca.A * lib.F;
    for (int a = 0; a < NARM; ++a)
      for (int j = 0; j < lib.F; ++j) cs[(a * lib.F + j) * kWave + lane] = a < ca.A ? cb[a * lib.F + j] : 0.0;
  }
  wave_lds_sync();
  int code_l = 0;  // lane j < F: the statics' exponents of term j
#pragma unroll
  for (int j = 0; j < INSITE_MAX_TERMS; ++j) code_l = lane == j ? (lib.ucode[j] & 0xffffff) : code_l;

  double acc[NSER][kCoTt];
#pragma unroll
  for (int s = 0; s < NSER; ++s)
#pragma unroll
    for (int j = 0; j < kCoTt; ++j) acc[s][j] = 0.0;
  double wacc = 0.0;
  uint64_t q_have = ~(uint64_t)0;  // the Threefry pair whose words the lane holds
  uint32_t wa = 0, wb = 0;

  const int64_t p_lo = chunk * ca.ppc;
  const int64_t p_hi = p_lo + ca.ppc < ca.N ? p_lo + ca.ppc : ca.N;
  // the rows of group g in [p_lo, p_hi), ascending: 64 group ids at a time, the ballot of `== g`, its set bits
  int64_t p0 = p_lo - kWave;
  uint64_t todo = 0;
  auto next_row = [&]() -> int64_t {
    while (todo == 0) {
      p0 += kWave;
      if (p0 >= p_hi) return -1;
      int grp = -1;
      if (p0 + lane < p_hi) grp = ca.group ? ca.group[p0 + lane] : 0;
      todo = __builtin_amdgcn_ballot_w64(grp == g);
    }
    const int64_t p = p0 + __builtin_ctzll(todo);
    todo &= todo - 1;
    return p;
  };
  auto load_arms = [&](int64_t p, int k0, int& va, int& vb) {
    va = vb = 0;
    if (k0 + lane < t_hi) {
      va = ca.arm_a[p * ca.lda + k0 + lane];
      if (NSER == 2) vb = ca.arm_b[p * ca.ldb + k0 + lane];
    }
  };
  auto load_row = [&](int64_t p) {
    CoRow row;
    row.y0 = ca.y0[p];
#pragma unroll
    for (int t = 0; t < INSITE_MAX_STATICS; ++t) row.uu[t] = t < lib.U ? ca.u[p * lib.U + t] : 0.0;
    load_arms(p, 0, row.va, row.vb);
    return row;
  };

  int64_t p = next_row();
  CoRow row;
  if (p >= 0) row = load_row(p);
  while (p >= 0) {
    // the next row's loads are in flight while this one is rolled
    const int64_t p_next = next_row();
    CoRow row_next = row;
    if (p_next >= 0) row_next = load_row(p_next);

    // ---- the lane's weight ---------------------------------------------------------------------------------
    double w = 1.0;
    if (ca.poisson) {
      const uint64_t gi = (uint64_t)(ca.off + p);
      const uint64_t q = gi >> 1;
      if (q != q_have) {  // (uniform)
        wa = (uint32_t)q;
        wb = (uint32_t)(q >> 32);
        threefry2x32_20(ca.seed, (uint32_t)r, wa, wb);
        q_have = q;
      }
      w = r == 0 ? 1.0 : (double)poisson1_weight((gi & 1) ? wb : wa);
    }
    const bool on = w != 0.0;
    wacc += w;
    // ---- prologue: the interval maps of the lane's replicate --------------------------------------------------
    // A patient's monomials are wave-uniform, so lane j computes term j once (the trip counts differ between lanes,
    // not between the terms' turns) and insite_affine.h's fold reads it back as a scalar, the coefficients from LDS
    // (all NARM arms: those past n_arms hold zeros and no step selects them).
    const double m_l = monomial_code(code_l, row.uu);
    double al[NARM], be[NARM];
    replicate_fold<NARM>(
        lib, NARM, ca.drop, [&](int a, int j) { return cs[(a * lib.F + j) * kWave + lane]; },
        [&](int j) { return readlane_f64(m_l, j); }, al, be);
    // a row the replicate did not draw rolls the zero trajectory of the zero map: a select, so that its y0 and u
    // (NaN or not) reach nothing
    double PA[NARM], PB[NARM];
    interval_map(ca.method, ca.substeps, h, al, be, PA, PB);
#pragma unroll
    for (int a = 0; a < NARM; ++a) {
      PA[a] = on ? PA[a] : 0.0;
      PB[a] = on ? PB[a] : 0.0;
    }
    double y[NSER];
#pragma unroll
    for (int s = 0; s < NSER; ++s) y[s] = on ? row.y0 : 0.0;
    CoArmMask<NARM> ma = co_arm_mask<NARM>(row.va, ca.A), mb = co_arm_mask<NARM>(row.vb, ca.A);
    auto window = [&](int k0) {  // a later window of the arms (T > 64): loaded where it starts
      if (k0 > 0 && (k0 & (kCoWin - 1)) == 0) {
        int va, vb;
        load_arms(p, k0, va, vb);
        ma = co_arm_mask<NARM>(va, ca.A);
        mb = co_arm_mask<NARM>(vb, ca.A);
      }
    };

    // ---- the steps before the tile: rolled, not accumulated (t_lo is a multiple of the 16-step block) ----------
    for (int k0 = 0; k0 < t_lo; k0 += kCoArmBlock) {
      window(k0);
      const int kb = k0 & (kCoWin - 1);
#pragma unroll
      for (int kk = 0; kk < kCoArmBlock; ++kk) {
        y[0] = co_step<NARM>(PA, PB, ma, kb + kk, y[0]);
        if (NSER == 2) y[NSER - 1] = co_step<NARM>(PA, PB, mb, kb + kk, y[NSER - 1]);
      }
    }
    // ---- the tile ----------------------------------------------------------------------------------------------
#pragma unroll
    for (int b = 0; b < kCoTt / kCoArmBlock; ++b) {
      const int k0 = t_lo + b * kCoArmBlock;
      const int nk = t_hi - k0;  // (<= 0: nothing left)
      if (nk > 0) window(k0);
      const int kb = k0 & (kCoWin - 1);
#pragma unroll
      for (int kk = 0; kk < kCoArmBlock; ++kk) {
        if (kk < nk) {  // (uniform)
          y[0] = co_step<NARM>(PA, PB, ma, kb + kk, y[0]);
          acc[0][b * kCoArmBlock + kk] = fma(w, y[0], acc[0][b * kCoArmBlock + kk]);
          if (NSER == 2) {
            y[NSER - 1] = co_step<NARM>(PA, PB, mb, kb + kk, y[NSER - 1]);
            acc[NSER - 1][b * kCoArmBlock + kk] = fma(w, y[NSER - 1], acc[NSER - 1][b * kCoArmBlock + kk]);
          }
        }
      }
    }
    p = p_next;
    row = row_next;
  }

  // ---- the block's partial: slot (chunk, g, rt), element [s][k][lane] -----------------------------------------
  const int64_t slot_i = (chunk * ca.G + g) * ca.n_rt + rt;
  double* out = ca.partial + slot_i * ((int64_t)2 * ca.T * kWave);
#pragma unroll
  for (int s = 0; s < NSER; ++s)
#pragma unroll
    for (int j = 0; j < kCoTt; ++j)
      if (t_lo + j < ca.T) out[((int64_t)s * ca.T + t_lo + j) * kWave + lane] = acc[s][j];
  if (tt == 0) ca.wpart[slot_i * kWave + lane] = wacc;
}

// thread = (g, rt, s, k, lane) of sums, then (g, rt, lane) of wsum: the chunks in chunk order
__global__ void __launch_bounds__(kCoRedBlock)
cohort_reduce_kernel(const double* __restrict__ partial, const double* __restrict__ wpart, int64_t n_chunks, int G,
                     int n_rt, int nser, int T, int R, double* __restrict__ sums, int64_t lds, double* __restrict__ wsum) {
  const int64_t idx = (int64_t)blockIdx.x * kCoRedBlock + threadIdx.x;
  const int64_t n_main = (int64_t)G * n_rt * nser * T * kWave;
  const int64_t n_w = (int64_t)G * n_rt * kWave;
  const int64_t slot = (int64_t)2 * T * kWave;
  if (idx < n_main) {
    const int lane = (int)(idx % kWave);
    int64_t e = idx / kWave;
    const int k = (int)(e % T);
    e /= T;
    const int s = (int)(e % nser);
    e /= nser;  // = g n_rt + rt
    const int rt = (int)(e % n_rt);
    const int g = (int)(e / n_rt);
    const int r = rt * kWave + lane;
    if (r >= R) return;
    const double* src = partial + e * slot + ((int64_t)s * T + k) * kWave + lane;
    double v = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) v += src[c * G * n_rt * slot];
    sums[(((int64_t)r * G + g) * nser + s) * lds + k] = v;
  } else if (idx < n_main + n_w) {
    const int64_t e = idx - n_main;
    const int lane = (int)(e % kWave);
    const int64_t gr = e / kWave;
    const int rt = (int)(gr % n_rt);
    const int g = (int)(gr / n_rt);
    const int r = rt * kWave + lane;
    if (r >= R) return;
    double v = 0.0;
    for (int64_t c = 0; c < n_chunks; ++c) v += wpart[c * n_w + e];
    wsum[(int64_t)r * G + g] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// cohort_finalize_kernel
// ---------------------------------------------------------------------------------------------
struct CoFinArgs {
  const double* sums;
  const double* wsum;
  double* out;
  int64_t lds, ldo;
  int32_t R, G, nser, T, Q, rpad;
  QuantileRank qr[INSITE_COHORT_MAX_QUANTILES];
};

// block = (group, step).  key: R_pad doubles of dynamic LDS.
__global__ void __launch_bounds__(kCoFinBlock) cohort_finalize_kernel(CoFinArgs fa) {
  extern __shared__ double key[];
  __shared__ double red[kCoFinBlock];
  const int t = threadIdx.x;
  const int k = blockIdx.x % fa.T;
  const int g = blockIdx.x / fa.T;
  const int NS = 3 + fa.Q;
  const int S = fa.nser == 2 ? 3 : 1;
  const double inf = std::numeric_limits<double>::infinity();
  for (int sv = 0; sv < S; ++sv) {
    __syncthreads();
    // the means of the series; slots R.. of the padding are +Inf
    int bad = 0;
    for (int r = t; r < fa.rpad; r += kCoFinBlock) {
      double v = inf;
      if (r < fa.R) {
        const double ws = fa.wsum[(int64_t)r * fa.G + g];
        const double* row = fa.sums + (((int64_t)r * fa.G + g) * fa.nser) * fa.lds + k;
        if (sv < 2) v = row[sv * fa.lds] / ws;
        else v = row[0] / ws - row[fa.lds] / ws;
        if (r >= 1 && v != v) bad = 1;
      }
      key[r] = v;
    }
    double* o = fa.out + (((int64_t)g * S + sv) * NS) * fa.ldo + k;
    co_block_series_stats<kCoFinBlock>(key, red, fa.R, fa.rpad, fa.Q, fa.qr, bad,
                                       [&](int i, double x) { o[i * fa.ldo] = x; });
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
bool co_groups_ok(int32_t n_groups) { return n_groups >= 1 && n_groups <= INSITE_COHORT_MAX_GROUPS; }

struct CoSumsCall {
  CoArgs ca;
  AffineLib lib;
  CoPlan plan;
  int nser;
  bool empty;  // n_rows = 0
};

// every check of the sums call, no HIP call
int32_t co_prepare_sums(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a, const int8_t* arm_b,
                        int64_t ld_arm_b, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                        int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method, int32_t substeps,
                        double drop_below, int32_t n_replicates, const int32_t* group, int32_t n_groups,
                        int32_t weighting, uint32_t seed, int64_t patient_offset, double* sums, int64_t ld_sums,
                        double* wsum, void* workspace, size_t workspace_bytes, CoSumsCall* c) {
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) || !co_groups_ok(n_groups) ||
      ld_arm_a < (int64_t)T || (arm_b && ld_arm_b < (int64_t)T) || ld_sums < (int64_t)T || patient_offset < 0 ||
      (weighting != INSITE_COHORT_WEIGHT_NONE && weighting != INSITE_COHORT_WEIGHT_POISSON))
    return INSITE_E_INVALID_ARG;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_COHORT_MAX_REPLICATES, &c->lib);
  if (st != INSITE_OK) return st;
  c->nser = arm_b ? 2 : 1;
  c->empty = n_rows == 0;
  if (c->empty) return INSITE_OK;
  if (!y0 || !arm_a || !coef || !sums || !wsum || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;
  c->plan = co_plan(n_rows, T, n_replicates, n_groups);
  if (c->plan.bytes == 0) return INSITE_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < c->plan.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return INSITE_E_INVALID_ARG;
  // blockIdx.x = chunk + n_chunks (rt + n_rt (g + G tile))
  if ((double)c->plan.n_chunks * c->plan.n_rt * n_groups * c->plan.n_tt > 2147483647.0) return INSITE_E_UNSUPPORTED;
  CoArgs& ca = c->ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.y0 = y0;
  ca.u = n_statics > 0 ? u : y0;  // never read
  ca.arm_a = arm_a;
  ca.arm_b = arm_b;
  ca.coef = coef;
  ca.group = group;
  ca.partial = static_cast<double*>(workspace);
  ca.wpart = ca.partial + c->plan.wpart_off;
  ca.lda = ld_arm_a;
  ca.ldb = arm_b ? ld_arm_b : 0;
  ca.N = n_rows;
  ca.off = patient_offset;
  ca.ppc = c->plan.ppc;
  ca.n_chunks = c->plan.n_chunks;
  ca.T = T;
  ca.A = n_arms;
  ca.substeps = substeps;
  ca.method = method;
  ca.R = n_replicates;
  ca.G = n_groups;
  ca.n_rt = c->plan.n_rt;
  ca.poisson = weighting == INSITE_COHORT_WEIGHT_POISSON;
  ca.seed = seed;
  ca.dt = dt;
  ca.drop = drop_below;
  return INSITE_OK;
}

template <int TT, int NARM>
void co_launch_sums(const CoSumsCall& c, dim3 grid, hipStream_t hs) {
  if (c.nser == 2) cohort_sums_kernel<TT, NARM, 2><<<grid, kWave, 0, hs>>>(c.ca, c.lib);
  else cohort_sums_kernel<TT, NARM, 1><<<grid, kWave, 0, hs>>>(c.ca, c.lib);
}

int32_t co_run_sums(const CoSumsCall& c, double* sums, int64_t ld_sums, double* wsum, hipStream_t hs) {
  const CoArgs& ca = c.ca;
  const dim3 grid((unsigned)(c.plan.n_chunks * c.plan.n_rt * ca.G * c.plan.n_tt));
  with_arm_slots(ca.A, [&](auto narm) {
    if (c.plan.tile == kCoTtShort) co_launch_sums<kCoTtShort, narm()>(c, grid, hs);
    else co_launch_sums<kCoTtLong, narm()>(c, grid, hs);
  });
  const int64_t n_el = (int64_t)ca.G * c.plan.n_rt * kWave * ((int64_t)c.nser * ca.T + 1);
  cohort_reduce_kernel<<<(unsigned)((n_el + kCoRedBlock - 1) / kCoRedBlock), kCoRedBlock, 0, hs>>>(
      ca.partial, ca.wpart, c.plan.n_chunks, ca.G, c.plan.n_rt, c.nser, ca.T, ca.R, sums, ld_sums, wsum);
  return launch_status();
}

// every check of the finalize call, no HIP call
int32_t co_prepare_finalize(const double* sums, int64_t ld_sums, const double* wsum, int32_t R, int32_t G,
                            int32_t n_series, int32_t T, const double* q, int32_t Q, double* out, int64_t ld_out,
                            CoFinArgs* fa) {
  if (!sums || !wsum || !out || R < 2 || G < 1 || G > INSITE_COHORT_MAX_GROUPS || (n_series != 1 && n_series != 2) ||
      T < 1 || ld_sums < (int64_t)T || ld_out < (int64_t)T ||
      check_quantiles(q, Q, INSITE_COHORT_MAX_QUANTILES) != INSITE_OK)
    return INSITE_E_INVALID_ARG;
  if (R > INSITE_COHORT_MAX_REPLICATES) return INSITE_E_UNSUPPORTED;
  std::memset(fa, 0, sizeof(*fa));
  fa->sums = sums;
  fa->wsum = wsum;
  fa->out = out;
  fa->lds = ld_sums;
  fa->ldo = ld_out;
  fa->R = R;
  fa->G = G;
  fa->nser = n_series;
  fa->T = T;
  fa->Q = Q;
  int rpad = 2;
  while (rpad < R) rpad <<= 1;
  fa->rpad = rpad;
  for (int j = 0; j < Q; ++j) fa->qr[j] = quantile_rank(q[j], R - 1);
  return INSITE_OK;
}

int32_t co_run_finalize(const CoFinArgs& fa, hipStream_t hs) {
  // G T <= 64 (2^31 - 1) blocks: past the grid's x limit the launch fails and the status says so
  const int64_t blocks = (int64_t)fa.G * fa.T;
  if (blocks > 2147483647LL) return INSITE_E_UNSUPPORTED;
  cohort_finalize_kernel<<<(unsigned)blocks, kCoFinBlock, (size_t)fa.rpad * sizeof(double), hs>>>(fa);
  return launch_status();
}

}  // namespace

extern "C" {

int32_t insite_cohort_abi_version(void) { return INSITE_COHORT_ABI_VERSION; }

size_t insite_cohort_effect_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                            int32_t n_replicates, int32_t n_groups) {
  // (no sub-steps and no dt here: 1 and 0 pass)
  if (!ensemble_shape_ok(n_rows, T, n_arms, 1, 0.0, n_replicates) || !co_groups_ok(n_groups) || n_terms < 1 ||
      n_terms > INSITE_MAX_TERMS || n_replicates > INSITE_COHORT_MAX_REPLICATES || n_rows == 0)
    return 0;
  return co_plan(n_rows, T, n_replicates, n_groups).bytes;
}

int32_t insite_cohort_effect_sums_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                      const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                      int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                      double dt, int32_t method, int32_t substeps, double drop_below,
                                      int32_t n_replicates, const int32_t* group, int32_t n_groups, int32_t weighting,
                                      uint32_t seed, int64_t patient_offset, double* sums, int64_t ld_sums,
                                      double* wsum, void* workspace, size_t workspace_bytes, void* stream) {
  CoSumsCall c;
  const int32_t st = co_prepare_sums(y0, u, arm_a, ld_arm_a, arm_b, ld_arm_b, coef, exps, n_terms, n_rows, T,
                                     n_statics, n_arms, dt, method, substeps, drop_below, n_replicates, group,
                                     n_groups, weighting, seed, patient_offset, sums, ld_sums, wsum, workspace,
                                     workspace_bytes, &c);
  if (st != INSITE_OK || c.empty) return st;
  return co_run_sums(c, sums, ld_sums, wsum, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_cohort_effect_finalize_f64(const double* sums, int64_t ld_sums, const double* wsum,
                                          int32_t n_replicates, int32_t n_groups, int32_t n_series, int32_t T,
                                          const double* q, int32_t n_quantiles, double* out, int64_t ld_out,
                                          void* stream) {
  CoFinArgs fa;
  const int32_t st = co_prepare_finalize(sums, ld_sums, wsum, n_replicates, n_groups, n_series, T, q, n_quantiles,
                                         out, ld_out, &fa);
  if (st != INSITE_OK) return st;
  return co_run_finalize(fa, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_cohort_effect_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                 const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                 int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                 double dt, int32_t method, int32_t substeps, double drop_below, int32_t n_replicates,
                                 const int32_t* group, int32_t n_groups, int32_t weighting, uint32_t seed,
                                 int64_t patient_offset, double* sums, int64_t ld_sums, double* wsum, const double* q,
                                 int32_t n_quantiles, double* out, int64_t ld_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  // the checks that need no pointer into the cohort first, so that n_rows = 0 is still validated in full
  if (check_quantiles(q, n_quantiles, INSITE_COHORT_MAX_QUANTILES) != INSITE_OK || !out || ld_out < (int64_t)T)
    return INSITE_E_INVALID_ARG;
  CoSumsCall c;
  int32_t st = co_prepare_sums(y0, u, arm_a, ld_arm_a, arm_b, ld_arm_b, coef, exps, n_terms, n_rows, T, n_statics,
                               n_arms, dt, method, substeps, drop_below, n_replicates, group, n_groups, weighting,
                               seed, patient_offset, sums, ld_sums, wsum, workspace, workspace_bytes, &c);
  if (st != INSITE_OK || c.empty) return st;
  CoFinArgs fa;
  st = co_prepare_finalize(sums, ld_sums, wsum, n_replicates, n_groups, c.nser, T, q, n_quantiles, out, ld_out, &fa);
  if (st != INSITE_OK) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  st = co_run_sums(c, sums, ld_sums, wsum, hs);
  if (st != INSITE_OK) return st;
  return co_run_finalize(fa, hs);
}

}  // extern "C"
