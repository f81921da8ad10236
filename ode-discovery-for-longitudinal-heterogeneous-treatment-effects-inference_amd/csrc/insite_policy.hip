// insite_policy.hip — the cohort value of a personalised plan choice over the bootstrap ensemble on MI355X (gfx950):
// include/insite_policy.h, DESIGN.md §9k.
//
// Kernels:
//   policy_rule_kernel     thread = row, replicate 0 only: the K objectives of the point model and their argmin, the
//                          rule when the caller gives none.
//   policy_sums_kernel     block = one wave, lane = replicate, as cohort_sums_kernel.  A block owns one 64-replicate
//                          tile, one group and a contiguous chunk of patients; it walks the rows of its group by the
//                          ballot of `group == g`.  Per visited patient (y0, u, the rule and the first window of plan
//                          0 loaded one patient ahead): one prologue -- the affine fold (insite_affine.h's
//                          replicate_fold, the coefficients from LDS), the interval maps of all arms, the lane's
//                          Poisson weight (one Threefry block per pair of global patient indices) -- then per plan the
//                          arms of 64 steps as ballot masks and the step weights in one register per lane (the next
//                          window's loads in flight while this one is rolled), per step a scalar bit test and a
//                          uniform branch, y <- A y + B and J <- w y + J; the running strict minimum and its index
//                          stay in registers.  2 K + 3 lane-private accumulators (K values, personalised, rule, K
//                          allocation counts, the weight), each updated under the weight select.  No cross-lane
//                          traffic but the read of a step's weight, no atomics.  The block ends with plain vector
//                          stores of its partial [column][lane] to its workspace slot.
//   policy_reduce_kernel   thread = one element of sums / wsum: the chunks' partials in chunk order.
//   policy_finalize_kernel block = (group, series) plus one block per group for the votes of the best fixed plan;
//                          thread = replicate forms its series value from the sums (the argmin over the K means in
//                          the thread), then insite_blockstats.h's co_block_series_stats, cohort_finalize_kernel's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_blockstats.h"
#include "insite_policy.h"

namespace {

constexpr int kPoWaves = 8192;  // waves a launch aims at: about two rounds of what the machine holds
constexpr size_t kPoMaxWs = ((size_t)1 << 30) - 4096;  // the bound of the partials
constexpr int kPoRedBlock = 256;
constexpr int kPoFinBlock = 256;
constexpr int kPoRuleBlock = 256;
constexpr int kPoWin = 64;  // steps whose arms and weights one load brings in (one per lane)

// a + b c in int64, or false when it does not fit (a, b, c >= 0)
inline bool po_mul_add(int64_t a, int64_t b, int64_t c, int64_t* out) {
  int64_t m;
  return !__builtin_mul_overflow(b, c, &m) && !__builtin_add_overflow(a, m, out);
}

struct PoPlan {
  int n_rt, cols;              // replicate tiles; columns of a slot: 2 K + 3 (the sums, then the weight)
  int64_t n_chunks, ppc;       // patient chunks and patients per chunk (a multiple of 64)
  int64_t slot;                // doubles of one (chunk, group, replicate tile) slot: cols x 64
  int64_t part_off;            // byte offset of the partials (after the rule)
  size_t bytes;                // 0: the rule and the partials together leave int64
};

inline PoPlan po_plan(int64_t N, int R, int G, int K) {
  PoPlan p;
  std::memset(&p, 0, sizeof(p));
  p.n_rt = (R + kWave - 1) / kWave;
  p.cols = 2 * K + 3;
  p.slot = (int64_t)p.cols * kWave;
  const int64_t per_chunk = (int64_t)G * p.n_rt * p.slot * 8;  // <= 64 x 64 x 35 x 64 x 8 bytes = 70 MiB
  const int64_t batches = (N + kWave - 1) / kWave;
  int64_t chunks = kPoWaves / ((int64_t)p.n_rt * G);
  const int64_t fit = (int64_t)kPoMaxWs / per_chunk;
  if (chunks > fit) chunks = fit;
  if (chunks > batches) chunks = batches;
  if (chunks < 1) chunks = 1;
  const int64_t bpc = (batches + chunks - 1) / chunks;
  p.n_chunks = (batches + bpc - 1) / bpc;
  p.ppc = bpc * kWave;
  p.part_off = ((N * 4 + 7) / 8) * 8;  // (the callers checked that 4 N + 7 fits)
  int64_t total;
  p.bytes = __builtin_add_overflow(p.part_off, p.n_chunks * per_chunk, &total) ? 0 : (size_t)total;
  return p;
}

struct PoArgs {
  const double* y0;
  const double* u;
  const int8_t* plans;
  const double* w;
  const double* cost;    // nullptr: zeros
  const double* coef;
  const int32_t* group;  // nullptr: every row in group 0
  const int32_t* rule;   // the caller's, or the workspace's
  double* partial;
  int64_t ps, ldp, ldw, N, off, ppc, n_chunks;
  int32_t T, A, K, substeps, method, R, G, n_rt, poisson;
  uint32_t seed;
  double dt, drop, sense;
};

// ---------------------------------------------------------------------------------------------
// policy_rule_kernel
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPoRuleBlock) policy_rule_kernel(PoArgs pa, AffineLib lib, int32_t* rule_ws,
                                                                   int32_t* rule_out) {
  constexpr int NA = INSITE_MAX_ARMS;
  static_assert(NA == 4, "the arm select below is written out for 4 arms");
  const int64_t p = (int64_t)blockIdx.x * kPoRuleBlock + threadIdx.x;
  if (p >= pa.N) return;
  const double h = pa.dt / (double)pa.substeps;
  double uu[INSITE_MAX_STATICS];
#pragma unroll
  for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? pa.u[p * lib.U + t] : 0.0;
  double al[NA], be[NA], PA[NA], PB[NA];
  replicate_fold<NA>(
      lib, pa.A, pa.drop, [&](int a, int j) { return pa.coef[a * lib.F + j]; },
      [&](int j) { return monomial_code(lib.ucode[j] & 0xffffff, uu); }, al, be);
  interval_map(pa.method, pa.substeps, h, al, be, PA, PB);
  const double y0 = pa.y0[p];
  double bestJ = 0.0;
  int besti = 0;
  bool abst = false;
  for (int j = 0; j < pa.K; ++j) {
    const int8_t* pl = pa.plans + (int64_t)j * pa.ps + p * pa.ldp;
    const double* wr = pa.w + p * pa.ldw;
    double y = y0, J = pa.cost ? pa.cost[j] : 0.0;
    for (int k = 0; k < pa.T; ++k) {
      int aa = pl[k];
      aa = (aa >= 1 && aa < pa.A) ? aa : 0;
      const double a_ = aa == 1 ? PA[1] : (aa == 2 ? PA[2] : (aa == 3 ? PA[3] : PA[0]));
      const double b_ = aa == 1 ? PB[1] : (aa == 2 ? PB[2] : (aa == 3 ? PB[3] : PB[0]));
      y = fma(a_, y, b_);
      J = fma(wr[k], y, J);
    }
    abst = abst || J != J;
    const bool better = j == 0 || pa.sense * J < pa.sense * bestJ;
    bestJ = better ? J : bestJ;
    besti = better ? j : besti;
  }
  const int pick = abst ? -1 : besti;
  rule_ws[p] = pick;
  if (rule_out) rule_out[p] = pick;
}

// ---------------------------------------------------------------------------------------------
// policy_sums_kernel
// ---------------------------------------------------------------------------------------------
// one interval under the step's (wave-uniform) arm: a scalar bit test and a branch, one FMA
template <int NARM>
__device__ __forceinline__ double po_step(const double (&PA)[NARM], const double (&PB)[NARM],
                                          const CoArmMask<NARM>& am, int k, double y) {
  if constexpr (NARM == 1) {
    return fma(PA[0], y, PB[0]);
  } else if constexpr (NARM == 2) {
    if ((am.m[0] >> k) & 1) return fma(PA[1], y, PB[1]);
    return fma(PA[0], y, PB[0]);
  } else {
    static_assert(NARM == 4, "1, 2 or 4 arm slots");
    if ((am.m[0] >> k) & 1) return fma(PA[1], y, PB[1]);
    if ((am.m[1] >> k) & 1) return fma(PA[2], y, PB[2]);
    if ((am.m[2] >> k) & 1) return fma(PA[3], y, PB[3]);
    return fma(PA[0], y, PB[0]);
  }
}

// what a patient's pass reads from memory before its first plan, loaded one patient ahead
struct PoRow {
  double y0, uu[INSITE_MAX_STATICS];
  int rule;   // (every lane the same)
  int va;     // lane l: the arm of step l of plan 0
  double ww;  // lane l: the weight of step l
};

// KB: the plan-count bucket (K <= KB; the plan loop is unrolled over it so that the accumulators stay in registers).
// Grid: x = chunk + n_chunks (rt + n_rt g).
template <int KB, int NARM>
__global__ void __launch_bounds__(kWave) policy_sums_kernel(PoArgs pa, AffineLib lib) {
  // the replicate tile's coefficients, transposed: cs[a F + j][lane] (conflict-free column reads)
  __shared__ double cs[NARM * INSITE_MAX_TERMS * kWave];
  const int lane = threadIdx.x;
  int64_t bx = blockIdx.x;
  const int64_t chunk = bx % pa.n_chunks;
  bx /= pa.n_chunks;
  const int rt = (int)(bx % pa.n_rt);
  const int g = (int)(bx / pa.n_rt);
  const int r = rt * kWave + lane;
  const int K = pa.K, T = pa.T;
  const double h = pa.dt / (double)pa.substeps;
  const double nan = std::numeric_limits<double>::quiet_NaN();

  {
    const double* cb = pa.coef + (int64_t)(r < pa.R ? r : 0) * pa.A * lib.F;
    for (int a = 0; a < NARM; ++a)
      for (int j = 0; j < lib.F; ++j) cs[(a * lib.F + j) * kWave + lane] = a < pa.A ? cb[a * lib.F + j] : 0.0;
  }
  wave_lds_sync();
  int code_l = 0;  // lane j < F: the statics' exponents of term j
#pragma unroll
  for (int j = 0; j < INSITE_MAX_TERMS; ++j) code_l = lane == j ? (lib.ucode[j] & 0xffffff) : code_l;

  double acc[KB], cnt[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) acc[j] = cnt[j] = 0.0;
  double acc_p = 0.0, acc_r = 0.0, wacc = 0.0;
  uint64_t q_have = ~(uint64_t)0;  // the Threefry pair whose words the lane holds
  uint32_t wa = 0, wb = 0;

  const int64_t p_lo = chunk * pa.ppc;
  const int64_t p_hi = p_lo + pa.ppc < pa.N ? p_lo + pa.ppc : pa.N;
  // the rows of group g in [p_lo, p_hi), ascending: 64 group ids at a time, the ballot of `== g`, its set bits
  int64_t p0 = p_lo - kWave;
  uint64_t todo = 0;
  auto next_row = [&]() -> int64_t {
    while (todo == 0) {
      p0 += kWave;
      if (p0 >= p_hi) return -1;
      int grp = -1;
      if (p0 + lane < p_hi) grp = pa.group ? pa.group[p0 + lane] : 0;
      todo = __builtin_amdgcn_ballot_w64(grp == g);
    }
    const int64_t p = p0 + __builtin_ctzll(todo);
    todo &= todo - 1;
    return p;
  };
  // one window of plan j: lane l reads step k0 + l (nothing past column T - 1)
  auto load_win = [&](int64_t p, int j, int k0, int& va, double& ww) {
    va = 0;
    ww = 0.0;
    if (k0 + lane < T) {
      va = pa.plans[(int64_t)j * pa.ps + p * pa.ldp + k0 + lane];
      ww = pa.w[p * pa.ldw + k0 + lane];
    }
  };
  auto load_row = [&](int64_t p) {
    PoRow row;
    row.y0 = pa.y0[p];
#pragma unroll
    for (int t = 0; t < INSITE_MAX_STATICS; ++t) row.uu[t] = t < lib.U ? pa.u[p * lib.U + t] : 0.0;
    row.rule = pa.rule[p];
    load_win(p, 0, 0, row.va, row.ww);
    return row;
  };

  int64_t p = next_row();
  PoRow row;
  if (p >= 0) row = load_row(p);
  while (p >= 0) {
    // the next row's loads are in flight while this one is rolled
    const int64_t p_next = next_row();
    PoRow row_next = row;
    if (p_next >= 0) row_next = load_row(p_next);

    // ---- the lane's row weight -------------------------------------------------------------------------------
    double om = 1.0;
    if (pa.poisson) {
      const uint64_t gi = (uint64_t)(pa.off + p);
      const uint64_t q = gi >> 1;
      if (q != q_have) {  // (uniform)
        wa = (uint32_t)q;
        wb = (uint32_t)(q >> 32);
        threefry2x32_20(pa.seed, (uint32_t)r, wa, wb);
        q_have = q;
      }
      om = r == 0 ? 1.0 : (double)poisson1_weight((gi & 1) ? wb : wa);
    }
    const bool on = om != 0.0;
    wacc += om;
    // ---- prologue, once for all K plans: the interval maps of the lane's replicate -----------------------------
    // (lane j computes the monomial of term j once; the fold reads it back as a scalar, the coefficients from LDS)
    const double m_l = monomial_code(code_l, row.uu);
    double al[NARM], be[NARM];
    replicate_fold<NARM>(
        lib, NARM, pa.drop, [&](int a, int j) { return cs[(a * lib.F + j) * kWave + lane]; },
        [&](int j) { return readlane_f64(m_l, j); }, al, be);
    double PA[NARM], PB[NARM];
    interval_map(pa.method, pa.substeps, h, al, be, PA, PB);
    const int rule_p = __builtin_amdgcn_readfirstlane(row.rule);

    // ---- the plans ------------------------------------------------------------------------------------------------
    int va = row.va;
    double ww = row.ww;
    double bestJ = 0.0, Jrule = nan;
    int besti = 0;
    bool abst = false;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < K) {  // (uniform)
        double y = row.y0;
        double J = pa.cost ? pa.cost[j] : 0.0;
        for (int k0 = 0; k0 < T; k0 += kPoWin) {
          // the window after this one: of this plan, or the first of the next
          int na = 0;
          double nw = 0.0;
          if (k0 + kPoWin < T) load_win(p, j, k0 + kPoWin, na, nw);
          else if (j + 1 < K) load_win(p, j + 1, 0, na, nw);
          const CoArmMask<NARM> am = co_arm_mask<NARM>(va, pa.A);
          const int nk = T - k0 < kPoWin ? T - k0 : kPoWin;
          for (int k = 0; k < nk; ++k) {
            const double wk = readlane_f64(ww, k);
            y = po_step<NARM>(PA, PB, am, k, y);
            J = fma(wk, y, J);
          }
          va = na;
          ww = nw;
        }
        abst = abst || J != J;
        const bool better = j == 0 || pa.sense * J < pa.sense * bestJ;
        bestJ = better ? J : bestJ;
        besti = better ? j : besti;
        // a row the replicate did not draw is left out by the select: its y0 and u (NaN or not) reach nothing
        acc[j] = on ? fma(om, J, acc[j]) : acc[j];
        Jrule = j == rule_p ? J : Jrule;  // (a scalar comparison: the row is wave-uniform)
      }
    }
    const double Jp = abst ? nan : bestJ;
    acc_p = on ? fma(om, Jp, acc_p) : acc_p;
    acc_r = on ? fma(om, Jrule, acc_r) : acc_r;
    const int vote = abst ? -1 : besti;
#pragma unroll
    for (int j = 0; j < KB; ++j) cnt[j] += (on && vote == j) ? om : 0.0;
    p = p_next;
    row = row_next;
  }

  // ---- the block's partial: slot (chunk, g, rt), element [column][lane] ----------------------------------------------
  const int64_t slot_i = (chunk * pa.G + g) * pa.n_rt + rt;
  double* out = pa.partial + slot_i * ((int64_t)(2 * K + 3) * kWave);
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < K) {
      out[j * kWave + lane] = acc[j];
      out[(K + 2 + j) * kWave + lane] = cnt[j];
    }
  out[K * kWave + lane] = acc_p;
  out[(K + 1) * kWave + lane] = acc_r;
  out[(2 * K + 2) * kWave + lane] = wacc;
}

// thread = (g, rt, column, lane): the chunks in chunk order; column 2 K + 2 is wsum
__global__ void __launch_bounds__(kPoRedBlock)
policy_reduce_kernel(const double* __restrict__ partial, int64_t n_chunks, int G, int n_rt, int K, int R,
                     double* __restrict__ sums, double* __restrict__ wsum) {
  const int cols = 2 * K + 3;
  const int64_t idx = (int64_t)blockIdx.x * kPoRedBlock + threadIdx.x;
  const int64_t n_el = (int64_t)G * n_rt * cols * kWave;
  if (idx >= n_el) return;
  const int lane = (int)(idx % kWave);
  int64_t e = idx / kWave;
  const int c = (int)(e % cols);
  e /= cols;  // = g n_rt + rt
  const int rt = (int)(e % n_rt);
  const int g = (int)(e / n_rt);
  const int r = rt * kWave + lane;
  if (r >= R) return;
  const int64_t slot = (int64_t)cols * kWave;
  const double* src = partial + e * slot + (int64_t)c * kWave + lane;
  double v = 0.0;
  for (int64_t ch = 0; ch < n_chunks; ++ch) v += src[ch * G * n_rt * slot];
  if (c < cols - 1) sums[((int64_t)r * G + g) * (cols - 1) + c] = v;
  else wsum[(int64_t)r * G + g] = v;
}

// ---------------------------------------------------------------------------------------------
// policy_finalize_kernel
// ---------------------------------------------------------------------------------------------
struct PoFinArgs {
  const double* sums;
  const double* wsum;
  double* out;
  double* fixwin;
  int32_t* best_fixed;
  int64_t ldo;
  int32_t R, G, K, Q, rpad;
  double sense;
  QuantileRank qr[INSITE_POLICY_MAX_QUANTILES];
};

// the best fixed plan of one (replicate, group): the smallest j attaining min_j s value_j; -1 if a value is NaN
__device__ __forceinline__ int po_jfix(const double* row, double ws, int K, double s, double* value) {
  double bv = 0.0;
  int bi = 0;
  bool abst = false;
  for (int j = 0; j < K; ++j) {
    const double v = row[j] / ws;
    abst = abst || v != v;
    const bool better = j == 0 || s * v < s * bv;
    bv = better ? v : bv;
    bi = better ? j : bi;
  }
  *value = abst ? std::numeric_limits<double>::quiet_NaN() : bv;
  return abst ? -1 : bi;
}

// block = (group, series 0..S-1), and series S: the votes.  key: R_pad doubles of dynamic LDS.
__global__ void __launch_bounds__(kPoFinBlock) policy_finalize_kernel(PoFinArgs fa) {
  extern __shared__ double key[];
  __shared__ double red[kPoFinBlock];
  const int t = threadIdx.x;
  const int K = fa.K;
  const int S = 2 * K + 6;
  const int sv = blockIdx.x % (S + 1);
  const int g = blockIdx.x / (S + 1);
  const int C = 2 * K + 2;
  const double s = fa.sense;
  const double inf = std::numeric_limits<double>::infinity();
  if (sv == S) {
    // the votes of the best fixed plan: jfix of every replicate into LDS, then thread j counts plan j (r ascending)
    int* jf = reinterpret_cast<int*>(key);
    for (int r = t; r < fa.R; r += kPoFinBlock) {
      double v;
      jf[r] = po_jfix(fa.sums + ((int64_t)r * fa.G + g) * C, fa.wsum[(int64_t)r * fa.G + g], K, s, &v);
    }
    __syncthreads();
    if (t < K) {
      int votes = 0;
      for (int r = 1; r < fa.R; ++r) votes += jf[r] == t ? 1 : 0;
      fa.fixwin[(int64_t)g * K + t] = (double)votes / (double)(fa.R - 1);
    }
    if (t == 0) fa.best_fixed[g] = jf[0];
    return;
  }
  // the series; slots R.. of the padding are +Inf
  int bad = 0;
  for (int r = t; r < fa.rpad; r += kPoFinBlock) {
    double v = inf;
    if (r < fa.R) {
      const double ws = fa.wsum[(int64_t)r * fa.G + g];
      const double* row = fa.sums + ((int64_t)r * fa.G + g) * C;
      if (sv <= K + 1) {
        v = row[sv] / ws;  // value_j, personalised, rule
      } else if (sv >= K + 6) {
        v = row[sv - 4] / ws;  // share_j: column K + 2 + j
      } else {
        double bf;
        po_jfix(row, ws, K, s, &bf);
        const double pers = row[K] / ws, rule = row[K + 1] / ws;
        if (sv == K + 2) v = bf;
        else if (sv == K + 3) v = s * bf - s * pers;
        else if (sv == K + 4) v = s * bf - s * rule;
        else v = s * rule - s * pers;
      }
      if (r >= 1 && v != v) bad = 1;
    }
    key[r] = v;
  }
  double* o = fa.out + ((int64_t)g * S + sv) * fa.ldo;
  co_block_series_stats<kPoFinBlock>(key, red, fa.R, fa.rpad, fa.Q, fa.qr, bad, [&](int i, double x) { o[i] = x; });
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct PoSumsCall {
  PoArgs pa;
  AffineLib lib;
  PoPlan plan;
  int32_t* rule_ws;   // where the rule kernel writes (nullptr: the caller gave the rule)
  int32_t* rule_out;
  double* sums;
  double* wsum;
  bool empty;  // n_rows = 0
};

inline bool po_sense_ok(int32_t sense) { return sense == INSITE_REGIMEN_MINIMIZE || sense == INSITE_REGIMEN_MAXIMIZE; }

// every check of the sums call, no HIP call
int32_t po_prepare_sums(const double* y0, const double* u, const int8_t* plans, int32_t n_plans, int64_t plan_stride,
                        int64_t ld_plan, const double* w, int64_t ld_w, const double* cost, int32_t sense,
                        const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T,
                        int32_t n_statics, int32_t n_arms, double dt, int32_t method, int32_t substeps,
                        double drop_below, int32_t n_replicates, const int32_t* group, int32_t n_groups,
                        int32_t weighting, uint32_t seed, int64_t patient_offset, const int32_t* rule,
                        int32_t* rule_out, double* sums, double* wsum, void* workspace, size_t workspace_bytes,
                        PoSumsCall* c) {
  int64_t top;
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) || n_groups < 1 || n_plans < 1 ||
      !po_sense_ok(sense) || patient_offset < 0 || __builtin_add_overflow(patient_offset, n_rows, &top) ||
      (weighting != INSITE_COHORT_WEIGHT_NONE && weighting != INSITE_COHORT_WEIGHT_POISSON))
    return INSITE_E_INVALID_ARG;
  // the strides: their lower bounds, and the largest element offset of every array must fit int64 (the kernels' index
  // arithmetic is int64)
  const int64_t last_row = n_rows > 0 ? n_rows - 1 : 0;
  int64_t span;
  if (ld_plan < 0 || (ld_plan != 0 && ld_plan < (int64_t)T) || plan_stride < (int64_t)T ||
      !po_mul_add(0, n_rows, ld_plan, &span) || plan_stride < span ||
      !po_mul_add((int64_t)T, (int64_t)(n_plans - 1), plan_stride, &top) || !po_mul_add(top, last_row, ld_plan, &top))
    return INSITE_E_INVALID_ARG;
  if (ld_w < 0 || (ld_w != 0 && ld_w < (int64_t)T) || !po_mul_add((int64_t)T, last_row, ld_w, &top))
    return INSITE_E_INVALID_ARG;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_POLICY_MAX_REPLICATES, &c->lib);
  if (st != INSITE_OK) return st;
  if (n_plans > INSITE_POLICY_MAX_PLANS || n_groups > INSITE_POLICY_MAX_GROUPS) return INSITE_E_UNSUPPORTED;
  c->empty = n_rows == 0;
  if (c->empty) return INSITE_OK;
  if (!y0 || !plans || !w || !coef || !sums || !wsum || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;
  if (!po_mul_add(7, n_rows, 4, &top)) return INSITE_E_INVALID_ARG;  // the rule's bytes
  c->plan = po_plan(n_rows, n_replicates, n_groups, n_plans);
  if (c->plan.bytes == 0) return INSITE_E_INVALID_ARG;
  if (!workspace || workspace_bytes < c->plan.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return INSITE_E_INVALID_ARG;
  // blockIdx.x = chunk + n_chunks (rt + n_rt g) <= 8192 + 64 x 64; the rule kernel: ceil(n_rows / 256) blocks
  if ((n_rows + kPoRuleBlock - 1) / kPoRuleBlock > 2147483647LL) return INSITE_E_UNSUPPORTED;
  PoArgs& pa = c->pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.y0 = y0;
  pa.u = n_statics > 0 ? u : y0;  // never read
  pa.plans = plans;
  pa.w = w;
  pa.cost = cost;
  pa.coef = coef;
  pa.group = group;
  c->rule_ws = rule ? nullptr : static_cast<int32_t*>(workspace);
  c->rule_out = rule_out;
  pa.rule = rule ? rule : c->rule_ws;
  pa.partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + c->plan.part_off);
  pa.ps = plan_stride;
  pa.ldp = ld_plan;
  pa.ldw = ld_w;
  pa.N = n_rows;
  pa.off = patient_offset;
  pa.ppc = c->plan.ppc;
  pa.n_chunks = c->plan.n_chunks;
  pa.T = T;
  pa.A = n_arms;
  pa.K = n_plans;
  pa.substeps = substeps;
  pa.method = method;
  pa.R = n_replicates;
  pa.G = n_groups;
  pa.n_rt = c->plan.n_rt;
  pa.poisson = weighting == INSITE_COHORT_WEIGHT_POISSON;
  pa.seed = seed;
  pa.dt = dt;
  pa.drop = drop_below;
  pa.sense = (double)sense;
  c->sums = sums;
  c->wsum = wsum;
  return INSITE_OK;
}

template <int NARM>
void po_launch_sums(const PoSumsCall& c, dim3 grid, hipStream_t hs) {
  const int K = c.pa.K;
  if (K <= 2) policy_sums_kernel<2, NARM><<<grid, kWave, 0, hs>>>(c.pa, c.lib);
  else if (K <= 4) policy_sums_kernel<4, NARM><<<grid, kWave, 0, hs>>>(c.pa, c.lib);
  else if (K <= 8) policy_sums_kernel<8, NARM><<<grid, kWave, 0, hs>>>(c.pa, c.lib);
  else policy_sums_kernel<16, NARM><<<grid, kWave, 0, hs>>>(c.pa, c.lib);
}

int32_t po_run_sums(const PoSumsCall& c, hipStream_t hs) {
  const PoArgs& pa = c.pa;
  if (c.rule_ws) {
    const unsigned blocks = (unsigned)((pa.N + kPoRuleBlock - 1) / kPoRuleBlock);
    policy_rule_kernel<<<blocks, kPoRuleBlock, 0, hs>>>(pa, c.lib, c.rule_ws, c.rule_out);
  }
  const dim3 grid((unsigned)(c.plan.n_chunks * c.plan.n_rt * pa.G));
  with_arm_slots(pa.A, [&](auto narm) { po_launch_sums<narm()>(c, grid, hs); });
  const int64_t n_el = (int64_t)pa.G * c.plan.n_rt * c.plan.cols * kWave;
  policy_reduce_kernel<<<(unsigned)((n_el + kPoRedBlock - 1) / kPoRedBlock), kPoRedBlock, 0, hs>>>(
      pa.partial, c.plan.n_chunks, pa.G, c.plan.n_rt, pa.K, pa.R, c.sums, c.wsum);
  return launch_status();
}

// every check of the finalize call, no HIP call
int32_t po_prepare_finalize(const double* sums, const double* wsum, int32_t R, int32_t G, int32_t K, int32_t sense,
                            const double* q, int32_t Q, double* out, int64_t ld_out, double* fixwin,
                            int32_t* best_fixed, PoFinArgs* fa) {
  int64_t top;
  if (!sums || !wsum || !out || !fixwin || !best_fixed || R < 2 || G < 1 || K < 1 || !po_sense_ok(sense) ||
      check_quantiles(q, Q, std::numeric_limits<int32_t>::max()) != INSITE_OK || ld_out < (int64_t)3 + Q ||
      !po_mul_add((int64_t)3 + Q, (int64_t)G * (2 * (int64_t)K + 6) - 1, ld_out, &top))
    return INSITE_E_INVALID_ARG;
  if (R > INSITE_POLICY_MAX_REPLICATES || G > INSITE_POLICY_MAX_GROUPS || K > INSITE_POLICY_MAX_PLANS ||
      Q > INSITE_POLICY_MAX_QUANTILES)
    return INSITE_E_UNSUPPORTED;
  std::memset(fa, 0, sizeof(*fa));
  fa->sums = sums;
  fa->wsum = wsum;
  fa->out = out;
  fa->fixwin = fixwin;
  fa->best_fixed = best_fixed;
  fa->ldo = ld_out;
  fa->R = R;
  fa->G = G;
  fa->K = K;
  fa->Q = Q;
  fa->sense = (double)sense;
  int rpad = 2;
  while (rpad < R) rpad <<= 1;
  fa->rpad = rpad;
  for (int j = 0; j < Q; ++j) fa->qr[j] = quantile_rank(q[j], R - 1);
  return INSITE_OK;
}

int32_t po_run_finalize(const PoFinArgs& fa, hipStream_t hs) {
  const unsigned blocks = (unsigned)(fa.G * (2 * fa.K + 7));  // <= 64 x 39
  policy_finalize_kernel<<<blocks, kPoFinBlock, (size_t)fa.rpad * sizeof(double), hs>>>(fa);
  return launch_status();
}

}  // namespace

extern "C" {

int32_t insite_policy_abi_version(void) { return INSITE_POLICY_ABI_VERSION; }

size_t insite_policy_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms, int32_t n_replicates,
                                     int32_t n_groups, int32_t n_plans) {
  // (no sub-steps and no dt here: 1 and 0 pass)
  int64_t top;
  if (!ensemble_shape_ok(n_rows, T, n_arms, 1, 0.0, n_replicates) || n_groups < 1 ||
      n_groups > INSITE_POLICY_MAX_GROUPS || n_plans < 1 || n_plans > INSITE_POLICY_MAX_PLANS || n_terms < 1 ||
      n_terms > INSITE_MAX_TERMS || n_replicates > INSITE_POLICY_MAX_REPLICATES || n_rows == 0 ||
      !po_mul_add(7, n_rows, 4, &top))
    return 0;
  return po_plan(n_rows, n_replicates, n_groups, n_plans).bytes;
}

int32_t insite_policy_sums_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                               int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w, const double* cost,
                               int32_t sense, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                               int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method,
                               int32_t substeps, double drop_below, int32_t n_replicates, const int32_t* group,
                               int32_t n_groups, int32_t weighting, uint32_t seed, int64_t patient_offset,
                               const int32_t* rule, int32_t* rule_out, double* sums, double* wsum, void* workspace,
                               size_t workspace_bytes, void* stream) {
  PoSumsCall c;
  const int32_t st = po_prepare_sums(y0, u, plans, n_plans, plan_stride, ld_plan, w, ld_w, cost, sense, coef, exps,
                                     n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below,
                                     n_replicates, group, n_groups, weighting, seed, patient_offset, rule, rule_out,
                                     sums, wsum, workspace, workspace_bytes, &c);
  if (st != INSITE_OK || c.empty) return st;
  return po_run_sums(c, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_policy_finalize_f64(const double* sums, const double* wsum, int32_t n_replicates, int32_t n_groups,
                                   int32_t n_plans, int32_t sense, const double* q, int32_t n_quantiles, double* out,
                                   int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream) {
  PoFinArgs fa;
  const int32_t st = po_prepare_finalize(sums, wsum, n_replicates, n_groups, n_plans, sense, q, n_quantiles, out,
                                         ld_out, fixwin, best_fixed, &fa);
  if (st != INSITE_OK) return st;
  return po_run_finalize(fa, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_policy_value_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                                int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w, const double* cost,
                                int32_t sense, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                                int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method,
                                int32_t substeps, double drop_below, int32_t n_replicates, const int32_t* group,
                                int32_t n_groups, int32_t weighting, uint32_t seed, int64_t patient_offset,
                                const int32_t* rule, int32_t* rule_out, double* sums, double* wsum, const double* q,
                                int32_t n_quantiles, double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed,
                                void* workspace, size_t workspace_bytes, void* stream) {
  // the finalize checks that need no pointer into the cohort first, so that n_rows = 0 is still validated in full
  // (sums and wsum may be NULL with no rows: a stand-in passes their NULL checks here, the sums call makes its own)
  static const double stand_in = 0.0;
  PoFinArgs fa;
  int32_t st = po_prepare_finalize(sums ? sums : &stand_in, wsum ? wsum : &stand_in, n_replicates, n_groups, n_plans,
                                   sense, q, n_quantiles, out, ld_out, fixwin, best_fixed, &fa);
  const int32_t st_fin = st;
  if (st == INSITE_E_INVALID_ARG) return st;
  PoSumsCall c;
  st = po_prepare_sums(y0, u, plans, n_plans, plan_stride, ld_plan, w, ld_w, cost, sense, coef, exps, n_terms, n_rows,
                       T, n_statics, n_arms, dt, method, substeps, drop_below, n_replicates, group, n_groups, weighting,
                       seed, patient_offset, rule, rule_out, sums, wsum, workspace, workspace_bytes, &c);
  if (st == INSITE_OK && st_fin != INSITE_OK) st = st_fin;  // (an invalid argument of either goes before a cap)
  if (st != INSITE_OK || c.empty) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  st = po_run_sums(c, hs);
  if (st != INSITE_OK) return st;
  return po_run_finalize(fa, hs);
}

}  // extern "C"
