// insite_rulevalue.hip — the cohort value of closed-loop treatment rules over the bootstrap ensemble on MI355X
// (gfx950): include/insite_rulevalue.h, DESIGN.md §9n.
//
// Kernels:
//   rulevalue_assign_kernel   thread = row, replicate 0 only: the K closed loops of the point model and their argmin,
//                             the assignment when the caller gives none (policy_rule_kernel's role).
//   rulevalue_sums_kernel     policy_sums_kernel's skeleton: block = one wave, lane = replicate; a block owns one
//                             64-replicate tile, one group and a contiguous chunk of patients and walks the rows of its
//                             group by the ballot of `group == g`.  Per visited patient (y0, u, the assignment, the 2 K
//                             thresholds and the first 64 step weights loaded one patient ahead, thresholds and weights
//                             one element per lane and read back by v_readlane): one prologue -- the affine fold, the
//                             interval maps of all arms, the lane's Poisson weight -- then per rule the closed loop of
//                             insite_feedback.hip at V = 1.  The arm is the lane's own, so there is no scalar branch on
//                             it: the `on` flag is per lane, a decision (k mod period == 0, a scalar countdown) compares
//                             the lane's state with the threshold its flag selects and re-selects the lane's active
//                             (A, B) and arm cost; the loop runs from decision to decision, so a step between
//                             decisions is the two FMAs of the open-loop step (with arm_cost, one add more) and the
//                             exposure is one integer add per run.  For T <= 64 the
//                             weights are loaded once per patient, not per rule.  3 K + 5 lane-private accumulators (K
//                             values, personalised, assigned, K allocation counts, K exposures, the exposures of the
//                             personalised and of the assigned rule, the weight), each updated under the weight select.
//                             No atomics; the block ends with plain vector stores of its partial [column][lane].
//   rulevalue_reduce_kernel   thread = one element of sums / wsum: the chunks' partials in chunk order.
//   rulevalue_finalize_kernel block = (group, series) plus one block per group for the votes of the best fixed rule;
//                             thread = replicate forms its series value from the sums, then insite_blockstats.h's
//                             co_block_series_stats.
//
// The closed-loop step is stated here a second time (rv_pick, rv_window).  Lifting insite_feedback.hip's fb_pick and the
// steps of a chunk of fb_closed_loop into a shared header was tried and taken back: 26 of the 48 instances of
// feedback_rules_kernel changed their register figures, so that file stays byte for byte.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_blockstats.h"
#include "insite_rulevalue.h"

namespace {

constexpr int kRvWaves = 8192;                         // waves a launch aims at (insite_policy.hip's)
constexpr size_t kRvMaxWs = ((size_t)1 << 30) - 4096;  // the bound of the partials
constexpr int kRvRedBlock = 256;
constexpr int kRvFinBlock = 256;
constexpr int kRvAsgBlock = 256;
constexpr int kRvWin = 64;  // steps whose weights one load brings in (one per lane)
static_assert(2 * INSITE_RULEVALUE_MAX_RULES <= kWave, "a row's thresholds: one per lane");

// a + b c in int64, or false when it does not fit (a, b, c >= 0)
inline bool rv_mul_add(int64_t a, int64_t b, int64_t c, int64_t* out) {
  int64_t m;
  return !__builtin_mul_overflow(b, c, &m) && !__builtin_add_overflow(a, m, out);
}

// The patient chunks: insite_policy.hip's po_plan with this call's column count.  A function of the shape alone;
// where the bound of the partials does not bind, the chunk boundaries are po_plan's.
struct RvPlan {
  int n_rt, cols;         // replicate tiles; columns of a slot: 3 K + 5 (the sums, then the weight)
  int64_t n_chunks, ppc;  // patient chunks and patients per chunk (a multiple of 64)
  int64_t slot;           // doubles of one (chunk, group, replicate tile) slot: cols x 64
  int64_t part_off;       // byte offset of the partials (after the assignment)
  size_t bytes;           // 0: the assignment and the partials together leave int64
};

inline RvPlan rv_plan(int64_t N, int R, int G, int K) {
  RvPlan p;
  std::memset(&p, 0, sizeof(p));
  p.n_rt = (R + kWave - 1) / kWave;
  p.cols = 3 * K + 5;
  p.slot = (int64_t)p.cols * kWave;
  const int64_t per_chunk = (int64_t)G * p.n_rt * p.slot * 8;  // <= 64 x 64 x 53 x 64 x 8 bytes = 106 MiB
  const int64_t batches = (N + kWave - 1) / kWave;
  int64_t chunks = kRvWaves / ((int64_t)p.n_rt * G);
  const int64_t fit = (int64_t)kRvMaxWs / per_chunk;
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

struct RvArgs {
  const double* y0;
  const double* u;
  const double* theta;
  const double* w;
  const double* cost;     // nullptr: zeros
  const double* coef;
  const int32_t* group;   // nullptr: every row in group 0
  const int32_t* assign;  // the caller's, or the workspace's
  double* partial;
  int64_t ldt, ldw, N, off, ppc, n_chunks;
  int32_t T, A, K, substeps, method, R, G, n_rt, poisson;
  uint32_t seed;
  double dt, drop, sense;
};

// One 8-byte element, indexed by the (wave-uniform) rule: code = arm_on | arm_off << 8 | start_on << 16.
struct RvRule {
  int32_t code, period;
};

// The host tables, a kernel argument of their own (insite_feedback.hip found that inside the argument struct they
// leave dead SGPR spill slots and a private segment no instruction uses).
struct RvTables {
  double ac[INSITE_MAX_ARMS];  // arm_cost (the AC instantiations)
  RvRule rule[INSITE_RULEVALUE_MAX_RULES];
};

// v[a] for a wave-uniform arm a in 0..NARM-1: selects between compile-time indices (the maps stay in registers)
template <int NARM>
__device__ __forceinline__ double rv_pick(const double (&v)[NARM], int a) {
  if constexpr (NARM == 1) {
    return v[0];
  } else if constexpr (NARM == 2) {
    return a == 1 ? v[1] : v[0];
  } else {
    const double lo = (a & 1) ? v[1] : v[0], hi = (a & 1) ? v[3] : v[2];
    return (a & 2) ? hi : lo;
  }
}

// The state of one closed loop: the flag, the active map and arm cost, the steps until the next decision.
struct RvLoop {
  bool on;
  double Aa, Ba, ca;
  int cd;  // (wave-uniform)
};

// The nk steps of one window of the closed loop of insite_feedback.h for one replicate; ww: lane i holds the weight
// of the window's step i.  The interval runs under (A1, B1) where (on ? hi_on : hi_off) holds and under (A0, B0)
// otherwise (hi_on, hi_off: wave-uniform).  SEL false: one map only.  The loop runs from decision to decision: a
// decision (one ordered comparison of the state before the interval, NaN: off) re-selects the active map and arm cost,
// then the steps up to the next decision (or the window's end) are the open-loop step -- two FMAs and, with AC, one
// add -- and the exposure is added once per run.  The operations on y and J and their order are fb_closed_loop's.
template <bool SEL, bool AC>
__device__ __forceinline__ void rv_window(RvLoop& st, int period, bool hi_on, bool hi_off, double ton, double toff,
                                          double c_on, double c_off, double ww, int nk, double A1, double B1, double A0,
                                          double B0, double& y, double& J, int& E) {
  int k = 0;
  while (k < nk) {
    if (st.cd == 0) {
      const double thr = st.on ? toff : ton;
      st.on = y >= thr;
      if constexpr (SEL) {
        const bool hi = st.on ? hi_on : hi_off;
        st.Aa = hi ? A1 : A0;
        st.Ba = hi ? B1 : B0;
      }
      if constexpr (AC) st.ca = st.on ? c_on : c_off;
      st.cd = period;
    }
    const int run = st.cd < nk - k ? st.cd : nk - k;  // (wave-uniform) the steps until the next decision
    for (int i = 0; i < run; ++i) {
      const double wk = readlane_f64(ww, k + i);
      y = fma(st.Aa, y, st.Ba);
      J = fma(wk, y, J);
      if constexpr (AC) J = J + st.ca;
    }
    E += st.on ? run : 0;
    st.cd -= run;
    k += run;
  }
}

// what a rule's loop needs of its host row and of the replicate's maps
template <int NARM>
struct RvRuleMaps {
  double A1, B1, A0, B0;
  bool hi_on, hi_off;
};

template <int NARM>
__device__ __forceinline__ RvRuleMaps<NARM> rv_rule_maps(const double (&PA)[NARM], const double (&PB)[NARM],
                                                        int arm_on, int arm_off) {
  RvRuleMaps<NARM> m;
  if constexpr (NARM <= 2) {
    // the arms' own maps: arm 1 where (on ? arm_on : arm_off) is 1
    m.A1 = PA[NARM - 1];
    m.B1 = PB[NARM - 1];
    m.A0 = PA[0];
    m.B0 = PB[0];
    m.hi_on = arm_on == 1;
    m.hi_off = arm_off == 1;
  } else {
    m.A1 = rv_pick<NARM>(PA, arm_on);
    m.B1 = rv_pick<NARM>(PB, arm_on);
    m.A0 = rv_pick<NARM>(PA, arm_off);
    m.B0 = rv_pick<NARM>(PB, arm_off);
    m.hi_on = true;
    m.hi_off = false;
  }
  return m;
}

// ---------------------------------------------------------------------------------------------
// rulevalue_assign_kernel
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRvAsgBlock) rulevalue_assign_kernel(RvArgs ra, RvTables tb, AffineLib lib,
                                                                       int has_ac, int32_t* assign_ws,
                                                                       int32_t* assign_out) {
  constexpr int NA = INSITE_MAX_ARMS;
  const int64_t p = (int64_t)blockIdx.x * kRvAsgBlock + threadIdx.x;
  if (p >= ra.N) return;
  const double h = ra.dt / (double)ra.substeps;
  double uu[INSITE_MAX_STATICS];
#pragma unroll
  for (int t = 0; t < INSITE_MAX_STATICS; ++t) uu[t] = t < lib.U ? ra.u[p * lib.U + t] : 0.0;
  double al[NA], be[NA], PA[NA], PB[NA];
  replicate_fold<NA>(
      lib, ra.A, ra.drop, [&](int a, int j) { return ra.coef[a * lib.F + j]; },
      [&](int j) { return monomial_code(lib.ucode[j] & 0xffffff, uu); }, al, be);
  interval_map(ra.method, ra.substeps, h, al, be, PA, PB);
  const double y0 = ra.y0[p];
  const double* wr = ra.w + p * ra.ldw;
  const double* th = ra.theta + p * ra.ldt;
  double bestJ = 0.0;
  int besti = 0;
  bool abst = false;
  for (int j = 0; j < ra.K; ++j) {
    const RvRule rl = tb.rule[j];
    const int arm_on = rl.code & 0xff, arm_off = (rl.code >> 8) & 0xff;
    const double ton = th[2 * j], toff = th[2 * j + 1];
    const double A1 = rv_pick<NA>(PA, arm_on), B1 = rv_pick<NA>(PB, arm_on);
    const double A0 = rv_pick<NA>(PA, arm_off), B0 = rv_pick<NA>(PB, arm_off);
    const double c_on = rv_pick<NA>(tb.ac, arm_on), c_off = rv_pick<NA>(tb.ac, arm_off);
    double y = y0, J = ra.cost ? ra.cost[j] : 0.0;
    bool on = (rl.code >> 16) != 0;
    int cd = 0;
    for (int k = 0; k < ra.T; ++k) {
      if (cd == 0) {
        on = y >= (on ? toff : ton);
        cd = rl.period;
      }
      --cd;
      y = fma(on ? A1 : A0, y, on ? B1 : B0);
      J = fma(wr[k], y, J);
      if (has_ac) J = J + (on ? c_on : c_off);
    }
    abst = abst || J != J;
    const bool better = j == 0 || ra.sense * J < ra.sense * bestJ;
    bestJ = better ? J : bestJ;
    besti = better ? j : besti;
  }
  const int pick = abst ? -1 : besti;
  assign_ws[p] = pick;
  if (assign_out) assign_out[p] = pick;
}

// ---------------------------------------------------------------------------------------------
// rulevalue_sums_kernel
// ---------------------------------------------------------------------------------------------
// what a patient's pass reads from memory before its first rule, loaded one patient ahead
struct RvRow {
  double y0, uu[INSITE_MAX_STATICS];
  int assign;  // (every lane the same)
  double th;   // lane l < 2 K: threshold l of the row (theta_on of rule l / 2, then its theta_off)
  double ww;   // lane l: the weight of step l
};

// KB: the rule-count bucket (K <= KB; the rule loop is unrolled over it so that the accumulators stay in registers);
// AC: the per-step arm cost is added.  Grid: x = chunk + n_chunks (rt + n_rt g).
template <int KB, int NARM, bool AC>
__global__ void __launch_bounds__(kWave) rulevalue_sums_kernel(RvArgs ra, RvTables tb, AffineLib lib) {
  // the replicate tile's coefficients, transposed: cs[a F + j][lane] (conflict-free column reads)
  __shared__ double cs[NARM * INSITE_MAX_TERMS * kWave];
  const int lane = threadIdx.x;
  int64_t bx = blockIdx.x;
  const int64_t chunk = bx % ra.n_chunks;
  bx /= ra.n_chunks;
  const int rt = (int)(bx % ra.n_rt);
  const int g = (int)(bx / ra.n_rt);
  const int r = rt * kWave + lane;
  const int K = ra.K, T = ra.T;
  const double h = ra.dt / (double)ra.substeps;
  const double nan = std::numeric_limits<double>::quiet_NaN();

  {
    const double* cb = ra.coef + (int64_t)(r < ra.R ? r : 0) * ra.A * lib.F;
    for (int a = 0; a < NARM; ++a)
      for (int j = 0; j < lib.F; ++j) cs[(a * lib.F + j) * kWave + lane] = a < ra.A ? cb[a * lib.F + j] : 0.0;
  }
  wave_lds_sync();
  int code_l = 0;  // lane j < F: the statics' exponents of term j
#pragma unroll
  for (int j = 0; j < INSITE_MAX_TERMS; ++j) code_l = lane == j ? (lib.ucode[j] & 0xffffff) : code_l;

  double acc[KB], cnt[KB], ex[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) acc[j] = cnt[j] = ex[j] = 0.0;
  double acc_p = 0.0, acc_a = 0.0, ex_p = 0.0, ex_a = 0.0, wacc = 0.0;
  uint64_t q_have = ~(uint64_t)0;  // the Threefry pair whose words the lane holds
  uint32_t wa = 0, wb = 0;

  const int64_t p_lo = chunk * ra.ppc;
  const int64_t p_hi = p_lo + ra.ppc < ra.N ? p_lo + ra.ppc : ra.N;
  // the rows of group g in [p_lo, p_hi), ascending: 64 group ids at a time, the ballot of `== g`, its set bits
  int64_t p0 = p_lo - kWave;
  uint64_t todo = 0;
  auto next_row = [&]() -> int64_t {
    while (todo == 0) {
      p0 += kWave;
      if (p0 >= p_hi) return -1;
      int grp = -1;
      if (p0 + lane < p_hi) grp = ra.group ? ra.group[p0 + lane] : 0;
      todo = __builtin_amdgcn_ballot_w64(grp == g);
    }
    const int64_t p = p0 + __builtin_ctzll(todo);
    todo &= todo - 1;
    return p;
  };
  // one window of the row's weights: lane l reads step k0 + l (nothing past column T - 1)
  auto load_win = [&](int64_t p, int k0) {
    double ww = 0.0;
    if (k0 + lane < T) ww = ra.w[p * ra.ldw + k0 + lane];
    return ww;
  };
  auto load_row = [&](int64_t p) {
    RvRow row;
    row.y0 = ra.y0[p];
#pragma unroll
    for (int t = 0; t < INSITE_MAX_STATICS; ++t) row.uu[t] = t < lib.U ? ra.u[p * lib.U + t] : 0.0;
    row.assign = ra.assign[p];
    row.th = 0.0;
    if (lane < 2 * K) row.th = ra.theta[p * ra.ldt + lane];  // (nothing past column 2 K - 1)
    row.ww = load_win(p, 0);
    return row;
  };

  int64_t p = next_row();
  RvRow row;
  if (p >= 0) row = load_row(p);
  while (p >= 0) {
    // the next row's loads are in flight while this one is rolled
    const int64_t p_next = next_row();
    RvRow row_next = row;
    if (p_next >= 0) row_next = load_row(p_next);

    // ---- the lane's row weight -------------------------------------------------------------------------------
    double om = 1.0;
    if (ra.poisson) {
      const uint64_t gi = (uint64_t)(ra.off + p);
      const uint64_t q = gi >> 1;
      if (q != q_have) {  // (uniform)
        wa = (uint32_t)q;
        wb = (uint32_t)(q >> 32);
        threefry2x32_20(ra.seed, (uint32_t)r, wa, wb);
        q_have = q;
      }
      om = r == 0 ? 1.0 : (double)poisson1_weight((gi & 1) ? wb : wa);
    }
    const bool live = om != 0.0;
    wacc += om;
    // ---- prologue, once for all K rules: the interval maps of the lane's replicate -----------------------------
    // (lane j computes the monomial of term j once; the fold reads it back as a scalar, the coefficients from LDS)
    const double m_l = monomial_code(code_l, row.uu);
    double al[NARM], be[NARM];
    replicate_fold<NARM>(
        lib, NARM, ra.drop, [&](int a, int j) { return cs[(a * lib.F + j) * kWave + lane]; },
        [&](int j) { return readlane_f64(m_l, j); }, al, be);
    double PA[NARM], PB[NARM];
    interval_map(ra.method, ra.substeps, h, al, be, PA, PB);
    const int asg = __builtin_amdgcn_readfirstlane(row.assign);

    // ---- the rules ------------------------------------------------------------------------------------------------
    double bestJ = 0.0, bestE = 0.0, Jasg = nan, Easg = nan;
    int besti = 0;
    bool abst = false;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < K) {  // (uniform)
        const RvRule rl = tb.rule[j];
        const int arm_on = rl.code & 0xff, arm_off = (rl.code >> 8) & 0xff;
        const double ton = readlane_f64(row.th, 2 * j), toff = readlane_f64(row.th, 2 * j + 1);
        const double c_on = AC ? rv_pick<INSITE_MAX_ARMS>(tb.ac, arm_on) : 0.0;
        const double c_off = AC ? rv_pick<INSITE_MAX_ARMS>(tb.ac, arm_off) : 0.0;
        const RvRuleMaps<NARM> mp = rv_rule_maps<NARM>(PA, PB, arm_on, arm_off);
        double y = row.y0;
        double J = ra.cost ? ra.cost[j] : 0.0;
        int E = 0;
        RvLoop st;
        st.on = (rl.code >> 16) != 0;
        st.Aa = mp.A0;  // step 0 is a decision step: set there
        st.Ba = mp.B0;
        st.ca = 0.0;
        st.cd = 0;
        double ww = row.ww;  // window 0 came with the row: for T <= 64 no rule reloads a weight
        for (int k0 = 0; k0 < T; k0 += kRvWin) {
          double nw = 0.0;  // the window after this one, in flight while this one is rolled
          if (k0 + kRvWin < T) nw = load_win(p, k0 + kRvWin);
          const int nk = T - k0 < kRvWin ? T - k0 : kRvWin;
          rv_window<(NARM > 1), AC>(st, rl.period, mp.hi_on, mp.hi_off, ton, toff, c_on, c_off, ww, nk, mp.A1, mp.B1, mp.A0,
                                    mp.B0, y, J, E);
          ww = nw;
        }
        // the exposure: an exact count; NaN where the trajectory is (a NaN state stays NaN: the last one tells)
        const double Ev = y != y ? nan : (double)E;
        abst = abst || J != J;
        const bool better = j == 0 || ra.sense * J < ra.sense * bestJ;
        bestJ = better ? J : bestJ;
        bestE = better ? Ev : bestE;
        besti = better ? j : besti;
        // a row the replicate did not draw is left out by the select: its y0, u and theta (NaN or not) reach nothing
        acc[j] = live ? fma(om, J, acc[j]) : acc[j];
        ex[j] = live ? fma(om, Ev, ex[j]) : ex[j];
        Jasg = j == asg ? J : Jasg;  // (a scalar comparison: the row is wave-uniform)
        Easg = j == asg ? Ev : Easg;
      }
    }
    const double Jp = abst ? nan : bestJ;
    const double Ep = abst ? nan : bestE;
    acc_p = live ? fma(om, Jp, acc_p) : acc_p;
    acc_a = live ? fma(om, Jasg, acc_a) : acc_a;
    ex_p = live ? fma(om, Ep, ex_p) : ex_p;
    ex_a = live ? fma(om, Easg, ex_a) : ex_a;
    const int vote = abst ? -1 : besti;
#pragma unroll
    for (int j = 0; j < KB; ++j) cnt[j] += (live && vote == j) ? om : 0.0;
    p = p_next;
    row = row_next;
  }

  // ---- the block's partial: slot (chunk, g, rt), element [column][lane] ----------------------------------------------
  const int64_t slot_i = (chunk * ra.G + g) * ra.n_rt + rt;
  double* out = ra.partial + slot_i * ((int64_t)(3 * K + 5) * kWave);
#pragma unroll
  for (int j = 0; j < KB; ++j)
    if (j < K) {
      out[j * kWave + lane] = acc[j];
      out[(K + 2 + j) * kWave + lane] = cnt[j];
      out[(2 * K + 2 + j) * kWave + lane] = ex[j];
    }
  out[K * kWave + lane] = acc_p;
  out[(K + 1) * kWave + lane] = acc_a;
  out[(3 * K + 2) * kWave + lane] = ex_p;
  out[(3 * K + 3) * kWave + lane] = ex_a;
  out[(3 * K + 4) * kWave + lane] = wacc;
}

// thread = (g, rt, column, lane): the chunks in chunk order; column 3 K + 4 is wsum
__global__ void __launch_bounds__(kRvRedBlock)
rulevalue_reduce_kernel(const double* __restrict__ partial, int64_t n_chunks, int G, int n_rt, int K, int R,
                        double* __restrict__ sums, double* __restrict__ wsum) {
  const int cols = 3 * K + 5;
  const int64_t idx = (int64_t)blockIdx.x * kRvRedBlock + threadIdx.x;
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
// rulevalue_finalize_kernel
// ---------------------------------------------------------------------------------------------
struct RvFinArgs {
  const double* sums;
  const double* wsum;
  double* out;
  double* fixwin;
  int32_t* best_fixed;
  int64_t ldo;
  int32_t R, G, K, Q, rpad;
  double sense;
  QuantileRank qr[INSITE_RULEVALUE_MAX_QUANTILES];
};

// the best fixed rule of one (replicate, group): the smallest j attaining min_j s value_j; -1 if a value is NaN
__device__ __forceinline__ int rv_jfix(const double* row, double ws, int K, double s, double* value) {
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
__global__ void __launch_bounds__(kRvFinBlock) rulevalue_finalize_kernel(RvFinArgs fa) {
  extern __shared__ double key[];
  __shared__ double red[kRvFinBlock];
  const int t = threadIdx.x;
  const int K = fa.K;
  const int S = 3 * K + 9;
  const int sv = blockIdx.x % (S + 1);
  const int g = blockIdx.x / (S + 1);
  const int C = 3 * K + 4;
  const double s = fa.sense;
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (sv == S) {
    // the votes of the best fixed rule: jfix of every replicate into LDS, then thread j counts rule j (r ascending)
    int* jf = reinterpret_cast<int*>(key);
    for (int r = t; r < fa.R; r += kRvFinBlock) {
      double v;
      jf[r] = rv_jfix(fa.sums + ((int64_t)r * fa.G + g) * C, fa.wsum[(int64_t)r * fa.G + g], K, s, &v);
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
  for (int r = t; r < fa.rpad; r += kRvFinBlock) {
    double v = inf;
    if (r < fa.R) {
      const double ws = fa.wsum[(int64_t)r * fa.G + g];
      const double* row = fa.sums + ((int64_t)r * fa.G + g) * C;
      if (sv <= K + 1) {
        v = row[sv] / ws;  // value_j, personalised, assigned
      } else if (sv >= K + 6 && sv <= 3 * K + 7) {
        v = row[sv - 4] / ws;  // share_j, exposure_j, exposure_personalised, exposure_assigned: column sv - 4
      } else {
        double bf;
        const int jf = rv_jfix(row, ws, K, s, &bf);
        const double pers = row[K] / ws, asg = row[K + 1] / ws;
        if (sv == K + 2) v = bf;
        else if (sv == K + 3) v = s * bf - s * pers;
        else if (sv == K + 4) v = s * bf - s * asg;
        else if (sv == K + 5) v = s * asg - s * pers;
        else v = jf >= 0 ? row[2 * K + 2 + jf] / ws : nan;  // exposure_best_fixed
      }
      if (r >= 1 && v != v) bad = 1;
    }
    key[r] = v;
  }
  double* o = fa.out + ((int64_t)g * S + sv) * fa.ldo;
  co_block_series_stats<kRvFinBlock>(key, red, fa.R, fa.rpad, fa.Q, fa.qr, bad, [&](int i, double x) { o[i] = x; });
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct RvSumsCall {
  RvArgs ra;
  RvTables tb;
  AffineLib lib;
  RvPlan plan;
  int32_t* assign_ws;  // where the assign kernel writes (nullptr: the caller gave the assignment)
  int32_t* assign_out;
  double* sums;
  double* wsum;
  bool ac;     // arm_cost given
  bool empty;  // n_rows = 0
};

inline bool rv_sense_ok(int32_t sense) { return sense == INSITE_FEEDBACK_MINIMIZE || sense == INSITE_FEEDBACK_MAXIMIZE; }

// every check of the sums call, no HIP call
int32_t rv_prepare_sums(const double* y0, const double* u, const double* theta, int64_t ld_theta, const int32_t* rules,
                        int32_t n_rules, const double* w, int64_t ld_w, const double* cost, const double* arm_cost,
                        int32_t sense, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                        int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method, int32_t substeps,
                        double drop_below, int32_t n_replicates, const int32_t* group, int32_t n_groups,
                        int32_t weighting, uint32_t seed, int64_t patient_offset, const int32_t* assign,
                        int32_t* assign_out, void* workspace, size_t workspace_bytes, double* sums, double* wsum,
                        RvSumsCall* c) {
  int64_t top;
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) || n_groups < 1 || n_rules < 1 || !rules ||
      !rv_sense_ok(sense) || patient_offset < 0 || __builtin_add_overflow(patient_offset, n_rows, &top) ||
      (weighting != INSITE_COHORT_WEIGHT_NONE && weighting != INSITE_COHORT_WEIGHT_POISSON))
    return INSITE_E_INVALID_ARG;
  for (int64_t j = 0; j < n_rules; ++j) {
    const int32_t* r = rules + 4 * j;
    if (r[0] < 0 || r[0] >= n_arms || r[1] < 0 || r[1] >= n_arms || r[2] < 1 || (r[3] != 0 && r[3] != 1))
      return INSITE_E_INVALID_ARG;
  }
  // the leading dimensions: their lower bounds, and the largest element offset of every array must fit int64 (the
  // kernels' index arithmetic is int64)
  const int64_t last_row = n_rows > 0 ? n_rows - 1 : 0;
  if (ld_theta < 0 || (ld_theta != 0 && ld_theta < 2 * (int64_t)n_rules) ||
      !rv_mul_add(2 * (int64_t)n_rules, last_row, ld_theta, &top))
    return INSITE_E_INVALID_ARG;
  if (ld_w < 0 || (ld_w != 0 && ld_w < (int64_t)T) || !rv_mul_add((int64_t)T, last_row, ld_w, &top))
    return INSITE_E_INVALID_ARG;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_RULEVALUE_MAX_REPLICATES, &c->lib);
  if (st != INSITE_OK) return st;
  if (n_rules > INSITE_RULEVALUE_MAX_RULES || n_groups > INSITE_RULEVALUE_MAX_GROUPS) return INSITE_E_UNSUPPORTED;
  c->empty = n_rows == 0;
  if (c->empty) return INSITE_OK;
  if (!y0 || !theta || !w || !coef || !sums || !wsum || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;
  if (!rv_mul_add(7, n_rows, 4, &top)) return INSITE_E_INVALID_ARG;  // the assignment's bytes
  c->plan = rv_plan(n_rows, n_replicates, n_groups, n_rules);
  if (c->plan.bytes == 0) return INSITE_E_INVALID_ARG;
  if (!workspace || workspace_bytes < c->plan.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return INSITE_E_INVALID_ARG;
  // blockIdx.x = chunk + n_chunks (rt + n_rt g) <= 8192 + 64 x 64; the assign kernel: ceil(n_rows / 256) blocks
  if ((n_rows + kRvAsgBlock - 1) / kRvAsgBlock > 2147483647LL) return INSITE_E_UNSUPPORTED;
  RvArgs& ra = c->ra;
  std::memset(&ra, 0, sizeof(ra));
  std::memset(&c->tb, 0, sizeof(c->tb));
  ra.y0 = y0;
  ra.u = n_statics > 0 ? u : y0;  // never read
  ra.theta = theta;
  ra.w = w;
  ra.cost = cost;
  ra.coef = coef;
  ra.group = group;
  c->assign_ws = assign ? nullptr : static_cast<int32_t*>(workspace);
  c->assign_out = assign_out;
  ra.assign = assign ? assign : c->assign_ws;
  ra.partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + c->plan.part_off);
  ra.ldt = ld_theta;
  ra.ldw = ld_w;
  ra.N = n_rows;
  ra.off = patient_offset;
  ra.ppc = c->plan.ppc;
  ra.n_chunks = c->plan.n_chunks;
  ra.T = T;
  ra.A = n_arms;
  ra.K = n_rules;
  ra.substeps = substeps;
  ra.method = method;
  ra.R = n_replicates;
  ra.G = n_groups;
  ra.n_rt = c->plan.n_rt;
  ra.poisson = weighting == INSITE_COHORT_WEIGHT_POISSON;
  ra.seed = seed;
  ra.dt = dt;
  ra.drop = drop_below;
  ra.sense = (double)sense;
  c->ac = arm_cost != nullptr;
  for (int a = 0; a < n_arms; ++a) c->tb.ac[a] = arm_cost ? arm_cost[a] : 0.0;
  for (int j = 0; j < n_rules; ++j)
    c->tb.rule[j] = RvRule{rules[4 * j] | rules[4 * j + 1] << 8 | rules[4 * j + 3] << 16, rules[4 * j + 2]};
  c->sums = sums;
  c->wsum = wsum;
  return INSITE_OK;
}

template <int NARM, bool AC>
void rv_launch_sums(const RvSumsCall& c, dim3 grid, hipStream_t hs) {
  const int K = c.ra.K;
  if (K <= 2) rulevalue_sums_kernel<2, NARM, AC><<<grid, kWave, 0, hs>>>(c.ra, c.tb, c.lib);
  else if (K <= 4) rulevalue_sums_kernel<4, NARM, AC><<<grid, kWave, 0, hs>>>(c.ra, c.tb, c.lib);
  else if (K <= 8) rulevalue_sums_kernel<8, NARM, AC><<<grid, kWave, 0, hs>>>(c.ra, c.tb, c.lib);
  else rulevalue_sums_kernel<16, NARM, AC><<<grid, kWave, 0, hs>>>(c.ra, c.tb, c.lib);
}

int32_t rv_run_sums(const RvSumsCall& c, hipStream_t hs) {
  const RvArgs& ra = c.ra;
  if (c.assign_ws) {
    const unsigned blocks = (unsigned)((ra.N + kRvAsgBlock - 1) / kRvAsgBlock);
    rulevalue_assign_kernel<<<blocks, kRvAsgBlock, 0, hs>>>(ra, c.tb, c.lib, c.ac ? 1 : 0, c.assign_ws, c.assign_out);
  }
  const dim3 grid((unsigned)(c.plan.n_chunks * c.plan.n_rt * ra.G));
  with_arm_slots(ra.A, [&](auto narm) {
    if (c.ac) rv_launch_sums<narm(), true>(c, grid, hs);
    else rv_launch_sums<narm(), false>(c, grid, hs);
  });
  const int64_t n_el = (int64_t)ra.G * c.plan.n_rt * c.plan.cols * kWave;
  rulevalue_reduce_kernel<<<(unsigned)((n_el + kRvRedBlock - 1) / kRvRedBlock), kRvRedBlock, 0, hs>>>(
      ra.partial, c.plan.n_chunks, ra.G, c.plan.n_rt, ra.K, ra.R, c.sums, c.wsum);
  return launch_status();
}

// every check of the finalize call, no HIP call
int32_t rv_prepare_finalize(const double* sums, const double* wsum, int32_t R, int32_t G, int32_t K, int32_t sense,
                            const double* q, int32_t Q, double* out, int64_t ld_out, double* fixwin,
                            int32_t* best_fixed, RvFinArgs* fa) {
  int64_t top;
  if (!sums || !wsum || !out || !fixwin || !best_fixed || R < 2 || G < 1 || K < 1 || !rv_sense_ok(sense) ||
      check_quantiles(q, Q, std::numeric_limits<int32_t>::max()) != INSITE_OK || ld_out < (int64_t)3 + Q ||
      !rv_mul_add((int64_t)3 + Q, (int64_t)G * (3 * (int64_t)K + 9) - 1, ld_out, &top))
    return INSITE_E_INVALID_ARG;
  if (R > INSITE_RULEVALUE_MAX_REPLICATES || G > INSITE_RULEVALUE_MAX_GROUPS || K > INSITE_RULEVALUE_MAX_RULES ||
      Q > INSITE_RULEVALUE_MAX_QUANTILES)
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

int32_t rv_run_finalize(const RvFinArgs& fa, hipStream_t hs) {
  const unsigned blocks = (unsigned)(fa.G * (3 * fa.K + 10));  // <= 64 x 58
  rulevalue_finalize_kernel<<<blocks, kRvFinBlock, (size_t)fa.rpad * sizeof(double), hs>>>(fa);
  return launch_status();
}

}  // namespace

extern "C" {

int32_t insite_rulevalue_abi_version(void) { return INSITE_RULEVALUE_ABI_VERSION; }

size_t insite_rulevalue_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                        int32_t n_replicates, int32_t n_groups, int32_t n_rules) {
  // (no sub-steps and no dt here: 1 and 0 pass)
  int64_t top;
  if (!ensemble_shape_ok(n_rows, T, n_arms, 1, 0.0, n_replicates) || n_groups < 1 ||
      n_groups > INSITE_RULEVALUE_MAX_GROUPS || n_rules < 1 || n_rules > INSITE_RULEVALUE_MAX_RULES || n_terms < 1 ||
      n_terms > INSITE_MAX_TERMS || n_replicates > INSITE_RULEVALUE_MAX_REPLICATES || n_rows == 0 ||
      !rv_mul_add(7, n_rows, 4, &top))
    return 0;
  return rv_plan(n_rows, n_replicates, n_groups, n_rules).bytes;
}

int32_t insite_rulevalue_sums_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                                  const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w,
                                  const double* cost, const double* arm_cost, int32_t sense, const double* coef,
                                  const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                                  int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const int32_t* group, int32_t n_groups, int32_t weighting,
                                  uint32_t seed, int64_t patient_offset, const int32_t* assign, int32_t* assign_out,
                                  void* workspace, size_t workspace_bytes, double* sums, double* wsum, void* stream) {
  RvSumsCall c;
  const int32_t st = rv_prepare_sums(y0, u, theta, ld_theta, rules, n_rules, w, ld_w, cost, arm_cost, sense, coef, exps,
                                     n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below,
                                     n_replicates, group, n_groups, weighting, seed, patient_offset, assign, assign_out,
                                     workspace, workspace_bytes, sums, wsum, &c);
  if (st != INSITE_OK || c.empty) return st;
  return rv_run_sums(c, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_rulevalue_finalize_f64(const double* sums, const double* wsum, int32_t n_replicates, int32_t n_groups,
                                      int32_t n_rules, int32_t sense, const double* q, int32_t n_quantiles,
                                      double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream) {
  RvFinArgs fa;
  const int32_t st = rv_prepare_finalize(sums, wsum, n_replicates, n_groups, n_rules, sense, q, n_quantiles, out,
                                         ld_out, fixwin, best_fixed, &fa);
  if (st != INSITE_OK) return st;
  return rv_run_finalize(fa, reinterpret_cast<hipStream_t>(stream));
}

int32_t insite_rulevalue_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                             const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w, const double* cost,
                             const double* arm_cost, int32_t sense, const double* coef, const int8_t* exps,
                             int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms, double dt,
                             int32_t method, int32_t substeps, double drop_below, int32_t n_replicates,
                             const int32_t* group, int32_t n_groups, int32_t weighting, uint32_t seed,
                             int64_t patient_offset, const int32_t* assign, int32_t* assign_out, void* workspace,
                             size_t workspace_bytes, double* sums, double* wsum, const double* q, int32_t n_quantiles,
                             double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream) {
  // the finalize checks that need no pointer into the cohort first, so that n_rows = 0 is still validated in full
  // (sums and wsum may be NULL with no rows: a stand-in passes their NULL checks here, the sums call makes its own)
  static const double stand_in = 0.0;
  RvFinArgs fa;
  int32_t st = rv_prepare_finalize(sums ? sums : &stand_in, wsum ? wsum : &stand_in, n_replicates, n_groups, n_rules,
                                   sense, q, n_quantiles, out, ld_out, fixwin, best_fixed, &fa);
  const int32_t st_fin = st;
  if (st == INSITE_E_INVALID_ARG) return st;
  RvSumsCall c;
  st = rv_prepare_sums(y0, u, theta, ld_theta, rules, n_rules, w, ld_w, cost, arm_cost, sense, coef, exps, n_terms,
                       n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below, n_replicates, group, n_groups,
                       weighting, seed, patient_offset, assign, assign_out, workspace, workspace_bytes, sums, wsum, &c);
  if (st == INSITE_OK && st_fin != INSITE_OK) st = st_fin;  // (an invalid argument of either goes before a cap)
  if (st != INSITE_OK || c.empty) return st;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  st = rv_run_sums(c, hs);
  if (st != INSITE_OK) return st;
  return rv_run_finalize(fa, hs);
}

}  // extern "C"
