// insite_feedback.hip — closed-loop treatment rules over the bootstrap ensemble on MI355X (gfx950):
// include/insite_feedback.h, DESIGN.md §9m.
//
// Kernel:
//   feedback_rules_kernel  wave = row.  Lane l holds V = R_pad / 64 replicates (replicate s 64 + l in slot s), as
//                          regimen_choice_kernel, and the skeleton is that kernel's: the prologue (insite_affine.h's
//                          ensemble_maps, once per row for all K rules), the row's weights in 16-step chunks read back
//                          by v_readlane, the running strict minimum of s J, J of the rules 0..K-2 in a lane-private
//                          LDS column, the votes by ballot + popcount, the statistics by insite_wavestats.h's
//                          ef_series_stats, and one rule's block flushed as one contiguous segment.  What is new is
//                          the step: the arm is the replicate's own, so there is no scalar branch on it.  The rule's
//                          two arms are wave-uniform: with more than two arms their maps (A_on, B_on, A_off, B_off)
//                          are picked out of PA / PB per slot once per rule, up to two arms the loop selects between
//                          the arms' own maps; the `on` flags are one lane mask per slot; at a decision step
//                          (k mod period == 0, a scalar countdown) every slot compares its state with the threshold
//                          its flag selects and re-selects its active (A, B); a step between decisions is the two
//                          FMAs of the regimen step plus the exposure count (an integer add per slot) and, with
//                          arm_cost, one select and one add.  The exposure statistics do not depend on the argmin:
//                          they are taken right after the rule's rollout and wait in LDS ([K][3 + Q]) for the
//                          rule's flush; only J waits for the regret.  The point model's arm (lane 0, slot 0) of
//                          every step of a chunk is collected in the chunk's lanes (lane i keeps step k0 + i) and
//                          written as one byte per lane per chunk.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "insite_affine.h"
#include "insite_feedback.h"
#include "insite_wavestats.h"

namespace {

constexpr int kFbTc = 16;                                    // steps per chunk of weights and schedule bytes
constexpr int kFbMaxStats = 3 + INSITE_FEEDBACK_MAX_QUANTILES;
constexpr int kFbStage = 40;                                 // doubles of the staging block: >= 2 kFbMaxStats
static_assert(2 * kFbMaxStats <= kFbStage && 3 * kFbMaxStats <= kWave, "one rule's block is flushed by one wave at once");
static_assert(INSITE_FEEDBACK_MAX_RULES <= kWave, "one lane per rule holds its votes");

// One 8-byte element, indexed by the (wave-uniform) rule: code = arm_on | arm_off << 8 | start_on << 16.
struct FbRule {
  int32_t code, period;
};

struct FbArgs {
  const double* y0;
  const double* u;
  const double* theta;
  const double* w;
  const double* cost;  // nullptr: zeros
  const double* coef;
  int32_t* choice;
  double* win;
  double* out;
  int8_t* sched;  // nullptr: not written
  int64_t ldt, ldw, ldo, lds, N, ppb;  // ppb: rows per block
  int32_t T, A, K, substeps, method, R, Q, Rpad;
  double dt, drop, sense;
};

// The host tables, a kernel argument of their own: with them inside FbArgs the register allocator left dead SGPR
// spill slots behind and the kernels asked for a private segment that no instruction used.
struct FbTables {
  double ac[INSITE_MAX_ARMS];  // arm_cost (the AC instantiations)
  FbRule rule[INSITE_FEEDBACK_MAX_RULES];
  QuantileRank qr[INSITE_FEEDBACK_MAX_QUANTILES];  // per quantile: i and g of insite_effect.h's formula
};

// v[a] for a wave-uniform arm a in 0..NARM-1: selects between compile-time indices (the maps stay in registers)
template <int NARM>
__device__ __forceinline__ double fb_pick(const double (&v)[NARM], int a) {
  if constexpr (NARM == 1) {
    return v[0];
  } else if constexpr (NARM == 2) {
    return a == 1 ? v[1] : v[0];
  } else {
    const double lo = (a & 1) ? v[1] : v[0], hi = (a & 1) ? v[3] : v[2];
    return (a & 2) ? hi : lo;
  }
}

// One rule's closed loop over the T steps for the lane's V replicates: y, J and the exposure count E are updated in
// place.  A slot's interval runs under the map (A1, B1) where (on ? hi_on : hi_off) holds and under (A0, B0)
// otherwise (hi_on, hi_off: wave-uniform; see the caller for what the two maps are).  SEL 0: one map only (A0, B0);
// SEL 1: the slot's active map is copied at a decision step, so a step between decisions is two FMAs; SEL 2: no copy,
// the map is selected at every step (where the copies would not fit the register file).  AC: the per-step arm cost
// is added; SC: the point model's arms are written to sc[0..T-1].
template <int V, int SEL, bool AC, bool SC>
__device__ __forceinline__ void fb_closed_loop(int arm_on, int arm_off, int period, bool start_on, bool hi_on,
                                               bool hi_off, double ton, double toff, double c_on, double c_off,
                                               const double* wr, int T, int lane, int8_t* sc, const double (&A1)[V],
                                               const double (&B1)[V], const double (&A0)[V], const double (&B0)[V],
                                               double (&y)[V], double (&J)[V], int (&E)[V]) {
  double Aa[V], Ba[V];  // SEL 1: the slot's active map
  bool on[V], hi[V];
#pragma unroll
  for (int s = 0; s < V; ++s) {
    Aa[s] = A0[s];  // step 0 is a decision step: set there
    Ba[s] = B0[s];
    on[s] = start_on;
    hi[s] = false;
  }
  int cd = 0;  // steps until the next decision
  for (int k0 = 0; k0 < T; k0 += kFbTc) {
    const int nk = T - k0 < kFbTc ? T - k0 : kFbTc;
    // the chunk: lane i < nk reads the weight of step k0 + i (nothing past column T - 1)
    double ww = 0.0;
    if (lane < nk) ww = wr[k0 + lane];
    int mine = 0;  // lane i: the point model's arm at step k0 + i
    for (int kk = 0; kk < nk; ++kk) {
      if (cd == 0) {
        // a decision step: z = the state before the interval, one ordered comparison (NaN: off)
#pragma unroll
        for (int s = 0; s < V; ++s) {
          const double thr = on[s] ? toff : ton;
          on[s] = y[s] >= thr;
          hi[s] = on[s] ? hi_on : hi_off;
          if constexpr (SEL == 1) {
            Aa[s] = hi[s] ? A1[s] : A0[s];
            Ba[s] = hi[s] ? B1[s] : B0[s];
          }
        }
        cd = period;
      }
      --cd;
      const double wk = readlane_f64(ww, kk);
#pragma unroll
      for (int s = 0; s < V; ++s) {
        if constexpr (SEL == 0) y[s] = fma(A0[s], y[s], B0[s]);
        else if constexpr (SEL == 1) y[s] = fma(Aa[s], y[s], Ba[s]);
        else y[s] = fma(hi[s] ? A1[s] : A0[s], y[s], hi[s] ? B1[s] : B0[s]);
        J[s] = fma(wk, y[s], J[s]);
        E[s] += on[s] ? 1 : 0;
      }
      if constexpr (AC) {
#pragma unroll
        for (int s = 0; s < V; ++s) J[s] = J[s] + (on[s] ? c_on : c_off);
      }
      if constexpr (SC) {
        const int arm0 = (__builtin_amdgcn_ballot_w64(on[0]) & 1ull) ? arm_on : arm_off;
        mine = lane == kk ? arm0 : mine;
      }
    }
    if constexpr (SC) {
      if (lane < nk) sc[k0 + lane] = (int8_t)mine;
    }
  }
}

// AC, SC: fb_closed_loop's options, chosen by the host (arm_cost / sched given)
template <int V, int NARM, bool AC, bool SC>
__global__ void __launch_bounds__(kWave) feedback_rules_kernel(FbArgs fa, FbTables tb, AffineLib lib) {
  extern __shared__ double fb_lds[];  // [kFbStage] staging, [K][3 + Q] exposure statistics, the columns [K - 1][Rpad]
  constexpr int NB = V <= 4 ? 2 : 1;
  const int lane = threadIdx.x;
  const int NS = 3 + fa.Q;
  const int n = fa.R - 1;
  const int K = fa.K;
  double* stage = fb_lds;
  double* exs = fb_lds + kFbStage;
  double* col = exs + K * NS;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double h = fa.dt / (double)fa.substeps;
  const int64_t p_lo = (int64_t)blockIdx.x * fa.ppb;
  const int64_t p_hi = p_lo + fa.ppb < fa.N ? p_lo + fa.ppb : fa.N;
  constexpr int SEL = NARM == 1 ? 0 : (V == 8 && NARM == 2 ? 2 : 1);

  bool valid[V];  // the slot holds a resampled replicate (1..R-1); replicate 0 is lane 0, slot 0
#pragma unroll
  for (int s = 0; s < V; ++s) valid[s] = s * kWave + lane >= 1 && s * kWave + lane < fa.R;

  for (int64_t p = p_lo; p < p_hi; ++p) {
    // ---- prologue: the interval maps of the lane's replicates (insite_affine.h) ------------------------------
    double PA[V][NARM], PB[V][NARM];
    ensemble_maps<V, NARM>(lib, fa.coef, fa.u + p * lib.U, fa.R, fa.A, fa.drop, fa.method, fa.substeps, h, lane, PA,
                           PB);
    const double y0 = fa.y0[p];
    const double* wr = fa.w + p * fa.ldw;
    const double* th = fa.theta + p * fa.ldt;

    // ---- phase 1: every rule's closed loop, the running minimum inside each replicate ------------------------
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
      const FbRule rl = tb.rule[j];
      const int arm_on = rl.code & 0xff, arm_off = (rl.code >> 8) & 0xff;
      const double ton = th[2 * j], toff = th[2 * j + 1];
      const double cj = fa.cost ? fa.cost[j] : 0.0;
      const double c_on = AC ? fb_pick<INSITE_MAX_ARMS>(tb.ac, arm_on) : 0.0;
      const double c_off = AC ? fb_pick<INSITE_MAX_ARMS>(tb.ac, arm_off) : 0.0;
      // The two maps a slot chooses between.  Up to two arms they are the arms' own maps (no copy: arm 1 where
      // (on ? arm_on : arm_off) is 1); with more arms the rule's two maps are picked out of PA / PB once per rule
      // (hi = on).
      double A1[V], B1[V], A0[V], B0[V], y[V];
      int E[V];
      bool hi_on, hi_off;
      if constexpr (NARM <= 2) {
        hi_on = arm_on == 1;
        hi_off = arm_off == 1;
      } else {
        hi_on = true;
        hi_off = false;
      }
#pragma unroll
      for (int s = 0; s < V; ++s) {
        if constexpr (NARM <= 2) {
          A1[s] = PA[s][NARM - 1];
          B1[s] = PB[s][NARM - 1];
          A0[s] = PA[s][0];
          B0[s] = PB[s][0];
        } else {
          A1[s] = fb_pick<NARM>(PA[s], arm_on);
          B1[s] = fb_pick<NARM>(PB[s], arm_on);
          A0[s] = fb_pick<NARM>(PA[s], arm_off);
          B0[s] = fb_pick<NARM>(PB[s], arm_off);
        }
        y[s] = y0;
        J[s] = cj;
        E[s] = 0;
      }
      int8_t* sc = SC ? fa.sched + p * fa.lds + (int64_t)j * fa.T : nullptr;
      fb_closed_loop<V, SEL, AC, SC>(arm_on, arm_off, rl.period, (rl.code >> 16) != 0, hi_on, hi_off, ton, toff, c_on,
                                     c_off, wr, fa.T, lane, sc, A1, B1, A0, B0, y, J, E);
      // the exposure: an exact count; NaN where the trajectory is (a NaN state stays NaN: the last one tells)
      {
        double v[1][V];
#pragma unroll
        for (int s = 0; s < V; ++s) v[0][s] = y[s] != y[s] ? nan : (double)E[s];
        ef_series_stats<1, V>(v, valid, lane, n, fa.Q, tb.qr, exs + j * NS, 1);
      }
#pragma unroll
      for (int s = 0; s < V; ++s) {
        abst[s] = abst[s] || J[s] != J[s];
        const bool better = j == 0 || fa.sense * J[s] < fa.sense * bestJ[s];
        bestJ[s] = better ? J[s] : bestJ[s];
        besti[s] = better ? j : besti[s];
      }
      if (j < K - 1) {
#pragma unroll
        for (int s = 0; s < V; ++s) col[j * fa.Rpad + s * kWave + lane] = J[s];
      }
    }
#pragma unroll
    for (int s = 0; s < V; ++s) besti[s] = abst[s] ? -1 : besti[s];

    // ---- the point model's choice and the votes ----------------------------------------------------------------
    const int pick = __builtin_amdgcn_readlane(besti[0], 0);
    const int mine = ef_vote_counts<V>(valid, besti, K, lane);
    if (lane == 0) fa.choice[p] = pick;
    if (lane < K) fa.win[p * K + lane] = (double)mine / (double)n;

    // ---- phase 2: per rule (the last first: its J is still in registers) the statistics of J and of the regret ----
    for (int j = K - 1; j >= 0; --j) {
      if (j < K - 1) {
#pragma unroll
        for (int s = 0; s < V; ++s) J[s] = col[j * fa.Rpad + s * kWave + lane];
      }
      double g[V];
#pragma unroll
      for (int s = 0; s < V; ++s) g[s] = abst[s] ? nan : fa.sense * J[s] - fa.sense * bestJ[s];
      if constexpr (NB == 2) {
        double v[2][V];
#pragma unroll
        for (int s = 0; s < V; ++s) {
          v[0][s] = J[s];
          v[1][s] = g[s];
        }
        ef_series_stats<2, V>(v, valid, lane, n, fa.Q, tb.qr, stage, 1);
      } else {
#pragma unroll 1
        for (int sv = 0; sv < 2; ++sv) {
          double v[1][V];
#pragma unroll
          for (int s = 0; s < V; ++s) v[0][s] = sv == 0 ? J[s] : g[s];
          ef_series_stats<1, V>(v, valid, lane, n, fa.Q, tb.qr, stage + sv * NS, 1);
        }
      }
      // flush the rule's block: out[p, j, :, :], 3 (3 + Q) contiguous doubles (J and the regret from the staging
      // block, the exposure from its table)
      wave_lds_sync();
      if (lane < 3 * NS)
        fa.out[p * fa.ldo + (int64_t)j * 3 * NS + lane] = lane < 2 * NS ? stage[lane] : exs[j * NS + lane - 2 * NS];
      wave_lds_sync();
    }
  }
}

// a + b c in int64, or false when it does not fit (a, b, c >= 0)
inline bool fb_mul_add(int64_t a, int64_t b, int64_t c, int64_t* out) {
  int64_t m;
  return !__builtin_mul_overflow(b, c, &m) && !__builtin_add_overflow(a, m, out);
}

}  // namespace

extern "C" {

int32_t insite_feedback_abi_version(void) { return INSITE_FEEDBACK_ABI_VERSION; }

int32_t insite_feedback_rules_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                                  const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w,
                                  const double* cost, const double* arm_cost, int32_t sense, const double* coef,
                                  const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                                  int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const double* q, int32_t n_quantiles, int32_t* choice,
                                  double* win, double* out, int64_t ld_out, int8_t* sched, int64_t ld_sched,
                                  void* stream) {
  if (!ensemble_shape_ok(n_rows, T, n_arms, substeps, dt, n_replicates) ||
      check_quantiles(q, n_quantiles, INSITE_FEEDBACK_MAX_QUANTILES) != INSITE_OK || n_rules < 1 ||
      n_rules > INSITE_FEEDBACK_MAX_RULES || !rules ||
      (sense != INSITE_FEEDBACK_MINIMIZE && sense != INSITE_FEEDBACK_MAXIMIZE))
    return INSITE_E_INVALID_ARG;
  for (int j = 0; j < n_rules; ++j) {
    const int32_t* r = rules + 4 * j;
    if (r[0] < 0 || r[0] >= n_arms || r[1] < 0 || r[1] >= n_arms || r[2] < 1 || (r[3] != 0 && r[3] != 1))
      return INSITE_E_INVALID_ARG;
  }
  // the leading dimensions: their lower bounds, and the largest element offset of every array must fit int64 (the
  // kernel's index arithmetic is int64)
  const int64_t last_row = n_rows > 0 ? n_rows - 1 : 0;
  int64_t top;
  if (ld_theta < 0 || (ld_theta != 0 && ld_theta < 2 * (int64_t)n_rules) ||
      !fb_mul_add(2 * (int64_t)n_rules, last_row, ld_theta, &top))
    return INSITE_E_INVALID_ARG;
  if (ld_w < 0 || (ld_w != 0 && ld_w < (int64_t)T) || !fb_mul_add((int64_t)T, last_row, ld_w, &top))
    return INSITE_E_INVALID_ARG;
  const int64_t block = (int64_t)n_rules * 3 * (3 + n_quantiles);
  if (ld_out < block || !fb_mul_add(block, last_row, ld_out, &top) || !fb_mul_add(0, n_rows, (int64_t)n_rules, &top))
    return INSITE_E_INVALID_ARG;
  const int64_t sblock = (int64_t)n_rules * (int64_t)T;
  if (sched && (ld_sched < sblock || !fb_mul_add(sblock, last_row, ld_sched, &top))) return INSITE_E_INVALID_ARG;
  AffineLib lib;
  const int32_t st =
      ensemble_lib(method, exps, n_terms, n_statics, n_replicates, INSITE_FEEDBACK_MAX_REPLICATES, &lib);
  if (st != INSITE_OK || n_rows == 0) return st;
  if (!y0 || !theta || !w || !coef || !choice || !win || !out || (n_statics > 0 && !u)) return INSITE_E_INVALID_ARG;

  FbArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  FbTables tb;
  std::memset(&tb, 0, sizeof(tb));
  fa.y0 = y0;
  fa.u = n_statics > 0 ? u : y0;  // never read
  fa.theta = theta;
  fa.w = w;
  fa.cost = cost;
  fa.coef = coef;
  fa.choice = choice;
  fa.win = win;
  fa.out = out;
  fa.sched = sched;
  fa.ldt = ld_theta;
  fa.ldw = ld_w;
  fa.ldo = ld_out;
  fa.lds = sched ? ld_sched : 0;
  fa.N = n_rows;
  fa.T = T;
  fa.A = n_arms;
  fa.K = n_rules;
  fa.substeps = substeps;
  fa.method = method;
  fa.R = n_replicates;
  fa.Q = n_quantiles;
  fa.dt = dt;
  fa.drop = drop_below;
  fa.sense = (double)sense;
  for (int a = 0; a < n_arms; ++a) tb.ac[a] = arm_cost ? arm_cost[a] : 0.0;
  for (int j = 0; j < n_rules; ++j)
    tb.rule[j] = FbRule{rules[4 * j] | rules[4 * j + 1] << 8 | rules[4 * j + 3] << 16, rules[4 * j + 2]};
  for (int j = 0; j < n_quantiles; ++j) tb.qr[j] = quantile_rank(q[j], n_replicates - 1);
  fa.Rpad = replicate_slots(n_replicates) * kWave;
  // staging + the exposure table + K - 1 columns: at most 40 + 16 x 19 + 15 x 512 doubles = 64192 bytes, below the
  // 64 KiB a launch may ask for
  const size_t lds = sizeof(double) * ((size_t)kFbStage + (size_t)n_rules * (size_t)(3 + n_quantiles) +
                                       (size_t)(n_rules - 1) * (size_t)fa.Rpad);
  fa.ppb = rows_per_block(n_rows);
  const dim3 grid((unsigned)((n_rows + fa.ppb - 1) / fa.ppb));
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  with_slots(n_replicates, n_arms, [&](auto v, auto narm) {
    if (arm_cost) {
      if (sched) feedback_rules_kernel<v(), narm(), true, true><<<grid, kWave, lds, hs>>>(fa, tb, lib);
      else feedback_rules_kernel<v(), narm(), true, false><<<grid, kWave, lds, hs>>>(fa, tb, lib);
    } else {
      if (sched) feedback_rules_kernel<v(), narm(), false, true><<<grid, kWave, lds, hs>>>(fa, tb, lib);
      else feedback_rules_kernel<v(), narm(), false, false><<<grid, kWave, lds, hs>>>(fa, tb, lib);
    }
  });
  return launch_status();
}

}  // extern "C"
