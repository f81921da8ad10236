/*
 * insite_rulevalue.h — the cohort and subgroup value of closed-loop treatment rules: what a cohort gains under rule j,
 * what it gains when every row gets its own best rule instead of the one best rule, how many treated steps per row
 * each of these policies costs, and how sure the bootstrap ensemble is of each number.  An extension of the C ABI of
 * libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_RULEVALUE_ABI_VERSION) so that the pinned surfaces of
 * insite_hip.h, insite_irregular.h, insite_weak.h, insite_bootstrap.h, insite_effect.h, insite_cohort.h,
 * insite_regimen.h, insite_policy.h and insite_feedback.h do not move.  The symbols live in the same shared library.
 *
 * The call is to insite_feedback.h what insite_policy.h is to insite_regimen.h: per replicate and row it rolls
 * insite_feedback.h's K closed loops, takes their argmin, and adds objectives, votes and exposures, weighted as
 * insite_cohort.h weighs rows, to 3 K + 4 sums per (replicate, group).  Under feedback every replicate follows a
 * treatment sequence of its own, so insite_policy_sums_f64 (whose step arm comes from a plan) cannot give these sums,
 * and the band of a cohort mean is not the mean of the rows' bands.  The per-replicate objectives never exist in
 * memory.  A second call turns the (all-reduced) sums into the statistics of 3 K + 9 series.  DESIGN.md §9n.
 *
 * Conventions are insite_policy.h's: device pointers to caller-owned memory (exps, q, rules and arm_cost: HOST
 * arrays), row-major, no allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK /
 * INSITE_E_*), every argument validated before any HIP call, n_rows = 0 a successful no-op.
 *
 * Where the workspace stands in the signatures.  insite_rulevalue_sums_f64 and insite_rulevalue_f64 need scratch (the
 * patient chunks' partial sums and the assignment), but their (workspace, workspace_bytes) pair stands before the
 * outputs, not in front of the stream: the project's workspace-contract test matrix holds a pinned list of every entry
 * point whose signature ends in (void* workspace, size_t workspace_bytes, void* stream), and these calls came after
 * that list was closed.  Their contract is that matrix's class "none" all the same: exactly
 * insite_rulevalue_workspace_bytes(...) bytes suffice, the buffer needs no initialisation, nothing is carried between
 * calls, and workspace_bytes is read only to refuse a buffer that is too small.
 *
 * Definition.
 *   Per-row quantities.  insite_feedback.h's, word for word.  Trajectories: the terms with |c| > drop_below are kept, a
 *     NaN coefficient makes alpha or beta of its arm (and the trajectory from the first use of that arm) NaN, one
 *     interval is the Euler or RK4 map with `substeps` sub-steps, y[r, p, j, k], k = 0..T-1, is the state of row p
 *     under replicate r and rule j after interval k.  Rule j is the HOST row rules[4 j .. 4 j + 3] = (arm_on, arm_off,
 *     period >= 1, start_on in {0, 1}) with theta_on = theta[p ld_theta + 2 j], theta_off = theta[p ld_theta + 2 j + 1]
 *     (ld_theta == 0: one shared [K, 2] table; otherwise ld_theta >= 2 K); both arms lie in 0..n_arms-1.  Decision:
 *     with z_k = y0[p] for k = 0 and y[k - 1] otherwise, and on_{-1} = start_on,
 *         k mod period == 0:  on_k = (z_k >= (on_{k-1} ? theta_off : theta_on));   otherwise:  on_k = on_{k-1};
 *     one ordered comparison (a NaN on either side: off), taken inside each replicate on its own z_k; interval k runs
 *     under arm_k = on_k ? arm_on : arm_off.  The weight of step k is w[p ld_w + k] (ld_w == 0: one shared [T]
 *     vector).  Objective: J[r, p, j] starts at cost[j] (0 when cost is NULL); for k ascending
 *     J <- fma(w[p, k], y[k], J) and then, only when arm_cost is not NULL, J <- J + arm_cost[arm_k] (a separate,
 *     rounded addition).  A weight is always multiplied.  Exposure: E[r, p, j] = #{k < T : on_k}, an exact integer as a
 *     double; NaN if any y[k] of that replicate and rule is NaN.
 *   Choice inside a replicate.  insite_regimen.h's: with s = sense (+1 minimise, -1 maximise), replicate r abstains for
 *     row p if any of its K objectives is NaN.  Otherwise best[r, p] is the smallest j that attains min_j s J[r, p, j]:
 *     the comparison is strict and runs in ascending j; +-Inf compare as values.
 *   Row weights and groups.  insite_cohort.h's, verbatim.  omega[r, p] (so called to keep them apart from the step
 *     weights w): INSITE_COHORT_WEIGHT_NONE: 1.  INSITE_COHORT_WEIGHT_POISSON: omega[0, p] = 1; for r >= 1 the
 *     Poisson(1) count of insite_bootstrap.h under the key (seed, r) and the global patient index patient_offset + p.
 *     Row p contributes to group group[p] iff 0 <= group[p] < n_groups (group NULL: every row is in group 0).  A row
 *     outside that range, and a row with omega[r, p] = 0, contributes nothing to (that replicate of) any sum, by a
 *     select and not by a multiplication by zero: its y0, u and theta may be NaN.
 *   Assignment.  assign[p] is the rule a fixed per-row assignment gives to row p.  (It is what insite_policy.h calls
 *     `rule`; here that word means one of the K candidates.)  assign NULL: the point model's own choice,
 *     assign[p] = best[0, p] (-1 where replicate 0 abstains), computed by the call for every row (grouped or not) and
 *     also written to assign_out when that is not NULL.  A value outside 0..K-1 contributes NaN to the two assigned
 *     columns of every (replicate, group) in which the row has weight > 0.
 *   Sums.  With the contributing rows p of group g and K = n_rules, sums[r, g, c] for c = 0..3K+3:
 *       c = j < K        sum_p omega J[r, p, j]               everyone follows rule j
 *       c = K            sum_p omega J[r, p, best[r, p]]      personalised; a row for which the replicate abstains adds NaN
 *       c = K + 1        sum_p omega J[r, p, assign[p]]       the given assignment under replicate r's model
 *       c = K + 2 + j    sum_p omega [best[r, p] = j]         the allocation: exact integers; an abstaining row votes
 *                                                             for nobody
 *       c = 2K + 2 + j   sum_p omega E[r, p, j]               exact integers as doubles; NaN where E is
 *       c = 3K + 2       sum_p omega E[r, p, best[r, p]]      NaN where the replicate abstains for a row
 *       c = 3K + 3       sum_p omega E[r, p, assign[p]]
 *     and wsum[r, g] = sum_p omega (exact).  Every sum is a plain accumulation acc <- fma(omega, v, acc) over the rows
 *     ascending inside a patient chunk, the chunks added in chunk order, the same order for every column, with no
 *     compensation term.  Rounding is monotone, so wherever nothing is NaN
 *       s sums[r, g, K] <= s sums[r, g, j] for every j   and   s sums[r, g, K] <= s sums[r, g, K + 1]
 *     hold exactly.  sums and wsum are additive over the shards of a cohort (the inequalities hold for the total of
 *     two shards only up to the rounding of that addition); patient_offset makes a shard draw the weights it has
 *     inside the whole cohort.  The patient chunks are a function of (n_rows, n_replicates, n_groups, n_rules) alone.
 *   Finalize, per (g, r).  Means are sums / wsum, 0 / 0 = NaN.  value_j = sums[r, g, j] / wsum[r, g].  The best fixed
 *     rule jfix[r, g] is the smallest j that attains min_j s value_j by a strict comparison in ascending j; it abstains
 *     (-1) if any value_j is NaN.  The S = 3 K + 9 series, in this order:
 *       0 .. K-1        value_0 .. value_{K-1}
 *       K               personalised          = sums[r, g, K] / wsum
 *       K + 1           assigned              = sums[r, g, K + 1] / wsum
 *       K + 2           best_fixed            = value_jfix (NaN where jfix abstains)
 *       K + 3           gain_personalised     = s best_fixed - s personalised
 *       K + 4           gain_assigned         = s best_fixed - s assigned
 *       K + 5           optimism              = s assigned - s personalised
 *       K + 6 + j       share_j               = sums[r, g, K + 2 + j] / wsum
 *       2K + 6 + j      exposure_j            = sums[r, g, 2K + 2 + j] / wsum   (treated steps per row under rule j)
 *       3K + 6          exposure_personalised = sums[r, g, 3K + 2] / wsum
 *       3K + 7          exposure_assigned     = sums[r, g, 3K + 3] / wsum
 *       3K + 8          exposure_best_fixed   = exposure_jfix (NaN where jfix abstains)
 *     gain_personalised and optimism are >= 0 in every replicate where they are not NaN, exactly +0 where both sides
 *     are bitwise equal.  gain_assigned has no such bound.
 *   Statistics over r, per (g, series), and the NaN rule are insite_effect.h's, with v[r] the series and n = R - 1:
 *     stat 0 = v[0], the point model; stat 1 = the mean over 1..R-1, evaluated as c + (sum_r (v[r] - c)) / n with the
 *     shift c = v[1] (c = 0 when v[1] is not finite); stat 2 = the standard deviation with ddof = 1, two-pass, NaN when
 *     n = 1; stats 3.. = the quantiles q[j] in the caller's order by the interpolation formula stated there.  If any
 *     of v[1..R-1] is NaN, the mean, the standard deviation and all quantiles there are NaN; the point value is not
 *     affected.  A replicate that drew no row of a group makes every series of the group NaN (0 / 0).
 *   Outputs.
 *     out[g, series, stat] at out[(g S + series) ld_out + stat], ld_out >= 3 + Q; the padding is not written.
 *     fixwin[g, j] = #{r >= 1 : jfix[r, g] = j} / (R - 1): an exact integer count, divided once, in double.
 *     best_fixed[g] = jfix[0, g], -1 if it abstains.
 *   Reproducibility.  Every reduction runs in a fixed order (a lane's rows ascending, the patient chunks in chunk
 *     order, the statistics in a fixed tree), no atomics: two calls give bitwise equal outputs.  Under
 *     theta_on = theta_off = -Inf (always on) or +Inf with start_on = 0 (always off) and arm_cost NULL, the columns
 *     0..2K+1 and wsum are insite_policy_sums_f64's under the constant plans arm_on (arm_off), bit for bit, wherever
 *     the two calls cut the cohort into the same patient chunks (they do unless a workspace bound binds).
 */
#ifndef INSITE_RULEVALUE_H_
#define INSITE_RULEVALUE_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_cohort.h"
#include "insite_feedback.h"
#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_RULEVALUE_ABI_VERSION 1

/* Caps; anything above one: INSITE_E_UNSUPPORTED.  Replicates (the point model included): the finalize kernel's sort
 * holds the keys of one series in one block's LDS.  Rules: the sums kernel keeps 3 K + 5 accumulators per lane. */
#define INSITE_RULEVALUE_MAX_REPLICATES 4096
#define INSITE_RULEVALUE_MAX_RULES 16
#define INSITE_RULEVALUE_MAX_GROUPS 64
#define INSITE_RULEVALUE_MAX_QUANTILES 16

int32_t insite_rulevalue_abi_version(void);

/* Bytes of workspace insite_rulevalue_sums_f64 / insite_rulevalue_f64 need for this shape: the assignment (one int32
 * per row, rounded up to 8 bytes) and the partial sums of the patient chunks, n_groups x ceil(n_replicates / 64) x 64 x
 * (3 n_rules + 5) doubles per chunk; below 1 GiB + 4 n_rows.  Returns 0 for invalid or unsupported arguments (those
 * calls' rules for n_rows, T, n_arms, n_terms, n_replicates, n_groups, n_rules), for shapes whose byte count leaves
 * int64, and for n_rows = 0. */
size_t insite_rulevalue_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                        int32_t n_replicates, int32_t n_groups, int32_t n_rules);

/* The weighted sums of one cohort (or shard).
 *   y0, u, theta / ld_theta, rules (HOST) / n_rules, w / ld_w, cost, arm_cost (HOST), sense, coef, exps (HOST),
 *   n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below: insite_feedback_rules_f64's
 *   n_replicates, group, n_groups, weighting, seed, patient_offset: insite_cohort_effect_sums_f64's
 *   assign    i32 [n_rows] or NULL (the point model's choice);  assign_out i32 [n_rows] or NULL: written only when
 *             assign is NULL
 *   workspace / workspace_bytes: at least insite_rulevalue_workspace_bytes(...) bytes, 8-byte aligned; needs no
 *             initialisation and carries nothing between calls (before the outputs: see the head of this file)
 *   sums      f64 [n_replicates, n_groups, 3 n_rules + 4];  wsum f64 [n_replicates, n_groups];  both overwritten
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0,
 * n_replicates < 2, n_groups < 1, n_rules < 1, rules NULL, a rule with an arm outside 0..n_arms-1, a period < 1 or a
 * start_on other than 0 / 1, a sense other than +1 / -1, an unknown weighting, patient_offset < 0 or
 * patient_offset + n_rows beyond int64, a negative leading dimension, ld_theta in 1..2 n_rules - 1, ld_w in 1..T-1,
 * leading dimensions whose largest element offset does not fit int64, an invalid table, and (when n_rows > 0) a NULL
 * y0, theta, w, coef, sums or wsum, a NULL u with n_statics > 0, a NULL, misaligned or too small workspace.
 * INSITE_E_UNSUPPORTED: an unknown method, a state exponent above 1, n_replicates, n_rules or n_groups above its cap.
 * n_rows = 0 is a successful no-op: nothing is written. */
int32_t insite_rulevalue_sums_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                                  const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w,
                                  const double* cost, const double* arm_cost, int32_t sense, const double* coef,
                                  const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                                  int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const int32_t* group, int32_t n_groups, int32_t weighting,
                                  uint32_t seed, int64_t patient_offset, const int32_t* assign, int32_t* assign_out,
                                  void* workspace, size_t workspace_bytes, double* sums, double* wsum, void* stream);

/* The statistics of the 3 n_rules + 9 series from (all-reduced) sums.
 *   sums  f64 [n_replicates, n_groups, 3 n_rules + 4];  wsum f64 [n_replicates, n_groups]
 *   q     f64 [n_quantiles] HOST, each in [0, 1], any order
 *   out   f64 [n_groups, 3 n_rules + 9, ld_out >= 3 + n_quantiles];  fixwin f64 [n_groups, n_rules];
 *   best_fixed i32 [n_groups]
 * INSITE_E_INVALID_ARG: NULL sums, wsum, q, out, fixwin or best_fixed, n_replicates < 2, n_groups, n_rules or
 * n_quantiles < 1, a sense other than +1 / -1, ld_out < 3 + n_quantiles or so large that the last element offset does
 * not fit int64, a q[j] NaN or outside [0, 1].  INSITE_E_UNSUPPORTED: n_replicates, n_groups, n_rules or n_quantiles
 * above its cap. */
int32_t insite_rulevalue_finalize_f64(const double* sums, const double* wsum, int32_t n_replicates, int32_t n_groups,
                                      int32_t n_rules, int32_t sense, const double* q, int32_t n_quantiles,
                                      double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream);

/* insite_rulevalue_sums_f64 followed on the stream by insite_rulevalue_finalize_f64, without host synchronisation;
 * sums and wsum are outputs of the caller's.  Every argument rule of the two holds (a NULL out, fixwin or best_fixed
 * is INSITE_E_INVALID_ARG whatever n_rows); n_rows = 0 is a successful no-op: nothing is written.  A cohort sharded
 * over several devices calls the two parts and all-reduces sums and wsum between them: that collective is the
 * caller's. */
int32_t insite_rulevalue_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                             const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w, const double* cost,
                             const double* arm_cost, int32_t sense, const double* coef, const int8_t* exps,
                             int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms, double dt,
                             int32_t method, int32_t substeps, double drop_below, int32_t n_replicates,
                             const int32_t* group, int32_t n_groups, int32_t weighting, uint32_t seed,
                             int64_t patient_offset, const int32_t* assign, int32_t* assign_out, void* workspace,
                             size_t workspace_bytes, double* sums, double* wsum, const double* q, int32_t n_quantiles,
                             double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_RULEVALUE_H_ */
