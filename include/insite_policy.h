/*
 * insite_policy.h — policy value: what a cohort gains when every row gets its own best plan of K candidates instead
 * of everyone getting the best single plan, and how sure the bootstrap ensemble is of that gain.  An extension of the
 * C ABI of libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_POLICY_ABI_VERSION) so that the pinned
 * surfaces of insite_hip.h, insite_irregular.h, insite_weak.h, insite_bootstrap.h, insite_effect.h, insite_cohort.h
 * and insite_regimen.h do not move.  The symbols live in the same shared library.
 *
 * The call is the reduction that joins insite_cohort.h and insite_regimen.h: per replicate and row it forms
 * insite_regimen.h's objectives of the K plans and their argmin, and adds them, weighted as insite_cohort.h weighs
 * rows, to 2 K + 2 sums per (replicate, group).  The per-replicate objectives never exist in memory.  A second call
 * turns the (all-reduced) sums into the statistics of 2 K + 6 series.  DESIGN.md §9k.
 *
 * Conventions are insite_cohort.h's: device pointers to caller-owned memory (exps and q: HOST arrays), row-major, no
 * allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every
 * argument validated before any HIP call, n_rows = 0 a successful no-op.
 *
 * Definition.
 *   Objectives.  J[r, p, j], j = 0..K-1, is insite_regimen.h's objective, word for word: y_j[r, p, k] is
 *     insite_effect.h's trajectory of row p under the replicate's coefficients coef[r] and the per-step arms of plan j
 *     (the terms with |c| > drop_below; a NaN coefficient makes alpha or beta of its arm, and the trajectory from the
 *     first use of that arm, NaN; an arm value outside 1..n_arms-1 selects arm 0); the arm of plan j, row p at step k
 *     is plans[j plan_stride + p ld_plan + k] (ld_plan == 0: every row shares plan j's [T] vector); the weight of step
 *     k is w[p ld_w + k] (ld_w == 0: one shared [T] vector); J starts at cost[j] (0 when cost is NULL) and accumulates
 *     over k ascending, each step one FMA: J <- fma(w[p, k], y_j[r, p, k], J).  A step weight is always multiplied.
 *   Choice inside a replicate.  With s = sense (+1 minimise, -1 maximise), replicate r abstains for row p if any of its
 *     K objectives is NaN.  Otherwise best[r, p] is the smallest j that attains min_j s J[r, p, j]: the comparison is
 *     strict and runs in ascending j; +-Inf compare as values.
 *   Row weights.  omega[r, p] (so called to keep them apart from the step weights w) are insite_cohort.h's weights,
 *     verbatim: INSITE_COHORT_WEIGHT_NONE: 1.  INSITE_COHORT_WEIGHT_POISSON: omega[0, p] = 1; for r >= 1 the
 *     Poisson(1) count of insite_bootstrap.h under the key (seed, r) and the global patient index patient_offset + p.
 *   Groups.  Row p contributes to group group[p] iff 0 <= group[p] < n_groups (group NULL: every row is in group 0).
 *     A row outside that range, and a row with omega[r, p] = 0, contributes nothing to (that replicate of) any sum, by
 *     a select and not by a multiplication by zero: its y0 and u may be NaN.
 *   The rule.  rule[p] is the plan a fixed per-row rule assigns to row p.  rule NULL: the point model's own choice,
 *     rule[p] = best[0, p] (-1 where replicate 0 abstains), computed by the call for every row (grouped or not) and
 *     also written to rule_out when that is not NULL.  A rule value outside 0..K-1 contributes NaN to the rule column
 *     of every (replicate, group) in which the row has weight > 0.
 *   Sums.  With the contributing rows p of group g and K = n_plans, sums[r, g, c] for c = 0..2K+1:
 *       c = j < K      sum_p omega J[r, p, j]                 everyone gets plan j
 *       c = K          sum_p omega J[r, p, best[r, p]]        the personalised rule re-derived in replicate r; a row
 *                                                              for which the replicate abstains adds NaN
 *       c = K + 1      sum_p omega J[r, p, rule[p]]           the given rule under replicate r's model
 *       c = K + 2 + j  sum_p omega [best[r, p] = j]           the allocation: exact integers; an abstaining row votes
 *                                                              for nobody
 *     and wsum[r, g] = sum_p omega (exact).  Every sum is a plain accumulation acc <- fma(omega, J, acc) over the rows
 *     ascending inside a patient chunk, the chunks added in chunk order, with no compensation term.  Rounding is
 *     monotone and the order is the same for every column, so wherever nothing is NaN
 *       s sums[r, g, K] <= s sums[r, g, j] for every j   and   s sums[r, g, K] <= s sums[r, g, K + 1]
 *     hold exactly.  sums and wsum are additive over the shards of a cohort (the inequalities hold for the total of
 *     two shards only up to the rounding of that addition, unless the shards are added column by column in the same
 *     order); patient_offset makes a shard draw the weights it has inside the whole cohort.
 *   Finalize, per (g, r).  Means are sums / wsum, 0 / 0 = NaN.  value_j = sums[r, g, j] / wsum[r, g].  The best fixed
 *     plan jfix[r, g] is the smallest j that attains min_j s value_j by a strict comparison in ascending j; it
 *     abstains (-1) if any value_j is NaN.  The S = 2 K + 6 series, in this order:
 *       0 .. K-1       value_0 .. value_{K-1}
 *       K              personalised      = sums[r, g, K] / wsum
 *       K + 1          rule              = sums[r, g, K + 1] / wsum
 *       K + 2          best_fixed        = value_jfix (NaN where jfix abstains)
 *       K + 3          gain_personalised = s best_fixed - s personalised   (= s (best_fixed - personalised))
 *       K + 4          gain_rule         = s best_fixed - s rule
 *       K + 5          optimism          = s rule - s personalised
 *       K + 6 + j      share_j           = sums[r, g, K + 2 + j] / wsum
 *     gain_personalised and optimism are >= 0 in every replicate where they are not NaN (the inequalities above,
 *     divided by one positive number), exactly +0 where both sides are bitwise equal.  gain_rule has no such bound: it
 *     is negative where the given rule does worse than the best fixed plan.
 *   Statistics over r, per (g, series), are insite_effect.h's, with v[r] the series and n = R - 1:
 *     stat 0 = v[0], the point model;
 *     stat 1 = the mean over 1..R-1, evaluated as c + (sum_r (v[r] - c)) / n with the shift c = v[1] (c = 0 when
 *              v[1] is not finite);
 *     stat 2 = the standard deviation with ddof = 1, two-pass: sqrt(sum_r (v[r] - mean)^2 / (n - 1)), NaN when n = 1;
 *     stats 3.. = the quantiles q[j] in the caller's order: with s the ascending sort of v[1..R-1], pos = q (n - 1),
 *              i = floor(pos) clamped to n - 1, g = pos - i (both computed on the host in double),
 *              hi = s[min(i + 1, n - 1)]; the result is s[i] when g == 0 or s[i] == hi, else s[i] + g (hi - s[i]).
 *   NaN.  If any of v[1..R-1] is NaN, the mean, the standard deviation and all quantiles there are NaN; the point
 *     value is not affected.  So a replicate r >= 1 whose model is NaN poisons value_j of the plans whose objective is
 *     NaN in it, personalised, best_fixed, the three differences, and rule where a contributing row's ruled plan is
 *     among them; the shares stay finite (the abstaining rows vote for nobody).  A replicate that drew no row of a
 *     group makes every series of the group NaN (0 / 0).
 *   Outputs.
 *     out[g, series, stat] at out[(g S + series) ld_out + stat], ld_out >= 3 + Q; the padding is not written.
 *     fixwin[g, j] = #{r >= 1 : jfix[r, g] = j} / (R - 1): an exact integer count, divided once, in double.
 *     best_fixed[g] = jfix[0, g], -1 if it abstains.
 *   Reproducibility.  Every reduction runs in a fixed order (a lane's rows ascending, the patient chunks in chunk
 *     order, the statistics in a fixed tree), no atomics: two calls give bitwise equal outputs.
 */
#ifndef INSITE_POLICY_H_
#define INSITE_POLICY_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_cohort.h"
#include "insite_hip.h"
#include "insite_regimen.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_POLICY_ABI_VERSION 1

/* Caps; anything above one: INSITE_E_UNSUPPORTED.  Replicates (the point model included): the finalize kernel's sort
 * holds the keys of one series in one block's LDS.  Plans: the sums kernel keeps 2 K + 3 accumulators per lane. */
#define INSITE_POLICY_MAX_REPLICATES 4096
#define INSITE_POLICY_MAX_PLANS 16
#define INSITE_POLICY_MAX_GROUPS 64
#define INSITE_POLICY_MAX_QUANTILES 16

int32_t insite_policy_abi_version(void);

/* Bytes of workspace insite_policy_sums_f64 / insite_policy_value_f64 need for this shape: the rule (one int32 per
 * row, rounded up to 8 bytes) and the partial sums of the patient chunks, n_groups x ceil(n_replicates / 64) x 64 x
 * (2 n_plans + 3) doubles per chunk; below 1 GiB + 4 n_rows.  Returns 0 for invalid or unsupported arguments (those
 * calls' rules for n_rows, T, n_arms, n_terms, n_replicates, n_groups, n_plans) and for n_rows = 0. */
size_t insite_policy_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms, int32_t n_replicates,
                                     int32_t n_groups, int32_t n_plans);

/* The weighted sums of one cohort (or shard).
 *   y0, u, plans / n_plans / plan_stride / ld_plan, w / ld_w, cost, sense, coef, exps (HOST), n_terms, n_rows, T,
 *   n_statics, n_arms, dt, method, substeps, drop_below: insite_regimen_choice_f64's
 *   n_replicates, group, n_groups, weighting, seed, patient_offset: insite_cohort_effect_sums_f64's
 *   rule      i32 [n_rows] or NULL (the point model's choice);  rule_out i32 [n_rows] or NULL: written only when rule
 *             is NULL
 *   sums      f64 [n_replicates, n_groups, 2 n_plans + 2];  wsum f64 [n_replicates, n_groups];  both overwritten
 *   workspace / workspace_bytes: at least insite_policy_workspace_bytes(...) bytes, 8-byte aligned; needs no
 *             initialisation and carries nothing between calls
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0,
 * n_replicates < 2, n_groups < 1, n_plans < 1, a sense other than +1 / -1, an unknown weighting, patient_offset < 0 or
 * patient_offset + n_rows beyond int64, a negative stride or leading dimension, ld_plan or ld_w in 1..T-1,
 * plan_stride < T or < n_rows ld_plan, strides whose largest element offset does not fit int64, an invalid table, and
 * (when n_rows > 0) a NULL y0, plans, w, coef, sums or wsum, a NULL u with n_statics > 0, a NULL, misaligned or too
 * small workspace.  INSITE_E_UNSUPPORTED: an unknown method, a state exponent above 1, n_replicates, n_plans or
 * n_groups above its cap.  n_rows = 0 is a successful no-op: nothing is written. */
int32_t insite_policy_sums_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                               int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w, const double* cost,
                               int32_t sense, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                               int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method,
                               int32_t substeps, double drop_below, int32_t n_replicates, const int32_t* group,
                               int32_t n_groups, int32_t weighting, uint32_t seed, int64_t patient_offset,
                               const int32_t* rule, int32_t* rule_out, double* sums, double* wsum, void* workspace,
                               size_t workspace_bytes, void* stream);

/* The statistics of the 2 n_plans + 6 series from (all-reduced) sums.
 *   sums  f64 [n_replicates, n_groups, 2 n_plans + 2];  wsum f64 [n_replicates, n_groups]
 *   q     f64 [n_quantiles] HOST, each in [0, 1], any order
 *   out   f64 [n_groups, 2 n_plans + 6, ld_out >= 3 + n_quantiles];  fixwin f64 [n_groups, n_plans];
 *   best_fixed i32 [n_groups]
 * INSITE_E_INVALID_ARG: NULL sums, wsum, q, out, fixwin or best_fixed, n_replicates < 2, n_groups, n_plans or
 * n_quantiles < 1, a sense other than +1 / -1, ld_out < 3 + n_quantiles or so large that the last element offset does
 * not fit int64, a q[j] NaN or outside [0, 1].  INSITE_E_UNSUPPORTED: n_replicates, n_groups, n_plans or n_quantiles
 * above its cap. */
int32_t insite_policy_finalize_f64(const double* sums, const double* wsum, int32_t n_replicates, int32_t n_groups,
                                   int32_t n_plans, int32_t sense, const double* q, int32_t n_quantiles, double* out,
                                   int64_t ld_out, double* fixwin, int32_t* best_fixed, void* stream);

/* insite_policy_sums_f64 followed on the stream by insite_policy_finalize_f64, without host synchronisation; sums and
 * wsum are outputs of the caller's.  Every argument rule of the two holds (a NULL out, fixwin or best_fixed is
 * INSITE_E_INVALID_ARG whatever n_rows); n_rows = 0 is a successful no-op: nothing is written.  A cohort sharded over
 * several devices calls the two parts and all-reduces sums and wsum between them: that collective is the caller's. */
int32_t insite_policy_value_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                                int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w, const double* cost,
                                int32_t sense, const double* coef, const int8_t* exps, int32_t n_terms, int64_t n_rows,
                                int32_t T, int32_t n_statics, int32_t n_arms, double dt, int32_t method,
                                int32_t substeps, double drop_below, int32_t n_replicates, const int32_t* group,
                                int32_t n_groups, int32_t weighting, uint32_t seed, int64_t patient_offset,
                                const int32_t* rule, int32_t* rule_out, double* sums, double* wsum, const double* q,
                                int32_t n_quantiles, double* out, int64_t ld_out, double* fixwin, int32_t* best_fixed,
                                void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_POLICY_H_ */
