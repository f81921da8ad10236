/*
 * insite_feedback.h — closed-loop treatment rules: "treat while the predicted state is above a threshold", evaluated
 * for each row under every replicate of the bootstrap ensemble.  An extension of the C ABI of libinsite_hip.so
 * (insite_hip.h), versioned on its own (INSITE_FEEDBACK_ABI_VERSION) so that the pinned surfaces of insite_hip.h,
 * insite_irregular.h, insite_weak.h, insite_bootstrap.h, insite_effect.h, insite_cohort.h, insite_regimen.h and
 * insite_policy.h do not move.  The symbols live in the same shared library.
 *
 * Under a state-feedback rule the arm of step k depends on the replicate's own trajectory, so every replicate of
 * insite_sindy_bootstrap_f64 follows a treatment sequence of its own: the exposure a rule leads to is a random
 * quantity with a band, and no fixed-plan call (insite_effect.h, insite_regimen.h) can give it.  For every row the call
 * rolls the K rules under every replicate, reduces each closed-loop trajectory to a scalar objective and to the number
 * of treated steps, takes the best rule inside each replicate, and gives the point model's choice, every rule's share
 * of the replicates' votes and, per rule, the objective, the regret and the exposure as point value, mean, standard
 * deviation and quantiles over the replicates.  The replicate trajectories live in one wave's registers and LDS and
 * never exist in memory.  DESIGN.md §9m.
 *
 * Conventions are insite_regimen.h's: device pointers to caller-owned memory (exps, q, rules and arm_cost: HOST
 * arrays), row-major, no allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK /
 * INSITE_E_*), every argument validated before any HIP call.
 *
 * No workspace.  The kernel needs no scratch memory, so insite_feedback_rules_f64 has no workspace arguments and there
 * is no workspace query: its signature ends in (..., void* stream).  A later version that needs scratch adds a new
 * symbol; this one keeps its signature.
 *
 * Definition.
 *   Trajectories.  insite_effect.h's: the terms with |c| > drop_below are kept, a NaN coefficient makes alpha or beta
 *     of its arm (and the trajectory from the first use of that arm) NaN, one interval is the Euler or RK4 map with
 *     `substeps` sub-steps, and y[r, p, j, k], k = 0..T-1, is the state of row p under replicate r and rule j after
 *     interval k.
 *   Rules.  Rule j is the HOST row rules[4 j .. 4 j + 3] = (arm_on, arm_off, period >= 1, start_on in {0, 1}) and two
 *     thresholds on the device: theta_on = theta[p ld_theta + 2 j], theta_off = theta[p ld_theta + 2 j + 1].
 *     ld_theta == 0: every row shares one [K, 2] table; otherwise ld_theta >= 2 K.  Both arms lie in 0..n_arms-1.
 *   Decision.  With z_k = y0[p] for k = 0 and y[k - 1] otherwise, and on_{-1} = start_on:
 *       k mod period == 0:  on_k = (z_k >= (on_{k-1} ? theta_off : theta_on));
 *       otherwise:          on_k = on_{k-1}.
 *     One ordered comparison: a NaN z_k or a NaN threshold gives off, +-Inf compare as values.  Interval k runs under
 *     arm_k = on_k ? arm_on : arm_off.  theta_off = theta_on is the memoryless rule, theta_off < theta_on is
 *     hysteresis.  The decision is taken inside each replicate, on that replicate's own z_k.
 *   Weights.  The weight of step k for row p is w[p ld_w + k].  ld_w == 0: one shared [T] vector.
 *   Objective.  J[r, p, j] starts at cost[j] (0 when cost is NULL); for k ascending J <- fma(w[p, k], y[k], J) and
 *     then, only when arm_cost is not NULL, J <- J + arm_cost[arm_k] (a separate, rounded addition).  A weight is
 *     always multiplied: a NaN in y reaches J even under weight 0.
 *   Exposure.  E[r, p, j] = #{k < T : on_k}, an exact integer as a double; NaN if any y[k], k < T, of that replicate
 *     and rule is NaN.
 *   Choice, votes, regret.  insite_regimen.h's, over the K rules: s = sense (+1 minimise, -1 maximise), sJ = s J;
 *     replicate r abstains for row p if any of its K objectives is NaN; otherwise best[r, p] is the smallest j that
 *     attains min_j sJ by a strict comparison in ascending j (+-Inf compare as values); the regret
 *     g[r, p, j] = sJ[r, p, j] - sJ[r, p, best] is >= 0, exactly +0 for the winner and NaN for every j of an abstaining
 *     replicate.
 *   Outputs.
 *     choice[p] = best[0, p], the point model's rule; -1 if replicate 0 abstains.
 *     win[p, j] = votes_j / (R - 1), votes_j = #{r >= 1 : best[r, p] = j}: an exact integer count, divided once.
 *     out[p, j, 0, :] = the statistics of J[., p, j];  out[p, j, 1, :] = those of g[., p, j];  out[p, j, 2, :] = those
 *       of E[., p, j].  Row p holds [K, 3, 3 + Q] contiguously.
 *     sched[p ld_sched + j T + k] = arm_k of the point model (replicate 0) under rule j, k = 0..T-1; written only when
 *       sched is not NULL.  Fed back as per-row plans to insite_effect_bands_f64 or insite_regimen_choice_f64 it gives
 *       the trajectory bands of the realised schedule.
 *   Statistics over r and the NaN rule are insite_effect.h's, with v[r] the series and n = R - 1: stat 0 = v[0], the
 *     point model; stat 1 = the mean over 1..R-1 (shifted by v[1]); stat 2 = the two-pass standard deviation with
 *     ddof = 1 (NaN when n = 1); stats 3.. = the quantiles q[j] in the caller's order, by the interpolation formula
 *     stated there.  If any of v[1..R-1] is NaN, every statistic but the point value is NaN.
 *   Untouched memory.  out[p, e] for e >= K 3 (3 + Q) and sched[p, e] for e >= K T (the padding up to ld_out and
 *     ld_sched) are not written; nothing of w past column T - 1 and nothing of theta past column 2 K - 1 is read.
 *   Reproducibility.  Every reduction runs in a fixed order: two calls give bitwise equal outputs.  Rows are
 *     independent: a shard of the rows needs no collective.  Under theta_on = theta_off = -Inf (always on) or +Inf
 *     with start_on = 0 (always off) and arm_cost NULL, choice, win and the series 0 and 1 are
 *     insite_regimen_choice_f64's under the constant plans arm_on (arm_off), bit for bit.
 */
#ifndef INSITE_FEEDBACK_H_
#define INSITE_FEEDBACK_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_FEEDBACK_ABI_VERSION 1

/* Replicates per call (the point model included); more: INSITE_E_UNSUPPORTED.  The cap is insite_regimen.h's: one wave
 * holds a row's R objectives, 8 per lane at 512. */
#define INSITE_FEEDBACK_MAX_REPLICATES 512
#define INSITE_FEEDBACK_MAX_QUANTILES 16
/* Rules per call: the objectives of K - 1 rules wait in one wave's LDS until the minimum is known. */
#define INSITE_FEEDBACK_MAX_RULES 16

#define INSITE_FEEDBACK_MINIMIZE 1
#define INSITE_FEEDBACK_MAXIMIZE (-1)

int32_t insite_feedback_abi_version(void);

/* The rules of one cohort (or shard: rows are independent).
 *   y0, u, coef, exps (HOST), n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below, n_replicates,
 *   q (HOST), n_quantiles: insite_regimen_choice_f64's, with 2 <= n_replicates <= INSITE_FEEDBACK_MAX_REPLICATES
 *   (more: INSITE_E_UNSUPPORTED) and 1 <= n_quantiles <= INSITE_FEEDBACK_MAX_QUANTILES
 *   theta    f64 (device); ld_theta == 0 (one shared [n_rules, 2] table) or ld_theta >= 2 n_rules
 *   rules    i32 HOST [n_rules, 4]: (arm_on, arm_off, period, start_on), 1 <= n_rules <= INSITE_FEEDBACK_MAX_RULES
 *   w        f64; ld_w == 0 (one shared [T] vector) or ld_w >= T
 *   cost     f64 (device) [n_rules] or NULL (zeros)
 *   arm_cost f64 HOST [n_arms] or NULL (no per-step cost: the addition is not made)
 *   sense    INSITE_FEEDBACK_MINIMIZE (+1) or INSITE_FEEDBACK_MAXIMIZE (-1)
 *   choice   i32 [n_rows];  win f64 [n_rows, n_rules];  out f64 [n_rows, ld_out >= n_rules 3 (3 + n_quantiles)]
 *   sched    i8 [n_rows, ld_sched >= n_rules T] or NULL (not written; ld_sched is then not looked at)
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0,
 * n_replicates < 2, n_quantiles outside its range, q NULL or a q[j] NaN or outside [0, 1], an invalid table, n_rules
 * outside 1..INSITE_FEEDBACK_MAX_RULES, rules NULL, a rule with an arm outside 0..n_arms-1, a period < 1 or a start_on
 * other than 0 / 1, a sense other than +1 / -1, a negative leading dimension, a leading dimension below the bounds
 * above, leading dimensions whose largest element offset does not fit int64, and (when n_rows > 0) a NULL y0, theta, w,
 * coef, choice, win or out, or a NULL u with n_statics > 0.  n_rows = 0 is a successful no-op: nothing is written. */
int32_t insite_feedback_rules_f64(const double* y0, const double* u, const double* theta, int64_t ld_theta,
                                  const int32_t* rules, int32_t n_rules, const double* w, int64_t ld_w,
                                  const double* cost, const double* arm_cost, int32_t sense, const double* coef,
                                  const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                                  int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const double* q, int32_t n_quantiles, int32_t* choice,
                                  double* win, double* out, int64_t ld_out, int8_t* sched, int64_t ld_sched,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_FEEDBACK_H_ */
