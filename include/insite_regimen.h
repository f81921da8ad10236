/*
 * insite_regimen.h — regimen choice: of K candidate treatment plans, which is best for each row, and how sure is the
 * bootstrap ensemble of that.  An extension of the C ABI of libinsite_hip.so (insite_hip.h), versioned on its own
 * (INSITE_REGIMEN_ABI_VERSION) so that the pinned surfaces of insite_hip.h, insite_irregular.h, insite_weak.h,
 * insite_bootstrap.h, insite_effect.h and insite_cohort.h do not move.  The symbols live in the same shared library.
 *
 * For every row (patient) the call rolls the K plans under every replicate of insite_sindy_bootstrap_f64, reduces each
 * trajectory to a scalar objective, takes the argmin inside each replicate -- so model uncertainty stays paired across
 * the plans -- and gives the point model's choice, every plan's share of the replicates' votes, and per plan the
 * objective and the regret as point value, mean, standard deviation and quantiles over the replicates.  "How often
 * does plan j win" is a statistic of the argmin inside the replicate: it cannot be had from per-plan or per-pair
 * quantiles.  The replicate objectives live in one wave's registers and LDS and never exist in memory: n_rows
 * (1 + K + K 2 (3 + Q)) numbers leave the chip.  DESIGN.md §9j.
 *
 * (The plugin says "plan" for a treatment sequence; "regimen" keeps the C names apart from the prepared launches of
 * the Python layer, which are called plans too.)
 *
 * Conventions are insite_effect.h's: device pointers to caller-owned memory (exps and q: HOST arrays), row-major, no
 * allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every
 * argument validated before any HIP call.
 *
 * Definition.
 *   Trajectories.  y_j[r, p, k], k = 0..T-1, is insite_effect.h's trajectory of row p under the replicate's
 *     coefficients coef[r] and the per-step arms of plan j, with every rule stated there: the terms with
 *     |c| > drop_below, a NaN coefficient makes alpha or beta of its arm (and the trajectory from the first use of that
 *     arm) NaN, an arm value outside 1..n_arms-1 selects arm 0.
 *   Plans.  The arm of plan j, row p at step k is plans[j plan_stride + p ld_plan + k].  ld_plan == 0: every row
 *     shares plan j's [T] vector.
 *   Weights.  The weight of step k for row p is w[p ld_w + k].  ld_w == 0: one shared [T] vector.
 *   Objective.  J[r, p, j] = cost[j] + sum_k w[p, k] y_j[r, p, k]: the sum starts at cost[j] (0 when cost is NULL) and
 *     accumulates over k ascending, each step one FMA: J <- fma(w[p, k], y_j[r, p, k], J).  A weight is always
 *     multiplied: a NaN in y reaches J even under weight 0.
 *   Choice inside a replicate.  With s = sense (+1 minimise, -1 maximise) and the signed objective sJ = s J (exact),
 *     replicate r abstains for row p if any of its K objectives is NaN.  Otherwise best[r, p] is the smallest j that
 *     attains min_j sJ[r, p, j]: the comparison is strict (sJ[j] < the running minimum) and runs in ascending j, so
 *     bitwise-equal objectives go to the lower index; +-Inf compare as values.
 *   Regret.  g[r, p, j] = sJ[r, p, j] - sJ[r, p, best] = s (J[r, p, j] - J[r, p, best]): >= 0, exactly +0 for the
 *     winner (with either sense), NaN for every j of an abstaining replicate (and where both objectives are the same
 *     infinity).
 *   Outputs.
 *     choice[p] = best[0, p], the point model's plan; -1 if replicate 0 abstains.
 *     win[p, j] = votes_j / (R - 1), votes_j = #{r >= 1 : best[r, p] = j}: an exact integer count, divided once, in
 *       double.  A row's win sums to 1 minus its abstaining share.
 *     out[p, j, 0, :] = the statistics of J[., p, j] (not negated);  out[p, j, 1, :] = those of g[., p, j].
 *   Statistics over r are insite_effect.h's, with v[r] the series and n = R - 1:
 *     stat 0 = v[0], the point model;
 *     stat 1 = the mean over 1..R-1, evaluated as c + (sum_r (v[r] - c)) / n with the shift c = v[1] (c = 0 when
 *              v[1] is not finite);
 *     stat 2 = the standard deviation with ddof = 1, two-pass: sqrt(sum_r (v[r] - mean)^2 / (n - 1)), NaN when n = 1;
 *     stats 3.. = the quantiles q[j] in the caller's order: with s the ascending sort of v[1..R-1], pos = q (n - 1),
 *              i = floor(pos) clamped to n - 1, g = pos - i (both computed on the host in double),
 *              hi = s[min(i + 1, n - 1)]; the result is s[i] when g == 0 or s[i] == hi, else s[i] + g (hi - s[i]).
 *   NaN.  If any of v[1..R-1] is NaN, the mean, the standard deviation and all quantiles there are NaN; the point
 *     value is not affected.  +-Inf sort as values.  So one abstaining replicate r >= 1 makes every regret statistic
 *     of the row but the point value NaN, and the value statistics of exactly those plans whose objective is NaN in it.
 *   Untouched memory.  out[p, e] for e >= K 2 (3 + Q) (the padding up to ld_out) is not written; nothing of plans or
 *     w past column T - 1 is read.
 *   Reproducibility.  Every reduction runs in a fixed order: two calls give bitwise equal outputs; choice and the
 *     point values do not depend on R or q.  Rows are independent: a shard of the rows needs no collective.
 */
#ifndef INSITE_REGIMEN_H_
#define INSITE_REGIMEN_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_REGIMEN_ABI_VERSION 1

/* Replicates per call (the point model included); more: INSITE_E_UNSUPPORTED.  The cap is insite_effect.h's: one wave
 * holds a row's R objectives, 8 per lane at 512. */
#define INSITE_REGIMEN_MAX_REPLICATES 512
#define INSITE_REGIMEN_MAX_QUANTILES 16
/* Plans per call: the objectives of K - 1 plans wait in one wave's LDS until the minimum is known (60 KiB at 16 plans
 * and 512 replicates). */
#define INSITE_REGIMEN_MAX_PLANS 16

#define INSITE_REGIMEN_MINIMIZE 1
#define INSITE_REGIMEN_MAXIMIZE (-1)

int32_t insite_regimen_abi_version(void);

/* Workspace of insite_regimen_choice_f64: this version needs none and returns 0 for every argument, valid or not (the
 * query exists so that a later version can ask for scratch without a new signature). */
size_t insite_regimen_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                      int32_t n_replicates, int32_t n_quantiles, int32_t n_plans);

/* The choice of one cohort (or shard: rows are independent).
 *   y0, u, coef, exps (HOST), n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below, n_replicates,
 *   q (HOST), n_quantiles: insite_effect_bands_f64's, with 2 <= n_replicates <= INSITE_REGIMEN_MAX_REPLICATES (more:
 *   INSITE_E_UNSUPPORTED) and 1 <= n_quantiles <= INSITE_REGIMEN_MAX_QUANTILES
 *   plans  i8, 1 <= n_plans <= INSITE_REGIMEN_MAX_PLANS; ld_plan == 0 (shared plans): plan_stride >= T; otherwise
 *          ld_plan >= T and plan_stride >= n_rows ld_plan
 *   w      f64; ld_w == 0 (one shared [T] vector) or ld_w >= T
 *   cost   f64 [n_plans] or NULL (zeros)
 *   sense  INSITE_REGIMEN_MINIMIZE (+1) or INSITE_REGIMEN_MAXIMIZE (-1)
 *   choice i32 [n_rows];  win f64 [n_rows, n_plans];  out f64 [n_rows, ld_out >= n_plans 2 (3 + n_quantiles)]: row p
 *          holds [n_plans, 2, 3 + n_quantiles] contiguously
 *   workspace / workspace_bytes: not used by this version (workspace may be NULL)
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0,
 * n_replicates < 2, n_quantiles outside its range, q NULL or a q[j] NaN or outside [0, 1], an invalid table, n_plans
 * outside 1..INSITE_REGIMEN_MAX_PLANS, a sense other than +1 / -1, a negative stride or leading dimension, a stride or
 * leading dimension below the bounds above, strides whose largest element offset does not fit int64, and (when
 * n_rows > 0) a NULL y0, plans, w, coef, choice, win or out, or a NULL u with n_statics > 0.  n_rows = 0 is a
 * successful no-op: nothing is written. */
int32_t insite_regimen_choice_f64(const double* y0, const double* u, const int8_t* plans, int32_t n_plans,
                                  int64_t plan_stride, int64_t ld_plan, const double* w, int64_t ld_w,
                                  const double* cost, int32_t sense, const double* coef, const int8_t* exps,
                                  int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                  double dt, int32_t method, int32_t substeps, double drop_below,
                                  int32_t n_replicates, const double* q, int32_t n_quantiles, int32_t* choice,
                                  double* win, double* out, int64_t ld_out, void* workspace, size_t workspace_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_REGIMEN_H_ */
