/*
 * insite_effect.h — paired treatment-effect bands over a bootstrap ensemble: an extension of the C ABI of
 * libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_EFFECT_ABI_VERSION) so that the pinned surfaces of
 * insite_hip.h, insite_irregular.h, insite_weak.h and insite_bootstrap.h do not move.  The symbols live in the same
 * shared library.
 *
 * For every row (patient) and step the call gives the counterfactual trajectory under plan A, under plan B and the
 * effect A - B, each as the point model's value plus mean, standard deviation and quantiles over the R - 1 resampled
 * replicates of insite_sindy_bootstrap_f64.  The replicate trajectories live in one wave's registers and never exist
 * in memory: only n_rows T (3 + Q) numbers per series leave the chip.  DESIGN.md §9h.
 *
 * Conventions are insite_bootstrap.h's: device pointers to caller-owned memory (exps and q: HOST arrays), row-major,
 * no allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every
 * argument validated before any HIP call.
 *
 * Definition.
 *   Trajectories.  For row p and replicate r, yA[r, k], k = 0..T-1, is insite_rollout_f64's trajectory of row p
 *     (y0[p], u[p, :]) under the per-step arms arm_a[p, :] with the coefficients coef[r] ([n_arms, F]): the
 *     right-hand side over the terms with |c| > drop_below, INSITE_METHOD_EULER / _RK4 with `substeps` sub-steps per
 *     interval, the state after interval k; an arm value outside 1..n_arms-1 selects arm 0, as there.  One rule
 *     differs: a NaN coefficient is not a dropped term (insite_rollout_f64's comparison drops it) but makes alpha or
 *     beta of its arm NaN, so a replicate whose refit failed gives a NaN trajectory on the steps after that arm is
 *     first used and cannot pass for a zero model.  yB is the same under arm_b, and d[r, k] = yA[r, k] - yB[r, k]:
 *     the difference is paired within the replicate.
 *   Series.  n_series = 1 (A only) when arm_b is NULL, else 3 in the order A, B, A - B.
 *   Statistics.  For a series v at (p, k), with n = R - 1 resampled values v[1..R-1]:
 *     stat 0 = v[0], the point model;
 *     stat 1 = the mean over 1..R-1, evaluated as c + (sum_r (v[r] - c)) / n with the shift c = v[1] (c = 0 when
 *              v[1] is not finite): equal to the plain mean to rounding, and exactly v[1] when all values are equal;
 *     stat 2 = the standard deviation with ddof = 1, two-pass: sqrt(sum_r (v[r] - mean)^2 / (n - 1)), NaN when n = 1;
 *     stats 3.. = the quantiles q[j], j = 0..Q-1, in the caller's order.
 *   Quantile.  With s the ascending sort of v[1..R-1]: pos = q (n - 1), i = floor(pos) clamped to n - 1, g = pos - i
 *     (both computed on the host in double), hi = s[min(i + 1, n - 1)]; the result is s[i] when g == 0 or s[i] == hi,
 *     else s[i] + g (hi - s[i]).  This is torch.quantile's linear interpolation up to rounding.
 *   NaN.  If any of v[1..R-1] at (p, k) is NaN, the mean, the standard deviation and all quantiles there are NaN
 *     (torch.quantile's behaviour); the point row is not affected.  +-Inf sort as values.
 *   Untouched memory.  out[.., p, k] for k >= T (the padding up to ld_out) is not written, and nothing of arm_a /
 *     arm_b past column T - 1 is read.
 *   Reproducibility.  Every reduction runs in a fixed order: two calls give bitwise equal outputs, and the point rows
 *     do not depend on R or q.
 */
#ifndef INSITE_EFFECT_H_
#define INSITE_EFFECT_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_EFFECT_ABI_VERSION 1

/* Replicates per call (the point model included); more: INSITE_E_UNSUPPORTED.  The cap is the register budget of
 * this version's kernel (one wave holds a row's R trajectories of both plans, 8 per lane at 512), not a principle. */
#define INSITE_EFFECT_MAX_REPLICATES 512
#define INSITE_EFFECT_MAX_QUANTILES 16

int32_t insite_effect_abi_version(void);

/* Workspace of insite_effect_bands_f64: this version needs none and returns 0 for every argument, valid or not (the
 * query exists so that a later version can ask for scratch without a new signature). */
size_t insite_effect_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                     int32_t n_replicates, int32_t n_quantiles);

/* The bands of one cohort (or shard: rows are independent).
 *   y0     f64 [n_rows];  u f64 [n_rows, n_statics] (may be NULL when n_statics = 0)
 *   arm_a  i8  [n_rows, ld_arm_a >= T] patient-major;  arm_b the same with ld_arm_b, or NULL (then ld_arm_b is not read)
 *   coef   f64 [n_replicates, n_arms, n_terms]: replicate 0 = the point model; shared by all rows
 *   exps   i8  [n_terms, 1 + n_statics]  HOST; the tables insite_bootstrap_gram_f64 accepts (state exponent <= 1,
 *          n_terms <= INSITE_MAX_TERMS), else INSITE_E_UNSUPPORTED / _INVALID_ARG
 *   dt, method, substeps, drop_below: insite_rollout_f64's (method other than Euler / RK4: INSITE_E_UNSUPPORTED)
 *   2 <= n_replicates <= INSITE_EFFECT_MAX_REPLICATES (more: INSITE_E_UNSUPPORTED)
 *   q      f64 [n_quantiles] HOST, 1 <= n_quantiles <= INSITE_EFFECT_MAX_QUANTILES, each in [0, 1], any order,
 *          repeats allowed
 *   out    f64 [n_series, 3 + n_quantiles, n_rows, ld_out >= T]
 *   workspace / workspace_bytes: not used by this version (workspace may be NULL)
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0, a leading
 * dimension below T, n_replicates < 2, n_quantiles outside its range, q NULL or a q[j] NaN or outside [0, 1], an
 * invalid table, and (when n_rows > 0) a NULL y0, arm_a, coef or out, or a NULL u with n_statics > 0.  n_rows = 0 is
 * a successful no-op. */
int32_t insite_effect_bands_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                double dt, int32_t method, int32_t substeps, double drop_below,
                                int32_t n_replicates, const double* q, int32_t n_quantiles, double* out,
                                int64_t ld_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_EFFECT_H_ */
