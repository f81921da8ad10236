/*
 * insite_cohort.h — cohort and subgroup average treatment effects (ATE / CATE) with bootstrap bands: an extension of
 * the C ABI of libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_COHORT_ABI_VERSION) so that the pinned
 * surfaces of insite_hip.h, insite_irregular.h, insite_weak.h, insite_bootstrap.h and insite_effect.h do not move.
 * The symbols live in the same shared library.
 *
 * For every group of rows (patients) and step the call gives the weighted mean trajectory of the group under plan A,
 * under plan B and the effect A - B, each as the point model's value plus mean, standard deviation and quantiles over
 * the R - 1 resampled replicates of insite_sindy_bootstrap_f64.  Replicate r averages its own trajectories with its
 * own patient weights (the Poisson weights its refit used), so model and sampling uncertainty stay paired inside the
 * replicate.  The replicate trajectories never exist in memory: the lane that rolls a trajectory adds it to the
 * group's sum.  DESIGN.md §9i.
 *
 * Conventions are insite_effect.h's: device pointers to caller-owned memory (exps and q: HOST arrays), row-major, no
 * allocation inside the library, asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every
 * argument validated before any HIP call.
 *
 * Definition.
 *   Trajectories.  yA[r, p, k] and yB[r, p, k], k = 0..T-1, are insite_effect.h's trajectories of row p under the
 *     replicate's coefficients coef[r] and the per-step arms arm_a[p, :] / arm_b[p, :], with every rule stated there:
 *     the terms with |c| > drop_below, a NaN coefficient makes alpha or beta of its arm (and the trajectory from the
 *     first use of that arm) NaN, an arm value outside 1..n_arms-1 selects arm 0.
 *   Weights.  INSITE_COHORT_WEIGHT_NONE: w[r, p] = 1.  INSITE_COHORT_WEIGHT_POISSON: the weights of
 *     insite_bootstrap.h, verbatim: w[0, p] = 1; for r >= 1 and the global patient index g = patient_offset + p the
 *     word v = (a if g is even else b) of Threefry-2x32-20 under the key (seed, r) and the counter
 *     (q & 0xffffffff, q >> 32), q = g >> 1, counted against the twelve thresholds T_k of that header:
 *     w = #{k : v >= T_k}.
 *   Groups.  Row p contributes to group group[p] iff 0 <= group[p] < n_groups (group NULL: every row is in group 0).
 *     A row outside that range, and a row whose weight is 0 in replicate r, contributes nothing to (that replicate
 *     of) any output, by a select and not by a multiplication by zero: its y0 and u may be NaN.
 *   Sums.  With s = A, B and the contributing rows p of group g:
 *       sums[r, g, s, k] = sum_p w[r, p] ys[r, p, k],      wsum[r, g] = sum_p w[r, p]
 *     (wsum is a sum of small integers: exact).  Both are additive over the shards of a cohort; patient_offset makes
 *     a shard draw the weights it has inside the whole cohort.
 *   Means.  m[r, g, s, k] = sums[r, g, s, k] / wsum[r, g]: 0 / 0 = NaN when replicate r drew no row of group g.
 *     m[r, g, effect, k] = m[r, g, A, k] - m[r, g, B, k]: paired within the replicate.
 *   Series.  n_series = 1 (A only) when arm_b is NULL, else 2 in `sums` (A, B) and 3 in `out` (A, B, A - B).
 *   Statistics over r, per (g, series, k), are insite_effect.h's, with v[r] = m[r, g, series, k] and n = R - 1:
 *     stat 0 = v[0], the point model;
 *     stat 1 = the mean over 1..R-1, evaluated as c + (sum_r (v[r] - c)) / n with the shift c = v[1] (c = 0 when
 *              v[1] is not finite);
 *     stat 2 = the standard deviation with ddof = 1, two-pass: sqrt(sum_r (v[r] - mean)^2 / (n - 1)), NaN when n = 1;
 *     stats 3.. = the quantiles q[j] in the caller's order: with s the ascending sort of v[1..R-1], pos = q (n - 1),
 *              i = floor(pos) clamped to n - 1, g = pos - i (both computed on the host in double),
 *              hi = s[min(i + 1, n - 1)]; the result is s[i] when g == 0 or s[i] == hi, else s[i] + g (hi - s[i]).
 *   NaN.  If any of v[1..R-1] is NaN, the mean, the standard deviation and all quantiles there are NaN; the point
 *     row is not affected.  +-Inf sort as values.
 *   Untouched memory.  sums[.., k] and out[.., k] for k >= T (the padding up to ld_sums / ld_out) are not written,
 *     and nothing of arm_a / arm_b past column T - 1 is read.
 *   Reproducibility.  Every reduction runs in a fixed order (a lane's rows ascending, the patient chunks in chunk
 *     order, the statistics in a fixed tree): two calls give bitwise equal outputs, and the point rows do not depend
 *     on R, q, the weighting or the seed.
 */
#ifndef INSITE_COHORT_H_
#define INSITE_COHORT_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_COHORT_ABI_VERSION 1

/* Replicates per call (the point model included); more: INSITE_E_UNSUPPORTED.  The cap is the finalize kernel's sort
 * (the keys of one series in one block's LDS). */
#define INSITE_COHORT_MAX_REPLICATES 4096
#define INSITE_COHORT_MAX_GROUPS 64
#define INSITE_COHORT_MAX_QUANTILES 16

#define INSITE_COHORT_WEIGHT_NONE 0
#define INSITE_COHORT_WEIGHT_POISSON 1

int32_t insite_cohort_abi_version(void);

/* Bytes of workspace insite_cohort_effect_sums_f64 / insite_cohort_effect_f64 need for this shape: the partial sums
 * of the patient chunks.  The number of chunks is bounded by the workspace, so the result is below 1 GiB for every
 * accepted shape.  Returns 0 for invalid arguments (those calls' rules for n_rows, T, n_arms, n_terms, n_replicates,
 * n_groups), for n_rows = 0, and for a shape whose single-chunk partial -- n_groups x ceil(n_replicates / 64) x 64
 * x (2 T + 1) doubles, the size of `sums` itself padded to 64 replicates -- does not fit 1 GiB: the calls refuse
 * that shape with INSITE_E_UNSUPPORTED. */
size_t insite_cohort_effect_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms,
                                            int32_t n_replicates, int32_t n_groups);

/* The weighted sums of one cohort (or shard).
 *   y0, u, arm_a / ld_arm_a, arm_b / ld_arm_b (or NULL), coef, exps (HOST), n_terms, n_rows, T, n_statics, n_arms,
 *   dt, method, substeps, drop_below, n_replicates: insite_effect_bands_f64's, with
 *   2 <= n_replicates <= INSITE_COHORT_MAX_REPLICATES (more: INSITE_E_UNSUPPORTED)
 *   group   i32 [n_rows] or NULL (every row in group 0);  1 <= n_groups <= INSITE_COHORT_MAX_GROUPS
 *   weighting  INSITE_COHORT_WEIGHT_NONE / _POISSON;  seed, patient_offset (>= 0): read only under _POISSON
 *   sums    f64 [n_replicates, n_groups, n_series, ld_sums >= T], n_series = 1 (arm_b NULL) or 2;  overwritten
 *   wsum    f64 [n_replicates, n_groups];  overwritten
 *   workspace / workspace_bytes: at least insite_cohort_effect_workspace_bytes(...) bytes, 8-byte aligned; needs no
 *           initialisation and carries nothing between calls
 * INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS, substeps < 1, dt not >= 0, a leading
 * dimension below T, n_replicates < 2, n_groups outside its range, an unknown weighting, patient_offset < 0, an
 * invalid table, and (when n_rows > 0) a NULL y0, arm_a, coef, sums or wsum, a NULL u with n_statics > 0, a NULL or
 * too small workspace.  n_rows = 0 is a successful no-op: sums and wsum are not written. */
int32_t insite_cohort_effect_sums_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                      const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                      int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                      double dt, int32_t method, int32_t substeps, double drop_below,
                                      int32_t n_replicates, const int32_t* group, int32_t n_groups, int32_t weighting,
                                      uint32_t seed, int64_t patient_offset, double* sums, int64_t ld_sums,
                                      double* wsum, void* workspace, size_t workspace_bytes, void* stream);

/* The statistics of the means from (all-reduced) sums.
 *   sums  f64 [n_replicates, n_groups, n_series, ld_sums >= T], n_series = 1 or 2;  wsum f64 [n_replicates, n_groups]
 *   q     f64 [n_quantiles] HOST, 1 <= n_quantiles <= INSITE_COHORT_MAX_QUANTILES, each in [0, 1], any order
 *   out   f64 [n_groups, S, 3 + n_quantiles, ld_out >= T], S = 1 (n_series = 1) or 3 (A, B, A - B)
 * INSITE_E_INVALID_ARG: NULL sums, wsum, q or out, n_replicates < 2, n_groups or n_quantiles outside their ranges,
 * n_series not 1 or 2, T < 1, a leading dimension below T, a q[j] NaN or outside [0, 1].  INSITE_E_UNSUPPORTED:
 * n_replicates > INSITE_COHORT_MAX_REPLICATES. */
int32_t insite_cohort_effect_finalize_f64(const double* sums, int64_t ld_sums, const double* wsum,
                                          int32_t n_replicates, int32_t n_groups, int32_t n_series, int32_t T,
                                          const double* q, int32_t n_quantiles, double* out, int64_t ld_out,
                                          void* stream);

/* insite_cohort_effect_sums_f64 followed on the stream by insite_cohort_effect_finalize_f64, without host
 * synchronisation; sums and wsum are outputs of the caller's.  Every argument rule of the two holds (a NULL out is
 * INSITE_E_INVALID_ARG whatever n_rows); n_rows = 0 is a successful no-op: nothing is written. */
int32_t insite_cohort_effect_f64(const double* y0, const double* u, const int8_t* arm_a, int64_t ld_arm_a,
                                 const int8_t* arm_b, int64_t ld_arm_b, const double* coef, const int8_t* exps,
                                 int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics, int32_t n_arms,
                                 double dt, int32_t method, int32_t substeps, double drop_below, int32_t n_replicates,
                                 const int32_t* group, int32_t n_groups, int32_t weighting, uint32_t seed,
                                 int64_t patient_offset, double* sums, int64_t ld_sums, double* wsum, const double* q,
                                 int32_t n_quantiles, double* out, int64_t ld_out, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_COHORT_H_ */
