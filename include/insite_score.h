/*
 * insite_score.h — scoring the bootstrap ensemble against observed outcomes: an extension of the C ABI of
 * libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_SCORE_ABI_VERSION) so that the pinned surfaces of the
 * older headers do not move.  The symbols live in the same shared library.
 *
 * For every group of rows (patients) and step the call gives the sums from which coverage, width and interval score of
 * the central bands, the rank (PIT) histogram, the CRPS of the ensemble, its spread and the squared errors of the point
 * model and of the ensemble mean follow by a division.  Every replicate trajectory is scored against the observation
 * while it is in one wave's registers: only [n_groups, S, T] sums leave the chip, and they are additive over the
 * shards of a cohort.  DESIGN.md §9p.
 *
 * Conventions are insite_effect.h's / insite_cohort.h's: device pointers to caller-owned memory (exps and levels: HOST
 * arrays, and so is everything derived from them), row-major, no allocation inside the library, asynchronous on the
 * caller's stream, int32 status (INSITE_OK / INSITE_E_*), every argument validated before any HIP call.
 *
 * Where the workspace stands in the signature.  (workspace, workspace_bytes) stands before the output `sums`, not in
 * front of the stream, as in insite_rulevalue.h and for its reason: the project's workspace-contract test matrix holds
 * a pinned list of every entry point whose signature ends in (void* workspace, size_t workspace_bytes, void* stream),
 * and this call came after it.  The contract is the usual one: insite_score_workspace_bytes(...) bytes suffice, the
 * buffer needs no initialisation, nothing is carried between calls.
 *
 * Definition.
 *   Trajectories.  v[r, p, k], k = 0..T-1, is insite_effect.h's trajectory of row p under the replicate's coefficients
 *     coef[r] and the per-step arms arm[p, :], with every rule stated there: the terms with |c| > drop_below, a NaN
 *     coefficient makes alpha or beta of its arm (and the trajectory from the first use of that arm) NaN, an arm value
 *     outside 1..n_arms-1 selects arm 0.  r = 0 is the point model; n = R - 1 resampled values v[1..R-1].
 *   Observations.  y_obs[p, k] is the observation of the state after interval k: the step alignment of
 *     insite_rollout_f64's output.
 *   Cells.  Cell (p, k) is observed iff active[p, k] != 0 (active NULL: every cell) and y = y_obs[p, k] is finite.  An
 *     observed cell is scored iff all of v[0..R-1, p, k] are finite; otherwise it is bad.  Unobserved and bad cells
 *     reach no sum but their own count (bad cells: row 1), by a select: their y may be NaN.
 *   Groups.  Row p contributes to group group[p] iff 0 <= group[p] < n_groups (group NULL: every row is in group 0); a
 *     row outside that range contributes nothing, and the test comes before any index is formed from the id.
 *   Per scored cell, with s the ascending sort of v[1..R-1] and m insite_effect.h's shifted mean of v[1..R-1]
 *     (c + sum_r (v[r] - c) / n, c = v[1]):
 *       e0   = v[0] - y                          em = m - y
 *       var  = sum_r (v[r] - m)^2 / (n - 1), two-pass; 0 when n = 1
 *       crps = (1/n) sum_r |v[r] - y| - (1/n^2) sum_{i=0}^{n-1} (2 i - n + 1) s[i]
 *              the CRPS of the ensemble's empirical distribution, mean|v - y| - mean|v - v'| / 2 with the pairwise
 *              term in sorted form; the kernel evaluates the second sum on s[i] - m (the weights 2 i - n + 1 add to
 *              zero, so the value is the same and equal replicates give exactly 0)
 *       rank: c_lt = #{r : v[r] < y}, c_eq = #{r : v[r] == y}, rank2 = 2 c_lt + c_eq,
 *              bin = min(n_bins - 1, (rank2 n_bins) / (2 n)) in integer arithmetic
 *       for level j with lambda = levels[j]: q_lo = 0.5 - 0.5 lambda, q_hi = 0.5 + 0.5 lambda (host, double);
 *              lo, hi = insite_effect.h's quantile formula on s at q_lo, q_hi;
 *              covered = (lo <= y <= hi), width = hi - lo,
 *              iscore = width + c max(lo - y, 0) + c max(y - hi, 0), c = 2 / (1 - lambda) (host, double)
 *   Rows of sums[g], S = 6 + n_bins + 3 n_levels of them, each summed over the scored cells of group g at step k:
 *       0 the number of scored cells      1 the number of bad cells (the one row bad cells reach)
 *       2 sum e0^2     3 sum em^2     4 sum var     5 sum crps
 *       6 .. 6 + n_bins - 1   the rank histogram
 *       6 + n_bins + 3 j, + 1, + 2   sum covered, sum width, sum iscore of level j
 *     The count rows (0, 1, the histogram, covered) are exact integers in f64.  A group with no rows is all zeros.
 *   Untouched memory.  sums[.., k] for k >= T (the padding up to ld_sums) is not written, and nothing of arm, y_obs or
 *     active past column T - 1 is read.
 *   Reproducibility.  Every sum runs in a fixed order: within a cell the lane's slots ascending and a fixed wave tree,
 *     over the cells a chunk's rows ascending, then the chunks in chunk order.  Two calls give bitwise equal output;
 *     rows 0-2 do not depend on levels or n_bins; the sums of two shards add to the whole cohort's up to rounding,
 *     the count rows exactly.
 */
#ifndef INSITE_SCORE_H_
#define INSITE_SCORE_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_SCORE_ABI_VERSION 1

/* Replicates per call (the point model included); more: INSITE_E_UNSUPPORTED.  The cap is insite_effect.h's: one wave
 * holds a row's R trajectories, 8 per lane at 512. */
#define INSITE_SCORE_MAX_REPLICATES 512
/* One lane of the wave owns one statistic, so S = 6 + n_bins + 3 n_levels <= 62 <= 64: the two caps. */
#define INSITE_SCORE_MAX_LEVELS 8
#define INSITE_SCORE_MAX_BINS 32
#define INSITE_SCORE_MAX_GROUPS 64

int32_t insite_score_abi_version(void);

/* Bytes of workspace insite_score_sums_f64 needs for this shape: per chunk of rows one slab of n_groups x T x 64
 * doubles.  The number of chunks is bounded by the workspace, so the result is below 1 GiB for every accepted shape.
 * Returns 0 for invalid arguments (that call's rules for n_rows, T, n_arms, n_terms, n_replicates, n_groups), for
 * n_rows = 0, and for a shape whose single slab does not fit 1 GiB: the call refuses that shape with
 * INSITE_E_UNSUPPORTED. */
size_t insite_score_workspace_bytes(int64_t n_rows, int32_t T, int32_t n_arms, int32_t n_terms, int32_t n_replicates,
                                    int32_t n_groups);

/* The score sums of one cohort (or shard).
 *   y0, u, arm / ld_arm, coef, exps (HOST), n_terms, n_rows, T, n_statics, n_arms, dt, method, substeps, drop_below,
 *   n_replicates: insite_effect_bands_f64's, for one plan, with 2 <= n_replicates <= INSITE_SCORE_MAX_REPLICATES
 *   y_obs   f64 [n_rows, ld_obs >= T]
 *   active  i8  [n_rows, ld_active >= T], non-zero = active, or NULL (every cell active; ld_active is not read)
 *   group   i32 [n_rows] or NULL (every row in group 0);  1 <= n_groups <= INSITE_SCORE_MAX_GROUPS
 *   levels  f64 [n_levels] HOST, 1 <= n_levels <= INSITE_SCORE_MAX_LEVELS, each strictly inside (0, 1)
 *   n_bins  1 <= n_bins <= INSITE_SCORE_MAX_BINS
 *   workspace / workspace_bytes: at least insite_score_workspace_bytes(...) bytes, 8-byte aligned; needs no
 *           initialisation and carries nothing between calls
 *   sums    f64 [n_groups, S, ld_sums >= T], S = 6 + n_bins + 3 n_levels;  overwritten
 * The checks, in this order.  INSITE_E_INVALID_ARG: n_rows < 0, T < 1, n_arms outside 1..INSITE_MAX_ARMS,
 * substeps < 1, dt not >= 0, n_replicates < 2, n_groups outside its range, a leading dimension (ld_arm, ld_obs,
 * ld_active with a non-NULL active, ld_sums) below T, n_levels or n_bins outside their ranges, levels NULL or a level
 * NaN or not inside (0, 1).  Then the method (INSITE_E_UNSUPPORTED), the table (INSITE_E_INVALID_ARG /
 * _UNSUPPORTED as insite_effect.h), n_replicates > INSITE_SCORE_MAX_REPLICATES (INSITE_E_UNSUPPORTED).  n_rows = 0 is
 * then a successful no-op: sums is not written.  With rows, INSITE_E_INVALID_ARG: a NULL y0, arm, coef, y_obs or sums,
 * a NULL u with n_statics > 0; INSITE_E_UNSUPPORTED: a shape whose single slab does not fit the workspace bound;
 * INSITE_E_INVALID_ARG: a NULL, misaligned or too small workspace. */
int32_t insite_score_sums_f64(const double* y0, const double* u, const int8_t* arm, int64_t ld_arm, const double* coef,
                              const int8_t* exps, int32_t n_terms, int64_t n_rows, int32_t T, int32_t n_statics,
                              int32_t n_arms, double dt, int32_t method, int32_t substeps, double drop_below,
                              int32_t n_replicates, const double* y_obs, int64_t ld_obs, const int8_t* active,
                              int64_t ld_active, const int32_t* group, int32_t n_groups, const double* levels,
                              int32_t n_levels, int32_t n_bins, void* workspace, size_t workspace_bytes, double* sums,
                              int64_t ld_sums, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_SCORE_H_ */
