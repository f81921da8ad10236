/*
 * insite_segboot.h — patient-level Poisson bootstrap of the treatment-segment discovery (cancer_sim / EQ_5): an
 * extension of the C ABI of libinsite_hip.so, versioned on its own (INSITE_SEGBOOT_ABI_VERSION) so that the pinned
 * surfaces of insite_hip.h and of the other extension headers do not move.  The symbols live in the same shared
 * library.  DESIGN.md §9o.
 *
 * On the segment path (insite_gram_segments_f64) a patient's samples are cut into treatment-constant segments and a
 * patient contributes rows to SEVERAL arms.  The resampling unit of the bootstrap is still the patient: replicate r
 * weighs every row of patient p, in every arm, with the same Poisson(1) count w_rp.  insite_bootstrap_gram_f64 takes
 * one arm per patient, and running it on (patient, arm) pairs would draw one weight per pair -- another bootstrap.
 * So the path has two entry points of its own: the per-(patient, arm) moments of the segment cut, and the weighted
 * Gram systems of the replicates from them.
 *
 * Conventions are insite_bootstrap.h's: device pointers to caller-owned memory (exps: host), row-major,
 * caller-owned workspace sized by insite_segboot_workspace_bytes (its first 512 bytes zero before the first use;
 * every call leaves them zero), asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every
 * argument validated before any HIP call, every reduction in a fixed order (two calls give bitwise equal outputs).
 * The workspace arguments stand BEFORE the outputs (as in insite_rulevalue.h) and the stream is last.
 *
 * Moments.  For patient p with L = min(max(seq_len[p], 0), n_steps - 1), the samples x(p, 0..L) and the per-step
 * arms arm(p, 0..L-1) are cut exactly as insite_gram_segments_f64 cuts them (consecutive segments share their
 * boundary sample, which counts once in each; every segment has >= 2 samples), with the derivative of
 * INSITE_FD_ORDER1 (forward differences, backward at a segment's last sample) or INSITE_FD_SMOOTHED1 (the same on
 * the savgol(2, 1)-smoothed segment); the library sees the raw samples in both.  Over the rows that p's segments of
 * arm a hold,
 *     mom_out[p, a, :] = {count, sum x, sum x^2, sum x_dot, sum x_dot x}.
 * An arm the patient never visits (or an arm value outside [0, n_arms)) gives five zeros / reaches nothing.  Samples
 * past L and arms from L on are never used (they may be NaN / arbitrary).
 *
 * Gram.  With m_j(u) the u-monomial of column j and e_j in {0, 1} its state exponent, patient p contributes
 *     g_pa[i,k] = m_i m_k mom[p,a,e_i + e_k],        h_pa[i] = m_i mom[p,a,3 + e_i]
 * to arm a iff mom[p,a,0] > 0 (a select, never a multiplication by zero: NaN moments behind a count of 0 reach no
 * output), and
 *     G[r, a] = sum_p w_rp g_pa,   b[r, a] = sum_p w_rp h_pa.
 * The weights w_rp are insite_bootstrap.h's, word for word: replicate 0 has weight 1 for every patient; for r >= 1
 * and the global index g = patient_offset + p, q = g >> 1,
 *     (a, b) = Threefry-2x32-20(key = (seed, r), counter = (q & 0xffffffff, q >> 32)),  v = a if g is even else b,
 *     w = #{k : v >= T_k} with the twelve thresholds T_k listed there.
 * One integer per (replicate, patient): it multiplies the patient's contribution to every arm.  Shards of a cohort
 * (patient_offset) add up to the whole cohort, to rounding.
 */
#ifndef INSITE_SEGBOOT_H_
#define INSITE_SEGBOOT_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_bootstrap.h"
#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_SEGBOOT_ABI_VERSION 1

int32_t insite_segboot_abi_version(void);

/* Per-(patient, arm) moments of the segment cut.  No workspace.
 *   x        f64 element (p, k) at x[p * ldx + k] (INSITE_LAYOUT_PATIENT_MAJOR, ldx >= n_steps) or x[k * ldx + p]
 *            (INSITE_LAYOUT_TIME_MAJOR, ldx >= n_patients), k < n_steps
 *   arm      int8 element (p, k), k < n_steps - 1, same layout, leading dimension ld_arm (>= n_steps - 1 / >=
 *            n_patients)
 *   seq_len  i32 [n_patients] (clamped to [0, n_steps - 1])
 *   mom_out  f64 [n_patients, n_arms, 5] (overwritten)
 * Statuses, in this order.  INSITE_E_INVALID_ARG: another layout; n_patients < 0, n_arms outside
 * 1..INSITE_MAX_ARMS, dt not > 0, n_steps < 1, ldx < 1, ld_arm < 1, a leading dimension too small for the layout,
 * or (n_patients > 0) a NULL x, arm, seq_len or mom_out.  INSITE_E_UNSUPPORTED: another fd_kind; a leading
 * dimension the 32-bit buffer offsets cannot span (the limit of insite_gram_segments_f64).  n_patients = 0 is a
 * successful no-op. */
int32_t insite_segboot_moments_f64(const double* x, int64_t ldx, const int8_t* arm, int64_t ld_arm, int32_t layout,
                                   int32_t n_steps, const int32_t* seq_len, int64_t n_patients, int32_t n_arms,
                                   int32_t fd_kind, double dt, double* mom_out, void* stream);

/* Workspace of insite_segboot_gram_f64 / insite_segboot_fit_f64 (0 for invalid arguments: n_patients < 0, n_arms
 * outside 1..INSITE_MAX_ARMS, n_terms outside 1..INSITE_MAX_TERMS, n_replicates outside
 * 1..INSITE_BOOT_MAX_REPLICATES). */
size_t insite_segboot_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t n_replicates);

/* The R weighted Gram systems of one cohort (or shard) from its per-(patient, arm) moments.
 *   mom    f64 [n_patients, n_arms, 5]
 *   u      f64 [n_patients, n_statics] (may be NULL when n_statics = 0)
 *   patient_offset >= 0: the global index of patient 0
 *   exps   i8  [n_terms, 1 + n_statics]  HOST; every table insite_bootstrap_gram_f64 accepts
 *   1 <= n_replicates <= INSITE_BOOT_MAX_REPLICATES; seed: any uint32
 *   G_out  f64 [R, n_arms, F, F] (both triangles), b_out f64 [R, n_arms, F] (overwritten): the n_sys = R n_arms
 *          systems of insite_stlsq_f64.  An arm without weighted patients has G = b = 0.
 * Statuses, in this order.  INSITE_E_INVALID_ARG: negative counts or offset, n_replicates < 1, n_arms outside
 * 1..INSITE_MAX_ARMS, NULL outputs, or (n_patients > 0) a NULL mom, or a NULL u with n_statics > 0; then the
 * table's own status (INSITE_E_INVALID_ARG / INSITE_E_UNSUPPORTED for a state exponent above 1);
 * INSITE_E_UNSUPPORTED: n_replicates > INSITE_BOOT_MAX_REPLICATES; INSITE_E_WORKSPACE: workspace NULL or too small
 * (the outputs are not written).  n_patients = 0 is a successful no-op (the outputs are not written). */
int32_t insite_segboot_gram_f64(const double* mom, const double* u, int64_t patient_offset, int64_t n_patients,
                                int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms,
                                int32_t n_replicates, uint32_t seed, void* workspace, size_t workspace_bytes,
                                double* G_out, double* b_out, void* stream);

/* insite_segboot_gram_f64 followed on the same stream, without host synchronisation, by
 * insite_stlsq_f64(G_out, b_out, R n_arms, n_terms, threshold, alpha, max_iter, unbias, ...).  coef_out
 * [R, n_arms, F]; mask_out [R, n_arms, F] int8 and iters_out [R, n_arms] may be NULL.  Checked first:
 * INSITE_E_INVALID_ARG for a NULL coef_out, a negative or NaN threshold or alpha, max_iter < 0. */
int32_t insite_segboot_fit_f64(const double* mom, const double* u, int64_t patient_offset, int64_t n_patients,
                               int32_t n_statics, int32_t n_arms, const int8_t* exps, int32_t n_terms,
                               int32_t n_replicates, uint32_t seed, double threshold, double alpha, int32_t max_iter,
                               int32_t unbias, void* workspace, size_t workspace_bytes, double* G_out, double* b_out,
                               double* coef_out, int8_t* mask_out, int32_t* iters_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_SEGBOOT_H_ */
