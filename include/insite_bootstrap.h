/*
 * insite_bootstrap.h — patient-level Poisson bootstrap of the discovered equations: an extension of the C ABI of
 * libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_BOOTSTRAP_ABI_VERSION) so that the pinned surfaces
 * of insite_hip.h, insite_irregular.h and insite_weak.h do not move.  The symbols live in the same shared library.
 *
 * All three Gram passes (insite_gram_moments_f64, insite_gram_irregular_f64, insite_gram_weak_f64) emit every
 * patient's five moments, and the Gram system of a resampled cohort is a weighted sum of per-patient contributions.
 * R bootstrap replicates are therefore one [R x N] . [N x entries] product; the weights are generated on chip and
 * never exist in memory.  DESIGN.md §9g.
 *
 * Conventions are insite_hip.h's: device pointers to caller-owned memory (exps: host), row-major, caller-owned
 * workspace sized by the *_workspace_bytes query (its first 512 bytes zero before the first use; every call leaves
 * them zero), asynchronous on the caller's stream, int32 status (INSITE_OK / INSITE_E_*), every argument validated
 * before any HIP call.
 *
 * Definition.  mom [N, 5] has the layout of insite_gram_moments_f64 (slot 0 = count, sum x, sum x^2, sum x_dot,
 * sum x_dot x).  With m_j(u) the u-monomial of column j and e_j in {0, 1} its state exponent, patient p contributes
 *     g_p[i,k] = m_i m_k mom_p[e_i + e_k],        h_p[i] = m_i mom_p[3 + e_i]
 * to arm arm[p] iff 0 <= arm[p] < n_arms and (rows is NULL or rows[p] >= min_rows).  Any other patient contributes
 * nothing (a select, never a multiplication by zero: NaN moments of such a patient reach no output).
 *
 * Weights (Poisson(1) bootstrap, counter-based).  Replicate 0 has weight 1 for every patient: it is the point
 * estimate.  For replicate r >= 1 and the global patient index g = patient_offset + p, with q = g >> 1:
 *     (a, b) = Threefry-2x32-20(key = (seed, r), counter = (q & 0xffffffff, q >> 32))
 *     v = a if g is even, else b;      w = #{k : v >= T_k},   T_k = floor(2^32 sum_{i <= k} e^-1 / i!),  k = 0..11
 *     T = {1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276,
 *          4294962463, 4294966817, 4294967252, 4294967292}
 * so w is in 0..12 and integer comparisons alone decide it.  patient_offset makes a shard of a cohort draw the
 * weights it has in the whole cohort; the shards' outputs then add up to the whole cohort's, to rounding.
 *
 * Outputs.  G_out [R, n_arms, F, F] (full symmetric), b_out [R, n_arms, F]:
 *     G[r, a] = sum_p w_rp g_p,   b[r, a] = sum_p w_rp h_p   over the contributing patients of arm a,
 * laid out as n_sys = R n_arms systems of insite_stlsq_f64 / insite_sr3_f64.  An arm without weighted patients has
 * G = b = 0.
 */
#ifndef INSITE_BOOTSTRAP_H_
#define INSITE_BOOTSTRAP_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"
#include "insite_weak.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_BOOTSTRAP_ABI_VERSION 1

#define INSITE_BOOT_MAX_REPLICATES 16384 /* replicates per call; more: INSITE_E_UNSUPPORTED */

int32_t insite_bootstrap_abi_version(void);

/* Workspace of insite_bootstrap_gram_f64 / insite_sindy_bootstrap_f64 (0 for invalid arguments). */
size_t insite_bootstrap_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t n_replicates);

/* The R weighted Gram systems of one cohort (or shard) from its per-patient moments.
 *   mom    f64 [n_patients, 5]
 *   u      f64 [n_patients, n_statics] (may be NULL when n_statics = 0)
 *   arm    i8  [n_patients];  rows i32 [n_patients] or NULL (then min_rows is not read)
 *   patient_offset >= 0: the global index of patient 0
 *   exps   i8  [n_terms, 1 + n_statics]  HOST; every table insite_gram_f64 accepts (state exponent <= 1, n_terms <=
 *          INSITE_MAX_TERMS, any static exponents), else INSITE_E_UNSUPPORTED / _INVALID_ARG
 *   1 <= n_replicates <= INSITE_BOOT_MAX_REPLICATES (more: INSITE_E_UNSUPPORTED); seed: any uint32
 *   G_out  f64 [R, n_arms, F, F], b_out f64 [R, n_arms, F] (overwritten)
 * INSITE_E_INVALID_ARG: negative counts or offset, n_replicates < 1, n_arms outside 1..INSITE_MAX_ARMS, NULL outputs
 * (or NULL mom / arm, or NULL u with n_statics > 0, when n_patients > 0).  INSITE_E_WORKSPACE: workspace NULL or too
 * small.  n_patients = 0 is a successful no-op (the outputs are not written).  Deterministic: every reduction runs
 * in a fixed order, two calls give bitwise equal outputs. */
int32_t insite_bootstrap_gram_f64(const double* mom, const double* u, const int8_t* arm, const int32_t* rows,
                                  int32_t min_rows, int64_t n_patients, int64_t patient_offset, int32_t n_statics,
                                  int32_t n_arms, const int8_t* exps, int32_t n_terms, int32_t n_replicates,
                                  uint32_t seed, double* G_out, double* b_out, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* insite_bootstrap_gram_f64 followed on the same stream, without host synchronisation, by the solve of the
 * R n_arms systems:
 *   optimizer INSITE_OPT_SR3:   insite_sr3_f64(G_out, b_out, R n_arms, ..., threshold, nu, tol, max_iter, unbias)
 *   optimizer INSITE_OPT_STLSQ: insite_stlsq_f64(G_out, b_out, R n_arms, ..., threshold, alpha, max_iter, unbias)
 * (INSITE_OPT_* of insite_weak.h; the parameters of the other optimizer are validated as well).  coef_out
 * [R, n_arms, F]; mask_out [R, n_arms, F] int8 and iters_out [R, n_arms] may be NULL.  Additionally
 * INSITE_E_INVALID_ARG for another optimizer value, a NULL coef_out or an invalid solver parameter. */
int32_t insite_sindy_bootstrap_f64(const double* mom, const double* u, const int8_t* arm, const int32_t* rows,
                                   int32_t min_rows, int64_t n_patients, int64_t patient_offset, int32_t n_statics,
                                   int32_t n_arms, const int8_t* exps, int32_t n_terms, int32_t n_replicates,
                                   uint32_t seed, int32_t optimizer, double threshold, double alpha, double nu,
                                   double tol, int32_t max_iter, int32_t unbias, double* G_out, double* b_out,
                                   double* coef_out, int8_t* mask_out, int32_t* iters_out, void* workspace,
                                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_BOOTSTRAP_H_ */
