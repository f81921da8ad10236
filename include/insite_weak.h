/*
 * insite_weak.h — weak-form SINDy discovery (test-function projections + SR3): an extension of the C ABI of
 * libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_WEAK_ABI_VERSION) so that the pinned surface
 * of insite_hip.h does not move.  The symbols live in the same shared library.
 *
 * Reference interface replaced: the `wsindy` backbone of libs_m/ct/src/models/sindy.py:218-239,
 * pysindy SINDy(SR3(thresholder="l1", normalize_columns=True), WeakPDELibrary(K=100)).fit(...): the
 * finite-difference derivative of the strong form is replaced by integrals of the trajectory against K
 * compactly supported test functions.
 *
 * Conventions are insite_hip.h's: device pointers to caller-owned memory (exps: host), row-major, leading
 * dimensions in elements, caller-owned workspace sized by the *_workspace_bytes query (its first 512 bytes
 * zero before the first use; every call leaves them zero), asynchronous on the caller's stream, int32 status
 * (INSITE_OK / INSITE_E_*), every argument validated before any HIP call.
 *
 * Definition.  The grid is uniform, t_i = i dt, i = 0..T-1.  The caller passes two dense weight matrices
 * W, D [K, ldw] (row k: the quadrature weights of test function k and of its derivative on the grid; zero
 * outside its support).  insite_amd.weak.test_function_weights builds the default pair,
 *     W[k,i] = dt (1 - tau^2)^p,   D[k,i] = dt (-2 p tau (1 - tau^2)^(p-1)) / H,   tau = (t_i - c_k) / H,
 * for |t_i - c_k| <= H; any other test function or quadrature can be passed.  For a patient p with all T
 * samples (rows[p] >= T), arm a = arm[p] in [0, n_arms) and every k:
 *     a_pk = sum_i W[k,i] x_p[i],   d_pk = -sum_i D[k,i] x_p[i],   c_k = sum_i W[k,i]
 *     Theta_pk[j] = m_j(u_p) (e_j ? a_pk : c_k)          (m_j: the u-monomial, e_j: the state exponent of column j)
 *     G[a] += sum_k Theta_pk Theta_pk^T,   b[a] += sum_k Theta_pk d_pk
 * A patient with rows[p] < T or an arm outside [0, n_arms) contributes nothing (what its samples hold, NaN
 * included, reaches no output).
 *
 * Speed.  The Gram pass multiplies only inside the nonzero column range of every tile of 16 consecutive rows of
 * W | D.  G, b and the moments do not depend on the order of the rows beyond rounding, so a caller whose test
 * functions have compact support should pass the rows sorted by centre (insite_amd.weak / SINDY.fit_weak do).
 */
#ifndef INSITE_WEAK_H_
#define INSITE_WEAK_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_WEAK_ABI_VERSION 1

#define INSITE_WEAK_MAX_K 1024 /* test functions per call; more: INSITE_E_UNSUPPORTED */

/* optimizer values of insite_sindy_fit_weak_f64 */
#define INSITE_OPT_SR3 0   /* insite_sr3_f64 */
#define INSITE_OPT_STLSQ 1 /* insite_stlsq_f64 */

int32_t insite_weak_abi_version(void);

/* Workspace of insite_gram_weak_f64 / insite_sindy_fit_weak_f64 (0 for invalid arguments). */
size_t insite_gram_weak_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms, int32_t K);

/* Per-arm Gram systems of the weak regression, one pass over x; the projections a, d stay on chip.
 *   x      f64, `layout` INSITE_LAYOUT_PATIENT_MAJOR x[p * ldx + i] (ldx >= n_steps) or
 *          INSITE_LAYOUT_TIME_MAJOR x[i * ldx + p] (ldx >= n_patients); n_steps = T >= 1
 *   W, D   f64 [K, ldw], ldw >= n_steps, 1 <= K (K > INSITE_WEAK_MAX_K: INSITE_E_UNSUPPORTED)
 *   u      f64 [n_patients, n_statics] (may be NULL when n_statics = 0)
 *   arm    i8  [n_patients];  rows i32 [n_patients]
 *   exps   i8  [n_terms, 1 + n_statics]  HOST; a library insite_gram_f64 accepts (state exponent <= 1,
 *          n_terms <= INSITE_MAX_TERMS), else INSITE_E_UNSUPPORTED / _INVALID_ARG
 *   G_out  f64 [n_arms, F, F], b_out f64 [n_arms, F] (overwritten; an arm without patients has G = b = 0)
 *   mom_out  f64 [n_patients, 5] or NULL: {sum c^2, sum c a, sum a^2, sum c d, sum a d} over k per patient --
 *          the layout of insite_gram_moments_f64 with 1 -> c, x -> a, x_dot -> d; zeros for a patient that
 *          contributes nothing
 * INSITE_E_INVALID_ARG: another layout, ldx or ldw too small, n_steps < 1, K < 1, n_arms outside
 * 1..INSITE_MAX_ARMS, negative counts, NULL outputs (or NULL inputs with n_patients > 0).
 * INSITE_E_WORKSPACE: workspace NULL or too small.  n_patients = 0 is a successful no-op (the outputs are not
 * written).  Deterministic: every reduction runs in a fixed order, two calls give bitwise equal outputs. */
int32_t insite_gram_weak_f64(const double* x, int64_t ldx, int32_t layout, int32_t n_steps, const double* W,
                             const double* D, int64_t ldw, int32_t K, const double* u, const int8_t* arm,
                             const int32_t* rows, int64_t n_patients, int32_t n_statics, int32_t n_arms,
                             const int8_t* exps, int32_t n_terms, double* G_out, double* b_out, double* mom_out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Batched SR3 with the l1 proximal operator on column-normalised Gram systems (n_sys systems G [n_sys, F, F],
 * b [n_sys, F], F = n_terms <= INSITE_MAX_TERMS, else INSITE_E_UNSUPPORTED).  Per system:
 *   1. n_j = sqrt(G_jj), Gn = G / (n n^T), bn = b / n
 *   2. v = Gn^-1 bn (Cholesky)
 *   3. A = Gn + I / nu, factored once
 *   4. repeat: w = A^-1 (bn + v / nu);  v+ = sign(w) max(|w| - threshold, 0)
 *   5. until sqrt(sum (v+ - v)^2) / nu < tol, or after max_iter iterations
 *   6. support = |v| > 1e-14
 *   7. coef = the least-squares solution of the un-normalised G, b on the support (unbias != 0), else v / n
 * iters_out [n_sys] (may be NULL) receives the iterations of step 4 run.  With one term and tol = threshold / nu
 * (the defaults of the Python layer) the first stopping value equals tol up to rounding whenever the coefficient
 * survives the first shrink, so the count is then 1 or 2 by the last bit (on an MI355X 14 of 32 random one-term
 * systems sat within 1e-6 of tol and one count differed from the numpy restatement; tests/test_gpu_library_matrix.py):
 * compare iteration counts at another tol.  A system whose Cholesky fails
 * (a non-positive G_jj or pivot, an all-zero system included) gets iters = -1, NaN coefficients and an empty
 * mask.  coef_out [n_sys, F]; mask_out [n_sys, F] int8 or NULL.
 * INSITE_E_INVALID_ARG: threshold or tol negative or NaN, nu <= 0 or NaN, max_iter < 0, n_sys < 0, n_terms < 1,
 * NULL G / b / coef_out with n_sys > 0.  n_sys = 0 is a successful no-op. */
int32_t insite_sr3_f64(const double* G, const double* b, int64_t n_sys, int32_t n_terms, double threshold, double nu,
                       double tol, int32_t max_iter, int32_t unbias, double* coef_out, int8_t* mask_out,
                       int32_t* iters_out, void* stream);

/* insite_gram_weak_f64 followed on the same stream, without host synchronisation, by the per-arm solve:
 *   optimizer INSITE_OPT_SR3:   insite_sr3_f64(G_out, b_out, n_arms, ..., threshold, nu, tol, max_iter, unbias)
 *   optimizer INSITE_OPT_STLSQ: insite_stlsq_f64(G_out, b_out, n_arms, ..., threshold, alpha, max_iter, unbias)
 * (the parameters of the other optimizer are validated as well).  coef_out [n_arms, F]; mask_out [n_arms, F],
 * iters_out [n_arms] may be NULL.  Additionally INSITE_E_INVALID_ARG for another optimizer value, a NULL
 * coef_out or an invalid solver parameter (insite_sr3_f64 / insite_stlsq_f64). */
int32_t insite_sindy_fit_weak_f64(const double* x, int64_t ldx, int32_t layout, int32_t n_steps, const double* W,
                                  const double* D, int64_t ldw, int32_t K, const double* u, const int8_t* arm,
                                  const int32_t* rows, int64_t n_patients, int32_t n_statics, int32_t n_arms,
                                  const int8_t* exps, int32_t n_terms, int32_t optimizer, double threshold,
                                  double alpha, double nu, double tol, int32_t max_iter, int32_t unbias,
                                  double* G_out, double* b_out, double* coef_out, int8_t* mask_out,
                                  int32_t* iters_out, double* mom_out, void* workspace, size_t workspace_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_WEAK_H_ */
