/*
 * insite_irregular.h — SINDy discovery on per-patient irregular observation grids: an extension of the C ABI
 * of libinsite_hip.so (insite_hip.h), versioned on its own (INSITE_IRREGULAR_ABI_VERSION) so that the pinned
 * surface of insite_hip.h does not move.  The symbols live in the same shared library.
 *
 * Reference interface replaced: pysindy SINDy(STLSQ, FiniteDifference(order=2, is_uniform=False),
 * PolynomialLibrary).fit(X_a, t=[t_p], u=U_a, multiple_trajectories=True) — the discovery of
 * libs_m/ct/src/models/sindy.py:190-192 on trajectories whose sampling times differ per patient and whose
 * lengths are ragged (the shape insite_rollout_rk45_f64 rolls a model out on).  The reference itself only
 * fits on a uniform grid; this is the half of that pipeline it lacks.
 *
 * Conventions are insite_hip.h's: device pointers to caller-owned memory (exps: host), row-major, leading
 * dimensions in elements, caller-owned workspace sized by the *_workspace_bytes query (its first 512 bytes
 * zero before the first use; every call leaves them zero), asynchronous on the caller's stream, int32 status
 * (INSITE_OK / INSITE_E_*), every argument validated before any HIP call.
 *
 * Derivative estimator.  For a patient with L = n_obs[p] samples, x_dot at sample k is the derivative at t_k of
 * the Lagrange interpolant through the W consecutive samples [lo, lo + W), lo = clamp(k - W/2, 0, L - W):
 * a central stencil for interior samples, a shifted one for the W/2 samples at each end.  With the window's
 * nodes t_j, the weight of x_j (j != k) is  prod_{m != j,k} (t_k - t_m) / (t_j - t_m) / (t_j - t_k)  and the
 * weight of x_k is  sum_{m != k} 1 / (t_k - t_m).
 *   INSITE_FD_NONUNIFORM2  W = 3: numpy.gradient(x, t, edge_order=2), pysindy FiniteDifference(order=2,
 *                          is_uniform=False)
 *   INSITE_FD_NONUNIFORM4  W = 5: the five-point form (fourth order; on a uniform grid its interior samples
 *                          are INSITE_FD_ORDER4's)
 * A patient with L < W contributes nothing.  The library columns see the raw samples.  Each grid must be
 * strictly increasing within its n_obs samples: pysindy raises otherwise, and the caller validates it (a
 * repeated time gives a non-finite G / b).  Samples at k >= n_obs[p] of x and t_obs may hold anything, NaN
 * included; they reach no output.
 */
#ifndef INSITE_IRREGULAR_H_
#define INSITE_IRREGULAR_H_

#include <stddef.h>
#include <stdint.h>

#include "insite_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define INSITE_IRREGULAR_ABI_VERSION 1

/* fd_kind values of this header (insite_hip.h's entry points answer INSITE_E_UNSUPPORTED for them) */
#define INSITE_FD_NONUNIFORM2 4 /* three-sample Lagrange derivative on the patient's own times */
#define INSITE_FD_NONUNIFORM4 5 /* five-sample Lagrange derivative on the patient's own times */

int32_t insite_irregular_abi_version(void);

/* Workspace of the two entry points below (0 for invalid arguments). */
size_t insite_gram_irregular_workspace_bytes(int64_t n_patients, int32_t n_arms, int32_t n_terms);

/* Per-arm Gram systems of the SINDy regression on irregular grids, one streaming pass over x and t_obs.
 *   x      f64 [n_patients, ldx]   patient-major samples, ldx >= T_max
 *   t_obs  f64 [n_patients, ld_t]  observation times of the same samples, ld_t >= T_max
 *   n_obs  i32 [n_patients]        samples of each patient, in [0, T_max] (larger values count as T_max)
 *   u      f64 [n_patients, n_statics]   static covariates (may be NULL when n_statics = 0)
 *   arm    i8  [n_patients]        the patient's factual arm in [0, n_arms); other values: contributes nothing
 *   exps   i8  [n_terms, 1 + n_statics]  HOST; a library insite_gram_f64 accepts (state exponent <= 1,
 *                                  n_terms <= INSITE_MAX_TERMS), else INSITE_E_UNSUPPORTED / _INVALID_ARG
 *   fd_kind  INSITE_FD_NONUNIFORM2 or INSITE_FD_NONUNIFORM4, else INSITE_E_INVALID_ARG
 *   G_out  f64 [n_arms, F, F], b_out f64 [n_arms, F]: Theta^T Theta and Theta^T x_dot of each arm, as
 *          insite_gram_f64 (G_out[a][0][0] of a library with a bias column is arm a's sample count; an arm
 *          without samples has G = b = 0)
 *   mom_out  f64 [n_patients, 5] or NULL: {samples used, sum x, sum x^2, sum x_dot, sum x_dot x} per patient,
 *          the layout of insite_gram_moments_f64; zeros for a patient that contributes nothing
 * INSITE_E_INVALID_ARG: ldx or ld_t < T_max, n_arms outside 1..INSITE_MAX_ARMS, negative counts, NULL outputs
 * (or NULL inputs with n_patients > 0).  INSITE_E_WORKSPACE: workspace NULL or too small.  n_patients = 0 is a
 * successful no-op (the outputs are not written).  Deterministic: the reduction order is fixed by block index,
 * two calls give bitwise equal outputs. */
int32_t insite_gram_irregular_f64(const double* x, int64_t ldx, const double* t_obs, int64_t ld_t,
                                  const int32_t* n_obs, const double* u, const int8_t* arm, int64_t n_patients,
                                  int32_t T_max, int32_t n_statics, int32_t n_arms, const int8_t* exps,
                                  int32_t n_terms, int32_t fd_kind, double* G_out, double* b_out, double* mom_out,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* The same pass followed by the per-arm STLSQ fit (threshold, alpha, max_iter, unbias and coef_out [n_arms, F],
 * mask_out [n_arms, F] or NULL, iters_out [n_arms] or NULL as insite_sindy_fit_f64); for n_terms = 7 the fit
 * runs in the finalisation of the same launch.  Additionally INSITE_E_INVALID_ARG for a NULL coef_out,
 * max_iter < 0, or threshold / alpha negative or NaN. */
int32_t insite_sindy_fit_irregular_f64(const double* x, int64_t ldx, const double* t_obs, int64_t ld_t,
                                       const int32_t* n_obs, const double* u, const int8_t* arm, int64_t n_patients,
                                       int32_t T_max, int32_t n_statics, int32_t n_arms, const int8_t* exps,
                                       int32_t n_terms, int32_t fd_kind, double threshold, double alpha,
                                       int32_t max_iter, int32_t unbias, double* G_out, double* b_out,
                                       double* coef_out, int8_t* mask_out, int32_t* iters_out, double* mom_out,
                                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* INSITE_IRREGULAR_H_ */
