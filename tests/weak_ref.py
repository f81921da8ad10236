"""CPU restatement (plain numpy) of the weak-form discovery (include/insite_weak.h): the checker of
tests/test_weak_oracle.py and tests/test_gpu_weak.py, never the thing measured.

Grid t_i = i dt, i = 0..T-1, L = (T - 1) dt.  Test function k: phi_k(t) = (1 - tau^2)^p, tau = (t - c_k) / H, over
the grid points with |t_i - c_k| <= H:  W[k,i] = dt (1 - tau^2)^p,  D[k,i] = dt (-2 p tau (1 - tau^2)^(p-1)) / H.
For a patient p (all T samples, arm a) and every k:  a_pk = sum_i W[k,i] x_p[i],  d_pk = -sum_i D[k,i] x_p[i],
c_k = sum_i W[k,i];  the row is Theta_pk[j] = m_j(u_p) (e_j ? a_pk : c_k) and the target d_pk.  The rows are built
literally here (not through the per-patient moments).  Every function takes its working dtype from its inputs, so
the same code runs in float64 and in numpy.longdouble.
"""
from __future__ import annotations

import numpy as np

from oracle import insite_ref as R

SUPPORT_EPS = 1e-14


def half_width(T, dt):
    return (int(T) - 1) * float(dt) / 20.0


def weights(T, dt, centres, H=None, p=4, dtype=np.float64):
    """(W, D) [K, T]."""
    c = np.asarray(centres, dtype=dtype).reshape(-1)
    dt_ = dtype(dt)
    H_ = dtype(half_width(T, dt)) if H is None else dtype(H)
    t = np.arange(int(T)).astype(dtype) * dt_
    K = c.shape[0]
    W = np.zeros((K, T), dtype=dtype)
    D = np.zeros((K, T), dtype=dtype)
    for k in range(K):
        for i in range(T):
            if abs(t[i] - c[k]) <= H_:
                tau = (t[i] - c[k]) / H_
                q = dtype(1) - tau * tau
                W[k, i] = dt_ * q ** p
                D[k, i] = dt_ * (dtype(-2) * p * tau * q ** (p - 1)) / H_
    return W, D


def contributes(rows, arm, T, n_arms):
    rows = np.asarray(rows)
    arm = np.asarray(arm)
    return (rows >= T) & (arm >= 0) & (arm < n_arms)


def monomials(exps, u, dtype):
    """m_j(u_p) [N, F]: the u-part of every library column (exps [F, 1 + U], column 0 = the state exponent)."""
    N = u.shape[0]
    m = np.ones((N, exps.shape[0]), dtype=dtype)
    for j, e in enumerate(exps):
        for i, k in enumerate(e[1:]):
            for _ in range(int(k)):
                m[:, j] = m[:, j] * u[:, i].astype(dtype)
    return m


def weak_rows(x, u, arm, rows, W, D, exps, n_arms):
    """Per arm: (Theta [n_a K, F], d [n_a K]) — every row built literally."""
    dtype = np.result_type(x.dtype, W.dtype).type
    exps = np.asarray(exps)
    if exps[:, 0].max() > 1:
        raise ValueError("the weak rows are defined for the affine libraries (state exponent <= 1)")
    K, T = W.shape
    x = np.asarray(x)[:, :T].astype(dtype)
    on = contributes(rows, arm, T, n_arms)
    m = monomials(exps, np.asarray(u), dtype)
    c = W.sum(axis=1)
    out = []
    for a in range(n_arms):
        TH, DD = [], []
        for p in np.nonzero(on & (np.asarray(arm) == a))[0]:
            ap = W @ x[p]
            dp = -(D @ x[p])
            th = np.empty((K, exps.shape[0]), dtype=dtype)
            for j in range(exps.shape[0]):
                th[:, j] = m[p, j] * (ap if exps[j, 0] else c)
            TH.append(th)
            DD.append(dp)
        F = exps.shape[0]
        out.append((np.concatenate(TH) if TH else np.zeros((0, F), dtype=dtype),
                    np.concatenate(DD) if DD else np.zeros((0,), dtype=dtype)))
    return out


def gram(x, u, arm, rows, W, D, exps, n_arms):
    """G [A, F, F], b [A, F] = Theta^T Theta, Theta^T d of the literal rows."""
    rws = weak_rows(x, u, arm, rows, W, D, exps, n_arms)
    G = np.stack([th.T @ th for th, _ in rws])
    b = np.stack([th.T @ d for th, d in rws])
    return G, b


def moments(x, arm, rows, W, D, n_arms):
    """[N, 5] = {sum c^2, sum c a, sum a^2, sum c d, sum a d} over k; zeros for a patient that contributes nothing."""
    dtype = np.result_type(x.dtype, W.dtype).type
    K, T = W.shape
    x = np.asarray(x)[:, :T].astype(dtype)
    on = contributes(rows, arm, T, n_arms)
    c = W.sum(axis=1)
    mom = np.zeros((x.shape[0], 5), dtype=dtype)
    for p in np.nonzero(on)[0]:
        a = W @ x[p]
        d = -(D @ x[p])
        mom[p] = [c @ c, c @ a, a @ a, c @ d, a @ d]
    return mom


def gram_from_moments(mom, u, arm, exps, n_arms):
    """The per-arm expansion G[a][i][j] = sum_p m_i m_j M_p[e_i + e_j], b[a][i] = sum_p m_i M_p[3 + e_i]."""
    exps = np.asarray(exps)
    dtype = mom.dtype.type
    m = monomials(exps, np.asarray(u), dtype)
    F = exps.shape[0]
    G = np.zeros((n_arms, F, F), dtype=dtype)
    b = np.zeros((n_arms, F), dtype=dtype)
    e = exps[:, 0]
    for a in range(n_arms):
        sel = np.asarray(arm) == a
        for i in range(F):
            b[a, i] = np.sum(m[sel, i] * mom[sel, 3 + e[i]])
            for j in range(F):
                G[a, i, j] = np.sum(m[sel, i] * m[sel, j] * mom[sel, e[i] + e[j]])
    return G, b


def ols_on_support(G, b, support):
    """Least squares of the Gram system on the support (zeros elsewhere)."""
    S = np.nonzero(np.asarray(support))[0]
    out = np.zeros(G.shape[0])
    if S.size:
        out[S] = np.linalg.solve(G[np.ix_(S, S)], b[S])
    return out


def sr3(G, b, threshold, nu=1.0, tol=1e-1, max_iter=1000, unbias=True):
    """SR3 with the l1 prox on the column-normalised Gram system, as defined in include/insite_weak.h.
    Returns (coef, support, iters, stops): stops[k] = the stopping value sqrt(sum (v+ - v)^2) / nu of iteration k.
    A failed Cholesky gives NaN coefficients, an empty support and iters = -1."""
    F = G.shape[0]
    fail = (np.full(F, np.nan), np.zeros(F, dtype=bool), -1, [])
    dg = np.diag(G)
    if not np.all(dg > 0):
        return fail
    n = np.sqrt(dg)
    Gn = G / np.outer(n, n)
    bn = b / n
    try:
        Lc = np.linalg.cholesky(Gn)
        v = np.linalg.solve(Lc.T, np.linalg.solve(Lc, bn))
        La = np.linalg.cholesky(Gn + np.eye(F) / nu)
    except np.linalg.LinAlgError:
        return fail
    it, stops = 0, []
    for k in range(max_iter):
        it = k + 1
        w = np.linalg.solve(La.T, np.linalg.solve(La, bn + v / nu))
        vn = np.sign(w) * np.maximum(np.abs(w) - threshold, 0.0)
        stop = np.sqrt(np.sum((vn - v) ** 2)) / nu
        stops.append(float(stop))
        v = vn
        if stop < tol:
            break
    sup = np.abs(v) > SUPPORT_EPS
    if unbias and sup.any():
        try:
            S = np.nonzero(sup)[0]
            np.linalg.cholesky(G[np.ix_(S, S)])
            coef = ols_on_support(G, b, sup)
        except np.linalg.LinAlgError:
            return fail
    else:
        coef = v / n
    return coef, sup, it, stops


def per_patient_fit(x, u, arm, rows, W, D, exps, global_coef, threshold, alpha, max_iter=100):
    """Per-patient weak refit: every contributing patient refits its own arm's equation on its own K weak rows
    with the initial support of the global model (oracle.insite_ref.stlsq_initial_mask, the strong form's
    per-patient solver); the other arms keep the global coefficients.  A patient that contributes nothing keeps
    the global model (iters 0); an arm outside [0, A) gives iters -2.  Returns coef [N, A, F], mask [N, F],
    iters [N]."""
    global_coef = np.asarray(global_coef, dtype=np.float64)
    N = x.shape[0]
    A, F = global_coef.shape
    T = W.shape[1]
    coef = np.repeat(global_coef[None], N, axis=0)
    mask = np.zeros((N, F), dtype=np.int8)
    iters = np.zeros(N, dtype=np.int32)
    on = contributes(rows, arm, T, A)
    for p in range(N):
        a = int(arm[p])
        if not 0 <= a < A:
            iters[p] = -2
            continue
        if not on[p]:
            mask[p] = np.abs(global_coef[a]) > SUPPORT_EPS
            continue
        th, d = weak_rows(x[p:p + 1], u[p:p + 1], np.zeros(1, dtype=np.int64), rows[p:p + 1], W, D, exps, 1)[0]
        c, ind, it = R.stlsq_initial_mask(th, d, threshold, alpha, global_coef[a], max_iter)
        coef[p, a] = c
        mask[p] = ind
        iters[p] = it
    return coef, mask, iters
