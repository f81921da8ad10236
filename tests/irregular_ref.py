"""CPU restatement (plain numpy) of the discovery on per-patient irregular observation grids
(include/insite_irregular.h): the checker of tests/test_irregular_oracle.py and tests/test_gpu_irregular.py,
never the thing measured.

x_dot at sample k of a patient with L samples is the derivative at t_k of the Lagrange interpolant through the W
consecutive samples [lo, lo + W), lo = clamp(k - W/2, 0, L - W); W = 3 is numpy.gradient(x, t, edge_order=2) =
pysindy FiniteDifference(order=2, is_uniform=False), W = 5 its five-point form.  Patients with L < W contribute
nothing; the library (oracle.insite_ref.poly_library column order) sees the raw samples.  Every function takes
the working dtype from its inputs, so the same code runs in float64 and in numpy.longdouble.
"""
from __future__ import annotations

import numpy as np

from oracle import insite_ref as R

WINDOW = {"nonuniform2": 3, "nonuniform4": 5}
K_GT = 16   # the kernel's time tile in steps (csrc/insite_hip.hip: INSITE_GT)


def lagrange_derivative(x, t, W):
    """x_dot [L] of the samples x [L] at the strictly increasing times t [L], L >= W."""
    x = np.asarray(x)
    t = np.asarray(t)
    L = x.shape[0]
    if L < W:
        raise ValueError("trajectory shorter than the stencil")
    dt = np.result_type(x.dtype, t.dtype)
    k = np.arange(L)
    lo = np.clip(k - W // 2, 0, L - W)
    kp = k - lo                                   # position of sample k in its window
    tw = t[lo[:, None] + np.arange(W)].astype(dt)  # [L, W] window nodes
    xw = x[lo[:, None] + np.arange(W)].astype(dt)
    tk = t[k].astype(dt)
    d = np.zeros(L, dtype=dt)
    one = dt.type(1)
    for j in range(W):
        own = kp == j                             # x_j is x_k itself: sum_{m != k} 1 / (t_k - t_m)
        wk = np.zeros(L, dtype=dt)
        wj = np.ones(L, dtype=dt)                 # else: prod_{m != j,k} (t_k - t_m) / (t_j - t_m) / (t_j - t_k)
        for m in range(W):
            if m == j:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                wk = wk + np.where(own, one / (tk - tw[:, m]), 0)
                wj = wj * np.where(own | (kp == m), one, (tk - tw[:, m]) / (tw[:, j] - tw[:, m]))
        with np.errstate(divide="ignore", invalid="ignore"):
            wj = np.where(own, wk, wj / (tw[:, j] - tk))
        d = d + wj * xw[:, j]
    return d


def eval_library(exps, Z):
    """oracle.insite_ref.eval_library in the dtype of Z."""
    Z = np.asarray(Z)
    th = np.ones((Z.shape[0], exps.shape[0]), dtype=Z.dtype)
    for j, e in enumerate(exps):
        for i, k in enumerate(e):
            for _ in range(int(k)):
                th[:, j] = th[:, j] * Z[:, i]
    return th


def gram_irregular(x, t_obs, n_obs, u, arm, exps, n_arms=2, fd="nonuniform4"):
    """(G [A, F, F], b [A, F], mom [N, 5]) of the per-arm regression: what insite_gram_irregular_f64 returns.
    mom = {samples used, sum x, sum x^2, sum x_dot, sum x_dot x} per patient (zeros when L < W)."""
    W = WINDOW[fd]
    dt = np.result_type(np.asarray(x).dtype, np.asarray(t_obs).dtype, np.asarray(u).dtype)
    F = exps.shape[0]
    N = x.shape[0]
    G = np.zeros((n_arms, F, F), dtype=dt)
    b = np.zeros((n_arms, F), dtype=dt)
    mom = np.zeros((N, 5), dtype=dt)
    for p in range(N):
        L = min(int(n_obs[p]), x.shape[1])
        a = int(arm[p])
        if L < W:
            continue
        xp = np.asarray(x[p, :L], dtype=dt)
        xd = lagrange_derivative(xp, np.asarray(t_obs[p, :L], dtype=dt), W)
        mom[p] = [L, xp.sum(), (xp * xp).sum(), xd.sum(), (xd * xp).sum()]
        if not 0 <= a < n_arms:
            continue
        Z = np.concatenate([xp[:, None], np.repeat(np.asarray(u[p], dtype=dt)[None, :], L, 0)], axis=1)
        th = eval_library(exps, Z)
        G[a] += th.T @ th
        b[a] += th.T @ xd
    return G, b, mom


def sindy_fit_irregular(x, t_obs, n_obs, u, arm, exps, threshold, alpha, n_arms=2, fd="nonuniform4", max_iter=100,
                        unbias=True):
    """(coef [A, F], support [A, F] bool, iters [A], G, b, mom): the Gram above, then oracle.insite_ref.stlsq_gram
    per arm -- what insite_sindy_fit_irregular_f64 returns."""
    G, b, mom = gram_irregular(x, t_obs, n_obs, u, arm, exps, n_arms, fd)
    fits = [R.stlsq_gram(np.asarray(G[a], np.float64), np.asarray(b[a], np.float64), threshold, alpha, max_iter,
                         unbias) for a in range(n_arms)]
    return (np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]),
            np.array([f[2] for f in fits], dtype=np.int32), G, b, mom)


# ---------------------------------------------------------------------------------------------------
# cohorts of the tests (seeded numpy; the GPU tests upload them)
# ---------------------------------------------------------------------------------------------------
def c5_grid(N, rng, T_max=60, n_min=20):
    """C5 grids (oracle/rk45_ref.irregular_grid), zero past each patient's samples: (t [N, T_max], n_obs)."""
    from oracle import rk45_ref
    t, n_obs = rk45_ref.irregular_grid(N, rng, n_min=n_min, n_max=T_max)
    return np.nan_to_num(t, nan=0.0), n_obs


def edge_lengths(T_max=60):
    """Sample counts that touch every tile edge of the kernel, its halo hand-over and the L < W rule."""
    return np.array([0, 2, 3, 4, 5, 6, K_GT - 1, K_GT, K_GT + 1, 2 * K_GT, 2 * K_GT + 1, T_max], dtype=np.int32)


def edge_grid(N, rng, T_max=60):
    """Grids whose lengths are drawn from ``edge_lengths`` (each value present when N allows), gaps ~ U(0.02, 0.3):
    the sampling density of a C5 grid whatever the length."""
    vals = edge_lengths(T_max)
    n_obs = rng.choice(vals, N).astype(np.int32)
    n_obs[:min(N, vals.size)] = rng.permutation(vals)[:min(N, vals.size)]
    t = np.zeros((N, T_max))
    t[:, 1:] = np.cumsum(rng.uniform(0.02, 0.3, (N, T_max - 1)), axis=1)
    t[np.arange(T_max)[None, :] >= n_obs[:, None]] = 0.0
    return t, n_obs


def jitter_grid(N, rng, T_max=60):
    """t_k = (k + U(-0.3, 0.3)) * 10 / 60 for every patient, full length."""
    k = np.arange(T_max)[None, :]
    t = (k + rng.uniform(-0.3, 0.3, (N, T_max))) * (R.MAX_TIME_HORIZON / 60.0)
    return t, np.full(N, T_max, dtype=np.int32)


def decay_cohort(t, n_obs, rng, noise=0.0, arm=None):
    """EQ_4_C on the given grids in closed form: c ~ N(0.5, 0.05), C = (c0 + 0.05, c1 + 0.15), y0 ~ U(1, 50),
    x = y0 exp(-C_arm t) (+ noise N(0, 1)); zeros past each patient's samples.  Returns (x, u, arm)."""
    N, T_max = t.shape
    c = rng.normal(0.5, 0.05, (N, 2))
    C = c + np.array([0.05, 0.15])
    y0 = rng.uniform(1.0, 50.0, N)
    if arm is None:
        arm = rng.integers(0, 2, N)
    arm = np.asarray(arm).astype(np.int8)
    x = y0[:, None] * np.exp(-C[np.arange(N), arm][:, None] * t)
    if noise:
        x = x + noise * rng.normal(size=x.shape)
    x[np.arange(T_max)[None, :] >= np.asarray(n_obs)[:, None]] = 0.0
    return x, c, arm
