"""numpy restatement of include/insite_feedback.h, the reference of tests/test_feedback_abi.py (CPU) and
tests/test_gpu_feedback.py (GPU), and the parity cases the two share.  Helper only: no tests in this file.

Trajectories come step by step from ``oracle.insite_ref.rollout`` called on one interval at a time with the step's
per-row arm (row r N + p is row p under replicate r, the oracle's per-row coefficient form), with regimen_ref's NaN
rule per arm (a replicate whose arm a has a NaN coefficient is NaN from the first step that uses arm a).  The decision
is the header's one ordered comparison, the objective a plain multiply-add over the steps ascending followed by the
separate addition of the arm cost, the choice is ``regimen_ref.choose`` and the statistics are ``effect_ref.stats``.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
import regimen_ref as G  # noqa: E402
from oracle import insite_ref as R  # noqa: E402


def closed_loop(y0, u, theta, rules, coef, exps, dt, w, cost=None, arm_cost=None, method="euler5", substeps=None):
    """The closed loops of K rules: theta [N, 2 K], rules [K, 4] = (arm_on, arm_off, period, start_on), w [N, T].
    Returns dict(J [R, N, K], E [R, N, K] (NaN where a state is NaN), arms [R, N, K, T], scale [N], dmargin [N]):
    scale s_p = max_{r, j} (|cost_j| + sum_k |w| |y|) + sum_a |arm_cost_a| over the non-NaN replicates; dmargin m_p =
    min over replicates, rules and decision steps of |z_k - theta| / max |y| (the threshold the flag selects; max |y|
    over the row's y0 and every finite state of every replicate and rule; NaN states and thresholds do not count)."""
    Rn, A = coef.shape[:2]
    N, T = w.shape
    K = len(rules)
    bad = np.isnan(coef).any(axis=2)                                   # [R, A]
    rows = np.repeat(np.where(np.isnan(coef), 0.0, coef), N, axis=0)   # [R N, A, F]
    badr = np.repeat(bad, N, axis=0)                                   # [R N, A]
    ur = np.tile(u, (Rn, 1))
    sel = np.arange(Rn * N)
    J = np.empty((Rn, N, K))
    S = np.empty((Rn, N, K))
    Ex = np.empty((Rn, N, K))
    arms = np.empty((Rn, N, K, T), dtype=np.int8)
    ymax = np.abs(np.asarray(y0, dtype=np.float64)).copy()
    dm = np.full(N, np.inf)
    for j, (a_on, a_off, period, start) in enumerate(rules):
        t_on, t_off = np.tile(theta[:, 2 * j], Rn), np.tile(theta[:, 2 * j + 1], Rn)
        y = np.tile(np.asarray(y0, dtype=np.float64), Rn)
        on = np.full(Rn * N, bool(start))
        poison = np.zeros(Rn * N, dtype=bool)
        c = 0.0 if cost is None else float(cost[j])
        acc = np.full(Rn * N, c)
        sc = np.full(Rn * N, abs(c))
        cnt = np.zeros(Rn * N)
        for k in range(T):
            if k % period == 0:
                thr = np.where(on, t_off, t_on)
                with np.errstate(invalid="ignore"):
                    on = y >= thr                                      # NaN on either side: off
                    gap = np.abs(y - thr)
                gap = np.where(np.isnan(gap), np.inf, gap).reshape(Rn, N).min(axis=0)
                dm = np.minimum(dm, gap)
            arm = np.where(on, a_on, a_off).astype(np.int8)
            arms[:, :, j, k] = arm.reshape(Rn, N)
            poison |= badr[sel, arm]
            y = R.rollout(np.where(poison, 0.0, y), ur, arm[:, None], rows, exps, dt, method=method,
                          substeps=substeps)[:, 0]
            y = np.where(poison, np.nan, y)
            with np.errstate(invalid="ignore", over="ignore"):
                acc = acc + np.tile(w[:, k], Rn) * y
                sc = sc + np.abs(np.tile(w[:, k], Rn)) * np.abs(y)
                if arm_cost is not None:
                    acc = acc + np.asarray(arm_cost, dtype=np.float64)[arm]
            cnt = cnt + on
            ymax = np.fmax(ymax, np.fmax.reduce(np.where(np.isfinite(y), np.abs(y), 0.0).reshape(Rn, N), axis=0))
        J[:, :, j] = acc.reshape(Rn, N)
        S[:, :, j] = sc.reshape(Rn, N)
        Ex[:, :, j] = np.where(poison, np.nan, cnt).reshape(Rn, N)
    scale = np.fmax.reduce(np.fmax.reduce(S, axis=2), axis=0)
    if arm_cost is not None:
        scale = scale + float(np.abs(arm_cost).sum())
    return {"J": J, "E": Ex, "arms": arms, "scale": scale, "dmargin": dm / ymax}


def feedback(y0, u, theta, rules, coef, exps, dt, q, w, cost=None, arm_cost=None, sense=1, method="euler5",
             substeps=None):
    """The definition: dict(choice [N], win [N, K], out [N, K, 3, 3 + Q], sched [N, K, T], scale [N], margin [N]
    (regimen_ref's argmin margin), dmargin [N], J, E, best)."""
    N = np.asarray(y0).shape[0]
    K = len(rules)
    theta = np.asarray(theta, dtype=np.float64)
    if theta.shape != (N, 2 * K):                                      # the shared [K, 2] table
        theta = np.broadcast_to(theta.reshape(1, 2 * K), (N, 2 * K))
    w = np.broadcast_to(w, (N, np.shape(w)[-1]))
    cl = closed_loop(y0, u, theta, rules, coef, exps, dt, w, cost, arm_cost, method, substeps)
    J = cl["J"]
    Rn = J.shape[0]
    best, regret, margin = G.choose(J, sense)
    votes = np.stack([(best[1:] == j).sum(axis=0) for j in range(K)], axis=1)
    win = votes.astype(np.float64) / float(Rn - 1)
    out = np.stack([E.stats(J, q), E.stats(regret, q), E.stats(cl["E"], q)])       # [3, 3 + Q, N, K]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.fmin.reduce(margin, axis=0) / cl["scale"]
    m = np.where(np.isnan(m), np.inf, m)
    return {"choice": best[0].astype(np.int32), "win": win, "out": np.ascontiguousarray(out.transpose(2, 3, 0, 1)),
            "sched": np.ascontiguousarray(cl["arms"][0]), "scale": cl["scale"], "margin": m,
            "dmargin": cl["dmargin"], "J": J, "E": cl["E"], "best": best}


# ---------------------------------------------------------------------------------------------------
# the parity cases (tests/test_gpu_feedback.py runs them; tests/test_feedback_abi.py asserts their input conditions)
# ---------------------------------------------------------------------------------------------------
DT, Q5, Q16 = G.DT, G.Q5, G.Q16
PAD_THETA, PAD_W, PAD_OUT, PAD_SCHED, POISON, POISON_I8 = 3, 2, 5, 7, -7.25, -77

# (R, N, T, n_arms, K, table, method, substeps, q, theta, weights, cost, arm_cost, sense): a sample, not the product.
# Every V (R <= 64, 128, 256, 512), partly filled top slots (65, 129, 200), n = 1 (R = 2); K = 1, 2, 3, 8, 16, with 16
# at R = 512 (the LDS worst case); T below, at and across the 16-step chunk; one row to three waves' worth of rows; 1, 2
# and 4 arms; several tables of tests/library_matrix.py; both methods, substeps 1 and 5.  theta "shared": [K, 2],
# "rows": [N, 2 K + pad]; weights "shared": [T + pad], "rows": [N, T + pad]; the padding holds NaN.  The periods of the
# rules cycle through 1, 1, 2, 5 and T + 3 (never decided again), start_on alternates.  Without a cost two rules that
# end up on the same arm at every step tie exactly, so the cases without one have one or two rules (and a seed key chosen for it).  The last
# entry is the seed key.
CASES = [
    (2, 3, 1, 1, 2, "x_only", "euler", 1, Q5, "shared", "shared", True, True, 1, 0),
    (3, 1, 2, 2, 3, "bias_x", "rk4", 1, Q5, "rows", "rows", True, False, -1, 0),
    (17, 130, 16, 2, 3, "std7", "euler", 5, Q5, "rows", "shared", True, True, 1, 0),
    (17, 3, 17, 2, 1, "dup4", "rk4", 1, Q5, "shared", "shared", False, True, 1, 0),
    (64, 3, 33, 4, 8, "noone3", "rk4", 5, Q16, "shared", "rows", True, True, 1, 0),
    (65, 3, 70, 2, 2, "lin3", "euler", 5, Q5, "rows", "rows", False, False, -1, 4),
    (129, 3, 17, 4, 16, "u3_first9", "euler", 1, Q16, "rows", "rows", True, True, 1, 0),
    (200, 3, 70, 2, 3, "std7", "rk4", 1, Q5, "shared", "shared", True, False, -1, 0),
    (256, 130, 33, 2, 8, "high_pow", "euler", 5, Q5, "rows", "rows", True, True, 1, 0),
    (512, 1, 70, 4, 16, "deg2_no_xx", "euler", 5, Q16, "rows", "rows", True, False, -1, 0),
    (2, 130, 33, 4, 8, "std7", "euler", 5, Q16, "rows", "rows", True, True, -1, 0),
]
CASE_IDS = [f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-K{c[4]}-{c[5]}-{c[6]}{c[7]}-Q{len(c[8])}-{c[9]}-{c[10]}"
            f"-{'cost' if c[11] else 'nocost'}-{'armcost' if c[12] else 'noarmcost'}-{'min' if c[13] > 0 else 'max'}"
            for c in CASES]
PERIODS = (1, 1, 2, 5)


def rule_table(rng, K, A, T):
    """[K, 4] int32: distinct arms where there are two, periods cycling through 1, 1, 2, 5 and T + 3, start_on
    alternating."""
    rules = np.empty((K, 4), dtype=np.int32)
    for j in range(K):
        a_on = int(rng.integers(0, A))
        a_off = int((a_on + 1 + rng.integers(0, A - 1)) % A) if A > 1 else 0
        period = T + 3 if j % 5 == 4 else PERIODS[j % 5]
        rules[j] = (a_on, a_off, period, j % 2)
    return rules


def inputs(seed_key, Rn, N, T, A, K, name, theta_mode="rows", w_mode="rows", with_cost=True, with_ac=True):
    """(y0 [N], u [N, U], theta [K, 2] or [N, 2 K + pad], rules [K, 4], w [T + pad] or [N, T + pad], cost [K] or None,
    arm_cost [A] or None, coef [R, A, F]), drawn like ``regimen_ref.inputs``: y0 ~ U(0.5, 3), u ~ U(0.6, 1.6),
    weights in [0, 1), costs in +-0.05, arm costs in +-0.02; theta_on = y0 U(0.6, 1.1) (shared: 1.75 U(0.6, 1.1)),
    theta_off = theta_on U(0.6, 1); the padding of theta and of the weights holds NaN."""
    rng = np.random.default_rng(M._seed(*seed_key))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    if theta_mode == "shared":
        t_on = 1.75 * rng.uniform(0.6, 1.1, K)
        theta = np.stack([t_on, t_on * rng.uniform(0.6, 1.0, K)], axis=1)
    else:
        t_on = y0[:, None] * rng.uniform(0.6, 1.1, (N, K))
        theta = np.full((N, 2 * K + PAD_THETA), np.nan)
        theta[:, 0:2 * K:2] = t_on
        theta[:, 1:2 * K:2] = t_on * rng.uniform(0.6, 1.0, (N, K))
    rules = rule_table(rng, K, A, T)
    wshape = (T + PAD_W,) if w_mode == "shared" else (N, T + PAD_W)
    w = rng.uniform(0.0, 1.0, wshape)
    w[..., T:] = np.nan
    cost = rng.uniform(-0.05, 0.05, K) if with_cost else None
    arm_cost = rng.uniform(-0.02, 0.02, A) if with_ac else None
    return y0, u, theta, rules, w, cost, arm_cost, G.coef_ensemble(rng, name, Rn, A)


def full_theta(theta, N, K):
    """[N, 2 K] of either threshold form."""
    if theta.shape == (K, 2) and not (theta.shape[0] == N and theta.shape[1] >= 2 * K):
        return np.ascontiguousarray(np.broadcast_to(theta.reshape(1, 2 * K), (N, 2 * K)))
    return np.ascontiguousarray(theta[:, :2 * K])


def reference(y0, u, theta, rules, coef, name, q, w, cost, arm_cost, sense, method, sub, T):
    N, K = y0.shape[0], len(rules)
    return feedback(y0, u, full_theta(theta, N, K), rules, coef, M.exps_of(name), DT, q,
                    np.broadcast_to(w[..., :T], (N, T)), cost, arm_cost, sense, method, sub)


@functools.lru_cache(maxsize=None)
def case(Rn, N, T, A, K, name, method, sub, q, theta_mode, w_mode, with_cost, with_ac, sense, key):
    """The inputs of one parity case and its reference (computed once, read-only)."""
    y0, u, theta, rules, w, cost, arm_cost, coef = inputs(("feedback", Rn, N, T, A, K, name, method, sub, key), Rn, N,
                                                          T, A, K, name, theta_mode, w_mode, with_cost, with_ac)
    ref = reference(y0, u, theta, rules, coef, name, q, w, cost, arm_cost, sense, method, sub, T)
    for a in (y0, u, theta, rules, w, cost, arm_cost, coef) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return y0, u, theta, rules, w, cost, arm_cost, coef, ref
