"""numpy restatement of include/insite_regimen.h, the reference of tests/test_regimen_abi.py (CPU) and
tests/test_gpu_regimen.py (GPU), and the parity cases the two share.  Helper only: no tests in this file.

Trajectories are ``effect_ref.trajectories`` per plan (a NaN coefficient poisons the trajectory of its arm's first use
onwards), the objective is a plain multiply-add over the steps ascending (the kernel's is an FMA: the difference is
inside the GPU tolerance), the choice is a strict comparison in ascending plan order, and the statistics are
``effect_ref.stats``.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402


def trajectories(y0, u, arm, coef, exps, dt, method="euler5", substeps=None):
    """``effect_ref.trajectories`` [R, N, T] with the header's NaN rule per arm: a replicate whose arm a has a NaN
    coefficient is NaN from the first step that uses arm a."""
    bad = np.isnan(coef).any(axis=2)                                   # [R, A]
    y = E.trajectories(y0, u, arm, np.where(np.isnan(coef), 0.0, coef), exps, dt, method, substeps)
    for r, a in zip(*np.nonzero(bad)):
        y[r][np.maximum.accumulate(arm == a, axis=1)] = np.nan
    return y


def objectives(y0, u, plans, coef, exps, dt, w, cost=None, method="euler5", substeps=None):
    """(J [R, N, K], scale [N]): plans [K, N, T] per-step arms, w [N, T], cost [K] or None.  J = cost[j] +
    sum_k w[p, k] y_j[r, p, k], from cost[j], k ascending; scale s_p = max_{r, j} (|cost_j| + sum_k |w| |y|) over the
    non-NaN replicates."""
    K, N, T = plans.shape
    Rn = coef.shape[0]
    J = np.empty((Rn, N, K))
    S = np.empty((Rn, N, K))
    for j in range(K):
        y = trajectories(y0, u, plans[j], coef, exps, dt, method, substeps)
        c = 0.0 if cost is None else float(cost[j])
        acc = np.full((Rn, N), c)
        sc = np.full((Rn, N), abs(c))
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(T):
                acc = acc + w[None, :, k] * y[:, :, k]
                sc = sc + np.abs(w[None, :, k]) * np.abs(y[:, :, k])
        J[:, :, j] = acc
        S[:, :, j] = sc
    scale = np.fmax.reduce(np.fmax.reduce(S, axis=2), axis=0)
    return J, scale


def choose(J, sense=1):
    """(best [R, N] (-1: the replicate abstains), regret [R, N, K], margin [R, N]) of J [R, N, K]: the smallest j
    that attains min_j s J by a strict comparison in ascending j; regret = s J - s J[best] (NaN where the replicate
    abstains); margin = second-best - best of s J (inf for K = 1, NaN where the replicate abstains)."""
    Rn, N, K = J.shape
    sJ = float(sense) * J
    abst = np.isnan(J).any(axis=2)
    bestv = sJ[:, :, 0].copy()
    best = np.zeros((Rn, N), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(1, K):
            better = sJ[:, :, j] < bestv
            bestv = np.where(better, sJ[:, :, j], bestv)
            best = np.where(better, j, best)
        regret = sJ - bestv[:, :, None]
        regret[abst] = np.nan
        if K > 1:
            srt = np.sort(np.where(abst[:, :, None], 0.0, sJ), axis=2)
            margin = srt[:, :, 1] - srt[:, :, 0]
        else:
            margin = np.full((Rn, N), np.inf)
    margin = np.where(abst, np.nan, margin)
    return np.where(abst, -1, best), regret, margin


def regimen(y0, u, plans, coef, exps, dt, q, w, cost=None, sense=1, method="euler5", substeps=None):
    """The definition: dict(choice [N] int, win [N, K], out [N, K, 2, 3 + Q], scale [N], margin [N]); margin m_p =
    min_r (second-best - best of s J) / s_p over the non-abstaining replicates (inf for K = 1)."""
    K, N, T = plans.shape
    w = np.broadcast_to(w, (N, T))
    J, scale = objectives(y0, u, plans, coef, exps, dt, w, cost, method, substeps)
    Rn = J.shape[0]
    best, regret, margin = choose(J, sense)
    votes = np.stack([(best[1:] == j).sum(axis=0) for j in range(K)], axis=1)       # [N, K] exact integers
    win = votes.astype(np.float64) / float(Rn - 1)
    out = np.stack([E.stats(J, q), E.stats(regret, q)])                              # [2, 3 + Q, N, K]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.fmin.reduce(margin, axis=0) / scale
    m = np.where(np.isnan(m), np.inf, m)                                             # every replicate abstains
    return {"choice": best[0].astype(np.int32), "win": win, "out": np.ascontiguousarray(out.transpose(2, 3, 0, 1)),
            "scale": scale, "margin": m, "J": J, "best": best}


# ---------------------------------------------------------------------------------------------------
# the parity cases (tests/test_gpu_regimen.py runs them; tests/test_regimen_abi.py asserts their input conditions)
# ---------------------------------------------------------------------------------------------------
DT = 0.1
Q5 = (0.0, 1.0, 0.5, 0.025, 0.5)                     # unsorted, with a repeat (tests/test_gpu_effect.py)
Q16 = tuple(np.linspace(0.0, 1.0, 16)[[3, 0, 15, 7, 1, 14, 2, 13, 4, 12, 5, 11, 6, 10, 8, 9]])
PAD_PLAN, PAD_W, PAD_OUT, POISON = 3, 2, 5, -7.25

# (R, N, T, n_arms, K, table, method, substeps, q, plans, weights, cost, sense): a sample, not the product.  Every V
# (R <= 64, 128, 256, 512), partly filled top slots (65, 129, 200), n = 1 (R = 2); K = 1, 2, 3, 8, 16, with 16 at
# R = 512 (the LDS worst case); T below, at and across the 16-step chunk; one row to three waves' worth of rows; 1, 2
# and 4 arms; every table of tests/library_matrix.py; both methods, substeps 1 and 5.  plans "shared": [K, T + pad],
# "rows": [K, N, T + pad], the padding holding out-of-range arms; weights "shared": [T + pad], "rows": [N, T + pad], the
# padding holding NaN.  With one arm every plan is the same trajectory, so those cases have K = 1 or a cost.
CASES = [
    (2, 3, 1, 1, 2, "x_only", "euler", 1, Q5, "shared", "shared", True, 1),
    (3, 1, 2, 2, 3, "bias_x", "rk4", 1, Q5, "rows", "rows", True, -1),
    (17, 130, 16, 2, 3, "std7", "euler", 5, Q5, "rows", "shared", True, 1),
    (64, 3, 33, 4, 8, "noone3", "rk4", 5, Q16, "shared", "rows", False, 1),
    (65, 3, 70, 2, 2, "lin3", "euler", 5, Q5, "rows", "rows", True, -1),
    (128, 130, 2, 1, 1, "dup4", "rk4", 1, Q5, "rows", "shared", True, 1),
    (129, 3, 17, 4, 16, "u3_first9", "euler", 1, Q16, "rows", "rows", False, 1),
    (200, 3, 70, 2, 3, "std7", "rk4", 1, Q5, "shared", "shared", True, -1),
    (256, 130, 33, 2, 8, "high_pow", "euler", 5, Q5, "rows", "rows", True, 1),
    (512, 3, 17, 2, 2, "u3_x9", "rk4", 5, Q5, "rows", "shared", False, 1),
    (512, 1, 70, 4, 16, "deg2_no_xx", "euler", 5, Q16, "rows", "rows", True, -1),
    (33, 3, 33, 2, 8, "u3_mixed9", "rk4", 1, Q5, "shared", "rows", True, 1),
    (2, 130, 33, 4, 8, "std7", "euler", 5, Q16, "rows", "rows", False, -1),
]
CASE_IDS = [f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-K{c[4]}-{c[5]}-{c[6]}{c[7]}-Q{len(c[8])}-{c[9]}-{c[10]}"
            f"-{'cost' if c[11] else 'nocost'}-{'min' if c[12] > 0 else 'max'}" for c in CASES]


def coef_ensemble(rng, name, Rn, A):
    """tests/test_gpu_effect.py's ``_coef``: a decaying model and bootstrap-like replicates of it (every coefficient
    scaled by 1 + 0.3 z, one term in five outside the replicate's support, one coefficient below drop_below)."""
    exps = M.exps_of(name)
    F = exps.shape[0]
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[rng.random((Rn, A, F)) < 0.2] = 0.0
    coef[0] = base
    coef[1, A - 1, F - 1] = 0.5 * M.DROP_BELOW
    return coef


def inputs(seed_key, Rn, N, T, A, K, name, plan_mode="rows", w_mode="rows", with_cost=True):
    """(y0 [N], u [N, U], plans [K, T + pad] or [K, N, T + pad] int8, w [T + pad] or [N, T + pad], cost [K] or None,
    coef [R, A, F]): y0 ~ U(0.5, 3), u ~ U(0.6, 1.6), uniformly random plans and weights in [0, 1), costs in +-0.05;
    the padding of the plans holds out-of-range arms, that of the weights NaN."""
    rng = np.random.default_rng(M._seed(*seed_key))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    shape = (K, T + PAD_PLAN) if plan_mode == "shared" else (K, N, T + PAD_PLAN)
    plans = rng.integers(0, A, shape)
    plans[..., T:] = [A + 3, -2, 127][:PAD_PLAN]
    wshape = (T + PAD_W,) if w_mode == "shared" else (N, T + PAD_W)
    w = rng.uniform(0.0, 1.0, wshape)
    w[..., T:] = np.nan
    cost = rng.uniform(-0.05, 0.05, K) if with_cost else None
    return y0, u, plans.astype(np.int8), w, cost, coef_ensemble(rng, name, Rn, A)


def full_plans(plans, N, T):
    """[K, N, T] of either plan form."""
    return np.ascontiguousarray(plans[..., :T] if plans.ndim == 3
                                else np.broadcast_to(plans[:, None, :T], (plans.shape[0], N, T)))


@functools.lru_cache(maxsize=None)
def case(Rn, N, T, A, K, name, method, sub, q, plan_mode, w_mode, with_cost, sense):
    """The inputs of one parity case and its reference (computed once, read-only)."""
    y0, u, plans, w, cost, coef = inputs(("regimen", Rn, N, T, A, K, name, method, sub), Rn, N, T, A, K, name,
                                         plan_mode, w_mode, with_cost)
    ref = regimen(y0, u, full_plans(plans, N, T), coef, M.exps_of(name), DT, q, w[..., :T], cost, sense, method, sub)
    for a in (y0, u, plans, w, cost, coef) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return y0, u, plans, w, cost, coef, ref
