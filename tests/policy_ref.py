"""numpy restatement of include/insite_policy.h, the reference of tests/test_policy_abi.py (CPU) and
tests/test_gpu_policy.py (GPU), and the parity cases the two share.  Helper only: no tests in this file.

The objectives and the choice inside a replicate are ``regimen_ref.objectives`` / ``choose``, the row weights
``cohort_effect_ref.weights``, the statistics ``effect_ref.stats``.  A row outside [0, n_groups) or with weight 0 is
left out by indexing, never multiplied by zero.  The sums are numpy sums (the kernel's are FMAs in a fixed order: the
difference is inside the GPU tolerance).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cohort_effect_ref as C  # noqa: E402
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
import regimen_ref as G  # noqa: E402


def series_names(K):
    return ([f"value_{j}" for j in range(K)]
            + ["personalised", "rule", "best_fixed", "gain_personalised", "gain_rule", "optimism"]
            + [f"share_{j}" for j in range(K)])


def sums(J, best, rule, om, group, n_groups):
    """J [R, N, K], best [R, N] (-1: abstains), rule int [N], om int64 [R, N], group int [N] or None ->
    (S [R, G, 2 K + 2], wsum [R, G])."""
    Rn, N, K = J.shape
    grp = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    S = np.zeros((Rn, n_groups, 2 * K + 2))
    wsum = np.zeros((Rn, n_groups))
    ok_rule = (rule >= 0) & (rule < K)
    for g in range(n_groups):
        rows = np.nonzero(grp == g)[0]
        for r in range(Rn):
            sel = rows[om[r, rows] > 0]
            w = om[r, sel].astype(np.float64)
            wsum[r, g] = w.sum()
            with np.errstate(invalid="ignore"):
                for j in range(K):
                    S[r, g, j] = (w * J[r, sel, j]).sum()
                    S[r, g, K + 2 + j] = w[best[r, sel] == j].sum()
                b = best[r, sel]
                S[r, g, K] = (w * np.where(b >= 0, J[r, sel, np.maximum(b, 0)], np.nan)).sum()
                rl = rule[sel]
                S[r, g, K + 1] = (w * np.where(ok_rule[sel], J[r, sel, np.clip(rl, 0, K - 1)], np.nan)).sum()
    return S, wsum


def fixed_choice(S, wsum, K, sense=1):
    """(value [R, G, K], jfix [R, G] (-1: abstains), best_fixed value [R, G], margin [R, G]): the best fixed plan of
    every (replicate, group) by the header's strict comparison; margin = second-best - best of s value."""
    with np.errstate(invalid="ignore", divide="ignore"):
        value = S[:, :, :K] / wsum[:, :, None]
    jf, _, margin = G.choose(value, sense)
    bf = np.where(jf >= 0, np.take_along_axis(value, np.maximum(jf, 0)[:, :, None], axis=2)[:, :, 0], np.nan)
    return value, jf, bf, margin


def finalize(S, wsum, q, sense=1):
    """(out [G, 2 K + 6, 3 + Q], fixwin [G, K], best_fixed int32 [G]) from the sums."""
    Rn, Gn, Cn = S.shape
    K = Cn // 2 - 1
    s = float(sense)
    value, jf, bf, _ = fixed_choice(S, wsum, K, sense)
    with np.errstate(invalid="ignore", divide="ignore"):
        pers = S[:, :, K] / wsum
        rule = S[:, :, K + 1] / wsum
        share = S[:, :, K + 2:] / wsum[:, :, None]
        ser = ([value[:, :, j] for j in range(K)] + [pers, rule, bf, s * bf - s * pers, s * bf - s * rule,
                                                      s * rule - s * pers]
               + [share[:, :, j] for j in range(K)])
    out = np.stack([E.stats(v, q) for v in ser])                      # [S, 3 + Q, G]
    fixwin = np.stack([(jf[1:] == j).sum(axis=0) for j in range(K)], axis=1).astype(np.float64) / float(Rn - 1)
    return np.ascontiguousarray(out.transpose(2, 0, 1)), fixwin, jf[0].astype(np.int32)


def policy(y0, u, plans, coef, exps, dt, q, w, cost=None, sense=1, rule=None, group=None, n_groups=1,
           weighting="poisson", seed=0, patient_offset=0, method="euler5", substeps=None):
    """The definition.  plans [K, N, T], w [N, T] (or [T]).  dict: out, fixwin, best_fixed, rule, sums, wsum, scale
    [G] (s_g = max over replicates, rows of the group and plans of |cost_j| + sum_k |w| |y|), row_margin (the smallest
    relative row-level argmin margin), fixed_margin (the smallest relative margin between fixed-plan cohort values in
    any replicate), J, best, jfix."""
    K, N, T = plans.shape
    w = np.broadcast_to(w, (N, T))
    J, row_scale = G.objectives(y0, u, plans, coef, exps, dt, w, cost, method, substeps)
    Rn = J.shape[0]
    best, _, margin = G.choose(J, sense)
    rule = best[0].astype(np.int32) if rule is None else np.asarray(rule, dtype=np.int32)
    om = C.weights(weighting, seed, Rn, N, patient_offset)
    S, wsum = sums(J, best, rule, om, group, n_groups)
    out, fixwin, best_fixed = finalize(S, wsum, q, sense)
    grp = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    scale = np.zeros(n_groups)
    for g in range(n_groups):
        rows = grp == g
        if rows.any():
            scale[g] = np.fmax.reduce(row_scale[rows])
    inc = (grp >= 0) & (grp < n_groups)
    with np.errstate(invalid="ignore", divide="ignore"):
        rm = np.fmin.reduce(margin, axis=0) / row_scale
    rm = np.where(np.isnan(rm), np.inf, rm)
    row_margin = float(rm.min())                                       # every row: the rule is computed for all
    _, jf, _, fm = fixed_choice(S, wsum, K, sense)
    with np.errstate(invalid="ignore", divide="ignore"):
        fmr = fm / scale[None, :]
    fixed_margin = float(np.where(np.isnan(fmr), np.inf, fmr).min())
    return {"out": out, "fixwin": fixwin, "best_fixed": best_fixed, "rule": rule, "sums": S, "wsum": wsum,
            "scale": scale, "row_margin": row_margin, "fixed_margin": fixed_margin, "J": J, "best": best, "jfix": jf,
            "included": inc}


# ---------------------------------------------------------------------------------------------------
# the parity cases (tests/test_gpu_policy.py runs them; tests/test_policy_abi.py asserts their input conditions)
# ---------------------------------------------------------------------------------------------------
DT, Q5, Q16 = G.DT, G.Q5, G.Q16
PAD_OUT, POISON = 3, G.POISON

# (R, N, T, n_arms, K, G, table, method, substeps, q, plans, weights, cost, sense, weighting, patient_offset, rule,
#  grouped, variant): a sample, not the product.  R = 2 (n = 1), the partly filled top tile (3, 17, 65, 130), more than
# one replicate tile (65, 130, 512, 4096), the finalize sort at its cap (4096); N = 1, one partial ballot word (3), three
# words (130), several patient chunks (700); T on either side of the 64-step window; every plan bucket (K = 1, 2 | 3 |
# 8 | 16), 16 at 4 arms (the largest register instance); 1, 2 and 4 arms; G = 1, 3, 64 with excluded rows (group ids
# -1 and G); both weightings, two patient offsets, both senses, cost given and NULL, shared and padded per-row plans
# and weights (the padding holds out-of-range arms and NaN), the rule given and NULL; every table of
# tests/library_matrix.py, both methods, substeps 1 and 5.  With one arm every plan is the same trajectory, so those
# cases have K = 1 or R < 17.  grouped False: group NULL (G = 1).  variant: picks the random stream (the seeds are
# chosen so that tests/test_policy_abi.py's input conditions hold).
CASES = [
    (2, 3, 1, 1, 1, 1, "x_only", "euler", 1, Q5, "shared", "shared", True, 1, "none", 0, "null", False, 0),
    (3, 1, 2, 2, 2, 1, "bias_x", "rk4", 1, Q5, "rows", "rows", True, -1, "poisson", 0, "given", True, 0),
    (17, 130, 63, 2, 3, 3, "std7", "euler", 5, Q5, "rows", "shared", True, 1, "poisson", 1000003, "null", True, 0),
    (64, 3, 64, 4, 8, 1, "noone3", "rk4", 5, Q16, "shared", "rows", False, 1, "none", 0, "null", False, 0),
    (65, 130, 65, 2, 2, 64, "lin3", "euler", 5, Q5, "rows", "rows", True, -1, "none", 0, "given", True, 0),
    (130, 700, 2, 2, 3, 3, "dup4", "rk4", 1, Q5, "rows", "shared", True, 1, "poisson", 7, "null", True, 3),
    (130, 3, 130, 4, 16, 1, "u3_first9", "euler", 1, Q16, "rows", "rows", False, 1, "none", 0, "null", False, 0),
    (512, 130, 63, 2, 8, 3, "high_pow", "euler", 5, Q5, "rows", "rows", True, 1, "poisson", 0, "given", True, 0),
    (4096, 3, 2, 2, 2, 1, "u3_x9", "rk4", 5, Q5, "rows", "shared", False, 1, "none", 0, "null", False, 0),
    (4096, 130, 1, 2, 3, 3, "std7", "euler", 5, Q16, "rows", "rows", True, -1, "poisson", 0, "null", True, 0),
    (17, 700, 65, 4, 8, 3, "deg2_no_xx", "euler", 5, Q16, "rows", "rows", True, -1, "poisson", 12345, "null", True, 0),
    (3, 3, 64, 1, 2, 1, "u3_mixed9", "rk4", 1, Q5, "shared", "rows", True, 1, "none", 0, "given", False, 0),
    (65, 130, 33, 4, 4, 3, "std7", "rk4", 1, Q5, "rows", "rows", False, 1, "poisson", 0, "null", True, 0),
]
CASE_IDS = [f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-K{c[4]}-G{c[5]}-{c[6]}-{c[7]}{c[8]}-Q{len(c[9])}-{c[10]}-{c[11]}"
            f"-{'cost' if c[12] else 'nocost'}-{'min' if c[13] > 0 else 'max'}-{c[14]}-off{c[15]}-rule{c[16]}"
            for c in CASES]
SEED = 11   # of the Poisson row weights


def groups_of(rng, N, Gn, grouped):
    """int32 [N] with ids in -1..G (-1 and G exclude the row), every group non-empty where N allows; or None."""
    if not grouped:
        return None
    g = rng.integers(-1, Gn + 1, N)
    g[:min(N, Gn)] = np.arange(min(N, Gn))
    return g.astype(np.int32)


def inputs(seed_key, Rn, N, T, A, K, Gn, name, plan_mode="rows", w_mode="rows", with_cost=True, rule_mode="null",
           grouped=True):
    """``regimen_ref.inputs`` plus (group int32 [N] or None, rule int32 [N] or None: uniformly random plans)."""
    y0, u, plans, w, cost, coef = G.inputs(seed_key, Rn, N, T, A, K, name, plan_mode, w_mode, with_cost)
    rng = np.random.default_rng(M._seed("policy-extra", *seed_key))
    group = groups_of(rng, N, Gn, grouped)
    rule = rng.integers(0, K, N).astype(np.int32) if rule_mode == "given" else None
    return y0, u, plans, w, cost, coef, group, rule


@functools.lru_cache(maxsize=None)
def case(Rn, N, T, A, K, Gn, name, method, sub, q, plan_mode, w_mode, with_cost, sense, weighting, off, rule_mode,
         grouped, variant):
    """The inputs of one parity case and its reference (computed once, read-only)."""
    y0, u, plans, w, cost, coef, group, rule = inputs(("policy", Rn, N, T, A, K, Gn, name, method, sub, variant), Rn,
                                                      N, T, A, K, Gn, name, plan_mode, w_mode, with_cost, rule_mode,
                                                      grouped)
    ref = policy(y0, u, G.full_plans(plans, N, T), coef, M.exps_of(name), DT, q, w[..., :T], cost, sense, rule, group,
                 Gn, weighting, SEED, off, method, sub)
    for a in (y0, u, plans, w, cost, coef, group, rule) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return y0, u, plans, w, cost, coef, group, rule, ref
