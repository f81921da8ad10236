"""numpy restatement of include/insite_rulevalue.h, the reference of tests/test_rulevalue_abi.py (CPU) and
tests/test_gpu_rulevalue.py (GPU), and the parity cases the two share.  Helper only: no tests in this file.

The closed loops (objective J and exposure E) are ``feedback_ref.closed_loop``, the choice inside a replicate is
``regimen_ref.choose``, the row weights ``cohort_effect_ref.weights``, the statistics ``effect_ref.stats``.  A row outside
[0, n_groups) or with weight 0 is left out by indexing, never multiplied by zero.  The sums are numpy sums (the kernel's
are FMAs in a fixed order: the difference is inside the GPU tolerance).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cohort_effect_ref as C  # noqa: E402
import effect_ref as E  # noqa: E402
import feedback_ref as F  # noqa: E402
import library_matrix as M  # noqa: E402
import policy_ref as P  # noqa: E402
import regimen_ref as G  # noqa: E402


def series_names(K):
    return ([f"value_{j}" for j in range(K)]
            + ["personalised", "assigned", "best_fixed", "gain_personalised", "gain_assigned", "optimism"]
            + [f"share_{j}" for j in range(K)] + [f"exposure_{j}" for j in range(K)]
            + ["exposure_personalised", "exposure_assigned", "exposure_best_fixed"])


def sums(J, Ex, best, assign, om, group, n_groups):
    """J, Ex [R, N, K], best [R, N] (-1: abstains), assign int [N], om int64 [R, N], group int [N] or None ->
    (S [R, G, 3 K + 4], wsum [R, G]): the seven column families of the header."""
    Rn, N, K = J.shape
    grp = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    S = np.zeros((Rn, n_groups, 3 * K + 4))
    wsum = np.zeros((Rn, n_groups))
    ok_asg = (assign >= 0) & (assign < K)
    for g in range(n_groups):
        rows = np.nonzero(grp == g)[0]
        for r in range(Rn):
            sel = rows[om[r, rows] > 0]
            w = om[r, sel].astype(np.float64)
            wsum[r, g] = w.sum()
            b = best[r, sel]
            a = np.clip(assign[sel], 0, K - 1)
            idx = np.arange(sel.size)
            with np.errstate(invalid="ignore"):
                for j in range(K):
                    S[r, g, j] = (w * J[r, sel, j]).sum()
                    S[r, g, K + 2 + j] = w[b == j].sum()
                    S[r, g, 2 * K + 2 + j] = (w * Ex[r, sel, j]).sum()
                S[r, g, K] = (w * np.where(b >= 0, J[r, sel][idx, np.maximum(b, 0)], np.nan)).sum()
                S[r, g, K + 1] = (w * np.where(ok_asg[sel], J[r, sel][idx, a], np.nan)).sum()
                S[r, g, 3 * K + 2] = (w * np.where(b >= 0, Ex[r, sel][idx, np.maximum(b, 0)], np.nan)).sum()
                S[r, g, 3 * K + 3] = (w * np.where(ok_asg[sel], Ex[r, sel][idx, a], np.nan)).sum()
    return S, wsum


def finalize(S, wsum, q, sense=1):
    """(out [G, 3 K + 9, 3 + Q], fixwin [G, K], best_fixed int32 [G]) from the sums."""
    Rn, Gn, Cn = S.shape
    K = (Cn - 4) // 3
    s = float(sense)
    value, jf, bf, _ = P.fixed_choice(S, wsum, K, sense)
    with np.errstate(invalid="ignore", divide="ignore"):
        pers = S[:, :, K] / wsum
        asg = S[:, :, K + 1] / wsum
        share = S[:, :, K + 2:2 * K + 2] / wsum[:, :, None]
        expo = S[:, :, 2 * K + 2:] / wsum[:, :, None]                  # K rules, personalised, assigned
        ebf = np.where(jf >= 0, np.take_along_axis(expo[:, :, :K], np.maximum(jf, 0)[:, :, None], axis=2)[:, :, 0],
                       np.nan)
        ser = ([value[:, :, j] for j in range(K)]
               + [pers, asg, bf, s * bf - s * pers, s * bf - s * asg, s * asg - s * pers]
               + [share[:, :, j] for j in range(K)] + [expo[:, :, j] for j in range(K + 2)] + [ebf])
    out = np.stack([E.stats(v, q) for v in ser])                      # [S, 3 + Q, G]
    fixwin = np.stack([(jf[1:] == j).sum(axis=0) for j in range(K)], axis=1).astype(np.float64) / float(Rn - 1)
    return np.ascontiguousarray(out.transpose(2, 0, 1)), fixwin, jf[0].astype(np.int32)


def rule_value(y0, u, theta, rules, coef, exps, dt, q, w, cost=None, arm_cost=None, sense=1, assign=None, group=None,
               n_groups=1, weighting="poisson", seed=0, patient_offset=0, method="euler5", substeps=None):
    """The definition.  theta [N, 2 K], rules [K, 4], w [N, T] (or [T]).  dict: out, fixwin, best_fixed, assign, sums,
    wsum, scale [G] (s_g: policy_ref's group scale, max over replicates, rows of the group and rules of |cost_j| +
    sum_k |w| |y|, plus sum_a |arm_cost_a|), dmargin (the smallest relative decision margin of any row), row_margin (the
    smallest relative row-level argmin margin), fixed_margin (the smallest relative margin between fixed-rule cohort
    values in any replicate), J, E, best, jfix."""
    N = np.asarray(y0).shape[0]
    K = len(rules)
    w = np.broadcast_to(w, (N, np.shape(w)[-1]))
    cl = F.closed_loop(y0, u, theta, rules, coef, exps, dt, w, cost, arm_cost, method, substeps)
    J, Ex, row_scale = cl["J"], cl["E"], cl["scale"]
    Rn = J.shape[0]
    best, _, margin = G.choose(J, sense)
    assign = best[0].astype(np.int32) if assign is None else np.asarray(assign, dtype=np.int32)
    om = C.weights(weighting, seed, Rn, N, patient_offset)
    S, wsum = sums(J, Ex, best, assign, om, group, n_groups)
    out, fixwin, best_fixed = finalize(S, wsum, q, sense)
    grp = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    scale = np.zeros(n_groups)
    for g in range(n_groups):
        rows = grp == g
        if rows.any():
            scale[g] = np.fmax.reduce(row_scale[rows])
    with np.errstate(invalid="ignore", divide="ignore"):
        rm = np.fmin.reduce(margin, axis=0) / row_scale
    rm = np.where(np.isnan(rm), np.inf, rm)
    _, jf, _, fm = P.fixed_choice(S, wsum, K, sense)
    with np.errstate(invalid="ignore", divide="ignore"):
        fmr = fm / scale[None, :]
    return {"out": out, "fixwin": fixwin, "best_fixed": best_fixed, "assign": assign, "sums": S, "wsum": wsum,
            "scale": scale, "dmargin": float(cl["dmargin"].min()), "row_margin": float(rm.min()),
            "fixed_margin": float(np.where(np.isnan(fmr), np.inf, fmr).min()), "J": J, "E": Ex, "best": best,
            "jfix": jf, "om": om}


# ---------------------------------------------------------------------------------------------------
# the parity cases (tests/test_gpu_rulevalue.py runs them; tests/test_rulevalue_abi.py asserts their input conditions)
# ---------------------------------------------------------------------------------------------------
DT, Q5, Q16 = G.DT, G.Q5, G.Q16
PAD_OUT, POISON = 3, G.POISON
SEED = 11   # of the Poisson row weights

# (R, N, T, n_arms, K, G, table, method, substeps, q, theta, weights, cost, arm_cost, sense, weighting, patient_offset,
#  assign, grouped, key): a sample, not the product.  R = 2 (n = 1), partly filled top tiles (3, 17, 65, 130), more
# than one replicate tile (65, 130, 512, 4096), the finalize sort at its cap (4096); N = 1, one partial ballot word (3,
# 40), three words (130), several patient chunks (700); T on either side of 16 (feedback_rules' chunk) and of the
# 64-step window; every rule bucket (K = 1, 2 | 3 | 8 | 16); 1, 2 and 4 arms; G = 1, 3, 64 with excluded rows (group
# ids -1 and G); both weightings, two patient offsets, both senses, cost and arm_cost given and NULL, shared and padded
# per-row thresholds and weights (the padding holds NaN), the assignment given and NULL; the periods of the rules
# cycle through 1, 1, 2, 5 and T + 3 and start_on alternates (feedback_ref.rule_table); several tables of
# tests/library_matrix.py, both methods, substeps 1 and 5.  Without a cost two rules that end up on the same arm at
# every step tie exactly, so the case without one has K = 1.  key: picks the random stream (chosen so that
# tests/test_rulevalue_abi.py's input conditions hold).
CASES = [
    (17, 130, 17, 2, 3, 3, "std7", "euler", 5, Q5, "rows", "shared", True, True, 1, "poisson", 1000003, "null", True, 0),
    (64, 3, 33, 4, 8, 1, "noone3", "rk4", 5, Q16, "shared", "rows", True, True, 1, "none", 0, "null", False, 0),
    (65, 130, 70, 2, 2, 64, "lin3", "euler", 5, Q5, "rows", "rows", True, False, 1, "none", 0, "given", True, 0),
    (130, 700, 2, 2, 3, 3, "dup4", "rk4", 1, Q5, "rows", "shared", True, True, 1, "poisson", 7, "null", True, 0),
    (130, 3, 33, 4, 16, 1, "u3_first9", "euler", 1, Q16, "rows", "rows", True, True, 1, "none", 0, "null", False, 0),
    (512, 40, 16, 2, 8, 3, "high_pow", "euler", 5, Q5, "rows", "rows", True, False, 1, "poisson", 0, "given", True, 0),
    (4096, 3, 2, 2, 2, 1, "u3_x9", "rk4", 5, Q5, "rows", "shared", True, True, 1, "none", 0, "null", False, 0),
    (4096, 130, 1, 2, 3, 3, "std7", "euler", 5, Q16, "rows", "rows", True, False, -1, "poisson", 0, "null", True, 0),
    (17, 700, 65, 4, 8, 3, "deg2_no_xx", "euler", 5, Q16, "rows", "rows", True, True, -1, "poisson", 12345, "null",
     True, 0),
    (2, 3, 1, 1, 2, 1, "x_only", "euler", 1, Q5, "shared", "shared", True, True, 1, "none", 0, "null", False, 0),
    (3, 1, 2, 2, 3, 1, "bias_x", "rk4", 1, Q5, "rows", "rows", True, False, -1, "poisson", 0, "given", True, 0),
    (17, 3, 17, 2, 1, 1, "dup4", "rk4", 1, Q5, "shared", "shared", False, True, 1, "none", 0, "null", False, 0),
]
CASE_IDS = [f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-K{c[4]}-G{c[5]}-{c[6]}-{c[7]}{c[8]}-Q{len(c[9])}-{c[10]}-{c[11]}"
            f"-{'cost' if c[12] else 'nocost'}-{'armcost' if c[13] else 'noarmcost'}-{'min' if c[14] > 0 else 'max'}"
            f"-{c[15]}-off{c[16]}-assign{c[17]}" for c in CASES]


def inputs(seed_key, Rn, N, T, A, K, Gn, name, theta_mode="rows", w_mode="rows", with_cost=True, with_ac=True,
           assign_mode="null", grouped=True):
    """``feedback_ref.inputs`` plus (group int32 [N] or None, assign int32 [N] or None: uniformly random rules)."""
    y0, u, theta, rules, w, cost, arm_cost, coef = F.inputs(seed_key, Rn, N, T, A, K, name, theta_mode, w_mode,
                                                            with_cost, with_ac)
    rng = np.random.default_rng(M._seed("rulevalue-extra", *seed_key))
    group = P.groups_of(rng, N, Gn, grouped)
    assign = rng.integers(0, K, N).astype(np.int32) if assign_mode == "given" else None
    return y0, u, theta, rules, w, cost, arm_cost, coef, group, assign


def reference(y0, u, theta, rules, coef, name, q, w, cost, arm_cost, sense, assign, group, Gn, weighting, seed, off,
              method, sub, T):
    N, K = y0.shape[0], len(rules)
    return rule_value(y0, u, F.full_theta(theta, N, K), rules, coef, M.exps_of(name), DT, q,
                      np.broadcast_to(w[..., :T], (N, T)), cost, arm_cost, sense, assign, group, Gn, weighting, seed,
                      off, method, sub)


@functools.lru_cache(maxsize=None)
def case(Rn, N, T, A, K, Gn, name, method, sub, q, theta_mode, w_mode, with_cost, with_ac, sense, weighting, off,
         assign_mode, grouped, key):
    """The inputs of one parity case and its reference (computed once, read-only)."""
    y0, u, theta, rules, w, cost, arm_cost, coef, group, assign = inputs(
        ("rulevalue", Rn, N, T, A, K, Gn, name, method, sub, key), Rn, N, T, A, K, Gn, name, theta_mode, w_mode,
        with_cost, with_ac, assign_mode, grouped)
    ref = reference(y0, u, theta, rules, coef, name, q, w, cost, arm_cost, sense, assign, group, Gn, weighting, SEED,
                    off, method, sub, T)
    for a in (y0, u, theta, rules, w, cost, arm_cost, coef, group, assign) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return y0, u, theta, rules, w, cost, arm_cost, coef, group, assign, ref
