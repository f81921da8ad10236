"""numpy restatement of include/insite_effect.h, the reference of tests/test_effect_abi.py (CPU) and
tests/test_gpu_effect.py (GPU).  Helper only: no tests in this file.

Trajectories are ``oracle.insite_ref.rollout`` per replicate (its drop threshold is RHS_COEF_EPS = 1e-3, so the GPU
tests pass drop_below = 1e-3, or coefficients cleaned of everything below it), the order statistics ``np.sort`` and
the header's quantile formula, the standard deviation two-pass, and the NaN rule is applied last.
"""
from __future__ import annotations

import numpy as np

from oracle import insite_ref as R


def quantile_sorted(s, q):
    """The header's formula on s [n, ...] sorted ascending along axis 0 (no NaN), for one q in [0, 1]."""
    n = s.shape[0]
    pos = float(q) * (n - 1)
    i = min(int(np.floor(pos)), n - 1)
    g = pos - i
    lo, hi = s[i], s[min(i + 1, n - 1)]
    if g == 0.0:
        return lo.copy()
    with np.errstate(invalid="ignore"):
        return np.where(lo == hi, lo, lo + g * (hi - lo))


def stats(v, q):
    """v [R, ...] (replicate 0: the point model) -> [3 + Q, ...]: point, mean, std (ddof 1, two-pass), quantiles
    over v[1:]; wherever one of v[1:] is NaN every statistic but the point is NaN."""
    v = np.asarray(v, dtype=np.float64)
    rep = v[1:]
    n = rep.shape[0]
    bad = np.isnan(rep).any(axis=0)
    safe = np.where(bad[None], 0.0, rep)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean = safe.sum(axis=0) / n
        dev = safe - mean[None]
        std = np.sqrt((dev * dev).sum(axis=0) / (n - 1)) if n > 1 else np.full(mean.shape, np.nan)
        s = np.sort(safe, axis=0)
        rows = [v[0], mean, std] + [quantile_sorted(s, qq) for qq in q]
    out = np.stack(rows)
    out[1:, bad] = np.nan
    return out


def trajectories(y0, u, arm, coef, exps, dt, method="euler5", substeps=None):
    """[R, N, T]: the rollout of every row under every replicate's coefficients coef [R, A, F]; a replicate with a
    NaN coefficient gives NaN (insite_effect.h: a NaN coefficient is not a dropped term; the tests put NaN in
    every coefficient of such a replicate)."""
    Rn, N = coef.shape[0], arm.shape[0]
    bad = np.isnan(coef).any(axis=(1, 2))
    # one call for all replicates: row r N + p is row p under coef[r] (the oracle's per-row coefficient form)
    rows = np.repeat(np.where(bad[:, None, None], 0.0, coef), N, axis=0)
    out = R.rollout(np.tile(y0, Rn), np.tile(u, (Rn, 1)), np.tile(arm, (Rn, 1)), rows, exps, dt, method=method,
                    substeps=substeps).reshape((Rn,) + arm.shape)
    out[bad] = np.nan
    return out


def bands(y0, u, arm_a, arm_b, coef, exps, dt, q, method="euler5", substeps=None):
    """(out [n_series, 3 + Q, N, T], scale [N, T]): the definition, and the largest |yA| or |yB| over the replicates
    at every (row, step) -- the scale of the GPU tolerance (NaN replicates do not count)."""
    ya = trajectories(y0, u, arm_a, coef, exps, dt, method, substeps)
    series = [ya]
    both = [np.abs(ya)]
    if arm_b is not None:
        yb = trajectories(y0, u, arm_b, coef, exps, dt, method, substeps)
        series += [yb, ya - yb]
        both.append(np.abs(yb))
    scale = np.fmax.reduce(np.concatenate(both), axis=0)
    return np.stack([stats(v, q) for v in series]), scale
