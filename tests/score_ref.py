"""numpy restatement of include/insite_score.h, the reference of tests/test_score_abi.py (CPU) and
tests/test_gpu_score.py (GPU).  Helper only: no tests in this file.

Trajectories are ``effect_ref.trajectories``, the order statistics ``np.sort`` and ``effect_ref.quantile_sorted``, the
variance two-pass, the CRPS in the header's sorted form (on the values themselves, not shifted), the rank and the
bin in integer arithmetic.  Besides the sums it gives, per cell, the scale s' = max(max_r |v_r|, |y|) of the GPU
tolerance and the decision margin: the smallest |v_r - y|, |lo_j - y|, |hi_j - y| over s' -- a cell whose margin is
tiny may land in another bin, or on the other side of a band end, under a rounding-level change of a trajectory.
"""
from __future__ import annotations

import numpy as np

import effect_ref as E

FIXED = 6


def n_rows(levels, n_bins):
    return FIXED + int(n_bins) + 3 * len(levels)


def crps_pairwise(rep, y):
    """mean |v - y| - mean |v - v'| / 2 over the n values rep [n]: the definition the sorted form restates."""
    rep = np.asarray(rep, dtype=np.float64)
    return np.abs(rep - y).mean() - 0.5 * np.abs(rep[:, None] - rep[None, :]).mean()


def crps_sorted(rep, y):
    """The header's form for rep [n, ...] and y [...]."""
    n = rep.shape[0]
    s = np.sort(rep, axis=0)
    w = (2.0 * np.arange(n) - n + 1.0).reshape((n,) + (1,) * (rep.ndim - 1))
    return np.abs(rep - y).sum(axis=0) / n - (w * s).sum(axis=0) / (float(n) * float(n))


def cells(v, y_obs, active, levels, n_bins):
    """v [R, N, T] (replicate 0: the point model), y_obs [N, T], active [N, T] or None -> a dict of per-cell arrays:
    ``stat`` [S, N, T] (the cell's contribution to every row of sums; 0 where it has none), ``bound`` [S, N, T] (the
    per-cell error bound of the non-count rows in units of the tolerance, 0 on the count rows), ``scored``, ``bad``,
    ``observed`` [N, T], ``sprime`` and ``margin`` [N, T] (inf where the cell is not scored)."""
    v = np.asarray(v, dtype=np.float64)
    y_obs = np.asarray(y_obs, dtype=np.float64)
    Rn, N, T = v.shape
    n = Rn - 1
    B, L = int(n_bins), len(levels)
    S = n_rows(levels, B)
    act = np.ones((N, T), dtype=bool) if active is None else np.asarray(active) != 0
    observed = act & np.isfinite(y_obs)
    fin = np.isfinite(v).all(axis=0)
    scored, bad = observed & fin, observed & ~fin
    vs = np.where(scored[None], v, 0.0)
    y = np.where(scored, y_obs, 0.0)
    rep = vs[1:]
    c = rep[0]
    mean = c + (rep - c[None]).sum(axis=0) / n
    var = ((rep - mean[None]) ** 2).sum(axis=0) / (n - 1) if n > 1 else np.zeros((N, T))
    s = np.sort(rep, axis=0)
    stat = np.zeros((S, N, T))
    bound = np.zeros((S, N, T))
    sprime = np.maximum(np.abs(vs).max(axis=0), np.abs(y))
    stat[0] = 1.0
    stat[2] = (vs[0] - y) ** 2
    stat[3] = (mean - y) ** 2
    stat[4] = var
    stat[5] = crps_sorted(rep, y)
    bound[2:5] = 4.0 * sprime ** 2
    bound[5] = 2.0 * sprime
    rank2 = 2 * (rep < y[None]).sum(axis=0) + (rep == y[None]).sum(axis=0)
    bins = np.minimum(B - 1, (rank2 * B) // (2 * n))
    for b in range(B):
        stat[FIXED + b] = bins == b
    margin = np.abs(rep - y[None]).min(axis=0)
    for j, lam in enumerate(levels):
        lam = float(lam)
        lo, hi = E.quantile_sorted(s, 0.5 - 0.5 * lam), E.quantile_sorted(s, 0.5 + 0.5 * lam)
        pen = 2.0 / (1.0 - lam)
        r0 = FIXED + B + 3 * j
        stat[r0] = (lo <= y) & (y <= hi)
        stat[r0 + 1] = hi - lo
        stat[r0 + 2] = (hi - lo) + pen * np.maximum(lo - y, 0.0) + pen * np.maximum(y - hi, 0.0)
        bound[r0 + 1] = 2.0 * sprime
        bound[r0 + 2] = (2.0 + 2.0 * pen) * sprime
        margin = np.minimum(margin, np.minimum(np.abs(lo - y), np.abs(hi - y)))
    stat *= scored[None]
    bound *= scored[None]
    stat[1] = bad
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(scored, margin / sprime, np.inf)
    return {"stat": stat, "bound": bound, "scored": scored, "bad": bad, "observed": observed, "sprime": sprime,
            "margin": margin}


def group_sums(per_cell, group, n_groups):
    """[S, N, T] -> [G, S, T]: the rows of every group added (ids outside 0..G-1 contribute nothing)."""
    S, N, T = per_cell.shape
    g = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    out = np.zeros((n_groups, S, T))
    for i in range(n_groups):
        out[i] = per_cell[:, g == i].sum(axis=1)
    return out


def count_rows(levels, n_bins):
    """The rows of sums that are exact integers: 0, 1, the histogram, covered of every level."""
    B = int(n_bins)
    return [0, 1] + list(range(FIXED, FIXED + B)) + [FIXED + B + 3 * j for j in range(len(levels))]


def score_replicates(v, y_obs, active, levels, n_bins, group=None, n_groups=1):
    """(sums [G, S, T], bound [G, S, T], the per-cell dict) from trajectories v [R, N, T]."""
    c = cells(v, y_obs, active, levels, n_bins)
    return group_sums(c["stat"], group, n_groups), group_sums(c["bound"], group, n_groups), c


def score(y0, u, arm, coef, exps, dt, y_obs, active, levels, n_bins, group=None, n_groups=1, method="euler5",
          substeps=None):
    """The definition: ``score_replicates`` on ``effect_ref.trajectories``."""
    v = E.trajectories(y0, u, arm, coef, exps, dt, method, substeps)
    return score_replicates(v, y_obs, active, levels, n_bins, group, n_groups)
