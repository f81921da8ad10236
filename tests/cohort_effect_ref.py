"""numpy restatement of include/insite_cohort.h, the reference of tests/test_cohort_abi.py (CPU) and
tests/test_gpu_cohort_effect.py (GPU).  Helper only: no tests in this file.

Trajectories are ``effect_ref.trajectories``, the weights ``insite_amd.bootstrap.weights`` (row 0 all ones; all ones
under "none"), the sums, weight sums and means as the header defines them (a row outside [0, n_groups) or with weight
0 is left out by indexing, never multiplied by zero), and the statistics ``effect_ref.stats`` on m[:, g, s, :].
"""
from __future__ import annotations

import numpy as np

import effect_ref as E


def weights(weighting, seed, R, N, patient_offset=0):
    """int64 [R, N]: the weights of the header."""
    from insite_amd import bootstrap
    if weighting == "none":
        return np.ones((R, N), dtype=np.int64)
    assert weighting == "poisson"
    return bootstrap.weights(seed, R, N, patient_offset)


def sums(ys, w, group, n_groups):
    """ys: list of [R, N, T] (yA or yA, yB); w int64 [R, N]; group int [N] or None.
    -> (S [R, G, n_series, T], wsum [R, G] float64 of exact integers, scale [G, T])."""
    R, N, T = ys[0].shape
    grp = np.zeros(N, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    S = np.zeros((R, n_groups, len(ys), T))
    wsum = np.zeros((R, n_groups))
    scale = np.zeros((n_groups, T))
    for g in range(n_groups):
        rows = np.nonzero(grp == g)[0]
        if rows.size:
            scale[g] = np.fmax.reduce(np.concatenate([np.abs(y[:, rows]).reshape(-1, T) for y in ys]), axis=0)
        for r in range(R):
            sel = rows[w[r, rows] > 0]
            wsum[r, g] = float(w[r, sel].sum())
            for s, y in enumerate(ys):
                S[r, g, s] = (w[r, sel, None] * y[r, sel]).sum(axis=0)
    return S, wsum, scale


def means(S, wsum):
    """m [R, G, 1 or 3, T]: sums / wsum (0 / 0 = NaN) and, with two plans, the paired difference."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = S / wsum[:, :, None, None]
    if m.shape[2] == 2:
        m = np.concatenate([m, m[:, :, :1] - m[:, :, 1:2]], axis=2)
    return m


def finalize(S, wsum, q):
    """out [G, S, 3 + Q, T] from the sums."""
    m = means(S, wsum)
    return np.stack([np.stack([E.stats(m[:, g, s], q) for s in range(m.shape[2])]) for g in range(m.shape[1])])


def cohort(y0, u, arm_a, arm_b, coef, exps, dt, q, group=None, n_groups=1, weighting="poisson", seed=0,
           patient_offset=0, method="euler5", substeps=None):
    """(out [G, S, 3 + Q, T], S [R, G, n_series, T], wsum [R, G], scale [G, T]): the definition; scale[g, k] is the
    largest |yA| or |yB| over the replicates and the contributing rows of group g (NaN replicates do not count)."""
    ys = [E.trajectories(y0, u, arm_a, coef, exps, dt, method, substeps)]
    if arm_b is not None:
        ys.append(E.trajectories(y0, u, arm_b, coef, exps, dt, method, substeps))
    w = weights(weighting, seed, coef.shape[0], y0.shape[0], patient_offset)
    S, wsum, scale = sums(ys, w, group, n_groups)
    return finalize(S, wsum, q), S, wsum, scale
