"""The patient-level bootstrap of the treatment-segment discovery (include/insite_segboot.h) restated in plain numpy:
what tests/test_segboot_abi.py (CPU) and tests/test_gpu_segboot.py (GPU) share.

Helper only: no tests in this file.  The per-(patient, arm) moments are built from the literal segment walk
(``oracle.segments_ref.segment_bounds``) and the derivative of ``tests/library_matrix._xdot_segment``; the weighted
Gram uses ``tests/bootstrap_ref``'s weights, monomials and entries, arm by arm.  Every sum takes its working dtype as
an argument or from its inputs and returns the per-entry SCALE (the sum of the absolute values of what it adds) next
to the value, as tests/library_matrix.py does.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_ref as BR  # noqa: E402
import library_matrix as M  # noqa: E402
from oracle import segments_ref as S  # noqa: E402


def moments(x, arm_steps, seq_len, dt, n_arms, fd, dtype=np.float64):
    """(mom [N, A, 5], S_mom [N, A, 5]): {count, sum x, sum x^2, sum x_dot, sum x_dot x} over the rows that patient
    p's segments add to arm a, and the same sums of absolute values.  seq_len is clamped to [0, n_steps - 1]; an arm
    outside [0, n_arms) reaches nothing."""
    N, T = x.shape
    mom = np.zeros((N, n_arms, 5), dtype=dtype)
    sc = np.zeros((N, n_arms, 5), dtype=dtype)
    for p in range(N):
        L = min(max(int(seq_len[p]), 0), T - 1)
        for a, lo, hi in S.segment_bounds(arm_steps[p], L):
            if not 0 <= a < n_arms:
                continue
            xs = np.asarray(x[p, lo:hi + 1], dtype=dtype)
            xd = M._xdot_segment(xs, dt, fd)
            mom[p, a] += [xs.shape[0], xs.sum(), (xs * xs).sum(), xd.sum(), (xd * xs).sum()]
            ax, ad = np.abs(xs), np.abs(xd)
            sc[p, a] += [xs.shape[0], ax.sum(), (xs * xs).sum(), ad.sum(), (ad * ax).sum()]
    return mom, sc


def gram(mom, u, exps, R, seed, patient_offset=0, scale_mom=None, weights=None):
    """(G [R, A, F, F], b [R, A, F], S_G, S_b): G[r, a] = sum_p w_rp g_pa over the patients with mom[p, a, 0] > 0
    (left out by indexing otherwise: whatever their moments hold reaches nothing), ONE weight per (replicate,
    patient) for every arm.  The scales are the same sums over the entries of ``scale_mom`` (default |mom|) and
    |u|.  ``weights`` [R, N] replaces the drawn ones."""
    mom = np.asarray(mom)
    dt = mom.dtype
    exps = np.asarray(exps)
    N, A = mom.shape[:2]
    F = exps.shape[0]
    u = np.asarray(u, dtype=dt).reshape(N, -1)
    w = (BR.weights(seed, R, N, patient_offset) if weights is None else np.asarray(weights)).astype(dt)
    sm = np.abs(mom) if scale_mom is None else np.asarray(scale_mom, dtype=dt)
    G = np.zeros((R, A, F, F), dtype=dt)
    b = np.zeros((R, A, F), dtype=dt)
    SG, Sb = np.zeros_like(G), np.zeros_like(b)
    for a in range(A):
        idx = np.nonzero(mom[:, a, 0] > 0)[0]
        if not idx.size:
            continue
        g, h = BR.entries(mom[idx, a], u[idx], exps)
        sg, sh = BR.entries(sm[idx, a], np.abs(u[idx]), exps)
        wa = w[:, idx]
        G[:, a] = np.tensordot(wa, g, axes=1)
        b[:, a] = np.tensordot(wa, h, axes=1)
        SG[:, a] = np.tensordot(wa, np.abs(sg), axes=1)
        Sb[:, a] = np.tensordot(wa, np.abs(sh), axes=1)
    return G, b, SG, Sb


def stlsq_margin(G, b, threshold, alpha, max_iter=100):
    """The smallest ||c_i| - threshold| / threshold over every coefficient of every ridge iterate that
    ``oracle.insite_ref.stlsq_gram`` forms on (G, b): how far the thresholding decisions of the system are from a
    tie."""
    F = G.shape[0]
    ind = np.ones(F, dtype=bool)
    prev = np.ones(F, dtype=bool)
    margin = np.inf
    for _ in range(max_iter):
        if not ind.any():
            break
        idx = np.nonzero(ind)[0]
        c = np.zeros(F)
        c[idx] = np.linalg.solve(G[np.ix_(idx, idx)] + alpha * np.eye(idx.size), b[idx])
        margin = min(margin, float(np.abs(np.abs(c[idx]) - threshold).min() / threshold))
        big = np.abs(c) >= threshold
        c[~big] = 0.0
        ind = big
        pattern = c != 0
        if int(ind.sum()) == F or np.array_equal(pattern, prev):
            break
        prev = pattern
    return margin


@functools.lru_cache(maxsize=None)
def segment_inputs(name, n_arms):
    """``library_matrix.segment_inputs`` for 2..4 arms.  That recipe draws "another arm" and so cannot make a one-arm
    cohort: for one arm it is the two-arm cohort with every read arm set to 0 and the arms from seq_len on -- which
    the reference never reads -- set to 1 (still poison: read, it would end the last segment early)."""
    if n_arms >= 2:
        return M.segment_inputs(name, n_arms)
    x, u, arm, sl = M.segment_inputs(name, 2)
    arm = np.zeros_like(arm)
    for p in range(arm.shape[0]):
        arm[p, sl[p]:] = 1
    arm.setflags(write=False)
    return x, u, arm, sl


@functools.lru_cache(maxsize=None)
def moments_case(name, n_arms, fd, dtype=np.float64):
    x, _, arm, sl = segment_inputs(name, n_arms)
    out = moments(x, arm, sl, M.DT, n_arms, fd, dtype)
    for a in out:
        a.setflags(write=False)
    return out


def numpy_moments(rng, N, n_arms):
    """[N, A, 5] built directly: ``bootstrap_ref.numpy_moments`` per arm, each (patient, arm) visited with
    probability 0.6 (five zeros otherwise); with N >= 3 patient 0 visits every arm, patient 1 none and patient 2
    only the last."""
    mom = np.stack([BR.numpy_moments(rng, N) for _ in range(n_arms)], axis=1)
    on = rng.random((N, n_arms)) < 0.6
    if N >= 3:
        on[0], on[1] = True, False
        on[2] = False
        on[2, n_arms - 1] = True
    mom[~on] = 0.0
    return mom


# the fit case of tests/test_gpu_segboot.py (its precondition is checked on the CPU in tests/test_segboot_abi.py)
FIT_R, FIT_SEED, FIT_DT = 33, 5, 0.1
FIT_THRESHOLD, FIT_ALPHA = 0.15, 0.5      # the planted coefficients are 0.2 .. 0.9; margin 0.18 (see stlsq_margin)


@functools.lru_cache(maxsize=None)
def fit_case():
    """``oracle.segments_ref.synthetic_cohort``: 4 arms, noise-free, 300 patients of 30 steps with switches and
    ragged lengths, and its restated systems: (x, u, arm_steps, seq_len, exps, mom, G [R, 4, F, F], b [R, 4, F])."""
    from oracle import insite_ref as R
    x, u, arm, sl = S.synthetic_cohort(300, 30, np.random.default_rng(42), switch_p=0.1, dt=FIT_DT, min_len=5)
    exps = R.poly_library(2, 2, True).astype(np.int64)
    mom, _ = moments(x, arm, sl, FIT_DT, 4, "order1")
    G, b, _, _ = gram(mom, u, exps, FIT_R, FIT_SEED)
    out = (x, u, arm, sl, exps, mom, G, b)
    for a in out:
        a.setflags(write=False)
    return out
