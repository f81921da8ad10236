"""The patient-level Poisson bootstrap of include/insite_bootstrap.h restated in plain numpy: what
tests/test_bootstrap_oracle.py (CPU) and tests/test_gpu_bootstrap.py (GPU) share.

Helper only: no tests in this file.  The weights come from ``oracle.jax_prng.threefry2x32_block`` and the threshold
list below (integer work: bit for bit what the kernel draws).  The per-patient contributions are the literal
Theta^T Theta and Theta^T x_dot of the definition written on the moments; every sum takes its working dtype from its
inputs (so the float64 reference can be checked against its numpy.longdouble self) and returns the per-entry SCALE
sum_p w_p |g_p| next to the value, as tests/library_matrix.py does.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import jax_prng as J  # noqa: E402

# T_k = floor(2^32 sum_{i <= k} e^-1 / i!), k = 0..11 (tests/test_bootstrap_oracle.py recomputes it at 60 digits)
THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276,
              4294962463, 4294966817, 4294967252, 4294967292)


def weights(seed, R, N, patient_offset=0):
    """int64 [R, N]: row 0 all ones; row r >= 1, patient p with g = patient_offset + p, q = g >> 1: the word a (g
    even) or b (g odd) of Threefry-2x32-20(key (seed, r), counter (q & 0xffffffff, q >> 32)) counted against
    THRESHOLDS."""
    g = [int(patient_offset) + p for p in range(N)]
    x0 = np.array([(v >> 1) & 0xFFFFFFFF for v in g], dtype=np.uint32)
    x1 = np.array([(v >> 1) >> 32 for v in g], dtype=np.uint32)
    odd = np.array([v & 1 for v in g], dtype=bool)
    thr = np.array(THRESHOLDS, dtype=np.uint64)
    w = np.ones((R, N), dtype=np.int64)
    for r in range(1, R):
        a, b = J.threefry2x32_block(seed, r, x0, x1)
        v = np.where(odd, b, a).astype(np.uint64)
        w[r] = (v[:, None] >= thr[None, :]).sum(1)
    return w


def monomials(exps, u, dtype):
    """m_j(u_p) [N, F]: the product of the statics' powers of column j (the state exponent is not applied)."""
    exps = np.asarray(exps)
    u = np.asarray(u, dtype=dtype).reshape(len(u), -1)
    m = np.ones((u.shape[0], exps.shape[0]), dtype=dtype)
    for j, e in enumerate(exps):
        for i, k in enumerate(e[1:]):
            for _ in range(int(k)):
                m[:, j] = m[:, j] * u[:, i]
    return m


def contributes(arm, rows, min_rows, n_arms):
    arm = np.asarray(arm)
    on = (arm >= 0) & (arm < n_arms)
    if rows is not None:
        on &= np.asarray(rows) >= min_rows
    return on


def entries(mom, u, exps):
    """g_p [N, F, F] = m_i m_k mom_p[e_i + e_k] and h_p [N, F] = m_i mom_p[3 + e_i] in the dtype of ``mom``."""
    mom = np.asarray(mom)
    exps = np.asarray(exps)
    m = monomials(exps, u, mom.dtype)
    ex = exps[:, 0].astype(np.int64)
    g = m[:, :, None] * m[:, None, :] * mom[:, ex[:, None] + ex[None, :]]
    h = m * mom[:, 3 + ex]
    return g, h


def gram(mom, u, arm, rows, min_rows, exps, n_arms, R, seed, patient_offset=0):
    """(G [R, A, F, F], b [R, A, F], S_G, S_b): the weighted sums over the contributing patients of every arm and
    their scales sum_p w_rp |g_p|, sum_p w_rp |h_p|.  A patient that does not contribute is left out by indexing,
    so whatever its moments hold reaches nothing."""
    mom = np.asarray(mom)
    dt = mom.dtype
    F = np.asarray(exps).shape[0]
    N = mom.shape[0]
    w = weights(seed, R, N, patient_offset).astype(dt)
    on = contributes(arm, rows, min_rows, n_arms)
    G = np.zeros((R, n_arms, F, F), dtype=dt)
    b = np.zeros((R, n_arms, F), dtype=dt)
    SG, Sb = np.zeros_like(G), np.zeros_like(b)
    for a in range(n_arms):
        idx = np.nonzero(on & (np.asarray(arm) == a))[0]
        if not idx.size:
            continue
        g, h = entries(mom[idx], np.asarray(u)[idx] if np.asarray(exps).shape[1] > 1 else np.zeros((idx.size, 0)),
                       exps)
        wa = w[:, idx]
        G[:, a] = np.tensordot(wa, g, axes=1)
        b[:, a] = np.tensordot(wa, h, axes=1)
        SG[:, a] = np.tensordot(wa, np.abs(g), axes=1)
        Sb[:, a] = np.tensordot(wa, np.abs(h), axes=1)
    return G, b, SG, Sb


def numpy_moments(rng, N):
    """Per-patient moments of a plausible trajectory, built directly (no Gram pass): count 5..40, x in (0.5, 3),
    x_dot in (-1, 0)."""
    L = rng.integers(5, 41, N).astype(np.float64)
    mx = rng.uniform(0.5, 3.0, N)
    md = -rng.uniform(0.05, 1.0, N)
    return np.stack([L, L * mx, L * mx * mx * rng.uniform(1.0, 1.2, N), L * md, L * md * mx * rng.uniform(0.9, 1.1, N)],
                    axis=1)


@functools.lru_cache(maxsize=None)
def published_cohort(eq):
    """The reference's seed-1 training cohort of ``eq`` (oracle.ref_cohort) in DE format, its library table and the
    per-patient moments of the strong form (tests/library_matrix.gram_ref): (x, u, arm, rows, exps, mom)."""
    import library_matrix as M
    from oracle import insite_ref as R
    from oracle import ref_cohort as RC
    tr = RC.make_collection(eq, with_tests=False)["train"]
    x, u, arm, rows = R.de_format(tr.data, tr.scaling_params)
    exps = R.poly_library(3, 2, True).astype(np.int64)
    mom = M.gram_ref(x, u, arm, rows, R.STANDARD_DT, exps, 2, "smoothed4")[4]
    for a in (x, u, arm, rows, exps, mom):
        a.setflags(write=False)
    return x, u, arm, rows, exps, mom
