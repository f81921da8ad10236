"""The library matrix: the exponent tables, cohorts and references that tests/test_library_matrix.py (CPU) and
tests/test_gpu_library_matrix.py (GPU) share.  Every kernel of the affine path takes its candidate library as a
table exps[F][1 + U]; the tables here reach the shape-dependent branches the two pysindy tables of the other GPU
tests never do (F = 1 and F = 9, U = 0 and U = 3, no bias column, a duplicate column, static exponents up to 8,
contraction plans at their 16-column and 16-row limits, and tables the MFMA plan refuses).

Helper only: no tests in this file.  Every reference is a plain numpy restatement that takes its working dtype
as an argument, so the float64 reference a GPU test compares with can be checked against its numpy.longdouble
version on the CPU, and returns the per-entry SCALE of what it sums next to the value: for G the sum of
|Theta|^T |Theta|, for b the sum of |Theta|^T |x_dot|.  The entries of these tables differ by three orders of
magnitude, so the GPU tolerance is applied per entry against that scale.
"""
from __future__ import annotations

import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irregular_ref as IR  # noqa: E402
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import rk45_ref as K45  # noqa: E402
from oracle import segments_ref as S  # noqa: E402

DT = 10.0 / 60.0
N_FULL = 300            # one full 256-patient block plus 44
GRAM_RTOL = 1e-10       # the project's bar for Gram sums (tests/test_gpu_deferred.py, tests/test_gpu_weak.py)
SELF_RTOL = 1e-13       # float64 reference vs its longdouble version, per entry scale


# ---------------------------------------------------------------------------------------------------
# a. the matrix
# ---------------------------------------------------------------------------------------------------
def _table(rows):
    from insite_amd.library import PolyLibrary
    e = np.array(rows, dtype=np.int8)
    return PolyLibrary(e, ("x0",) + tuple(f"u{i}" for i in range(e.shape[1] - 1)))


def _libs():
    from insite_amd.library import polynomial_library
    deg2 = polynomial_library(2, 2, False).exps
    return {
        "x_only": _table([[1]]),
        "bias_x": _table([[0], [1]]),
        "lin3": polynomial_library(3, 1),
        "std7": polynomial_library(2, 2, True),
        "noone3": _table([[0, 1, 0], [1, 1, 0], [1, 0, 1]]),
        "dup4": _table([[0, 0], [1, 0], [1, 0], [0, 1]]),
        "u3_first9": _table(polynomial_library(3, 2, True).exps[:9]),
        # no bias column; its x0 column carries the atom "1", so 9 atoms and 10 Q columns (noone3 is the table that
        # has the "1" atom appended)
        "u3_x9": _table([[1, 0, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [1, 1, 1, 0], [1, 1, 0, 1],
                         [1, 0, 1, 1], [1, 2, 0, 0], [1, 1, 1, 1]]),
        "deg2_no_xx": _table([e for e in deg2.tolist() if e[0] < 2]),
        "u3_mixed9": _table([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1], [1, 1, 1, 0],
                             [0, 2, 0, 0], [1, 0, 0, 2], [0, 1, 1, 1]]),
        "high_pow": _table([[0, 0], [1, 0], [0, 3], [1, 8]]),
    }


LIBS = _libs()

# name -> (F, U, the MFMA plan fits before the arm count is applied); pinned by tests/test_library_matrix.py
TABLE = {
    "x_only": (1, 0, True), "bias_x": (2, 0, True), "lin3": (5, 3, True), "std7": (7, 2, True),
    "noone3": (3, 2, True), "dup4": (4, 1, True), "u3_first9": (9, 3, True), "u3_x9": (9, 3, True),
    "deg2_no_xx": (9, 2, False), "u3_mixed9": (9, 3, False), "high_pow": (4, 1, False),
}


def exps_of(name):
    return LIBS[name].exps.astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# b. the planner's verdict, restated
# ---------------------------------------------------------------------------------------------------
def q_columns(exps):
    """The distinct (atom, moment) columns the MFMA contraction of the strong-form Gram needs, or None when a
    static exponent is above 2.  An atom is a distinct tuple of static exponents among the columns (the all-zero
    tuple, "1", is added when no column carries it: the right-hand side b needs it).  Entry (i, k), i <= k, of G
    is atom(k) times the moment sum x^(e_i + e_k) (x^0: the row count); entry i of b is the atom "1" times the
    moment sum x_dot x^(e_i)."""
    exps = np.asarray(exps)
    if exps.shape[1] > 1 and exps[:, 1:].max() > 2:
        return None
    F = exps.shape[0]
    atom = [tuple(int(v) for v in e[1:]) for e in exps]
    one = tuple(0 for _ in range(exps.shape[1] - 1))
    cols = set()
    for i in range(F):
        for k in range(i, F):
            cols.add((atom[k], "x", int(exps[i, 0] + exps[k, 0])))
        cols.add((one, "xdot", int(exps[i, 0])))
    return cols


def narm_pad(n_arms):
    """Arm counts are padded to 1, 2 or 4 (three arms count as four)."""
    return 1 if n_arms <= 1 else (2 if n_arms <= 2 else 4)


def mfma_fits(exps, n_arms):
    """True when the strong-form Gram takes the MFMA contraction: every static exponent <= 2, at most 16
    distinct Q columns, and narm_pad(n_arms) * F <= 16 rows."""
    q = q_columns(exps)
    return q is not None and len(q) <= 16 and narm_pad(n_arms) * np.asarray(exps).shape[0] <= 16


# ---------------------------------------------------------------------------------------------------
# d. cohorts
# ---------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _decay(rng, t, N):
    """x = y0 exp(-r t) + 0.01 noise, y0 ~ U(0.5, 3), r ~ U(0.2, 1): |b| / S_b stays near 1."""
    y0 = rng.uniform(0.5, 3.0, (N, 1))
    r = rng.uniform(0.2, 1.0, (N, 1))
    return y0 * np.exp(-r * t) + 0.01 * rng.normal(size=(N, t.shape[-1]))


EDGE_ROWS = (0, 4, 5, 6, 7, 8, 16, 17)


def cohort(N, T, U, seed, n_arms=2, empty_arm=None):
    """(x [N, T], u [N, U], arm [N], rows [N]) on the uniform grid t_i = i DT: u ~ U(0.6, 1.6) (u^8 within 0.02 and
    43), arm uniform in [0, n_arms) (``empty_arm`` moves its patients to arm 0), ragged rows that include
    0, 4, 5, 6, 7, 8, 16, 17 and T when N allows; samples past rows[p] are NaN."""
    rng = np.random.default_rng(seed)
    x = _decay(rng, np.arange(T) * DT, N)
    u = rng.uniform(0.6, 1.6, (N, U))
    arm = rng.integers(0, n_arms, N)
    if empty_arm is not None:
        arm = np.where(arm == empty_arm, 0, arm)
    rows = rng.integers(0, T + 1, N)
    edge = np.array(EDGE_ROWS + (T,))
    if N >= edge.size:
        rows[:edge.size] = edge
    else:
        rows[:] = T
    x[np.arange(T)[None, :] >= rows[:, None]] = np.nan
    return x, u, arm.astype(np.int64), rows.astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# c. references: (values, scales) in any dtype
# ---------------------------------------------------------------------------------------------------
def _stencil5(x, W):
    """oracle.insite_ref._stencil5 in the dtype of x (the tables keep their float64 values)."""
    W = W.astype(x.dtype)
    L = x.shape[0]
    y = np.empty_like(x)
    y[0] = W[0] @ x[0:5]
    y[1] = W[1] @ x[0:5]
    c = W[2]
    y[2:L - 2] = c[0] * x[0:L - 4] + c[1] * x[1:L - 3] + c[2] * x[2:L - 2] + c[3] * x[3:L - 1] + c[4] * x[4:L]
    y[L - 2] = W[3] @ x[L - 5:L]
    y[L - 1] = W[4] @ x[L - 5:L]
    return y


def _xdot_uniform(x, dt, fd):
    if fd == "smoothed4":
        return _stencil5(_stencil5(x, R.SAVGOL_5_3), R.FD4) / x.dtype.type(dt)
    if fd == "order4":
        return _stencil5(x, R.FD4) / x.dtype.type(dt)
    raise ValueError(fd)


def _xdot_segment(x, dt, fd):
    """oracle.segments_ref.derivative in the dtype of x: forward differences (backward at the last sample) of the
    raw samples ("order1") or of the savgol(2, 1) smoothed ones ("smoothed1")."""
    if fd == "smoothed1":
        y = np.empty_like(x)
        y[:-1] = x.dtype.type(0.5) * (x[:-1] + x[1:])
        y[0] = x[0]
        y[-1] = x[-1]
        x = y
    elif fd != "order1":
        raise ValueError(fd)
    d = np.empty_like(x)
    d[:-1] = (x[1:] - x[:-1]) / x.dtype.type(dt)
    d[-1] = (x[-1] - x[-2]) / x.dtype.type(dt)
    return d


class _Sums:
    """G, b and their scales S_G = sum |Theta|^T |Theta|, S_b = sum |Theta|^T |x_dot| per arm."""

    def __init__(self, exps, n_arms, dtype):
        self.exps = np.asarray(exps)
        F = self.exps.shape[0]
        self.G = np.zeros((n_arms, F, F), dtype=dtype)
        self.b = np.zeros((n_arms, F), dtype=dtype)
        self.SG = np.zeros((n_arms, F, F), dtype=dtype)
        self.Sb = np.zeros((n_arms, F), dtype=dtype)
        self.dtype = dtype

    def add(self, a, xs, up, xd):
        """The rows of one trajectory: samples xs [L], statics up [U], targets xd [L]."""
        L = xs.shape[0]
        Z = np.concatenate([xs[:, None], np.repeat(np.asarray(up, dtype=self.dtype)[None, :], L, 0)], axis=1)
        th = IR.eval_library(self.exps, Z)
        ath, axd = np.abs(th), np.abs(xd)
        self.G[a] += th.T @ th
        self.b[a] += th.T @ xd
        self.SG[a] += ath.T @ ath
        self.Sb[a] += ath.T @ axd

    def out(self):
        return self.G, self.b, self.SG, self.Sb


def gram_ref(x, u, arm, rows, dt, exps, n_arms, fd, dtype=np.float64):
    """oracle.insite_ref.gram_moments restated in ``dtype``: (G, b, S_G, S_b, mom).  A patient with fewer than 5
    rows contributes nothing (mom = 0); one whose arm is outside [0, n_arms) reaches no G | b.  mom [N, 5] =
    {L, sum x, sum x^2, sum x_dot, sum x_dot x} per patient."""
    s = _Sums(exps, n_arms, dtype)
    N = x.shape[0]
    mom = np.zeros((N, 5), dtype=dtype)
    for p in range(N):
        L = min(int(rows[p]), x.shape[1])
        if L < 5:
            continue
        xp = np.asarray(x[p, :L], dtype=dtype)
        xd = _xdot_uniform(xp, dt, fd)
        mom[p] = [L, xp.sum(), (xp * xp).sum(), xd.sum(), (xd * xp).sum()]
        if 0 <= int(arm[p]) < n_arms:
            s.add(int(arm[p]), xp, u[p], xd)
    return s.out() + (mom,)


def irregular_ref(x, t_obs, n_obs, u, arm, exps, n_arms, fd, dtype=np.float64):
    """tests/irregular_ref.gram_irregular restated with the scales: (G, b, S_G, S_b, mom)."""
    W = IR.WINDOW[fd]
    s = _Sums(exps, n_arms, dtype)
    N = x.shape[0]
    mom = np.zeros((N, 5), dtype=dtype)
    for p in range(N):
        L = min(int(n_obs[p]), x.shape[1])
        if L < W:
            continue
        xp = np.asarray(x[p, :L], dtype=dtype)
        xd = IR.lagrange_derivative(xp, np.asarray(t_obs[p, :L], dtype=dtype), W)
        mom[p] = [L, xp.sum(), (xp * xp).sum(), xd.sum(), (xd * xp).sum()]
        if 0 <= int(arm[p]) < n_arms:
            s.add(int(arm[p]), xp, u[p], xd)
    return s.out() + (mom,)


def segments_ref(x, u, arm_steps, seq_len, dt, exps, n_arms, fd, dtype=np.float64):
    """oracle.segments_ref.gram_segments restated with the scales: (G, b, S_G, S_b).  Every treatment-constant
    segment (oracle.segments_ref.segment_bounds: consecutive segments share their boundary sample) is one
    trajectory of its arm."""
    s = _Sums(exps, n_arms, dtype)
    for p in range(x.shape[0]):
        for a, lo, hi in S.segment_bounds(arm_steps[p], seq_len[p]):
            xs = np.asarray(x[p, lo:hi + 1], dtype=dtype)
            s.add(a, xs, u[p], _xdot_segment(xs, dt, fd))
    return s.out()


def weak_ref(x, u, arm, rows, W, D, exps, n_arms, dtype=np.float64):
    """tests/weak_ref.gram and .moments in ``dtype`` with their scales: (G, b, S_G, S_b, mom, S_mom).  The scale is
    the restatement run on |x|, |u|, |W|, |D| (entrywise absolute values of its outputs): the projections cancel
    inside W x, so |Theta| of the finished rows would understate what the sums round against."""
    c = lambda a: np.asarray(a, dtype=dtype)   # noqa: E731
    xs, us, Ws, Ds = c(x), c(u), c(W), c(D)
    G, b = WR.gram(xs, us, arm, rows, Ws, Ds, exps, n_arms)
    mom = WR.moments(xs, arm, rows, Ws, Ds, n_arms)
    SG, Sb = WR.gram(np.abs(xs), np.abs(us), arm, rows, np.abs(Ws), np.abs(Ds), exps, n_arms)
    Sm = WR.moments(np.abs(xs), arm, rows, np.abs(Ws), np.abs(Ds), n_arms)
    return G, b, np.abs(SG), np.abs(Sb), mom, np.abs(Sm)


def worst_ratio(got, ref, scale):
    """max over the entries of |got - ref| / scale (an entry of scale 0 must be exact: else inf)."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    scale = np.asarray(scale, dtype=np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------
# the cases of the GPU file (shared with the CPU self-check); every cached array is read-only
# ---------------------------------------------------------------------------------------------------
def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# a. strong form: (library, n_arms, T)
STRONG_ARMS = {
    1: tuple(TABLE),
    2: ("lin3", "std7", "deg2_no_xx", "u3_first9", "high_pow"),
    3: ("lin3", "noone3", "std7"),
    4: ("bias_x", "dup4", "noone3", "std7"),
}
STRONG_T = 23            # one 16-step tile plus 7
STRONG_T_LONG = 40       # two 16-step tiles plus a remainder
STRONG_LONG = ("u3_first9", "deg2_no_xx", "high_pow")
STRONG_CASES = [(name, A, STRONG_T) for A, names in STRONG_ARMS.items() for name in names] + \
               [(name, A, STRONG_T_LONG) for A, names in STRONG_ARMS.items() for name in names if name in STRONG_LONG]
STRONG_FDS = ("smoothed4", "order4")
STRONG_LOADS = ("pm16", "pm8", "tm")   # patient-major even ld | patient-major odd ld | time-major ld = N + 5


@functools.lru_cache(maxsize=None)
def strong_inputs(name, n_arms, T, N=N_FULL):
    """With three arms arm 1 has no patients (its G | b must be exactly zero)."""
    U = TABLE[name][1]
    out = cohort(N, T, U, _seed("strong", name, n_arms, T, N), n_arms, empty_arm=1 if n_arms == 3 else None)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def strong_ref(name, n_arms, T, fd, dtype=np.float64):
    out = gram_ref(*strong_inputs(name, n_arms, T), DT, exps_of(name), n_arms, fd, dtype)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def short_wave_inputs():
    """std7, two arms, N = 65: the second 64-patient wave holds one patient, and that one has 3 rows."""
    x, u, arm, rows = cohort(65, STRONG_T, 2, _seed("short-wave"), 2)
    rows[64] = 3
    x[64, 3:] = np.nan
    _freeze(x, u, arm, rows)
    return x, u, arm, rows


# c. weak, irregular and segment Grams
SCALAR_LIBS = ("x_only", "lin3", "noone3", "u3_x9", "deg2_no_xx", "u3_mixed9", "high_pow")
WEAK_ARMS = (1, 4)
WEAK_SHAPE = (N_FULL, 23, 33)
IRR_ARMS = (1, 3)
IRR_FDS = ("nonuniform2", "nonuniform4")
# tests/irregular_ref.edge_lengths(23) holds 32 and 33 samples, more than a 23-column grid stores: the lengths are
# built for T_max >= 2 * 16 + 1, so the irregular cases run at T_max = 60 with N = 130 (two waves and two patients)
IRR_SHAPE = (130, 60)
SEG_ARMS = (2, 4)
SEG_FDS = ("order1", "smoothed1")
SEG_SHAPE = (N_FULL, 23)


def weak_weights(T, dt=DT):
    """W, D [33, T]: rows 0..15 compact test functions sorted by centre, rows 16..31 all zero (the kernel skips the
    16-row tile: lo >= hi), row 32 dense (every weight non-zero, off the grid so D has no zero either)."""
    rng = np.random.default_rng(_seed("weak-weights", T))
    L = (T - 1) * dt
    H = max(L / 20.0, 1.5 * dt)
    W = np.zeros((33, T))
    D = np.zeros((33, T))
    W[:16], D[:16] = WR.weights(T, dt, np.sort(rng.uniform(H, L - H, 16)), H=H)
    W[32:], D[32:] = WR.weights(T, dt, [0.5 * L + 0.3 * dt], H=L)
    return W, D


@functools.lru_cache(maxsize=None)
def weak_inputs(name, n_arms):
    """Full-length patients but: every 7th has rows = T - 1 and every 11th / 13th an arm of -1 / n_arms (they
    contribute nothing and their samples are NaN), every 17th rows = T + 3."""
    N, T, _ = WEAK_SHAPE
    U = TABLE[name][1]
    rng = np.random.default_rng(_seed("weak", name, n_arms))
    x = _decay(rng, np.arange(T) * DT, N)
    u = rng.uniform(0.6, 1.6, (N, U))
    k = np.arange(N)
    arm = np.where(k % 11 == 3, -1, np.where(k % 13 == 5, n_arms, rng.integers(0, n_arms, N)))
    rows = np.where(k % 7 == 2, T - 1, np.where(k % 17 == 4, T + 3, T))
    W, D = weak_weights(T)
    assert np.all(W[32] != 0) and np.all(D[32] != 0) and not W[16:32].any()
    x[~WR.contributes(rows, arm, T, n_arms)] = np.nan
    out = (x, u, arm, rows, W, D)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def weak_case_ref(name, n_arms, dtype=np.float64):
    out = weak_ref(*weak_inputs(name, n_arms), exps_of(name), n_arms, dtype)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def irregular_inputs(name, n_arms):
    """(x, t_obs, n_obs, u, arm): edge-length grids, the decay recipe on every patient's own times; every 11th /
    13th patient has an arm of -1 / n_arms; samples and times past n_obs[p] are NaN."""
    N, T_max = IRR_SHAPE
    U = TABLE[name][1]
    rng = np.random.default_rng(_seed("irregular", name, n_arms))
    t, n_obs = IR.edge_grid(N, rng, T_max)
    x = _decay(rng, t, N)
    u = rng.uniform(0.6, 1.6, (N, U))
    k = np.arange(N)
    arm = np.where(k % 11 == 3, -1, np.where(k % 13 == 5, n_arms, rng.integers(0, n_arms, N)))
    past = np.arange(T_max)[None, :] >= n_obs[:, None]
    x[past] = np.nan
    t[past] = np.nan
    out = (x, t, n_obs, u, arm)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def irregular_case_ref(name, n_arms, fd, dtype=np.float64):
    out = irregular_ref(*irregular_inputs(name, n_arms), exps_of(name), n_arms, fd, dtype)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def segment_inputs(name, n_arms):
    """(x [N, T], u, arm_steps [N, T - 1], seq_len): per-step arms that switch to another arm with probability
    0.3, seq_len in [0, T - 1] with 0, 1, 2 and T - 1 present; what the reference never reads is poisoned (samples
    past seq_len are NaN, the arms from seq_len on are changed)."""
    N, T = SEG_SHAPE
    U = TABLE[name][1]
    rng = np.random.default_rng(_seed("segments", name, n_arms))
    x = _decay(rng, np.arange(T) * DT, N)
    u = rng.uniform(0.6, 1.6, (N, U))
    arm = np.empty((N, T - 1), dtype=np.int64)
    arm[:, 0] = rng.integers(0, n_arms, N)
    for k in range(1, T - 1):
        other = (arm[:, k - 1] + rng.integers(1, n_arms, N)) % n_arms
        arm[:, k] = np.where(rng.random(N) < 0.3, other, arm[:, k - 1])
    sl = rng.integers(0, T, N)
    sl[:6] = [0, 1, 2, 3, T - 1, T - 2]
    arm[4, -1] = (arm[4, -2] + 1) % n_arms     # a switch at the last step
    for p in range(N):
        x[p, sl[p] + 1:] = np.nan
        arm[p, sl[p]:] = (arm[p, sl[p]:] + 1) % n_arms
    out = (x, u, arm, sl)
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def segment_case_ref(name, n_arms, fd, dtype=np.float64):
    out = segments_ref(*segment_inputs(name, n_arms), DT, exps_of(name), n_arms, fd, dtype)
    _freeze(*out)
    return out


# d. solvers
SOLVER_F = tuple(range(1, 11))      # STLSQ: 1..10 (10: the first size of the one-wave-per-system route)
SR3_F = tuple(range(1, 10))
SR3_THRESHOLD, SR3_TOL = 0.1, 0.03
STLSQ_THRESHOLD, STLSQ_ALPHA = 0.2, 0.5


@functools.lru_cache(maxsize=None)
def solver_systems(F):
    """32 well-conditioned F x F Gram systems with a sparse truth (the recipe of tests/test_gpu_weak._sr3_systems),
    seed 4200 + F: (G [32, F, F], b [32, F])."""
    rng = np.random.default_rng(4200 + F)
    Gs, bs = [], []
    for _ in range(32):
        A = rng.normal(size=(60, F)) * rng.uniform(0.5, 2.0, F)
        c = np.where(rng.random(F) < 0.4, rng.uniform(0.5, 2.0, F) * rng.choice([-1.0, 1.0], F), 0.0)
        y = A @ c + 0.05 * rng.normal(size=60)
        Gs.append(A.T @ A)
        bs.append(A.T @ y)
    out = (np.stack(Gs), np.stack(bs))
    _freeze(*out)
    return out


# e. rollouts
ROLLOUT_LIBS = ("x_only", "lin3", "u3_x9", "deg2_no_xx", "high_pow")
ROLLOUT_SHAPE = (65, 33)
ROLLOUT_DT = 0.1
DROP_BELOW = 1e-3


def rollout_coef(name, n_arms, rng):
    """[A, F] coefficients of size 0.1 (|c| in [0.05, 0.15], random signs: every arm keeps a term of either state
    exponent where the table has one) and one coefficient below ``drop_below``: the last column of the last arm
    (with F = 1 that arm's right-hand side is then zero and it holds the state)."""
    F = TABLE[name][0]
    coef = rng.uniform(0.05, 0.15, (n_arms, F)) * rng.choice([-1.0, 1.0], (n_arms, F))
    coef[n_arms - 1, F - 1] = 0.5 * DROP_BELOW
    return coef


@functools.lru_cache(maxsize=None)
def rollout_inputs(name, n_arms):
    """(y0 [N], u [N, U], arm [N, T + 2] per-step arms, coef [A, F])."""
    N, T = ROLLOUT_SHAPE
    rng = np.random.default_rng(_seed("rollout", name, n_arms))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, TABLE[name][1]))
    arm = rng.integers(0, n_arms, (N, T + 2)).astype(np.int8)
    out = (y0, u, arm, rollout_coef(name, n_arms, rng))
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def rollout_case_ref(name, n_arms, method):
    y0, u, arm, coef = rollout_inputs(name, n_arms)
    y = R.rollout(y0, u, arm[:, :ROLLOUT_SHAPE[1]], coef, exps_of(name), ROLLOUT_DT, method=method)
    _freeze(y)
    return y


RK45_N, RK45_T_END, RK45_N_MIN, RK45_N_MAX = 65, 2.0, 5, 24


@functools.lru_cache(maxsize=None)
def rk45_inputs(name):
    """(t [N, T_max] NaN past the grid, n_obs, u, arm [N, T_max] in {0, 1}, y0, coef [2, F]): grids from
    oracle.rk45_ref.irregular_grid over [0, 2] with 5..24 samples (rates of 0.1 u^8 stay within e^9 there)."""
    rng = np.random.default_rng(_seed("rk45", name))
    t, n_obs = K45.irregular_grid(RK45_N, rng, t_max=RK45_T_END, n_min=RK45_N_MIN, n_max=RK45_N_MAX)
    u = rng.uniform(0.6, 1.6, (RK45_N, TABLE[name][1]))
    arm = (rng.random((RK45_N, RK45_N_MAX)) < 0.5).astype(np.int8)
    y0 = rng.uniform(0.5, 3.0, RK45_N)
    out = (t, n_obs, u, arm, y0, rollout_coef(name, 2, rng))
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def rk45_case_ref(name):
    t, n_obs, u, arm, y0, coef = rk45_inputs(name)
    y, steps = K45.rollout_rk45(y0, u, arm, t, n_obs, coef, exps_of(name))
    _freeze(y, steps)
    return y, steps
