"""The step matrix: the cases and references that tests/test_step_matrix.py (CPU) and tests/test_gpu_step_matrix.py
(GPU) share for the step family -- insite_fit_rollout_f64 (step_kernel), insite_fit_rollout_deferred_f64 and
insite_fit_rollout_lagged_f64 (step_deferred_kernel) -- on small edge shapes: both derivative kinds, the three
rollout methods, two 7-term libraries, the static and the claimed gram tail, the short-trajectory lengths, ragged and
degenerate row counts, every bit layout of the rollout role and ranges that start mid-tile.

Helper only: no tests in this file, and nothing here touches a torch device.  The cohorts, the Gram reference with
its per-entry scales, worst_ratio and the bars are those of tests/library_matrix.py; the rollout reference is
oracle.insite_ref.rollout restated in a working dtype, so its float64 result can be checked against longdouble.

The constants of section b restate the host planner (csrc/insite_hip.hip, run_fit_rollout, and the INSITE_DEF_DYN*
knobs above step_deferred_kernel); tests/test_step_matrix.py pins what they give for every case, and the GPU file
reads the slot header the launch wrote to confirm the instantiation a case took.
"""
from __future__ import annotations

import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
from oracle import insite_ref as R  # noqa: E402

DT = M.DT
GRAM_RTOL = M.GRAM_RTOL
SELF_RTOL = M.SELF_RTOL
DROP_BELOW = M.DROP_BELOW
ROLLOUT_DT = M.ROLLOUT_DT
COEF_ATOL = 1e-8                 # coefficient L-inf against the reference fit (tests/test_gpu_fused.py)
Y_RTOL, Y_ATOL = 1e-11, 1e-12    # rollout against the reference (tests/test_gpu_parity.py)
THRESHOLD, ALPHA = 0.1, 0.5      # the project's STLSQ settings
THRESHOLD_LOW = 0.02             # a second threshold, at which most fits keep three or more terms
PERTURB = 1e-10                  # the well-posedness check moves G | b by +-PERTURB x scale (= GRAM_RTOL)
WELL_POSED_COEF = 1e-9           # ... and the fits must stay within this of one another

# ---------------------------------------------------------------------------------------------------
# a. libraries: the step kernels take F = 7, state degree <= 1, an MFMA plan for two arms
# ---------------------------------------------------------------------------------------------------
LIBS = {
    "std7": M.LIBS["std7"],
    # three statics, no bias column: 14 Q columns
    "u3_nobias7": M._table([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [0, 0, 2, 0],
                            [1, 0, 1, 1]]),
}
Q_COLUMNS = {"std7": 13, "u3_nobias7": 14}


def exps_of(lib):
    return LIBS[lib].exps.astype(np.int64)


# ---------------------------------------------------------------------------------------------------
# b. the host planner, restated (run_fit_rollout in csrc/insite_hip.hip)
# ---------------------------------------------------------------------------------------------------
WAVE = 64                 # patients per tile (kWave)
GT = 16                   # steps per gram group (kGT)
ROLL_GS = 32              # steps per arm group of the rollout (kRollGS)
WAVES_PER_BLOCK = 4       # kWavesPerBlock
DYN_MIN = 128             # INSITE_DEF_DYN_MIN: units per gram wave from which a launch takes the claimed tail
DYN_TAIL = 250            # INSITE_DEF_DYN_TAIL: per mille of the tiles that are claimed
DYN_PG = 2                # INSITE_DEF_DYN_PG: gram groups per claimed piece
GRAM_MAX_BLOCKS = 1024    # kGramMaxBlocks
GB_OVER = 1_000_000       # a gram_blocks above any grid: clamped to grid - 2 (deferred, lagged) or grid - 1 (fused),
#                           which leaves the rollout role one block of four waves
# the deferred workspace: [claim areas, 4096 B][slot 0][slot 1]; a slot starts with a 512-B header of 32-bit words
DEF_AREA_BYTES = 4096
SLOT_REC = 112            # kSlotRec: {magic, gram blocks, entries, fingerprint}
DYN_REC_DONE, DYN_REC_P = 116, 117   # kDynRecDone, kDynRecP: pieces processed / pieces streamed (0: static launch)


def ceil_div(a, b):
    return -(-a // b)


def gram_units(N, T):
    return ceil_div(N, WAVE) * ceil_div(T, GT)


def claimed_tail(N, T, gblocks):
    """True when a deferred / lagged launch with ``gblocks`` gram blocks (after the planner's clamps) takes the
    claimed instantiation (DYN = 1)."""
    return N > 0 and gram_units(N, T) >= DYN_MIN * WAVES_PER_BLOCK * gblocks


def tail_geometry(N, T):
    """(tile0, pieces per tile, P, groups in a tile's last piece) of a claimed launch with the default knobs.  (The
    planner coarsens the pieces when P exceeds the slot's row budget, ~3900 rows; the cases here stay below 200.)"""
    n_tiles, ngs = ceil_div(N, WAVE), ceil_div(T, GT)
    tail = n_tiles * DYN_TAIL // 1000
    pg = max(1, min(DYN_PG, ngs))
    ppt = ceil_div(ngs, pg)
    return n_tiles - tail, ppt, tail * ppt, ngs - (ppt - 1) * pg


def args_ok(N, T, ldx, lib, Nr, Tr, ld_arm, ld_y, gram_blocks):
    """The argument checks of run_fit_rollout that depend on the shapes."""
    e = exps_of(lib)
    if e.shape[0] != 7 or e[:, 0].max() > 1 or not M.mfma_fits(e, 2):
        return False
    if N < 0 or T < 0 or ldx < max(N, 1) or ldx > (1 << 31) // (8 * GT) or gram_blocks < 0:
        return False
    if Nr < 0 or Tr < 0 or ld_y < Nr:
        return False
    return ld_arm >= ceil_div(Nr, 32) if ld_arm >= 0 else -ld_arm >= Tr


# ---------------------------------------------------------------------------------------------------
# c. discovery cases
# ---------------------------------------------------------------------------------------------------
Disc = collections.namedtuple("Disc", "name lib N T pattern gram_blocks fd path")
# pattern: ragged (library_matrix.cohort: 0, 4, 5, 6, 7, 8, 16, 17 and T planted, rows above T clamp) | full |
# clamp (every third patient has rows above T) | short_mid / short_last / short_tail (a whole 64-patient tile with
# every row < 5: tile 2, the last tile, tile 14 = a claimed tail tile of the 1025-patient cohort) | all_short
# path: "static" | "claimed" (deferred and lagged; the fused kernel has the static tail only)
_S, _O = "smoothed4", "order4"
DISC_CASES = [
    # T: the short-trajectory lengths (5..7 smoothed), kMinMain = 8 / 5, one and several 16-step groups + remainder
    Disc("t5_s", "std7", 300, 5, "ragged", 0, _S, "static"),
    Disc("t5_o", "std7", 300, 5, "ragged", 7, _O, "static"),
    Disc("t7_s", "std7", 300, 7, "ragged", 7, _S, "static"),
    Disc("t7_o", "std7", 300, 7, "ragged", 1, _O, "static"),
    Disc("t8_s", "std7", 300, 8, "ragged", 0, _S, "static"),
    Disc("t8_o", "std7", 300, 8, "ragged", GB_OVER, _O, "static"),
    Disc("t9_s", "std7", 300, 9, "ragged", GB_OVER, _S, "static"),
    Disc("t9_o", "std7", 300, 9, "ragged", 0, _O, "static"),
    Disc("t15_s", "std7", 300, 15, "ragged", 1, _S, "static"),
    Disc("t16_o", "std7", 300, 16, "ragged", 7, _O, "static"),
    Disc("t17_s", "std7", 300, 17, "ragged", 7, _S, "static"),
    Disc("t23_o", "std7", 300, 23, "ragged", 0, _O, "static"),
    Disc("t40_s", "std7", 300, 40, "ragged", GB_OVER, _S, "static"),
    Disc("t40_o", "std7", 300, 40, "ragged", 1, _O, "static"),
    # N: one patient, one tile less one, one tile, one tile and one
    Disc("n1_s", "std7", 1, 23, "full", 0, _S, "static"),
    Disc("n1_o", "std7", 1, 8, "full", GB_OVER, _O, "static"),
    Disc("n63_s", "std7", 63, 17, "ragged", 1, _S, "static"),
    Disc("n64_o", "std7", 64, 16, "ragged", 0, _O, "static"),
    Disc("n65_s", "std7", 65, 40, "ragged", 7, _S, "static"),
    Disc("n65_o", "std7", 65, 9, "ragged", GB_OVER, _O, "static"),
    # rows
    Disc("full_s", "std7", 300, 16, "full", 7, _S, "static"),
    Disc("full_o", "std7", 64, 9, "full", 1, _O, "static"),
    Disc("clamp_s", "std7", 65, 23, "clamp", 0, _S, "static"),
    Disc("clamp_o", "std7", 300, 7, "clamp", GB_OVER, _O, "static"),
    Disc("shortmid_s", "std7", 300, 23, "short_mid", 0, _S, "static"),
    Disc("shortmid_o", "std7", 300, 17, "short_mid", 7, _O, "static"),
    Disc("shortlast_s", "std7", 300, 40, "short_last", 1, _S, "static"),
    Disc("shortlast_o", "std7", 65, 15, "short_last", 0, _O, "static"),
    Disc("allshort_s", "std7", 300, 23, "all_short", 0, _S, "static"),
    Disc("allshort_o", "std7", 65, 8, "all_short", 7, _O, "static"),
    # the claimed tail: 17 x 31 = 527 units >= 512 x 1; 34 x 31 = 1054 >= 512 x 2; 527 < 1024 is static
    Disc("c1025_g1_s", "std7", 1025, 490, "ragged", 1, _S, "claimed"),
    Disc("c1025_g2_s", "std7", 1025, 490, "ragged", 2, _S, "static"),
    Disc("c1025_g1_o", "std7", 1025, 490, "ragged", 1, _O, "claimed"),
    Disc("c1025_g1_shorttail", "std7", 1025, 490, "short_tail", 1, _S, "claimed"),
    Disc("c2113_g2_s", "std7", 2113, 490, "ragged", 2, _S, "claimed"),
    # the second library
    Disc("u3_t23_s", "u3_nobias7", 300, 23, "ragged", 0, _S, "static"),
    Disc("u3_t7_o", "u3_nobias7", 65, 7, "ragged", 7, _O, "static"),
    Disc("u3_t6_s", "u3_nobias7", 300, 6, "full", 1, _S, "static"),
    Disc("u3_t40_o", "u3_nobias7", 300, 40, "short_last", GB_OVER, _O, "static"),
    Disc("u3_c1025_g1_o", "u3_nobias7", 1025, 490, "ragged", 1, _O, "claimed"),
]
DISC = {c.name: c for c in DISC_CASES}
assert len(DISC) == len(DISC_CASES)


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _cohort_key(c):
    """Cases that differ in gram_blocks / fd only share their cohort."""
    return c.lib, c.N, c.T, c.pattern


@functools.lru_cache(maxsize=None)
def _cohort(lib, N, T, pattern):
    U = LIBS[lib].n_statics
    x, u, arm, rows = M.cohort(N, T, U, M._seed("step", lib, N, T, pattern), 2)
    if pattern == "ragged":
        out = (x, u, arm, rows)
        _freeze(*out)
        return out
    rng = np.random.default_rng(M._seed("step-x", lib, N, T, pattern))
    x = M._decay(rng, np.arange(T) * DT, N)
    k = np.arange(N)
    short = k % 5
    if pattern == "full":
        rows = np.full(N, T)
    elif pattern == "clamp":
        rows = np.where(k % 3 == 0, T + 1 + 100 * (k % 4), rows)
    elif pattern == "short_mid":
        rows = np.where((k >= 2 * WAVE) & (k < 3 * WAVE), short, rows)
    elif pattern == "short_last":
        rows = np.where(k >= (ceil_div(N, WAVE) - 1) * WAVE, short, rows)
    elif pattern == "short_tail":
        rows = np.where((k >= 14 * WAVE) & (k < 15 * WAVE), short, rows)
    elif pattern == "all_short":
        rows = short
    else:
        raise ValueError(pattern)
    rows = rows.astype(np.int64)
    x[np.arange(T)[None, :] >= rows[:, None]] = np.nan
    out = (x, u, arm, rows)
    _freeze(*out)
    return out


def disc_inputs(name):
    """(x [N, T] NaN past rows, u [N, U], arm [N] in {0, 1}, rows [N])."""
    return _cohort(*_cohort_key(DISC[name]))


@functools.lru_cache(maxsize=None)
def _disc_ref(lib, N, T, pattern, fd, dtype):
    out = M.gram_ref(*_cohort(lib, N, T, pattern), DT, exps_of(lib), 2, fd, dtype)[:4]
    _freeze(*out)
    return out


def disc_ref(name, dtype=np.float64):
    """(G [2, 7, 7], b [2, 7], S_G, S_b) of library_matrix.gram_ref."""
    c = DISC[name]
    return _disc_ref(c.lib, c.N, c.T, c.pattern, c.fd, dtype)


def next_in_stream(name):
    """The cohort a deferred / lagged stream sends after ``name``: the next case of the same library (cyclic)."""
    same = [c.name for c in DISC_CASES if c.lib == DISC[name].lib]
    return same[(same.index(name) + 1) % len(same)]


# ---------------------------------------------------------------------------------------------------
# d. fits: the reference, and which cases have a fit that G | b within the bar cannot move
# ---------------------------------------------------------------------------------------------------
def fit_ref(G, b, threshold):
    """(coef [2, 7], support [2, 7], iters [2]) of oracle.insite_ref.stlsq_gram per arm."""
    out = [R.stlsq_gram(np.asarray(G[a], dtype=np.float64), np.asarray(b[a], dtype=np.float64), threshold, ALPHA)
           for a in range(2)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def supports_by_iteration(G, b, threshold):
    """The support after 1, 2, ... iterations of stlsq_gram (its max_iter cut short), per arm."""
    out = []
    for a in range(2):
        Ga, ba = np.asarray(G[a], dtype=np.float64), np.asarray(b[a], dtype=np.float64)
        it = R.stlsq_gram(Ga, ba, threshold, ALPHA)[2]
        out.append([tuple(R.stlsq_gram(Ga, ba, threshold, ALPHA, max_iter=k, unbias=False)[1].tolist())
                    for k in range(1, it + 1)])
    return out


def sign_patterns(F=7):
    """A few fixed entrywise sign patterns (sG [F, F] symmetric, sb [F])."""
    i, j = np.indices((F, F))
    rng = np.random.default_rng(7)
    r = rng.choice([-1.0, 1.0], (F, F))
    r = np.triu(r) + np.triu(r, 1).T
    return [(np.ones((F, F)), np.ones(F)), (-np.ones((F, F)), np.ones(F)), (np.ones((F, F)), -np.ones(F)),
            (np.where((i + j) % 2 == 0, 1.0, -1.0), np.where(np.arange(F) % 2 == 0, -1.0, 1.0)),
            (r, rng.choice([-1.0, 1.0], F))]


FitChecks = collections.namedtuple("FitChecks", "reference_agrees support_stable coef_move")


@functools.lru_cache(maxsize=None)
def fit_checks(name, threshold):
    """What the reference itself decides about the fit of a case:

    reference_agrees  the float64 G | b and the longdouble-derived G | b give the same support at every iteration, the
                      same iteration count, and coefficients within 1e-9 of one another;
    support_stable    so do (supports and iteration counts) G | b moved entrywise by +-1e-10 x scale, for every sign
                      pattern of sign_patterns(): a kernel whose G | b are inside the bar must find this support;
    coef_move         the largest coefficient change among those moved systems (inf when one cannot be solved)."""
    G, b, SG, Sb = disc_ref(name)
    Gl, bl = disc_ref(name, np.longdouble)[:2]
    try:
        c0, s0, i0 = fit_ref(G, b, threshold)
        t0 = supports_by_iteration(G, b, threshold)
    except np.linalg.LinAlgError:
        return FitChecks(False, False, np.inf)

    def same(Gv, bv):
        try:
            c, s, i = fit_ref(Gv, bv, threshold)
            ok = np.array_equal(s, s0) and np.array_equal(i, i0) and supports_by_iteration(Gv, bv, threshold) == t0
        except np.linalg.LinAlgError:
            return False, np.inf
        d = float(np.max(np.abs(c - c0))) if np.all(np.isfinite(c)) and np.all(np.isfinite(c0)) else np.inf
        return ok, d

    ok_ld, d_ld = same(np.asarray(Gl, dtype=np.float64), np.asarray(bl, dtype=np.float64))
    moved = [same(G + PERTURB * sG * SG, b + PERTURB * sb * Sb) for sG, sb in sign_patterns()]
    return FitChecks(ok_ld and d_ld <= WELL_POSED_COEF, all(ok for ok, _ in moved), max(d for _, d in moved))


def well_posed(name, threshold):
    """Every condition at once: the reference agrees with its longdouble version, the support does not move with
    G | b inside the bar, and neither do the coefficients by more than 1e-9."""
    f = fit_checks(name, threshold)
    return f.reference_agrees and f.support_stable and f.coef_move <= WELL_POSED_COEF


# The GPU file asserts the fit (support, iteration count, coefficients within COEF_ATOL) of every case but these, per
# threshold: here the reference does not decide the fit (tests/test_step_matrix.py shows it for each: a single patient
# leaves the statics' columns exactly collinear, so the unbias solve is singular).  They assert G | b only.
GB_ONLY = {
    THRESHOLD: ("n1_s",),
    THRESHOLD_LOW: ("n1_s", "n1_o"),
}
# The cases that also pass the coefficient part of well_posed.  For the others the supports are stable but a move of
# G | b by 1e-10 x scale moves a coefficient by 1e-9 .. 1e-6: these libraries on statics in [0.6, 1.6] have Gram
# condition numbers of 1e2 .. 1e5, so the G | b bar alone does not imply the coefficient bar there.  The GPU file
# asserts both bars on them all the same, each being the project's own (tests/test_gpu_fused.py).
WELL_POSED = {
    THRESHOLD: ("n1_o", "allshort_s", "allshort_o", "c2113_g2_s", "u3_c1025_g1_o"),
    THRESHOLD_LOW: ("allshort_s", "allshort_o"),
}


def asserts_fit(name, threshold):
    return name not in GB_ONLY[threshold]


# ---------------------------------------------------------------------------------------------------
# e. rollout cases
# ---------------------------------------------------------------------------------------------------
Roll = collections.namedtuple("Roll", "name Nr Tr bits method")
# bits: "tm" time-major words with ld_arm = ceil(Nr / 32); "tm_even" the same words in rows padded to the next even
# word count (a last tile of <= 32 patients then takes the wide two-word load where "tm" takes the per-lane one:
# rollout_bits_range, wide = lda < 0 || 2 * tile + 1 < lda); "tile" tile-major [ceil(Nr / 64), Tr, 2]
# method: rk4 | euler5 | euler3 (method "euler" with substeps 3)
ROLL_CASES = [
    Roll("r1_t1", 1, 1, "tm", "rk4"),
    Roll("r1_t33", 1, 33, "tile", "euler5"),
    Roll("r31_t5", 31, 5, "tm", "euler3"),
    Roll("r31_t64", 31, 64, "tm_even", "rk4"),
    Roll("r33_t16", 33, 16, "tm", "euler5"),
    Roll("r33_t97", 33, 97, "tile", "rk4"),
    Roll("r64_t17", 64, 17, "tm", "rk4"),
    Roll("r64_t32", 64, 32, "tm_even", "euler3"),
    Roll("r65_t33_lane", 65, 33, "tm", "rk4"),
    Roll("r65_t33_wide", 65, 33, "tm_even", "rk4"),
    Roll("r65_t201", 65, 201, "tile", "euler5"),
    Roll("r96_t64_lane", 96, 64, "tm", "euler5"),
    Roll("r96_t64_wide", 96, 64, "tm_even", "euler5"),
    Roll("r96_t5", 96, 5, "tile", "euler3"),
    Roll("r130_t97_lane", 130, 97, "tm", "rk4"),
    Roll("r130_t97_wide", 130, 97, "tm_even", "euler3"),
    Roll("r130_t32", 130, 32, "tile", "rk4"),
    Roll("r300_t201", 300, 201, "tm", "rk4"),
    Roll("r300_t17", 300, 17, "tm_even", "euler5"),
    Roll("r300_t1", 300, 1, "tile", "rk4"),
    Roll("r300_t100", 300, 100, "tm", "rk4"),       # 5 tiles x 4 arm groups: the range cases
    Roll("r0_t5", 0, 5, "tm", "rk4"),               # n_rows = 0: gram only
]
ROLL = {c.name: c for c in ROLL_CASES}
assert len(ROLL) == len(ROLL_CASES)
LONGEST_ROLL = "r300_t201"
METHODS = {"rk4": ("rk4", None), "euler5": ("euler5", None), "euler3": ("euler", 3)}


def roll_ld_arm(c):
    W = ceil_div(c.Nr, 32)
    return {"tm": max(W, 1), "tm_even": W + 1 if W % 2 else W + 2, "tile": -c.Tr}[c.bits]


def last_tile_wide(c):
    """The load form rollout_bits_range takes on the last tile of the case."""
    lda = roll_ld_arm(c)
    return lda < 0 or 2 * (ceil_div(c.Nr, WAVE) - 1) + 1 < lda


@functools.lru_cache(maxsize=None)
def roll_inputs(name, lib):
    """(y0 [Nr], u [Nr, U], arm [Nr, Tr] int8 in {0, 1}, coef [2, 7]): |c| in [0.05, 0.15] with random signs, and the
    last coefficient of arm 1 below drop_below."""
    c = ROLL[name]
    rng = np.random.default_rng(M._seed("step-roll", name, lib))
    y0 = rng.uniform(0.5, 3.0, c.Nr)
    u = rng.uniform(0.6, 1.6, (c.Nr, LIBS[lib].n_statics))
    arm = rng.integers(0, 2, (c.Nr, c.Tr)).astype(np.int8)
    coef = rng.uniform(0.05, 0.15, (2, 7)) * rng.choice([-1.0, 1.0], (2, 7))
    coef[1, 6] = 0.5 * DROP_BELOW
    out = (y0, u, arm, coef)
    _freeze(*out)
    return out


def rollout_ref(y0, u, arm, coef, exps, dt, method, dtype=np.float64):
    """oracle.insite_ref.rollout (global model) in ``dtype``: y [Nr, Tr], the state after every interval."""
    meth, sub = METHODS[method]
    y = np.asarray(y0, dtype=dtype).copy()
    u = np.asarray(u, dtype=dtype)
    coef = np.asarray(coef, dtype=dtype)
    N, T = arm.shape
    out = np.empty((N, T), dtype=dtype)
    n_sub = R.STEPS_FOR_DT if meth == "euler5" else int(sub or 1)
    h = dtype(dt) / dtype(n_sub)
    half, two, six = dtype(0.5), dtype(2.0), dtype(6.0)
    for k in range(T):
        cr = coef[arm[:, k].astype(np.int64)]
        for _ in range(n_sub):
            if meth == "rk4":
                k1 = R.rhs_literal(y, u, cr, exps)
                k2 = R.rhs_literal(y + half * h * k1, u, cr, exps)
                k3 = R.rhs_literal(y + half * h * k2, u, cr, exps)
                k4 = R.rhs_literal(y + h * k3, u, cr, exps)
                y = y + (h / six) * (k1 + two * k2 + two * k3 + k4)
            else:
                y = y + R.rhs_literal(y, u, cr, exps) * h
        out[:, k] = y
    return out


@functools.lru_cache(maxsize=None)
def roll_ref(name, lib):
    c = ROLL[name]
    y = rollout_ref(*roll_inputs(name, lib), exps_of(lib), ROLLOUT_DT, c.method)
    _freeze(y)
    return y


# ---------------------------------------------------------------------------------------------------
# f. pairs: every discovery case and every rollout case at least once (round robin), plus the range cases
# ---------------------------------------------------------------------------------------------------
def _pairs():
    nd, nr = len(DISC_CASES), len(ROLL_CASES)
    out = [(DISC_CASES[k % nd].name, ROLL_CASES[k % nr].name) for k in range(max(nd, nr))]
    # ranges that start mid-tile and straddle tiles: 20 units over the 4 waves an over-large gram_blocks leaves;
    # hundreds of rollout waves, most without a unit, with one gram block
    out += [("t40_s", "r300_t100"), ("t8_o", "r300_t100"), ("t15_s", "r300_t100"), ("u3_t40_o", "r300_t100"),
            ("u3_t6_s", "r300_t100")]
    # the claimed tail next to the longest rollout and to the empty one
    out += [("c1025_g1_s", LONGEST_ROLL), ("c2113_g2_s", "r0_t5"), ("u3_c1025_g1_o", "r130_t97_wide")]
    seen = []
    for p in out:
        if p not in seen:
            seen.append(p)
    return seen


PAIRS = _pairs()
