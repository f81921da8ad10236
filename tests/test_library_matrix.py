"""CPU checks of the library matrix (tests/library_matrix.py): the table is pinned, every kernel family meets a
library that fits the MFMA contraction plan and one that does not, every float64 reference the GPU file compares
with lies within 1e-13 x its per-entry scale of its numpy.longdouble version (the condition that keeps the GPU
tolerance of 1e-10 x scale honest) and equals the project's own restatement, and the SR3 systems decide their
iteration counts away from the stopping threshold, so the GPU test leaves no system out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irregular_ref as IR  # noqa: E402
import library_matrix as M  # noqa: E402
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import segments_ref as S  # noqa: E402

LD = np.longdouble
# distinct (atom, moment) columns of the tables the plan accepts
Q_COLUMNS = {"x_only": 2, "bias_x": 5, "lin3": 11, "std7": 13, "noone3": 7, "dup4": 7, "u3_first9": 16, "u3_x9": 10}


@pytest.mark.parametrize("name", list(M.TABLE))
def test_table_is_pinned(name):
    F, U, fits = M.TABLE[name]
    lib = M.LIBS[name]
    assert lib.exps.dtype == np.int8 and lib.exps.shape == (F, 1 + U)
    assert lib.n_terms == F and lib.n_statics == U and len(lib.input_names) == 1 + U
    assert lib.exps[:, 0].max() <= 1 and lib.exps.min() >= 0 and lib.exps.max() <= 8
    assert M.mfma_fits(lib.exps, 1) is fits
    q = M.q_columns(lib.exps)
    if name in Q_COLUMNS:
        assert len(q) == Q_COLUMNS[name]
    else:
        assert q is None or len(q) > 16


def test_tables_have_the_properties_they_are_named_for():
    e = {k: M.exps_of(k) for k in M.TABLE}
    assert not (e["noone3"][:, 1:] == 0).all(axis=1).any()      # no column with zero static exponents: "1" is appended
    assert (e["u3_x9"][:, 0] == 1).all() and (e["u3_x9"][:, 1:] == 0).all(axis=1).sum() == 1   # no bias, 9 atoms
    assert len({tuple(r) for r in e["u3_x9"][:, 1:].tolist()}) == 9
    assert np.array_equal(e["dup4"][1], e["dup4"][2])           # a duplicate column
    assert (e["x_only"].shape, e["bias_x"].shape) == ((1, 1), (2, 1))                          # U = 0
    assert e["u3_mixed9"][0].sum() == 0 and e["u3_mixed9"][:, 1:].max() == 2                   # bias first, any order
    assert e["high_pow"].max() == 8 and M.q_columns(e["high_pow"]) is None
    assert np.array_equal(e["std7"], R.poly_library(3, 2, True))
    assert np.array_equal(e["lin3"], R.poly_library(4, 1, True))
    assert np.array_equal(e["u3_first9"], R.poly_library(4, 2, True)[:9])
    full = R.poly_library(3, 2, False)
    assert np.array_equal(e["deg2_no_xx"], full[full[:, 0] < 2]) and full.shape[0] == 10


def test_planner_verdicts_named_by_the_issue():
    f = lambda name, A: M.mfma_fits(M.exps_of(name), A)   # noqa: E731
    assert f("u3_first9", 1)                       # 16 Q columns: exactly at the limit
    assert f("noone3", 4) and f("dup4", 4)         # 12 -> 16 padded rows, 16 rows
    assert f("noone3", 3)                          # three arms count as four: 12 rows
    assert not f("lin3", 3)                        # padded 20 although 15 <= 16
    assert not f("lin3", 4) and f("lin3", 2) and not f("std7", 3) and f("std7", 2)
    assert not f("u3_first9", 2) and not f("u3_x9", 2)
    assert not f("deg2_no_xx", 1)                  # Q overflow
    assert not f("u3_mixed9", 1)
    assert not f("high_pow", 1)                    # static exponent above 2
    assert [M.narm_pad(a) for a in (1, 2, 3, 4)] == [1, 2, 4, 4]


def test_every_family_meets_a_fitting_and_a_non_fitting_pair():
    families = {
        "strong": [(n, a) for n, a, _ in M.STRONG_CASES],
        "weak": [(n, a) for n in M.SCALAR_LIBS for a in M.WEAK_ARMS],
        "irregular": [(n, a) for n in M.SCALAR_LIBS for a in M.IRR_ARMS],
        "segments": [(n, a) for n in M.SCALAR_LIBS for a in M.SEG_ARMS],
        "rollout": [(n, a) for n in M.ROLLOUT_LIBS for a in (2, 4)],
        "rk45": [(n, 2) for n in M.ROLLOUT_LIBS],
    }
    for fam, pairs in families.items():
        verdicts = {M.mfma_fits(M.exps_of(n), a) for n, a in pairs}
        assert verdicts == {True, False}, fam
    # the strong cases hold what the issue lists and reach every padded arm count on either path
    assert len(M.STRONG_CASES) == 23 + 6
    for pad in (1, 2, 4):
        assert {M.mfma_fits(M.exps_of(n), a) for n, a, _ in M.STRONG_CASES if M.narm_pad(a) == pad} == {True, False}
    for fam in ("weak", "irregular", "segments", "rollout"):
        sizes = {M.TABLE[n][:2] for n, _ in families[fam]}
        assert {f for f, _ in sizes} >= {1, 9} and {u for _, u in sizes} >= {0, 3}, fam


def _self_check(f64, ld, pairs, what):
    """pairs: (index of the value, index of its scale) in the reference tuples."""
    worst = 0.0
    for iv, isc in pairs:
        r = M.worst_ratio(f64[iv], ld[iv], ld[isc])
        worst = max(worst, r)
        assert r <= M.SELF_RTOL, (what, iv, r)
        assert np.all(np.asarray(ld[isc]) >= 0)
    return worst


@pytest.mark.parametrize("fd", M.STRONG_FDS)
@pytest.mark.parametrize("name,n_arms,T", M.STRONG_CASES)
def test_strong_reference(name, n_arms, T, fd):
    x, u, arm, rows = M.strong_inputs(name, n_arms, T)
    assert x.shape == (M.N_FULL, T) and set(M.EDGE_ROWS + (T,)) <= set(rows.tolist())
    assert np.isnan(x[np.arange(T)[None, :] >= rows[:, None]]).all()
    assert arm.min() == 0 and arm.max() == n_arms - 1 and (n_arms != 3 or not (arm == 1).any())
    f64 = M.strong_ref(name, n_arms, T, fd)
    ld = M.gram_ref(x, u, arm, rows, M.DT, M.exps_of(name), n_arms, fd, LD)
    assert ld[0].dtype == LD and f64[0].dtype == np.float64
    w = _self_check(f64, ld, ((0, 2), (1, 3)), (name, n_arms, T, fd))
    print(f"float64 vs longdouble: {w:.2e} x scale")
    # the restatement is the oracle's
    Go, bo = R.gram_moments(x, u, arm, rows, M.DT, M.exps_of(name), n_arms, fd)
    assert M.worst_ratio(f64[0], Go, f64[2]) <= M.SELF_RTOL and M.worst_ratio(f64[1], bo, f64[3]) <= M.SELF_RTOL
    # the cohort keeps the right-hand side away from cancellation: |b| is a fair share of its scale
    on = f64[3] > 0
    assert np.median(np.abs(f64[1][on]) / f64[3][on]) > 0.3
    if n_arms == 3:
        assert not f64[0][1].any() and not f64[2][1].any()


def test_strong_reference_does_not_depend_on_the_patient_order():
    name, n_arms, T, fd = "u3_first9", 1, M.STRONG_T, "smoothed4"
    x, u, arm, rows = M.strong_inputs(name, n_arms, T)
    f64 = M.strong_ref(name, n_arms, T, fd)
    perm = np.random.default_rng(0).permutation(x.shape[0])
    again = M.gram_ref(x[perm], u[perm], arm[perm], rows[perm], M.DT, M.exps_of(name), n_arms, fd)
    assert M.worst_ratio(again[0], f64[0], f64[2]) <= 1e-14 and M.worst_ratio(again[1], f64[1], f64[3]) <= 1e-14
    assert np.array_equal(again[4], f64[4][perm])


@pytest.mark.parametrize("fd", M.STRONG_FDS)
def test_short_wave_reference(fd):
    x, u, arm, rows = M.short_wave_inputs()
    assert x.shape == (65, M.STRONG_T) and rows[64] == 3 and (rows[:64] >= 5).any()
    f64 = M.gram_ref(x, u, arm, rows, M.DT, M.exps_of("std7"), 2, fd)
    ld = M.gram_ref(x, u, arm, rows, M.DT, M.exps_of("std7"), 2, fd, LD)
    _self_check(f64, ld, ((0, 2), (1, 3)), ("short wave", fd))
    assert not f64[4][rows < 5].any() and np.array_equal(f64[4][:, 0], np.where(rows < 5, 0, rows))


@pytest.mark.parametrize("n_arms", M.WEAK_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_weak_reference(name, n_arms):
    x, u, arm, rows, W, D = M.weak_inputs(name, n_arms)
    N, T, K = M.WEAK_SHAPE
    assert W.shape == D.shape == (K, T) and not W[16:32].any() and not D[16:32].any() and np.all(W[32] != 0)
    on = WR.contributes(rows, arm, T, n_arms)
    assert 0.6 * N < on.sum() < N and np.isnan(x[~on]).all() and np.isfinite(x[on]).all()
    assert (arm == -1).any() and (arm == n_arms).any() and (rows == T + 3).any() and (rows == T - 1).any()
    f64 = M.weak_case_ref(name, n_arms)
    ld = M.weak_ref(x, u, arm, rows, W, D, M.exps_of(name), n_arms, LD)
    assert ld[0].dtype == LD
    w = _self_check(f64, ld, ((0, 2), (1, 3), (4, 5)), (name, n_arms))
    print(f"float64 vs longdouble: {w:.2e} x scale")
    assert not f64[4][~on].any()


@pytest.mark.parametrize("fd", M.IRR_FDS)
@pytest.mark.parametrize("n_arms", M.IRR_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_irregular_reference(name, n_arms, fd):
    x, t, n_obs, u, arm = M.irregular_inputs(name, n_arms)
    assert x.shape == M.IRR_SHAPE and set(IR.edge_lengths(M.IRR_SHAPE[1]).tolist()) <= set(n_obs.tolist())
    assert (arm == -1).any() and (arm == n_arms).any()
    f64 = M.irregular_case_ref(name, n_arms, fd)
    ld = M.irregular_ref(x, t, n_obs, u, arm, M.exps_of(name), n_arms, fd, LD)
    assert ld[0].dtype == LD
    w = _self_check(f64, ld, ((0, 2), (1, 3)), (name, n_arms, fd))
    print(f"float64 vs longdouble: {w:.2e} x scale")
    assert np.abs(f64[4] - ld[4]).max() <= 1e-12 * np.abs(ld[4]).max()
    Go, bo, momo = IR.gram_irregular(np.nan_to_num(x), np.nan_to_num(t), n_obs, u, arm, M.exps_of(name), n_arms, fd)
    assert M.worst_ratio(f64[0], Go, f64[2]) <= M.SELF_RTOL and M.worst_ratio(f64[1], bo, f64[3]) <= M.SELF_RTOL
    assert np.array_equal(f64[4], momo)


@pytest.mark.parametrize("fd", M.SEG_FDS)
@pytest.mark.parametrize("n_arms", M.SEG_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_segment_reference(name, n_arms, fd):
    x, u, arm, sl = M.segment_inputs(name, n_arms)
    T = M.SEG_SHAPE[1]
    assert x.shape == M.SEG_SHAPE and arm.shape == (M.N_FULL, T - 1) and {0, 1, 2, T - 1} <= set(sl.tolist())
    assert set(np.unique(arm).tolist()) == set(range(n_arms))
    f64 = M.segment_case_ref(name, n_arms, fd)
    ld = M.segments_ref(x, u, arm, sl, M.DT, M.exps_of(name), n_arms, fd, LD)
    assert ld[0].dtype == LD
    w = _self_check(f64, ld, ((0, 2), (1, 3)), (name, n_arms, fd))
    print(f"float64 vs longdouble: {w:.2e} x scale")
    Go, bo, _ = S.gram_segments(x, u, arm, sl, M.DT, M.exps_of(name), n_arms, fd)
    assert M.worst_ratio(f64[0], Go, f64[2]) <= M.SELF_RTOL and M.worst_ratio(f64[1], bo, f64[3]) <= M.SELF_RTOL


@pytest.mark.parametrize("F", M.SR3_F + (10,))
def test_sr3_systems_need_no_exclusions(F):
    """No stopping value of the restatement lies within 1e-6 (relative) of tol, and every system iterates: the
    GPU test compares every iteration count."""
    G, b = M.solver_systems(F)
    assert G.shape == (32, F, F) and b.shape == (32, F)
    for unbias in (True, False):
        for s in range(32):
            coef, sup, it, stops = WR.sr3(G[s], b[s], M.SR3_THRESHOLD, tol=M.SR3_TOL, unbias=unbias)
            assert it > 0 and np.all(np.isfinite(coef)), (F, s)
            assert all(abs(v - M.SR3_TOL) > 1e-6 * M.SR3_TOL for v in stops), (F, s, stops)


def test_sr3_default_tolerance_sits_on_the_first_stopping_value_at_one_term():
    """Why the GPU test does not use tol = threshold / nu: with one term the first stopping value is
    threshold / nu up to rounding for every system whose coefficient survives the first shrink."""
    G, b = M.solver_systems(1)
    near = sum(abs(WR.sr3(G[s], b[s], M.SR3_THRESHOLD)[3][0] - 0.1) <= 1e-6 * 0.1 for s in range(32))
    assert near >= 8


@pytest.mark.parametrize("F", M.SOLVER_F)
def test_stlsq_systems_are_well_posed(F):
    G, b = M.solver_systems(F)
    for s in range(32):
        coef, ind, it = R.stlsq_gram(G[s], b[s], M.STLSQ_THRESHOLD, M.STLSQ_ALPHA)
        assert it >= 1 and np.all(np.isfinite(coef))
        # no ridge iterate sits on the threshold: the support does not hang on the last bit
        assert np.linalg.cond(G[s]) < 1e4


@pytest.mark.parametrize("name", M.ROLLOUT_LIBS)
def test_rollout_inputs(name):
    ex = M.exps_of(name)[:, 0]
    F = M.TABLE[name][0]
    for n_arms in (2, 4):
        y0, u, arm, coef = M.rollout_inputs(name, n_arms)
        assert coef.shape == (n_arms, F) and (np.abs(coef) <= M.DROP_BELOW).sum() == 1
        assert set(np.unique(arm).tolist()) == set(range(n_arms))
        for a in range(n_arms):
            for e in (0, 1):
                if (ex == e).any() and not (F == 1 and a == n_arms - 1):
                    assert (np.abs(coef[a][ex == e]) > M.DROP_BELOW).any()
        for method in ("euler5", "rk4"):
            assert np.all(np.isfinite(M.rollout_case_ref(name, n_arms, method)))
    t, n_obs, u, arm, y0, coef = M.rk45_inputs(name)
    y, steps = M.rk45_case_ref(name)
    assert np.array_equal(np.isnan(y), np.arange(M.RK45_N_MAX)[None, :] >= (n_obs - 1)[:, None])
    assert n_obs.min() >= M.RK45_N_MIN and np.abs(y[~np.isnan(y)]).max() < 1e6
