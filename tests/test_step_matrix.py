"""CPU checks of the step matrix (tests/step_matrix.py): every float64 reference the GPU file compares with lies within
1e-13 x its per-entry scale of its numpy.longdouble version, the planner restatement says "claimed" or "static" exactly
where the case list does, every shape passes the entry points' argument checks, both libraries take the MFMA plan, the
rollout reference is the oracle's and drifts from longdouble far less than the GPU tolerance on the longest case, and
the fits the GPU file asserts are the ones the reference decides.

The fit checks (SM.fit_checks): one would like every asserted fit to keep its support AND its coefficients within 1e-9
when G | b move entrywise by +-1e-10 x scale, so that the Gram bar implied the coefficient bar.  The supports do (for
every case but the two single-patient ones); the coefficients do not: the two libraries on statics in [0.6, 1.6] give
Gram condition numbers of 1e2 .. 1e5, and such a move shifts a coefficient by 1e-9 .. 1e-6 on 34 of the 40 cases at
threshold 0.1 and on 36 at 0.02 (test_coefficient_moves_are_pinned prints them).  So the Gram bar does not imply the
coefficient bar on these cohorts, and the GPU file asserts each of the two bars on its own: the coefficients against
the reference fit at 1e-8 on every case whose support the reference decides, which is all but the cases of
SM.GB_ONLY."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
import step_matrix as SM  # noqa: E402
from oracle import insite_ref as R  # noqa: E402

LD = np.longdouble
NAMES = [c.name for c in SM.DISC_CASES]
THRESHOLDS = (SM.THRESHOLD, SM.THRESHOLD_LOW)


# ---------------------------------------------------------------------------------------------------
# libraries and the planner
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", list(SM.LIBS))
def test_libraries_take_the_step_kernels(lib):
    e = SM.exps_of(lib)
    assert e.shape[0] == 7 and e[:, 0].max() <= 1 and e[:, 1:].max() <= 2
    assert len(M.q_columns(e)) == SM.Q_COLUMNS[lib] <= 16 and M.mfma_fits(e, 2)
    assert SM.LIBS[lib].n_statics == e.shape[1] - 1
    if lib == "u3_nobias7":
        assert not (e == 0).all(axis=1).any() and e.shape[1] == 4


def test_case_list_spans_what_it_is_meant_to():
    C = SM.DISC_CASES
    assert {c.T for c in C} >= {5, 7, 8, 9, 15, 16, 17, 23, 40}
    assert {c.N for c in C} >= {1, 63, 64, 65, 300}
    assert {c.pattern for c in C} == {"ragged", "full", "clamp", "short_mid", "short_last", "short_tail", "all_short"}
    assert {c.gram_blocks for c in C} == {0, 1, 2, 7, SM.GB_OVER}
    for lib in SM.LIBS:
        for fd in ("smoothed4", "order4"):
            assert {c.path for c in C if c.lib == lib and c.fd == fd} >= {"static"}
        assert {c.path for c in C if c.lib == lib} == {"static", "claimed"}
    assert {(c.fd, c.path) for c in C} == {(f, p) for f in ("smoothed4", "order4") for p in ("static", "claimed")}
    # the smoothed short-trajectory lengths 5, 6, 7 each occur as a row count
    for L in (5, 6, 7):
        assert any(c.fd == "smoothed4" and (np.minimum(SM.disc_inputs(c.name)[3], c.T) == L).any() for c in C)
    R_ = SM.ROLL_CASES
    assert {c.Nr for c in R_} >= {1, 31, 33, 64, 65, 96, 130, 300}
    assert {c.Tr for c in R_} >= {1, 5, 16, 17, 32, 33, 64, 97, 201}
    assert {(c.bits, c.method) for c in R_} == {(b, m) for b in ("tm", "tm_even", "tile") for m in SM.METHODS}
    assert max(c.Tr for c in R_) <= 201
    # every case is paired at least once
    assert {d for d, _ in SM.PAIRS} == set(SM.DISC) and {r for _, r in SM.PAIRS} == set(SM.ROLL)
    assert len(SM.PAIRS) == len(set(SM.PAIRS))


@pytest.mark.parametrize("name", NAMES)
def test_claimed_tail_predicate(name):
    c = SM.DISC[name]
    if c.gram_blocks in (0, SM.GB_OVER):
        # the planner's own block count (half the grid, or the grid less two): at least one, so units below the
        # threshold of a single block are static whatever the grid
        assert c.path == "static" and not SM.claimed_tail(c.N, c.T, 1)
    else:
        assert SM.claimed_tail(c.N, c.T, c.gram_blocks) is (c.path == "claimed")


def test_claimed_tail_cases_named_by_the_issue():
    assert SM.gram_units(1025, 490) == 17 * 31 == 527 and SM.gram_units(2113, 490) == 34 * 31 == 1054
    assert SM.claimed_tail(1025, 490, 1) and not SM.claimed_tail(1025, 490, 2) and SM.claimed_tail(2113, 490, 2)
    # four tail tiles of 16 pieces: fifteen of two groups and a last one of a single group
    assert SM.tail_geometry(1025, 490) == (13, 16, 64, 1)
    assert SM.tail_geometry(2113, 490) == (26, 16, 128, 1)
    # the all-short tile of the short_tail pattern is a claimed one; the ragged tail tiles hold rows < 5 too
    rows = SM.disc_inputs("c1025_g1_shorttail")[3]
    assert 13 <= 14 < 17 and (rows[14 * 64:15 * 64] < 5).all() and (rows[13 * 64:14 * 64] >= 5).any()
    rows = SM.disc_inputs("c1025_g1_s")[3]
    assert (rows[13 * 64:] < 5).any() and (rows[13 * 64:] >= 5).any()


@pytest.mark.parametrize("d,r", SM.PAIRS)
def test_shapes_pass_the_argument_checks(d, r):
    c, q = SM.DISC[d], SM.ROLL[r]
    assert SM.args_ok(c.N, c.T, c.N + 5, c.lib, q.Nr, q.Tr, SM.roll_ld_arm(q), q.Nr + 5, c.gram_blocks)
    assert SM.args_ok(0, c.T, c.N + 5, c.lib, q.Nr, q.Tr, SM.roll_ld_arm(q), q.Nr + 5, c.gram_blocks)   # the flush
    assert SM.DISC[SM.next_in_stream(d)].lib == c.lib and SM.next_in_stream(d) != d


def test_bit_layouts_take_both_load_forms():
    wide = {c.name: SM.last_tile_wide(c) for c in SM.ROLL_CASES if c.Nr}
    for a, b in (("r65_t33_lane", "r65_t33_wide"), ("r96_t64_lane", "r96_t64_wide"),
                 ("r130_t97_lane", "r130_t97_wide")):
        assert not wide[a] and wide[b]
        assert SM.ROLL[a][1:3] == SM.ROLL[b][1:3]
    assert not wide["r1_t1"] and not wide["r31_t5"] and wide["r31_t64"] and wide["r1_t33"]
    assert SM.roll_ld_arm(SM.ROLL["r65_t33_lane"]) == 3 and SM.roll_ld_arm(SM.ROLL["r65_t33_wide"]) == 4
    assert SM.roll_ld_arm(SM.ROLL["r64_t32"]) == 4 and SM.roll_ld_arm(SM.ROLL["r130_t32"]) == -32
    # the range case: 5 tiles x 4 arm groups
    q = SM.ROLL["r300_t100"]
    assert SM.ceil_div(q.Nr, SM.WAVE) * SM.ceil_div(q.Tr, SM.ROLL_GS) == 20


# ---------------------------------------------------------------------------------------------------
# cohorts and Gram references
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cohort(name):
    c = SM.DISC[name]
    x, u, arm, rows = SM.disc_inputs(name)
    assert x.shape == (c.N, c.T) and u.shape == (c.N, SM.LIBS[c.lib].n_statics) and set(arm.tolist()) <= {0, 1}
    assert np.isnan(x[np.arange(c.T)[None, :] >= rows[:, None]]).all()
    assert np.isfinite(x[np.arange(c.T)[None, :] < rows[:, None]]).all()
    if c.pattern == "ragged" and c.N >= 9:
        assert set(M.EDGE_ROWS + (c.T,)) <= set(rows.tolist())
    if c.pattern == "full":
        assert (rows == c.T).all()
    if c.pattern in ("clamp",) or (c.pattern == "ragged" and c.T < 17 and c.N >= 9):
        assert (rows > c.T).any()
    if c.pattern == "short_mid":
        assert (rows[128:192] < 5).all() and (rows[:128] >= 5).any() and (rows[192:] >= 5).any()
    if c.pattern == "short_last":
        lo = (SM.ceil_div(c.N, 64) - 1) * 64
        assert (rows[lo:] < 5).all() and (rows[:lo] >= 5).any() and lo > 0
    if c.pattern == "all_short":
        assert (rows < 5).all() and set(rows.tolist()) == {0, 1, 2, 3, 4}
        G, b = SM.disc_ref(name)[:2]
        assert not G.any() and not b.any()


@pytest.mark.parametrize("name", NAMES)
def test_gram_reference(name):
    c = SM.DISC[name]
    f64 = SM.disc_ref(name)
    ld = SM.disc_ref(name, LD)
    assert ld[0].dtype == LD and f64[0].dtype == np.float64
    for iv, isc in ((0, 2), (1, 3)):
        r = M.worst_ratio(f64[iv], ld[iv], ld[isc])
        print(f"{name} float64 vs longdouble [{iv}]: {r:.2e} x scale")
        assert r <= SM.SELF_RTOL, (name, iv, r)
    x, u, arm, rows = SM.disc_inputs(name)
    Go, bo = R.gram_moments(np.nan_to_num(x), u, arm, np.minimum(rows, c.T), SM.DT, SM.exps_of(c.lib), 2, c.fd)
    assert M.worst_ratio(f64[0], Go, f64[2]) <= SM.SELF_RTOL and M.worst_ratio(f64[1], bo, f64[3]) <= SM.SELF_RTOL


# ---------------------------------------------------------------------------------------------------
# fits
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_asserted_fits_are_decided_by_the_reference(name, threshold):
    f = SM.fit_checks(name, threshold)
    if SM.asserts_fit(name, threshold):
        assert f.reference_agrees and f.support_stable, (name, threshold, f)
        coef, sup, it = SM.fit_ref(*SM.disc_ref(name)[:2], threshold)
        assert np.all(np.isfinite(coef)) and np.all(it >= 1) and np.array_equal(sup, np.abs(coef) > R.SUPPORT_EPS)
    else:
        assert not (f.reference_agrees and f.support_stable), (name, threshold, f)
        assert SM.DISC[name].N == 1


def test_few_cases_assert_the_gram_only():
    for t in THRESHOLDS:
        assert set(SM.GB_ONLY[t]) <= set(SM.DISC) and 4 * len(SM.GB_ONLY[t]) <= len(SM.DISC_CASES)


def test_zero_systems_fit_as_the_solver_defines():
    """Every patient below five rows: G = b = 0, no term survives, and the iteration count is 2 (the first iteration
    empties the support, the second finds it empty), for either threshold."""
    for name in ("allshort_s", "allshort_o"):
        for t in THRESHOLDS:
            coef, sup, it = SM.fit_ref(*SM.disc_ref(name)[:2], t)
            assert not coef.any() and not sup.any() and it.tolist() == [2, 2]


def test_the_low_threshold_keeps_three_terms():
    keeps = [name for name in NAMES if SM.asserts_fit(name, SM.THRESHOLD_LOW)
             and SM.fit_ref(*SM.disc_ref(name)[:2], SM.THRESHOLD_LOW)[1].sum(axis=1).max() >= 3]
    assert 4 * len(keeps) >= 3 * len(NAMES), keeps
    differs = [name for name in keeps if not np.array_equal(SM.fit_ref(*SM.disc_ref(name)[:2], SM.THRESHOLD_LOW)[1],
                                                            SM.fit_ref(*SM.disc_ref(name)[:2], SM.THRESHOLD)[1])]
    assert 2 * len(differs) >= len(NAMES)     # and it is another fit than the one at 0.1


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_coefficient_moves_are_pinned(threshold):
    """Which cases pass every condition of SM.well_posed, and by how much the others' coefficients move."""
    passed = []
    for name in NAMES:
        f = SM.fit_checks(name, threshold)
        print(f"{name} thr {threshold}: reference agrees {f.reference_agrees}, support stable {f.support_stable}, "
              f"coefficients move by {f.coef_move:.2e}")
        if SM.well_posed(name, threshold):
            passed.append(name)
        elif SM.asserts_fit(name, threshold):
            assert SM.WELL_POSED_COEF < f.coef_move < 1e-5, (name, f)
    assert tuple(passed) == SM.WELL_POSED[threshold]


# ---------------------------------------------------------------------------------------------------
# rollouts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", list(SM.LIBS))
@pytest.mark.parametrize("name", [c.name for c in SM.ROLL_CASES])
def test_rollout_reference_is_the_oracles(name, lib):
    c = SM.ROLL[name]
    y0, u, arm, coef = SM.roll_inputs(name, lib)
    assert y0.shape == (c.Nr,) and arm.shape == (c.Nr, c.Tr) and coef.shape == (2, 7)
    assert (np.abs(coef) <= SM.DROP_BELOW).sum() == 1 and (np.abs(coef) >= 0.05).sum() == 13
    y = SM.roll_ref(name, lib)
    meth, sub = SM.METHODS[c.method]
    if c.Nr:
        assert np.array_equal(y, R.rollout(y0, u, arm, coef, SM.exps_of(lib), SM.ROLLOUT_DT, method=meth, substeps=sub))
        assert np.all(np.isfinite(y)) and np.abs(y).max() < 1e6
    # dropping the small coefficient is visible at the GPU tolerance: a rollout that kept it would fail
    if c.Nr >= 31 and c.Tr >= 16:
        kept = coef.copy()
        kept[1, 6] = 2.0 * SM.DROP_BELOW
        y2 = SM.rollout_ref(y0, u, arm, kept, SM.exps_of(lib), SM.ROLLOUT_DT, c.method)
        assert not np.allclose(y2, y, rtol=100 * SM.Y_RTOL, atol=100 * SM.Y_ATOL)


@pytest.mark.parametrize("lib", list(SM.LIBS))
@pytest.mark.parametrize("name", [SM.LONGEST_ROLL, "r65_t201", "r130_t97_wide"])
def test_rollout_reference_drift_is_far_inside_the_gpu_tolerance(name, lib):
    """float64 against longdouble on the longest case (and the longest of the other two methods): a tenth of the
    GPU test's rtol 1e-11 / atol 1e-12."""
    c = SM.ROLL[name]
    assert c.Tr == max(q.Tr for q in SM.ROLL_CASES if q.method == c.method)
    y = SM.roll_ref(name, lib)
    yl = SM.rollout_ref(*SM.roll_inputs(name, lib), SM.exps_of(lib), SM.ROLLOUT_DT, c.method, LD)
    assert yl.dtype == LD
    err = np.abs(y.astype(LD) - yl)
    print(f"{name} {lib}: worst relative drift {float((err / np.maximum(np.abs(yl), 1e-300)).max()):.2e}")
    assert np.all(err <= 0.1 * (SM.Y_ATOL + SM.Y_RTOL * np.abs(yl)))
