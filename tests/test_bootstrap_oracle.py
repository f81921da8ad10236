"""CPU tests of the bootstrap's definition (include/insite_bootstrap.h) on its numpy restatement
(tests/bootstrap_ref.py): the threshold table, the weights, that weighting per-patient moments IS resampling
patients, and the published equations as replicate 0 with the inclusion frequencies of their supports."""
import json
import math
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import bootstrap_ref as BR
import library_matrix as M
from oracle import insite_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ANCHORS = json.load(open(os.path.join(HERE, "golden", "reference_log_anchors.json")))
NAMES = R.library_names(R.poly_library(3, 2, True), ["x0", "u0", "u1"])


def test_thresholds_are_the_poisson_cdf():
    """T_k = floor(2^32 CDF_k) of Poisson(1), computed at 60 digits (decimal) and from the exact series of 1 / e
    (fractions): the header's list, the helper's and the package's."""
    from insite_amd import bootstrap as B
    getcontext().prec = 60
    inv_e = Decimal(1) / Decimal(1).exp()
    cdf, dec = Decimal(0), []
    for k in range(12):
        cdf += inv_e / math.factorial(k)
        dec.append(int((cdf * 2 ** 32).to_integral_value(rounding="ROUND_FLOOR")))
    fr_e = sum(Fraction((-1) ** n, math.factorial(n)) for n in range(60))      # 1 / e to 1 / 60!
    cdf, fr = Fraction(0), []
    for k in range(12):
        cdf += fr_e / math.factorial(k)
        fr.append((cdf * 2 ** 32).__floor__())
    assert tuple(dec) == tuple(fr) == BR.THRESHOLDS == tuple(int(v) for v in B.poisson_thresholds())
    assert all(0 < v < 2 ** 32 for v in dec) and len(dec) == 12
    src = open(os.path.join(os.path.dirname(HERE), "include", "insite_bootstrap.h")).read()
    for v in dec:
        assert str(v) in src


def test_weights():
    from insite_amd import bootstrap as B
    w = BR.weights(7, 257, 1000)
    assert np.all(w[0] == 1) and w.min() >= 0 and w.max() <= 12
    draws = w[1:]                                                  # 256 x 1000 draws
    assert 0.98 <= draws.mean() <= 1.02 and 0.36 <= (draws == 0).mean() <= 0.375
    # a shard with its offset draws its slice of the whole cohort's weights (even, odd and past-2^32 offsets)
    whole = BR.weights(3, 9, 64)
    for off in (0, 1, 2, 37):
        assert np.array_equal(BR.weights(3, 9, 21, off), whole[:, off:off + 21])
    big = 2 ** 32 + 5
    assert np.array_equal(BR.weights(3, 9, 21, big), BR.weights(3, 9, 30, big - 3)[:, 3:24])
    hi = BR.weights(3, 9, 8, 2 ** 32 + 5)
    assert not np.array_equal(hi[1:], BR.weights(3, 9, 8, 5)[1:])    # the counter's high word is used
    assert not np.array_equal(BR.weights(3, 9, 64)[1:], BR.weights(4, 9, 64)[1:])
    # the package's restatement is the same integers
    for off in (0, 1, 2 ** 32 + 5):
        assert np.array_equal(B.weights(7, 17, 130, off), BR.weights(7, 17, 130, off))


def test_weighted_moments_equal_literal_resampling():
    """One replicate on the reference's EQ_4_D cohort: the weighted per-patient Gram equals the Gram of the cohort
    with every patient repeated w times (oracle.insite_ref.gram_moments), to 1e-12 of the largest entry."""
    x, u, arm, rows, exps, mom = BR.published_cohort("EQ_4_D")
    w = BR.weights(7, 2, x.shape[0])[1]
    rep = np.repeat(np.arange(x.shape[0]), w)
    assert rep.size != x.shape[0] or not np.array_equal(rep, np.arange(x.shape[0]))
    G_lit, b_lit = R.gram_moments(x[rep], u[rep], arm[rep], rows[rep], R.STANDARD_DT, exps)
    G, b, _, _ = BR.gram(mom, u, arm, rows, 5, exps, 2, 2, 7)
    eg = np.max(np.abs(G[1] - G_lit)) / np.max(np.abs(G_lit))
    eb = np.max(np.abs(b[1] - b_lit)) / np.max(np.abs(b_lit))
    print(f"weighted vs literal: G {eg:.2e} b {eb:.2e}")
    assert eg <= 1e-12 and eb <= 1e-12
    # replicate 0 is the cohort itself
    G0, b0 = R.gram_moments(x, u, arm, rows, R.STANDARD_DT, exps)
    assert np.max(np.abs(G[0] - G0)) <= 1e-12 * np.max(np.abs(G0))
    assert np.max(np.abs(b[0] - b0)) <= 1e-12 * np.max(np.abs(b0))


def test_float64_reference_against_longdouble():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 here: the self-check has no reference")
    rng = np.random.default_rng(11)
    for name, n_arms in (("std7", 2), ("u3_mixed9", 3), ("high_pow", 1), ("x_only", 4)):
        exps = M.exps_of(name)
        N = 130
        mom = BR.numpy_moments(rng, N)
        u = rng.uniform(0.6, 1.6, (N, exps.shape[1] - 1))
        arm = rng.integers(0, n_arms, N)
        rows = rng.integers(3, 9, N)
        f64 = BR.gram(mom, u, arm, rows, 5, exps, n_arms, 5, 9, 1)
        ld = BR.gram(mom.astype(np.longdouble), u.astype(np.longdouble), arm, rows, 5, exps, n_arms, 5, 9, 1)
        for k, what in ((0, "G"), (1, "b")):
            r = M.worst_ratio(f64[k], ld[k], ld[k + 2])
            assert r <= M.SELF_RTOL, (name, what, r)


def _logged(eq):
    out = np.zeros((2, len(NAMES)))
    for a, part in enumerate(ANCHORS[f"{eq}/sindy"]["global_equation_string"].split(" | ")):
        for term in part.split("= ", 1)[1].split("+")[1:]:
            c, name = term.split("*", 1)
            out[a, NAMES.index(name.replace("*", " "))] = float(c)
    return out


@pytest.mark.parametrize("eq", ["EQ_4_A", "EQ_4_D"])
def test_published_equations_and_inclusion(eq):
    """Replicate 0 through the oracle's STLSQ is the published equation; over R = 64 every replicate keeps exactly
    the published support."""
    _, u, arm, rows, exps, mom = BR.published_cohort(eq)
    ref = _logged(eq)
    Rn = 64
    G, b, _, _ = BR.gram(mom, u, arm, rows, 5, exps, 2, Rn, 7)
    coef = np.stack([[R.stlsq_gram(G[r, a], b[r, a], 0.1, 0.5)[0] for a in range(2)] for r in range(Rn)])
    assert np.array_equal(coef[0] != 0, ref != 0)
    assert np.max(np.abs(coef[0] - ref)) < 1e-10
    inclusion = (coef[1:] != 0).mean(0)
    assert np.array_equal(inclusion, (ref != 0).astype(float)), inclusion
    lo, hi = np.quantile(coef[1:], [0.025, 0.975], axis=0)
    assert np.all((lo <= coef[0] + 1e-3) & (coef[0] - 1e-3 <= hi))
