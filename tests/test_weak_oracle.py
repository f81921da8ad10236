"""CPU tests of the weak-form discovery: the numpy restatement (tests/weak_ref.py) against itself (moment
expansion vs literal rows, float64 vs longdouble), the Python helpers of insite_amd.weak against it, and the
restatement against the reference's published wsindy runs (tests/golden/reference_log_wsindy.json)."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EXPS = R.poly_library(3, 2, True)          # columns over (x0, u0, u1): 1 x0 u0 u1 x0u0 x0u1 u0u1
NAMES = R.library_names(EXPS, ["x0", "u0", "u1"])
DT = 10.0 / 60.0
THRESHOLD = 0.1                            # configs/config.yaml: sindy_threshold of the EQ_4 family


@functools.lru_cache(maxsize=None)
def cohort(eq):
    """The reference's seed-1 training cohort in DE format: x (1000, 60), rows all 58."""
    tr = RC.make_collection(eq, with_tests=False)["train"]
    x, u, arm, rows = R.de_format(tr.data, tr.scaling_params, 1)
    T = int(rows.max())
    assert np.all(rows == T)
    return x, u, arm, rows, T


@functools.lru_cache(maxsize=None)
def weak_system(eq, seed, K=100):
    x, u, arm, rows, T = cohort(eq)
    W, D = WR.weights(T, DT, np.random.default_rng(seed).uniform(WR.half_width(T, DT), (T - 1) * DT
                                                                  - WR.half_width(T, DT), K))
    return WR.gram(x, u, arm, rows, W, D, EXPS, 2)


def small_cohort(N=37, T=23, K=9, n_arms=3, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 3.0, (N, 1)) * np.exp(-rng.uniform(0.2, 1.0, (N, 1)) * np.arange(T) * DT) \
        + 0.01 * rng.normal(size=(N, T))
    u = rng.normal(0.5, 0.05, (N, 2))
    arm = rng.integers(-1, n_arms + 1, N)
    rows = np.where(rng.random(N) < 0.2, T - 1, T)
    H = WR.half_width(T, DT) * 3
    W, D = WR.weights(T, DT, rng.uniform(H, (T - 1) * DT - H, K), H=H)
    return x, u, arm, rows, W, D, n_arms


def test_moment_expansion_is_the_literal_gram():
    x, u, arm, rows, W, D, n_arms = small_cohort()
    G, b = WR.gram(x, u, arm, rows, W, D, EXPS, n_arms)
    mom = WR.moments(x, arm, rows, W, D, n_arms)
    Gm, bm = WR.gram_from_moments(mom, u, arm, EXPS, n_arms)
    scale = max(np.abs(G).max(), np.abs(b).max())
    assert scale > 0
    assert np.abs(Gm - G).max() <= 1e-12 * scale      # the project's Gram agreement
    assert np.abs(bm - b).max() <= 1e-12 * scale
    off = ~WR.contributes(rows, arm, W.shape[1], n_arms)
    assert off.any() and np.all(mom[off] == 0)


def test_draw_centres_is_the_numpy_draw():
    from insite_amd import weak
    for T, K, seed in ((58, 100, 0), (58, 100, 2), (7, 17, 11)):
        L = (T - 1) * DT
        H = L / 20.0
        ref = np.random.default_rng(seed).uniform(H, L - H, K)
        assert np.array_equal(weak.draw_centres(T, DT, K, seed), ref)


def test_test_function_weights_match_the_restatement():
    from insite_amd import weak
    for T, K, p, H in ((58, 100, 4, None), (7, 17, 4, None), (64, 16, 2, 0.9), (5, 1, 1, 0.3)):
        c = weak.draw_centres(T, DT, K, 3, H=H)
        W, D = weak.test_function_weights(T, DT, torch.as_tensor(c), H=H, p=p)
        assert W.device.type == "cpu" and W.dtype == torch.float64 and tuple(W.shape) == (K, T)
        Wr, Dr = WR.weights(T, DT, c, H=H, p=p)
        np.testing.assert_allclose(W.numpy(), Wr, rtol=1e-13, atol=1e-15 * DT)
        np.testing.assert_allclose(D.numpy(), Dr, rtol=1e-13, atol=1e-15 * DT)
        assert np.array_equal(W.numpy() == 0, Wr == 0)


def published(eq, seed=1):
    with open(os.path.join(HERE, "golden", "reference_log_wsindy.json")) as f:
        rec = json.load(f)[f"{eq}/wsindy/{seed}"]
    out = []
    for part in rec["global_equation_string"].split(" | "):
        terms = {}
        for m in re.finditer(r"\+(-?[0-9.eE+-]+?)\*([a-z0-9*]+)(?=\+|$)", part.split("x_dot = ")[1]):
            terms[NAMES.index(m.group(2).replace("*", " "))] = float(m.group(1))
        out.append(terms)
    return out


@pytest.mark.parametrize("eq", ["EQ_4_A", "EQ_4_B", "EQ_4_C", "EQ_4_D"])
def test_published_coefficients_inside_the_subdomain_spread(eq):
    """OLS of the weak regression on the published support, 16 subdomain draws (K = 100, p = 4, H = L / 20):
    every published seed-1 coefficient lies inside the [min, max] of the draws.  Pins the weak regression, not
    the optimiser."""
    pub = published(eq)
    assert len(pub) == 2 and all(len(t) >= 1 for t in pub)
    fits = [[], []]
    for seed in range(16):
        G, b = weak_system(eq, seed)
        for a in range(2):
            sup = np.zeros(EXPS.shape[0], dtype=bool)
            sup[list(pub[a])] = True
            fits[a].append(WR.ols_on_support(G[a], b[a], sup))
    for a in range(2):
        c = np.stack(fits[a])
        for j, v in pub[a].items():
            print(f"{eq} arm {a} {NAMES[j]}: published {v:.5f} in [{c[:, j].min():.5f}, {c[:, j].max():.5f}]")
            assert c[:, j].min() <= v <= c[:, j].max()


@pytest.mark.parametrize("seed", [0, 2])
def test_sr3_support_on_eq_4_a(seed):
    """SR3 (threshold 0.1, nu 1, tol 1e-1) on the weak Gram of EQ_4_A: the published support {x0 u0} / {x0 u1}
    on these two draws (not on every draw: DESIGN.md §9f)."""
    G, b = weak_system("EQ_4_A", seed)
    for a, name in ((0, "x0 u0"), (1, "x0 u1")):
        coef, sup, it, _ = WR.sr3(G[a], b[a], THRESHOLD)
        assert it > 0
        assert [NAMES[j] for j in np.nonzero(sup)[0]] == [name]
        assert abs(coef[NAMES.index(name)] + 1.0) < 0.05


def test_sr3_reports_a_singular_system():
    G = np.ones((3, 3))
    coef, sup, it, _ = WR.sr3(G, np.ones(3), 0.1)
    assert it == -1 and np.all(np.isnan(coef)) and not sup.any()
    coef, sup, it, _ = WR.sr3(np.zeros((3, 3)), np.zeros(3), 0.1)
    assert it == -1 and np.all(np.isnan(coef))


def test_float64_gram_against_longdouble():
    """Rounding of the float64 restatement on the EQ_4_C cohort (K = 100): error relative to the largest entry."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is float64 on this platform")
    x, u, arm, rows, T = cohort("EQ_4_C")
    H = WR.half_width(T, DT)
    c = np.random.default_rng(0).uniform(H, (T - 1) * DT - H, 100)
    W, D = WR.weights(T, DT, c)
    G, b = WR.gram(x, u, arm, rows, W, D, EXPS, 2)
    ld = np.longdouble
    Wl, Dl = WR.weights(T, DT, c, dtype=ld)
    Gl, bl = WR.gram(x.astype(ld), u.astype(ld), arm, rows, Wl, Dl, EXPS, 2)
    scale = max(np.abs(Gl).max(), np.abs(bl).max())
    err = float(max(np.abs(G - Gl).max(), np.abs(b - bl).max()) / scale)
    print(f"float64 vs longdouble weak Gram: {err:.3e} of the largest entry")
    RECORDED = 2.7e-15   # observed on the CPU (5e4 rows per arm summed in float64); the margin
    #                      below is for BLAS summation order
    assert err < 8 * RECORDED
