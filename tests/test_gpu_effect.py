"""GPU tests of the paired treatment-effect bands (include/insite_effect.h: effect_bands_kernel, ops.effect_bands,
SINDY.predict_bands / treatment_effect) against the numpy restatement tests/effect_ref.py.

Tolerance: every output within TOL s of the restatement, s the largest |yA| or |yB| over the replicates at that
(row, step): ten times the project's 1e-11 rollout bar, because each statistic (order statistic, interpolation,
difference, mean, two-pass standard deviation) is Lipschitz with constant <= 2 in the sup norm of the replicate
values.  A scale-relative absolute bar: A - B and the standard deviation cancel.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
DT = 0.1
Q5 = (0.0, 1.0, 0.5, 0.025, 0.5)                     # unsorted, with a repeat
Q16 = tuple(np.linspace(0.0, 1.0, 16)[[3, 0, 15, 7, 1, 14, 2, 13, 4, 12, 5, 11, 6, 10, 8, 9]])
PAD_ARM, PAD_OUT, POISON = 3, 5, -7.25

# a sample of R x N x T x n_arms x table x method x substeps x quantiles (not the product): every V (R <= 64, 128,
# 256, 512), partly filled top slots (65, 129, 200), n = 1 (R = 2), every table of tests/library_matrix.py, both
# methods, substeps 1 and 5, T below, at and across the 16-step staging chunk, one row to three waves' worth of rows
CASES = [
    (2, 3, 1, 1, "x_only", "euler", 1, Q5),
    (3, 1, 2, 2, "bias_x", "rk4", 1, Q5),
    (17, 130, 31, 2, "std7", "euler", 5, Q5),
    (64, 3, 33, 4, "noone3", "rk4", 5, Q16),
    (65, 3, 70, 2, "lin3", "euler", 5, Q5),
    (128, 130, 2, 1, "dup4", "rk4", 1, Q5),
    (129, 3, 33, 4, "u3_first9", "euler", 1, Q16),
    (200, 3, 70, 2, "std7", "rk4", 1, Q5),
    (256, 130, 33, 2, "high_pow", "euler", 5, Q5),
    (512, 3, 31, 2, "u3_x9", "rk4", 5, Q5),
    (512, 1, 70, 4, "deg2_no_xx", "euler", 5, Q16),
    (33, 3, 33, 2, "u3_mixed9", "rk4", 1, Q5),
    (2, 130, 33, 4, "std7", "euler", 5, Q16),
]


def _plans(rng, N, T, A):
    """Per-step arms [N, T + PAD_ARM] of two plans: random, with a switch at step 1 and at step T - 1 in every row
    (and rows that start on different arms); the columns past T hold out-of-range arms."""
    out = []
    for _ in range(2):
        arm = rng.integers(0, A, (N, T + PAD_ARM))
        if A > 1 and T >= 2:
            arm[:, 1] = (arm[:, 0] + 1) % A
            arm[:, T - 1] = (arm[:, T - 2] + 1) % A
        arm[:, T:] = [A + 3, -2, 127][:PAD_ARM]
        out.append(arm.astype(np.int8))
    return out


def _coef(rng, name, Rn, A):
    """[R, A, F]: a decaying model (state-exponent-1 terms negative, the others of either sign, |c| in
    [0.05, 0.15]) and bootstrap-like replicates of it: every coefficient scaled by 1 + 0.3 z, one term in five
    outside the replicate's support, and the last column of the last arm below drop_below in replicate 1.  The
    perturbation is of the size of the differences between rows, so the replicates' trajectories cross."""
    exps = M.exps_of(name)
    F = exps.shape[0]
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[rng.random((Rn, A, F)) < 0.2] = 0.0
    coef[0] = base
    coef[1, A - 1, F - 1] = 0.5 * M.DROP_BELOW
    return coef


@functools.lru_cache(maxsize=None)
def _case(Rn, N, T, A, name, method, sub, q):
    rng = np.random.default_rng(M._seed("effect", Rn, N, T, A, name, method, sub))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    arm_a, arm_b = _plans(rng, N, T, A)
    coef = _coef(rng, name, Rn, A)
    ref, scale = E.bands(y0, u, arm_a[:, :T], arm_b[:, :T], coef, M.exps_of(name), DT, q, method, sub)
    out = (y0, u, arm_a, arm_b, coef, ref, scale)
    for a in out:
        a.setflags(write=False)
    return out


def _run(dev, name, y0, u, arm_a, arm_b, coef, q, method, sub, T, pad=0, **kw):
    import torch
    from insite_amd import ops
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    N = y0.shape[0]
    out = None
    if pad:
        S = 1 if arm_b is None else 3
        out = torch.full((S, 3 + len(q), N, T + pad), POISON, dtype=torch.float64, device=dev)
    got = ops.effect_bands(t(y0), t(u), t(arm_a), None if arm_b is None else t(arm_b), t(coef), M.LIBS[name], DT, q,
                           method=method, substeps=sub, drop_below=M.DROP_BELOW, T=T, out=out, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _worst(got, ref, scale):
    """max |got - ref| / scale over the entries; a NaN on one side only, or an entry off where the scale is 0, is inf."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(got - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(scale, got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("Rn,N,T,A,name,method,sub,q", CASES,
                         ids=[f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-{c[4]}-{c[5]}{c[6]}-Q{len(c[7])}" for c in CASES])
def test_parity(dev, Rn, N, T, A, name, method, sub, q):
    """Three series against the restatement; the padding of out keeps its poison, the out-of-range arms past T are
    never read (they would select another arm), and the run without plan B is series A bit for bit."""
    y0, u, arm_a, arm_b, coef, ref, scale = _case(Rn, N, T, A, name, method, sub, q)
    full = _run(dev, name, y0, u, arm_a, arm_b, coef, q, method, sub, T, pad=PAD_OUT)
    assert full.shape == (3, 3 + len(q), N, T + PAD_OUT)
    assert np.all(full[..., T:] == POISON)
    got = full[..., :T]
    w = _worst(got, ref, scale)
    print(f"worst |got - ref| / s = {w:.3e}")
    assert w <= TOL
    if Rn == 2:
        assert np.isnan(got[:, 2]).all()
    exact = _run(dev, name, y0, u, arm_a[:, :T], arm_b[:, :T], coef, q, method, sub, T)
    assert np.array_equal(_bits(exact), _bits(got))
    only_a = _run(dev, name, y0, u, arm_a, None, coef, q, method, sub, T)
    assert only_a.shape == (1, 3 + len(q), N, T) and np.array_equal(_bits(only_a[0]), _bits(got[0]))


EXACT = [(2, 3, 33, 2, "std7"), (65, 3, 33, 4, "lin3"), (130, 130, 18, 2, "std7"), (300, 2, 33, 2, "u3_first9")]


@pytest.mark.parametrize("Rn,N,T,A,name", EXACT)
def test_exact_properties(dev, Rn, N, T, A, name):
    y0, u, arm_a, arm_b, coef, _, _ = _case(Rn, N, T, A, name, "euler", 5, Q5)
    run = functools.partial(_run, dev, name, y0, u)
    base = run(arm_a, arm_b, coef, Q5, "euler", 5, T)
    # two calls are bitwise equal
    assert np.array_equal(_bits(base), _bits(run(arm_a, arm_b, coef, Q5, "euler", 5, T)))
    # plan B = plan A: the effect is exactly zero in every statistic; its std is 0 too, NaN only for R = 2
    same = run(arm_a, arm_a, coef, Q5, "euler", 5, T)
    assert np.array_equal(_bits(same[0]), _bits(same[1])) and np.array_equal(_bits(same[0]), _bits(base[0]))
    eff = np.delete(same[2], 2, axis=0)
    assert np.all(eff == 0.0)
    assert np.isnan(same[2, 2]).all() if Rn == 2 else np.all(same[2, 2] == 0.0)
    # every replicate equal to replicate 0: mean and quantiles are the point row bit for bit, std is 0
    flat = run(arm_a, arm_b, np.broadcast_to(coef[:1], coef.shape), Q5, "euler", 5, T)
    for s in range(3):
        for st in [1] + list(range(3, 3 + len(Q5))):
            assert np.array_equal(_bits(flat[s, st]), _bits(flat[s, 0])), (s, st)
        assert np.isnan(flat[s, 2]).all() if Rn == 2 else np.all(flat[s, 2] == 0.0)
    assert np.array_equal(_bits(flat[:, 0]), _bits(base[:, 0]))
    # the point rows do not depend on R or q
    for r2, q2 in ((2, Q16), (min(Rn, 64), (0.3,)), (min(Rn, 129), Q16)):
        other = run(arm_a, arm_b, coef[:r2], q2, "euler", 5, T)
        assert np.array_equal(_bits(other[:, 0]), _bits(base[:, 0])), r2


def test_plan_and_out(dev):
    """``plan_effect_bands`` writes into the caller's out and repeats bit for bit."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, name = 65, 3, 33, 4, "lin3"
    y0, u, arm_a, arm_b, coef, _, _ = _case(Rn, N, T, A, name, "euler", 5, Q5)
    base = _run(dev, name, y0, u, arm_a, arm_b, coef, Q5, "euler", 5, T)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    out = torch.zeros((3, 3 + len(Q5), N, T), dtype=torch.float64, device=dev)
    plan = ops.plan_effect_bands(t(y0), t(u), t(arm_a), t(arm_b), t(coef), M.LIBS[name], DT, Q5, method="euler",
                                 substeps=5, drop_below=M.DROP_BELOW, T=T, out=out)
    for _ in range(2):
        assert plan() is out
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(base))
    with pytest.raises(ValueError):
        ops.effect_bands(t(y0), t(u), t(arm_a), t(arm_b), t(coef), M.LIBS[name], DT, (0.5, 1.5), T=T)
    with pytest.raises(ValueError):
        ops.effect_bands(t(y0), t(u), t(arm_a), t(arm_b[:2]), t(coef), M.LIBS[name], DT, Q5, T=T)
    with pytest.raises(ValueError):
        ops.effect_bands(t(y0), t(u), t(arm_a), t(arm_b), t(coef[:1]), M.LIBS[name], DT, Q5, T=T)


@pytest.mark.parametrize("Rn,N,T,A,name", [(17, 3, 18, 2, "std7"), (130, 2, 33, 4, "lin3")])
def test_nan_replicates(dev, Rn, N, T, A, name):
    y0, u, arm_a, arm_b, coef, _, _ = _case(Rn, N, T, A, name, "rk4", 1, Q5)
    exps = M.exps_of(name)
    base = _run(dev, name, y0, u, arm_a, arm_b, coef, Q5, "rk4", 1, T)
    assert not np.isnan(base).any()
    # a resampled replicate with NaN coefficients: every statistic but the point row is NaN at every (p, k)
    c1 = coef.copy()
    c1[Rn - 2] = np.nan
    got = _run(dev, name, y0, u, arm_a, arm_b, c1, Q5, "rk4", 1, T)
    assert np.isnan(got[:, 1:]).all()
    assert np.array_equal(_bits(got[:, 0]), _bits(base[:, 0]))
    ref, scale = E.bands(y0, u, arm_a[:, :T], arm_b[:, :T], c1, exps, DT, Q5, "rk4", 1)
    assert _worst(got, ref, scale) <= TOL
    # replicate 0 NaN instead: only the point rows are NaN
    c0 = coef.copy()
    c0[0] = np.nan
    got = _run(dev, name, y0, u, arm_a, arm_b, c0, Q5, "rk4", 1, T)
    assert np.isnan(got[:, 0]).all() and not np.isnan(got[:, 1:]).any()
    assert np.array_equal(_bits(got[:, 1:]), _bits(base[:, 1:]))


# ---------------------------------------------------------------------------------------------------
# plugin
# ---------------------------------------------------------------------------------------------------
OV = ["+backbone=sindy", "+dataset=pkpd_sim", "dataset.equation_str=EQ_4_D", "model.dataset_name=EQ_4_D",
      "model.sindy_threshold=0.1", "model.sindy_alpha=0.5"]


@functools.lru_cache(maxsize=None)
def _train():
    return RC.make_collection("EQ_4_D", {"train": 200, "val": 10, "test": 4}, with_tests=False)["train"]


@pytest.fixture(scope="module")
def model(dev):
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    tr = _train()
    m = SINDY(C.compose(OV), device=dev).fit(tr)
    m.bootstrap(tr, n_replicates=33, seed=3)
    return m


def test_plugin_predict_bands(dev, model):
    """Every row of the dataset: the rows of ``predict_interval(ds, max_rows=None)``, its replicate 0 and the
    moments of its replicates, within the bar (in the standardised scale of both)."""
    tr = _train()
    q = (0.025, 0.975)
    band, y = model.predict_interval(tr, quantiles=q, max_rows=None, return_replicates=True)
    res = model.predict_bands(tr, quantiles=q)
    assert res.series == ("a",) and res.q == q
    y = y.cpu().numpy()                                           # [N, R, T]
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    s = np.abs(y * std + mean).max(axis=1) / std                  # the largest |yA|, in standardised units
    N, T = s.shape
    assert res.point.shape == (1, N, T) and res.quantiles.shape == (1, 2, N, T)
    assert _worst(res.quantiles[0].cpu().numpy(), band.cpu().numpy(), s) <= TOL
    assert _worst(res.point[0].cpu().numpy(), y[:, 0], s) <= TOL
    assert _worst(res.mean[0].cpu().numpy(), y[:, 1:].mean(axis=1), s) <= TOL
    assert _worst(res.std[0].cpu().numpy(), y[:, 1:].std(axis=1, ddof=1), s) <= TOL


def test_plugin_treatment_effect(dev, model):
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    prev, stat = R.unscale_inputs(tr.data, tr.scaling_params)
    arms = np.argmax(tr.data["current_treatments"], axis=-1)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    ref, scale = E.bands(prev[:, 0], stat, arms, np.zeros_like(arms), coef, R.poly_library(3, 2, True), model.dt, q,
                         "euler5")
    res = model.treatment_effect(tr, plan_b=0)
    assert res.series == ("a", "b", "effect") and res.q == q
    got = np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                          res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)
    want = ref / std
    want[:2, [0, 1, 3, 4, 5]] = (ref[:2, [0, 1, 3, 4, 5]] - mean) / std
    w = _worst(got, want, scale / std)                            # the bar in standardised units
    print(f"worst |got - ref| / s = {w:.3e}")
    assert w <= TOL
    # the plan forms: an int array and a one-hot array of plan B = arm 0 are the int's result
    N, T = arms.shape
    A = tr.data["current_treatments"].shape[-1]
    as_int = model.treatment_effect(tr, plan_b=np.zeros((N, T), dtype=np.int64), plan_a=arms)
    one_hot = model.treatment_effect(tr, plan_b=np.eye(A)[np.zeros((N, T), dtype=np.int64)])
    for other in (as_int, one_hot):
        assert np.array_equal(_bits(other.quantiles.cpu().numpy()), _bits(res.quantiles.cpu().numpy()))
    # plan B = the dataset's own treatments: identically zero
    zero = model.treatment_effect(tr, plan_b=None)
    for t in (zero.point, zero.mean, zero.std, zero.quantiles):
        assert bool((t[2] == 0.0).all())
    assert np.array_equal(_bits(zero.point[0].cpu().numpy()), _bits(zero.point[1].cpu().numpy()))
    with pytest.raises(ValueError):
        model.treatment_effect(tr, plan_b=A)
    with pytest.raises(ValueError):
        model.treatment_effect(tr, plan_b=np.zeros((N, T + 1), dtype=np.int64))
