"""GPU tests of the regimen choice (include/insite_regimen.h: regimen_choice_kernel, ops.regimen_choice,
SINDY.choose_plan) against the numpy restatement tests/regimen_ref.py.

Tolerance: ``out`` within TOL s_p of the restatement, s_p = max_{r, j} (|cost_j| + sum_k |w[p, k]| |y_j[r, p, k]|) the
row's scale: the bar of tests/test_gpu_effect.py for this arithmetic (the objective adds at most T rounding steps to
the trajectory error, and every statistic is Lipschitz with constant <= 2 in the sup norm of the replicate values).
``choice`` and ``win`` are compared exactly: tests/test_regimen_abi.py asserts that every replicate's argmin in these
cases has a margin of at least 1e-8 s_p, a hundred times the bar.

Worst |got - ref| / s_p over the parity cases on an MI355X: 7.5e-15.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
import regimen_ref as G  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
DT, Q5, Q16 = G.DT, G.Q5, G.Q16


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(dev, name, y0, u, plans, w, cost, coef, q, method, sub, T, sense=1, pad_out=0):
    """(choice [N], win [N, K], out [N, K, 2, 3 + Q], the padding of out or None) as numpy arrays."""
    import torch
    from insite_amd import ops
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    N, K, NS = y0.shape[0], plans.shape[0], 3 + len(q)
    out = buf = None
    if pad_out:
        buf = torch.full((N, K * 2 * NS + pad_out), G.POISON, dtype=torch.float64, device=dev)
        out = buf[:, :K * 2 * NS].unflatten(1, (K, 2, NS))
    choice, win, got = ops.regimen_choice(t(y0), t(u), t(plans), t(coef), M.LIBS[name], DT, q, t(w), cost=t(cost),
                                          maximize=sense < 0, method=method, substeps=sub, drop_below=M.DROP_BELOW,
                                          T=T, out=out)
    torch.cuda.synchronize()
    if pad_out:
        assert got is out
    pad = None if buf is None else buf[:, K * 2 * NS:].cpu().numpy()
    return choice.cpu().numpy(), win.cpu().numpy(), got.cpu().numpy(), pad


def _worst(got, ref, scale):
    """max |got - ref| / s_p over the entries of out [N, K, 2, 3 + Q]; a NaN on one side only is inf."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(got - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(scale[:, None, None, None], got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_parity(dev, case):
    """choice and win equal the restatement exactly, out within the bar; the padding of out keeps its poison, the
    out-of-range arms and the NaN weights past T are never read, and the run on unpadded inputs is the padded run bit
    for bit."""
    Rn, N, T, A, K, name, method, sub, q, _, _, _, sense = case
    y0, u, plans, w, cost, coef, ref = G.case(*case)
    choice, win, out, pad = _run(dev, name, y0, u, plans, w, cost, coef, q, method, sub, T, sense, pad_out=G.PAD_OUT)
    assert out.shape == (N, K, 2, 3 + len(q)) and win.shape == (N, K) and choice.shape == (N,)
    assert np.all(pad == G.POISON)
    worst = _worst(out, ref["out"], ref["scale"])
    print(f"worst |got - ref| / s_p = {worst:.3e}")
    assert np.array_equal(choice, ref["choice"])
    assert np.array_equal(_bits(win), _bits(ref["win"]))
    assert worst <= TOL
    if Rn == 2:
        assert np.isnan(out[..., 2]).all()
    assert (out[:, :, 1, 0] >= 0).all() and (np.nan_to_num(out[:, :, 1, 3:], nan=0.0) >= 0).all()
    c2, w2, o2, _ = _run(dev, name, y0, u, plans[..., :T], w[..., :T], cost, coef, q, method, sub, T, sense)
    assert np.array_equal(c2, choice) and np.array_equal(_bits(w2), _bits(win)) and np.array_equal(_bits(o2), _bits(out))


EXACT = [(2, 3, 33, 2, 3, "std7"), (65, 3, 33, 4, 4, "lin3"), (130, 130, 18, 2, 3, "std7"),
         (300, 2, 33, 2, 8, "u3_first9")]


@functools.lru_cache(maxsize=None)
def _exact_inputs(Rn, N, T, A, K, name):
    out = G.inputs(("regimen-exact", Rn, N, T, A, K, name), Rn, N, T, A, K, name)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("Rn,N,T,A,K,name", EXACT)
def test_exact_properties(dev, Rn, N, T, A, K, name):
    y0, u, plans, w, cost, coef = _exact_inputs(Rn, N, T, A, K, name)
    run = functools.partial(_run, dev, name, y0, u)
    args = (Q5, "euler", 5, T)
    c0, w0, o0, _ = run(plans, w, cost, coef, *args)
    # two calls are bitwise equal
    c1, w1, o1, _ = run(plans, w, cost, coef, *args)
    assert np.array_equal(c0, c1) and np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(o0), _bits(o1))
    assert not np.isnan(np.delete(o0, 2, axis=-1)).any()
    # the last plan a copy of plan 0 (same cost): the same objective bit for bit, no vote, the same regret
    j2 = K - 1
    pd = plans.copy()
    pd[j2] = pd[0]
    cd = cost.copy()
    cd[j2] = cd[0]
    cc, wc, oc, _ = run(pd, w, cd, coef, *args)
    assert np.array_equal(_bits(oc[:, j2, 0]), _bits(oc[:, 0, 0]))
    assert np.all(wc[:, j2] == 0.0) and np.all(cc != j2)
    loc = [0, 1] + list(range(3, 3 + len(Q5)))
    assert np.array_equal(_bits(oc[:, j2, 1][:, loc]), _bits(oc[:, 0, 1][:, loc]))
    # every replicate equal to replicate 0: one winner with every vote, mean and quantiles are the point value bit
    # for bit, the standard deviation is 0 (NaN for R = 2)
    cf, wf, of, _ = run(plans, w, cost, np.broadcast_to(coef[:1], coef.shape), *args)
    assert np.array_equal(cf, c0) and np.all(wf[np.arange(N), cf] == 1.0) and np.all(wf.sum(axis=1) == 1.0)
    for st in loc[1:]:
        assert np.array_equal(_bits(of[..., st]), _bits(of[..., 0])), st
    assert np.isnan(of[..., 2]).all() if Rn == 2 else np.all(of[..., 2] == 0.0)
    assert np.array_equal(_bits(of[..., 0]), _bits(o0[..., 0]))
    # choice and the point values do not depend on R or q
    for r2, q2 in ((2, Q16), (min(Rn, 64), (0.3,)), (min(Rn, 129), Q16)):
        c2, _, o2, _ = run(plans, w, cost, coef[:r2], q2, "euler", 5, T)
        assert np.array_equal(c2, c0) and np.array_equal(_bits(o2[..., 0]), _bits(o0[..., 0])), r2
    # permuting the plans permutes the outputs (no ties here)
    perm = np.roll(np.arange(K), 1)
    cp, wp, op, _ = run(plans[perm], w, cost[perm], coef, *args)
    assert np.array_equal(perm[cp], c0) and np.array_equal(_bits(wp), _bits(w0[:, perm]))
    assert np.array_equal(_bits(op), _bits(o0[:, perm]))
    # maximise (w, cost) = minimise (-w, -cost): the same choice, votes and regret; the values negated
    cx, wx, ox, _ = run(plans, w, cost, coef, *args, sense=-1)
    cn, wn, on, _ = run(plans, -w, -cost, coef, *args, sense=1)
    assert np.array_equal(cx, cn) and np.array_equal(_bits(wx), _bits(wn))
    assert np.array_equal(_bits(ox[:, :, 1]), _bits(on[:, :, 1]))
    for st in (0, 1):
        assert np.array_equal(_bits(ox[:, :, 0, st]), _bits(-on[:, :, 0, st])), st
    assert np.array_equal(_bits(ox[:, :, 0, 2]), _bits(on[:, :, 0, 2]))
    assert np.array_equal(_bits(ox[:, :, 0, 3]), _bits(-on[:, :, 0, 4]))          # Q5: the minimum and the maximum
    # K = 1: the plan is chosen by every replicate and its regret is +0, under either sense
    for sense in (1, -1):
        c1, w1, o1, _ = run(plans[:1], w, cost[:1], coef, *args, sense=sense)
        assert np.all(c1 == 0) and np.all(w1 == 1.0)
        reg = np.delete(o1[:, 0, 1], 2, axis=-1)
        assert np.all(reg == 0.0) and not np.signbit(reg).any()
        assert np.isnan(o1[:, 0, 1, 2]).all() if Rn == 2 else np.all(_bits(o1[:, 0, 1, 2]) == 0)
        assert np.array_equal(_bits(o1[:, 0, 0]), _bits(o0[:, 0, 0]))


def test_known_answer(dev):
    """EQ_4's dynamics: arm a clears the state at the rate u_a (dx/dt = -x u_a), every replicate a positive multiple
    of that model.  Of the two constant plans the one with the larger clearance leaves the smaller terminal state in
    every replicate: choice = argmax(u[p]) with every vote."""
    rng = np.random.default_rng(7)
    Rn, N, T = 70, 37, 20
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, 2))
    base = np.zeros((2, 7))
    base[0, 4] = base[1, 5] = -1.0                      # std7: 1, x, u0, u1, x u0, x u1, u0 u1
    assert M.exps_of("std7")[4].tolist() == [1, 1, 0] and M.exps_of("std7")[5].tolist() == [1, 0, 1]
    coef = base[None] * rng.uniform(0.5, 1.5, (Rn, 1, 1))
    coef[0] = base
    plans = np.stack([np.zeros(T, dtype=np.int8), np.ones(T, dtype=np.int8)])
    w = np.zeros(T)
    w[T - 1] = 1.0
    for method, sub in (("euler", 5), ("rk4", 1)):
        choice, win, out, _ = _run(dev, "std7", y0, u, plans, w, None, coef, (0.5,), method, sub, T)
        best = np.argmax(u, axis=1)
        assert np.array_equal(choice, best)
        assert np.all(win[np.arange(N), best] == 1.0) and np.all(win[np.arange(N), 1 - best] == 0.0)
        assert np.all(out[np.arange(N), best, 1] == 0.0) and np.all(out[np.arange(N), 1 - best, 1, 0] > 0.0)
        want = y0[:, None] * np.exp(-u * T * DT)                        # the point model's terminal state
        assert np.allclose(out[:, :, 0, 0], want, rtol=0.06 if method == "euler" else 1e-4)


@pytest.mark.parametrize("Rn,N,T,A,K,name", [(17, 3, 18, 2, 3, "std7"), (130, 2, 33, 4, 4, "lin3")])
def test_nan_replicates(dev, Rn, N, T, A, K, name):
    y0, u, plans, w, cost, coef = _exact_inputs(Rn, N, T, A, K, name)
    exps = M.exps_of(name)
    run = functools.partial(_run, dev, name, y0, u)
    args = (Q5, "rk4", 1, T)
    c0, w0, o0, _ = run(plans, w, cost, coef, *args)
    assert not np.isnan(o0).any() and np.all(np.abs(w0.sum(axis=1) - 1.0) <= 4e-16)

    def ref_of(pl, cf):
        return G.regimen(y0, u, G.full_plans(pl, N, T), cf, exps, DT, Q5, w[..., :T], cost, 1, "rk4", 1)

    # a resampled replicate with NaN coefficients abstains: its vote is nobody's, every statistic but the point is NaN
    c1 = coef.copy()
    c1[Rn - 2] = np.nan
    cg, wg, og, _ = run(plans, w, cost, c1, *args)
    ref = ref_of(plans, c1)
    assert np.array_equal(cg, c0) and np.array_equal(_bits(wg), _bits(ref["win"]))
    assert np.allclose(wg.sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=4e-16)
    assert np.isnan(og[..., 1:]).all() and np.array_equal(_bits(og[..., 0]), _bits(o0[..., 0]))
    # replicate 0 NaN: no choice and NaN point values, the votes and the other statistics intact
    cz = coef.copy()
    cz[0] = np.nan
    cg, wg, og, _ = run(plans, w, cost, cz, *args)
    assert np.all(cg == -1) and np.isnan(og[..., 0]).all()
    assert np.array_equal(_bits(wg), _bits(w0)) and np.array_equal(_bits(og[..., 1:]), _bits(o0[..., 1:]))
    # NaN in one coefficient of arm 1 of one replicate, and plan 0 never uses arm 1 (the others start with it): plan
    # 0's value statistics stay finite, the replicate abstains, so every regret statistic but the point is NaN
    ca = coef.copy()
    ca[Rn - 2, 1, 1] = np.nan
    pa = plans.copy()
    pa[0] = 0
    pa[1:, ..., 0] = 1
    cg, wg, og, _ = run(pa, w, cost, ca, *args)
    ref = ref_of(pa, ca)
    assert np.isfinite(og[:, 0, 0]).all() and np.isnan(og[:, 1:, 0, 1:]).all() and np.isnan(og[:, :, 1, 1:]).all()
    assert np.isfinite(og[..., 0]).all()
    assert np.array_equal(cg, ref["choice"]) and np.array_equal(_bits(wg), _bits(ref["win"]))
    assert _worst(og, ref["out"], ref["scale"]) <= TOL
    # a NaN in y reaches J under weight 0: arm 1 is used at the last step only, and the weight is 0 there
    wz = np.array(w)
    wz[..., T - 1] = 0.0
    pz = np.zeros_like(pa)
    pz[1:, ..., T - 1] = 1
    _, _, og, _ = run(pz, wz, cost, ca, *args)
    assert np.isfinite(og[:, 0, 0]).all() and np.isnan(og[:, 1:, 0, 1:]).all()


def test_plan_and_out(dev):
    """``plan_regimen_choice`` writes into the caller's out and repeats bit for bit; shape and argument errors."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, name = 65, 3, 33, 4, 4, "lin3"
    y0, u, plans, w, cost, coef = _exact_inputs(Rn, N, T, A, K, name)
    c0, w0, o0, _ = _run(dev, name, y0, u, plans, w, cost, coef, Q5, "euler", 5, T)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    lib = M.LIBS[name]
    out = torch.zeros((N, K, 2, 3 + len(Q5)), dtype=torch.float64, device=dev)
    ty0, tu, tp, tw, tc, tcoef = t(y0), t(u), t(plans), t(w), t(cost), t(coef)
    plan = ops.plan_regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw, cost=tc, method="euler", substeps=5,
                                   drop_below=M.DROP_BELOW, T=T, out=out)
    for _ in range(2):
        choice, win, got = plan()
        assert got is out and plan.out[2] is out
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(o0))
        assert np.array_equal(choice.cpu().numpy(), c0) and np.array_equal(_bits(win.cpu().numpy()), _bits(w0))
        out.zero_()
    kw = dict(cost=tc, T=T)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, (0.5, 1.5), tw, **kw)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp[:, :2], tcoef, lib, DT, Q5, tw, **kw)                 # rows of the plans
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp.repeat(5, 1, 1), tcoef, lib, DT, Q5, tw, T=T)         # 20 plans
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef[:1], lib, DT, Q5, tw, **kw)                    # no resample
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw[:2], **kw)                    # rows of the weights
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw[:, :T - 1], **kw)             # fewer than T weights
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw, cost=tc[:2], T=T)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw, out=out[:, :2], **kw)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw, T=T + 10, cost=tc)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp.to(torch.int32), tcoef, lib, DT, Q5, tw, **kw)
    with pytest.raises(ValueError):
        ops.regimen_choice(ty0, tu, tp, tcoef, lib, DT, Q5, tw, method="heun", **kw)


def test_no_rows(dev):
    """n_rows = 0 is a successful no-op with empty outputs, in both plan forms."""
    Rn, N, T, A, K, name = 65, 3, 33, 4, 4, "lin3"
    y0, u, plans, w, cost, coef = _exact_inputs(Rn, N, T, A, K, name)
    for pl, ww in ((plans[:, :0], w[:0]), (plans[:, 0], w[0])):
        choice, win, out, _ = _run(dev, name, y0[:0], u[:0], pl, ww, cost, coef, Q5, "euler", 5, T)
        assert choice.shape == (0,) and win.shape == (0, K) and out.shape == (0, K, 2, 3 + len(Q5))


# ---------------------------------------------------------------------------------------------------
# plugin
# ---------------------------------------------------------------------------------------------------
OV = ["+backbone=sindy", "+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A",
      "model.sindy_threshold=0.1", "model.sindy_alpha=0.5"]


@functools.lru_cache(maxsize=None)
def _train():
    return RC.make_collection("EQ_4_A", {"train": 200, "val": 10, "test": 4}, with_tests=False)["train"]


@pytest.fixture(scope="module")
def model(dev):
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    tr = _train()
    m = SINDY(C.compose(OV), device=dev).fit(tr)
    m.bootstrap(tr, n_replicates=33, seed=3)
    return m


def _stack(res):
    """[2, 3 + Q, N, K] of a RegimenChoiceResult."""
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def test_plugin_choose_plan(dev, model):
    """``choose_plan([None, 0, 1])`` is ``ops.regimen_choice`` on the plugin's inputs after the stated unit change:
    value = (J - mean sum_k w) / std with the costs passed as cost std, the regret divided by std only."""
    import torch
    from insite_amd import ops
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    costs = [0.0, 0.02, -0.01]
    res = model.choose_plan(tr, [None, 0, 1], objective="mean", costs=costs)
    assert res.series == ("value", "regret") and res.q == q
    prev, stat, _, _ = model._unscaled_inputs(tr)
    arms = np.argmax(tr.data["current_treatments"], axis=-1).astype(np.int8)
    N, T = arms.shape
    plans = np.stack([arms, np.zeros_like(arms), np.ones_like(arms)])
    ae = tr.data["active_entries"][..., 0].astype(np.float64)
    w = ae / ae.sum(axis=1, keepdims=True)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)   # noqa: E731
    choice, win, out = ops.regimen_choice(prev[:, 0].contiguous(), stat, t(plans), t(coef), model.library, model.dt, q,
                                          t(w), cost=t(np.array(costs) * std), method=model.integrator,
                                          drop_below=0.0, T=T)
    torch.cuda.synchronize()
    assert np.array_equal(res.choice.cpu().numpy(), choice.cpu().numpy())
    assert np.array_equal(_bits(res.win.cpu().numpy()), _bits(win.cpu().numpy()))
    assert res.win.shape == (N, 3) and res.point.shape == (2, N, 3) and res.quantiles.shape == (2, 3, N, 3)
    o = out.cpu().numpy().transpose(2, 3, 0, 1)                   # [2, 3 + Q, N, K]
    want = o / std
    want[0, [0, 1, 3, 4, 5]] = (o[0, [0, 1, 3, 4, 5]] - mean * w.sum(axis=1)[None, :, None]) / std
    assert np.allclose(_stack(res), want, rtol=1e-13, atol=1e-13)
    # against the restatement, in standardised units
    ref = G.regimen(prev[:, 0].cpu().numpy(), stat.cpu().numpy(), plans, coef, R.poly_library(3, 2, True), model.dt, q,
                    w, np.array(costs) * std, 1, "euler5")
    assert np.array_equal(choice.cpu().numpy(), ref["choice"])
    worst = _worst(out.cpu().numpy(), ref["out"], ref["scale"])
    print(f"worst |got - ref| / s_p = {worst:.3e}")
    assert worst <= TOL
    # the plan forms and the refusals of the arguments
    one_hot = model.choose_plan(tr, [np.eye(2)[arms.astype(np.int64)], np.zeros((N, T), dtype=np.int64), 1],
                                costs=costs)
    assert np.array_equal(_bits(_stack(one_hot)), _bits(_stack(res)))
    with pytest.raises(ValueError):
        model.choose_plan(tr, [0, 2])
    with pytest.raises(ValueError):
        model.choose_plan(tr, [0, 1], objective="median")
    with pytest.raises(ValueError):
        model.choose_plan(tr, [0, 1], objective=np.ones(T + 1))


def test_plugin_terminal_value_is_the_effect_series(dev, model):
    """Under ``objective="terminal"`` the value of plan j is the "a" series of ``treatment_effect(plan_a=j)`` at the
    row's last active step, and with two plans the regret of the point model's losing plan is |effect| there."""
    tr = _train()
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    ae = tr.data["active_entries"][..., 0]
    N, T = ae.shape
    last = T - 1 - np.argmax(ae[:, ::-1] > 0, axis=1)
    rows = np.arange(N)
    res = model.choose_plan(tr, [0, 1], objective="terminal")
    te = model.treatment_effect(tr, plan_b=1, plan_a=0)
    s = (np.abs(te.point[:2].cpu().numpy() * std + mean).max() + abs(mean)) / std     # the scale, standardised
    for j, name in enumerate(("a", "b")):
        for field in ("point", "mean"):
            want = te[name][field].cpu().numpy()[rows, last]
            got = res["value"][field].cpu().numpy()[:, j]
            assert np.max(np.abs(got - want)) <= TOL * s, (name, field)
    eff = te["effect"]["point"].cpu().numpy()[rows, last]
    choice = res.choice.cpu().numpy()
    assert np.array_equal(choice, (eff > 0).astype(np.int32))         # a - b > 0: plan b is the smaller
    reg = res["regret"]["point"].cpu().numpy()
    assert np.all(reg[rows, choice] == 0.0)
    assert np.max(np.abs(reg[rows, 1 - choice] - np.abs(eff))) <= TOL * s
    assert np.all((res.win.cpu().numpy().sum(axis=1) - 1.0) == 0.0)
