"""GPU tests of the closed-loop rules (include/insite_feedback.h: feedback_rules_kernel, ops.feedback_rules,
SINDY.evaluate_rules) against the numpy restatement tests/feedback_ref.py.

Tolerance: the J and regret statistics within TOL s_p of the restatement, s_p = max_{r, j} (|cost_j| + sum_k |w[p, k]|
|y[r, p, j, k]|) + sum_a |arm_cost_a| the row's scale: the bar of tests/test_gpu_regimen.py for this arithmetic.  The
exposure mean, standard deviation and quantiles within TOL T (a count of at most T steps).  ``choice``, ``win``,
``sched`` and the exposure point values are compared exactly: tests/test_feedback_abi.py asserts that every decision
and every replicate's argmin in these cases has a margin of at least 1e-8, a hundred times the bar.

Worst |got - ref| / s_p over the parity cases on an MI355X: 9.5e-15; worst exposure statistic: 1.4e-15 T (DESIGN.md
§9m).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_ref as F  # noqa: E402
import library_matrix as M  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
DT, Q5, Q16 = F.DT, F.Q5, F.Q16


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _run(dev, name, y0, u, theta, rules, w, cost, ac, coef, q, method, sub, T, sense=1, pad_out=0, sched=True,
         pad_sched=0):
    """(choice [N], win [N, K], out [N, K, 3, 3 + Q], sched [N, K, T] or None, the padding of out or None, the padding
    of sched or None) as numpy arrays."""
    import torch
    from insite_amd import ops
    N, K, NS = y0.shape[0], len(rules), 3 + len(q)
    out = buf = sbuf = None
    if pad_out:
        buf = torch.full((N, K * 3 * NS + pad_out), F.POISON, dtype=torch.float64, device=dev)
        out = buf[:, :K * 3 * NS].unflatten(1, (K, 3, NS))
    if pad_sched:
        sbuf = torch.full((N, K * T + pad_sched), F.POISON_I8, dtype=torch.int8, device=dev)
        sched = sbuf[:, :K * T].unflatten(1, (K, T))
    choice, win, got, sc = ops.feedback_rules(_t(dev, y0), _t(dev, u), _t(dev, theta), rules, _t(dev, coef),
                                              M.LIBS[name], DT, q, _t(dev, w), cost=_t(dev, cost), arm_cost=ac,
                                              maximize=sense < 0, method=method, substeps=sub,
                                              drop_below=M.DROP_BELOW, T=T, out=out, sched=sched)
    torch.cuda.synchronize()
    if pad_out:
        assert got is out
    pad = None if buf is None else buf[:, K * 3 * NS:].cpu().numpy()
    spad = None if sbuf is None else sbuf[:, K * T:].cpu().numpy()
    return (choice.cpu().numpy(), win.cpu().numpy(), got.cpu().numpy(), None if sc is None else sc.cpu().numpy(), pad,
            spad)


def _worst(got, ref, scale):
    """max |got - ref| / scale over the entries of [N, K, S, 3 + Q]; scale [N] or a number; a NaN on one side only is
    inf."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(got - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1, 1), got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("case", F.CASES, ids=F.CASE_IDS)
def test_parity(dev, case):
    """choice, win, sched and the exposure point values equal the restatement exactly, the statistics within the bar;
    the padding of out and sched keeps its poison, the NaN padding of theta and w is never read, and the run on
    unpadded inputs is the padded run bit for bit."""
    Rn, N, T, A, K, name, method, sub, q, _, _, _, _, sense, _ = case
    y0, u, theta, rules, w, cost, ac, coef, ref = F.case(*case)
    choice, win, out, sched, pad, spad = _run(dev, name, y0, u, theta, rules, w, cost, ac, coef, q, method, sub, T,
                                              sense, pad_out=F.PAD_OUT, pad_sched=F.PAD_SCHED)
    assert out.shape == (N, K, 3, 3 + len(q)) and win.shape == (N, K) and choice.shape == (N,)
    assert sched.shape == (N, K, T)
    assert np.all(pad == F.POISON) and np.all(spad == F.POISON_I8)
    worst = _worst(out[:, :, :2], ref["out"][:, :, :2], ref["scale"])
    worst_e = _worst(out[:, :, 2:], ref["out"][:, :, 2:], float(T))
    print(f"worst |got - ref| / s_p = {worst:.3e}; exposure statistics: worst |got - ref| / T = {worst_e:.3e}")
    assert np.array_equal(choice, ref["choice"])
    assert np.array_equal(_bits(win), _bits(ref["win"]))
    assert np.array_equal(sched, ref["sched"])
    assert np.array_equal(_bits(out[:, :, 2, 0]), _bits(ref["out"][:, :, 2, 0]))
    assert worst <= TOL
    assert worst_e <= TOL
    if Rn == 2:
        assert np.isnan(out[..., 2]).all()
    assert (out[:, :, 1, 0] >= 0).all() and (np.nan_to_num(out[:, :, 1, 3:], nan=0.0) >= 0).all()
    th2 = theta if theta.shape == (K, 2) and theta.shape[0] != N else theta[:, :2 * K]
    c2, w2, o2, s2, _, _ = _run(dev, name, y0, u, th2, rules, w[..., :T], cost, ac, coef, q, method, sub, T, sense)
    assert np.array_equal(c2, choice) and np.array_equal(_bits(w2), _bits(win)) and np.array_equal(_bits(o2), _bits(out))
    assert np.array_equal(s2, sched)


EXACT = [(2, 3, 33, 2, 3, "std7"), (65, 3, 33, 4, 4, "lin3"), (130, 130, 18, 2, 3, "std7"),
         (300, 2, 33, 2, 8, "u3_first9")]


@functools.lru_cache(maxsize=None)
def _exact_inputs(Rn, N, T, A, K, name):
    out = F.inputs(("feedback-exact", Rn, N, T, A, K, name), Rn, N, T, A, K, name)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _regimen(dev, name, y0, u, plans, w, cost, coef, q, method, sub, T):
    import torch
    from insite_amd import ops
    choice, win, out = ops.regimen_choice(_t(dev, y0), _t(dev, u), _t(dev, plans), _t(dev, coef), M.LIBS[name], DT, q,
                                          _t(dev, w), cost=_t(dev, cost), method=method, substeps=sub,
                                          drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    return choice.cpu().numpy(), win.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("Rn,N,T,A,K,name", EXACT)
def test_exact_anchors(dev, Rn, N, T, A, K, name):
    """All bitwise, with arm_cost NULL."""
    y0, u, theta, rules, w, cost, _, coef = _exact_inputs(Rn, N, T, A, K, name)
    theta = theta[:, :2 * K]
    w = w[..., :T]
    run = functools.partial(_run, dev, name, y0, u)
    args = (Q5, "euler", 5, T)
    loc = [0, 1] + list(range(3, 3 + len(Q5)))
    c0, w0, o0, s0, _, _ = run(theta, rules, w, cost, None, coef, *args)
    # two calls are bitwise equal; the schedule is optional and changes nothing else
    c1, w1, o1, s1, _, _ = run(theta, rules, w, cost, None, coef, *args, sched=None)
    assert s1 is None
    assert np.array_equal(c0, c1) and np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(o0), _bits(o1))
    c1, w1, o1, s1, _, _ = run(theta, rules, w, cost, None, coef, *args)
    assert np.array_equal(c0, c1) and np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(o0), _bits(o1))
    assert np.array_equal(s0, s1)
    assert not np.isnan(np.delete(o0, 2, axis=-1)).any()
    # theta = -Inf: ops.regimen_choice under the constant plans arm_on; +Inf with start_on = 0: under arm_off
    for th, col, expo in ((-np.inf, 0, float(T)), (np.inf, 1, 0.0)):
        rl = rules.copy()
        rl[:, 3] = 0
        cf, wf, of, sf, _, _ = run(np.full((K, 2), th), rl, w, cost, None, coef, *args)
        plans = np.ascontiguousarray(np.broadcast_to(rl[:, col][:, None], (K, T)).astype(np.int8))
        cr, wr, orr = _regimen(dev, name, y0, u, plans, w, cost, coef, *args)
        assert np.array_equal(cf, cr) and np.array_equal(_bits(wf), _bits(wr))
        assert np.array_equal(_bits(of[:, :, :2]), _bits(orr))
        assert np.all(of[:, :, 2][..., loc] == expo)
        assert np.isnan(of[:, :, 2, 2]).all() if Rn == 2 else np.all(_bits(of[:, :, 2, 2]) == 0)
        assert np.array_equal(sf, np.broadcast_to(plans[None], (N, K, T)))
    # period >= T: decided once, on y0: exposure 0 or T per row, the same in every replicate
    rl = rules.copy()
    rl[:, 2] = T + np.arange(K)
    _, _, op, sp, _, _ = run(theta, rl, w, cost, None, coef, *args)
    want = np.where(y0[:, None] >= np.where(rl[:, 3] == 1, theta[:, 1::2], theta[:, 0::2]), float(T), 0.0)
    for st in loc:
        assert np.array_equal(_bits(op[:, :, 2, st]), _bits(want)), st
    assert np.isnan(op[:, :, 2, 2]).all() if Rn == 2 else np.all(_bits(op[:, :, 2, 2]) == 0)
    assert np.all((sp == rl[None, :, 0, None]) == (want[:, :, None] == T))
    # the point model's schedule fed back to ops.regimen_choice as per-row plans reproduces the point value of J
    plans = np.ascontiguousarray(s0.transpose(1, 0, 2))
    _, _, orr = _regimen(dev, name, y0, u, plans, w, cost, coef, *args)
    assert np.array_equal(_bits(orr[:, :, 0, 0]), _bits(o0[:, :, 0, 0]))
    assert np.array_equal(o0[:, :, 2, 0], (s0 == rules[None, :, 0, None]).sum(axis=2))
    # a shard of the rows equals the same rows of the whole
    lo = N // 3
    cs, ws, os_, ss, _, _ = _run(dev, name, y0[lo:], u[lo:], theta[lo:], rules, w[lo:], cost, None, coef, *args)
    assert np.array_equal(cs, c0[lo:]) and np.array_equal(_bits(ws), _bits(w0[lo:]))
    assert np.array_equal(_bits(os_), _bits(o0[lo:])) and np.array_equal(ss, s0[lo:])
    # choice, the point values and the schedule do not depend on R or q
    for r2, q2 in ((2, Q16), (min(Rn, 64), (0.3,))):
        c2, _, o2, s2, _, _ = run(theta, rules, w, cost, None, coef[:r2], q2, "euler", 5, T)
        assert np.array_equal(c2, c0) and np.array_equal(_bits(o2[..., 0]), _bits(o0[..., 0])), r2
        assert np.array_equal(s2, s0)


@pytest.mark.parametrize("Rn,N,T,A,K,name", [(17, 3, 18, 2, 3, "std7"), (130, 2, 33, 4, 4, "lin3")])
def test_nan_rules(dev, Rn, N, T, A, K, name):
    y0, u, theta, rules, w, cost, ac, coef = _exact_inputs(Rn, N, T, A, K, name)
    theta = theta[:, :2 * K]
    w = w[..., :T]
    run = functools.partial(_run, dev, name, y0, u)
    args = (Q5, "rk4", 1, T)
    c0, w0, o0, s0, _, _ = run(theta, rules, w, cost, ac, coef, *args)
    assert not np.isnan(o0).any() and np.all(np.abs(w0.sum(axis=1) - 1.0) <= 4e-16)
    # a resampled replicate with NaN coefficients: every statistic of the row but the point is NaN, the exposure's
    # too; its vote is nobody's; the point model's schedule is untouched
    c1 = coef.copy()
    c1[Rn - 2] = np.nan
    cg, wg, og, sg, _, _ = run(theta, rules, w, cost, ac, c1, *args)
    ref = F.reference(y0, u, theta, rules, c1, name, Q5, w, cost, ac, 1, "rk4", 1, T)
    assert np.array_equal(cg, c0) and np.array_equal(_bits(wg), _bits(ref["win"])) and np.array_equal(sg, s0)
    assert np.allclose(wg.sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=4e-16)
    assert np.isnan(og[..., 1:]).all() and np.array_equal(_bits(og[..., 0]), _bits(o0[..., 0]))
    # replicate 0 NaN: no choice and NaN point values (the exposure's too), the votes and the other statistics intact
    cz = coef.copy()
    cz[0] = np.nan
    cg, wg, og, _, _, _ = run(theta, rules, w, cost, ac, cz, *args)
    assert np.all(cg == -1) and np.isnan(og[..., 0]).all()
    assert np.array_equal(_bits(wg), _bits(w0)) and np.array_equal(_bits(og[..., 1:]), _bits(o0[..., 1:]))
    # NaN in one coefficient of arm 1 of one replicate; rule 0 stays on arm 0, rule 1 on arm 1: rule 0 keeps its value
    # and exposure statistics, the replicate abstains, so every regret statistic but the point is NaN
    ca = coef.copy()
    ca[Rn - 2, 1, 1] = np.nan
    rl = rules.copy()
    rl[0, :2] = 0
    rl[1, :2] = 1
    cg, wg, og, sg, _, _ = run(theta, rl, w, cost, ac, ca, *args)
    ref = F.reference(y0, u, theta, rl, ca, name, Q5, w, cost, ac, 1, "rk4", 1, T)
    assert np.isfinite(og[:, 0, 0]).all() and np.isfinite(og[:, 0, 2]).all()
    assert np.isnan(og[:, 1, 0, 1:]).all() and np.isnan(og[:, 1, 2, 1:]).all() and np.isnan(og[:, :, 1, 1:]).all()
    assert np.isfinite(og[..., 0]).all()
    assert np.array_equal(cg, ref["choice"]) and np.array_equal(_bits(wg), _bits(ref["win"]))
    assert np.array_equal(sg, ref["sched"])
    assert _worst(og[:, :, :2], ref["out"][:, :, :2], ref["scale"]) <= TOL
    assert _worst(og[:, :, 2:], ref["out"][:, :, 2:], float(T)) <= TOL
    # a NaN threshold means off: rule 1 never switches on, whatever its flag was
    th = theta.copy()
    th[:, 2:4] = np.nan
    for start in (0, 1):
        rl = rules.copy()
        rl[1, 3] = start
        _, _, og, sg, _, _ = run(th, rl, w, cost, ac, coef, *args)
        assert np.all(og[:, 1, 2][:, [0, 1, 3, 4, 5, 6, 7]] == 0.0) and np.all(sg[:, 1] == rl[1, 1])
    ref = F.reference(y0, u, th, rl, coef, name, Q5, w, cost, ac, 1, "rk4", 1, T)
    assert _worst(og[:, :, :2], ref["out"][:, :, :2], ref["scale"]) <= TOL
    # one NaN threshold only: theta_on = NaN never switches on from off; started on it is held by theta_off
    th = theta.copy()
    th[:, 2] = np.nan
    th[:, 3] = -np.inf
    for start, expo in ((0, 0.0), (1, float(T))):
        rl = rules.copy()
        rl[1, 3] = start
        _, _, og, _, _, _ = run(th, rl, w, cost, ac, coef, *args)
        assert np.all(og[:, 1, 2, 0] == expo), start


def test_plan_and_out(dev):
    """``plan_feedback_rules`` writes into the caller's out and sched and repeats bit for bit; shape and argument
    errors."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, name = 65, 3, 33, 4, 4, "lin3"
    y0, u, theta, rules, w, cost, ac, coef = _exact_inputs(Rn, N, T, A, K, name)
    c0, w0, o0, s0, _, _ = _run(dev, name, y0, u, theta, rules, w, cost, ac, coef, Q5, "euler", 5, T)
    t = functools.partial(_t, dev)
    lib = M.LIBS[name]
    out = torch.zeros((N, K, 3, 3 + len(Q5)), dtype=torch.float64, device=dev)
    sched = torch.zeros((N, K, T), dtype=torch.int8, device=dev)
    ty0, tu, tth, tw, tc, tcoef = t(y0), t(u), t(theta), t(w), t(cost), t(coef)
    plan = ops.plan_feedback_rules(ty0, tu, tth, rules, tcoef, lib, DT, Q5, tw, cost=tc, arm_cost=ac, method="euler",
                                   substeps=5, drop_below=M.DROP_BELOW, T=T, out=out, sched=sched)
    for _ in range(2):
        choice, win, got, sc = plan()
        assert got is out and sc is sched and plan.out[2] is out
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(o0)) and np.array_equal(sched.cpu().numpy(), s0)
        assert np.array_equal(choice.cpu().numpy(), c0) and np.array_equal(_bits(win.cpu().numpy()), _bits(w0))
        out.zero_()
        sched.zero_()
    kw = dict(cost=tc, arm_cost=ac, T=T)
    call = functools.partial(ops.feedback_rules, ty0, tu)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, (0.5, 1.5), tw, **kw)
    with pytest.raises(ValueError):
        call(tth[:2], rules, tcoef, lib, DT, Q5, tw, **kw)                        # rows of the thresholds
    with pytest.raises(ValueError):
        call(tth[:, :2 * K - 1], rules, tcoef, lib, DT, Q5, tw, **kw)             # fewer than 2 K thresholds
    with pytest.raises(ValueError):
        call(tth, np.tile(rules, (5, 1)), tcoef, lib, DT, Q5, tw, T=T)            # 20 rules
    bad = rules.copy()
    bad[1, 0] = A
    with pytest.raises(ValueError):
        call(tth, bad, tcoef, lib, DT, Q5, tw, **kw)                              # an arm out of range
    bad = rules.copy()
    bad[2, 2] = 0
    with pytest.raises(ValueError):
        call(tth, bad, tcoef, lib, DT, Q5, tw, **kw)                              # period 0
    bad = rules.copy()
    bad[0, 3] = 2
    with pytest.raises(ValueError):
        call(tth, bad, tcoef, lib, DT, Q5, tw, **kw)                              # start_on = 2
    with pytest.raises(ValueError):
        call(tth, rules, tcoef[:1], lib, DT, Q5, tw, **kw)                        # no resample
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw[:2], **kw)                        # rows of the weights
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw[:, :T - 1], **kw)                 # fewer than T weights
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, cost=tc[:2], T=T)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, cost=tc, arm_cost=ac[:2], T=T)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, out=out[:, :2], **kw)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, sched=sched[:, :, :T - 1], **kw)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, sched=sched.to(torch.int32), **kw)
    with pytest.raises(ValueError):
        call(tth, rules, tcoef, lib, DT, Q5, tw, method="heun", **kw)


def test_no_rows(dev):
    """n_rows = 0 is a successful no-op with empty outputs, in both threshold forms."""
    Rn, N, T, A, K, name = 65, 3, 33, 4, 4, "lin3"
    y0, u, theta, rules, w, cost, ac, coef = _exact_inputs(Rn, N, T, A, K, name)
    for th, ww in ((theta[:0], w[:0]), (np.zeros((K, 2)), w[0])):
        choice, win, out, sched, _, _ = _run(dev, name, y0[:0], u[:0], th, rules, ww, cost, ac, coef, Q5, "euler", 5,
                                             T)
        assert choice.shape == (0,) and win.shape == (0, K) and out.shape == (0, K, 3, 3 + len(Q5))
        assert sched.shape == (0, K, T)


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
    """[3, 3 + Q, N, K] of a FeedbackResult."""
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def test_plugin_evaluate_rules(dev, model):
    """``evaluate_rules`` against the restatement on the plugin's inputs, with the units round-tripped: thresholds
    are given in ``get_predictions`` units and passed as theta std + mean, costs and arm costs as cost std; value =
    (J - mean sum_k w) / std, the regret is divided by std only, the exposure is a count."""
    from insite_amd.effect import ThresholdRule
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    prev, stat, _, _ = model._unscaled_inputs(tr)
    y0 = prev[:, 0].cpu().numpy()
    z0 = (y0 - mean) / std                                   # the first state in get_predictions units
    N = y0.shape[0]
    T = tr.data["current_treatments"].shape[1]
    rules = [ThresholdRule(float(np.median(z0))),
             ThresholdRule(float(np.quantile(z0, 0.75)), float(np.quantile(z0, 0.25)), every=2, start_on=True),
             ThresholdRule(z0 - 0.05, z0 - 0.4, arm_on=0, arm_off=1, every=5)]
    costs, arm_costs = [0.0, 0.02, -0.01], [0.0, 0.004]
    res = model.evaluate_rules(tr, rules, objective="mean", costs=costs, arm_costs=arm_costs, schedule=True)
    assert res.series == ("value", "regret", "exposure") and res.q == q
    assert res.win.shape == (N, 3) and res.point.shape == (3, N, 3) and res.quantiles.shape == (3, 3, N, 3)
    assert res.schedule.shape == (N, 3, T) and res.schedule.dtype.is_floating_point is False
    assert model.evaluate_rules(tr, rules, costs=costs, arm_costs=arm_costs).schedule is None
    # the restatement, in raw units
    th = np.empty((N, 6))
    th[:, 0] = th[:, 1] = np.median(z0)
    th[:, 2], th[:, 3] = np.quantile(z0, 0.75), np.quantile(z0, 0.25)
    th[:, 4], th[:, 5] = z0 - 0.05, z0 - 0.4
    table = np.array([[1, 0, 1, 0], [1, 0, 2, 1], [0, 1, 5, 0]], dtype=np.int32)
    ae = tr.data["active_entries"][..., 0].astype(np.float64)
    w = ae / ae.sum(axis=1, keepdims=True)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    ref = F.feedback(y0, stat.cpu().numpy(), th * std + mean, table, coef, R.poly_library(3, 2, True), model.dt, q, w,
                     np.array(costs) * std, np.array(arm_costs) * std, 1, "euler5")
    print(f"decision margin {ref['dmargin'].min():.3e}, argmin margin {ref['margin'].min():.3e}")
    assert ref["dmargin"].min() >= 1e-8 and ref["margin"].min() >= 1e-8          # the inputs decide nothing by a hair
    assert np.array_equal(res.choice.cpu().numpy(), ref["choice"])
    assert np.array_equal(_bits(res.win.cpu().numpy()), _bits(ref["win"]))
    assert np.array_equal(res.schedule.cpu().numpy(), ref["sched"])
    got = _stack(res).transpose(2, 3, 0, 1)                                      # [N, K, 3, 3 + Q]
    want = ref["out"].copy()
    want[:, :, :2] /= std
    loc = [0, 1, 3, 4, 5]
    want[:, :, 0, loc] = (ref["out"][:, :, 0, loc] - (mean * w.sum(axis=1))[:, None, None]) / std
    assert np.array_equal(_bits(got[:, :, 2, 0]), _bits(want[:, :, 2, 0]))
    # the value is a difference of two numbers of the size of |J_raw|: the bar is on the raw scale, standardised
    scale = (ref["scale"] + abs(mean) * w.sum(axis=1)) / std
    worst = _worst(got[:, :, :2], want[:, :, :2], scale)
    worst_e = _worst(got[:, :, 2:], want[:, :, 2:], float(T))
    print(f"worst |got - ref| / s_p = {worst:.3e}; exposure statistics: worst |got - ref| / T = {worst_e:.3e}")
    assert worst <= TOL and worst_e <= TOL
    # the schedule is a set of plans choose_plan takes: the point value of its plan j is the point value of rule j
    # without the arm costs
    res0 = model.evaluate_rules(tr, rules, costs=costs, schedule=True)
    sched = res0.schedule.cpu().numpy()
    cp = model.choose_plan(tr, [sched[:, j].astype(np.int64) for j in range(3)], objective="mean", costs=costs)
    assert np.array_equal(_bits(cp.point.cpu().numpy()[0]), _bits(res0.point.cpu().numpy()[0]))
    with pytest.raises(ValueError):
        model.evaluate_rules(tr, [ThresholdRule(0.0, arm_on=2)])
    with pytest.raises(ValueError):
        model.evaluate_rules(tr, [ThresholdRule(0.0, every=0)])
    with pytest.raises(ValueError):
        model.evaluate_rules(tr, [ThresholdRule(np.zeros(N + 1))])
    with pytest.raises(ValueError):
        model.evaluate_rules(tr, rules, objective="median")
