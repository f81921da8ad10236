"""GPU tests of the rule value (include/insite_rulevalue.h: rulevalue_assign_kernel, rulevalue_sums_kernel,
rulevalue_reduce_kernel, rulevalue_finalize_kernel, ops.rule_value, SINDY.rule_value) against the numpy restatement
tests/rule_value_ref.py.

Tolerance: the J-based sums and series within TOL s_g of the restatement, s_g = max over replicates, rows of the group
and rules of (|cost_j| + sum_k |w| |y|) + sum_a |arm_cost_a|: the bar of tests/test_gpu_policy.py and
tests/test_gpu_feedback.py for this arithmetic.  The shares within 1e-12 absolute, the exposure series (means of counts
of at most T steps) within TOL T.  ``wsum``, the allocation and the exposure columns of ``sums``, ``assign``,
``best_fixed`` and ``fixwin`` are compared exactly: tests/test_rulevalue_abi.py asserts that every decision and every
argmin behind them has a margin of at least 1e-8 of its scale, a hundred times the bar.

Worst figures over the parity cases on an MI355X are in DESIGN.md §9n.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cohort_effect_ref as CR  # noqa: E402
import library_matrix as M  # noqa: E402
import rule_value_ref as V  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, TOL_SHARE = 1e-10, 1e-12
DT, Q5, Q16 = V.DT, V.Q5, V.Q16
KEYS = ("out", "fixwin", "best_fixed", "assign", "sums", "wsum")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _run(dev, name, y0, u, theta, rules, w, cost, arm_cost, coef, q, method, sub, T, sense=1, assign=None, group=None,
         Gn=1, weighting="none", seed=V.SEED, off=0, pad_out=0, workspace=None):
    """dict(out [G, 3 K + 9, 3 + Q], fixwin, best_fixed, assign, sums, wsum, pad: the padding of out or None)."""
    import torch
    from insite_amd import ops
    t = functools.partial(_t, dev)
    K, NS = len(rules), 3 + len(q)
    out = buf = None
    if pad_out:
        buf = torch.full((Gn, 3 * K + 9, NS + pad_out), V.POISON, dtype=torch.float64, device=dev)
        out = buf[:, :, :NS]
    got = ops.rule_value(t(y0), t(u), t(theta), rules, t(coef), M.LIBS[name], DT, q, t(w), cost=t(cost),
                         arm_cost=arm_cost, maximize=sense < 0, assign=t(assign), group=t(group), n_groups=Gn,
                         weighting=weighting, seed=seed, patient_offset=off, method=method, substeps=sub,
                         drop_below=M.DROP_BELOW, T=T, out=out, workspace=workspace)
    torch.cuda.synchronize()
    if pad_out:
        assert got[0] is out
    res = dict(zip(KEYS, (a.cpu().numpy() for a in got)))
    res["pad"] = None if buf is None else buf[:, :, NS:].cpu().numpy()
    return res


def _same(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def _rel(got, ref, scale):
    """max |got - ref| / scale (broadcast); a NaN on one side only is inf."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(got - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(scale, got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _worst(res, ref, K, T):
    """(the worst relative error of the J-based series of out and columns of sums, the worst absolute error of the
    share series, the worst error of the exposure series relative to T)."""
    s = ref["scale"]
    cont = _rel(res["out"][:, :K + 6], ref["out"][:, :K + 6], s[:, None, None])
    sm = _rel(res["sums"][:, :, :K + 2], ref["sums"][:, :, :K + 2], (s[None, :] * ref["wsum"])[:, :, None])
    share = _rel(res["out"][:, K + 6:2 * K + 6], ref["out"][:, K + 6:2 * K + 6], 1.0)
    expo = _rel(res["out"][:, 2 * K + 6:], ref["out"][:, 2 * K + 6:], float(T))
    return max(cont, sm), share, expo


def _check_exact_sums(res, K, sense):
    """The header's inequalities and the allocation identity on the returned sums, with no tolerance."""
    S, ws = res["sums"], res["wsum"]
    s = float(sense)
    ok = ~np.isnan(S[:, :, :K + 2]).any(axis=2)
    for j in range(K):
        assert (s * S[:, :, K] <= s * S[:, :, j])[ok].all(), j
    assert (s * S[:, :, K] <= s * S[:, :, K + 1])[ok].all()
    alloc = S[:, :, K + 2:2 * K + 2]
    assert np.array_equal(alloc.sum(axis=2)[ok], ws[ok])
    assert np.array_equal(alloc, np.round(alloc)) and np.array_equal(ws, np.round(ws))
    ex = S[:, :, 2 * K + 2:]
    assert np.array_equal(ex, np.round(ex), equal_nan=True)
    # so the personalised gain and the optimism are >= 0 in every statistic that is a value of some replicate
    loc = [0] + list(range(3, res["out"].shape[2]))
    d = res["out"][:, [K + 3, K + 5]][:, :, loc]
    assert (np.nan_to_num(d, nan=0.0) >= 0).all()


def _check_against(res, ref, K, T, what=""):
    worst, share, expo = _worst(res, ref, K, T)
    print(f"{what}worst |got - ref| / s_g = {worst:.3e}, shares abs {share:.3e}, exposures / T {expo:.3e}")
    assert np.array_equal(res["wsum"], ref["wsum"])
    assert np.array_equal(res["sums"][:, :, K + 2:], ref["sums"][:, :, K + 2:], equal_nan=True)
    assert np.array_equal(res["assign"], ref["assign"])
    assert np.array_equal(res["best_fixed"], ref["best_fixed"])
    assert np.array_equal(_bits(res["fixwin"]), _bits(ref["fixwin"]))
    assert worst <= TOL
    assert share <= TOL_SHARE
    assert expo <= TOL


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_parity(dev, case):
    (Rn, N, T, A, K, Gn, name, method, sub, q, _, _, _, _, sense, weighting, off, _, _, _) = case
    y0, u, theta, rules, w, cost, arm_cost, coef, group, assign, ref = V.case(*case)
    kw = dict(sense=sense, assign=assign, group=group, Gn=Gn, weighting=weighting, off=off)
    res = _run(dev, name, y0, u, theta, rules, w, cost, arm_cost, coef, q, method, sub, T, pad_out=V.PAD_OUT, **kw)
    assert res["out"].shape == (Gn, 3 * K + 9, 3 + len(q)) and res["sums"].shape == (Rn, Gn, 3 * K + 4)
    assert res["fixwin"].shape == (Gn, K) and res["best_fixed"].shape == (Gn,) and res["assign"].shape == (N,)
    assert np.all(res["pad"] == V.POISON)
    _check_against(res, ref, K, T)
    _check_exact_sums(res, K, sense)
    if Rn == 2:
        assert np.isnan(res["out"][..., 2]).all()
    # the NaN thresholds past 2 K and the NaN weights past T are never read: unpadded inputs give the same bits
    th2 = theta if case[10] == "shared" else theta[:, :2 * K]
    r2 = _run(dev, name, y0, u, th2, rules, w[..., :T], cost, arm_cost, coef, q, method, sub, T, **kw)
    _same(r2, res)


# ---------------------------------------------------------------------------------------------------
# exact anchors
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_inputs(Rn, N, T, A, K, Gn, name, theta_mode="rows"):
    out = V.inputs(("rulevalue-exact", Rn, N, T, A, K, Gn, name), Rn, N, T, A, K, Gn, name, theta_mode=theta_mode)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _exact_ref(Rn, N, T, A, K, Gn, name, sense, weighting, off, method, sub):
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    return V.reference(y0, u, theta, rules, coef, name, Q5, w, cost, arm_cost, sense, None, group, Gn, weighting,
                       V.SEED, off, method, sub, T)


EXACT = [(2, 3, 33, 2, 3, 1, "std7"), (65, 130, 65, 4, 4, 3, "lin3"), (130, 200, 18, 2, 8, 3, "std7")]


@pytest.mark.parametrize("Rn,N,T,A,K,Gn,name", EXACT)
def test_exact_properties(dev, Rn, N, T, A, K, Gn, name):
    """The inequalities, repeatability, a constant assignment, K = 1 and identical rules, with no tolerance."""
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    run = functools.partial(_run, dev, name, y0, u)
    args = (coef, Q5, "euler", 5, T)
    kw = dict(group=group, Gn=Gn, weighting="poisson", off=3)
    for sense in (1, -1):
        r0 = run(theta, rules, w, cost, arm_cost, *args, sense=sense, **kw)
        _check_exact_sums(r0, K, sense)
        # two calls are bitwise equal
        _same(run(theta, rules, w, cost, arm_cost, *args, sense=sense, **kw), r0)
        # a constant assignment j reproduces the columns of rule j bit for bit, and changes nothing else
        for j in (0, K - 1):
            rj = run(theta, rules, w, cost, arm_cost, *args, sense=sense, assign=np.full(N, j, dtype=np.int32), **kw)
            assert np.array_equal(_bits(rj["sums"][:, :, K + 1]), _bits(rj["sums"][:, :, j])), j
            assert np.array_equal(_bits(rj["sums"][:, :, 3 * K + 3]), _bits(rj["sums"][:, :, 2 * K + 2 + j])), j
            keep = [c for c in range(3 * K + 4) if c not in (K + 1, 3 * K + 3)]
            assert np.array_equal(_bits(rj["sums"][:, :, keep]), _bits(r0["sums"][:, :, keep]))
            assert np.array_equal(_bits(rj["out"][:, K + 1]), _bits(rj["out"][:, j]))
            assert np.array_equal(_bits(rj["out"][:, 3 * K + 7]), _bits(rj["out"][:, 2 * K + 6 + j]))
        # K = 1: the personalised, assigned and value_0 columns are the same bits, the three differences exactly +0
        k1 = run(theta[:, :2], rules[:1], w, cost[:1], arm_cost, *args, sense=sense, **kw)
        for c in (1, 2):
            assert np.array_equal(_bits(k1["sums"][:, :, c]), _bits(k1["sums"][:, :, 0]))
        for c in (5, 6):
            assert np.array_equal(_bits(k1["sums"][:, :, c]), _bits(k1["sums"][:, :, 4]))
        assert np.array_equal(k1["sums"][:, :, 3], k1["wsum"]) and np.all(k1["assign"] == 0)
        ok = (k1["wsum"] > 0).all(axis=0)                       # groups that every replicate drew
        d = np.delete(k1["out"][ok][:, 4:7], 2, axis=-1)
        assert np.all(_bits(d) == 0)
        assert np.all(k1["fixwin"][ok] == 1.0) and np.all(k1["best_fixed"][ok] == 0)
        assert np.array_equal(_bits(k1["out"][:, 0]), _bits(r0["out"][:, 0]))
        assert np.array_equal(_bits(k1["out"][:, 8]), _bits(r0["out"][:, 2 * K + 6]))      # exposure_0
    # identical rules (and costs) put every vote on rule 0
    th = np.tile(theta[:, :2], (1, K))
    same = run(th, np.repeat(rules[:1], K, axis=0), w, np.repeat(cost[:1], K), arm_cost, *args, **kw)
    assert np.all(same["sums"][:, :, K + 3:2 * K + 2] == 0) and np.array_equal(same["sums"][:, :, K + 2], same["wsum"])
    assert np.all(same["assign"] == 0)
    ok = (same["wsum"] > 0).all(axis=0)
    assert np.all(same["best_fixed"][ok] == 0) and np.all(same["fixwin"][ok][:, 0] == 1.0)
    for c in range(1, K + 2):
        assert np.array_equal(_bits(same["sums"][:, :, c]), _bits(same["sums"][:, :, 0])), c
    for c in range(2 * K + 3, 3 * K + 4):
        assert np.array_equal(_bits(same["sums"][:, :, c]), _bits(same["sums"][:, :, 2 * K + 2])), c


CONSTANT = [(2, 3, 33, 1, 2, 1, "x_only", "shared", "none"), (65, 130, 65, 4, 4, 3, "lin3", "rows", "poisson"),
            (17, 700, 18, 2, 8, 3, "std7", "rows", "poisson"), (130, 200, 70, 2, 16, 3, "std7", "shared", "none")]


@pytest.mark.parametrize("Rn,N,T,A,K,Gn,name,theta_mode,weighting", CONSTANT)
def test_constant_rules_are_policy_sums(dev, Rn, N, T, A, K, Gn, name, theta_mode, weighting):
    """theta = -Inf (always on) or +Inf with start_on 0 (always off) and no arm cost: the columns 0..2K+1 and wsum are
    ``ops.policy_sums``' under the constant plans, bit for bit (one to several patient chunks: the two calls cut the
    cohort alike); the assignment is its rule; the exposure sums are exactly T wsum or 0."""
    import torch
    from insite_amd import ops
    y0, u, theta, rules, w, cost, _, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name, theta_mode)
    theta, rules = theta.copy(), rules.copy()
    arms = np.empty(K, dtype=np.int8)
    for j in range(K):
        cols = (j, slice(None)) if theta_mode == "shared" else (slice(None), slice(2 * j, 2 * j + 2))
        if j % 2 == 0:                                           # always on: arm_on at every step
            theta[cols] = -np.inf
            arms[j] = rules[j, 0]
        else:                                                    # always off: arm_off at every step
            theta[cols] = np.inf
            rules[j, 3] = 0
            arms[j] = rules[j, 1]
    plans = np.repeat(arms[:, None], T, axis=1)
    t = functools.partial(_t, dev)
    for sense in (1, -1):
        kw = dict(group=group, Gn=Gn, weighting=weighting, off=5)
        res = _run(dev, name, y0, u, theta, rules, w, cost, None, coef, Q5, "rk4", 1, T, sense=sense, **kw)
        sums, wsum, rule = ops.policy_sums(t(y0), t(u), t(plans), t(coef), M.LIBS[name], DT, t(w), cost=t(cost),
                                           maximize=sense < 0, group=t(group), n_groups=Gn, weighting=weighting,
                                           seed=V.SEED, patient_offset=5, method="rk4", substeps=1,
                                           drop_below=M.DROP_BELOW, T=T)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(res["sums"][:, :, :2 * K + 2]), _bits(sums.cpu().numpy()))
        assert np.array_equal(_bits(res["wsum"]), _bits(wsum.cpu().numpy()))
        assert np.array_equal(res["assign"], rule.cpu().numpy())
        for j in range(K):
            want = T * res["wsum"] if j % 2 == 0 else np.zeros_like(res["wsum"])
            assert np.array_equal(res["sums"][:, :, 2 * K + 2 + j], want), j
        # the personalised and the assigned exposure: T where the chosen rule is an always-on one
        even = sum(res["sums"][:, :, K + 2 + j] for j in range(0, K, 2))
        assert np.array_equal(res["sums"][:, :, 3 * K + 2], T * even)


@pytest.mark.parametrize("Rn,N,T,A,K,name,sense", [(65, 130, 65, 4, 4, "lin3", 1), (512, 70, 18, 2, 8, "std7", -1)])
def test_agrees_with_feedback_rules(dev, Rn, N, T, A, K, name, sense):
    """``assign`` is ``ops.feedback_rules``' choice; with weighting NONE and one group the summed allocation of the
    resampled replicates is (R - 1) times its summed ``win``, exactly; with one row the value_j and exposure_j
    statistics are its per-row statistics, within the bar."""
    import torch
    from insite_amd import ops
    y0, u, theta, rules, w, cost, arm_cost, coef, _, _ = _exact_inputs(Rn, N, T, A, K, 1, name)
    res = _run(dev, name, y0, u, theta, rules, w, cost, arm_cost, coef, Q5, "euler", 5, T, sense=sense)
    t = functools.partial(_t, dev)
    choice, win, out, _ = ops.feedback_rules(t(y0), t(u), t(theta), rules, t(coef), M.LIBS[name], DT, Q5, t(w),
                                             cost=t(cost), arm_cost=arm_cost, maximize=sense < 0, method="euler",
                                             substeps=5, drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    choice, win, out = choice.cpu().numpy(), win.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(res["assign"], choice)
    votes = np.rint(win * (Rn - 1))
    assert np.array_equal(votes / (Rn - 1), win)
    assert np.array_equal(res["sums"][1:, 0, K + 2:2 * K + 2].sum(axis=0), votes.sum(axis=0))
    scale = np.abs(out[:, :, 0, 0]).max() + float(np.abs(arm_cost).sum())
    assert np.max(np.abs(res["out"][0, :K, 0] - out[:, :, 0, 0].mean(axis=0))) <= TOL * scale
    assert np.max(np.abs(res["out"][0, 2 * K + 6:3 * K + 6, 0] - out[:, :, 2, 0].mean(axis=0))) <= TOL * T
    pick = out[np.arange(N), choice, 0, 0]
    assert abs(res["out"][0, K + 1, 0] - pick.mean()) <= TOL * scale
    # one row: the series over the replicates are the row's own
    for p in (0, N - 1):
        one = _run(dev, name, y0[p:p + 1], u[p:p + 1], theta[p:p + 1], rules, w[p:p + 1], cost, arm_cost, coef, Q5,
                   "euler", 5, T, sense=sense)
        s = np.abs(out[p, :, 0]).max() + float(np.abs(arm_cost).sum())
        assert one["assign"][0] == choice[p]
        assert np.max(np.abs(one["out"][0, :K] - out[p, :, 0])) <= TOL * s
        assert np.max(np.abs(one["out"][0, 2 * K + 6:3 * K + 6] - out[p, :, 2])) <= TOL * T
        assert np.array_equal(_bits(one["out"][0, :K, 0]), _bits(out[p, :, 0, 0]))           # the point model's J
        assert np.array_equal(one["fixwin"][0], win[p])


@pytest.mark.parametrize("split", [64, 37])
def test_shards_and_finalize_alone(dev, split):
    """Two shards (an even and an odd split) with ``patient_offset`` add to the whole: wsum, the allocation and the
    exposures exactly, the values within the bar; ``rule_value_finalize`` on the added sums, and on the restatement's
    sums, gives the whole cohort's statistics; on the whole call's own sums it gives that call's out bit for bit."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    off = 1000
    ref = _exact_ref(Rn, N, T, A, K, Gn, name, -1, "poisson", off, "euler", 5)
    whole = _run(dev, name, y0, u, theta, rules, w, cost, arm_cost, coef, Q5, "euler", 5, T, sense=-1, group=group,
                 Gn=Gn, weighting="poisson", off=off)
    _check_against(whole, ref, K, T, "whole: ")
    t = functools.partial(_t, dev)
    lib = M.LIBS[name]
    parts = []
    for lo, hi in ((0, split), (split, N)):
        parts.append(ops.rule_value_sums(t(y0[lo:hi]), t(u[lo:hi]), t(theta[lo:hi]), rules, t(coef), lib, DT,
                                         t(w[lo:hi]), cost=t(cost), arm_cost=arm_cost, maximize=True,
                                         group=t(group[lo:hi]), n_groups=Gn, weighting="poisson", seed=V.SEED,
                                         patient_offset=off + lo, method="euler", substeps=5, drop_below=M.DROP_BELOW,
                                         T=T))
    sums, wsum = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assign = torch.cat([parts[0][2], parts[1][2]]).cpu().numpy()
    assert np.array_equal(assign, whole["assign"])
    assert np.array_equal(wsum.cpu().numpy(), whole["wsum"])
    assert np.array_equal(sums.cpu().numpy()[:, :, K + 2:], whole["sums"][:, :, K + 2:])
    out, fixwin, bf = (a.cpu().numpy() for a in ops.rule_value_finalize(sums, wsum, Q5, maximize=True))
    got = {"out": out, "sums": sums.cpu().numpy(), "wsum": wsum.cpu().numpy(), "assign": assign, "fixwin": fixwin,
           "best_fixed": bf}
    _check_against(got, ref, K, T, f"shards at {split}: ")
    # finalize alone on the restatement's sums
    out, fixwin, bf = (a.cpu().numpy() for a in ops.rule_value_finalize(t(ref["sums"]), t(ref["wsum"]), Q5,
                                                                        maximize=True))
    got = dict(got, out=out, fixwin=fixwin, best_fixed=bf, sums=ref["sums"])
    _check_against(got, ref, K, T, "finalize of the restatement's sums: ")
    # and finalize of the whole call's own sums is the whole call's out, bit for bit
    pad = torch.full((Gn, 3 * K + 9, 3 + len(Q5) + 2), V.POISON, dtype=torch.float64, device=dev)
    out, fixwin, bf = ops.rule_value_finalize(t(whole["sums"]), t(whole["wsum"]), Q5, maximize=True,
                                              out=pad[:, :, :3 + len(Q5)])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(whole["out"]))
    assert np.array_equal(_bits(fixwin.cpu().numpy()), _bits(whole["fixwin"]))
    assert np.array_equal(bf.cpu().numpy(), whole["best_fixed"]) and bool((pad[:, :, 3 + len(Q5):] == V.POISON).all())


def test_rules(dev):
    """A zero-weight or excluded row with NaN y0, u and theta reaches nothing; a NaN replicate poisons exactly what the
    header says; a replicate that drew no row gives 0 / 0 = NaN in every series of the group; an assignment of -1 or
    K makes the two assigned columns NaN and nothing else."""
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    run = functools.partial(_run, dev, name)
    args = (Q5, "rk4", 1, T)
    kw = dict(group=group, Gn=Gn, weighting="poisson", off=0)
    r0 = run(y0, u, theta, rules, w, cost, arm_cost, coef, *args, **kw)
    om = CR.weights("poisson", V.SEED, Rn, N, 0)
    assert not np.isnan(r0["out"]).any()
    S_, C_ = 3 * K + 9, 3 * K + 4
    # row 5 is excluded by its group, row 6 only counts in the replicates that drew it
    g2 = np.array(group)
    g2[5], g2[6] = -1, 1
    base = run(y0, u, theta, rules, w, cost, arm_cost, coef, *args, **dict(kw, group=g2))
    yn, un, tn = y0.copy(), u.copy(), theta.copy()
    yn[5], un[5], tn[5] = np.nan, np.nan, np.nan
    rn = run(yn, un, tn, rules, w, cost, arm_cost, coef, *args, **dict(kw, group=g2))
    assert rn["assign"][5] == -1
    _same(rn, base, ("out", "fixwin", "sums", "wsum"))
    yn[6] = np.nan
    rn = run(yn, un, tn, rules, w, cost, arm_cost, coef, *args, **dict(kw, group=g2))
    hit = om[:, 6] > 0
    assert hit[0] and not hit.all()
    assert np.isnan(rn["sums"][hit, 1, :K + 2]).all() and np.isnan(rn["sums"][hit, 1, 2 * K + 2:]).all()
    assert np.array_equal(_bits(rn["sums"][~hit]), _bits(base["sums"][~hit]))
    assert np.array_equal(_bits(rn["sums"][:, [0, 2]]), _bits(base["sums"][:, [0, 2]]))
    assert np.array_equal(rn["wsum"], base["wsum"])
    # a NaN threshold alone is "off", not NaN: nothing becomes NaN
    tq = theta.copy()
    tq[6] = np.nan
    rq = run(y0, u, tq, rules, w, cost, arm_cost, coef, *args, **dict(kw, group=g2))
    assert not np.isnan(rq["sums"]).any() and np.array_equal(rq["wsum"], base["wsum"])
    # a NaN replicate: its value, personalised, assigned and exposure sums are NaN, it allocates nothing and votes for
    # no fixed rule; every statistic but the point of the J-based and exposure series is NaN, the shares stay finite
    cn = coef.copy()
    cn[Rn - 2] = np.nan
    rn = run(y0, u, theta, rules, w, cost, arm_cost, cn, *args, **kw)
    assert np.isnan(rn["sums"][Rn - 2, :, :K + 2]).all() and np.all(rn["sums"][Rn - 2, :, K + 2:2 * K + 2] == 0)
    assert np.isnan(rn["sums"][Rn - 2, :, 2 * K + 2:]).all()
    others = np.arange(Rn) != Rn - 2
    assert np.array_equal(_bits(rn["sums"][others]), _bits(r0["sums"][others]))
    assert np.isnan(rn["out"][:, :K + 6, 1:]).all() and np.isfinite(rn["out"][:, K + 6:2 * K + 6]).all()
    assert np.isnan(rn["out"][:, 2 * K + 6:, 1:]).all()
    assert np.array_equal(_bits(rn["out"][..., 0]), _bits(r0["out"][..., 0]))
    assert np.array_equal(rn["best_fixed"], r0["best_fixed"]) and np.array_equal(rn["assign"], r0["assign"])
    assert np.allclose(rn["fixwin"].sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=4e-16)
    # an empty replicate: group 2 holds row 9 alone, which some replicate did not draw
    g3 = np.where(np.array(group) == 2, -1, group)
    g3[9] = 2
    assert (om[1:, 9] == 0).any()
    rn = run(y0, u, theta, rules, w, cost, arm_cost, coef, *args, **dict(kw, group=g3))
    assert np.array_equal(rn["wsum"][:, 2], om[:, 9].astype(float))
    assert rn["out"].shape[1] == S_ and np.isnan(rn["out"][2, :, 1:]).all() and np.isfinite(rn["out"][2, :, 0]).all()
    assert np.isfinite(rn["out"][:2]).all()
    # an assignment of -1 or K: the assigned columns are NaN wherever the row has weight, and nothing else changes
    for bad in (-1, K):
        al = r0["assign"].copy()
        p = int(np.nonzero(np.array(group) == 1)[0][0])
        al[p] = bad
        rb = run(y0, u, theta, rules, w, cost, arm_cost, coef, *args, assign=al, **kw)
        hit = om[:, p] > 0
        assert np.isnan(rb["sums"][hit, 1, K + 1]).all() and np.isnan(rb["sums"][hit, 1, 3 * K + 3]).all() and hit[0]
        assert np.array_equal(_bits(rb["sums"][~hit]), _bits(r0["sums"][~hit]))
        keep = [c for c in range(C_) if c not in (K + 1, 3 * K + 3)]
        assert np.array_equal(_bits(rb["sums"][:, :, keep]), _bits(r0["sums"][:, :, keep]))
        assert np.array_equal(_bits(rb["sums"][:, [0, 2]]), _bits(r0["sums"][:, [0, 2]]))
        touched = (K + 1, K + 4, K + 5, 3 * K + 7)
        ser = [s for s in range(S_) if s not in touched]
        assert np.array_equal(_bits(rb["out"][:, ser]), _bits(r0["out"][:, ser]))
        assert np.isnan(rb["out"][1, touched]).all()


def test_no_rows_and_arguments(dev):
    """n_rows = 0 is a successful no-op (fresh sums stay zero); ``plan_rule_value`` repeats bit for bit; shape and
    argument errors."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    shared = np.ascontiguousarray(theta[0, :2 * K].reshape(K, 2))
    for th, ww in ((theta[:0], w[:0]), (shared, w[0])):
        res = _run(dev, name, y0[:0], u[:0], th, rules, ww, cost, arm_cost, coef, Q5, "euler", 5, T, group=group[:0],
                   Gn=Gn)
        assert res["assign"].shape == (0,) and np.all(res["sums"] == 0) and np.all(res["wsum"] == 0)
    r0 = _run(dev, name, y0, u, theta, rules, w, cost, arm_cost, coef, Q5, "euler", 5, T, group=group, Gn=Gn,
              weighting="poisson")
    t = functools.partial(_t, dev)
    lib = M.LIBS[name]
    ty0, tu, tth, tw, tc, tcoef, tg = t(y0), t(u), t(theta), t(w), t(cost), t(coef), t(group)
    kw = dict(cost=tc, arm_cost=arm_cost, group=tg, n_groups=Gn, seed=V.SEED, method="euler", substeps=5,
              drop_below=M.DROP_BELOW, T=T)
    plan = ops.plan_rule_value(ty0, tu, tth, rules, tcoef, lib, DT, Q5, tw, **kw)
    for _ in range(2):
        got = plan()
        torch.cuda.synchronize()
        for key, a in zip(KEYS, got):
            assert np.array_equal(a.cpu().numpy(), r0[key], equal_nan=True), key
        got[0].zero_()
        got[4].zero_()
    bad_rules = np.array(rules)
    bad_rules[1, 0] = A
    for bad in (dict(assign=t(np.zeros(N - 1, dtype=np.int32))), dict(assign=t(np.zeros(N, dtype=np.int64))),
                dict(group=tg[:5]), dict(n_groups=65), dict(n_groups=0), dict(weighting="binomial"),
                dict(seed=-1), dict(patient_offset=-1), dict(method="heun"), dict(cost=tc[:2]), dict(T=T + 10),
                dict(arm_cost=arm_cost[:2]),
                dict(out=torch.zeros((Gn, 3 * K + 8, 3 + len(Q5)), dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            ops.rule_value(ty0, tu, tth, rules, tcoef, lib, DT, Q5, tw, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ops.rule_value(ty0, tu, tth, rules, tcoef, lib, DT, (0.5, 1.5), tw, **kw)
    with pytest.raises(ValueError):
        ops.rule_value(ty0, tu, tth, bad_rules, tcoef, lib, DT, Q5, tw, **kw)
    with pytest.raises(ValueError):
        ops.rule_value(ty0, tu, tth[:, :2 * K - 1], rules, tcoef, lib, DT, Q5, tw, **kw)
    with pytest.raises(ValueError):
        ops.rule_value(ty0, tu, tth, rules, tcoef[:1], lib, DT, Q5, tw, **kw)                      # no resample


# ---------------------------------------------------------------------------------------------------
# the workspace contract (class "none" of tests/workspace_matrix.py, which cannot take a row for these signatures)
# ---------------------------------------------------------------------------------------------------
GUARD = 4096


class _GuardedWorkspace:
    """What ``ops`` needs of a ``Workspace``: hands out exactly the bytes asked for, between two guards."""

    def __init__(self, buf):
        self.buf, self.asked = buf, []

    def claim(self, kind):
        assert kind == "scratch"
        return self

    def get(self, nbytes, device):
        self.asked.append(int(nbytes))
        assert GUARD + nbytes + GUARD <= self.buf.numel()
        return self.buf[GUARD:GUARD + int(nbytes)]


def _ws_shape(dev, Rn, N):
    T, A, K, Gn, name = 18, 2, 3, 3, "std7"
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = _exact_inputs(65, 130, T, A, K, Gn, name)
    args = (name, y0[:N], u[:N], theta[:N], rules, w[:N], cost, arm_cost, coef[:Rn], Q5, "euler", 5, T)
    kw = dict(group=group[:N], Gn=Gn, weighting="poisson", off=2)
    from insite_amd import _lib
    need = _lib.load().insite_rulevalue_workspace_bytes(N, T, A, coef.shape[2], Rn, Gn, K)
    return args, kw, need


def test_workspace_contract(dev):
    """Exactly the queried bytes suffice, the buffer needs no initialisation and carries nothing between calls: a
    zeroed buffer, then a buffer of exactly the queried size between two 4 KiB guards filled with 0xFF and with 0x5A,
    give bitwise equal outputs and leave the guards alone; the wrapper asks for no more than the query; the sequence
    largest, smallest, n = 0, smallest, largest on one buffer that is never zeroed again repeats them."""
    import torch
    shapes = {(Rn, N): _ws_shape(dev, Rn, N) for Rn in (2, 65) for N in (40, 130)}
    biggest = max(need for _, _, need in shapes.values())
    assert min(need for _, _, need in shapes.values()) > 0
    want = {}
    for key, (args, kw, need) in shapes.items():
        buf = torch.zeros(GUARD + need + GUARD, dtype=torch.uint8, device=dev)
        ws = _GuardedWorkspace(buf)
        want[key] = _run(dev, *args, workspace=ws, **kw)
        assert ws.asked == [need]                                # no more than the query
        for fill in (0xFF, 0x5A):
            buf.fill_(fill)
            got = _run(dev, *args, workspace=ws, **kw)
            _same(got, want[key])
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + need:] == fill).all()), (key, fill)
            # the null assignment is scratch too: given, the call writes the same sums
            got = _run(dev, *args, workspace=ws, assign=want[key]["assign"], **kw)
            _same(got, want[key])
    # one buffer, never zeroed again: nothing a call leaves behind reaches the next one
    buf = torch.full((GUARD + biggest + GUARD,), 0xA7, dtype=torch.uint8, device=dev)
    ws = _GuardedWorkspace(buf)
    large, small = (65, 130), (2, 40)
    for key in (large, small, None, small, large):
        if key is None:
            args, kw, _ = shapes[small]
            name, y0, u, theta, rules, w = args[:6]
            res = _run(dev, name, y0[:0], u[:0], theta[:0], rules, w[:0], *args[6:], workspace=ws,
                       **dict(kw, group=kw["group"][:0]))
            assert np.all(res["sums"] == 0) and ws.asked[-1] == 0
            continue
        args, kw, need = shapes[key]
        _same(_run(dev, *args, workspace=ws, **kw), want[key])
        assert ws.asked[-1] == need
    assert bool((buf[:GUARD] == 0xA7).all()) and bool((buf[GUARD + biggest:] == 0xA7).all())


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
    """[S, 3 + Q, G] of a RuleValueResult."""
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def test_plugin_rule_value(dev, model):
    """``rule_value`` is ``ops.rule_value`` on the plugin's inputs after the stated unit change, its assignment is
    ``evaluate_rules``' choice, it agrees with the restatement, the personalised gain and the optimism are >= 0, and
    groups split the cohort."""
    import torch
    from insite_amd import effect, ops
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    prev, stat, _, _ = model._unscaled_inputs(tr)
    N, T = tr.data["current_treatments"].shape[:2]
    z0 = (prev[:, 0].cpu().numpy() - mean) / std
    TR = effect.ThresholdRule
    rules = [TR(on=float(np.median(z0))), TR(on=z0 * 0.9, off=z0 * 0.6, every=2, start_on=True),
             TR(on=-1e9, arm_on=0, arm_off=1)]
    costs, arm_costs = [0.0, 0.02, -0.01], [0.0, 0.003]
    K = 3
    res = model.rule_value(tr, rules, objective="mean", costs=costs, arm_costs=arm_costs)
    assert res.series == effect.rule_value_series(K) and res.q == q and res.n_rules == K
    ev = model.evaluate_rules(tr, rules, objective="mean", costs=costs, arm_costs=arm_costs)
    assert np.array_equal(res.assign.cpu().numpy(), ev.choice.cpu().numpy())
    th = np.empty((N, 2 * K))
    th[:, 0] = th[:, 1] = np.median(z0)
    th[:, 2], th[:, 3] = z0 * 0.9, z0 * 0.6
    th[:, 4] = th[:, 5] = -1e9
    th = th * std + mean
    table = np.array([(1, 0, 1, 0), (1, 0, 2, 1), (0, 1, 1, 0)], dtype=np.int32)
    ae = tr.data["active_entries"][..., 0].astype(np.float64)
    w = ae / ae.sum(axis=1, keepdims=True)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    t = functools.partial(_t, dev)
    out, fixwin, bf, assign, sums, wsum = ops.rule_value(
        prev[:, 0].contiguous(), stat, t(th), table, t(coef), model.library, model.dt, q, t(w),
        cost=t(np.array(costs) * std), arm_cost=np.array(arm_costs) * std, weighting="poisson", seed=3,
        method=model.integrator, drop_below=0.0, T=T)
    torch.cuda.synchronize()
    S_ = 3 * K + 9
    assert res.point.shape == (S_, 1) and res.quantiles.shape == (S_, 3, 1)
    assert res.fixwin.shape == (1, K) and res.weight_sum.shape == (33, 1)
    assert res.share["point"].shape == (K, 1) and res.exposure["point"].shape == (K + 3, 1)
    o = out.cpu().numpy().transpose(1, 2, 0)                      # [S, 3 + Q, G]
    want = o.copy()
    want[:K + 6] = o[:K + 6] / std
    want[:K + 3, [0, 1, 3, 4, 5]] = (o[:K + 3, [0, 1, 3, 4, 5]] - mean * 1.0) / std
    assert np.allclose(_stack(res), want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(res.fixwin.cpu().numpy(), fixwin.cpu().numpy())
    assert np.array_equal(res.best_fixed.cpu().numpy(), bf.cpu().numpy())
    # against the restatement
    ref = V.rule_value(prev[:, 0].cpu().numpy(), stat.cpu().numpy(), th, table, coef, R.poly_library(3, 2, True),
                       model.dt, q, w, np.array(costs) * std, np.array(arm_costs) * std, 1, None, None, 1, "poisson",
                       3, 0, "euler5")
    got = dict(zip(KEYS, (a.cpu().numpy() for a in (out, fixwin, bf, assign, sums, wsum))))
    _check_against(got, ref, K, T, "plugin: ")
    # rule 2 is always on (arm 0): its exposure is T in every replicate
    assert np.all(res["exposure_2"]["point"].cpu().numpy() == T) and np.all(res["exposure_2"]["std"].cpu().numpy() == 0)
    for name in ("gain_personalised", "optimism"):
        assert (res[name]["point"] >= 0).all() and (res[name]["quantiles"] >= 0).all(), name
    assert (res["gain_assigned"]["point"] >= 0).all()
    assert float(res["optimism"]["point"]) == 0.0
    assert abs(float(res.share["point"].sum()) - 1.0) <= 1e-12
    # a given assignment, groups and the weightings
    grp = (np.arange(N) % 3) - 1                                     # -1 excludes a third of the rows
    rg = model.rule_value(tr, rules, assignment=ev.choice.cpu().numpy(), costs=costs, arm_costs=arm_costs, groups=grp,
                          resample=None)
    assert rg.point.shape == (S_, 2) and (rg.weight_sum.cpu().numpy() == np.array([67.0, 66.0])).all()
    assert (rg["gain_personalised"]["point"] >= 0).all() and np.all(rg["optimism"]["point"].cpu().numpy() == 0.0)
    ind = model.rule_value(tr, rules[:2], objective="terminal", resample="independent", seed=11, maximize=True)
    assert (ind["gain_personalised"]["point"] >= 0).all() and ind.assign.shape == (N,)
    with pytest.raises(ValueError):
        model.rule_value(tr, [TR(0.0, arm_on=2)])
    with pytest.raises(ValueError):
        model.rule_value(tr, rules, assignment=np.full(N, 3))
