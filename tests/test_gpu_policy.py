"""GPU tests of the policy value (include/insite_policy.h: policy_rule_kernel, policy_sums_kernel,
policy_finalize_kernel, ops.policy_value, SINDY.policy_value) against the numpy restatement tests/policy_ref.py.

Tolerance: the continuous outputs within TOL s_g of the restatement, s_g = max over replicates, rows of the group and
plans of (|cost_j| + sum_k |w| |y|): the bar of tests/test_gpu_cohort_effect.py and tests/test_gpu_regimen.py for this
arithmetic (a weighted mean of objectives is no larger than the largest, and every statistic is Lipschitz with
constant <= 2 in the sup norm of the replicate values).  The shares within 1e-12 absolute.  ``wsum``, the allocation
columns of ``sums``, ``rule``, ``best_fixed`` and ``fixwin`` are compared exactly: tests/test_policy_abi.py asserts
that every argmin behind them has a margin of at least 1e-8 of its scale, a hundred times the bar.

Worst |got - ref| / s_g over the parity cases on an MI355X: 1.2e-14, shares 1.4e-14 absolute.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cohort_effect_ref as CR  # noqa: E402
import library_matrix as M  # noqa: E402
import policy_ref as P  # noqa: E402
import regimen_ref as G  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, TOL_SHARE = 1e-10, 1e-12
DT, Q5, Q16 = P.DT, P.Q5, P.Q16


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _run(dev, name, y0, u, plans, w, cost, coef, q, method, sub, T, sense=1, rule=None, group=None, Gn=1,
         weighting="none", seed=P.SEED, off=0, pad_out=0):
    """dict(out [G, 2 K + 6, 3 + Q], fixwin, best_fixed, rule, sums, wsum, pad: the padding of out or None)."""
    import torch
    from insite_amd import ops
    t = functools.partial(_t, dev)
    K, NS = plans.shape[0], 3 + len(q)
    out = buf = None
    if pad_out:
        buf = torch.full((Gn, 2 * K + 6, NS + pad_out), P.POISON, dtype=torch.float64, device=dev)
        out = buf[:, :, :NS]
    got = ops.policy_value(t(y0), t(u), t(plans), t(coef), M.LIBS[name], DT, q, t(w), cost=t(cost), maximize=sense < 0,
                           rule=t(rule), group=t(group), n_groups=Gn, weighting=weighting, seed=seed,
                           patient_offset=off, method=method, substeps=sub, drop_below=M.DROP_BELOW, T=T, out=out)
    torch.cuda.synchronize()
    if pad_out:
        assert got[0] is out
    res = dict(zip(("out", "fixwin", "best_fixed", "rule", "sums", "wsum"), (a.cpu().numpy() for a in got)))
    res["pad"] = None if buf is None else buf[:, :, NS:].cpu().numpy()
    return res


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


def _worst(res, ref, K):
    """(the worst relative error of the continuous series of out and of the continuous columns of sums, the worst
    absolute error of the share series)."""
    s = ref["scale"]
    cont = _rel(res["out"][:, :K + 6], ref["out"][:, :K + 6], s[:, None, None])
    sm = _rel(res["sums"][:, :, :K + 2], ref["sums"][:, :, :K + 2], (s[None, :] * ref["wsum"])[:, :, None])
    share = _rel(res["out"][:, K + 6:], ref["out"][:, K + 6:], 1.0)
    return max(cont, sm), share


def _check_exact_sums(res, K, sense):
    """The header's inequalities and the allocation identity on the returned sums, with no tolerance."""
    S, ws = res["sums"], res["wsum"]
    s = float(sense)
    ok = ~np.isnan(S[:, :, :K + 2]).any(axis=2)
    for j in range(K):
        assert (s * S[:, :, K] <= s * S[:, :, j])[ok].all(), j
    assert (s * S[:, :, K] <= s * S[:, :, K + 1])[ok].all()
    assert np.array_equal(S[:, :, K + 2:].sum(axis=2)[ok], ws[ok])
    assert np.array_equal(S[:, :, K + 2:], np.round(S[:, :, K + 2:])) and np.array_equal(ws, np.round(ws))
    # so the personalised gain and the optimism are >= 0 in every statistic that is a value of some replicate
    # (gain_rule has no such bound: a given rule may be worse than the best fixed plan)
    loc = [0] + list(range(3, res["out"].shape[2]))
    d = res["out"][:, [K + 3, K + 5]][:, :, loc]
    assert (np.nan_to_num(d, nan=0.0) >= 0).all()


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_parity(dev, case):
    (Rn, N, T, A, K, Gn, name, method, sub, q, _, _, _, sense, weighting, off, _, _, _) = case
    y0, u, plans, w, cost, coef, group, rule, ref = P.case(*case)
    kw = dict(sense=sense, rule=rule, group=group, Gn=Gn, weighting=weighting, off=off)
    res = _run(dev, name, y0, u, plans, w, cost, coef, q, method, sub, T, pad_out=P.PAD_OUT, **kw)
    assert res["out"].shape == (Gn, 2 * K + 6, 3 + len(q)) and res["sums"].shape == (Rn, Gn, 2 * K + 2)
    assert res["fixwin"].shape == (Gn, K) and res["best_fixed"].shape == (Gn,) and res["rule"].shape == (N,)
    assert np.all(res["pad"] == P.POISON)
    worst, share = _worst(res, ref, K)
    print(f"worst |got - ref| / s_g = {worst:.3e}, shares abs {share:.3e}")
    assert np.array_equal(res["wsum"], ref["wsum"])
    assert np.array_equal(res["sums"][:, :, K + 2:], ref["sums"][:, :, K + 2:])
    assert np.array_equal(res["rule"], ref["rule"])
    assert np.array_equal(res["best_fixed"], ref["best_fixed"])
    assert np.array_equal(_bits(res["fixwin"]), _bits(ref["fixwin"]))
    assert worst <= TOL
    assert share <= TOL_SHARE
    _check_exact_sums(res, K, sense)
    if Rn == 2:
        assert np.isnan(res["out"][..., 2]).all()
    # the out-of-range arms and the NaN weights past T are never read: unpadded inputs give the same bits
    r2 = _run(dev, name, y0, u, plans[..., :T], w[..., :T], cost, coef, q, method, sub, T, **kw)
    for key in ("out", "fixwin", "sums", "wsum"):
        assert np.array_equal(_bits(r2[key]), _bits(res[key])), key
    assert np.array_equal(r2["rule"], res["rule"]) and np.array_equal(r2["best_fixed"], res["best_fixed"])


EXACT = [(2, 3, 33, 2, 3, 1, "std7"), (65, 130, 65, 4, 4, 3, "lin3"), (130, 200, 18, 2, 8, 3, "std7"),
         (300, 70, 33, 2, 16, 2, "u3_first9")]


@functools.lru_cache(maxsize=None)
def _exact_inputs(Rn, N, T, A, K, Gn, name):
    out = P.inputs(("policy-exact", Rn, N, T, A, K, Gn, name), Rn, N, T, A, K, Gn, name)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("Rn,N,T,A,K,Gn,name", EXACT)
def test_exact_properties(dev, Rn, N, T, A, K, Gn, name):
    y0, u, plans, w, cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    run = functools.partial(_run, dev, name, y0, u)
    args = (coef, Q5, "euler", 5, T)
    kw = dict(group=group, Gn=Gn, weighting="poisson", off=3)
    for sense in (1, -1):
        r0 = run(plans, w, cost, *args, sense=sense, **kw)
        _check_exact_sums(r0, K, sense)
        # two calls are bitwise equal
        r1 = run(plans, w, cost, *args, sense=sense, **kw)
        for key in ("out", "fixwin", "sums", "wsum"):
            assert np.array_equal(_bits(r0[key]), _bits(r1[key])), key
        assert np.array_equal(r0["rule"], r1["rule"]) and np.array_equal(r0["best_fixed"], r1["best_fixed"])
        # a constant rule j reproduces column j bit for bit, and changes nothing else
        for j in (0, K - 1):
            rj = run(plans, w, cost, *args, sense=sense, rule=np.full(N, j, dtype=np.int32), **kw)
            assert np.array_equal(_bits(rj["sums"][:, :, K + 1]), _bits(rj["sums"][:, :, j])), j
            keep = [c for c in range(2 * K + 2) if c != K + 1]
            assert np.array_equal(_bits(rj["sums"][:, :, keep]), _bits(r0["sums"][:, :, keep]))
            assert np.array_equal(_bits(rj["out"][:, K + 1]), _bits(rj["out"][:, j]))
        # K = 1: the personalised, rule and value_0 columns are the same bits, the three differences exactly +0
        k1 = run(plans[:1], w, cost[:1], *args, sense=sense, **kw)
        assert np.array_equal(_bits(k1["sums"][:, :, 1]), _bits(k1["sums"][:, :, 0]))
        assert np.array_equal(_bits(k1["sums"][:, :, 2]), _bits(k1["sums"][:, :, 0]))
        assert np.array_equal(k1["sums"][:, :, 3], k1["wsum"]) and np.all(k1["rule"] == 0)
        ok = (k1["wsum"] > 0).all(axis=0)                       # groups that every replicate drew
        d = np.delete(k1["out"][ok][:, 4:7], 2, axis=-1)
        assert np.all(_bits(d) == 0)
        assert np.all(k1["fixwin"][ok] == 1.0) and np.all(k1["best_fixed"][ok] == 0)
        assert np.array_equal(_bits(k1["out"][:, 0]), _bits(r0["out"][:, 0]))
    # identical plans (and costs) put every vote on plan 0
    same = run(np.repeat(plans[:1], K, axis=0), w, np.repeat(cost[:1], K), *args, **kw)
    assert np.all(same["sums"][:, :, K + 3:] == 0) and np.array_equal(same["sums"][:, :, K + 2], same["wsum"])
    assert np.all(same["rule"] == 0)
    ok = (same["wsum"] > 0).all(axis=0)
    assert np.all(same["best_fixed"][ok] == 0) and np.all(same["fixwin"][ok][:, 0] == 1.0)
    for c in range(1, K + 2):
        assert np.array_equal(_bits(same["sums"][:, :, c]), _bits(same["sums"][:, :, 0])), c


def test_rules(dev):
    """A zero-weight or excluded row with NaN y0 and u reaches nothing; a NaN replicate poisons exactly what the
    header says; a replicate that drew no row gives 0 / 0 = NaN; a rule of -1 or K makes the rule column NaN and
    nothing else."""
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, plans, w, cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    run = functools.partial(_run, dev, name)
    args = (Q5, "rk4", 1, T)
    kw = dict(group=group, Gn=Gn, weighting="poisson", off=0)
    r0 = run(y0, u, plans, w, cost, coef, *args, **kw)
    om = CR.weights("poisson", P.SEED, Rn, N, 0)
    assert not np.isnan(r0["out"]).any()
    # row 5 is excluded by its group, row 6 only counts in the replicates that drew it: NaN inputs of row 5 change
    # nothing; NaN inputs of row 6 reach exactly the replicates with omega > 0 (replicate 0 among them)
    g2 = np.array(group)
    g2[5], g2[6] = -1, 1
    base = run(y0, u, plans, w, cost, coef, *args, **dict(kw, group=g2))
    yn, un = y0.copy(), u.copy()
    yn[5], un[5] = np.nan, np.nan
    rn = run(yn, un, plans, w, cost, coef, *args, **dict(kw, group=g2))
    assert rn["rule"][5] == -1
    for key in ("out", "fixwin", "sums", "wsum"):
        assert np.array_equal(_bits(rn[key]), _bits(base[key])), key
    yn[6] = np.nan
    rn = run(yn, un, plans, w, cost, coef, *args, **dict(kw, group=g2))
    hit = om[:, 6] > 0
    assert hit[0] and not hit.all()
    assert np.isnan(rn["sums"][hit, 1, :K + 2]).all()
    assert np.array_equal(_bits(rn["sums"][~hit]), _bits(base["sums"][~hit]))
    assert np.array_equal(_bits(rn["sums"][:, [0, 2]]), _bits(base["sums"][:, [0, 2]]))
    assert np.array_equal(rn["wsum"], base["wsum"])
    # a NaN replicate: its value, personalised and rule sums are NaN, it allocates nothing and votes for no fixed
    # plan; every statistic but the point of the first K + 6 series is NaN, the shares stay finite
    cn = coef.copy()
    cn[Rn - 2] = np.nan
    rn = run(y0, u, plans, w, cost, cn, *args, **kw)
    assert np.isnan(rn["sums"][Rn - 2, :, :K + 2]).all() and np.all(rn["sums"][Rn - 2, :, K + 2:] == 0)
    others = np.arange(Rn) != Rn - 2
    assert np.array_equal(_bits(rn["sums"][others]), _bits(r0["sums"][others]))
    assert np.isnan(rn["out"][:, :K + 6, 1:]).all() and np.isfinite(rn["out"][:, K + 6:]).all()
    assert np.array_equal(_bits(rn["out"][..., 0]), _bits(r0["out"][..., 0]))
    assert np.array_equal(rn["best_fixed"], r0["best_fixed"]) and np.array_equal(rn["rule"], r0["rule"])
    assert np.allclose(rn["fixwin"].sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=4e-16)
    # NaN in one coefficient of arm 1, and plan 0 never uses arm 1 (the others start with it): value_0 stays finite,
    # the replicate abstains for every row
    ca = coef.copy()
    ca[Rn - 2, 1, 1] = np.nan
    pa = plans.copy()
    pa[0] = 0
    pa[1:, ..., 0] = 1
    rn = run(y0, u, pa, w, cost, ca, *args, **kw)
    ref = P.policy(y0, u, G.full_plans(pa, N, T), ca, M.exps_of(name), DT, Q5, w[..., :T], cost, 1, None, group, Gn,
                   "poisson", P.SEED, 0, "rk4", 1)
    assert np.isfinite(rn["out"][:, 0]).all() and np.isnan(rn["out"][:, 1:K, 1:]).all()
    assert np.isnan(rn["out"][:, K, 1:]).all() and np.isnan(rn["out"][:, K + 2:K + 6, 1:]).all()
    assert np.all(rn["sums"][Rn - 2, :, K + 2:] == 0)
    assert np.array_equal(rn["rule"], ref["rule"]) and np.array_equal(rn["best_fixed"], ref["best_fixed"])
    assert max(_worst(rn, ref, K)) <= TOL
    # an empty replicate: group 2 holds row 9 alone, which some replicate did not draw
    g3 = np.where(np.array(group) == 2, -1, group)
    g3[9] = 2
    assert (om[1:, 9] == 0).any()
    rn = run(y0, u, plans, w, cost, coef, *args, **dict(kw, group=g3))
    assert np.array_equal(rn["wsum"][:, 2], om[:, 9].astype(float))
    assert np.isnan(rn["out"][2, :, 1:]).all() and np.isfinite(rn["out"][2, :, 0]).all()
    assert np.isfinite(rn["out"][:2]).all()
    # a rule value of -1 or K: the rule column is NaN wherever the row has weight, and nothing else changes
    for bad in (-1, K):
        rl = r0["rule"].copy()
        p = int(np.nonzero(np.array(group) == 1)[0][0])
        rl[p] = bad
        rb = run(y0, u, plans, w, cost, coef, *args, rule=rl, **kw)
        hit = om[:, p] > 0
        assert np.isnan(rb["sums"][hit, 1, K + 1]).all() and hit[0]
        assert np.array_equal(_bits(rb["sums"][~hit]), _bits(r0["sums"][~hit]))
        keep = [c for c in range(2 * K + 2) if c != K + 1]
        assert np.array_equal(_bits(rb["sums"][:, :, keep]), _bits(r0["sums"][:, :, keep]))
        assert np.array_equal(_bits(rb["sums"][:, [0, 2]]), _bits(r0["sums"][:, [0, 2]]))
        ser = [s for s in range(2 * K + 6) if s not in (K + 1, K + 4, K + 5)]
        assert np.array_equal(_bits(rb["out"][:, ser]), _bits(r0["out"][:, ser]))
        assert np.isnan(rb["out"][1, [K + 1, K + 4, K + 5]]).all()


def test_no_rows_and_arguments(dev):
    """n_rows = 0 is a successful no-op (fresh sums stay zero); ``plan_policy_value`` repeats bit for bit; shape and
    argument errors."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, plans, w, cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    for pl, ww in ((plans[:, :0], w[:0]), (plans[:, 0], w[0])):
        res = _run(dev, name, y0[:0], u[:0], pl, ww, cost, coef, Q5, "euler", 5, T, group=group[:0], Gn=Gn)
        assert res["rule"].shape == (0,) and np.all(res["sums"] == 0) and np.all(res["wsum"] == 0)
    r0 = _run(dev, name, y0, u, plans, w, cost, coef, Q5, "euler", 5, T, group=group, Gn=Gn, weighting="poisson")
    t = functools.partial(_t, dev)
    lib = M.LIBS[name]
    ty0, tu, tp, tw, tc, tcoef, tg = t(y0), t(u), t(plans), t(w), t(cost), t(coef), t(group)
    kw = dict(cost=tc, group=tg, n_groups=Gn, seed=P.SEED, method="euler", substeps=5, drop_below=M.DROP_BELOW, T=T)
    plan = ops.plan_policy_value(ty0, tu, tp, tcoef, lib, DT, Q5, tw, **kw)
    for _ in range(2):
        got = plan()
        torch.cuda.synchronize()
        for key, a in zip(("out", "fixwin", "best_fixed", "rule", "sums", "wsum"), got):
            assert np.array_equal(a.cpu().numpy(), r0[key], equal_nan=True), key
        got[0].zero_()
        got[4].zero_()
    for bad in (dict(rule=t(np.zeros(N - 1, dtype=np.int32))), dict(rule=t(np.zeros(N, dtype=np.int64))),
                dict(group=tg[:5]), dict(n_groups=65), dict(n_groups=0), dict(weighting="binomial"),
                dict(seed=-1), dict(patient_offset=-1), dict(method="heun"), dict(cost=tc[:2]), dict(T=T + 10),
                dict(out=torch.zeros((Gn, 2 * K + 5, 3 + len(Q5)), dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            ops.policy_value(ty0, tu, tp, tcoef, lib, DT, Q5, tw, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ops.policy_value(ty0, tu, tp, tcoef, lib, DT, (0.5, 1.5), tw, **kw)
    with pytest.raises(ValueError):
        ops.policy_value(ty0, tu, tp.repeat(5, 1, 1), tcoef, lib, DT, Q5, tw, T=T)             # 20 plans
    with pytest.raises(ValueError):
        ops.policy_value(ty0, tu, tp, tcoef[:1], lib, DT, Q5, tw, **kw)                        # no resample


@pytest.mark.parametrize("split", [64, 37])
def test_shards_and_finalize_alone(dev, split):
    """Two shards (an even and an odd split) with ``patient_offset`` add to the whole: wsum and the allocation
    exactly, the values within the bar; ``policy_finalize`` on the added sums, and on the restatement's sums, gives
    the whole cohort's statistics."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, Gn, name = 65, 130, 65, 4, 4, 3, "lin3"
    y0, u, plans, w, cost, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    off = 1000
    ref = P.policy(y0, u, G.full_plans(plans, N, T), coef, M.exps_of(name), DT, Q5, w[..., :T], cost, -1, None, group,
                   Gn, "poisson", P.SEED, off, "euler", 5)
    whole = _run(dev, name, y0, u, plans, w, cost, coef, Q5, "euler", 5, T, sense=-1, group=group, Gn=Gn,
                 weighting="poisson", off=off)
    t = functools.partial(_t, dev)
    lib = M.LIBS[name]
    parts = []
    for lo, hi in ((0, split), (split, N)):
        parts.append(ops.policy_sums(t(y0[lo:hi]), t(u[lo:hi]), t(plans[:, lo:hi]), t(coef), lib, DT, t(w[lo:hi]),
                                     cost=t(cost), maximize=True, group=t(group[lo:hi]), n_groups=Gn,
                                     weighting="poisson", seed=P.SEED, patient_offset=off + lo, method="euler",
                                     substeps=5, drop_below=M.DROP_BELOW, T=T))
    sums, wsum = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    rule = torch.cat([parts[0][2], parts[1][2]]).cpu().numpy()
    assert np.array_equal(rule, whole["rule"]) and np.array_equal(rule, ref["rule"])
    assert np.array_equal(wsum.cpu().numpy(), whole["wsum"])
    assert np.array_equal(sums.cpu().numpy()[:, :, K + 2:], whole["sums"][:, :, K + 2:])
    out, fixwin, bf = (a.cpu().numpy() for a in ops.policy_finalize(sums, wsum, Q5, maximize=True))
    got = {"out": out, "sums": sums.cpu().numpy()}
    worst, share = _worst(got, ref, K)
    print(f"shards at {split}: worst |got - ref| / s_g = {worst:.3e}")
    assert worst <= TOL and share <= TOL_SHARE
    assert np.array_equal(bf, ref["best_fixed"]) and np.array_equal(_bits(fixwin), _bits(ref["fixwin"]))
    assert _rel(out[:, :K + 6], whole["out"][:, :K + 6], ref["scale"][:, None, None]) <= TOL
    # finalize alone on the restatement's sums
    out, fixwin, bf = (a.cpu().numpy() for a in ops.policy_finalize(t(ref["sums"]), t(ref["wsum"]), Q5, maximize=True))
    assert _rel(out[:, :K + 6], ref["out"][:, :K + 6], ref["scale"][:, None, None]) <= TOL
    assert _rel(out[:, K + 6:], ref["out"][:, K + 6:], 1.0) <= TOL_SHARE
    assert np.array_equal(bf, ref["best_fixed"]) and np.array_equal(_bits(fixwin), _bits(ref["fixwin"]))
    # and finalize of the whole call's own sums is the whole call's out, bit for bit
    out, fixwin, bf = (a.cpu().numpy() for a in ops.policy_finalize(t(whole["sums"]), t(whole["wsum"]), Q5,
                                                                    maximize=True))
    assert np.array_equal(_bits(out), _bits(whole["out"])) and np.array_equal(_bits(fixwin), _bits(whole["fixwin"]))


@pytest.mark.parametrize("Rn,N,T,A,K,name,sense", [(65, 130, 65, 4, 4, "lin3", 1), (512, 70, 18, 2, 8, "std7", -1)])
def test_agrees_with_regimen_choice(dev, Rn, N, T, A, K, name, sense):
    """With weighting NONE and one group: the summed allocation of the resampled replicates is (R - 1) times the
    summed ``win`` of ``ops.regimen_choice``, exactly; the rule is its ``choice``; the point value of value_j is the
    row mean of its point objective."""
    import torch
    from insite_amd import ops
    y0, u, plans, w, cost, coef, _, _ = _exact_inputs(Rn, N, T, A, K, 1, name)
    res = _run(dev, name, y0, u, plans, w, cost, coef, Q5, "euler", 5, T, sense=sense)
    t = functools.partial(_t, dev)
    choice, win, out = ops.regimen_choice(t(y0), t(u), t(plans), t(coef), M.LIBS[name], DT, Q5, t(w), cost=t(cost),
                                          maximize=sense < 0, method="euler", substeps=5, drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    choice, win, out = choice.cpu().numpy(), win.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(res["rule"], choice)
    votes = np.rint(win * (Rn - 1))
    assert np.array_equal(votes / (Rn - 1), win)
    assert np.array_equal(res["sums"][1:, 0, K + 2:].sum(axis=0), votes.sum(axis=0))
    scale = np.abs(out[:, :, 0, 0]).max()
    assert np.max(np.abs(res["out"][0, :K, 0] - out[:, :, 0, 0].mean(axis=0))) <= TOL * scale
    # the point value of the rule series: the mean of every row's chosen objective
    pick = out[np.arange(N), choice, 0, 0]
    assert abs(res["out"][0, K + 1, 0] - pick.mean()) <= TOL * scale
    assert abs(res["out"][0, K, 0] - pick.mean()) <= TOL * scale


def test_agrees_with_cohort_effect(dev):
    """With a terminal unit weight and no cost, every statistic of value_j is ``ops.cohort_effect``'s single-plan
    output at step T - 1."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, K, Gn, name = 130, 200, 18, 2, 8, 3, "std7"
    y0, u, plans, _, _, coef, group, _ = _exact_inputs(Rn, N, T, A, K, Gn, name)
    w = np.zeros(T)
    w[T - 1] = 1.0
    res = _run(dev, name, y0, u, plans[..., :T], w, None, coef, Q5, "rk4", 1, T, group=group, Gn=Gn,
               weighting="poisson", off=5)
    t = functools.partial(_t, dev)
    for j in (0, 3, K - 1):
        arm = t(plans[j][:, :T])
        out, _, wsum = ops.cohort_effect(t(y0), t(u), arm, None, t(coef), M.LIBS[name], DT, Q5, group=t(group),
                                         n_groups=Gn, weighting="poisson", seed=P.SEED, patient_offset=5,
                                         method="rk4", substeps=1, drop_below=M.DROP_BELOW, T=T)
        torch.cuda.synchronize()
        want = out.cpu().numpy()[:, 0, :, T - 1]                  # [G, 3 + Q]
        assert np.array_equal(wsum.cpu().numpy(), res["wsum"])
        # the scale: the largest |y[T - 1]| over the replicates and rows, from the restatement's trajectories
        scale = np.abs(G.trajectories(y0, u, plans[j][:, :T], coef, M.exps_of(name), DT, "rk4", 1)[:, :, T - 1]).max()
        assert np.max(np.abs(res["out"][:, j] - want)) <= TOL * scale, j


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
    """[S, 3 + Q, G] of a PolicyValueResult."""
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def test_plugin_policy_value(dev, model):
    """``policy_value([None, 0, 1])`` is ``ops.policy_value`` on the plugin's inputs after the stated unit change, its
    rule is ``choose_plan``'s choice, the personalised gain and the optimism are >= 0, and groups split the cohort."""
    import torch
    from insite_amd import effect, ops
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    costs = [0.0, 0.02, -0.01]
    K = 3
    res = model.policy_value(tr, [None, 0, 1], objective="mean", costs=costs)
    assert res.series == effect.policy_series(K) and res.q == q and res.n_plans == K
    assert res.series[K:K + 6] == ("personalised", "rule", "best_fixed", "gain_personalised", "gain_rule", "optimism")
    ch = model.choose_plan(tr, [None, 0, 1], objective="mean", costs=costs)
    assert np.array_equal(res.rule.cpu().numpy(), ch.choice.cpu().numpy())
    prev, stat, _, _ = model._unscaled_inputs(tr)
    arms = np.argmax(tr.data["current_treatments"], axis=-1).astype(np.int8)
    N, T = arms.shape
    plans = np.stack([arms, np.zeros_like(arms), np.ones_like(arms)])
    ae = tr.data["active_entries"][..., 0].astype(np.float64)
    w = ae / ae.sum(axis=1, keepdims=True)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    t = functools.partial(_t, dev)
    out, fixwin, bf, rule, sums, wsum = ops.policy_value(
        prev[:, 0].contiguous(), stat, t(plans), t(coef), model.library, model.dt, q, t(w),
        cost=t(np.array(costs) * std), weighting="poisson", seed=3, method=model.integrator, drop_below=0.0, T=T)
    torch.cuda.synchronize()
    assert res.point.shape == (2 * K + 6, 1) and res.quantiles.shape == (2 * K + 6, 3, 1)
    assert res.fixwin.shape == (1, K) and res.weight_sum.shape == (33, 1) and res.share["point"].shape == (K, 1)
    o = out.cpu().numpy().transpose(1, 2, 0)                      # [S, 3 + Q, G]
    want = o.copy()
    want[:K + 6] = o[:K + 6] / std
    want[:K + 3, [0, 1, 3, 4, 5]] = (o[:K + 3, [0, 1, 3, 4, 5]] - mean * 1.0) / std
    assert np.allclose(_stack(res), want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(res.fixwin.cpu().numpy(), fixwin.cpu().numpy())
    assert np.array_equal(res.best_fixed.cpu().numpy(), bf.cpu().numpy())
    # against the restatement
    ref = P.policy(prev[:, 0].cpu().numpy(), stat.cpu().numpy(), plans, coef, R.poly_library(3, 2, True), model.dt, q,
                   w, np.array(costs) * std, 1, None, None, 1, "poisson", 3, 0, "euler5")
    got = {"out": out.cpu().numpy(), "sums": sums.cpu().numpy()}
    worst, share = _worst(got, ref, K)
    print(f"worst |got - ref| / s_g = {worst:.3e}")
    assert worst <= TOL and share <= TOL_SHARE and np.array_equal(rule.cpu().numpy(), ref["rule"])
    # the personalised gain and the optimism are >= 0 in the point model and in every quantile (gain_rule only in the
    # point model, where the rule is the personalised choice itself); with the point model's own
    # rule the point optimism is exactly 0
    for name in ("gain_personalised", "optimism"):
        assert (res[name]["point"] >= 0).all() and (res[name]["quantiles"] >= 0).all(), name
    assert (res["gain_rule"]["point"] >= 0).all()
    assert float(res["optimism"]["point"]) == 0.0
    assert abs(float(res.share["point"].sum()) - 1.0) <= 1e-12
    # a given rule, groups and the weightings
    grp = (np.arange(N) % 3) - 1                                     # -1 excludes a third of the rows
    rg = model.policy_value(tr, [None, 0, 1], rule=ch.choice.cpu().numpy(), costs=costs, groups=grp, resample=None)
    assert rg.point.shape == (2 * K + 6, 2) and (rg.weight_sum.cpu().numpy() == np.array([67.0, 66.0])).all()
    assert (rg["gain_personalised"]["point"] >= 0).all() and np.all(rg["optimism"]["point"].cpu().numpy() == 0.0)
    ind = model.policy_value(tr, [0, 1], objective="terminal", resample="independent", seed=11, maximize=True)
    assert (ind["gain_personalised"]["point"] >= 0).all() and ind.rule.shape == (N,)
    with pytest.raises(ValueError):
        model.policy_value(tr, [0, 2])
    with pytest.raises(ValueError):
        model.policy_value(tr, [0, 1], rule=np.full(N, 2))
