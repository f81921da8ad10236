"""GPU tests of the ensemble score (include/insite_score.h: score_sums_kernel, ops.ensemble_score,
SINDY.score_bands) against the numpy restatement tests/score_ref.py.

Tolerance.  The count rows (scored, bad, the rank histogram, covered) are exactly the restatement's.  Every other
row is within TOL times the per-cell bound summed over the cells it adds: 4 s'^2 for the squared errors and the
variance, 2 s' for the CRPS and the width, (2 + 2 c) s' for the interval score, s' = max(max_r |v_r|, |y|) at the
cell -- tests/test_gpu_effect.py's bar (ten times the project's 1e-11 rollout bar) and its Lipschitz argument, applied
cell by cell.  A count can only be exact where no decision hangs on a rounding: before either side runs, the helper
marks every cell whose decision margin (tests/score_ref.py) is below 1e-6 inactive, and the test asserts that this
removed at most 1 % of the observed cells.

Ties.  With dt = 0 the Euler interval map is y <- fma(1, y, 0): every replicate reproduces y0 bit for bit, so the
tie case is built that way and not from identical replicates.
"""
import functools
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
import score_ref as SR  # noqa: E402
from oracle import cancer_sim_ref as CS  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
MARGIN = 1e-6
DT = 0.1
PAD, POISON = 3, -7.25
L1, L3 = (0.9,), (0.5, 0.9, 0.95)
L8 = (0.5, 0.1, 0.99, 0.8, 0.3, 0.95, 0.9, 0.7)      # unsorted

# a sample of R x N x T x n_arms x table x method x substeps x levels x bins x groups (not the product): every V
# (R <= 64, 128, 256, 512) and partly filled top slots (65, 129, 200), n = 1 (R = 2), one row, a few and more than a
# wave's worth, several rows per chunk (N = 5000: chunks of 2 rows), T across the 64-step window, 1 to 64 groups
CASES = [
    (2, 3, 1, 1, "x_only", "euler", 1, L1, 1, 1),
    (3, 1, 2, 2, "bias_x", "rk4", 1, L3, 10, 1),
    (17, 130, 17, 2, "std7", "euler", 5, L3, 10, 3),
    (64, 3, 33, 4, "noone3", "rk4", 5, L8, 32, 1),
    (65, 3, 70, 2, "lin3", "euler", 5, L3, 10, 64),
    (129, 130, 2, 1, "dup4", "rk4", 1, L1, 32, 3),
    (200, 3, 70, 2, "std7", "rk4", 1, L8, 10, 1),
    (512, 3, 33, 4, "u3_x9", "euler", 5, L3, 10, 3),
    (512, 1, 17, 2, "high_pow", "rk4", 5, L8, 32, 1),
    (2, 5000, 2, 2, "std7", "euler", 1, L1, 10, 3),
]
IDS = [f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-{c[4]}-{c[5]}{c[6]}-L{len(c[7])}-B{c[8]}-G{c[9]}" for c in CASES]


def _arms(rng, N, T, A):
    """tests/test_gpu_effect.py's plan: random per-step arms with a switch at step 1 and at step T - 1; the columns
    past T hold out-of-range arms."""
    arm = rng.integers(0, A, (N, T + PAD))
    if A > 1 and T >= 2:
        arm[:, 1] = (arm[:, 0] + 1) % A
        arm[:, T - 1] = (arm[:, T - 2] + 1) % A
    arm[:, T:] = [A + 3, -2, 127][:PAD]
    return arm.astype(np.int8)


def _coef(rng, name, Rn, A):
    """tests/test_gpu_effect.py's ensemble: a decaying model and bootstrap-like replicates of it whose trajectories
    cross."""
    exps = M.exps_of(name)
    F = exps.shape[0]
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[rng.random((Rn, A, F)) < 0.2] = 0.0
    coef[0] = base
    coef[1, A - 1, F - 1] = 0.5 * M.DROP_BELOW
    return coef


def _groups(rng, N, G):
    """Group ids with -1 and G present and one empty group, where N and G leave room for them; None: one group."""
    if G == 1 and N < 3:
        return None
    g = rng.integers(0, G, N)
    if G > 1:
        g[g == (G - 1) // 2] = G - 1                      # an empty group
    g[0] = -1
    if N >= 5:
        g[N - 1] = G                                      # (N = 3: row 1 is the inactive row, row 2 the scored one)
    return g.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(Rn, N, T, A, name, method, sub, levels, B, G):
    """The inputs (padded arrays with poison past T), the trajectories and the restatement, computed once."""
    rng = np.random.default_rng(M._seed("score", Rn, N, T, A, name, method, sub))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    arm = _arms(rng, N, T, A)
    coef = _coef(rng, name, Rn, A)
    v = E.trajectories(y0, u, arm[:, :T], coef, M.exps_of(name), DT, method, sub)
    sd = v[1:].std(axis=0)
    s = np.abs(v).max(axis=0)
    pick = rng.integers(0, Rn, (N, T))
    y_obs = np.full((N, T + PAD), 1e30)
    y_obs[:, :T] = (v[pick, np.arange(N)[:, None], np.arange(T)[None]] + rng.normal(size=(N, T)) * (1.5 * sd + 0.02 * s))
    active = np.ones((N, T + PAD), dtype=np.int8)
    active[:, :T] = np.where(rng.random((N, T)) < 0.1, 0, rng.integers(1, 4, (N, T)) * rng.choice([-1, 1], (N, T)))
    y_obs[:, :T][rng.random((N, T)) < 0.03] = np.nan
    if N > 1:
        active[N // 2, :T] = 0                            # one row fully inactive
    group = _groups(rng, N, G)
    # cells whose count could hang on a rounding are taken out before either side runs
    c = SR.cells(v, y_obs[:, :T], active[:, :T], levels, B)
    close = c["margin"] < MARGIN
    removed = int(close.sum()) / max(int(c["observed"].sum()), 1)
    active[:, :T][close] = 0
    sums, bound, c = SR.score_replicates(v, y_obs[:, :T], active[:, :T], levels, B, group, G)
    out = (y0, u, arm, coef, y_obs, active, group, v, sums, bound)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out + (removed,)


def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _run(dev, name, y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T, pad=0, dt=DT, **kw):
    import torch
    from insite_amd import ops
    out = None
    if pad:
        out = torch.full((G, ops.score_rows(len(levels), B), T + pad), POISON, dtype=torch.float64, device=dev)
    got = ops.ensemble_score(_t(dev, y0), _t(dev, u), _t(dev, arm), _t(dev, y_obs), _t(dev, active), _t(dev, coef),
                             M.LIBS[name], dt, levels, n_bins=B, group=_t(dev, group), n_groups=G, method=method,
                             substeps=sub, drop_below=M.DROP_BELOW, T=T, out=out, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check(got, ref, bound, levels, B, slack=None):
    """Count rows exactly (or within ``slack`` cells), the others within TOL x the summed per-cell bound; returns the
    worst ratio."""
    rows = SR.count_rows(levels, B)
    diff = np.abs(got[:, rows] - ref[:, rows])
    assert np.all(diff <= (0 if slack is None else slack[:, None])), "count rows differ"
    rest = [r for r in range(ref.shape[1]) if r not in rows]
    err, b = np.abs(got[:, rest] - ref[:, rest]), bound[:, rest]
    assert not np.isnan(got).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("Rn,N,T,A,name,method,sub,levels,B,G", CASES, ids=IDS)
def test_parity(dev, Rn, N, T, A, name, method, sub, levels, B, G):
    """The sums against the restatement; the padding of sums keeps its poison; the poison past T in arm (other
    arms), y_obs (1e30) and active (non-zero) is never read; two calls and a NaN-filled workspace give the same bits."""
    import torch
    from insite_amd import ops
    y0, u, arm, coef, y_obs, active, group, _, ref, bound, removed = _case(Rn, N, T, A, name, method, sub, levels, B, G)
    print(f"cells removed for their margin: {100 * removed:.3f} %")
    assert removed <= 0.01
    full = _run(dev, name, y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T, pad=PAD)
    assert full.shape == (G, SR.n_rows(levels, B), T + PAD)
    assert np.all(full[..., T:] == POISON)
    got = full[..., :T]
    w = _check(got, ref, bound, levels, B)
    cov = ref[:, 6 + B::3].sum() / max(ref[:, 0].sum() * len(levels), 1)
    print(f"worst |got - ref| / bound = {w:.3e}; scored {int(ref[:, 0].sum())}, mean coverage {cov:.2f}")
    assert w <= TOL
    assert np.array_equal(got[:, 6:6 + B].sum(axis=1), got[:, 0])
    again = _run(dev, name, y0, u, arm[:, :T], coef, y_obs[:, :T], active[:, :T], group, G, levels, B, method, sub, T)
    assert np.array_equal(_bits(again), _bits(got))
    ws = ops.Workspace("scratch")
    nbytes = ops._lib.load().insite_score_workspace_bytes(N, T, A, coef.shape[2], Rn, G)
    ws.get(nbytes, dev).fill_(0xFF)                       # every double a NaN
    dirty = _run(dev, name, y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T, workspace=ws)
    assert np.array_equal(_bits(dirty), _bits(got))


EXACT = [(17, 130, 17, 2, "std7", "euler", 5, L3, 10, 3), (200, 3, 70, 2, "std7", "rk4", 1, L8, 10, 1),
         (2, 5000, 2, 2, "std7", "euler", 1, L1, 10, 3)]


@pytest.mark.parametrize("Rn,N,T,A,name,method,sub,levels,B,G", EXACT, ids=[f"R{c[0]}-N{c[1]}" for c in EXACT])
def test_exact_properties(dev, Rn, N, T, A, name, method, sub, levels, B, G):
    y0, u, arm, coef, y_obs, active, group, v, ref, bound, _ = _case(Rn, N, T, A, name, method, sub, levels, B, G)
    run = functools.partial(_run, dev, name)
    base = run(y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T)
    # rows 0-2 do not depend on levels or bins
    for lv2, B2 in (((0.3,), 1), (L8, 32)):
        other = run(y0, u, arm, coef, y_obs, active, group, G, lv2, B2, method, sub, T)
        assert np.array_equal(_bits(other[:, :3]), _bits(base[:, :3])), (lv2, B2)
    # no mask = a mask of ones
    ones = np.ones_like(active)
    assert np.array_equal(_bits(run(y0, u, arm, coef, y_obs, None, group, G, levels, B, method, sub, T)),
                          _bits(run(y0, u, arm, coef, y_obs, ones, group, G, levels, B, method, sub, T)))
    # a resampled replicate with NaN coefficients: every observed cell is bad and reaches row 1 only; the values of
    # the excluded rows and of the unobserved cells (NaN) reach nothing
    if Rn > 2:
        c1 = coef.copy()
        c1[Rn - 2] = np.nan
        got = run(y0, u, arm, c1, y_obs, active, group, G, levels, B, method, sub, T)
        observed = SR.group_sums(((active[:, :T] != 0) & np.isfinite(y_obs[:, :T]))[None].astype(float), group, G)
        assert np.array_equal(got[:, 1], observed[:, 0]) and np.all(np.delete(got, 1, axis=1) == 0.0)
    y2, y02 = y_obs.copy(), y0.copy()
    y2[:, :T][active[:, :T] == 0] = np.nan
    if group is not None:
        y02[(group < 0) | (group >= G)] = np.nan
    assert np.array_equal(_bits(run(y02, u, arm, coef, y2, active, group, G, levels, B, method, sub, T)), _bits(base))
    # two shards add to the whole: the count rows exactly, the rest to the bar
    cut = N // 3 + 1
    sl = lambda a, s: None if a is None else a[s]   # noqa: E731
    parts = [run(y0[s], u[s], arm[s], coef, y_obs[s], active[s], sl(group, s), G, levels, B, method, sub, T)
             for s in (slice(0, cut), slice(cut, N))]
    w = _check(parts[0] + parts[1], ref, 2.0 * bound, levels, B)
    assert w <= TOL
    rest = [r for r in range(ref.shape[1]) if r not in SR.count_rows(levels, B)]
    assert np.all(np.abs((parts[0] + parts[1] - base)[:, rest]) <= 2 * TOL * bound[:, rest])


def test_ties(dev):
    """dt = 0, Euler, y_obs = y0: every replicate equals the observation.  c_eq = n puts the cell in the middle bin
    (even B); crps, width and interval score are exactly 0; every level is covered; the errors and the variance are 0."""
    Rn, N, T, A, name, levels, B = 130, 5, 9, 2, "std7", L3, 10
    y0, u, arm, coef, _, _, _, _, _, _, _ = _case(Rn, N, T, A, name, "euler", 1, levels, B, 1)
    y_obs = np.repeat(y0[:, None], T, axis=1)
    got = _run(dev, name, y0, u, arm, coef, y_obs, None, None, 1, levels, B, "euler", 1, T, dt=0.0)[0]
    want = np.zeros_like(got)
    want[0] = want[6 + B // 2] = N
    want[6 + B::3] = N
    assert np.array_equal(got, want)


@pytest.mark.parametrize("Rn,N,T,A,name,method,sub,levels,B,G",
                         [CASES[2], CASES[4], CASES[6], CASES[7]], ids=[IDS[2], IDS[4], IDS[6], IDS[7]])
def test_against_effect_bands(dev, Rn, N, T, A, name, method, sub, levels, B, G):
    """Coverage and width recomputed from ``ops.effect_bands`` with the 2 L band ends as quantiles: the sort and the
    interpolation are shared code, so coverage is equal exactly (no margin exception) and the width to the bar."""
    import torch
    from insite_amd import ops
    y0, u, arm, coef, y_obs, active, group, _, ref, bound, _ = _case(Rn, N, T, A, name, method, sub, levels, B, G)
    got = _run(dev, name, y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T)
    q = [0.5 - 0.5 * float(lam) for lam in levels] + [0.5 + 0.5 * float(lam) for lam in levels]
    bands = ops.effect_bands(_t(dev, y0), _t(dev, u), _t(dev, arm), None, _t(dev, coef), M.LIBS[name], DT, q,
                             method=method, substeps=sub, drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    bands = bands.cpu().numpy()[0]                            # [3 + 2 L, N, T]
    L = len(levels)
    y = y_obs[:, :T]
    scored = (active[:, :T] != 0) & np.isfinite(y)            # no NaN replicate here
    ys = np.where(scored, y, 0.0)
    for j in range(L):
        lo, hi = bands[3 + j], bands[3 + L + j]
        cov = SR.group_sums((scored & (lo <= ys) & (ys <= hi))[None].astype(float), group, G)[:, 0]
        wid = SR.group_sums(np.where(scored, hi - lo, 0.0)[None], group, G)[:, 0]
        r0 = 6 + B + 3 * j
        assert np.array_equal(got[:, r0], cov), j
        assert np.all(np.abs(got[:, r0 + 1] - wid) <= TOL * bound[:, r0 + 1]), j


def test_plan_and_refusals(dev):
    """``plan_ensemble_score`` writes into the caller's out and repeats bit for bit; bad arguments raise."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, name, method, sub, levels, B, G = CASES[2]
    y0, u, arm, coef, y_obs, active, group, _, _, _, _ = _case(*CASES[2])
    base = _run(dev, name, y0, u, arm, coef, y_obs, active, group, G, levels, B, method, sub, T)
    t = functools.partial(_t, dev)
    out = torch.zeros((G, ops.score_rows(len(levels), B), T), dtype=torch.float64, device=dev)
    args = (t(y0), t(u), t(arm), t(y_obs), t(active), t(coef), M.LIBS[name], DT)
    plan = ops.plan_ensemble_score(*args, levels, n_bins=B, group=t(group), n_groups=G, method=method, substeps=sub,
                                   drop_below=M.DROP_BELOW, T=T, out=out)
    for _ in range(2):
        assert plan() is out
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(base))
    for bad in ((0.5, 1.0), (0.0,), (), tuple(np.linspace(0.1, 0.9, 9))):
        with pytest.raises(ValueError):
            ops.ensemble_score(*args, bad, T=T)
    for nb in (0, 33):
        with pytest.raises(ValueError):
            ops.ensemble_score(*args, levels, n_bins=nb, T=T)
    with pytest.raises(ValueError):
        ops.ensemble_score(args[0], args[1], args[2], args[3][:2], *args[4:], levels, T=T)
    with pytest.raises(ValueError):
        ops.ensemble_score(*args, levels, group=t(group)[:2], n_groups=G, T=T)
    # no rows: nothing is launched, a fresh output is zero
    empty = ops.ensemble_score(args[0][:0], args[1][:0], args[2][:0], args[3][:0], args[4][:0], *args[5:], levels, T=T)
    assert empty.shape == (1, ops.score_rows(len(levels), 10), T) and bool((empty == 0).all())


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


def test_plugin_score_bands(dev, model):
    """``score_bands`` is the restatement fed with ``predict_interval(return_replicates=True)``'s replicates,
    un-standardised (those went through a standardise / un-standardise round trip, so a count may move by the cells
    whose margin is below 1e-6: none in practice, and at most 1 %); ``rmse_point`` is the masked RMSE of the point
    model from ``ops.masked_sse``'s un-normalised SSE and count."""
    import torch
    from insite_amd import ops
    tr = _train()
    levels, B, G = (0.5, 0.9, 0.95), 10, 3
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    N = tr.data["current_treatments"].shape[0]
    groups = np.arange(N) % (G + 1) - 1                       # ids -1 .. G - 1
    res = model.score_bands(tr, levels=levels, n_bins=B, groups=groups)
    _, y = model.predict_interval(tr, max_rows=None, return_replicates=True)
    v = (y.cpu().numpy() * std + mean).transpose(1, 0, 2)     # [R, N, T]
    y_obs = np.asarray(tr.data["unscaled_outputs"][..., 0], dtype=np.float64)
    active = np.asarray(tr.data["active_entries"][..., 0])
    ref, bound, c = SR.score_replicates(v, y_obs, active, levels, B, groups, G)
    close = c["margin"] < MARGIN
    assert close.sum() <= 0.01 * c["observed"].sum()
    slack = SR.group_sums(close[None].astype(float), groups, G)[:, 0]
    got = res.sums.cpu().numpy()
    assert got.shape == ref.shape and res.levels == levels and res.n_bins == B and res.scale == std
    w = _check(got, ref, bound, levels, B, slack=slack)
    print(f"worst |got - ref| / bound = {w:.3e}; margin cells {int(close.sum())}; pooled coverage "
          f"{res.pooled['coverage'].cpu().numpy().round(3).tolist()}")
    assert w <= TOL
    assert np.all(got[:, 1] == 0)
    assert got[:, 0].sum() == ((active != 0) & np.isfinite(y_obs) & (groups >= 0)[:, None]).sum()
    # one group: the point model's masked RMSE
    one = model.score_bands(tr, levels=levels, n_bins=B)
    pred = model._predict_device(tr)
    per, cnt, _ = ops.masked_sse(pred.contiguous(), torch.as_tensor(y_obs, device=dev),
                                 torch.as_tensor(np.ascontiguousarray(active, dtype=np.float64), device=dev),
                                 scale=std, shift=mean)
    per, cnt = per.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(one.n.cpu().numpy()[0], cnt)
    keep = cnt > 0
    rm = one.rmse_point.cpu().numpy()[0]
    assert np.allclose(rm[keep], np.sqrt(per[keep] / cnt[keep]) / std, rtol=1e-10, atol=0)
    assert np.isnan(rm[~keep]).all()
    pooled = float(one.pooled["rmse_point"].cpu().numpy()[0])
    assert abs(pooled - np.sqrt(per.sum() / cnt.sum()) / std) <= 1e-10 * pooled
    # merge: the same shard twice doubles every count and leaves the frequencies
    twice = res.merge(res)
    assert np.array_equal(twice.n.cpu().numpy(), 2 * res.n.cpu().numpy())
    assert np.array_equal(_bits(twice.coverage.cpu().numpy()), _bits(res.coverage.cpu().numpy()))
    with pytest.raises(ValueError):
        model.score_bands(tr, levels=(0.5, 1.0))


def test_plugin_segment_model(dev):
    """A treatment-segment model scores its bands once ``bootstrap_segments`` has stored its ensemble."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr = CS.make_collection(1, {"train": 200, "val": 20, "test": 10}, with_tests=False)["train"]
    a = C.compose(["+backbone=sindy", "+dataset=pkpd_sim", "model.sindy_threshold=0.001", "model.sindy_alpha=0.5"])
    a["model"].update({"dataset_name": "cancer_sim", "dim_treatments": 4, "dim_static_features": 1, "dim_outcomes": 1})
    m = SINDY(a, device=dev).fit(tr)
    with pytest.raises(NotImplementedError, match="bootstrap_segments"):
        m.score_bands(tr)
    m.bootstrap_segments(tr, n_replicates=33, seed=3)
    res = m.score_bands(tr, levels=(0.5, 0.9), n_bins=8)
    n = res.n.cpu().numpy()
    assert res.sums.shape[:2] == (1, 6 + 8 + 6) and n.sum() > 0
    for k in ("rmse_point", "rmse_mean", "spread", "crps", "coverage", "width", "interval_score", "pit_hist"):
        val = res.pooled[k].cpu().numpy()
        assert np.isfinite(val).all(), k
    assert np.isfinite(res.crps.cpu().numpy()[n > 0]).all()
    assert np.array_equal(res.pit_hist.cpu().numpy().shape, (1, 8, n.shape[1]))
