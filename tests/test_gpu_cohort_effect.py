"""GPU tests of the cohort / subgroup average effects (include/insite_cohort.h: cohort_sums_kernel,
cohort_reduce_kernel, cohort_finalize_kernel, ops.cohort_effect*, SINDY.average_effect) against the numpy restatement
tests/cohort_effect_ref.py.

Tolerance: every output, and sums / wsum, within TOL s of the restatement, s[g, k] the largest |yA| or |yB| over the
replicates and the contributing rows of group g: the project's bar for these statistics (tests/test_gpu_effect.py).  A
weighted mean is a convex combination, so it is 1-Lipschitz in the sup norm of the trajectories (1e-11 s, the rollout
bar), and a fixed-order sum of N <= 5000 terms rounds at about N eps s ~ 1e-12 s.  wsum is a sum of small integers:
bitwise equal.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cohort_effect_ref as CR  # noqa: E402
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402
from test_gpu_effect import _bits, _coef, _plans, _worst  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
DT = 0.1
Q5 = (0.0, 1.0, 0.5, 0.025, 0.5)                     # unsorted, with a repeat
PAD_OUT, POISON = 5, -7.25
SEED = 7

# (R, N, T, arms, G, table, method, substeps, weighting, patient_offset); group[p] = p % G
CASES = [
    (2, 3, 1, 1, 1, "x_only", "euler", 1, "none", 0),
    (3, 1, 2, 2, 1, "bias_x", "rk4", 1, "none", 0),
    (17, 130, 31, 2, 3, "std7", "euler", 5, "poisson", 0),
    (64, 130, 33, 4, 1, "noone3", "rk4", 5, "poisson", 0),
    (65, 257, 64, 2, 4, "lin3", "euler", 5, "poisson", 0),
    (129, 130, 65, 2, 2, "std7", "rk4", 1, "poisson", 0),
    (200, 64, 130, 2, 1, "high_pow", "euler", 1, "none", 0),
    (513, 130, 7, 2, 3, "std7", "rk4", 5, "poisson", 0),          # above the per-row kernel's cap
    (4096, 70, 3, 1, 1, "bias_x", "euler", 1, "poisson", 0),
    (65, 5000, 8, 2, 64, "std7", "euler", 5, "poisson", 0),       # several patient chunks, the group cap
    (33, 130, 33, 4, 5, "u3_mixed9", "rk4", 1, "poisson", 0),
    (17, 130, 31, 2, 3, "std7", "euler", 5, "poisson", 12345),
    (65, 257, 64, 2, 4, "lin3", "euler", 5, "poisson", 12345),
]


def _id(c):
    return f"R{c[0]}-N{c[1]}-T{c[2]}-A{c[3]}-G{c[4]}-{c[5]}-{c[6]}{c[7]}-{c[8]}-off{c[9]}"


@functools.lru_cache(maxsize=None)
def _inputs(Rn, N, T, A, name, method, sub):
    """The inputs of a case (shared by its offsets), read-only."""
    rng = np.random.default_rng(M._seed("cohort", Rn, N, T, A, name, method, sub))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    arm_a, arm_b = _plans(rng, N, T, A)               # columns past T hold out-of-range arms
    coef = _coef(rng, name, Rn, A)
    out = (y0, u, arm_a, arm_b, coef)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _case(Rn, N, T, A, G, name, method, sub, weighting, off, q=Q5):
    y0, u, arm_a, arm_b, coef = _inputs(Rn, N, T, A, name, method, sub)
    group = (np.arange(N) % G).astype(np.int32)
    ref = CR.cohort(y0, u, arm_a[:, :T], arm_b[:, :T], coef, M.exps_of(name), DT, q, group, G, weighting, SEED, off,
                    method, sub)
    for a in ref + (group,):
        a.setflags(write=False)
    return (y0, u, arm_a, arm_b, coef, group) + ref


def _t(dev, a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _run(dev, name, y0, u, arm_a, arm_b, coef, q, method, sub, T, group=None, G=1, weighting="poisson", seed=SEED,
         off=0, pad=0):
    """-> (out [G, S, 3 + Q, T + pad], sums, wsum) as numpy."""
    import torch
    from insite_amd import ops
    out = None
    if pad:
        S = 1 if arm_b is None else 3
        out = torch.full((G, S, 3 + len(q), T + pad), POISON, dtype=torch.float64, device=dev)
    got = ops.cohort_effect(_t(dev, y0), _t(dev, u), _t(dev, arm_a), _t(dev, arm_b), _t(dev, coef), M.LIBS[name], DT,
                            q, group=_t(dev, group), n_groups=G, weighting=weighting, seed=seed, patient_offset=off,
                            method=method, substeps=sub, drop_below=M.DROP_BELOW, T=T, out=out)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_parity(dev, case):
    """out, sums / wsum and the exact wsum against the restatement; the padding of out keeps its poison and the
    out-of-range arms past T are never read (they would select another arm)."""
    Rn, N, T, A, G, name, method, sub, weighting, off = case
    y0, u, arm_a, arm_b, coef, group, ref, S_ref, w_ref, scale = _case(*case)
    # no replicate is empty in any group: a comparison of NaN to NaN would hide a failure
    # (the only NaN of the reference is the standard deviation of one resample, R = 2)
    nan_ok = np.zeros(ref.shape, dtype=bool)
    nan_ok[:, :, 2] = Rn == 2
    assert w_ref.min() >= 1 and np.array_equal(np.isnan(ref), nan_ok)
    full, sums, wsum = _run(dev, name, y0, u, arm_a, arm_b, coef, Q5, method, sub, T, group, G, weighting, SEED, off,
                            pad=PAD_OUT)
    assert full.shape == (G, 3, 3 + len(Q5), T + PAD_OUT) and sums.shape == (Rn, G, 2, T) and wsum.shape == (Rn, G)
    assert np.all(full[..., T:] == POISON)
    assert np.array_equal(_bits(wsum), _bits(w_ref))
    got = full[..., :T]
    s_out = scale[:, None, None, :]
    w_out = _worst(got, ref, s_out)
    w_mean = _worst(sums / wsum[:, :, None, None], S_ref / w_ref[:, :, None, None], scale[None, :, None, :])
    print(f"worst |got - ref| / s: out {w_out:.3e}, sums / wsum {w_mean:.3e}")
    assert w_out <= TOL and w_mean <= TOL
    if Rn == 2:
        assert np.isnan(got[:, :, 2]).all()


BASE = (65, 257, 64, 2, 4, "lin3", "euler", 5, "poisson", 0)


def _base_run(dev, **kw):
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    args = dict(y0=y0, u=u, arm_a=arm_a, arm_b=arm_b, coef=coef, q=Q5, group=group, G=G, weighting=weighting,
                seed=SEED, off=off)
    args.update(kw)
    return _run(dev, name, args["y0"], args["u"], args["arm_a"], args["arm_b"], args["coef"], args["q"], method, sub,
                T, args["group"], args["G"], args["weighting"], args["seed"], args["off"])


def test_two_calls_are_bitwise_equal(dev):
    a, b = _base_run(dev), _base_run(dev)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.isnan(a[0]).any()


def test_without_plan_b_is_series_a(dev):
    full, sums, wsum = _base_run(dev)
    only, sums_a, wsum_a = _base_run(dev, arm_b=None)
    assert only.shape[1] == 1 and sums_a.shape[2] == 1
    assert np.array_equal(_bits(only[:, 0]), _bits(full[:, 0]))
    assert np.array_equal(_bits(sums_a[:, :, 0]), _bits(sums[:, :, 0])) and np.array_equal(_bits(wsum_a), _bits(wsum))


def test_point_rows_do_not_depend_on_r_q_weighting_seed(dev):
    coef = _case(*BASE)[4]
    base = _base_run(dev)[0]
    for kw in (dict(coef=coef[:2]), dict(coef=coef[:64], q=(0.3,)), dict(weighting="none"), dict(seed=99),
               dict(off=12345)):
        other = _base_run(dev, **kw)[0]
        assert np.array_equal(_bits(other[:, :, 0]), _bits(base[:, :, 0])), kw


def test_excluded_rows_change_no_bit(dev):
    """Rows with group = -1 or >= G, with NaN y0 / u or not, change no output bit against the cohort without them."""
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    ex = np.array([0, 5, 64, 65, 130, 256])
    g2 = group.copy()
    g2[ex] = [-1, G, -7, G + 60, 2 ** 31 - 1, -2 ** 31]
    base = _base_run(dev, group=g2)
    y0n, un = y0.copy(), u.copy()
    y0n[ex[:3]] = np.nan
    un[ex[3:]] = np.nan
    got = _base_run(dev, group=g2, y0=y0n, u=un)
    for x, y in zip(base, got):
        assert not np.isnan(x).any() and np.array_equal(_bits(x), _bits(y))
    # and they are left out: wsum is the restatement's without them
    w = CR.weights("poisson", SEED, Rn, N)
    w[:, ex] = 0
    want = np.stack([w[:, g2 == g].sum(axis=1) for g in range(G)], axis=1).astype(np.float64)
    assert np.array_equal(_bits(base[2]), _bits(want))


def test_zero_weight_row_is_selected_out(dev):
    """A row whose weight is 0 in replicate r and whose y0 is NaN leaves replicate r's sums finite (a select, not a
    multiplication by zero); the replicates that drew it are NaN."""
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    w = CR.weights("poisson", SEED, Rn, N)
    p = 100
    zero = np.nonzero(w[:, p] == 0)[0]
    assert zero.size and (w[1:, p] > 0).any()
    for field in ("y0", "u"):
        bad = (y0 if field == "y0" else u).copy()
        bad[p] = np.nan
        _, sums, wsum = _base_run(dev, **{field: bad})
        g = group[p]
        assert np.isfinite(sums[zero]).all()
        if field == "y0":
            assert np.isnan(sums[w[:, p] > 0][:, g]).all()
        else:       # a replicate whose support holds no term in u is not touched by a NaN u
            assert np.isnan(sums[w[:, p] > 0][:, g]).any()
        assert np.isfinite(np.delete(sums, g, axis=1)).all()
        assert np.array_equal(_bits(wsum), _bits(_case(*BASE)[8]))


def test_nan_replicate(dev):
    """A replicate with NaN coefficients: mean, std and quantiles are NaN, the point row is untouched."""
    coef = _case(*BASE)[4]
    base = _base_run(dev)[0]
    c1 = coef.copy()
    c1[coef.shape[0] - 2] = np.nan
    got = _base_run(dev, coef=c1)[0]
    assert np.isnan(got[:, :, 1:]).all()
    assert np.array_equal(_bits(got[:, :, 0]), _bits(base[:, :, 0]))
    c0 = coef.copy()
    c0[0] = np.nan
    got = _base_run(dev, coef=c0)[0]
    assert np.isnan(got[:, :, 0]).all() and np.array_equal(_bits(got[:, :, 1:]), _bits(base[:, :, 1:]))


def test_empty_replicate_gives_nan_statistics(dev):
    """A group that some replicate does not draw (one row, weight 0 in some replicate): NaN statistics, a finite
    point, an exact wsum."""
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, _ = _case(*BASE)[:6]
    Rs = 9
    w = CR.weights("poisson", SEED, Rs, 1)
    assert (w[1:, 0] == 0).any()
    out, sums, wsum = _run(dev, name, y0[:1], u[:1], arm_a[:1], arm_b[:1], coef[:Rs], Q5, method, sub, T, None, 1,
                           "poisson", SEED, 0)
    assert np.isnan(out[0, :, 1:]).all() and np.isfinite(out[0, :, 0]).all()
    assert np.array_equal(_bits(wsum[:, 0]), _bits(w[:, 0].astype(np.float64)))
    assert np.all(sums[w[:, 0] == 0] == 0.0)
    ref = CR.cohort(y0[:1], u[:1], arm_a[:1, :T], arm_b[:1, :T], coef[:Rs], M.exps_of(name), DT, Q5, None, 1,
                    "poisson", SEED, 0, method, sub)
    assert _worst(out, ref[0], ref[3][:, None, None, :]) <= TOL


def test_no_rows_is_a_no_op(dev):
    import torch
    from insite_amd import ops
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    out = torch.full((G, 3, 3 + len(Q5), T), POISON, dtype=torch.float64, device=dev)
    sums = torch.full((Rn, G, 2, T), POISON, dtype=torch.float64, device=dev)
    wsum = torch.full((Rn, G), POISON, dtype=torch.float64, device=dev)
    ops.cohort_effect_sums(_t(dev, y0[:0]), _t(dev, u[:0]), _t(dev, arm_a[:0]), _t(dev, arm_b[:0]), _t(dev, coef),
                           M.LIBS[name], DT, group=_t(dev, group[:0]), n_groups=G, seed=SEED, method=method,
                           substeps=sub, T=T, out=(sums, wsum))
    got = ops.cohort_effect(_t(dev, y0[:0]), _t(dev, u[:0]), _t(dev, arm_a[:0]), _t(dev, arm_b[:0]), _t(dev, coef),
                            M.LIBS[name], DT, Q5, group=_t(dev, group[:0]), n_groups=G, seed=SEED, method=method,
                            substeps=sub, T=T, out=out)
    torch.cuda.synchronize()
    assert got[0] is out
    assert bool((out == POISON).all()) and bool((sums == POISON).all()) and bool((wsum == POISON).all())


@pytest.mark.parametrize("split", [100, 101])
def test_shards_add_up(dev, split):
    """The cohort in two shards (an even split, and an odd one that crosses a Threefry pair), each with its
    patient_offset: the sums and wsum added in shard order and finalised are the whole cohort's (wsum bit for bit)."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group, ref, _, w_ref, scale = _case(*BASE)
    whole = _base_run(dev)
    parts = []
    for lo, hi in ((0, split), (split, N)):
        parts.append(ops.cohort_effect_sums(_t(dev, y0[lo:hi]), _t(dev, u[lo:hi]), _t(dev, arm_a[lo:hi]),
                                            _t(dev, arm_b[lo:hi]), _t(dev, coef), M.LIBS[name], DT,
                                            group=_t(dev, group[lo:hi]), n_groups=G, weighting="poisson", seed=SEED,
                                            patient_offset=lo, method=method, substeps=sub,
                                            drop_below=M.DROP_BELOW, T=T))
    sums = parts[0][0] + parts[1][0]
    wsum = parts[0][1] + parts[1][1]
    out = ops.cohort_effect_finalize(sums, wsum, Q5)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wsum.cpu().numpy()), _bits(whole[2])) and np.array_equal(_bits(whole[2]), _bits(w_ref))
    assert _worst(out.cpu().numpy(), ref, scale[:, None, None, :]) <= TOL
    assert _worst(out.cpu().numpy(), whole[0], scale[:, None, None, :]) <= TOL


def test_finalize_alone_reproduces_the_combined_call(dev):
    import torch
    from insite_amd import ops
    out, sums, wsum = _base_run(dev)
    again = ops.cohort_effect_finalize(_t(dev, sums), _t(dev, wsum), Q5)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(out))
    # the sums call alone gives the combined call's sums
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    s2, w2 = ops.cohort_effect_sums(_t(dev, y0), _t(dev, u), _t(dev, arm_a), _t(dev, arm_b), _t(dev, coef),
                                    M.LIBS[name], DT, group=_t(dev, group), n_groups=G, seed=SEED, method=method,
                                    substeps=sub, drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(s2.cpu().numpy()), _bits(sums)) and np.array_equal(_bits(w2.cpu().numpy()), _bits(wsum))


def test_plan_and_out(dev):
    """``plan_cohort_effect`` writes into the caller's out and repeats bit for bit; the ops' refusals."""
    import torch
    from insite_amd import ops
    Rn, N, T, A, G, name, method, sub, weighting, off = BASE
    y0, u, arm_a, arm_b, coef, group = _case(*BASE)[:6]
    base = _base_run(dev)
    out = torch.zeros((G, 3, 3 + len(Q5), T), dtype=torch.float64, device=dev)
    args = (_t(dev, y0), _t(dev, u), _t(dev, arm_a), _t(dev, arm_b), _t(dev, coef), M.LIBS[name], DT)
    plan = ops.plan_cohort_effect(*args, Q5, group=_t(dev, group), n_groups=G, seed=SEED, method=method, substeps=sub,
                                  drop_below=M.DROP_BELOW, T=T, out=out)
    for _ in range(2):
        got = plan()
        torch.cuda.synchronize()
        assert got[0] is out
        for x, y in zip(got, base):
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(y))
    with pytest.raises(ValueError):
        ops.cohort_effect(*args, (0.5, 1.5), T=T)
    with pytest.raises(ValueError):
        ops.cohort_effect(*args, Q5, n_groups=65, T=T)
    with pytest.raises(ValueError):
        ops.cohort_effect(*args, Q5, weighting="rows", T=T)
    with pytest.raises(ValueError):
        ops.cohort_effect(*args, Q5, group=_t(dev, group[:5]), n_groups=G, T=T)
    with pytest.raises(ValueError):
        ops.cohort_effect(*args[:4], _t(dev, coef[:1]), *args[5:], Q5, T=T)


def test_against_effect_bands(dev):
    """Weighting "none", one group: point and mean of all three series are the row-mean of ``ops.effect_bands``'
    point and mean (the mean is linear; the quantiles are not)."""
    import torch
    from insite_amd import ops
    case = (200, 130, 33, 2, 1, "std7", "euler", 5, "none", 0)
    Rn, N, T, A, G, name, method, sub, weighting, off = case
    y0, u, arm_a, arm_b, coef, group, ref, _, _, scale = _case(*case)
    out = _run(dev, name, y0, u, arm_a, arm_b, coef, Q5, method, sub, T, None, 1, "none")[0]
    bands = ops.effect_bands(_t(dev, y0), _t(dev, u), _t(dev, arm_a), _t(dev, arm_b), _t(dev, coef), M.LIBS[name], DT,
                             Q5, method=method, substeps=sub, drop_below=M.DROP_BELOW, T=T)
    torch.cuda.synchronize()
    rows = bands.cpu().numpy().mean(axis=2)                     # [3, 3 + Q, T]
    for st in (0, 1):
        w = _worst(out[0, :, st], rows[:, st], scale[0][None])
        print(f"stat {st}: worst |cohort - mean of rows| / s = {w:.3e}")
        assert w <= TOL
    assert _worst(out, ref, scale[:, None, None, :]) <= TOL


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
    m.bootstrap(tr, n_replicates=64, seed=3)
    return m


def _as_array(res):
    """[S, 3 + Q, G, T] from a CohortEffectResult."""
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def test_plugin_average_effect(dev, model):
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    q = (0.025, 0.5, 0.975)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    prev, stat = R.unscale_inputs(tr.data, tr.scaling_params)
    arms = np.argmax(tr.data["current_treatments"], axis=-1)
    N = arms.shape[0]
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    groups = np.arange(N) % 3
    groups[[4, 9]] = -1
    ref, _, w_ref, scale = CR.cohort(prev[:, 0], stat, arms, np.zeros_like(arms), coef, R.poly_library(3, 2, True),
                                     model.dt, q, groups, 3, "poisson", 3, 0, "euler5")
    assert w_ref.min() >= 1
    res = model.average_effect(tr, plan_b=0, groups=groups, resample="paired")
    assert res.series == ("a", "b", "effect") and res.q == q
    assert res.point.shape == (3, 3, arms.shape[1]) and res.quantiles.shape == (3, 3, 3, arms.shape[1])
    assert np.array_equal(_bits(res.weight_sum.cpu().numpy()), _bits(w_ref))
    want = ref.transpose(1, 2, 0, 3) / std                       # [S, 3 + Q, G, T]
    loc = [0, 1, 3, 4, 5]
    want[:2, loc] = (ref.transpose(1, 2, 0, 3)[:2, loc] - mean) / std
    w = _worst(_as_array(res), want, scale[None, None] / std)    # the bar in standardised units
    print(f"worst |got - ref| / s = {w:.3e}")
    assert w <= TOL
    # resample=None: the point row is the row-mean of treatment_effect's point rows
    none = model.average_effect(tr, plan_b=0, resample=None)
    rows = model.treatment_effect(tr, plan_b=0).point.cpu().numpy()          # [3, N, T]
    s_all = np.fmax.reduce(scale, axis=0) / std
    assert _worst(none.point.cpu().numpy()[:, 0], rows.mean(axis=1), s_all[None]) <= TOL
    assert bool((none.weight_sum == N).all())
    # "independent" needs another seed and then differs from the paired band; the single-plan form is series a
    ind = model.average_effect(tr, plan_b=0, groups=groups, resample="independent", seed=4)
    assert np.array_equal(_bits(ind.point.cpu().numpy()), _bits(res.point.cpu().numpy()))
    assert not np.array_equal(_bits(ind.mean.cpu().numpy()), _bits(res.mean.cpu().numpy()))
    one = model.predict_average(tr, groups=groups)
    assert one.series == ("a",)
    assert np.array_equal(_bits(_as_array(one)[0]), _bits(_as_array(res)[0]))


def test_plugin_refusals(dev, model):
    import copy
    import torch
    from insite_amd import bootstrap
    tr = _train()
    N = tr.data["current_treatments"].shape[0]
    with pytest.raises(ValueError, match="independent"):
        model.average_effect(tr, plan_b=0, resample="independent")
    with pytest.raises(ValueError, match="independent"):
        model.average_effect(tr, plan_b=0, resample="independent", seed=3)
    with pytest.raises(ValueError, match="groups"):
        model.average_effect(tr, plan_b=0, groups=np.full(N, 64))
    with pytest.raises(ValueError, match="groups"):
        model.average_effect(tr, plan_b=0, groups=np.zeros(N + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="two plans"):
        model.average_effect(tr, None, None)
    m2 = copy.copy(model)
    del m2.bootstrap_
    with pytest.raises(RuntimeError, match="bootstrap"):
        m2.average_effect(tr, plan_b=0)
    bs = model.bootstrap_
    m2.bootstrap_ = bootstrap.summarize(bs.coef[:1], bs.mask[:1], seed=3)
    with pytest.raises(ValueError, match="n_replicates"):
        m2.average_effect(tr, plan_b=0)
    for attr in ("joint_model", "segment_mode"):
        m3 = copy.copy(model)
        setattr(m3, attr, True)
        with pytest.raises(NotImplementedError, match="average_effect"):
            m3.average_effect(tr, plan_b=0)
    assert isinstance(model.bootstrap_.coef, torch.Tensor)
