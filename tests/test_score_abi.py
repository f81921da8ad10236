"""CPU tests of the ensemble-score extension ABI (include/insite_score.h): header, bindings and exported symbols
agree, every argument check answers before any HIP call and in the header's order, the workspace query stays below
1 GiB, the numpy restatement tests/score_ref.py (the reference of tests/test_gpu_score.py) agrees with the pairwise
definition of the CRPS, and ``effect.from_score`` / ``merge`` / ``SINDY.score_bands`` do their host-side part."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_score.h")
FN_RE = r"^\s*(?:const\s+char\s*\*|int32_t|size_t)\s+(insite_\w+)\s*\("

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from insite_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_and_bindings_agree(L):
    from insite_amd import _lib
    src = open(HEADER).read()
    fns = sorted(set(re.findall(FN_RE, src, re.M)))
    assert fns == sorted(_lib.SCORE_SYMBOLS) and len(fns) == 3
    older = set()
    for name in dir(_lib):
        if (name.endswith("EXPORTS") or name.endswith("SYMBOLS")) and name != "SCORE_SYMBOLS":
            older |= set(getattr(_lib, name))
    assert not set(fns) & older
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES and name in syms, name

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_SCORE_ABI_VERSION") == _lib.SCORE_ABI_VERSION == 1 == L.insite_score_abi_version()
    assert const("INSITE_SCORE_MAX_REPLICATES") == _lib.SCORE_MAX_REPLICATES == 512
    assert const("INSITE_SCORE_MAX_LEVELS") == _lib.SCORE_MAX_LEVELS == 8
    assert const("INSITE_SCORE_MAX_BINS") == _lib.SCORE_MAX_BINS == 32
    assert const("INSITE_SCORE_MAX_GROUPS") == _lib.SCORE_MAX_GROUPS == _lib.COHORT_MAX_GROUPS == 64
    assert 6 + _lib.SCORE_MAX_BINS + 3 * _lib.SCORE_MAX_LEVELS <= 64      # one lane owns one statistic
    for name in fns:
        if name == "insite_score_abi_version":
            continue
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_score.h happens before any HIP call (this host has no GPU), in the header's order."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4096)()
    lv = np.array([0.5, 0.9, 0.95])
    lp = lv.ctypes.data_as(ctypes.c_void_p)
    wsb = L.insite_score_workspace_bytes
    big = 1 << 30

    def call(y0=x, u=x, arm=x, lda=12, coef=x, e=ep, F=7, N=5, T=12, U=2, A=2, dt=0.1, m=0, sub=5, drop=1e-3, Rn=9,
             yo=x, ldy=12, act=x, ldm=12, grp=x, G=3, lev=lp, nl=3, B=10, ws=x, wsn=big, s=x, lds=12):
        return L.insite_score_sums_f64(y0, u, arm, lda, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn, yo, ldy, act,
                                       ldm, grp, G, lev, nl, B, ws, wsn, s, lds, nul)

    # insite_effect_bands_f64's list
    assert call(y0=nul) == -1 and call(u=nul) == -1 and call(arm=nul) == -1 and call(coef=nul) == -1
    assert call(e=nul) == -1
    assert call(N=-1) == -1 and call(T=0) == -1 and call(T=-3) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(A=0) == -1 and call(A=_lib.MAX_ARMS + 1) == -1
    assert call(F=0) == -1 and call(F=_lib.MAX_TERMS + 1) == -1
    assert call(sub=0) == -1 and call(dt=-0.1) == -1 and call(dt=float("nan")) == -1
    assert call(m=2) == -2 and call(m=-1) == -2
    assert call(Rn=1) == -1 and call(Rn=0) == -1 and call(Rn=-4) == -1
    assert call(Rn=513) == -2 and call(Rn=_lib.SCORE_MAX_REPLICATES + 1) == -2
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                      # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    # this header's additions
    assert call(lda=11) == -1 and call(ldy=11) == -1 and call(ldm=11) == -1 and call(lds=11) == -1
    assert call(yo=nul) == -1 and call(s=nul) == -1
    assert call(G=0) == -1 and call(G=-1) == -1 and call(G=65) == -1
    assert call(nl=0) == -1 and call(nl=9) == -1 and call(nl=-1) == -1 and call(lev=nul) == -1
    assert call(B=0) == -1 and call(B=33) == -1 and call(B=-2) == -1
    for bad in (0.0, 1.0, float("nan"), -0.1, 1.5, float("inf")):
        lb = np.array([0.5, bad, 0.9])
        assert call(lev=lb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
    assert call(ws=nul) == -1 and call(wsn=wsb(5, 12, 2, 7, 9, 3) - 1) == -1
    odd = ctypes.c_void_p(ctypes.addressof(x) + 4)
    assert call(ws=odd) == -1
    # the order: an invalid argument wins over an unsupported one, the method over the table, the table over the cap
    assert call(m=2, T=0) == -1 and call(Rn=513, B=0) == -1 and call(Rn=513, lev=nul) == -1
    assert call(m=2, e=e3.ctypes.data_as(ctypes.c_void_p)) == -2
    assert call(Rn=513, e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call(Rn=513, yo=nul) == -2 and call(m=2, N=0) == -2
    # n_rows = 0: a successful no-op whatever the cohort's pointers, still validated
    assert call(N=0) == 0
    assert call(N=0, y0=nul, u=nul, arm=nul, coef=nul, yo=nul, act=nul, grp=nul, s=nul, ws=nul, wsn=0) == 0
    l8 = np.linspace(0.1, 0.99, 8)
    assert call(N=0, Rn=512, G=64, lev=l8.ctypes.data_as(ctypes.c_void_p), nl=8, B=32) == 0
    assert call(N=0, Rn=1) == -1 and call(N=0, T=0) == -1 and call(N=0, G=65) == -1 and call(N=0, B=33) == -1
    assert call(N=0, nl=9) == -1 and call(N=0, Rn=513) == -2 and call(N=0, ldy=11) == -1
    assert call(N=0, lev=np.array([0.5, 1.0, 0.9]).ctypes.data_as(ctypes.c_void_p)) == -1


def test_workspace_query(L):
    wsb = L.insite_score_workspace_bytes
    GiB = 1 << 30
    assert 0 < wsb(1_000_000, 255, 4, 9, 512, 64) < GiB
    for N, T, A, F, Rn, G in ((1, 1, 1, 1, 2, 1), (130, 33, 2, 7, 65, 3), (100_000, 60, 2, 7, 256, 1),
                              (1_000_000, 60, 4, 9, 512, 1), (100_000_000, 60, 2, 7, 512, 8), (5000, 8, 2, 7, 65, 64)):
        b = wsb(N, T, A, F, Rn, G)
        assert 0 < b < GiB, (N, T, Rn, G)
        assert b >= G * T * 64 * 8 and b % (G * T * 64 * 8) == 0           # whole slabs, at least one
        assert b <= min(N, 4096) * G * T * 64 * 8
    # invalid arguments, no rows, and a shape whose single slab passes 1 GiB: 0
    assert wsb(-1, 60, 2, 7, 256, 1) == 0 and wsb(0, 60, 2, 7, 256, 1) == 0
    assert wsb(10, 0, 2, 7, 256, 1) == 0 and wsb(10, 60, 0, 7, 256, 1) == 0 and wsb(10, 60, 5, 7, 256, 1) == 0
    assert wsb(10, 60, 2, 0, 256, 1) == 0 and wsb(10, 60, 2, 10, 256, 1) == 0
    assert wsb(10, 60, 2, 7, 1, 1) == 0 and wsb(10, 60, 2, 7, 513, 1) == 0
    assert wsb(10, 60, 2, 7, 256, 0) == 0 and wsb(10, 60, 2, 7, 256, 65) == 0
    assert wsb(10, 100_000, 2, 7, 256, 64) == 0


def test_ops_refuse_host_tensors_and_bad_arguments(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0 = torch.zeros(4, dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros((4, 6), dtype=torch.int8)
    yo = torch.zeros((4, 6), dtype=torch.float64)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    for fn in (ops.ensemble_score, ops.plan_ensemble_score):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, arm, yo, None, coef, lib, 0.1, (0.5, 0.9))
    assert ops.score_rows(3, 10) == 25 and ops.score_rows(8, 32) == 62


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65, 511])
def test_sorted_crps_is_the_pairwise_definition(n):
    import score_ref as SR
    rng = np.random.default_rng(n)
    worst = 0.0
    for _ in range(3):
        rep = rng.normal(size=n) * rng.uniform(0.1, 3.0) + rng.normal()
        rep[rng.integers(0, n)] = rep[0]                                  # a tie among the values
        for y in (rng.normal(), rep[n // 2], rep.min() - 1.0, rep.max() + 2.0):
            a, b = float(SR.crps_sorted(rep[:, None], np.array([y]))[0]), SR.crps_pairwise(rep, y)
            worst = max(worst, abs(a - b) / max(np.abs(rep).max(), abs(y)))
    print(f"n = {n}: worst |sorted - pairwise| / scale = {worst:.3e}")
    assert worst <= 1e-14
    if n == 1:
        assert SR.crps_sorted(np.array([[2.0]]), np.array([0.5]))[0] == 1.5  # one value: |v - y|


def _small(seed, Rn=17, N=12, T=9, A=2, name="std7"):
    import library_matrix as M
    rng = np.random.default_rng(seed)
    exps = M.exps_of(name)
    F = exps.shape[0]
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    arm = rng.integers(0, A, (N, T)).astype(np.int8)
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[0] = base
    return y0, u, arm, coef, exps, rng


def test_restatement_rules():
    """The histogram rows add to row 0, count rows are integers, unobserved and bad cells reach only their own
    count, excluded rows nothing, rows 0-2 do not depend on levels or bins, and shards add to the whole."""
    import effect_ref as E
    import score_ref as SR
    y0, u, arm, coef, exps, rng = _small(3)
    N, T = arm.shape
    levels, B, G = (0.5, 0.9), 10, 3
    v = E.trajectories(y0, u, arm, coef, exps, 0.1, "euler", 5)
    y_obs = v[rng.integers(1, coef.shape[0], (N, T)), np.arange(N)[:, None], np.arange(T)[None]]
    y_obs = y_obs + rng.normal(size=(N, T)) * (1.5 * v[1:].std(axis=0, ddof=1) + 0.02 * np.abs(v).max(axis=0))
    active = (rng.random((N, T)) > 0.1).astype(np.int8)
    active[4] = 0
    y_obs[2, 3] = np.nan
    y_obs[4, 1] = np.nan
    group = np.arange(N) % G
    group[5], group[7] = -1, G
    sums, bound, c = SR.score_replicates(v, y_obs, active, levels, B, group, G)
    S = SR.n_rows(levels, B)
    assert sums.shape == (G, S, T) and S == 6 + 10 + 6
    assert np.array_equal(sums[:, 6:6 + B].sum(axis=1), sums[:, 0])
    rows = SR.count_rows(levels, B)
    assert np.array_equal(sums[:, rows], np.round(sums[:, rows]))
    inc = (group >= 0) & (group < G)
    assert sums[:, 0].sum() == c["scored"][inc].sum() == ((active != 0) & np.isfinite(y_obs))[inc].sum()
    assert np.all(sums[:, 1] == 0) and np.all(bound[:, rows] == 0) and np.all(bound[:, 2:6].sum(axis=2) > 0)
    cover = sums[:, 6 + B::3].sum(axis=(0, 2)) / sums[:, 0].sum()
    assert 0.05 < cover[0] < cover[1] < 0.95                                # both outcomes occur at both levels
    # a replicate of NaN coefficients: every observed cell is bad and nothing else is reached
    vb = v.copy()
    vb[5] = np.nan
    sb, _, _ = SR.score_replicates(vb, y_obs, active, levels, B, group, G)
    assert np.array_equal(sb[:, 1], sums[:, 0]) and np.all(np.delete(sb, 1, axis=1) == 0)
    # the excluded rows' values reach nothing
    y2, v2 = y_obs.copy(), v.copy()
    y2[5], v2[:, 7] = 1e9, -1e9
    assert np.array_equal(SR.score_replicates(v2, y2, active, levels, B, group, G)[0], sums)
    # rows 0-2 under other levels and bins
    other = SR.score_replicates(v, y_obs, active, (0.3,), 32, group, G)[0]
    assert np.array_equal(other[:, :6], sums[:, :6])
    # two shards
    a = SR.score_replicates(v[:, :5], y_obs[:5], active[:5], levels, B, group[:5], G)[0]
    b = SR.score_replicates(v[:, 5:], y_obs[5:], active[5:], levels, B, group[5:], G)[0]
    assert np.array_equal((a + b)[:, rows], sums[:, rows]) and np.allclose(a + b, sums, rtol=1e-13, atol=0)
    # the margin: one cell moved onto a replicate's value has margin 0
    y3 = y_obs.copy()
    y3[0, 0] = v[3, 0, 0]
    active3 = active.copy()
    active3[0, 0] = 1
    assert SR.cells(v, y3, active3, levels, B)["margin"][0, 0] == 0.0
    assert np.all(c["margin"][~c["scored"]] == np.inf)


def test_from_score_and_merge():
    import torch
    import effect_ref as E
    import score_ref as SR
    from insite_amd import effect
    y0, u, arm, coef, exps, rng = _small(4)
    N, T = arm.shape
    levels, B, G = (0.5, 0.9, 0.95), 4, 2
    v = E.trajectories(y0, u, arm, coef, exps, 0.1, "rk4", 1)
    y_obs = v[3] + 0.05 * rng.normal(size=(N, T))
    active = np.ones((N, T), dtype=np.int8)
    active[:, T - 1] = 0                                                      # a step with no cell: 0 / 0
    group = np.arange(N) % G
    sums, _, _ = SR.score_replicates(v, y_obs, active, levels, B, group, G)
    scale = 4.0
    res = effect.from_score(torch.tensor(sums), levels, B, scale=scale)
    n = sums[:, 0]
    assert res.levels == levels and res.n_bins == B and res.sums.shape == (G, 6 + B + 9, T)
    assert np.array_equal(res.n.numpy(), n) and np.array_equal(res.n_bad.numpy(), sums[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.allclose(res.rmse_point.numpy(), np.sqrt(sums[:, 2] / n) / scale, rtol=1e-15, equal_nan=True)
        assert np.allclose(res.rmse_mean.numpy(), np.sqrt(sums[:, 3] / n) / scale, rtol=1e-15, equal_nan=True)
        assert np.allclose(res.spread.numpy(), np.sqrt(sums[:, 4] / n) / scale, rtol=1e-15, equal_nan=True)
        assert np.allclose(res.crps.numpy(), sums[:, 5] / n / scale, rtol=1e-15, equal_nan=True)
        assert np.allclose(res.pit_hist.numpy(), sums[:, 6:6 + B] / n[:, None], rtol=1e-15, equal_nan=True)
        lv = sums[:, 6 + B:].reshape(G, 3, 3, T)
        assert np.allclose(res.coverage.numpy(), lv[:, :, 0] / n[:, None], rtol=1e-15, equal_nan=True)
        assert np.allclose(res.width.numpy(), lv[:, :, 1] / n[:, None] / scale, rtol=1e-15, equal_nan=True)
        assert np.allclose(res.interval_score.numpy(), lv[:, :, 2] / n[:, None] / scale, rtol=1e-15, equal_nan=True)
    assert res.coverage.shape == (G, 3, T) and res.pit_hist.shape == (G, B, T)
    assert np.isnan(res.rmse_point.numpy()[:, T - 1]).all() and np.isnan(res.coverage.numpy()[:, :, T - 1]).all()
    assert np.allclose(res.pit_hist.numpy()[:, :, :T - 1].sum(axis=1), 1.0, rtol=1e-14)
    # pooled: the sums over the steps first, the division after
    tot = sums.sum(axis=2)
    p = res.pooled
    assert p["n"].shape == (G,) and np.array_equal(p["n"].numpy(), tot[:, 0])
    assert np.allclose(p["rmse_point"].numpy(), np.sqrt(tot[:, 2] / tot[:, 0]) / scale, rtol=1e-15)
    assert np.allclose(p["crps"].numpy(), tot[:, 5] / tot[:, 0] / scale, rtol=1e-15)
    assert np.allclose(p["coverage"].numpy(), tot[:, 6 + B::3] / tot[:, :1], rtol=1e-15)
    assert p["pit_hist"].shape == (G, B) and np.isfinite(p["interval_score"].numpy()).all()
    # merge: the shards' sums added
    a = SR.score_replicates(v[:, :5], y_obs[:5], active[:5], levels, B, group[:5], G)[0]
    b = SR.score_replicates(v[:, 5:], y_obs[5:], active[5:], levels, B, group[5:], G)[0]
    ra, rb = (effect.from_score(torch.tensor(s), levels, B, scale=scale) for s in (a, b))
    m = ra.merge(rb)
    assert np.array_equal(m.sums.numpy(), a + b) and np.array_equal(m.n.numpy(), n)
    assert np.allclose(m.crps.numpy(), res.crps.numpy(), rtol=1e-12, equal_nan=True)
    with pytest.raises(ValueError):
        ra.merge(effect.from_score(torch.tensor(b), levels, B, scale=1.0))
    with pytest.raises(ValueError):
        ra.merge(effect.from_score(torch.tensor(SR.score_replicates(v, y_obs, active, (0.5,), B)[0]), (0.5,), B))
    with pytest.raises(ValueError):
        effect.from_score(torch.tensor(sums), levels, B + 1)


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``score_bands`` raises as the other ensemble methods do: the joint, degree-4 and (before
    ``bootstrap_segments``) treatment-segment modes name the method, it needs ``bootstrap()`` first, at least one
    resample and at most the kernel's cap."""
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.sindy import SINDY
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
        m = SINDY(C.compose(["+backbone=sindy"] + cfg), device="cpu")
        with pytest.raises(NotImplementedError, match="score_bands"):
            m.score_bands(None)
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.score_bands(None)
    for Rn in (1, _lib.SCORE_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.EFFECT_MAX_REPLICATES)):
            m.score_bands(None)
