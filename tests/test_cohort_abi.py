"""CPU tests of the cohort-effect extension ABI (include/insite_cohort.h): header, bindings and exported symbols
agree, the five older headers did not move, every argument check answers before any HIP call, the workspace query
stays below 1 GiB, and the numpy restatement tests/cohort_effect_ref.py (the reference of
tests/test_gpu_cohort_effect.py) agrees with a literally repeated cohort and with tests/effect_ref.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_cohort.h")
FN_RE = r"^\s*(?:const\s+char\s*\*|int32_t|size_t)\s+(insite_\w+)\s*\("

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from insite_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _functions(header):
    return sorted(set(re.findall(FN_RE, open(header).read(), re.M)))


def test_header_and_bindings_agree(L):
    from insite_amd import _lib
    fns = _functions(HEADER)
    assert fns == sorted(_lib.COHORT_EXPORTS) and len(fns) == 5
    older = (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
             | set(_lib.EFFECT_EXPORTS))
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_COHORT_ABI_VERSION") == _lib.COHORT_ABI_VERSION == 1
    assert const("INSITE_COHORT_MAX_REPLICATES") == _lib.COHORT_MAX_REPLICATES == 4096
    assert const("INSITE_COHORT_MAX_GROUPS") == _lib.COHORT_MAX_GROUPS == 64
    assert const("INSITE_COHORT_MAX_QUANTILES") == _lib.COHORT_MAX_QUANTILES == 16
    assert const("INSITE_COHORT_WEIGHT_NONE") == _lib.COHORT_WEIGHT_NONE == 0
    assert const("INSITE_COHORT_WEIGHT_POISSON") == _lib.COHORT_WEIGHT_POISSON == 1
    assert L.insite_cohort_abi_version() == 1
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in fns:
        if name == "insite_cohort_abi_version":
            continue
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    assert len(_functions(os.path.join(inc, "insite_hip.h"))) == 43
    assert len(_functions(os.path.join(inc, "insite_irregular.h"))) == 4
    assert len(_functions(os.path.join(inc, "insite_weak.h"))) == 5
    assert len(_functions(os.path.join(inc, "insite_bootstrap.h"))) == 4
    assert len(_functions(os.path.join(inc, "insite_effect.h"))) == 3
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1 and L.insite_effect_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5
    assert len(_lib.BOOT_EXPORTS) == 4 and len(_lib.EFFECT_EXPORTS) == 3 and len(_lib.COHORT_EXPORTS) == 5


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.COHORT_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_cohort.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4096)()
    qs = np.array([0.025, 0.5, 0.975])
    qp = qs.ctypes.data_as(ctypes.c_void_p)
    wsb = L.insite_cohort_effect_workspace_bytes
    big = 1 << 30

    def sums(y0=x, u=x, aa=x, lda=12, ab=x, ldb=12, coef=x, e=ep, F=7, N=5, T=12, U=2, A=2, dt=0.1, m=0, sub=5,
             drop=1e-3, Rn=9, grp=x, G=3, wt=1, seed=7, off=0, s=x, lds=12, w=x, ws=x, wsn=big):
        return L.insite_cohort_effect_sums_f64(y0, u, aa, lda, ab, ldb, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn,
                                               grp, G, wt, seed, off, s, lds, w, ws, wsn, nul)

    def both(y0=x, u=x, aa=x, lda=12, ab=x, ldb=12, coef=x, e=ep, F=7, N=5, T=12, U=2, A=2, dt=0.1, m=0, sub=5,
             drop=1e-3, Rn=9, grp=x, G=3, wt=1, seed=7, off=0, s=x, lds=12, w=x, q=qp, Q=3, out=x, ldo=12, ws=x,
             wsn=big):
        return L.insite_cohort_effect_f64(y0, u, aa, lda, ab, ldb, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn, grp, G,
                                          wt, seed, off, s, lds, w, q, Q, out, ldo, ws, wsn, nul)

    def fin(s=x, lds=12, w=x, Rn=9, G=3, ns=2, T=12, q=qp, Q=3, out=x, ldo=12):
        return L.insite_cohort_effect_finalize_f64(s, lds, w, Rn, G, ns, T, q, Q, out, ldo, nul)

    for call in (sums, both):
        # insite_effect_bands_f64's list
        assert call(y0=nul) == -1 and call(u=nul) == -1 and call(aa=nul) == -1 and call(coef=nul) == -1
        assert call(e=nul) == -1
        assert call(N=-1) == -1 and call(T=0) == -1 and call(T=-3) == -1 and call(U=-1) == -1 and call(U=4) == -1
        assert call(A=0) == -1 and call(A=_lib.MAX_ARMS + 1) == -1
        assert call(F=0) == -1 and call(F=_lib.MAX_TERMS + 1) == -1
        assert call(lda=11) == -1 and call(ldb=11) == -1 and call(lds=11) == -1
        assert call(sub=0) == -1 and call(dt=-0.1) == -1 and call(dt=float("nan")) == -1
        assert call(m=2) == -2 and call(m=-1) == -2
        assert call(Rn=1) == -1 and call(Rn=0) == -1 and call(Rn=-4) == -1
        assert call(Rn=_lib.COHORT_MAX_REPLICATES + 1) == -2 and call(Rn=4097) == -2
        e2 = exps.copy()
        e2[1, 0] = 2
        assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                      # state exponent above 1
        e3 = exps.copy()
        e3[2, 1] = -1
        assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
        # this header's additions
        assert call(G=0) == -1 and call(G=-1) == -1 and call(G=65) == -1
        assert call(G=_lib.COHORT_MAX_GROUPS + 1) == -1
        assert call(wt=2) == -1 and call(wt=-1) == -1
        assert call(off=-1) == -1
        assert call(s=nul) == -1 and call(w=nul) == -1
        assert call(ws=nul) == -1 and call(wsn=wsb(5, 12, 2, 7, 9, 3) - 1) == -1
        # n_rows = 0: a successful no-op, whatever the cohort's pointers; an unused arm_b takes any leading dimension
        assert call(N=0) == 0
        assert call(N=0, y0=nul, u=nul, aa=nul, coef=nul, grp=nul, s=nul, w=nul, ws=nul, wsn=0) == 0
        assert call(N=0, ab=nul, ldb=0) == 0 and call(N=0, Rn=4096, G=64, wt=0) == 0
        assert call(N=0, Rn=1) == -1 and call(N=0, T=0) == -1 and call(N=0, G=65) == -1     # still validated
        assert call(N=0, wt=5) == -1 and call(N=0, off=-2) == -1 and call(N=0, Rn=4097) == -2
    assert wsb(5, 12, 2, 7, 9, 3) > 0
    # the quantile and output rules of the combined call and of finalize
    for call in (both, fin):
        assert call(q=nul) == -1 and call(out=nul) == -1 and call(ldo=11) == -1
        assert call(Q=0) == -1 and call(Q=_lib.COHORT_MAX_QUANTILES + 1) == -1 and call(Q=-1) == -1
        for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
            qb = np.array([0.5, bad, 0.1])
            assert call(q=qb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
    assert both(N=0, out=nul) == -1 and both(N=0, q=nul) == -1
    assert fin(s=nul) == -1 and fin(w=nul) == -1 and fin(lds=11) == -1 and fin(T=0) == -1
    assert fin(Rn=1) == -1 and fin(Rn=4097) == -2 and fin(G=0) == -1 and fin(G=65) == -1
    assert fin(ns=0) == -1 and fin(ns=3) == -1


def test_workspace_query(L):
    wsb = L.insite_cohort_effect_workspace_bytes
    GiB = 1 << 30
    assert 0 < wsb(1_000_000, 60, 4, 9, 4096, 64) < GiB
    for N, T, A, F, Rn, G in ((1, 1, 1, 1, 2, 1), (130, 33, 2, 7, 65, 3), (1_000_000, 60, 2, 7, 256, 1),
                              (1_000_000, 60, 2, 7, 256, 8), (100_000_000, 60, 2, 7, 4096, 1),
                              (5000, 8, 2, 7, 65, 64), (10_000_000, 255, 4, 9, 4096, 64)):
        b = wsb(N, T, A, F, Rn, G)
        assert 0 < b < GiB, (N, T, Rn, G)
        # at least one chunk's partials: G x ceil(R / 64) x 64 x (2 T + 1) doubles
        assert b >= G * ((Rn + 63) // 64) * 64 * (2 * T + 1) * 8 and b % 8 == 0
    # invalid arguments, no rows, and a shape whose single-chunk partial passes 1 GiB: 0
    assert wsb(-1, 60, 2, 7, 256, 1) == 0 and wsb(0, 60, 2, 7, 256, 1) == 0
    assert wsb(10, 0, 2, 7, 256, 1) == 0 and wsb(10, 60, 0, 7, 256, 1) == 0 and wsb(10, 60, 5, 7, 256, 1) == 0
    assert wsb(10, 60, 2, 0, 256, 1) == 0 and wsb(10, 60, 2, 10, 256, 1) == 0
    assert wsb(10, 60, 2, 7, 1, 1) == 0 and wsb(10, 60, 2, 7, 4097, 1) == 0
    assert wsb(10, 60, 2, 7, 256, 0) == 0 and wsb(10, 60, 2, 7, 256, 65) == 0
    assert wsb(10, 100_000, 2, 7, 4096, 64) == 0


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0 = torch.zeros(4, dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros((4, 6), dtype=torch.int8)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    for fn in (ops.cohort_effect, ops.plan_cohort_effect):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, arm, arm, coef, lib, 0.1, (0.1, 0.9))
    with pytest.raises(ValueError, match="device tensor"):
        ops.cohort_effect_sums(y0, u, arm, None, coef, lib, 0.1)
    with pytest.raises(ValueError, match="device tensor"):
        ops.cohort_effect_finalize(torch.zeros((5, 1, 2, 6), dtype=torch.float64),
                                   torch.zeros((5, 1), dtype=torch.float64), (0.5,))


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``average_effect`` covers the per-arm EQ_4 model over the affine library: the joint, treatment-segment and
    degree-4 modes raise, naming the method; it needs ``bootstrap()`` first, at least one resample and at most the
    cohort kernel's cap, a seed for "independent", and two plans."""
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.sindy import SINDY
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="average_effect"):
                m.average_effect(None, 0)
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.average_effect(None, 0)
    for Rn in (1, _lib.COHORT_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.COHORT_MAX_REPLICATES)):
            m.average_effect(None, 0)
    # between the two caps: the per-row methods still name theirs, the averaged path does not refuse the count
    Rn = _lib.EFFECT_MAX_REPLICATES + 1
    coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
    for call in (lambda: m.predict_bands(None), lambda: m.treatment_effect(None, 0)):
        with pytest.raises(ValueError, match=str(_lib.EFFECT_MAX_REPLICATES)):
            call()
    with pytest.raises(ValueError, match="two plans"):
        m.average_effect(None, None, None)
    with pytest.raises(ValueError, match="independent"):
        m.average_effect(None, 0, resample="independent")
    with pytest.raises(ValueError, match="independent"):
        m.average_effect(None, 0, resample="independent", seed=3)
    with pytest.raises(ValueError, match="resample"):
        m.average_effect(None, 0, resample="rows")
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8))      # no seed recorded
    with pytest.raises(ValueError, match="paired"):
        m.average_effect(None, 0)


def test_cohort_result_scaling():
    """``effect.from_cohort``: locations of a and b are shifted and divided, spreads and the effect divided only."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(2)
    out = torch.tensor(rng.normal(size=(4, 3, 5, 6)))            # [G, S, 3 + Q, T]
    wsum = torch.tensor(rng.integers(1, 9, (7, 4)).astype(np.float64))
    res = effect.from_cohort(out, wsum, (0.1, 0.9), shift=2.0, scale=4.0)
    assert res.series == ("a", "b", "effect") and res.q == (0.1, 0.9) and res.weight_sum is wsum
    o = out.numpy().transpose(1, 2, 0, 3)                        # [S, 3 + Q, G, T]
    assert res.point.shape == (3, 4, 6) and res.quantiles.shape == (3, 2, 4, 6)
    assert np.array_equal(res.point.numpy()[:2], (o[:2, 0] - 2.0) / 4.0)
    assert np.array_equal(res.mean.numpy()[:2], (o[:2, 1] - 2.0) / 4.0)
    assert np.array_equal(res.quantiles.numpy()[:2], (o[:2, 3:] - 2.0) / 4.0)
    assert np.array_equal(res.std.numpy(), o[:, 2] / 4.0)
    assert np.array_equal(res.point.numpy()[2], o[2, 0] / 4.0)
    assert np.array_equal(res.quantiles.numpy()[2], o[2, 3:] / 4.0)
    assert np.array_equal(res["effect"]["mean"].numpy(), o[2, 1] / 4.0)
    one = effect.from_cohort(out[:, :1], wsum, (0.1, 0.9), shift=2.0, scale=4.0)
    assert one.series == ("a",) and np.array_equal(one.mean.numpy()[0], (o[0, 1] - 2.0) / 4.0)
    with pytest.raises(ValueError):
        effect.from_cohort(out[:, :2], wsum, (0.1, 0.9))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def _small(seed, Rn, N, T, A, name="std7"):
    import library_matrix as M
    rng = np.random.default_rng(seed)
    exps = M.exps_of(name)
    F = exps.shape[0]
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, M.TABLE[name][1]))
    arm_a = rng.integers(0, A, (N, T)).astype(np.int8)
    arm_b = rng.integers(0, A, (N, T)).astype(np.int8)
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[0] = base
    return y0, u, arm_a, arm_b, coef, exps


def test_reference_weighted_mean_is_the_repeated_cohort():
    """The weighted mean of the restatement equals the plain mean over the cohort with every patient literally
    repeated w times, to 1e-13 of the scale, per replicate and group; wsum is the number of repeated rows."""
    import cohort_effect_ref as CR
    import effect_ref as E
    Rn, N, T, A, G = 9, 40, 12, 2, 3
    y0, u, arm_a, arm_b, coef, exps = _small(5, Rn, N, T, A)
    group = np.arange(N) % G
    group[7] = -1
    group[11] = G
    _, S, wsum, scale = CR.cohort(y0, u, arm_a, arm_b, coef, exps, 0.1, (0.5,), group, G, "poisson", seed=7,
                                  patient_offset=3, method="euler", substeps=5)
    m = CR.means(S, wsum)
    w = CR.weights("poisson", 7, Rn, N, 3)
    assert (w[0] == 1).all() and (w[1:] == 0).any() and (w[1:] > 1).any()
    ys = [E.trajectories(y0, u, a, coef, exps, 0.1, "euler", 5) for a in (arm_a, arm_b)]
    worst = 0.0
    for r in range(Rn):
        for g in range(G):
            rep = np.repeat(np.nonzero(group == g)[0], w[r, group == g])
            assert wsum[r, g] == rep.size and rep.size > 0
            for s in range(2):
                worst = max(worst, np.max(np.abs(ys[s][r, rep].mean(axis=0) - m[r, g, s]) / scale[g]))
            d = ys[0][r, rep].mean(axis=0) - ys[1][r, rep].mean(axis=0)
            worst = max(worst, np.max(np.abs(d - m[r, g, 2]) / scale[g]))
    print(f"worst |repeated - weighted| / s = {worst:.3e}")
    assert worst <= 1e-13


def test_reference_none_is_the_row_mean_of_the_bands():
    """Under "none" the point and mean rows of every series are the row-mean of ``effect_ref.bands``' point and mean
    (the mean is linear); the quantiles are not (the replicates' trajectories cross), so they differ."""
    import cohort_effect_ref as CR
    import effect_ref as E
    Rn, N, T, A = 33, 30, 12, 2
    q = (0.025, 0.5, 0.975)
    y0, u, arm_a, arm_b, coef, exps = _small(6, Rn, N, T, A)
    out, _, wsum, scale = CR.cohort(y0, u, arm_a, arm_b, coef, exps, 0.1, q, None, 1, "none", method="rk4",
                                    substeps=1)
    assert (wsum == N).all()
    bands, _ = E.bands(y0, u, arm_a, arm_b, coef, exps, 0.1, q, "rk4", 1)       # [3, 3 + Q, N, T]
    rows = bands.mean(axis=2)                                                   # [3, 3 + Q, T]
    for st in (0, 1):
        assert np.max(np.abs(out[0, :, st] - rows[:, st]) / scale[0]) <= 1e-13, st
    # the band of the mean is narrower than the mean of the bands wherever the rows' replicates cross
    assert np.max(np.abs(out[0, :, 3:] - rows[:, 3:]) / scale[0]) > 1e-6
    width = out[0, :, 5] - out[0, :, 3]
    assert (width <= (rows[:, 5] - rows[:, 3]) + 1e-12).all()


def test_reference_rules():
    """The select rule, the excluded rows and the empty replicate, on the restatement itself."""
    import cohort_effect_ref as CR
    Rn, N, T, A = 9, 6, 5, 2
    y0, u, arm_a, arm_b, coef, exps = _small(8, Rn, N, T, A)
    w = CR.weights("poisson", 7, Rn, N)
    r, p = [int(v[0]) for v in np.nonzero(w == 0)]
    y0n = y0.copy()
    y0n[p] = np.nan
    _, S, wsum, _ = CR.cohort(y0n, u, arm_a, arm_b, coef, exps, 0.1, (0.5,), None, 1, "poisson", seed=7,
                              method="euler", substeps=1)
    assert np.isfinite(S[r]).all() and np.isnan(S[0]).all()
    assert np.array_equal(wsum[:, 0], w.sum(axis=1))
    group = np.array([0, -1, 0, 1, 0, 0])
    base = CR.cohort(y0, u, arm_a, arm_b, coef, exps, 0.1, (0.5,), group, 1, "poisson", seed=7, method="euler",
                     substeps=1)
    y0n = y0.copy()
    y0n[[1, 3]] = np.nan
    other = CR.cohort(y0n, u, arm_a, arm_b, coef, exps, 0.1, (0.5,), group, 1, "poisson", seed=7, method="euler",
                      substeps=1)
    for a, b in zip(base, other):
        assert np.array_equal(a, b, equal_nan=True) and np.isfinite(a).any()
    # one row that replicate r does not draw: NaN statistics, a finite point, an exact wsum
    w1 = CR.weights("poisson", 7, Rn, 1)
    assert (w1[1:, 0] == 0).any()
    out, _, wsum, _ = CR.cohort(y0[:1], u[:1], arm_a[:1], arm_b[:1], coef, exps, 0.1, (0.5,), None, 1, "poisson",
                                seed=7, method="euler", substeps=1)
    assert np.isnan(out[0, :, 1:]).all() and np.isfinite(out[0, :, 0]).all()
    assert np.array_equal(wsum[:, 0], w1[:, 0])
