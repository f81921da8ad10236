"""CPU tests of the regimen-choice extension ABI (include/insite_regimen.h): header, bindings and exported symbols
agree, the six older headers did not move, every argument check answers before any HIP call, the plugin refuses what
it does not cover, the numpy restatement tests/regimen_ref.py (the reference of tests/test_gpu_regimen.py) agrees with
a brute-force loop and obeys the header's rules, and the inputs of the GPU parity cases leave no replicate's argmin
ambiguous."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_regimen.h")
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
    assert fns == sorted(_lib.REGIMEN_EXPORTS) and len(fns) == 3
    older = (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
             | set(_lib.EFFECT_EXPORTS) | set(_lib.COHORT_EXPORTS))
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_REGIMEN_ABI_VERSION") == _lib.REGIMEN_ABI_VERSION == 1
    assert const("INSITE_REGIMEN_MAX_REPLICATES") == _lib.REGIMEN_MAX_REPLICATES == 512
    assert const("INSITE_REGIMEN_MAX_QUANTILES") == _lib.REGIMEN_MAX_QUANTILES == 16
    assert const("INSITE_REGIMEN_MAX_PLANS") == _lib.REGIMEN_MAX_PLANS == 16
    assert const("INSITE_REGIMEN_MINIMIZE") == _lib.REGIMEN_MINIMIZE == 1
    assert const("INSITE_REGIMEN_MAXIMIZE") == _lib.REGIMEN_MAXIMIZE == -1
    assert L.insite_regimen_abi_version() == 1
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in fns:
        if name == "insite_regimen_abi_version":
            continue
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert L.insite_regimen_workspace_bytes(1000, 60, 2, 7, 256, 3, 8) == 0


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    assert len(_functions(os.path.join(inc, "insite_hip.h"))) == 43
    assert len(_functions(os.path.join(inc, "insite_irregular.h"))) == 4
    assert len(_functions(os.path.join(inc, "insite_weak.h"))) == 5
    assert len(_functions(os.path.join(inc, "insite_bootstrap.h"))) == 4
    assert len(_functions(os.path.join(inc, "insite_effect.h"))) == 3
    assert len(_functions(os.path.join(inc, "insite_cohort.h"))) == 5
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1 and L.insite_effect_abi_version() == 1
    assert L.insite_cohort_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5
    assert len(_lib.BOOT_EXPORTS) == 4 and len(_lib.EFFECT_EXPORTS) == 3 and len(_lib.COHORT_EXPORTS) == 5
    assert len(_lib.REGIMEN_EXPORTS) == 3


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.REGIMEN_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_regimen.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4096)()
    qs = np.array([0.025, 0.5, 0.975])
    qp = qs.ctypes.data_as(ctypes.c_void_p)
    q16 = np.linspace(0.0, 1.0, 17)
    qp16 = q16.ctypes.data_as(ctypes.c_void_p)

    # N = 5, T = 12, K = 3, Q = 3: ld_plan 12, plan_stride 60, ld_w 12, ld_out 3 * 2 * 6 = 36
    def call(y0=x, u=x, pl=x, K=3, ps=60, ldp=12, w=x, ldw=12, cost=x, sense=1, coef=x, e=ep, F=7, N=5, T=12, U=2,
             A=2, dt=0.1, m=0, sub=5, drop=1e-3, Rn=9, q=qp, Q=3, ch=x, win=x, out=x, ldo=36):
        return L.insite_regimen_choice_f64(y0, u, pl, K, ps, ldp, w, ldw, cost, sense, coef, e, F, N, T, U, A, dt, m,
                                           sub, drop, Rn, q, Q, ch, win, out, ldo, nul, 0, nul)

    # insite_effect_bands_f64's list
    assert call(y0=nul) == -1 and call(u=nul) == -1 and call(coef=nul) == -1 and call(e=nul) == -1
    assert call(N=-1) == -1 and call(T=0) == -1 and call(T=-3) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(A=0) == -1 and call(A=_lib.MAX_ARMS + 1) == -1
    assert call(F=0) == -1 and call(F=_lib.MAX_TERMS + 1) == -1
    assert call(sub=0) == -1 and call(dt=-0.1) == -1 and call(dt=float("nan")) == -1
    assert call(m=2) == -2 and call(m=-1) == -2
    assert call(Rn=1) == -1 and call(Rn=0) == -1 and call(Rn=-4) == -1
    assert call(Rn=_lib.REGIMEN_MAX_REPLICATES + 1) == -2 and call(Rn=513) == -2 and call(Rn=512, N=0) == 0
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                      # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call(q=nul) == -1 and call(Q=0) == -1 and call(Q=-1) == -1
    assert call(q=qp16, Q=_lib.REGIMEN_MAX_QUANTILES + 1, ldo=3 * 2 * 20) == -1
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        qb = np.array([0.5, bad, 0.1])
        assert call(q=qb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
    # this header's additions
    assert call(K=0) == -1 and call(K=-1) == -1 and call(K=17, ldo=17 * 2 * 6) == -1
    assert call(K=_lib.REGIMEN_MAX_PLANS + 1, ps=60, ldo=1 << 20) == -1
    assert call(sense=0) == -1 and call(sense=2) == -1 and call(sense=-2) == -1
    for ld in range(1, 12):
        assert call(ldp=ld) == -1, ld                                            # 0 < ld_plan < T
        assert call(ldw=ld) == -1, ld                                            # 0 < ld_w < T
    assert call(ldp=-1) == -1 and call(ldw=-1) == -1 and call(ps=-1) == -1
    assert call(ldp=0, ps=11) == -1                                              # shared plans: plan_stride >= T
    assert call(ps=59) == -1 and call(ps=12) == -1                               # plan_stride >= n_rows ld_plan
    assert call(ldp=13, ps=64) == -1
    assert call(ldo=35) == -1 and call(ldo=0) == -1 and call(ldo=-36) == -1
    assert call(q=qp16, Q=16, ldo=3 * 2 * 19 - 1) == -1 and call(K=16, ps=60, ldo=16 * 2 * 6 - 1) == -1
    assert call(pl=nul) == -1 and call(w=nul) == -1 and call(ch=nul) == -1 and call(win=nul) == -1
    assert call(out=nul) == -1
    # strides whose largest offset leaves int64
    big = (1 << 62)
    assert call(ps=big) == -1 and call(ldw=big) == -1 and call(ldo=big) == -1 and call(ldp=big, ps=big) == -1
    # n_rows = 0: a successful no-op, whatever the pointers (the accepted side of every bound above: a valid call with
    # rows would launch); still validated
    assert call(N=0) == 0
    assert call(N=0, ldp=0, ps=12) == 0 and call(N=0, ldp=13, ps=65) == 0 and call(N=0, ldw=0) == 0
    assert call(N=0, ldw=40) == 0 and call(N=0, ldo=36) == 0 and call(N=0, q=qp16, Q=16, ldo=3 * 2 * 19) == 0
    assert call(N=0, cost=nul) == 0 and call(N=0, sense=-1) == 0 and call(N=0, K=1) == 0
    assert call(N=0, K=16, ldo=16 * 2 * 6) == 0
    assert call(N=0, y0=nul, u=nul, pl=nul, w=nul, cost=nul, coef=nul, ch=nul, win=nul, out=nul) == 0
    assert call(N=0, K=2, ps=big, ldp=big, ldw=big, ldo=big) == 0 and call(N=0, ps=12) == 0
    assert call(N=0, K=3, ps=big) == -1                                          # 2 plan_stride leaves int64
    assert call(N=0, Rn=1) == -1 and call(N=0, T=0) == -1 and call(N=0, K=17) == -1 and call(N=0, K=0) == -1
    assert call(N=0, sense=0) == -1 and call(N=0, ldp=5) == -1 and call(N=0, ldw=5) == -1
    assert call(N=0, ldo=35) == -1 and call(N=0, ps=11) == -1 and call(N=0, Rn=513) == -2
    assert call(N=0, q=nul) == -1 and call(N=0, e=nul) == -1 and call(N=0, m=3) == -2


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0 = torch.zeros(4, dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    plans = torch.zeros((3, 4, 6), dtype=torch.int8)
    w = torch.zeros((4, 6), dtype=torch.float64)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    for fn in (ops.regimen_choice, ops.plan_regimen_choice):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, plans, coef, lib, 0.1, (0.1, 0.9), w)
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, plans[:, 0], coef, lib, 0.1, (0.1, 0.9), w[0], cost=torch.zeros(3, dtype=torch.float64))


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``choose_plan`` covers the per-arm EQ_4 model over the affine library: the joint, treatment-segment and
    degree-4 modes raise, naming the method; it needs ``bootstrap()`` first, at least one resample and at most the
    kernel's cap (named in the message), and between 1 and 16 plans."""
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.sindy import SINDY
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="choose_plan"):
                m.choose_plan(None, [0, 1])
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.choose_plan(None, [0, 1])
    for Rn in (1, _lib.REGIMEN_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.REGIMEN_MAX_REPLICATES)):
            m.choose_plan(None, [0, 1])
    assert _lib.REGIMEN_MAX_REPLICATES == _lib.EFFECT_MAX_REPLICATES == 512
    coef = torch.zeros((9, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    with pytest.raises(ValueError, match="1 to 16"):
        m.choose_plan(None, [])
    with pytest.raises(ValueError, match="1 to 16"):
        m.choose_plan(None, [0] * 17)
    with pytest.raises(ValueError, match="1 to 16"):
        m.choose_plan(None, 0)
    with pytest.raises(ValueError, match="costs"):
        m.choose_plan(None, [0, 1], costs=[0.0])


def test_regimen_result_scaling():
    """``effect.from_regimen``: the locations of the value series are shifted (per row) and divided, its spread and
    the regret divided only."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(2)
    out = torch.tensor(rng.normal(size=(4, 3, 2, 5)))            # [N, K, 2, 3 + Q]
    choice = torch.tensor([0, 2, -1, 1], dtype=torch.int32)
    win = torch.tensor(rng.random((4, 3)))
    shift = torch.tensor(rng.normal(size=4))
    res = effect.from_regimen(choice, win, out, (0.1, 0.9), shift=shift, scale=4.0)
    assert res.series == ("value", "regret") and res.q == (0.1, 0.9) and res.choice is choice and res.win is win
    o = out.numpy().transpose(2, 3, 0, 1)                        # [2, 3 + Q, N, K]
    sh = shift.numpy()[:, None]
    assert res.point.shape == (2, 4, 3) and res.quantiles.shape == (2, 2, 4, 3)
    assert np.array_equal(res.point.numpy()[0], (o[0, 0] - sh) / 4.0)
    assert np.array_equal(res.mean.numpy()[0], (o[0, 1] - sh) / 4.0)
    assert np.array_equal(res.quantiles.numpy()[0], (o[0, 3:] - sh) / 4.0)
    assert np.array_equal(res.std.numpy(), o[:, 2] / 4.0)
    assert np.array_equal(res.point.numpy()[1], o[1, 0] / 4.0)
    assert np.array_equal(res.quantiles.numpy()[1], o[1, 3:] / 4.0)
    assert np.array_equal(res["regret"]["mean"].numpy(), o[1, 1] / 4.0)
    flat = effect.from_regimen(choice, win, out, (0.1, 0.9), shift=2.0, scale=4.0)
    assert np.array_equal(flat.mean.numpy()[0], (o[0, 1] - 2.0) / 4.0)
    with pytest.raises(ValueError):
        effect.from_regimen(choice, win, out[:, :, :1], (0.1, 0.9))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def _small(seed, Rn, N, T, A, K, name="std7"):
    import regimen_ref as G
    y0, u, plans, w, cost, coef = G.inputs(("regimen-small", seed), Rn, N, T, A, K, name)
    return y0, u, np.ascontiguousarray(plans[..., :T]), np.ascontiguousarray(w[..., :T]), cost, coef


def test_reference_against_brute_force():
    """The restatement against loops over (replicate, row, plan) with nothing vectorised."""
    import effect_ref as E
    import library_matrix as M
    import regimen_ref as G
    Rn, N, T, A, K = 9, 4, 7, 2, 3
    q = (0.0, 0.3, 1.0)
    y0, u, plans, w, cost, coef = _small(1, Rn, N, T, A, K)
    exps = M.exps_of("std7")
    for sense in (1, -1):
        ref = G.regimen(y0, u, plans, coef, exps, 0.1, q, w, cost, sense, "euler", 5)
        ys = [E.trajectories(y0, u, plans[j], coef, exps, 0.1, "euler", 5) for j in range(K)]
        for p in range(N):
            votes = [0] * K
            J = np.empty((Rn, K))
            g = np.empty((Rn, K))
            for r in range(Rn):
                for j in range(K):
                    acc = float(cost[j])
                    for k in range(T):
                        acc = acc + w[p, k] * ys[j][r, p, k]
                    J[r, j] = acc
                best = 0
                for j in range(1, K):
                    if sense * J[r, j] < sense * J[r, best]:
                        best = j
                for j in range(K):
                    g[r, j] = sense * J[r, j] - sense * J[r, best]
                assert g[r].min() == 0.0 and g[r, best] == 0.0
                if r == 0:
                    assert ref["choice"][p] == best
                else:
                    votes[best] += 1
            assert np.array_equal(ref["win"][p], np.array(votes) / (Rn - 1.0))
            for j in range(K):
                for s, v in enumerate((J[:, j], g[:, j])):
                    rep = sorted(v[1:])
                    got = ref["out"][p, j, s]
                    assert got[0] == v[0]
                    assert abs(got[1] - sum(rep) / len(rep)) <= 1e-14 * max(1.0, abs(got[1]))
                    assert abs(got[2] - np.std(v[1:], ddof=1)) <= 1e-13
                    assert got[3] == rep[0] and got[5] == rep[-1]
                    pos = 0.3 * (len(rep) - 1)
                    i = int(np.floor(pos))
                    assert abs(got[4] - (rep[i] + (pos - i) * (rep[i + 1] - rep[i]))) <= 1e-14


def test_reference_rules():
    """Ties go to the lower index, a replicate with a NaN objective abstains, maximise is minimise of (-w, -cost),
    and K = 1 gives win = 1 and regret = 0."""
    import library_matrix as M
    import regimen_ref as G
    Rn, N, T, A, K = 9, 5, 6, 2, 4
    q = (0.0, 0.5, 1.0)
    exps = M.exps_of("std7")
    y0, u, plans, w, cost, coef = _small(2, Rn, N, T, A, K)
    base = G.regimen(y0, u, plans, coef, exps, 0.1, q, w, cost, 1, "rk4", 1)
    assert (base["win"].sum(axis=1) == 1.0).all() and (base["out"][:, :, 1] >= 0).all()
    # plan 2 a copy of plan 0 (same cost): bitwise-equal objectives, and plan 2 never wins
    p2 = plans.copy()
    p2[2] = p2[0]
    c2 = cost.copy()
    c2[2] = c2[0]
    tie = G.regimen(y0, u, p2, coef, exps, 0.1, q, w, c2, 1, "rk4", 1)
    assert np.array_equal(tie["out"][:, 2, 0], tie["out"][:, 0, 0]) and (tie["win"][:, 2] == 0).all()
    assert (tie["choice"] != 2).all() and (tie["win"][:, 0] > 0).any()
    # maximise (w, cost) = minimise (-w, -cost): the same choice, votes and regret, the values negated
    mx = G.regimen(y0, u, plans, coef, exps, 0.1, q, w, cost, -1, "rk4", 1)
    mn = G.regimen(y0, u, plans, coef, exps, 0.1, q, -w, -cost, 1, "rk4", 1)
    assert np.array_equal(mx["choice"], mn["choice"]) and np.array_equal(mx["win"], mn["win"])
    assert np.array_equal(mx["out"][:, :, 1], mn["out"][:, :, 1])
    assert np.array_equal(mx["out"][:, :, 0, 0], -mn["out"][:, :, 0, 0])
    assert not np.array_equal(mx["choice"], base["choice"])
    # a replicate with NaN coefficients abstains: its vote is nobody's, the regret statistics are NaN
    cn = coef.copy()
    cn[4] = np.nan
    ab = G.regimen(y0, u, plans, cn, exps, 0.1, q, w, cost, 1, "rk4", 1)
    assert np.allclose(ab["win"].sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=1e-15)
    assert (ab["best"][4] == -1).all() and np.array_equal(ab["choice"], base["choice"])
    assert np.isnan(ab["out"][:, :, :, 1:]).all() and np.array_equal(ab["out"][..., 0], base["out"][..., 0])
    # NaN only in arm 1, and plan 0 never uses arm 1: its value stays finite, the replicate still abstains
    cn = coef.copy()
    cn[4, 1, 2] = np.nan
    p0 = plans.copy()
    p0[0] = 0
    p0[1:, :, 0] = 1
    ab = G.regimen(y0, u, p0, cn, exps, 0.1, q, w, cost, 1, "rk4", 1)
    assert np.isfinite(ab["out"][:, 0, 0]).all() and np.isnan(ab["out"][:, 1:, 0, 1:]).all()
    assert np.isnan(ab["out"][:, :, 1, 1:]).all() and (ab["best"][4] == -1).all()
    # a NaN reaches J under weight 0
    w0 = w.copy()
    w0[:, 0] = 0.0
    ab = G.regimen(y0, u, p0, cn, exps, 0.1, q, w0, cost, 1, "rk4", 1)
    assert np.isnan(ab["J"][4, :, 1:]).all()
    # K = 1
    one = G.regimen(y0, u, plans[:1], coef, exps, 0.1, q, w, cost[:1], 1, "rk4", 1)
    assert (one["choice"] == 0).all() and (one["win"] == 1.0).all() and np.isinf(one["margin"]).all()
    reg = np.delete(one["out"][:, 0, 1], 2, axis=-1)
    assert (reg == 0.0).all() and not np.signbit(reg).any()


def test_parity_case_inputs_are_unambiguous():
    """The input conditions of the GPU parity cases.  min_p m_p >= 1e-8 in every case: no replicate's argmin is
    ambiguous at the GPU tolerance of 1e-10 of the scale, so ``choice`` and ``win`` are compared exactly there.  Every
    case with K >= 2 and R >= 17 has at least two distinct winners and a row with a split vote: the argmin comparison
    is not vacuous."""
    import regimen_ref as G
    for c, cid in zip(G.CASES, G.CASE_IDS):
        ref = G.case(*c)[-1]
        Rn, K = c[0], c[4]
        m = float(ref["margin"].min())
        winners = np.unique(ref["best"][ref["best"] >= 0])
        split = int(((ref["win"] > 0) & (ref["win"] < 1)).any(axis=1).sum())
        print(f"{cid}: smallest margin {m:.3e}, {winners.size} distinct winners, split votes in {split} rows")
        assert m >= 1e-8, cid
        assert not np.isnan(ref["out"]).any() or Rn == 2, cid
        if K >= 2 and Rn >= 17:
            assert winners.size >= 2, cid
            assert split >= 1, cid
