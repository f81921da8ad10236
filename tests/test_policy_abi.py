"""CPU tests of the policy-value extension ABI (include/insite_policy.h): header, bindings and exported symbols agree,
the seven older headers did not move, every argument check and cap answers before any HIP call, the workspace query,
the plugin refuses what it does not cover, the numpy restatement tests/policy_ref.py (the reference of
tests/test_gpu_policy.py) agrees with a brute-force triple loop, and the inputs of the GPU parity cases leave no argmin
ambiguous -- neither a row's inside a replicate nor a group's best fixed plan."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_policy.h")
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
    assert fns == sorted(_lib.POLICY_EXPORTS) and len(fns) == 5
    older = (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
             | set(_lib.EFFECT_EXPORTS) | set(_lib.COHORT_EXPORTS) | set(_lib.REGIMEN_EXPORTS))
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_POLICY_ABI_VERSION") == _lib.POLICY_ABI_VERSION == 1
    assert const("INSITE_POLICY_MAX_REPLICATES") == _lib.POLICY_MAX_REPLICATES == 4096
    assert const("INSITE_POLICY_MAX_PLANS") == _lib.POLICY_MAX_PLANS == 16
    assert const("INSITE_POLICY_MAX_GROUPS") == _lib.POLICY_MAX_GROUPS == 64
    assert const("INSITE_POLICY_MAX_QUANTILES") == _lib.POLICY_MAX_QUANTILES == 16
    assert L.insite_policy_abi_version() == 1
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in fns:
        if name == "insite_policy_abi_version":
            continue
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    for header, n in (("insite_hip.h", 43), ("insite_irregular.h", 4), ("insite_weak.h", 5), ("insite_bootstrap.h", 4),
                      ("insite_effect.h", 3), ("insite_cohort.h", 5), ("insite_regimen.h", 3)):
        assert len(_functions(os.path.join(inc, header))) == n, header
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1 and L.insite_effect_abi_version() == 1
    assert L.insite_cohort_abi_version() == 1 and L.insite_regimen_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5
    assert len(_lib.BOOT_EXPORTS) == 4 and len(_lib.EFFECT_EXPORTS) == 3 and len(_lib.COHORT_EXPORTS) == 5
    assert len(_lib.REGIMEN_EXPORTS) == 3 and len(_lib.POLICY_EXPORTS) == 5


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.POLICY_EXPORTS:
        assert name in syms, name


def test_workspace_query(L):
    """The rule (4 bytes per row, rounded up to 8) plus the chunks' partials: G x ceil(R / 64) x 64 x (2 K + 3)
    doubles per chunk, one chunk per 64 rows until 8192 waves are out; 0 for invalid or unsupported shapes."""
    ws = L.insite_policy_workspace_bytes
    assert ws(1000, 60, 2, 7, 256, 8, 8) == 4000 + 16 * (8 * 4 * 19 * 64 * 8)
    assert ws(1, 1, 1, 1, 2, 1, 1) == 8 + 1 * 1 * 5 * 64 * 8
    assert ws(3, 60, 2, 7, 65, 3, 16) == 16 + 3 * 2 * 35 * 64 * 8
    # many rows: the chunk count stops at 8192 / (n_rt G) and the partials stay below 1 GiB
    big = ws(10 ** 7, 60, 2, 7, 4096, 64, 16)
    assert big == 4 * 10 ** 7 + 2 * (64 * 64 * 35 * 64 * 8) and big - 4 * 10 ** 7 < 1 << 30
    assert ws(0, 60, 2, 7, 256, 8, 8) == 0 and ws(-1, 60, 2, 7, 256, 8, 8) == 0 and ws(10, 0, 2, 7, 256, 8, 8) == 0
    assert ws(10, 60, 0, 7, 256, 8, 8) == 0 and ws(10, 60, 5, 7, 256, 8, 8) == 0 and ws(10, 60, 2, 0, 256, 8, 8) == 0
    assert ws(10, 60, 2, 10, 256, 8, 8) == 0 and ws(10, 60, 2, 7, 1, 8, 8) == 0 and ws(10, 60, 2, 7, 4097, 8, 8) == 0
    assert ws(10, 60, 2, 7, 256, 0, 8) == 0 and ws(10, 60, 2, 7, 256, 65, 8) == 0 and ws(10, 60, 2, 7, 256, 8, 0) == 0
    assert ws(10, 60, 2, 7, 256, 8, 17) == 0 and ws((1 << 62), 60, 2, 7, 256, 8, 8) == 0
    assert ws(10, 60, 2, 7, 4096, 64, 16) > 0


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_policy.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4096)()
    qs = np.array([0.025, 0.5, 0.975])
    qp = qs.ctypes.data_as(ctypes.c_void_p)
    q17 = np.linspace(0.0, 1.0, 17)
    qp17 = q17.ctypes.data_as(ctypes.c_void_p)
    big = 1 << 62

    # N = 5, T = 12, K = 3, Q = 3: ld_plan 12, plan_stride 60, ld_w 12, ld_out 6
    def head(y0=x, u=x, pl=x, K=3, ps=60, ldp=12, w=x, ldw=12, cost=x, sense=1, coef=x, e=ep, F=7, N=5, T=12, U=2,
             A=2, dt=0.1, m=0, sub=5, drop=1e-3, Rn=9, grp=x, G=2, wt=1, seed=3, off=0, rule=x, ro=x, sums=x, wsum=x):
        return (y0, u, pl, K, ps, ldp, w, ldw, cost, sense, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn, grp, G, wt,
                seed, off, rule, ro, sums, wsum)

    def call(ws=x, wsb=1 << 20, **kw):
        return L.insite_policy_sums_f64(*head(**kw), ws, wsb, nul)

    def value(q=qp, Q=3, out=x, ldo=6, fw=x, bf=x, ws=x, wsb=1 << 20, **kw):
        return L.insite_policy_value_f64(*head(**kw), q, Q, out, ldo, fw, bf, ws, wsb, nul)

    def fin(sums=x, wsum=x, Rn=9, G=2, K=3, sense=1, q=qp, Q=3, out=x, ldo=6, fw=x, bf=x):
        return L.insite_policy_finalize_f64(sums, wsum, Rn, G, K, sense, q, Q, out, ldo, fw, bf, nul)

    for f in (call, value):
        # insite_regimen_choice_f64's list
        assert f(y0=nul) == -1 and f(u=nul) == -1 and f(coef=nul) == -1 and f(e=nul) == -1
        assert f(N=-1) == -1 and f(T=0) == -1 and f(T=-3) == -1 and f(U=-1) == -1 and f(U=4) == -1
        assert f(A=0) == -1 and f(A=_lib.MAX_ARMS + 1) == -1 and f(F=0) == -1 and f(F=_lib.MAX_TERMS + 1) == -1
        assert f(sub=0) == -1 and f(dt=-0.1) == -1 and f(dt=float("nan")) == -1
        assert f(m=2) == -2 and f(m=-1) == -2
        assert f(Rn=1) == -1 and f(Rn=0) == -1 and f(Rn=-4) == -1
        e2 = exps.copy()
        e2[1, 0] = 2
        assert f(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                      # state exponent above 1
        e3 = exps.copy()
        e3[2, 1] = -1
        assert f(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
        assert f(K=0) == -1 and f(K=-1) == -1
        assert f(sense=0) == -1 and f(sense=2) == -1 and f(sense=-2) == -1
        for ld in range(1, 12):
            assert f(ldp=ld) == -1, ld                                            # 0 < ld_plan < T
            assert f(ldw=ld) == -1, ld                                            # 0 < ld_w < T
        assert f(ldp=-1) == -1 and f(ldw=-1) == -1 and f(ps=-1) == -1
        assert f(ldp=0, ps=11) == -1                                              # shared plans: plan_stride >= T
        assert f(ps=59) == -1 and f(ps=12) == -1                                  # plan_stride >= n_rows ld_plan
        assert f(ldp=13, ps=64) == -1
        assert f(pl=nul) == -1 and f(w=nul) == -1
        assert f(ps=big) == -1 and f(ldw=big) == -1 and f(ldp=big, ps=big) == -1   # the largest offset leaves int64
        # insite_cohort_effect_sums_f64's list
        assert f(G=0) == -1 and f(G=-1) == -1 and f(wt=2) == -1 and f(wt=-1) == -1 and f(off=-1) == -1
        assert f(off=(1 << 63) - 3) == -1                                         # patient_offset + n_rows
        assert f(sums=nul) == -1 and f(wsum=nul) == -1
        assert f(ws=nul) == -1 and f(wsb=0) == -1
        need = L.insite_policy_workspace_bytes(5, 12, 2, 7, 9, 2, 3)
        assert need > 0 and f(wsb=need - 1) == -1
        assert f(ws=ctypes.c_void_p(ctypes.addressof(x) + 4)) == -1               # misaligned
        # the caps: INSITE_E_UNSUPPORTED
        assert f(Rn=_lib.POLICY_MAX_REPLICATES + 1) == -2 and f(Rn=4097, N=0) == -2 and f(Rn=4096, N=0) == 0
        assert f(K=17) == -2 and f(K=_lib.POLICY_MAX_PLANS + 1, N=0) == -2 and f(K=16, N=0) == 0
        assert f(G=65) == -2 and f(G=_lib.POLICY_MAX_GROUPS + 1, N=0) == -2 and f(G=64, N=0) == 0
        # an invalid argument goes before a cap
        assert f(K=17, sense=0) == -1 and f(G=65, T=0) == -1 and f(Rn=5000, ldp=3) == -1
        # n_rows = 0: a successful no-op, whatever the pointers; still validated
        assert f(N=0) == 0
        assert f(N=0, y0=nul, u=nul, pl=nul, w=nul, cost=nul, coef=nul, grp=nul, rule=nul, ro=nul, sums=nul, wsum=nul,
                 ws=nul, wsb=0) == 0
        assert f(N=0, ldp=0, ps=12) == 0 and f(N=0, ldp=13, ps=65) == 0 and f(N=0, ldw=0) == 0 and f(N=0, ldw=40) == 0
        assert f(N=0, cost=nul) == 0 and f(N=0, sense=-1) == 0 and f(N=0, K=1) == 0 and f(N=0, wt=0) == 0
        assert f(N=0, K=2, ps=big, ldp=big, ldw=big) == 0 and f(N=0, off=(1 << 63) - 1) == 0
        assert f(N=0, K=3, ps=big) == -1                                          # 2 plan_stride leaves int64
        assert f(N=0, Rn=1) == -1 and f(N=0, T=0) == -1 and f(N=0, K=0) == -1 and f(N=0, G=0) == -1
        assert f(N=0, sense=0) == -1 and f(N=0, ldp=5) == -1 and f(N=0, ldw=5) == -1 and f(N=0, ps=11) == -1
        assert f(N=0, e=nul) == -1 and f(N=0, m=3) == -2 and f(N=0, wt=5) == -1 and f(N=0, off=-2) == -1
        # NULL rule and rule_out are valid arguments: with rows and everything else valid the call would launch, so
        # here they ride on a call that another NULL stops
        assert f(rule=nul, ro=nul, cost=nul, grp=nul, sums=nul) == -1

    # the finalize call and the finalize half of the combined call
    for f in (fin, lambda **kw: value(N=0, **kw)):
        assert f(q=nul) == -1 and f(Q=0) == -1 and f(Q=-1) == -1 and f(out=nul) == -1 and f(fw=nul) == -1
        assert f(bf=nul) == -1 and f(ldo=5) == -1 and f(ldo=0) == -1 and f(ldo=-6) == -1
        assert f(ldo=1 << 62) == -1 and f(ldo=(1 << 63) - 1) == -1                # (G S - 1) ld_out leaves int64
        assert f(q=qp17, Q=16, ldo=18) == -1
        assert f(q=qp17, Q=17, ldo=20) == -2 and f(q=qp17, Q=17, ldo=19) == -1
        for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
            qb = np.array([0.5, bad, 0.1])
            assert f(q=qb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
        assert f(Rn=1) == -1 and f(G=0) == -1 and f(K=0) == -1 and f(sense=0) == -1 and f(sense=3) == -1
        assert f(Rn=4097) == -2 and f(G=65) == -2 and f(K=17) == -2
        assert f(K=17, ldo=5) == -1 and f(Rn=4097, q=nul) == -1
    assert fin(sums=nul) == -1 and fin(wsum=nul) == -1
    assert value(N=0) == 0 and value(N=0, q=qp17, Q=16, ldo=19) == 0 and value(N=0, sums=nul, wsum=nul) == 0
    assert value(out=nul) == -1 and value(N=0, out=nul) == -1 and value(N=0, fw=nul) == -1
    assert value(N=0, bf=nul) == -1 and value(N=0, q=nul) == -1 and value(N=0, ldo=5) == -1
    assert value(N=0, q=qp17, Q=17, ldo=20) == -2 and value(N=0, q=qp17, Q=17, ldo=20, sense=0) == -1


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
    for fn in (ops.policy_value, ops.plan_policy_value):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, plans, coef, lib, 0.1, (0.1, 0.9), w)
    with pytest.raises(ValueError, match="device tensor"):
        ops.policy_sums(y0, u, plans[:, 0], coef, lib, 0.1, w[0], cost=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device tensor"):
        ops.policy_finalize(torch.zeros((5, 1, 8), dtype=torch.float64), torch.zeros((5, 1), dtype=torch.float64),
                            (0.5,))


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``policy_value`` covers the per-arm EQ_4 model over the affine library; it needs ``bootstrap()`` first, between
    2 and 4096 replicates (the cap named in the message), a valid ``resample``, 1 to 16 plans, a rule of plan indices
    and an [N, T] objective whose rows have one common sum."""
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.sindy import SINDY
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="policy_value"):
                m.policy_value(None, [0, 1])
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.policy_value(None, [0, 1])
    for Rn in (1, _lib.POLICY_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.POLICY_MAX_REPLICATES)):
            m.policy_value(None, [0, 1])
    assert _lib.POLICY_MAX_REPLICATES == _lib.COHORT_MAX_REPLICATES == 4096
    coef = torch.zeros((9, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    with pytest.raises(ValueError, match="resample"):
        m.policy_value(None, [0, 1], resample="both")
    with pytest.raises(ValueError, match="independent"):
        m.policy_value(None, [0, 1], resample="independent")
    with pytest.raises(ValueError, match="independent"):
        m.policy_value(None, [0, 1], resample="independent", seed=3)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=None)
    with pytest.raises(ValueError, match="paired"):
        m.policy_value(None, [0, 1])
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    for plans in ([], [0] * 17, 0):
        with pytest.raises(ValueError, match="1 to 16"):
            m.policy_value(None, plans)
    with pytest.raises(ValueError, match="costs"):
        m.policy_value(None, [0, 1], costs=[0.0])
    # a host stand-in of a dataset: the rule and the objective are checked before anything touches a device
    N, T = 6, 5
    ct = np.zeros((N, T, 2))
    ct[..., 0] = 1.0
    ds = types.SimpleNamespace(data={"current_treatments": ct, "active_entries": np.ones((N, T, 1))})
    for rule in (np.zeros(N - 1, dtype=np.int64), np.full(N, 2), np.full(N, -1), np.zeros(N), np.zeros((N, 1), dtype=int)):
        with pytest.raises(ValueError, match="rule"):
            m.policy_value(ds, [0, 1], rule=rule)
    w = np.ones((N, T))
    w[2] *= 1.0 + 1e-9
    with pytest.raises(ValueError, match="same sum"):
        m.policy_value(ds, [0, 1], objective=w)
    with pytest.raises(ValueError, match="objective"):
        m.policy_value(ds, [0, 1], objective="median")


def test_policy_result_scaling():
    """``effect.from_policy``: the locations of the value-like series are shifted and divided, their spread and the
    three differences divided only, the shares untouched; named access and the share block."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(5)
    K, Gn, Q = 3, 2, 2
    out = torch.tensor(rng.normal(size=(Gn, 2 * K + 6, 3 + Q)))
    fixwin, bf = torch.tensor(rng.random((Gn, K))), torch.tensor([1, -1], dtype=torch.int32)
    rule, wsum = torch.tensor([0, 2, 1], dtype=torch.int32), torch.tensor(rng.random((4, Gn)))
    res = effect.from_policy(out, fixwin, bf, rule, wsum, (0.1, 0.9), shift=2.0, scale=4.0)
    assert res.series == ("value_0", "value_1", "value_2", "personalised", "rule", "best_fixed", "gain_personalised",
                          "gain_rule", "optimism", "share_0", "share_1", "share_2")
    assert res.series == effect.policy_series(3) and res.n_plans == 3 and res.q == (0.1, 0.9)
    assert res.fixwin is fixwin and res.best_fixed is bf and res.rule is rule and res.weight_sum is wsum
    o = out.numpy().transpose(1, 2, 0)                           # [S, 3 + Q, G]
    assert res.point.shape == (12, Gn) and res.quantiles.shape == (12, Q, Gn)
    for i in range(K + 3):
        assert np.array_equal(res.point.numpy()[i], (o[i, 0] - 2.0) / 4.0)
        assert np.array_equal(res.mean.numpy()[i], (o[i, 1] - 2.0) / 4.0)
        assert np.array_equal(res.std.numpy()[i], o[i, 2] / 4.0)
        assert np.array_equal(res.quantiles.numpy()[i], (o[i, 3:] - 2.0) / 4.0)
    for i in range(K + 3, K + 6):
        assert np.array_equal(res.point.numpy()[i], o[i, 0] / 4.0)
        assert np.array_equal(res.quantiles.numpy()[i], o[i, 3:] / 4.0)
    assert np.array_equal(res.point.numpy()[K + 6:], o[K + 6:, 0]) and np.array_equal(res.std.numpy()[K + 6:], o[K + 6:, 2])
    assert np.array_equal(res["optimism"]["mean"].numpy(), o[K + 5, 1] / 4.0)
    assert np.array_equal(res["share_1"]["point"].numpy(), o[K + 7, 0])
    sh = res.share
    assert sh["point"].shape == (K, Gn) and sh["quantiles"].shape == (Q, K, Gn)
    assert np.array_equal(sh["mean"].numpy(), o[K + 6:, 1])
    with pytest.raises(ValueError):
        effect.from_policy(out[:, :7], fixwin, bf, rule, wsum, (0.1, 0.9))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def test_reference_against_brute_force():
    """The restatement against loops over (replicate, row, plan) with nothing vectorised."""
    import cohort_effect_ref as C
    import effect_ref as E
    import library_matrix as M
    import policy_ref as P
    Rn, N, T, A, K, Gn = 9, 12, 7, 2, 3, 2
    q = (0.0, 0.3, 1.0)
    y0, u, plans, w, cost, coef, group, _ = P.inputs(("policy-small", 1), Rn, N, T, A, K, Gn, "std7")
    plans, w = np.ascontiguousarray(plans[..., :T]), np.ascontiguousarray(w[..., :T])
    exps = M.exps_of("std7")
    rule = np.array([0, 1, 2, 0, 1, 2, 3, -1, 0, 1, 2, 0], dtype=np.int32)       # rows 6 and 7: outside 0..K-1
    assert ((group < 0) | (group >= Gn)).any()                                    # excluded rows
    for sense, rl in ((1, None), (-1, rule)):
        ref = P.policy(y0, u, plans, coef, exps, 0.1, q, w, cost, sense, rl, group, Gn, "poisson", 5, 40, "euler", 5)
        om = C.weights("poisson", 5, Rn, N, 40)
        ys = [E.trajectories(y0, u, plans[j], coef, exps, 0.1, "euler", 5) for j in range(K)]
        J = np.empty((Rn, N, K))
        best = np.empty((Rn, N), dtype=int)
        for r in range(Rn):
            for p in range(N):
                for j in range(K):
                    acc = float(cost[j])
                    for k in range(T):
                        acc = acc + w[p, k] * ys[j][r, p, k]
                    J[r, p, j] = acc
                b = 0
                for j in range(1, K):
                    if sense * J[r, p, j] < sense * J[r, p, b]:
                        b = j
                best[r, p] = b
        use = best[0] if rl is None else rl
        assert np.array_equal(ref["rule"], use)
        ser = np.full((Rn, Gn, 2 * K + 6), np.nan)
        jfix = np.empty((Rn, Gn), dtype=int)
        for r in range(Rn):
            for g in range(Gn):
                S = [0.0] * (2 * K + 2)
                ws = 0
                for p in range(N):
                    if group[p] != g or om[r, p] == 0:
                        continue
                    ws += int(om[r, p])
                    for j in range(K):
                        S[j] += om[r, p] * J[r, p, j]
                    S[K] += om[r, p] * J[r, p, best[r, p]]
                    S[K + 1] += om[r, p] * (J[r, p, use[p]] if 0 <= use[p] < K else np.nan)
                    S[K + 2 + best[r, p]] += om[r, p]
                assert ref["wsum"][r, g] == ws
                assert np.allclose(ref["sums"][r, g], S, rtol=1e-13, atol=0, equal_nan=True)
                assert np.array_equal(ref["sums"][r, g, K + 2:], S[K + 2:]) and sum(S[K + 2:]) == ws
                if ws == 0:
                    jfix[r, g] = -1
                    continue
                val = [S[j] / ws for j in range(K)]
                b = 0
                for j in range(1, K):
                    if sense * val[j] < sense * val[b]:
                        b = j
                jfix[r, g] = b
                pers, rul = S[K] / ws, S[K + 1] / ws
                ser[r, g] = val + [pers, rul, val[b], sense * (val[b] - pers), sense * (val[b] - rul),
                                   sense * (rul - pers)] + [S[K + 2 + j] / ws for j in range(K)]
                assert sense * pers <= sense * val[b] + 1e-12
                assert rul != rul or sense * pers <= sense * rul + 1e-12
        assert np.array_equal(ref["best_fixed"], jfix[0])
        for g in range(Gn):
            votes = [int((jfix[1:, g] == j).sum()) for j in range(K)]
            assert np.array_equal(ref["fixwin"][g], np.array(votes) / (Rn - 1.0))
            for sv in range(2 * K + 6):
                v = ser[:, g, sv]
                got = ref["out"][g, sv]
                assert got[0] == v[0] or (np.isnan(got[0]) and np.isnan(v[0])) or abs(got[0] - v[0]) <= 1e-13
                rep = sorted(v[1:])
                if np.isnan(v[1:]).any():
                    assert np.isnan(got[1:]).all()
                    continue
                assert abs(got[1] - sum(rep) / len(rep)) <= 1e-13
                assert abs(got[2] - np.std(v[1:], ddof=1)) <= 1e-13
                assert abs(got[3] - rep[0]) <= 1e-13 and abs(got[5] - rep[-1]) <= 1e-13
                pos = 0.3 * (len(rep) - 1)
                i = int(np.floor(pos))
                assert abs(got[4] - (rep[i] + (pos - i) * (rep[i + 1] - rep[i]))) <= 1e-13
        if rl is not None:
            # a row with a rule outside 0..K-1 makes the rule column NaN exactly where it has weight > 0
            for r in range(Rn):
                for g in range(Gn):
                    hit = any(group[p] == g and om[r, p] > 0 and not 0 <= rl[p] < K for p in range(N))
                    assert np.isnan(ref["sums"][r, g, K + 1]) == hit


def test_reference_rules():
    """K = 1: the personalised, rule and value columns agree and the differences are +0; identical plans put every
    vote on plan 0; a constant rule reproduces its column; a NaN replicate poisons what the header says."""
    import library_matrix as M
    import policy_ref as P
    Rn, N, T, A, K, Gn = 9, 10, 6, 2, 3, 2
    q = (0.0, 0.5, 1.0)
    exps = M.exps_of("std7")
    y0, u, plans, w, cost, coef, group, _ = P.inputs(("policy-small", 2), Rn, N, T, A, K, Gn, "std7")
    plans, w = np.ascontiguousarray(plans[..., :T]), np.ascontiguousarray(w[..., :T])
    args = (coef, exps, 0.1, q, w)
    base = P.policy(y0, u, plans, *args, cost, 1, None, group, Gn, "none")
    S = base["sums"]
    assert (S[:, :, K] <= S[:, :, :K].min(axis=2) + 1e-12).all() and (S[:, :, K] <= S[:, :, K + 1] + 1e-12).all()
    assert np.array_equal(S[:, :, K + 2:].sum(axis=2), base["wsum"])
    one = P.policy(y0, u, plans[:1], *args, cost[:1], -1, None, group, Gn, "none")
    assert np.array_equal(one["sums"][:, :, 0], one["sums"][:, :, 1]) and np.array_equal(one["sums"][:, :, 0], one["sums"][:, :, 2])
    diff = np.delete(one["out"][:, 4:7], 2, axis=-1)
    assert (diff == 0.0).all() and not np.signbit(diff).any() and (one["fixwin"] == 1.0).all()
    same = P.policy(y0, u, np.repeat(plans[:1], K, axis=0), *args, None, 1, None, group, Gn, "none")
    assert (same["sums"][:, :, K + 3:] == 0).all() and np.array_equal(same["sums"][:, :, K + 2], same["wsum"])
    assert (same["rule"] == 0).all() and (same["best_fixed"] == 0).all() and (same["fixwin"][:, 0] == 1.0).all()
    for j in range(K):
        cj = P.policy(y0, u, plans, *args, cost, 1, np.full(N, j, dtype=np.int32), group, Gn, "none")
        assert np.array_equal(cj["sums"][:, :, K + 1], cj["sums"][:, :, j])
    cn = coef.copy()
    cn[4] = np.nan
    ab = P.policy(y0, u, plans, cn, exps, 0.1, q, w, cost, 1, None, group, Gn, "none")
    assert np.isnan(ab["sums"][4, :, :K + 2]).all() and (ab["sums"][4, :, K + 2:] == 0).all()
    assert np.isnan(ab["out"][:, :K + 6, 1:]).all() and np.isfinite(ab["out"][:, K + 6:]).all()
    assert np.array_equal(ab["out"][..., 0], base["out"][..., 0]) and (ab["jfix"][4] == -1).all()
    assert np.allclose(ab["fixwin"].sum(axis=1), (Rn - 2) / (Rn - 1.0), rtol=0, atol=1e-15)


def test_parity_case_inputs_are_unambiguous():
    """The input conditions of the GPU parity cases.  Every row-level argmin margin and every margin between the
    fixed plans' cohort values is at least 1e-8 of its scale, a hundred times the GPU bar of 1e-10: ``rule``, the
    allocation counts, ``fixwin`` and ``best_fixed`` are compared exactly there.  Every case with K >= 2 and R >= 17
    spreads the allocation over at least two plans and has at least two distinct best fixed plans across the
    replicates: neither argmin comparison is vacuous."""
    import policy_ref as P
    for c, cid in zip(P.CASES, P.CASE_IDS):
        ref = P.case(*c)[-1]
        Rn, K = c[0], c[4]
        alloc = ref["sums"][:, :, K + 2:].sum(axis=(0, 1))
        jf = np.unique(ref["jfix"][ref["jfix"] >= 0])
        print(f"{cid}: row margin {ref['row_margin']:.3e}, fixed-plan margin {ref['fixed_margin']:.3e}, "
              f"{int((alloc > 0).sum())} plans allocated, {jf.size} distinct best fixed plans")
        assert ref["row_margin"] >= 1e-8, cid
        assert ref["fixed_margin"] >= 1e-8, cid
        assert (ref["wsum"] > 0).all(), cid
        assert not np.isnan(ref["out"]).any() or Rn == 2, cid
        if K >= 2 and Rn >= 17:
            assert (alloc > 0).sum() >= 2, cid
            assert jf.size >= 2, cid
