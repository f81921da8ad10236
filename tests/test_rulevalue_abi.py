"""CPU tests of the rule-value extension ABI (include/insite_rulevalue.h): header, bindings and exported symbols agree,
the nine older headers did not move, the names stay clear of the pins of tests/test_feedback_abi.py and
tests/test_workspace_matrix.py, every argument check and cap answers before any HIP call, the workspace query, the
plugin refuses what it does not cover, the numpy restatement tests/rule_value_ref.py (the reference of
tests/test_gpu_rulevalue.py) agrees with a brute-force scalar triple loop, and the inputs of the GPU parity cases leave
no comparison ambiguous -- neither a decision, nor a row's argmin inside a replicate, nor a group's best fixed rule."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_rulevalue.h")
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


def _prototype(src, name):
    return re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)


def test_header_and_bindings_agree(L):
    from insite_amd import _lib
    fns = _functions(HEADER)
    assert fns == sorted(_lib.RULEVALUE_SYMBOLS) and len(fns) == 5
    older = (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
             | set(_lib.EFFECT_EXPORTS) | set(_lib.COHORT_EXPORTS) | set(_lib.REGIMEN_EXPORTS)
             | set(_lib.POLICY_EXPORTS) | set(_lib.FEEDBACK_SYMBOLS))
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_RULEVALUE_ABI_VERSION") == _lib.RULEVALUE_ABI_VERSION == 1
    assert const("INSITE_RULEVALUE_MAX_REPLICATES") == _lib.RULEVALUE_MAX_REPLICATES == 4096
    assert const("INSITE_RULEVALUE_MAX_RULES") == _lib.RULEVALUE_MAX_RULES == 16
    assert const("INSITE_RULEVALUE_MAX_GROUPS") == _lib.RULEVALUE_MAX_GROUPS == 64
    assert const("INSITE_RULEVALUE_MAX_QUANTILES") == _lib.RULEVALUE_MAX_QUANTILES == 16
    assert L.insite_rulevalue_abi_version() == 1
    assert ("insite_rulevalue_abi_version", 1, "rulevalue ") in _lib._ABI_VERSIONS
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in fns:
        if name == "insite_rulevalue_abi_version":
            continue
        assert len(_prototype(src, name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    for header, n in (("insite_hip.h", 43), ("insite_irregular.h", 4), ("insite_weak.h", 5), ("insite_bootstrap.h", 4),
                      ("insite_effect.h", 3), ("insite_cohort.h", 5), ("insite_regimen.h", 3), ("insite_policy.h", 5),
                      ("insite_feedback.h", 2)):
        assert len(_functions(os.path.join(inc, header))) == n, header
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1 and L.insite_effect_abi_version() == 1
    assert L.insite_cohort_abi_version() == 1 and L.insite_regimen_abi_version() == 1
    assert L.insite_policy_abi_version() == 1 and L.insite_feedback_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5
    assert len(_lib.BOOT_EXPORTS) == 4 and len(_lib.EFFECT_EXPORTS) == 3 and len(_lib.COHORT_EXPORTS) == 5
    assert len(_lib.REGIMEN_EXPORTS) == 3 and len(_lib.POLICY_EXPORTS) == 5 and len(_lib.FEEDBACK_SYMBOLS) == 2


def test_names_stay_clear_of_the_pins(L):
    """tests/test_feedback_abi.py pins the symbols that start with insite_feedback_, tests/test_workspace_matrix.py the
    ``_lib`` names that end in EXPORTS and every signature that ends in (void* workspace, size_t, void* stream)."""
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.RULEVALUE_SYMBOLS:
        assert name in syms, name
        assert not name.startswith("insite_feedback_") and not name.startswith("insite_policy_")
    assert {s for s in syms if s.startswith("insite_rulevalue_")} == set(_lib.RULEVALUE_SYMBOLS)
    assert {s for s in syms if s.startswith("insite_feedback_")} == set(_lib.FEEDBACK_SYMBOLS)
    assert {s for s in syms if s.startswith("insite_policy_")} == set(_lib.POLICY_EXPORTS)
    for attr in dir(_lib):
        if "RULEVALUE" in attr:
            assert not attr.endswith("EXPORTS"), attr
    src = open(HEADER).read()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name in _lib.RULEVALUE_SYMBOLS:
        args = _lib._SIGNATURES[name][1]
        assert tuple(args[-3:]) != (vp, sz, vp), name
        if name == "insite_rulevalue_abi_version":
            continue
        words = [a.split()[-1].lstrip("*") for a in _prototype(src, name).split(",")]
        assert words[-3:-1] != ["workspace", "workspace_bytes"], name
    # the two calls that need scratch take it before their outputs
    for name in ("insite_rulevalue_sums_f64", "insite_rulevalue_f64"):
        words = [a.split()[-1].lstrip("*") for a in _prototype(src, name).split(",")]
        i = words.index("workspace")
        assert words[i - 2:i + 4] == ["assign", "assign_out", "workspace", "workspace_bytes", "sums", "wsum"], name
        assert words[-1] == "stream"
        assert _lib._SIGNATURES[name][1][i] is vp and _lib._SIGNATURES[name][1][i + 1] is sz


def test_workspace_query(L):
    """The assignment (4 bytes per row, rounded up to 8) plus the chunks' partials: G x ceil(R / 64) x 64 x (3 K + 5)
    doubles per chunk, one chunk per 64 rows until 8192 waves are out (insite_policy.h's chunks); 0 for invalid,
    unsupported or overflowing shapes."""
    ws = L.insite_rulevalue_workspace_bytes
    assert ws(1000, 60, 2, 7, 256, 8, 8) == 4000 + 16 * (8 * 4 * 29 * 64 * 8)
    assert ws(1, 1, 1, 1, 2, 1, 1) == 8 + 1 * 1 * 8 * 64 * 8
    assert ws(3, 60, 2, 7, 65, 3, 16) == 16 + 3 * 2 * 53 * 64 * 8
    # where no bound binds the chunk count is insite_policy_workspace_bytes': the same rows per block
    for N, R, G, K in ((1000, 256, 8, 8), (700, 17, 3, 8), (130, 65, 64, 2), (40, 2, 1, 3), (10 ** 6, 256, 1, 2)):
        a, p = ws(N, 60, 2, 7, R, G, K), L.insite_policy_workspace_bytes(N, 60, 2, 7, R, G, K)
        head = (4 * N + 7) // 8 * 8
        assert (a - head) % (3 * K + 5) == 0 and (p - head) % (2 * K + 3) == 0
        assert (a - head) // (3 * K + 5) == (p - head) // (2 * K + 3), (N, R, G, K)
    # many rows: the chunk count stops at 8192 / (n_rt G) and the partials stay below 1 GiB
    big = ws(10 ** 7, 60, 2, 7, 4096, 64, 16)
    assert big == 4 * 10 ** 7 + 2 * (64 * 64 * 53 * 64 * 8) and big - 4 * 10 ** 7 < 1 << 30
    assert ws(0, 60, 2, 7, 256, 8, 8) == 0 and ws(-1, 60, 2, 7, 256, 8, 8) == 0 and ws(10, 0, 2, 7, 256, 8, 8) == 0
    assert ws(10, 60, 0, 7, 256, 8, 8) == 0 and ws(10, 60, 5, 7, 256, 8, 8) == 0 and ws(10, 60, 2, 0, 256, 8, 8) == 0
    assert ws(10, 60, 2, 10, 256, 8, 8) == 0 and ws(10, 60, 2, 7, 1, 8, 8) == 0 and ws(10, 60, 2, 7, 4097, 8, 8) == 0
    assert ws(10, 60, 2, 7, 256, 0, 8) == 0 and ws(10, 60, 2, 7, 256, 65, 8) == 0 and ws(10, 60, 2, 7, 256, 8, 0) == 0
    assert ws(10, 60, 2, 7, 256, 8, 17) == 0
    assert ws(1 << 62, 60, 2, 7, 256, 8, 8) == 0 and ws((1 << 63) - 1, 60, 2, 7, 2, 1, 1) == 0      # 4 N leaves int64
    assert ws((1 << 61) - 64, 60, 2, 7, 4096, 64, 16) == 0                     # 4 N fits, 4 N + the partials do not
    assert ws(10, 60, 2, 7, 4096, 64, 16) > 0


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_rulevalue.h happens before any HIP call (this host has no GPU)."""
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
    rl3 = np.array([[1, 0, 1, 0], [0, 1, 2, 1], [1, 1, 5, 0]], dtype=np.int32)
    rl17 = np.ascontiguousarray(np.tile(rl3[:1], (17, 1)))
    ac = np.array([0.01, -0.02])

    def rp(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    # N = 5, T = 12, K = 3, Q = 3: ld_theta 6, ld_w 12, ld_out 6
    def head(y0=x, u=x, th=x, ldt=6, rl=rl3, K=3, w=x, ldw=12, cost=x, armc=ac, sense=1, coef=x, e=ep, F=7, N=5, T=12,
             U=2, A=2, dt=0.1, m=0, sub=5, drop=1e-3, Rn=9, grp=x, G=2, wt=1, seed=3, off=0, asg=x, ao=x, ws=x,
             wsb=1 << 20, sums=x, wsum=x):
        return (y0, u, th, ldt, nul if rl is None else rp(rl), K, w, ldw, cost, nul if armc is None else rp(armc),
                sense, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn, grp, G, wt, seed, off, asg, ao, ws, wsb, sums,
                wsum)

    def call(**kw):
        return L.insite_rulevalue_sums_f64(*head(**kw), nul)

    def value(q=qp, Q=3, out=x, ldo=6, fw=x, bf=x, **kw):
        return L.insite_rulevalue_f64(*head(**kw), q, Q, out, ldo, fw, bf, nul)

    def fin(sums=x, wsum=x, Rn=9, G=2, K=3, sense=1, q=qp, Q=3, out=x, ldo=6, fw=x, bf=x):
        return L.insite_rulevalue_finalize_f64(sums, wsum, Rn, G, K, sense, q, Q, out, ldo, fw, bf, nul)

    for f in (call, value):
        # insite_feedback_rules_f64's list
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
        assert f(K=0) == -1 and f(K=-1) == -1 and f(rl=None) == -1 and f(rl=None, N=0) == -1
        assert f(sense=0) == -1 and f(sense=2) == -1 and f(sense=-2) == -1
        # every field of the first and of the last rule, at and past its bounds
        for j in (0, 2):
            for col, good, bad in ((0, (0, 1), (-1, 2, 127, 256)), (1, (0, 1), (-1, 2, 1 << 20)),
                                   (2, (1, 2 ** 31 - 1), (0, -1, -2 ** 31)), (3, (0, 1), (-1, 2, 256))):
                for v in good:
                    r2 = rl3.copy()
                    r2[j, col] = v
                    assert f(rl=r2, N=0) == 0, (j, col, v)
                for v in bad:
                    r2 = rl3.copy()
                    r2[j, col] = v
                    assert f(rl=r2) == -1 and f(rl=r2, N=0) == -1, (j, col, v)
        r2 = rl3.copy()
        r2[1, 0] = 1
        assert f(rl=r2, A=1) == -1                                                # arms lie in 0..n_arms-1
        for ld in range(1, 6):
            assert f(ldt=ld) == -1, ld                                            # 0 < ld_theta < 2 K
        for ld in range(1, 12):
            assert f(ldw=ld) == -1, ld                                            # 0 < ld_w < T
        assert f(ldt=-1) == -1 and f(ldw=-1) == -1
        assert f(th=nul) == -1 and f(w=nul) == -1
        assert f(ldt=big) == -1 and f(ldw=big) == -1                              # the largest offset leaves int64
        # insite_cohort_effect_sums_f64's list
        assert f(G=0) == -1 and f(G=-1) == -1 and f(wt=2) == -1 and f(wt=-1) == -1 and f(off=-1) == -1
        assert f(off=(1 << 63) - 3) == -1                                         # patient_offset + n_rows
        assert f(sums=nul) == -1 and f(wsum=nul) == -1
        assert f(ws=nul) == -1 and f(wsb=0) == -1
        need = L.insite_rulevalue_workspace_bytes(5, 12, 2, 7, 9, 2, 3)
        assert need > 0 and f(wsb=need - 1) == -1
        assert f(ws=ctypes.c_void_p(ctypes.addressof(x) + 4)) == -1               # misaligned
        # the caps: INSITE_E_UNSUPPORTED
        assert f(Rn=_lib.RULEVALUE_MAX_REPLICATES + 1) == -2 and f(Rn=4097, N=0) == -2 and f(Rn=4096, N=0) == 0
        assert f(K=17, rl=rl17, ldt=34) == -2 and f(K=17, rl=rl17, ldt=34, N=0) == -2
        assert f(K=16, rl=rl17, ldt=32, N=0) == 0
        assert f(G=65) == -2 and f(G=_lib.RULEVALUE_MAX_GROUPS + 1, N=0) == -2 and f(G=64, N=0) == 0
        # an invalid argument goes before a cap
        assert f(K=17, rl=rl17, ldt=34, sense=0) == -1 and f(G=65, T=0) == -1 and f(Rn=5000, ldw=3) == -1
        # n_rows = 0: a successful no-op, whatever the pointers; still validated
        assert f(N=0) == 0
        assert f(N=0, y0=nul, u=nul, th=nul, w=nul, cost=nul, armc=None, coef=nul, grp=nul, asg=nul, ao=nul, sums=nul,
                 wsum=nul, ws=nul, wsb=0) == 0
        assert f(N=0, ldt=0) == 0 and f(N=0, ldt=9) == 0 and f(N=0, ldw=0) == 0 and f(N=0, ldw=40) == 0
        assert f(N=0, cost=nul) == 0 and f(N=0, sense=-1) == 0 and f(N=0, K=1) == 0 and f(N=0, wt=0) == 0
        assert f(N=0, ldt=big, ldw=big) == 0 and f(N=0, off=(1 << 63) - 1) == 0
        assert f(N=0, Rn=1) == -1 and f(N=0, T=0) == -1 and f(N=0, K=0) == -1 and f(N=0, G=0) == -1
        assert f(N=0, sense=0) == -1 and f(N=0, ldt=5) == -1 and f(N=0, ldw=5) == -1
        assert f(N=0, e=nul) == -1 and f(N=0, m=3) == -2 and f(N=0, wt=5) == -1 and f(N=0, off=-2) == -1
        # NULL assign, assign_out, cost, arm_cost and group are valid arguments: with rows and everything else valid
        # the call would launch, so here they ride on a call that another NULL stops
        assert f(asg=nul, ao=nul, cost=nul, armc=None, grp=nul, sums=nul) == -1

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
        assert f(Rn=4097) == -2 and f(G=65) == -2
        assert f(Rn=4097, q=nul) == -1
    assert fin(K=17) == -2 and fin(K=17, ldo=5) == -1
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
    theta = torch.zeros((3, 2), dtype=torch.float64)
    rules = [(1, 0, 1, 0)] * 3
    w = torch.zeros((4, 6), dtype=torch.float64)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    for fn in (ops.rule_value, ops.plan_rule_value):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, theta, rules, coef, lib, 0.1, (0.1, 0.9), w)
    with pytest.raises(ValueError, match="device tensor"):
        ops.rule_value_sums(y0, u, theta, rules, coef, lib, 0.1, w[0], cost=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="device tensor"):
        ops.rule_value_finalize(torch.zeros((5, 1, 13), dtype=torch.float64), torch.zeros((5, 1), dtype=torch.float64),
                                (0.5,))
    for rl in ([], [(1, 0, 1, 0)] * 17):
        with pytest.raises(ValueError, match="between 1 and 16 rules"):
            ops.rule_value(y0, u, theta, rl, coef, lib, 0.1, (0.5,), w)


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``rule_value`` covers the per-arm EQ_4 model over the affine library; it needs ``bootstrap()`` first, between 2
    and 4096 replicates (the cap named in the message), a valid ``resample``, 1 to 16 ``effect.ThresholdRule``, an
    assignment of rule indices and an [N, T] objective whose rows have one common sum."""
    import torch
    from insite_amd import _lib, bootstrap, config as C, effect
    from insite_amd.sindy import SINDY
    TR = effect.ThresholdRule
    two = [TR(0.5), TR(0.2, 0.1)]
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="rule_value"):
                m.rule_value(None, two)
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.rule_value(None, two)
    for Rn in (1, _lib.RULEVALUE_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.RULEVALUE_MAX_REPLICATES)):
            m.rule_value(None, two)
    assert _lib.RULEVALUE_MAX_REPLICATES == _lib.COHORT_MAX_REPLICATES == 4096
    # 513 replicates: beyond evaluate_rules, inside rule_value (the refusal that follows is the resample's)
    coef = torch.zeros((513, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((513, 2, 7), dtype=torch.int8), seed=3)
    with pytest.raises(ValueError, match="512"):
        m.evaluate_rules(None, two)
    with pytest.raises(ValueError, match="resample"):
        m.rule_value(None, two, resample="both")
    coef = torch.zeros((9, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    with pytest.raises(ValueError, match="independent"):
        m.rule_value(None, two, resample="independent")
    with pytest.raises(ValueError, match="independent"):
        m.rule_value(None, two, resample="independent", seed=3)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=None)
    with pytest.raises(ValueError, match="paired"):
        m.rule_value(None, two)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    for rules in ([], [TR(0.5)] * 17, TR(0.5), [(1, 0, 1, 0)]):
        with pytest.raises(ValueError, match="1 to 16"):
            m.rule_value(None, rules)
    # a host stand-in of a dataset: rules, costs, assignment and objective are checked before anything touches a device
    N, T = 6, 5
    ct = np.zeros((N, T, 2))
    ct[..., 0] = 1.0
    ds = types.SimpleNamespace(data={"current_treatments": ct, "active_entries": np.ones((N, T, 1))})
    with pytest.raises(ValueError, match="costs"):
        m.rule_value(ds, two, costs=[0.0])
    with pytest.raises(ValueError, match="arm_costs"):
        m.rule_value(ds, two, arm_costs=[0.0])
    for bad in (TR(0.5, arm_on=2), TR(0.5, arm_off=-1), TR(0.5, every=0), TR(np.zeros(N - 1))):
        with pytest.raises(ValueError, match=r"rules\[1\]"):
            m.rule_value(ds, [TR(0.5), bad])
    for asg in (np.zeros(N - 1, dtype=np.int64), np.full(N, 2), np.full(N, -1), np.zeros(N), np.zeros((N, 1), dtype=int)):
        with pytest.raises(ValueError, match="assignment"):
            m.rule_value(ds, two, assignment=asg)
    w = np.ones((N, T))
    w[2] *= 1.0 + 1e-9
    with pytest.raises(ValueError, match="same sum"):
        m.rule_value(ds, two, objective=w)
    with pytest.raises(ValueError, match="objective"):
        m.rule_value(ds, two, objective="median")


def test_rule_value_result_scaling():
    """``effect.from_rule_value``: the locations of the value-like series are shifted and divided, their spread and the
    three differences divided only, the shares and the exposures untouched; named access and the two blocks."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(5)
    K, Gn, Q = 3, 2, 2
    out = torch.tensor(rng.normal(size=(Gn, 3 * K + 9, 3 + Q)))
    fixwin, bf = torch.tensor(rng.random((Gn, K))), torch.tensor([1, -1], dtype=torch.int32)
    asg, wsum = torch.tensor([0, 2, 1], dtype=torch.int32), torch.tensor(rng.random((4, Gn)))
    res = effect.from_rule_value(out, fixwin, bf, asg, wsum, (0.1, 0.9), shift=2.0, scale=4.0)
    assert res.series == ("value_0", "value_1", "value_2", "personalised", "assigned", "best_fixed",
                          "gain_personalised", "gain_assigned", "optimism", "share_0", "share_1", "share_2",
                          "exposure_0", "exposure_1", "exposure_2", "exposure_personalised", "exposure_assigned",
                          "exposure_best_fixed")
    assert res.series == effect.rule_value_series(3) and res.n_rules == 3 and res.q == (0.1, 0.9)
    assert res.fixwin is fixwin and res.best_fixed is bf and res.assign is asg and res.weight_sum is wsum
    o = out.numpy().transpose(1, 2, 0)                           # [S, 3 + Q, G]
    assert res.point.shape == (18, Gn) and res.quantiles.shape == (18, Q, Gn)
    for i in range(K + 3):
        assert np.array_equal(res.point.numpy()[i], (o[i, 0] - 2.0) / 4.0)
        assert np.array_equal(res.mean.numpy()[i], (o[i, 1] - 2.0) / 4.0)
        assert np.array_equal(res.std.numpy()[i], o[i, 2] / 4.0)
        assert np.array_equal(res.quantiles.numpy()[i], (o[i, 3:] - 2.0) / 4.0)
    for i in range(K + 3, K + 6):
        assert np.array_equal(res.point.numpy()[i], o[i, 0] / 4.0)
        assert np.array_equal(res.quantiles.numpy()[i], o[i, 3:] / 4.0)
    assert np.array_equal(res.point.numpy()[K + 6:], o[K + 6:, 0]) and np.array_equal(res.std.numpy()[K + 6:], o[K + 6:, 2])
    assert np.array_equal(res.quantiles.numpy()[K + 6:], o[K + 6:, 3:])
    assert np.array_equal(res["optimism"]["mean"].numpy(), o[K + 5, 1] / 4.0)
    assert np.array_equal(res["share_1"]["point"].numpy(), o[K + 7, 0])
    assert np.array_equal(res["exposure_best_fixed"]["mean"].numpy(), o[3 * K + 8, 1])
    sh, ex = res.share, res.exposure
    assert sh["point"].shape == (K, Gn) and sh["quantiles"].shape == (Q, K, Gn)
    assert np.array_equal(sh["mean"].numpy(), o[K + 6:2 * K + 6, 1])
    assert ex["point"].shape == (K + 3, Gn) and ex["quantiles"].shape == (Q, K + 3, Gn)
    assert np.array_equal(ex["mean"].numpy(), o[2 * K + 6:, 1]) and np.array_equal(ex["std"].numpy(), o[2 * K + 6:, 2])
    with pytest.raises(ValueError):
        effect.from_rule_value(out[:, :16], fixwin, bf, asg, wsum, (0.1, 0.9))


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def _scalar_loop(y0, u, theta, rule, coef_r, exps, dt, w, cost, arm_cost, method, sub):
    """One (replicate, row, rule) with nothing vectorised: (J, E)."""
    from oracle import insite_ref as R
    a_on, a_off, period, start = (int(v) for v in rule)
    y, on, acc, cnt = float(y0), bool(start), float(cost), 0
    for k in range(len(w)):
        if k % period == 0:
            on = y >= (theta[1] if on else theta[0])
        arm = a_on if on else a_off
        y = float(R.rollout(np.array([y]), u[None], np.array([[arm]], dtype=np.int8), coef_r, exps, dt, method=method,
                            substeps=sub)[0, 0])
        acc = acc + w[k] * y
        if arm_cost is not None:
            acc = acc + arm_cost[arm]
        cnt += on
    return acc, float(cnt)


def test_reference_against_brute_force():
    """The restatement against loops over (replicate, row, rule) with nothing vectorised."""
    import cohort_effect_ref as C
    import feedback_ref as F
    import library_matrix as M
    import rule_value_ref as V
    Rn, N, T, A, K, Gn = 7, 10, 6, 2, 3, 2
    q = (0.0, 0.3, 1.0)
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = V.inputs(("rulevalue-small", 1), Rn, N, T, A, K, Gn, "std7")
    theta, w = F.full_theta(theta, N, K), np.ascontiguousarray(w[..., :T])
    exps = M.exps_of("std7")
    asg_in = np.array([0, 1, 2, 0, 1, 2, 3, -1, 0, 1], dtype=np.int32)           # rows 6 and 7: outside 0..K-1
    assert ((group < 0) | (group >= Gn)).any()                                    # excluded rows
    for sense, al, ac in ((1, None, arm_cost), (-1, asg_in, None)):
        ref = V.rule_value(y0, u, theta, rules, coef, exps, 0.1, q, w, cost, ac, sense, al, group, Gn, "poisson", 5,
                           40, "euler", 5)
        om = C.weights("poisson", 5, Rn, N, 40)
        J = np.empty((Rn, N, K))
        Ex = np.empty((Rn, N, K))
        best = np.empty((Rn, N), dtype=int)
        for r in range(Rn):
            for p in range(N):
                for j in range(K):
                    J[r, p, j], Ex[r, p, j] = _scalar_loop(y0[p], u[p], theta[p, 2 * j:2 * j + 2], rules[j], coef[r],
                                                           exps, 0.1, w[p], cost[j], ac, "euler", 5)
                b = 0
                for j in range(1, K):
                    if sense * J[r, p, j] < sense * J[r, p, b]:
                        b = j
                best[r, p] = b
        assert np.allclose(ref["J"], J, rtol=1e-13, atol=0) and np.array_equal(ref["E"], Ex)
        use = best[0] if al is None else al
        assert np.array_equal(ref["assign"], use)
        S_ = 3 * K + 9
        ser = np.full((Rn, Gn, S_), np.nan)
        jfix = np.empty((Rn, Gn), dtype=int)
        for r in range(Rn):
            for g in range(Gn):
                S = [0.0] * (3 * K + 4)
                ws = 0
                for p in range(N):
                    if group[p] != g or om[r, p] == 0:
                        continue
                    o = int(om[r, p])
                    ws += o
                    ok = 0 <= use[p] < K
                    for j in range(K):
                        S[j] += o * J[r, p, j]
                        S[2 * K + 2 + j] += o * Ex[r, p, j]
                    S[K] += o * J[r, p, best[r, p]]
                    S[K + 1] += o * (J[r, p, use[p]] if ok else np.nan)
                    S[K + 2 + best[r, p]] += o
                    S[3 * K + 2] += o * Ex[r, p, best[r, p]]
                    S[3 * K + 3] += o * (Ex[r, p, use[p]] if ok else np.nan)
                assert ref["wsum"][r, g] == ws
                assert np.allclose(ref["sums"][r, g], S, rtol=1e-13, atol=0, equal_nan=True)
                assert np.array_equal(ref["sums"][r, g, K + 2:], S[K + 2:], equal_nan=True)   # integers: exact
                assert sum(S[K + 2:2 * K + 2]) == ws
                if ws == 0:
                    jfix[r, g] = -1
                    continue
                val = [S[j] / ws for j in range(K)]
                b = 0
                for j in range(1, K):
                    if sense * val[j] < sense * val[b]:
                        b = j
                jfix[r, g] = b
                pers, asg = S[K] / ws, S[K + 1] / ws
                ser[r, g] = (val + [pers, asg, val[b], sense * (val[b] - pers), sense * (val[b] - asg),
                                    sense * (asg - pers)] + [S[K + 2 + j] / ws for j in range(2 * K + 2)]
                             + [S[2 * K + 2 + b] / ws])
                assert sense * pers <= sense * val[b] + 1e-12
                assert asg != asg or sense * pers <= sense * asg + 1e-12
        assert np.array_equal(ref["best_fixed"], jfix[0])
        for g in range(Gn):
            votes = [int((jfix[1:, g] == j).sum()) for j in range(K)]
            assert np.array_equal(ref["fixwin"][g], np.array(votes) / (Rn - 1.0))
            for sv in range(S_):
                v = ser[:, g, sv]
                got = ref["out"][g, sv]
                assert got[0] == v[0] or (np.isnan(got[0]) and np.isnan(v[0])) or abs(got[0] - v[0]) <= 1e-12
                rep = sorted(v[1:])
                if np.isnan(v[1:]).any():
                    assert np.isnan(got[1:]).all()
                    continue
                assert abs(got[1] - sum(rep) / len(rep)) <= 1e-12
                assert abs(got[2] - np.std(v[1:], ddof=1)) <= 1e-12
                assert abs(got[3] - rep[0]) <= 1e-12 and abs(got[5] - rep[-1]) <= 1e-12
                pos = 0.3 * (len(rep) - 1)
                i = int(np.floor(pos))
                assert abs(got[4] - (rep[i] + (pos - i) * (rep[i + 1] - rep[i]))) <= 1e-12
        if al is not None:
            # a row with an assignment outside 0..K-1 makes both assigned columns NaN exactly where it has weight > 0
            for r in range(Rn):
                for g in range(Gn):
                    hit = any(group[p] == g and om[r, p] > 0 and not 0 <= al[p] < K for p in range(N))
                    assert np.isnan(ref["sums"][r, g, K + 1]) == hit and np.isnan(ref["sums"][r, g, 3 * K + 3]) == hit


def test_reference_rules():
    """K = 1: the personalised, assigned and value columns agree and the differences are +0; always-on and always-off
    thresholds give exposures of T and 0; a constant assignment reproduces its columns; a NaN replicate poisons what the
    header says."""
    import feedback_ref as F
    import library_matrix as M
    import rule_value_ref as V
    Rn, N, T, A, K, Gn = 9, 10, 6, 2, 3, 2
    q = (0.0, 0.5, 1.0)
    exps = M.exps_of("std7")
    y0, u, theta, rules, w, cost, arm_cost, coef, group, _ = V.inputs(("rulevalue-small", 2), Rn, N, T, A, K, Gn, "std7")
    theta, w = F.full_theta(theta, N, K), np.ascontiguousarray(w[..., :T])
    args = (coef, exps, 0.1, q, w)
    base = V.rule_value(y0, u, theta, rules, *args, cost, arm_cost, 1, None, group, Gn, "none")
    S = base["sums"]
    assert (S[:, :, K] <= S[:, :, :K].min(axis=2) + 1e-12).all() and (S[:, :, K] <= S[:, :, K + 1] + 1e-12).all()
    assert np.array_equal(S[:, :, K + 2:2 * K + 2].sum(axis=2), base["wsum"])
    assert np.array_equal(S[:, :, 2 * K + 2:], np.round(S[:, :, 2 * K + 2:]))
    one = V.rule_value(y0, u, theta[:, :2], rules[:1], *args, cost[:1], arm_cost, -1, None, group, Gn, "none")
    for c in (1, 2):
        assert np.array_equal(one["sums"][:, :, 0], one["sums"][:, :, c])
    for c in (5, 6):
        assert np.array_equal(one["sums"][:, :, 4], one["sums"][:, :, c])
    diff = np.delete(one["out"][:, 4:7], 2, axis=-1)
    assert (diff == 0.0).all() and not np.signbit(diff).any() and (one["fixwin"] == 1.0).all()
    th = theta.copy()
    th[:, 0:2] = -np.inf
    th[:, 2:4] = np.inf
    rl = np.array(rules)
    rl[1, 3] = 0
    ends = V.rule_value(y0, u, th, rl, *args, cost, None, 1, None, group, Gn, "none")
    assert np.array_equal(ends["sums"][:, :, 2 * K + 2], T * ends["wsum"]) and (ends["sums"][:, :, 2 * K + 3] == 0).all()
    for j in range(K):
        cj = V.rule_value(y0, u, theta, rules, *args, cost, arm_cost, 1, np.full(N, j, dtype=np.int32), group, Gn,
                          "none")
        assert np.array_equal(cj["sums"][:, :, K + 1], cj["sums"][:, :, j])
        assert np.array_equal(cj["sums"][:, :, 3 * K + 3], cj["sums"][:, :, 2 * K + 2 + j])
    cn = coef.copy()
    cn[4] = np.nan
    ab = V.rule_value(y0, u, theta, rules, cn, exps, 0.1, q, w, cost, arm_cost, 1, None, group, Gn, "none")
    assert np.isnan(ab["sums"][4, :, :K + 2]).all() and (ab["sums"][4, :, K + 2:2 * K + 2] == 0).all()
    assert np.isnan(ab["sums"][4, :, 2 * K + 2:]).all()
    assert np.isnan(ab["out"][:, :K + 6, 1:]).all() and np.isfinite(ab["out"][:, K + 6:2 * K + 6]).all()
    assert np.isnan(ab["out"][:, 2 * K + 6:, 1:]).all()
    assert np.array_equal(ab["out"][..., 0], base["out"][..., 0]) and (ab["jfix"][4] == -1).all()


def test_parity_case_inputs_are_unambiguous():
    """The input conditions of the GPU parity cases: conditions, not measurements.  Every decision margin (the distance
    of a compared state from its threshold, relative to the row's largest state), every row-level argmin margin and
    every margin between the fixed rules' cohort values is at least 1e-8 of its scale, a hundred times the GPU bar of
    1e-10: ``assign``, the allocation counts, the exposure sums, ``fixwin`` and ``best_fixed`` are compared exactly
    there.  Every case with K >= 2 and R >= 17 spreads the allocation over at least two rules; in the cases with
    T >= 16 the exposure varies over the replicates in at least a third of the (row, rule) pairs, so the closed loop
    is not an open loop in disguise."""
    import rule_value_ref as V
    cover = {k: set() for k in ("R", "N", "K", "A", "G")}
    for c, cid in zip(V.CASES, V.CASE_IDS):
        ref = V.case(*c)[-1]
        Rn, N, T, A, K, Gn = c[:6]
        for k, v in zip(("R", "N", "K", "A", "G"), (Rn, N, K, A, Gn)):
            cover[k].add(v)
        alloc = ref["sums"][:, :, K + 2:2 * K + 2].sum(axis=(0, 1))
        Ex = ref["E"][1:]
        varies = int((np.nanmax(Ex, axis=0) != np.nanmin(Ex, axis=0)).sum())
        print(f"{cid}: decision margin {ref['dmargin']:.3e}, row margin {ref['row_margin']:.3e}, fixed-rule margin "
              f"{ref['fixed_margin']:.3e}, {int((alloc > 0).sum())} rules allocated, exposure varies in {varies} of "
              f"{N * K} pairs")
        assert ref["dmargin"] >= 1e-8, cid
        assert ref["row_margin"] >= 1e-8, cid
        assert ref["fixed_margin"] >= 1e-8, cid
        assert (ref["wsum"][0] > 0).all(), cid                     # every group has a row
        if K >= 2 and Rn >= 17:
            assert (alloc > 0).sum() >= 2, cid
        if T >= 16:
            assert 3 * varies >= N * K, cid
    assert cover["R"] >= {2, 3, 17, 64, 65, 130, 512, 4096} and cover["N"] >= {1, 3, 40, 130, 700}
    assert cover["K"] >= {1, 2, 3, 8, 16} and cover["A"] >= {1, 2, 4} and cover["G"] >= {1, 3, 64}
    assert {c[14] for c in V.CASES} == {1, -1} and {c[15] for c in V.CASES} == {"none", "poisson"}
    assert {c[12] for c in V.CASES} == {True, False} and {c[13] for c in V.CASES} == {True, False}
    assert {c[17] for c in V.CASES} == {"null", "given"} and {c[7] for c in V.CASES} == {"euler", "rk4"}
    assert {c[10] for c in V.CASES} == {"rows", "shared"} == {c[11] for c in V.CASES}
    assert {c[8] for c in V.CASES} == {1, 5} and {len(c[9]) for c in V.CASES} == {5, 16}
    assert any(c[2] < 16 for c in V.CASES) and any(16 < c[2] < 64 for c in V.CASES) and any(c[2] > 64 for c in V.CASES)
