"""CPU tests of the closed-loop rules extension ABI (include/insite_feedback.h): header, bindings and exported symbols
agree, the eight older lists did not move, every argument check answers before any HIP call, the plugin refuses what it
does not cover, the numpy restatement tests/feedback_ref.py (the reference of tests/test_gpu_feedback.py) agrees with a
brute-force scalar loop and obeys the header's rules, and the inputs of the GPU parity cases leave no decision and no
argmin ambiguous."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_feedback.h")
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
    assert fns == sorted(_lib.FEEDBACK_SYMBOLS) and len(fns) == 2
    older = (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
             | set(_lib.EFFECT_EXPORTS) | set(_lib.COHORT_EXPORTS) | set(_lib.REGIMEN_EXPORTS)
             | set(_lib.POLICY_EXPORTS))
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_FEEDBACK_ABI_VERSION") == _lib.FEEDBACK_ABI_VERSION == 1
    assert const("INSITE_FEEDBACK_MAX_REPLICATES") == _lib.FEEDBACK_MAX_REPLICATES == 512
    assert const("INSITE_FEEDBACK_MAX_QUANTILES") == _lib.FEEDBACK_MAX_QUANTILES == 16
    assert const("INSITE_FEEDBACK_MAX_RULES") == _lib.FEEDBACK_MAX_RULES == 16
    assert const("INSITE_FEEDBACK_MINIMIZE") == _lib.FEEDBACK_MINIMIZE == 1
    assert const("INSITE_FEEDBACK_MAXIMIZE") == _lib.FEEDBACK_MAXIMIZE == -1
    assert L.insite_feedback_abi_version() == 1
    assert ("insite_feedback_abi_version", 1, "feedback ") in _lib._ABI_VERSIONS
    # the C prototype and the ctypes signature have the same number of arguments
    proto = re.search(r"int32_t\s+insite_feedback_rules_f64\s*\(([^;]*?)\);", src, re.S).group(1)
    sig = _lib._SIGNATURES["insite_feedback_rules_f64"][1]
    assert len(proto.split(",")) == len(sig) == 32
    # no workspace: no query, and the signature does not end in (void*, size_t, void*)
    assert not [n for n in fns if n.endswith("_workspace_bytes")]
    assert sig[-1] is ctypes.c_void_p and sig[-2] is ctypes.c_int64 and "workspace" not in proto
    assert not [n for n in dir(_lib) if n.endswith("EXPORTS") and "FEEDBACK" in n]


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    counts = [("insite_hip.h", 43), ("insite_irregular.h", 4), ("insite_weak.h", 5), ("insite_bootstrap.h", 4),
              ("insite_effect.h", 3), ("insite_cohort.h", 5), ("insite_regimen.h", 3), ("insite_policy.h", 5)]
    for name, n in counts:
        assert len(_functions(os.path.join(inc, name))) == n, name
    lists = (_lib.EXPORTS, _lib.EXT_EXPORTS, _lib.WEAK_EXPORTS, _lib.BOOT_EXPORTS, _lib.EFFECT_EXPORTS,
             _lib.COHORT_EXPORTS, _lib.REGIMEN_EXPORTS, _lib.POLICY_EXPORTS)
    assert [len(x) for x in lists] == [43, 4, 5, 4, 3, 5, 3, 5]
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1 and L.insite_effect_abi_version() == 1
    assert L.insite_cohort_abi_version() == 1 and L.insite_regimen_abi_version() == 1
    assert L.insite_policy_abi_version() == 1


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.FEEDBACK_SYMBOLS:
        assert name in syms, name
    assert {s for s in syms if s.startswith("insite_feedback_")} == set(_lib.FEEDBACK_SYMBOLS)


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_feedback.h happens before any HIP call (this host has no GPU)."""
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
    rules3 = np.array([[1, 0, 1, 0], [0, 1, 5, 1], [1, 1, 2147483647, 0]], dtype=np.int32)
    rules16 = np.tile(rules3[:1], (17, 1))
    ac = np.array([0.0, 0.01, 0.0, 0.0])

    def rp(r):
        return r.ctypes.data_as(ctypes.c_void_p)

    # N = 5, T = 12, K = 3, Q = 3: ld_theta 6, ld_w 12, ld_out 3 * 3 * 6 = 54, ld_sched 36
    def call(y0=x, u=x, th=x, ldt=6, rl=rules3, K=3, w=x, ldw=12, cost=x, arm_cost=ac, sense=1, coef=x, e=ep, F=7, N=5,
             T=12, U=2, A=2, dt=0.1, m=0, sub=5, drop=1e-3, Rn=9, q=qp, Q=3, ch=x, win=x, out=x, ldo=54, sc=x, lds=36):
        return L.insite_feedback_rules_f64(y0, u, th, ldt, rp(rl) if rl is not None else nul, K, w, ldw, cost,
                                           rp(arm_cost) if arm_cost is not None else nul, sense, coef, e, F, N, T, U,
                                           A, dt, m, sub, drop, Rn, q, Q, ch, win, out, ldo, sc, lds, nul)

    # insite_regimen_choice_f64's list
    assert call(y0=nul) == -1 and call(u=nul) == -1 and call(coef=nul) == -1 and call(e=nul) == -1
    assert call(N=-1) == -1 and call(T=0) == -1 and call(T=-3) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(A=0) == -1 and call(A=_lib.MAX_ARMS + 1) == -1
    assert call(F=0) == -1 and call(F=_lib.MAX_TERMS + 1) == -1
    assert call(sub=0) == -1 and call(dt=-0.1) == -1 and call(dt=float("nan")) == -1
    assert call(m=2) == -2 and call(m=-1) == -2
    assert call(Rn=1) == -1 and call(Rn=0) == -1 and call(Rn=-4) == -1
    assert call(Rn=_lib.FEEDBACK_MAX_REPLICATES + 1) == -2 and call(Rn=513) == -2 and call(Rn=512, N=0) == 0
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                      # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call(q=nul) == -1 and call(Q=0) == -1 and call(Q=-1) == -1
    assert call(q=qp16, Q=_lib.FEEDBACK_MAX_QUANTILES + 1, ldo=3 * 3 * 20) == -1
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        qb = np.array([0.5, bad, 0.1])
        assert call(q=qb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
    assert call(sense=0) == -1 and call(sense=2) == -1 and call(sense=-2) == -1
    assert call(w=nul) == -1 and call(ch=nul) == -1 and call(win=nul) == -1 and call(out=nul) == -1
    for ld in range(1, 12):
        assert call(ldw=ld) == -1, ld                                            # 0 < ld_w < T
    assert call(ldw=-1) == -1
    # this header's additions: the rule table
    assert call(K=0) == -1 and call(K=-1) == -1 and call(rl=rules16, K=17, ldt=34, ldo=1 << 20, lds=1 << 20) == -1
    assert call(rl=None) == -1 and call(rl=None, N=0) == -1
    for col, bad in ((0, 2), (0, -1), (1, 2), (1, -1), (0, 127), (2, 0), (2, -1), (2, -2147483648), (3, 2), (3, -1)):
        r = rules3.copy()
        r[1, col] = bad
        assert call(rl=r) == -1 and call(rl=r, N=0) == -1, (col, bad)
    r = rules3.copy()
    r[2, 0] = 3
    assert call(rl=r, A=3, N=0) == -1 and call(rl=r, A=4, N=0) == 0              # the arm range is n_arms'
    # the thresholds
    for ld in range(1, 6):
        assert call(ldt=ld) == -1 and call(ldt=ld, N=0) == -1, ld                # 0 < ld_theta < 2 K
    assert call(ldt=-1) == -1 and call(ldt=-6) == -1 and call(th=nul) == -1
    # out and sched
    assert call(ldo=53) == -1 and call(ldo=0) == -1 and call(ldo=-54) == -1
    assert call(q=qp16, Q=16, ldo=3 * 3 * 19 - 1) == -1
    for ld in (35, 12, 1, 0, -1, -36):
        assert call(lds=ld) == -1 and call(lds=ld, N=0) == -1, ld                # ld_sched < K T
    # strides whose largest offset leaves int64
    big = (1 << 62)
    assert call(ldw=big) == -1 and call(ldo=big) == -1 and call(ldt=big) == -1 and call(lds=big) == -1
    assert call(ldt=(1 << 63) - 1) == -1 and call(lds=(1 << 63) - 1) == -1 and call(ldo=(1 << 63) - 1) == -1
    # n_rows = 0: a successful no-op, whatever the pointers (the accepted side of every bound above: a valid call with
    # rows would launch); still validated
    assert call(N=0) == 0
    assert call(N=0, ldt=0) == 0 and call(N=0, ldt=7) == 0 and call(N=0, ldw=0) == 0 and call(N=0, ldw=40) == 0
    assert call(N=0, ldo=54) == 0 and call(N=0, q=qp16, Q=16, ldo=3 * 3 * 19) == 0 and call(N=0, lds=36) == 0
    assert call(N=0, sc=nul, lds=0) == 0 and call(N=0, sc=nul, lds=-5) == 0      # no schedule: ld_sched is not looked at
    assert call(N=0, cost=nul) == 0 and call(N=0, arm_cost=None) == 0 and call(N=0, sense=-1) == 0
    assert call(N=0, K=1, ldt=2, ldo=18, lds=12) == 0
    assert call(N=0, rl=rules16, K=16, ldt=32, ldo=16 * 3 * 6, lds=16 * 12) == 0
    assert call(N=0, y0=nul, u=nul, th=nul, w=nul, cost=nul, coef=nul, ch=nul, win=nul, out=nul, sc=nul) == 0
    assert call(N=0, ldt=big, ldw=big, ldo=big, lds=big) == 0
    assert call(N=0, Rn=1) == -1 and call(N=0, T=0) == -1 and call(N=0, K=17) == -1 and call(N=0, K=0) == -1
    assert call(N=0, sense=0) == -1 and call(N=0, ldw=5) == -1 and call(N=0, ldo=53) == -1 and call(N=0, Rn=513) == -2
    assert call(N=0, q=nul) == -1 and call(N=0, e=nul) == -1 and call(N=0, m=3) == -2


def test_ops_refuse_host_tensors_and_bad_rules(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0 = torch.zeros(4, dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    theta = torch.zeros((3, 2), dtype=torch.float64)
    w = torch.zeros((4, 6), dtype=torch.float64)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    rules = [(1, 0, 1, 0), (0, 1, 2, 1), (1, 1, 9, 0)]
    for fn in (ops.feedback_rules, ops.plan_feedback_rules):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, theta, rules, coef, lib, 0.1, (0.1, 0.9), w)
        with pytest.raises(ValueError, match="between 1 and 16 rules"):
            fn(y0, u, theta, [], coef, lib, 0.1, (0.1, 0.9), w)
        with pytest.raises(ValueError, match="between 1 and 16 rules"):
            fn(y0, u, theta, rules * 6, coef, lib, 0.1, (0.1, 0.9), w)


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


def test_plugin_refusals():
    """``evaluate_rules`` covers what ``choose_plan`` covers: the joint, treatment-segment and degree-4 modes raise,
    naming the method; it needs ``bootstrap()`` first, at least one resample and at most the kernel's cap (named in
    the message), and between 1 and 16 ``ThresholdRule``."""
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.effect import ThresholdRule
    from insite_amd.sindy import SINDY
    rules = [ThresholdRule(0.5), ThresholdRule(0.7, 0.3)]
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in OV]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (OV + ["model.joint_model=true"], OV + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="evaluate_rules"):
                m.evaluate_rules(None, rules)
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.evaluate_rules(None, rules)
    for Rn in (1, _lib.FEEDBACK_MAX_REPLICATES + 1):
        coef = torch.zeros((Rn, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((Rn, 2, 7), dtype=torch.int8), seed=3)
        with pytest.raises(ValueError, match=str(_lib.FEEDBACK_MAX_REPLICATES)):
            m.evaluate_rules(None, rules)
    assert _lib.FEEDBACK_MAX_REPLICATES == _lib.REGIMEN_MAX_REPLICATES == 512
    coef = torch.zeros((9, 2, 7), dtype=torch.float64)
    m.bootstrap_ = bootstrap.summarize(coef, torch.ones((9, 2, 7), dtype=torch.int8), seed=3)
    with pytest.raises(ValueError, match="1 to 16"):
        m.evaluate_rules(None, [])
    with pytest.raises(ValueError, match="1 to 16"):
        m.evaluate_rules(None, rules * 9)
    with pytest.raises(ValueError, match="1 to 16"):
        m.evaluate_rules(None, [(1, 0, 1, 0)])
    with pytest.raises(ValueError, match="costs"):
        m.evaluate_rules(None, rules, costs=[0.0])
    with pytest.raises(ValueError, match="arm_costs"):
        m.evaluate_rules(None, rules, arm_costs=[0.0, 0.1, 0.2])


def test_feedback_result_scaling():
    """``effect.from_feedback``: the locations of the value series are shifted (per row) and divided, its spread and
    the regret divided only, the exposure left as it is."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(2)
    out = torch.tensor(rng.normal(size=(4, 3, 3, 5)))            # [N, K, 3, 3 + Q]
    choice = torch.tensor([0, 2, -1, 1], dtype=torch.int32)
    win = torch.tensor(rng.random((4, 3)))
    sched = torch.zeros((4, 3, 6), dtype=torch.int8)
    shift = torch.tensor(rng.normal(size=4))
    res = effect.from_feedback(choice, win, out, (0.1, 0.9), schedule=sched, shift=shift, scale=4.0)
    assert res.series == ("value", "regret", "exposure") and res.q == (0.1, 0.9)
    assert res.choice is choice and res.win is win and res.schedule is sched
    o = out.numpy().transpose(2, 3, 0, 1)                        # [3, 3 + Q, N, K]
    sh = shift.numpy()[:, None]
    assert res.point.shape == (3, 4, 3) and res.quantiles.shape == (3, 2, 4, 3)
    assert np.array_equal(res.point.numpy()[0], (o[0, 0] - sh) / 4.0)
    assert np.array_equal(res.mean.numpy()[0], (o[0, 1] - sh) / 4.0)
    assert np.array_equal(res.quantiles.numpy()[0], (o[0, 3:] - sh) / 4.0)
    assert np.array_equal(res.std.numpy()[:2], o[:2, 2] / 4.0)
    assert np.array_equal(res.point.numpy()[1], o[1, 0] / 4.0)
    assert np.array_equal(res["regret"]["quantiles"].numpy(), o[1, 3:] / 4.0)
    for f, want in (("point", o[2, 0]), ("mean", o[2, 1]), ("std", o[2, 2]), ("quantiles", o[2, 3:])):
        assert np.array_equal(res["exposure"][f].numpy(), want), f
    assert effect.from_feedback(choice, win, out, (0.1, 0.9)).schedule is None
    with pytest.raises(ValueError):
        effect.from_feedback(choice, win, out[:, :, :2], (0.1, 0.9))
    r = effect.ThresholdRule(0.5)
    assert (r.off, r.arm_on, r.arm_off, r.every, r.start_on) == (None, 1, 0, 1, False)


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def _small(seed, Rn, N, T, A, K, name="std7"):
    import feedback_ref as F
    y0, u, theta, rules, w, cost, ac, coef = F.inputs(("feedback-small", seed), Rn, N, T, A, K, name)
    return y0, u, np.ascontiguousarray(theta[:, :2 * K]), rules, np.ascontiguousarray(w[..., :T]), cost, ac, coef


def _rhs(y, u, c, exps):
    return sum(c[f] * y ** exps[f, 0] * np.prod(u ** exps[f, 1:]) for f in range(len(c)) if abs(c[f]) > 1e-3)


def test_reference_against_brute_force():
    """The restatement against scalar loops over (replicate, row, rule, step) with nothing vectorised and the Euler
    sub-steps written out."""
    import feedback_ref as F
    import library_matrix as M
    Rn, N, T, A, K = 7, 3, 9, 2, 4
    q = (0.0, 0.3, 1.0)
    y0, u, theta, rules, w, cost, ac, coef = _small(1, Rn, N, T, A, K)
    exps = M.exps_of("std7")
    for sense in (1, -1):
        ref = F.feedback(y0, u, theta, rules, coef, exps, 0.1, q, w, cost, ac, sense, "euler", 5)
        varies = 0
        for p in range(N):
            J = np.empty((Rn, K))
            Ex = np.empty((Rn, K))
            for r in range(Rn):
                for j, (a_on, a_off, period, start) in enumerate(rules):
                    y, on, acc, cnt = float(y0[p]), bool(start), float(cost[j]), 0
                    for k in range(T):
                        if k % period == 0:
                            on = y >= (theta[p, 2 * j + 1] if on else theta[p, 2 * j])
                        arm = a_on if on else a_off
                        if r == 0:
                            assert ref["sched"][p, j, k] == arm
                        for _ in range(5):
                            y = y + _rhs(y, u[p], coef[r, arm], exps) * (0.1 / 5)
                        acc = acc + w[p, k] * y
                        acc = acc + ac[arm]
                        cnt += on
                    J[r, j], Ex[r, j] = acc, cnt
            assert np.allclose(J, ref["J"][:, p], rtol=1e-13, atol=0) and np.array_equal(Ex, ref["E"][:, p])
            varies += int((Ex[1:].max(axis=0) != Ex[1:].min(axis=0)).sum())
            best = [int(np.argmin(sense * J[r])) for r in range(Rn)]
            assert ref["choice"][p] == best[0]
            votes = [sum(b == j for b in best[1:]) for j in range(K)]
            assert np.array_equal(ref["win"][p], np.array(votes) / (Rn - 1.0))
            for j in range(K):
                g = np.array([sense * ref["J"][r, p, j] - sense * ref["J"][r, p, best[r]] for r in range(Rn)])
                for s, v in enumerate((ref["J"][:, p, j], g, Ex[:, j])):
                    rep = sorted(v[1:])
                    got = ref["out"][p, j, s]
                    assert got[0] == v[0]
                    assert abs(got[1] - sum(rep) / len(rep)) <= 1e-14 * max(1.0, abs(got[1]))
                    assert abs(got[2] - np.std(v[1:], ddof=1)) <= 1e-13
                    assert got[3] == rep[0] and got[5] == rep[-1]
                    pos = 0.3 * (len(rep) - 1)
                    i = int(np.floor(pos))
                    assert abs(got[4] - (rep[i] + (pos - i) * (rep[i + 1] - rep[i]))) <= 1e-14 * max(1.0, abs(got[4]))
        assert varies > 0


def test_reference_rules():
    """The header's rules on the restatement: -Inf / +Inf thresholds are the constant plans of regimen_ref, a period
    >= T decides once, a NaN threshold means off, hysteresis holds the flag between the thresholds, a NaN replicate
    turns the statistics of the row NaN (the exposure too) but not the point values, and the exposure is a count."""
    import feedback_ref as F
    import library_matrix as M
    import regimen_ref as G
    Rn, N, T, A, K = 9, 5, 11, 2, 3
    q = (0.0, 0.5, 1.0)
    exps = M.exps_of("std7")
    y0, u, theta, rules, w, cost, ac, coef = _small(2, Rn, N, T, A, K)
    base = F.feedback(y0, u, theta, rules, coef, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    assert (base["win"].sum(axis=1) == 1.0).all() and (base["out"][:, :, 1] >= 0).all()
    assert ((base["E"] >= 0) & (base["E"] <= T) & (base["E"] == np.round(base["E"]))).all()
    # always on / always off: regimen_ref under the constant plans, bit for bit; exposure T / 0 with std 0
    for th, start, col, expo in ((-np.inf, 0, 0, T), (np.inf, 0, 1, 0), (-np.inf, 1, 0, T)):
        rl = rules.copy()
        rl[:, 3] = start
        fb = F.feedback(y0, u, np.full((N, 2 * K), th), rl, coef, exps, 0.1, q, w, cost, None, 1, "rk4", 1)
        plans = np.broadcast_to(rl[:, col][:, None, None], (K, N, T)).astype(np.int8)
        rg = G.regimen(y0, u, plans, coef, exps, 0.1, q, w, cost, 1, "rk4", 1)
        assert np.array_equal(fb["choice"], rg["choice"]) and np.array_equal(fb["win"], rg["win"])
        assert np.array_equal(fb["out"][:, :, :2], rg["out"])
        assert (fb["out"][:, :, 2, [0, 1, 3, 4, 5]] == expo).all() and (fb["out"][:, :, 2, 2] == 0).all()
        assert (fb["sched"] == plans.transpose(1, 0, 2)).all()
    # +Inf with start_on = 1 and theta_off = -Inf: the flag holds, always on
    th = np.full((N, 2 * K), np.inf)
    th[:, 1::2] = -np.inf
    rl = rules.copy()
    rl[:, 3] = 1
    assert (F.feedback(y0, u, th, rl, coef, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)["E"] == T).all()
    # period >= T: decided once, on y0: the same exposure, 0 or T, in every replicate
    rl = rules.copy()
    rl[:, 2] = (T, T + 1, 2147483647)
    one = F.feedback(y0, u, theta, rl, coef, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    want = np.where(y0[:, None] >= np.where(rl[:, 3] == 1, theta[:, 1::2], theta[:, 0::2]), T, 0)
    assert (one["E"] == want[None]).all() and (one["out"][:, :, 2, 2] == 0).all()
    # a NaN threshold means off
    th = theta.copy()
    th[:, 2] = th[:, 3] = np.nan
    off = F.feedback(y0, u, th, rules, coef, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    assert (off["E"][:, :, 1] == 0).all() and (off["sched"][:, 1] == rules[1, 1]).all()
    assert np.array_equal(off["E"][:, :, 0], base["E"][:, :, 0])
    # hysteresis: with theta_off far below, a rule that switches on stays on
    th = theta.copy()
    th[:, 1::2] = -1e9
    hy = F.feedback(y0, u, th, rules, coef, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    on = hy["sched"] == rules[None, :, 0, None]
    assert (np.diff(on.astype(int), axis=2) >= 0).all() and (hy["E"] >= base["E"]).all()
    # a NaN replicate r >= 1: every statistic of the row but the point is NaN, the exposure's too
    cn = coef.copy()
    cn[4] = np.nan
    ab = F.feedback(y0, u, theta, rules, cn, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    assert np.isnan(ab["out"][..., 1:]).all() and np.array_equal(ab["out"][..., 0], base["out"][..., 0])
    assert (ab["best"][4] == -1).all() and np.isnan(ab["E"][4]).all() and np.array_equal(ab["sched"], base["sched"])
    # NaN in arm 1 only: a rule that never uses arm 1 in that replicate keeps its statistics
    cn = coef.copy()
    cn[4, 1, 2] = np.nan
    rl = rules.copy()
    rl[0, :2] = 0
    rl[1, :2] = 1                                   # rule 1 is on arm 1 throughout: the replicate abstains
    ab = F.feedback(y0, u, theta, rl, cn, exps, 0.1, q, w, cost, ac, 1, "rk4", 1)
    assert np.isfinite(ab["out"][:, 0, 0]).all() and np.isfinite(ab["out"][:, 0, 2]).all()
    assert np.isnan(ab["out"][:, :, 1, 1:]).all()
    # the arm cost is what separates two rules with the same trajectory and different arms... and K = 1
    one = F.feedback(y0, u, theta[:, :2], rules[:1], coef, exps, 0.1, q, w, cost[:1], ac, 1, "rk4", 1)
    assert (one["choice"] == 0).all() and (one["win"] == 1.0).all() and np.isinf(one["margin"]).all()
    reg = np.delete(one["out"][:, 0, 1], 2, axis=-1)
    assert (reg == 0.0).all() and not np.signbit(reg).any()


def test_parity_case_inputs_are_unambiguous():
    """The input conditions of the GPU parity cases.  Every decision margin and every argmin margin is >= 1e-8, a
    hundred times the GPU bar of 1e-10, so ``choice``, ``win``, ``sched`` and the exposure counts are compared exactly
    there.  In every case with R >= 17 at least one (row, rule) has an exposure that differs between the replicates,
    and (K >= 2) at least two rules win somewhere: the per-lane path is not vacuous."""
    import feedback_ref as F
    for c, cid in zip(F.CASES, F.CASE_IDS):
        ref = F.case(*c)[-1]
        Rn, K = c[0], c[4]
        dm, am = float(ref["dmargin"].min()), float(ref["margin"].min())
        Ex = ref["E"][1:]
        vary = int((Ex.max(axis=0) != Ex.min(axis=0)).sum())
        winners = np.unique(ref["best"][ref["best"] >= 0])
        print(f"{cid}: decision margin {dm:.3e}, argmin margin {am:.3e}, exposure varies in {vary} of {Ex[0].size} "
              f"(row, rule) pairs, {winners.size} distinct winners")
        assert dm >= 1e-8, cid
        assert am >= 1e-8, cid
        assert not np.isnan(ref["out"]).any() or Rn == 2, cid
        if Rn >= 17:
            assert vary >= 1, cid
            if K >= 2:
                assert winners.size >= 2, cid
