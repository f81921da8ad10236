"""CPU tests of the segment-bootstrap extension ABI (include/insite_segboot.h): header, bindings and exported symbols
agree, the ten older headers and the eight export lists did not move, the names stay clear of the pins of
tests/test_workspace_matrix.py, every argument check answers before any HIP call, the numpy restatement
tests/segboot_ref.py (the reference of tests/test_gpu_segboot.py) agrees with the literal segment regression, and the
plugin opens its ensemble methods to a segment model only after ``bootstrap_segments``."""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_segboot.h")
FN_RE = r"^\s*(?:const\s+char\s*\*|int32_t|size_t)\s+(insite_\w+)\s*\("

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_ref as BR  # noqa: E402
import library_matrix as M  # noqa: E402
import segboot_ref as SB  # noqa: E402
from oracle import cancer_sim_ref as CS  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import segments_ref as S  # noqa: E402

EXPORT_LISTS = {"EXPORTS": 43, "EXT_EXPORTS": 4, "WEAK_EXPORTS": 5, "BOOT_EXPORTS": 4, "EFFECT_EXPORTS": 3,
                "COHORT_EXPORTS": 5, "REGIMEN_EXPORTS": 3, "POLICY_EXPORTS": 5}


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


# ---------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------
def test_header_bindings_and_symbols_agree(L):
    from insite_amd import _lib
    fns = _functions(HEADER)
    assert fns == sorted(_lib.SEGBOOT_SYMBOLS) and len(fns) == 5
    assert all(f.startswith("insite_segboot_") for f in fns)
    older = set(_lib.FEEDBACK_SYMBOLS) | set(_lib.RULEVALUE_SYMBOLS)
    for name in EXPORT_LISTS:
        older |= set(getattr(_lib, name))
    assert not set(fns) & older
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {s for s in syms if s.startswith("insite_segboot_")} == set(fns)
    src = open(HEADER).read()
    assert int(re.search(r"#define INSITE_SEGBOOT_ABI_VERSION (\d+)", src).group(1)) == _lib.SEGBOOT_ABI_VERSION == 1
    assert L.insite_segboot_abi_version() == 1
    assert ("insite_segboot_abi_version", 1, "segboot ") in _lib._ABI_VERSIONS
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
        if name != "insite_segboot_abi_version":
            assert len(_prototype(src, name).split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_older_headers_and_export_lists_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    for header, n in (("insite_hip.h", 43), ("insite_irregular.h", 4), ("insite_weak.h", 5), ("insite_bootstrap.h", 4),
                      ("insite_effect.h", 3), ("insite_cohort.h", 5), ("insite_regimen.h", 3), ("insite_policy.h", 5),
                      ("insite_feedback.h", 2), ("insite_rulevalue.h", 5)):
        assert len(_functions(os.path.join(inc, header))) == n, header
    for getter, want in (("insite_abi_version", 9), ("insite_irregular_abi_version", 1), ("insite_weak_abi_version", 1),
                         ("insite_bootstrap_abi_version", 1), ("insite_effect_abi_version", 1),
                         ("insite_cohort_abi_version", 1), ("insite_regimen_abi_version", 1),
                         ("insite_policy_abi_version", 1), ("insite_feedback_abi_version", 1),
                         ("insite_rulevalue_abi_version", 1)):
        assert getattr(L, getter)() == want, getter
    for name, n in EXPORT_LISTS.items():
        assert len(getattr(_lib, name)) == n, name
    assert len(_lib.FEEDBACK_SYMBOLS) == 2 and len(_lib.RULEVALUE_SYMBOLS) == 5


def test_names_stay_clear_of_the_pins():
    """tests/test_workspace_matrix.py pins the ``_lib`` names that end in EXPORTS and every signature that ends in
    (void* workspace, size_t, void* stream): the new list is SEGBOOT_SYMBOLS and the workspace stands before the
    outputs."""
    from insite_amd import _lib
    assert {n for n in dir(_lib) if n.endswith("EXPORTS")} == set(EXPORT_LISTS)
    src = open(HEADER).read()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    for name in _lib.SEGBOOT_SYMBOLS:
        args = _lib._SIGNATURES[name][1]
        assert tuple(args[-3:]) != (vp, sz, vp), name
        if name == "insite_segboot_abi_version":
            continue
        words = [a.split()[-1].lstrip("*") for a in _prototype(src, name).split(",")]
        if "workspace" in words:
            i = words.index("workspace")
            assert words[i + 1] == "workspace_bytes" and words[i + 2:i + 4] == ["G_out", "b_out"], name
            assert words[-1] == "stream", name
    assert "workspace" not in _prototype(src, "insite_segboot_moments_f64")


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_segboot.h happens before any HIP call (this host has no GPU), in the documented order."""
    from insite_amd import _lib
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4000)()
    xp = ctypes.cast(x, ctypes.c_void_p)
    mo, gram, fit, wsb = (L.insite_segboot_moments_f64, L.insite_segboot_gram_f64, L.insite_segboot_fit_f64,
                          L.insite_segboot_workspace_bytes)

    def cmom(xx=xp, ldx=23, arm=xp, lda=22, lay=0, T=23, sl=xp, N=10, A=4, fd=_lib.FD_ORDER1, dt=0.1, out=xp):
        return mo(xx, ldx, arm, lda, lay, T, sl, N, A, fd, dt, out, nul)

    assert cmom(lay=2) == -1 and cmom(lay=-1) == -1
    assert cmom(lay=2, fd=0) == -1                                # the layout answers before fd_kind
    assert cmom(N=-1) == -1 and cmom(A=0) == -1 and cmom(A=5) == -1
    assert cmom(dt=0.0) == -1 and cmom(dt=-1.0) == -1 and cmom(dt=float("nan")) == -1
    assert cmom(T=0) == -1 and cmom(ldx=0) == -1 and cmom(lda=0) == -1
    assert cmom(ldx=22) == -1 and cmom(lda=21) == -1              # patient-major: ld >= n_steps / n_steps - 1
    assert cmom(lay=1, ldx=9) == -1 and cmom(lay=1, ldx=10, lda=9) == -1 and cmom(lay=1, ldx=10, lda=10, N=0) == 0
    assert cmom(xx=nul) == -1 and cmom(arm=nul) == -1 and cmom(sl=nul) == -1 and cmom(out=nul) == -1
    assert cmom(fd=_lib.FD_SMOOTHED4) == -2 and cmom(fd=_lib.FD_ORDER4) == -2 and cmom(fd=7) == -2
    assert cmom(xx=nul, fd=7) == -1                               # NULL answers before fd_kind
    assert cmom(ldx=2 ** 31) == -2 and cmom(lda=2 ** 31) == -2 and cmom(lay=1, ldx=2 ** 31, lda=2 ** 31) == -2
    assert cmom(N=0) == 0 and cmom(N=0, xx=nul, arm=nul, sl=nul, out=nul) == 0     # successful no-op

    need = wsb(10, 4, 7, 3)
    g = (ctypes.c_double * (3 * 4 * 49))()
    bb = (ctypes.c_double * (3 * 4 * 7))()
    co = (ctypes.c_double * (3 * 4 * 7))()

    def call(mom=xp, u=xp, off=0, N=10, U=2, A=4, e=ep, F=7, Rn=3, seed=7, ws=xp, wsn=need, G=g, b=bb):
        return gram(mom, u, off, N, U, A, e, F, Rn, seed, ws, wsn, G, b, nul)

    assert call(mom=nul) == -1 and call(u=nul) == -1 and call(G=nul) == -1 and call(b=nul) == -1
    assert call(N=-1) == -1 and call(off=-1) == -1 and call(off=2 ** 63 - 5) == -1
    assert call(Rn=0) == -1 and call(Rn=-3) == -1 and call(A=0) == -1 and call(A=5) == -1
    assert call(e=nul) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(F=_lib.MAX_TERMS + 1) == -1 and call(F=0) == -1
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                          # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call(Rn=_lib.BOOT_MAX_REPLICATES + 1) == -2
    assert call(Rn=_lib.BOOT_MAX_REPLICATES + 1, e=e3.ctypes.data_as(ctypes.c_void_p)) == -1   # the table first
    assert call(Rn=0, wsn=0) == -1 and call(e=e2.ctypes.data_as(ctypes.c_void_p), wsn=0) == -2  # ... the workspace last
    assert call(ws=nul) == -3 and call(wsn=need - 1) == -3 and call(wsn=0) == -3
    assert call(N=0, wsn=wsb(0, 4, 7, 3)) == 0 and call(N=0, mom=nul, u=nul, wsn=wsb(0, 4, 7, 3)) == 0
    assert call(U=0, u=nul, e=np.zeros((7, 1), np.int8).ctypes.data_as(ctypes.c_void_p), N=0) == 0

    # the documented zero queries, and a bound for every shape
    assert wsb(-1, 4, 7, 3) == 0 and wsb(10, 5, 7, 3) == 0 and wsb(10, 0, 7, 3) == 0
    assert wsb(10, 4, 0, 3) == 0 and wsb(10, 4, _lib.MAX_TERMS + 1, 3) == 0
    assert wsb(10, 4, 7, 0) == 0 and wsb(10, 4, 7, _lib.BOOT_MAX_REPLICATES + 1) == 0
    assert 512 < need <= wsb(10 ** 7, 4, 7, 3) and need % 8 == 0
    assert wsb(10 ** 6, 4, 9, _lib.BOOT_MAX_REPLICATES) < 2 ** 30
    # the tiling is insite_bootstrap.h's: the same partials for the same column count
    for N, A, F, Rn in ((10, 4, 7, 3), (10 ** 6, 4, 7, 1024), (300, 2, 9, 200), (1, 1, 1, 1)):
        assert wsb(N, A, F, Rn) == L.insite_bootstrap_workspace_bytes(N, A, F, Rn)

    nan = float("nan")

    def cfit(thr=0.1, alpha=0.5, it=100, coef=co, wsn=need, Rn=3, N=10, A=4):
        return fit(xp, xp, 0, N, 2, A, ep, 7, Rn, 7, thr, alpha, it, 1, xp, wsn, g, bb, coef, nul, nul, nul)

    assert cfit(coef=nul) == -1 and cfit(thr=-1.0) == -1 and cfit(thr=nan) == -1
    assert cfit(alpha=-1.0) == -1 and cfit(alpha=nan) == -1 and cfit(it=-1) == -1
    assert cfit(Rn=0) == -1 and cfit(A=5) == -1 and cfit(Rn=_lib.BOOT_MAX_REPLICATES + 1) == -2
    assert cfit(wsn=need - 1) == -3 and cfit(coef=nul, wsn=0) == -1
    assert cfit(N=0) == 0


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    mom = torch.zeros((4, 4, 5), dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    for fn, extra in ((ops.segboot_gram, ()), (ops.plan_segboot_gram, ()), (ops.sindy_bootstrap_segments, (0.1,)),
                      (ops.plan_sindy_bootstrap_segments, (0.1,))):
        with pytest.raises(ValueError, match="device tensor"):
            fn(mom, u, lib, 8, *extra)
    x = torch.zeros((4, 9), dtype=torch.float64)
    arm = torch.zeros((4, 8), dtype=torch.int8)
    sl = torch.zeros(4, dtype=torch.int32)
    for fn in (ops.segment_moments, ops.plan_segment_moments):
        with pytest.raises(ValueError, match="device tensor"):
            fn(x, arm, sl, 0.1)
        with pytest.raises(ValueError, match="fd must be"):
            fn(x, arm, sl, 0.1, fd="smoothed4")
        with pytest.raises(ValueError, match="layout"):
            fn(x, arm, sl, 0.1, layout="tile")


# ---------------------------------------------------------------------------------------------------
# the restatement against the literal
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fd", M.SEG_FDS)
@pytest.mark.parametrize("n_arms", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["std7", "noone3"])
def test_entries_sum_to_the_segment_gram(name, n_arms, fd):
    """Replicate 0 of the restatement (every weight 1) is ``library_matrix.segments_ref``: the per-(patient, arm)
    moments carry everything the segment regression sums.  In float64 against the longdouble literal, per entry scale
    (the bar of tests/test_library_matrix.py for a float64 reference)."""
    x, u, arm, sl = SB.segment_inputs(name, n_arms)
    exps = M.exps_of(name)
    mom, sc = SB.moments_case(name, n_arms, fd)
    G, b, _, _ = SB.gram(mom, u, exps, 1, 0, scale_mom=sc)
    Gl, bl, SG, Sb = M.segments_ref(x, u, arm, sl, M.DT, exps, n_arms, fd, np.longdouble)
    assert np.all(np.isfinite(mom))
    if name == "std7":                    # bias first: G[a, 0, 0] is the arm's sample count
        assert np.array_equal(G[0, :, 0, 0], mom[:, :, 0].sum(0))
    rg, rb = M.worst_ratio(G[0], Gl, SG), M.worst_ratio(b[0], bl, Sb)
    print(f"{name} A={n_arms} {fd}: G {rg:.2e} b {rb:.2e}")
    assert rg <= M.SELF_RTOL and rb <= M.SELF_RTOL
    # the scales of the restatement are the literal's
    _, _, SG2, Sb2 = SB.gram(mom, u, exps, 1, 0, scale_mom=sc)
    assert M.worst_ratio(SG2[0], SG, SG) <= M.SELF_RTOL and M.worst_ratio(Sb2[0], Sb, Sb) <= M.SELF_RTOL
    # a patient the cohort gives no rows (seq_len 0) has no moments, and a never-visited arm is five zeros
    assert not mom[sl == 0].any()
    visited = np.zeros(mom.shape[:2], dtype=bool)
    for p in range(x.shape[0]):
        for a, _, _ in S.segment_bounds(arm[p], sl[p]):
            visited[p, a] = True
    assert np.array_equal(mom[:, :, 0] > 0, visited) and not mom[~visited].any()


@pytest.fixture(scope="module")
def cancer():
    """A small cancer_sim training cohort in DE format (oracle.cancer_sim_ref.make_train, 240 patients)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        data, sp, _ = CS.make_train(seed=1, num_patients=240)
    x, u, arm, sl = CS.de_format_segments(data, sp)
    exps = R.poly_library(2, 2, True).astype(np.int64)
    mom, sc = SB.moments(x, arm, sl, R.STANDARD_DT, 4, "order1")
    return x, u, arm, sl, exps, mom, sc


def test_integer_weights_are_repeated_patients(cancer):
    """Replicate r of the restatement is the oracle's segment Gram of the cohort with patient p repeated w_rp times:
    the weight multiplies ALL of the patient's segments, whichever arm they are in.  Both sides are float64 sums of
    the same <= 13 x 240 x 61 products in different orders: the project's Gram bar per entry scale."""
    x, u, arm, sl, exps, mom, sc = cancer
    Rn, seed = 4, 11
    w = BR.weights(seed, Rn, x.shape[0])
    assert w[1:].max() >= 3 and (w[1:] == 0).any()
    G, b, SG, Sb = SB.gram(mom, u, exps, Rn, seed, scale_mom=sc)
    for r in range(Rn):
        rep = np.repeat(np.arange(x.shape[0]), w[r])
        Go, bo, cnt = S.gram_segments(x[rep], u[rep], arm[rep], sl[rep], R.STANDARD_DT, exps, 4, "order1")
        assert np.array_equal(G[r, :, 0, 0], cnt.astype(np.float64))
        rg, rb = M.worst_ratio(G[r], Go, SG[r]), M.worst_ratio(b[r], bo, Sb[r])
        print(f"replicate {r}: G {rg:.2e} b {rb:.2e}")
        assert rg <= M.GRAM_RTOL and rb <= M.GRAM_RTOL


def test_replicate_zero_is_the_segment_fit(cancer):
    """Replicate 0 through ``stlsq_gram`` has the supports of the row-form ``sindy_fit_segments`` and its
    coefficients within 1e-10 (relative to max(1, |c|), the measure of tests/test_gpu_reference_segments.py)."""
    x, u, arm, sl, exps, mom, _ = cancer
    G, b, _, _ = SB.gram(mom, u, exps, 1, 0)
    coef, ind, _, e2 = S.sindy_fit_segments(x, u, arm, sl, R.STANDARD_DT, threshold=1e-3, alpha=0.5)
    assert np.array_equal(e2, exps)
    for a in range(4):
        c, s, _ = R.stlsq_gram(G[0, a], b[0, a], 1e-3, 0.5)
        assert np.array_equal(s, ind[a]), (a, s, ind[a])
        err = float(np.max(np.abs(c - coef[a]) / np.maximum(1.0, np.abs(coef[a]))))
        print(f"arm {a}: {err:.2e}")
        assert err < 1e-10, (a, err)


def test_fit_case_has_no_tie_at_the_threshold():
    """The precondition of tests/test_gpu_segboot.py::test_fit: no ridge iterate of any of its R n_arms systems lies
    within a relative 1e-3 of the threshold."""
    G, b = SB.fit_case()[-2:]
    worst = min(SB.stlsq_margin(G[r, a], b[r, a], SB.FIT_THRESHOLD, SB.FIT_ALPHA)
                for r in range(G.shape[0]) for a in range(G.shape[1]))
    print(f"margin {worst:.3e}")
    assert worst > 1e-3


# ---------------------------------------------------------------------------------------------------
# the plugin
# ---------------------------------------------------------------------------------------------------
def _segment_args(eq, extra=()):
    from insite_amd import config as C
    a = C.compose(["+backbone=sindy", "+dataset=pkpd_sim", "model.sindy_threshold=0.001", "model.sindy_alpha=0.5",
                   *extra])
    a["model"].update({"dataset_name": eq, "dim_treatments": 4, "dim_static_features": 1 if eq == "cancer_sim" else 2,
                       "dim_outcomes": 1})
    return a


def _ensemble_calls(m):
    from insite_amd.effect import ThresholdRule as TR
    two = [TR(0.5), TR(0.2, 0.1)]
    return {"predict_interval": lambda: m.predict_interval(None), "predict_bands": lambda: m.predict_bands(None),
            "treatment_effect": lambda: m.treatment_effect(None, 0),
            "average_effect": lambda: m.average_effect(None, 0),
            "predict_average": lambda: m.predict_average(None), "choose_plan": lambda: m.choose_plan(None, [0, 1]),
            "policy_value": lambda: m.policy_value(None, [0, 1]), "evaluate_rules": lambda: m.evaluate_rules(None, two),
            "rule_value": lambda: m.rule_value(None, two)}


@pytest.mark.parametrize("eq", ["cancer_sim", "EQ_5_B"])
def test_plugin_gate(eq):
    """A fresh segment model refuses every ensemble method, naming it and pointing to ``bootstrap_segments``;
    ``bootstrap`` and ``bootstrap_irregular`` refuse it always; an ensemble marked as the segment model's own passes
    the gate (and reaches the replicate-cap check)."""
    import torch
    from insite_amd import bootstrap
    from insite_amd.sindy import SINDY
    m = SINDY(_segment_args(eq), device="cpu")
    F = m.library.n_terms
    for name, call in _ensemble_calls(m).items():
        with pytest.raises(NotImplementedError, match=rf"{name}.*bootstrap_segments"):
            call()
    # a one-arm-per-patient ensemble on the model does not open it
    m.bootstrap_ = bootstrap.summarize(torch.zeros((1, 4, F), dtype=torch.float64),
                                       torch.ones((1, 4, F), dtype=torch.int8), seed=3)
    for mode in (None, "arms"):
        m.bootstrap_mode_ = mode
        for name, call in _ensemble_calls(m).items():
            with pytest.raises(NotImplementedError, match=name):
                call()
    m.bootstrap_mode_ = "segments"
    for name, call in _ensemble_calls(m).items():
        with pytest.raises(ValueError, match="n_replicates"):
            call()
    for name, call in (("bootstrap", lambda: m.bootstrap(None)),
                       ("bootstrap_irregular", lambda: m.bootstrap_irregular(None, None, None, None, None))):
        with pytest.raises(NotImplementedError, match=rf"{name}.*bootstrap_segments"):
            call()


def test_bootstrap_segments_refuses_what_it_does_not_cover():
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    for extra in (["model.weak_form=true"], ["model.joint_model=true"],
                  ["model.ablation_more_complex_basis_functions=true"]):
        m = SINDY(_segment_args("cancer_sim", extra), device="cpu")
        with pytest.raises(NotImplementedError, match="bootstrap_segments"):
            m.bootstrap_segments(None)
    ov = ["+backbone=sindy", "+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A",
          "model.sindy_threshold=0.1", "model.sindy_alpha=0.5"]
    with pytest.raises(NotImplementedError, match="bootstrap_segments"):
        SINDY(C.compose(ov), device="cpu").bootstrap_segments(None)
