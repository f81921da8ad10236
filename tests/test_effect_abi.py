"""CPU tests of the effect-band extension ABI (include/insite_effect.h): header, bindings and exported symbols agree,
the four older headers did not move, every argument check answers before any HIP call, and the numpy restatement
tests/effect_ref.py (the reference of tests/test_gpu_effect.py) agrees with torch.quantile and numpy.std."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_effect.h")
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
    assert fns == sorted(_lib.EFFECT_EXPORTS) and len(fns) == 3
    older = set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS) | set(_lib.BOOT_EXPORTS)
    assert not set(fns) & older
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_EFFECT_ABI_VERSION") == _lib.EFFECT_ABI_VERSION == 1
    assert const("INSITE_EFFECT_MAX_REPLICATES") == _lib.EFFECT_MAX_REPLICATES == 512
    assert const("INSITE_EFFECT_MAX_QUANTILES") == _lib.EFFECT_MAX_QUANTILES == 16
    assert L.insite_effect_abi_version() == 1
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in ("insite_effect_bands_f64", "insite_effect_workspace_bytes"):
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    inc = os.path.join(ROOT, "include")
    assert len(_functions(os.path.join(inc, "insite_hip.h"))) == 43
    assert len(_functions(os.path.join(inc, "insite_irregular.h"))) == 4
    assert len(_functions(os.path.join(inc, "insite_weak.h"))) == 5
    assert len(_functions(os.path.join(inc, "insite_bootstrap.h"))) == 4
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert L.insite_bootstrap_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5
    assert len(_lib.BOOT_EXPORTS) == 4 and len(_lib.EFFECT_EXPORTS) == 3


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.EFFECT_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_effect.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 4096)()
    qs = np.array([0.025, 0.5, 0.975])
    qp = qs.ctypes.data_as(ctypes.c_void_p)
    bands, wsb = L.insite_effect_bands_f64, L.insite_effect_workspace_bytes

    def call(y0=x, u=x, aa=x, lda=12, ab=x, ldb=12, coef=x, e=ep, F=7, N=5, T=12, U=2, A=2, dt=0.1, m=0, sub=5,
             drop=1e-3, Rn=9, q=qp, Q=3, out=x, ldo=12):
        return bands(y0, u, aa, lda, ab, ldb, coef, e, F, N, T, U, A, dt, m, sub, drop, Rn, q, Q, out, ldo, nul, 0, nul)

    assert call(y0=nul) == -1 and call(u=nul) == -1 and call(aa=nul) == -1 and call(coef=nul) == -1
    assert call(out=nul) == -1 and call(e=nul) == -1 and call(q=nul) == -1
    assert call(N=-1) == -1 and call(T=0) == -1 and call(T=-3) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(A=0) == -1 and call(A=_lib.MAX_ARMS + 1) == -1
    assert call(F=0) == -1 and call(F=_lib.MAX_TERMS + 1) == -1
    assert call(lda=11) == -1 and call(ldb=11) == -1 and call(ldo=11) == -1
    assert call(sub=0) == -1 and call(dt=-0.1) == -1 and call(dt=float("nan")) == -1
    assert call(m=2) == -2 and call(m=-1) == -2                                      # insite_rollout_f64's rule
    assert call(Rn=1) == -1 and call(Rn=0) == -1 and call(Rn=-4) == -1
    assert call(Rn=_lib.EFFECT_MAX_REPLICATES + 1) == -2
    assert call(Q=0) == -1 and call(Q=_lib.EFFECT_MAX_QUANTILES + 1) == -1 and call(Q=-1) == -1
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        qb = np.array([0.5, bad, 0.1])
        assert call(q=qb.ctypes.data_as(ctypes.c_void_p)) == -1, bad
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                          # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    # n_rows = 0: a successful no-op, whatever the pointers; an unused arm_b takes any leading dimension
    assert call(N=0) == 0 and call(N=0, y0=nul, u=nul, aa=nul, coef=nul, out=nul) == 0
    q16 = np.linspace(0.0, 1.0, 16)
    assert call(N=0, ab=nul, ldb=0) == 0 and call(N=0, Rn=512) == 0
    assert call(N=0, Rn=2, q=q16.ctypes.data_as(ctypes.c_void_p), Q=16) == 0
    assert call(N=0, Rn=1) == -1 and call(N=0, T=0) == -1                            # still validated
    # the workspace query: this version needs none
    assert wsb(10, 60, 2, 7, 256, 3) == 0 and wsb(-1, 0, 0, 0, 0, 0) == 0


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0 = torch.zeros(4, dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros((4, 6), dtype=torch.int8)
    coef = torch.zeros((5, 2, 7), dtype=torch.float64)
    for fn in (ops.effect_bands, ops.plan_effect_bands):
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, arm, arm, coef, lib, 0.1, (0.1, 0.9))
        with pytest.raises(ValueError, match="device tensor"):
            fn(y0, u, arm, None, coef, lib, 0.1, (0.1, 0.9))


def test_plugin_raises_for_unsupported_modes_and_before_bootstrap():
    """``predict_bands`` and ``treatment_effect`` cover the per-arm EQ_4 model over the affine library; the joint,
    treatment-segment and degree-4 modes raise, naming the method, and both need ``bootstrap()`` first."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    ov = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
          "model.sindy_alpha=0.5"]
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in ov]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (ov + ["model.joint_model=true"], ov + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="predict_bands"):
                m.predict_bands(None)
            with pytest.raises(NotImplementedError, match="treatment_effect"):
                m.treatment_effect(None, 0)
    m = SINDY(C.compose(["+backbone=sindy"] + ov), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.predict_bands(None)
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.treatment_effect(None, 0)


def test_plugin_names_the_replicate_cap():
    import torch
    from insite_amd import _lib, bootstrap, config as C
    from insite_amd.sindy import SINDY
    ov = ["+backbone=sindy", "+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A",
          "model.sindy_threshold=0.1", "model.sindy_alpha=0.5"]
    m = SINDY(C.compose(ov), device="cpu")
    for R in (1, _lib.EFFECT_MAX_REPLICATES + 1):
        coef = torch.zeros((R, 2, 7), dtype=torch.float64)
        m.bootstrap_ = bootstrap.summarize(coef, torch.ones((R, 2, 7), dtype=torch.int8))
        for call in (lambda: m.predict_bands(None), lambda: m.treatment_effect(None, 0)):
            with pytest.raises(ValueError, match=str(_lib.EFFECT_MAX_REPLICATES)):
                call()


def test_effect_result_scaling():
    """``effect.from_bands``: locations of a and b are shifted and divided, spreads and the effect divided only."""
    import torch
    from insite_amd import effect
    rng = np.random.default_rng(2)
    out = torch.tensor(rng.normal(size=(3, 5, 4, 6)))
    res = effect.from_bands(out, (0.1, 0.9), shift=2.0, scale=4.0)
    assert res.series == ("a", "b", "effect") and res.q == (0.1, 0.9)
    o = out.numpy()
    assert np.array_equal(res.point.numpy()[:2], (o[:2, 0] - 2.0) / 4.0)
    assert np.array_equal(res.mean.numpy()[:2], (o[:2, 1] - 2.0) / 4.0)
    assert np.array_equal(res.quantiles.numpy()[:2], (o[:2, 3:] - 2.0) / 4.0)
    assert np.array_equal(res.std.numpy(), o[:, 2] / 4.0)
    assert np.array_equal(res.point.numpy()[2], o[2, 0] / 4.0)
    assert np.array_equal(res.quantiles.numpy()[2], o[2, 3:] / 4.0)
    assert np.array_equal(res["effect"]["mean"].numpy(), o[2, 1] / 4.0)
    one = effect.from_bands(out[:1], (0.1, 0.9), shift=2.0, scale=4.0)
    assert one.series == ("a",) and np.array_equal(one.mean.numpy()[0], (o[0, 1] - 2.0) / 4.0)
    with pytest.raises(ValueError):
        effect.from_bands(out[:2], (0.1, 0.9))


def test_reference_matches_torch_quantile_and_numpy_std():
    """tests/effect_ref.stats on random [R, T] data with ties: its quantiles equal torch.quantile(..., dim) and its
    standard deviation numpy.std(ddof=1), to 1e-14 relative; the NaN rule and n = 1."""
    import torch
    import effect_ref as E
    rng = np.random.default_rng(11)
    q = (0.0, 0.025, 0.5, 1.0)
    for R, T in ((2, 5), (3, 7), (18, 9), (65, 33), (130, 4), (512, 6)):
        v = rng.normal(size=(R, T)) * 3.0 + 1.0
        v[rng.random((R, T)) < 0.3] = 0.75            # ties
        v[:, 0] = 2.5                                 # a column of equal values
        got = E.stats(v, q)
        rep = v[1:]
        assert got.shape == (3 + len(q), T)
        assert np.array_equal(got[0], v[0])
        want_q = torch.quantile(torch.tensor(rep), torch.tensor(q, dtype=torch.float64), dim=0).numpy()
        assert np.allclose(got[3:], want_q, rtol=1e-14, atol=0.0), R
        assert np.allclose(got[1], rep.mean(0), rtol=1e-14, atol=1e-15), R
        if R > 2:
            want_s = rep.std(0, ddof=1)
            assert np.allclose(got[2], want_s, rtol=1e-14, atol=1e-14 * np.abs(rep).max()), R
            assert np.array_equal(got[2:, 0], [0.0, 2.5, 2.5, 2.5, 2.5])
        else:
            assert np.isnan(got[2]).all()
    # the NaN rule: a NaN among the resamples blanks every statistic but the point; a NaN point blanks only itself
    v = rng.normal(size=(9, 4))
    v[3, 1] = np.nan
    v[0, 2] = np.nan
    got = E.stats(v, q)
    assert np.isnan(got[1:, 1]).all() and got[0, 1] == v[0, 1]
    assert np.isnan(got[0, 2]) and not np.isnan(got[1:, 2]).any()
    tq = torch.quantile(torch.tensor(v[1:]), torch.tensor(q, dtype=torch.float64), dim=0).numpy()
    assert np.array_equal(np.isnan(tq), np.isnan(got[3:]))
