"""CPU tests of the weak-form extension ABI (include/insite_weak.h): header, bindings and exported symbols agree,
and insite_hip.h's pinned surface did not move.  The new symbols are listed in ``_lib.WEAK_EXPORTS`` (not in
``_lib.EXT_EXPORTS``, which tests/test_irregular_oracle.py pins to insite_irregular.h's four functions)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_weak.h")
FN_RE = r"^\s*(?:const\s+char\s*\*|int32_t|size_t)\s+(insite_\w+)\s*\("


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
    assert fns == sorted(_lib.WEAK_EXPORTS) and len(fns) == 5
    assert not set(fns) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS))
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_WEAK_ABI_VERSION") == _lib.WEAK_ABI_VERSION == 1
    assert const("INSITE_WEAK_MAX_K") == _lib.WEAK_MAX_K
    assert (const("INSITE_OPT_SR3"), const("INSITE_OPT_STLSQ")) == (_lib.OPT_SR3, _lib.OPT_STLSQ)
    assert L.insite_weak_abi_version() == 1


def test_pinned_headers_did_not_move(L):
    assert len(_functions(os.path.join(ROOT, "include", "insite_hip.h"))) == 43
    assert len(_functions(os.path.join(ROOT, "include", "insite_irregular.h"))) == 4
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.WEAK_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_weak.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 600)()
    xp = ctypes.cast(x, ctypes.c_void_p)
    g = (ctypes.c_double * 98)()
    bb = (ctypes.c_double * 14)()
    co = (ctypes.c_double * 14)()
    gram, fit, sr3 = L.insite_gram_weak_f64, L.insite_sindy_fit_weak_f64, L.insite_sr3_f64
    need = L.insite_gram_weak_workspace_bytes(10, 2, 7, 100)

    def call(ldx=58, lay=0, T=58, ldw=58, K=100, N=10, U=2, A=2, e=ep, F=7, G=g, b=bb, ws=xp, wsn=need, W=x):
        return gram(x, ldx, lay, T, W, x, ldw, K, x, x, x, N, U, A, e, F, G, b, nul, ws, wsn, nul)

    assert call(ldx=57) == -1 and call(lay=1, ldx=9) == -1 and call(ldw=57) == -1   # leading dimensions
    assert call(lay=2) == -1 and call(lay=-1) == -1                                  # layouts of the rollouts
    assert call(T=0) == -1 and call(K=0) == -1 and call(N=-1) == -1 and call(U=-1) == -1
    assert call(A=0) == -1 and call(A=5) == -1
    assert call(G=nul) == -1 and call(b=nul) == -1 and call(W=nul) == -1
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                          # state exponent above 1
    assert call(F=_lib.MAX_TERMS + 1) == -1 and call(e=nul) == -1
    assert call(K=_lib.WEAK_MAX_K + 1) == -2
    assert call(ws=nul) == -3 and call(wsn=need - 1) == -3
    assert call(N=0, wsn=L.insite_gram_weak_workspace_bytes(0, 2, 7, 100)) == 0      # successful no-op
    assert L.insite_gram_weak_workspace_bytes(-1, 2, 7, 100) == 0
    assert L.insite_gram_weak_workspace_bytes(10, 5, 7, 100) == 0
    assert L.insite_gram_weak_workspace_bytes(10, 2, 7, 0) == 0
    assert 512 < need <= L.insite_gram_weak_workspace_bytes(10 ** 7, 2, 7, 100)

    def csr3(S=2, F=7, thr=0.1, nu=1.0, tol=0.1, it=1000, G=g, b=bb, coef=co):
        return sr3(G, b, S, F, thr, nu, tol, it, 1, coef, nul, nul, nul)

    nan = float("nan")
    assert csr3(thr=-0.1) == -1 and csr3(thr=nan) == -1 and csr3(tol=-1.0) == -1 and csr3(tol=nan) == -1
    assert csr3(nu=0.0) == -1 and csr3(nu=-1.0) == -1 and csr3(nu=nan) == -1 and csr3(it=-1) == -1
    assert csr3(S=-1) == -1 and csr3(F=0) == -1 and csr3(F=_lib.MAX_TERMS + 1) == -2
    assert csr3(G=nul) == -1 and csr3(b=nul) == -1 and csr3(coef=nul) == -1
    assert csr3(S=0) == 0

    def cfit(opt=0, thr=0.1, alpha=0.5, nu=1.0, tol=0.1, it=1000, coef=co, wsn=need, ldx=58):
        return fit(x, ldx, 0, 58, x, x, 58, 100, x, x, x, 10, 2, 2, ep, 7, opt, thr, alpha, nu, tol, it, 1, g, bb,
                   coef, nul, nul, nul, xp, wsn, nul)

    assert cfit(opt=2) == -1 and cfit(opt=-1) == -1 and cfit(coef=nul) == -1
    assert cfit(thr=-1.0) == -1 and cfit(alpha=-1.0) == -1 and cfit(nu=0.0) == -1 and cfit(tol=nan) == -1
    assert cfit(it=-1) == -1 and cfit(ldx=57) == -1 and cfit(opt=1, alpha=nan) == -1
    assert cfit(wsn=need - 1) == -3 and cfit(opt=1, wsn=0) == -3


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops, weak
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    x = torch.zeros((4, 10), dtype=torch.float64)
    W, D = weak.test_function_weights(10, 0.1, weak.draw_centres(10, 0.1, 3, 0), device="cpu")
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros(4, dtype=torch.int8)
    rows = torch.full((4,), 10, dtype=torch.int32)
    for fn, extra in ((ops.gram_weak, ()), (ops.plan_gram_weak, ()), (ops.sindy_fit_weak, (0.1,)),
                      (ops.plan_sindy_fit_weak, (0.1,))):
        with pytest.raises(ValueError, match="device tensor"):
            fn(x, W, D, u, arm, rows, lib, *extra)
    G = torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(ValueError, match="device tensor"):
        ops.sr3(G, torch.ones((1, 3), dtype=torch.float64), 0.1)
    with pytest.raises(ValueError, match="device tensor"):
        ops.plan_sr3(G, torch.ones((1, 3), dtype=torch.float64), 0.1)


def test_plugin_keys():
    """``weak_form`` is the new key (``+backbone=weak``); ``wsindy: true`` keeps raising."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    ov = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
          "model.sindy_alpha=0.5"]
    m = SINDY(C.compose(["+backbone=weak"] + ov), device="cpu")
    assert m.weak_form and not m.wsindy and m.weak_K == 100 and m.weak_p == 4 and m.weak_optimizer == "sr3"
    assert not SINDY(C.compose(["+backbone=sindy"] + ov), device="cpu").weak_form
    with pytest.raises(NotImplementedError):
        SINDY(C.compose(["+backbone=weak", "model.wsindy=true"] + ov), device="cpu")
    with pytest.raises(ValueError, match="weak_optimizer"):
        SINDY(C.compose(["+backbone=weak", "model.weak_optimizer=lasso"] + ov), device="cpu")
    for bad in ("model.joint_model=true", "model.ablation_more_complex_basis_functions=true"):
        with pytest.raises(NotImplementedError, match="fit_weak"):
            SINDY(C.compose(["+backbone=weak", bad] + ov), device="cpu").fit_weak(None)
