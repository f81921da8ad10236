"""CPU tests of the bootstrap extension ABI (include/insite_bootstrap.h): header, bindings and exported symbols
agree, the three older headers did not move, and every argument check answers before any HIP call.  The new symbols
are listed in ``_lib.BOOT_EXPORTS`` (``EXT_EXPORTS`` and ``WEAK_EXPORTS`` are pinned to their own headers)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_bootstrap.h")
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
    assert fns == sorted(_lib.BOOT_EXPORTS) and len(fns) == 4
    assert not set(fns) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.WEAK_EXPORTS))
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_BOOTSTRAP_ABI_VERSION") == _lib.BOOTSTRAP_ABI_VERSION == 1
    assert const("INSITE_BOOT_MAX_REPLICATES") == _lib.BOOT_MAX_REPLICATES == 16384
    assert L.insite_bootstrap_abi_version() == 1
    # the C prototypes and the ctypes signatures have the same number of arguments
    for name in ("insite_bootstrap_gram_f64", "insite_sindy_bootstrap_f64", "insite_bootstrap_workspace_bytes"):
        proto = re.search(rf"(?:int32_t|size_t)\s+{name}\s*\(([^;]*?)\);", src, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_pinned_headers_did_not_move(L):
    from insite_amd import _lib
    assert len(_functions(os.path.join(ROOT, "include", "insite_hip.h"))) == 43
    assert len(_functions(os.path.join(ROOT, "include", "insite_irregular.h"))) == 4
    assert len(_functions(os.path.join(ROOT, "include", "insite_weak.h"))) == 5
    assert L.insite_abi_version() == 9 and L.insite_irregular_abi_version() == 1 and L.insite_weak_abi_version() == 1
    assert len(_lib.EXPORTS) == 43 and len(_lib.EXT_EXPORTS) == 4 and len(_lib.WEAK_EXPORTS) == 5


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.BOOT_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_bootstrap.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    from oracle import insite_ref as R
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(R.poly_library(3, 2, True).astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 600)()
    xp = ctypes.cast(x, ctypes.c_void_p)
    g = (ctypes.c_double * (3 * 98))()
    bb = (ctypes.c_double * (3 * 14))()
    co = (ctypes.c_double * (3 * 14))()
    gram, fit, wsb = L.insite_bootstrap_gram_f64, L.insite_sindy_bootstrap_f64, L.insite_bootstrap_workspace_bytes
    need = wsb(10, 2, 7, 3)

    def call(mom=x, u=x, arm=x, rows=x, mr=5, N=10, off=0, U=2, A=2, e=ep, F=7, Rn=3, seed=7, G=g, b=bb, ws=xp,
             wsn=need):
        return gram(mom, u, arm, rows, mr, N, off, U, A, e, F, Rn, seed, G, b, ws, wsn, nul)

    assert call(mom=nul) == -1 and call(arm=nul) == -1 and call(u=nul) == -1 and call(G=nul) == -1
    assert call(b=nul) == -1 and call(e=nul) == -1
    assert call(N=-1) == -1 and call(off=-1) == -1 and call(U=-1) == -1 and call(U=4) == -1
    assert call(Rn=0) == -1 and call(Rn=-3) == -1
    assert call(Rn=_lib.BOOT_MAX_REPLICATES + 1) == -2
    assert call(A=0) == -1 and call(A=5) == -1
    assert call(F=_lib.MAX_TERMS + 1) == -1 and call(F=0) == -1
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2                          # state exponent above 1
    e3 = exps.copy()
    e3[2, 1] = -1
    assert call(e=e3.ctypes.data_as(ctypes.c_void_p)) == -1
    assert call(ws=nul) == -3 and call(wsn=need - 1) == -3 and call(wsn=0) == -3
    assert call(N=0, wsn=wsb(0, 2, 7, 3)) == 0                                       # successful no-op
    assert call(N=0, mom=nul, u=nul, arm=nul, wsn=wsb(0, 2, 7, 3)) == 0
    assert wsb(-1, 2, 7, 3) == 0 and wsb(10, 5, 7, 3) == 0 and wsb(10, 0, 7, 3) == 0
    assert wsb(10, 2, 0, 3) == 0 and wsb(10, 2, _lib.MAX_TERMS + 1, 3) == 0
    assert wsb(10, 2, 7, 0) == 0 and wsb(10, 2, 7, _lib.BOOT_MAX_REPLICATES + 1) == 0
    assert 512 < need <= wsb(10 ** 7, 2, 7, 3)
    assert wsb(10 ** 6, 4, 9, _lib.BOOT_MAX_REPLICATES) < 2 ** 30                    # bounded for every shape

    nan = float("nan")

    def cfit(opt=1, thr=0.1, alpha=0.5, nu=1.0, tol=0.1, it=100, coef=co, wsn=need, Rn=3, N=10, A=2):
        return fit(x, x, x, x, 5, N, 0, 2, A, ep, 7, Rn, 7, opt, thr, alpha, nu, tol, it, 1, g, bb, coef, nul, nul,
                   xp, wsn, nul)

    assert cfit(opt=2) == -1 and cfit(opt=-1) == -1 and cfit(coef=nul) == -1
    assert cfit(thr=-1.0) == -1 and cfit(thr=nan) == -1 and cfit(alpha=-1.0) == -1 and cfit(opt=1, alpha=nan) == -1
    assert cfit(nu=0.0) == -1 and cfit(opt=1, nu=nan) == -1 and cfit(tol=nan) == -1 and cfit(opt=0, tol=-1.0) == -1
    assert cfit(it=-1) == -1 and cfit(Rn=0) == -1 and cfit(A=5) == -1
    assert cfit(Rn=_lib.BOOT_MAX_REPLICATES + 1) == -2
    assert cfit(wsn=need - 1) == -3 and cfit(opt=0, wsn=0) == -3
    assert cfit(N=0) == 0 and cfit(opt=0, N=0) == 0


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    mom = torch.zeros((4, 5), dtype=torch.float64)
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros(4, dtype=torch.int8)
    rows = torch.full((4,), 10, dtype=torch.int32)
    for fn, extra in ((ops.bootstrap_gram, ()), (ops.plan_bootstrap_gram, ()), (ops.sindy_bootstrap, (0.1,)),
                      (ops.plan_sindy_bootstrap, (0.1,))):
        with pytest.raises(ValueError, match="device tensor"):
            fn(mom, u, arm, rows, lib, 8, *extra)


def test_summarize_on_host_tensors():
    """``bootstrap.summarize`` is plain torch: the statistics run over the replicates 1..R-1."""
    import torch
    from insite_amd import bootstrap as B
    rng = np.random.default_rng(5)
    coef = rng.normal(size=(9, 2, 3))
    mask = rng.random((9, 2, 3)) < 0.6
    coef[~mask] = 0.0
    res = B.summarize(torch.tensor(coef), torch.tensor(mask.astype(np.int8)), (0.1, 0.5))
    assert res.n_replicates == 9 and res.q == (0.1, 0.5)
    assert np.array_equal(res.point.numpy(), coef[0])
    assert np.allclose(res.inclusion.numpy(), mask[1:].mean(0), rtol=0, atol=1e-15)
    assert np.allclose(res.mean.numpy(), coef[1:].mean(0), rtol=1e-13, atol=1e-15)
    assert np.allclose(res.std.numpy(), coef[1:].std(0, ddof=1), rtol=1e-12, atol=1e-15)
    assert np.allclose(res.quantiles.numpy(), np.quantile(coef[1:], [0.1, 0.5], axis=0), rtol=1e-13, atol=1e-15)
    one = B.summarize(torch.tensor(coef[:1]), torch.tensor(mask[:1].astype(np.int8)))
    assert bool(torch.isnan(one.inclusion).all()) and one.quantiles.shape == (3, 2, 3)
    with pytest.raises(ValueError):
        B.summarize(torch.tensor(coef), torch.tensor(mask[:, :1].astype(np.int8)))


def test_plugin_raises_for_unsupported_modes():
    """``bootstrap``, ``bootstrap_irregular`` and ``predict_interval`` cover the per-arm EQ_4 model over the affine
    library; the joint, treatment-segment and degree-4 modes raise, naming the method."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    ov = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
          "model.sindy_alpha=0.5"]
    seg = [o.replace("EQ_4_A", "EQ_5_A") for o in ov]
    for back in ("+backbone=sindy", "+backbone=weak"):
        for cfg in (ov + ["model.joint_model=true"], ov + ["model.ablation_more_complex_basis_functions=true"], seg):
            m = SINDY(C.compose([back] + cfg), device="cpu")
            with pytest.raises(NotImplementedError, match="bootstrap"):
                m.bootstrap(None)
            with pytest.raises(NotImplementedError, match="bootstrap_irregular"):
                m.bootstrap_irregular(None, None, None, None, None)
            with pytest.raises(NotImplementedError, match="predict_interval"):
                m.predict_interval(None)
    m = SINDY(C.compose(["+backbone=sindy"] + ov), device="cpu")
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.predict_interval(None)
