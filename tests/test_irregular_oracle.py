"""CPU tests of the discovery on irregular observation grids: the numpy oracle (tests/irregular_ref.py)
against numpy.gradient, exact polynomial differentiation, the uniform five-point stencil and its own longdouble
run; and the extension ABI (include/insite_irregular.h) without a device."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irregular_ref as IR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "insite_irregular.h")
EXPS = R.poly_library(3, 2, True)


@pytest.fixture(scope="module")
def L():
    from insite_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------ the estimator
def test_three_samples_is_numpy_gradient_on_c5_grids():
    rng = np.random.default_rng(0)
    t, n_obs = IR.c5_grid(40, rng)
    x, _, _ = IR.decay_cohort(t, n_obs, rng, noise=0.01)
    for p in range(t.shape[0]):
        Lp = int(n_obs[p])
        d = IR.lagrange_derivative(x[p, :Lp], t[p, :Lp], 3)
        ref = np.gradient(x[p, :Lp], t[p, :Lp], edge_order=2)
        np.testing.assert_allclose(d, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())


@pytest.mark.parametrize("W", [3, 5])
def test_polynomials_below_the_window_are_exact(W):
    rng = np.random.default_rng(W)
    for _ in range(20):
        Lp = int(rng.integers(W, 40))
        t = np.cumsum(rng.uniform(0.05, 1.0, Lp))
        for deg in range(W):
            c = rng.normal(size=deg + 1)
            d = IR.lagrange_derivative(np.polyval(c, t), t, W)
            ref = np.polyval(np.polyder(c), t) if deg else np.zeros(Lp)
            scale = max(1.0, float(np.abs(np.polyval(np.abs(c), t)).max()))
            assert np.abs(d - ref).max() <= 1e-9 * scale, (deg, np.abs(d - ref).max(), scale)


def test_five_samples_interior_is_fd_order4_on_a_uniform_grid():
    rng = np.random.default_rng(2)
    dt = 10.0 / 60.0
    t = np.arange(60) * dt
    x = 30.0 * np.exp(-0.6 * t) + 0.01 * rng.normal(size=60)
    d = IR.lagrange_derivative(x, t, 5)
    np.testing.assert_allclose(d[2:-2], R.fd_order4(x, dt)[2:-2], rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("fd", ["nonuniform2", "nonuniform4"])
def test_float64_oracle_agrees_with_longdouble(fd, noise):
    """Error of G and of b relative to the array's largest entry, at the largest cohort of the GPU parity test.
    Measured (seeds 5, 6, 7; smallest gaps 2.6e-6, 5.4e-8, 3.9e-6): G <= 1.2e-15; b <= 2.7e-14 (three samples)
    and <= 7.4e-14 (five samples).  The error of b is the conditioning of a stencil on clustered nodes
    (~ eps |x| / gap per sample) and does not shrink with the gap alone: it is set by the few worst windows against
    a largest entry that grows with the cohort, so a 60-patient cohort can reach 3e-13 (seed 5)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 here: the oracle has no higher-precision yardstick")
    rng = np.random.default_rng(5)
    t, n_obs = IR.c5_grid(1000, rng)
    x, u, arm = IR.decay_cohort(t, n_obs, rng, noise=noise)
    G, b, _ = IR.gram_irregular(x, t, n_obs, u, arm, EXPS, 2, fd)
    ld = np.longdouble
    Gl, bl, _ = IR.gram_irregular(x.astype(ld), t.astype(ld), n_obs, u.astype(ld), arm, EXPS, 2, fd)
    for got, ref in ((G, Gl), (b, bl)):
        err = float(np.abs(got.astype(ld) - ref).max() / max(1.0, float(np.abs(ref).max())))
        assert err <= 1e-13, (fd, noise, err)


def test_short_patients_contribute_nothing():
    rng = np.random.default_rng(7)
    t, n_obs = IR.edge_grid(24, rng)
    x, u, arm = IR.decay_cohort(t, n_obs, rng)
    for fd, W in IR.WINDOW.items():
        G, b, mom = IR.gram_irregular(x, t, n_obs, u, arm, EXPS, 2, fd)
        assert np.all(mom[n_obs < W] == 0)
        assert G[:, 0, 0].sum() == n_obs[n_obs >= W].sum()


# ------------------------------------------------------------------------------------------ the ABI, no device
def _header_functions():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int32_t|size_t)\s+(insite_\w+)\s*\(", src, re.M)))


def test_header_and_bindings_agree(L):
    from insite_amd import _lib
    fns = _header_functions()
    assert fns == sorted(_lib.EXT_EXPORTS) and len(fns) == 4
    assert not set(fns) & set(_lib.EXPORTS)
    for name in fns:
        assert hasattr(L, name) and name in _lib._SIGNATURES, name
    src = open(HEADER).read()

    def const(name):
        return int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))

    assert const("INSITE_IRREGULAR_ABI_VERSION") == _lib.IRREGULAR_ABI_VERSION == 1
    assert (const("INSITE_FD_NONUNIFORM2"), const("INSITE_FD_NONUNIFORM4")) == \
        (_lib.FD_NONUNIFORM2, _lib.FD_NONUNIFORM4) == (4, 5)
    assert L.insite_irregular_abi_version() == 1
    assert L.insite_abi_version() == 9


def test_new_symbols_have_c_linkage(L):
    from insite_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in _lib.EXT_EXPORTS:
        assert name in syms, name


def test_invalid_arguments_rejected_without_device(L):
    """Every check of insite_irregular.h happens before any HIP call (this host has no GPU)."""
    from insite_amd import _lib
    nul = ctypes.c_void_p(0)
    exps = np.ascontiguousarray(EXPS.astype(np.int8))
    ep = exps.ctypes.data_as(ctypes.c_void_p)
    x = (ctypes.c_double * 600)()
    g = (ctypes.c_double * 98)()
    bb = (ctypes.c_double * 14)()
    n4 = _lib.FD_NONUNIFORM4
    gram, fit = L.insite_gram_irregular_f64, L.insite_sindy_fit_irregular_f64

    def call(ldx=60, ld_t=60, N=10, T=60, U=2, A=2, e=ep, F=7, fd=n4, G=g, b=bb, ws=nul, wsn=0):
        return gram(x, ldx, x, ld_t, x, x, x, N, T, U, A, e, F, fd, G, b, nul, ws, wsn, nul)

    assert call(ldx=59) == -1 and call(ld_t=59) == -1                     # leading dimensions below T_max
    assert call(A=0) == -1 and call(A=5) == -1                            # n_arms outside 1..4
    for kind in (_lib.FD_SMOOTHED4, _lib.FD_ORDER4, _lib.FD_ORDER1, _lib.FD_SMOOTHED1, 6, -1):
        assert call(fd=kind) == -1                                        # not one of the two new kinds
    assert call(N=-1) == -1 and call(T=-1) == -1 and call(U=-1) == -1     # negative counts
    assert call(G=nul) == -1 and call(b=nul) == -1                        # NULL outputs
    e2 = exps.copy()
    e2[1, 0] = 2
    assert call(e=e2.ctypes.data_as(ctypes.c_void_p)) == -2               # state exponent above 1
    assert call(F=_lib.MAX_TERMS + 1) == gram_f64_status(L, _lib.MAX_TERMS + 1, ep)   # outside insite_gram_f64's
    assert call() == -3                                                   # no workspace
    need = L.insite_gram_irregular_workspace_bytes(10, 2, 7)
    assert need > 0 and call(ws=ctypes.cast(x, ctypes.c_void_p), wsn=need - 1) == -3
    assert call(N=0, ws=ctypes.cast(x, ctypes.c_void_p), wsn=L.insite_gram_irregular_workspace_bytes(0, 2, 7)) == 0
    assert L.insite_gram_irregular_workspace_bytes(-1, 2, 7) == 0
    assert L.insite_gram_irregular_workspace_bytes(10, 5, 7) == 0
    assert 0 < need <= L.insite_gram_irregular_workspace_bytes(10 ** 7, 2, 7)
    # the fit validates its own arguments too: NULL coef_out, negative threshold / alpha / max_iter
    co = (ctypes.c_double * 14)()

    def cfit(thr=0.1, alpha=0.5, it=100, coef=co, fd=n4, ldx=60):
        return fit(x, ldx, x, 60, x, x, x, 10, 60, 2, 2, ep, 7, fd, thr, alpha, it, 1, g, bb, coef, nul, nul, nul,
                   nul, 0, nul)

    assert cfit(coef=nul) == -1 and cfit(thr=-0.1) == -1 and cfit(alpha=-1.0) == -1 and cfit(it=-1) == -1
    assert cfit(fd=_lib.FD_ORDER4) == -1 and cfit(ldx=59) == -1
    assert cfit() == -3
    # insite_hip.h's entry points do not know the new kinds
    assert L.insite_gram_f64(x, 60, 0, 60, x, x, x, 10, 2, 2, ep, 7, n4, 0.1, g, bb, nul, 0, nul) == -2
    assert L.insite_gram_f64(x, 60, 0, 60, x, x, x, 10, 2, 2, ep, 7, _lib.FD_NONUNIFORM2, 0.1, g, bb, nul, 0,
                             nul) == -2


def gram_f64_status(L, F, ep):
    """What insite_gram_f64 answers for a library of F terms (the irregular entry points accept the same set)."""
    x = (ctypes.c_double * 600)()
    g = (ctypes.c_double * 400)()
    return L.insite_gram_f64(x, 60, 0, 60, x, x, x, 10, 2, 2, ep, F, 0, 0.1, g, g, ctypes.c_void_p(0), 0,
                             ctypes.c_void_p(0))


def test_ops_refuse_host_tensors(L):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    x = torch.zeros((4, 10), dtype=torch.float64)
    n = torch.full((4,), 10, dtype=torch.int32)
    u = torch.zeros((4, 2), dtype=torch.float64)
    arm = torch.zeros(4, dtype=torch.int8)
    for fn, extra in ((ops.gram_irregular, ()), (ops.plan_gram_irregular, ()),
                      (ops.sindy_fit_irregular, (0.1, 0.5)), (ops.plan_sindy_fit_irregular, (0.1, 0.5))):
        with pytest.raises(ValueError, match="device tensor"):
            fn(x, x, n, u, arm, lib, *extra)
    with pytest.raises(ValueError, match="fd must be"):
        ops.gram_irregular(x, x, n, u, arm, lib, fd="order4")
