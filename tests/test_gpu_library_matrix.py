"""Every kernel that takes a library table, on the non-default libraries of tests/library_matrix.py: the strong-form
Gram on its MFMA and its scalar path (three load modes, two estimators), which of the two a shape takes (through
insite_gram_moments_f64), the weak, irregular-grid and segment Grams (the scalar per-lane expansion at F = 1 and
F = 9, U = 0 and U = 3, static exponents up to 8), stlsq_kernel<F> / sr3_kernel<F> for every F, and the rollouts.

Every case compares with the plain numpy restatements, never with another kernel.  Gram sums: per entry,
|G - G_ref| <= 1e-10 S_G and |b - b_ref| <= 1e-10 S_b with the scales of tests/library_matrix.py (the entries
of these tables differ by three orders of magnitude; a bound scaled by the largest entry would not see an error
in a small one).  tests/test_library_matrix.py proves on the CPU that the float64 references used here lie
within 1e-13 x scale of their longdouble versions.  Measured worst |error| / scale on an MI355X: 1.3e-15 (strong
MFMA), 1.2e-15 (strong scalar), 1.2e-15 (weak), 3.0e-15 (irregular), 2.3e-15 (segments); run with -s to print them
and the wall time of the file."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}   # family -> worst |error| / scale seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for fam in sorted(WORST):
        print(f"\n[library-matrix] worst error / scale, {fam}: {WORST[fam]:.3e}", end="")
    print(f"\n[library-matrix] wall time of the file: {time.perf_counter() - t0:.1f} s")


def _t(a, dev, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=dev, dtype=dtype)


def _u(u, dev):
    """The statics, or None for a table without any (the ABI takes NULL; the kernels then alias u = x)."""
    return _t(u, dev) if u.shape[1] else None


def _padded(a, ld, dev):
    """[R, C] array -> a device view [R, C] with row stride ld, NaN in the padding."""
    import torch
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float64, device=dev)
    buf[:, :a.shape[1]] = _t(a, dev)
    return buf[:, :a.shape[1]]


def _check(family, got, ref, scale, what, rtol=M.GRAM_RTOL):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert np.all(np.isfinite(got)), (family, what)
    r = M.worst_ratio(got, ref, scale)
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f"{family} {what}: worst |error| / scale {r:.3e}")
    assert r <= rtol, (family, what, r)


def _family(name, n_arms):
    return "strong MFMA" if M.mfma_fits(M.exps_of(name), n_arms) else "strong scalar"


# ---------------------------------------------------------------------------------------------------
# a. strong form
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _strong_args(dev, name, n_arms, T, load):
    """(x, u, arm, rows) on the device and the layout.  pm16: patient-major, even leading dimension (16-byte
    loads); pm8: odd leading dimension (8-byte loads); tm: time-major [T, N + 5].  Padding is NaN."""
    import torch
    x, u, arm, rows = M.strong_inputs(name, n_arms, T)
    N = x.shape[0]
    if load == "tm":
        xd, layout = _padded(np.ascontiguousarray(x.T), N + 5, dev).as_strided((T, N + 5), (N + 5, 1)), "time"
    else:
        ld = T + (T % 2 if load == "pm16" else 1 - T % 2)
        xd, layout = _padded(x, ld, dev), "patient"
        assert xd.stride(0) % 2 == (0 if load == "pm16" else 1) and xd.data_ptr() % 16 == 0
    return (xd, _u(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32)), layout


@pytest.mark.parametrize("fd", M.STRONG_FDS)
@pytest.mark.parametrize("load", M.STRONG_LOADS)
@pytest.mark.parametrize("name,n_arms,T", M.STRONG_CASES)
def test_strong_gram(dev, name, n_arms, T, load, fd):
    import torch
    from insite_amd import ops
    args, layout = _strong_args(dev, name, n_arms, T, load)
    G, b = ops.gram(*args, M.DT, M.LIBS[name], n_arms=n_arms, fd=fd, layout=layout)
    G2, b2 = ops.gram(*args, M.DT, M.LIBS[name], n_arms=n_arms, fd=fd, layout=layout)
    Gr, br, SG, Sb, _ = M.strong_ref(name, n_arms, T, fd)
    fam = _family(name, n_arms)
    _check(fam, G, Gr, SG, f"G {name} A={n_arms} T={T} {load} {fd}")
    _check(fam, b, br, Sb, f"b {name} A={n_arms} T={T} {load} {fd}")
    assert torch.equal(G, G.transpose(1, 2))
    assert torch.equal(G, G2) and torch.equal(b, b2)
    if n_arms == 3:   # arm 1 has no patients
        assert not bool(G[1].any()) and not bool(b[1].any())


# ---------------------------------------------------------------------------------------------------
# b. which path a shape takes, through the public ABI
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fd", M.STRONG_FDS)
@pytest.mark.parametrize("load", M.STRONG_LOADS)
@pytest.mark.parametrize("name,n_arms", [(n, a) for n, a, T in M.STRONG_CASES if T == M.STRONG_T])
def test_gram_moments_succeeds_exactly_where_the_plan_fits(dev, name, n_arms, load, fd):
    """insite_gram_moments_f64 answers INSITE_E_UNSUPPORTED exactly when the MFMA plan is not used.  Where it runs,
    G | b equal ops.gram's bitwise in the patient-major layouts: both calls then cut the cohort into the same
    (64-patient tile, whole trajectory) items.  The time-major ops.gram cuts every trajectory into 16-step ranges,
    so there its sums are compared with the reference only."""
    import torch
    from insite_amd import ops
    from insite_amd._lib import InsiteError
    T = M.STRONG_T
    args, layout = _strong_args(dev, name, n_arms, T, load)
    lib = M.LIBS[name]
    if not M.mfma_fits(lib.exps, n_arms):
        with pytest.raises(InsiteError) as e:
            ops.gram_moments(*args, M.DT, lib, n_arms=n_arms, fd=fd, layout=layout)
        assert e.value.code == -2
        return
    _, _, _, G, b, mom = ops.gram_moments(*args, M.DT, lib, n_arms=n_arms, fd=fd, layout=layout)
    Gr, br, SG, Sb, momr = M.strong_ref(name, n_arms, T, fd)
    _check("strong MFMA", G, Gr, SG, f"moments-call G {name} A={n_arms} {load} {fd}")
    _check("strong MFMA", b, br, Sb, f"moments-call b {name} A={n_arms} {load} {fd}")
    mom = mom.cpu().numpy()
    assert np.array_equal(mom[:, 0], momr[:, 0])
    err = np.abs(mom - momr).max(axis=0)
    print(f"moments: column errors {err} of {np.abs(momr).max(axis=0)}")
    assert np.all(err <= 1e-10 * np.abs(momr).max(axis=0))
    if layout == "patient":
        G1, b1 = ops.gram(*args, M.DT, lib, n_arms=n_arms, fd=fd, layout=layout)
        assert torch.equal(G, G1) and torch.equal(b, b1)


@pytest.mark.parametrize("fd", M.STRONG_FDS)
@pytest.mark.parametrize("layout", ["patient", "time"])
def test_gram_moments_writes_the_moments_of_a_wave_without_a_usable_patient(dev, layout, fd):
    """N = 65: the second 64-patient wave holds one patient, and that one has 3 rows.  The call writes every
    patient's moments, zeros for one with fewer than 5 rows -- also where a whole wave has nothing to stream (the
    output is pre-filled with NaN here)."""
    import torch
    from insite_amd import ops
    name, n_arms, N = "std7", 2, 65
    x, u, arm, rows = M.short_wave_inputs()
    Gr, br, SG, Sb, momr = M.gram_ref(x, u, arm, rows, M.DT, M.exps_of(name), n_arms, fd)
    xd = _t(x, dev) if layout == "patient" else _t(x.T, dev)
    F = M.TABLE[name][0]
    out = (None, None, None, torch.full((n_arms, F, F), float("nan"), dtype=torch.float64, device=dev),
           torch.full((n_arms, F), float("nan"), dtype=torch.float64, device=dev),
           torch.full((N, 5), float("nan"), dtype=torch.float64, device=dev))
    ops.gram_moments(xd, _t(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32), M.DT, M.LIBS[name],
                     n_arms=n_arms, fd=fd, layout=layout, out=out)
    _check("strong MFMA", out[3], Gr, SG, f"N=65 G {layout} {fd}")
    _check("strong MFMA", out[4], br, Sb, f"N=65 b {layout} {fd}")
    mom = out[5].cpu().numpy()
    assert not momr[64].any() and np.array_equal(mom[rows < 5], momr[rows < 5]), mom[rows < 5]
    assert np.array_equal(mom[:, 0], momr[:, 0])
    assert np.all(np.abs(mom - momr).max(axis=0) <= 1e-10 * np.abs(momr).max(axis=0))


# ---------------------------------------------------------------------------------------------------
# c. weak, irregular and segment Grams (the scalar per-lane expansion)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["patient", "time"])
@pytest.mark.parametrize("n_arms", M.WEAK_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_weak_gram(dev, name, n_arms, layout):
    import torch
    from insite_amd import ops
    x, u, arm, rows, W, D = M.weak_inputs(name, n_arms)
    N, T, K = M.WEAK_SHAPE
    xs = x if layout == "patient" else np.ascontiguousarray(x.T)
    args = (_padded(xs, xs.shape[1] + 3, dev), _padded(W, T + 3, dev), _padded(D, T + 3, dev), _u(u, dev),
            _t(arm, dev, torch.int8), _t(rows, dev, torch.int32))
    out = ops.gram_weak(*args, M.LIBS[name], n_arms=n_arms, layout=layout, moments=True)
    again = ops.gram_weak(*args, M.LIBS[name], n_arms=n_arms, layout=layout, moments=True)
    Gr, br, SG, Sb, momr, Sm = M.weak_case_ref(name, n_arms)
    what = f"{name} A={n_arms} {layout}"
    _check("weak", out[0], Gr, SG, "G " + what)
    _check("weak", out[1], br, Sb, "b " + what)
    _check("weak", out[2], momr, Sm, "moments " + what)
    assert torch.equal(out[0], out[0].transpose(1, 2))
    assert all(torch.equal(p, q) for p, q in zip(out, again))
    off = ~WR.contributes(rows, arm, T, n_arms)
    assert not bool(out[2][_t(off, dev)].any())


@pytest.mark.parametrize("fd", M.IRR_FDS)
@pytest.mark.parametrize("n_arms", M.IRR_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_irregular_gram(dev, name, n_arms, fd):
    import torch
    from insite_amd import ops
    x, t, n_obs, u, arm = M.irregular_inputs(name, n_arms)
    args = (_t(x, dev), _t(t, dev), _t(n_obs, dev, torch.int32), _u(u, dev), _t(arm, dev, torch.int8))
    out = ops.gram_irregular(*args, M.LIBS[name], n_arms=n_arms, fd=fd, moments=True)
    again = ops.gram_irregular(*args, M.LIBS[name], n_arms=n_arms, fd=fd, moments=True)
    Gr, br, SG, Sb, momr = M.irregular_case_ref(name, n_arms, fd)
    what = f"{name} A={n_arms} {fd}"
    _check("irregular", out[0], Gr, SG, "G " + what)
    _check("irregular", out[1], br, Sb, "b " + what)
    mom = out[2].cpu().numpy()
    assert np.array_equal(mom[:, 0], momr[:, 0])
    assert np.all(np.abs(mom - momr).max(axis=0) <= 1e-10 * np.abs(momr).max(axis=0))
    assert torch.equal(out[0], out[0].transpose(1, 2))
    assert all(torch.equal(p, q) for p, q in zip(out, again))


@pytest.mark.parametrize("layout", ["patient", "time"])
@pytest.mark.parametrize("fd", M.SEG_FDS)
@pytest.mark.parametrize("n_arms", M.SEG_ARMS)
@pytest.mark.parametrize("name", M.SCALAR_LIBS)
def test_segment_gram(dev, name, n_arms, fd, layout):
    import torch
    from insite_amd import ops
    x, u, arm, sl = M.segment_inputs(name, n_arms)
    N = x.shape[0]
    if layout == "patient":
        xd, ad = _t(x, dev), _t(arm, dev, torch.int8)
    else:
        xd = _padded(np.ascontiguousarray(x.T), N + 3, dev).as_strided((x.shape[1], N + 3), (N + 3, 1))
        at = np.zeros((arm.shape[1], N + 3), dtype=np.int8)
        at[:, :N] = arm.T
        ad = _t(at, dev, torch.int8)
    args = (xd, ad, _t(sl, dev, torch.int32), _u(u, dev), M.DT, M.LIBS[name])
    G, b = ops.gram_segments(*args, n_arms=n_arms, fd=fd, layout=layout)
    G2, b2 = ops.gram_segments(*args, n_arms=n_arms, fd=fd, layout=layout)
    Gr, br, SG, Sb = M.segment_case_ref(name, n_arms, fd)
    what = f"{name} A={n_arms} {fd} {layout}"
    _check("segments", G, Gr, SG, "G " + what)
    _check("segments", b, br, Sb, "b " + what)
    assert torch.equal(G, G.transpose(1, 2))
    assert torch.equal(G, G2) and torch.equal(b, b2)


# ---------------------------------------------------------------------------------------------------
# d. solvers: every instantiation of stlsq_kernel<F> and sr3_kernel<F>
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", M.SOLVER_F)
def test_stlsq_every_size(dev, F):
    """F = 1..9 are the register-resident instantiations, F = 10 the first size of the one-wave-per-system route."""
    from insite_amd import ops
    G, b = M.solver_systems(F)
    coef, mask, iters = ops.stlsq(_t(G, dev), _t(b, dev), M.STLSQ_THRESHOLD, M.STLSQ_ALPHA)
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    for s in range(G.shape[0]):
        c_ref, s_ref, it_ref = R.stlsq_gram(G[s], b[s], M.STLSQ_THRESHOLD, M.STLSQ_ALPHA)
        assert np.array_equal(mask[s] != 0, s_ref), (s, mask[s], s_ref)
        assert iters[s] == it_ref, (s, iters[s], it_ref)
        np.testing.assert_allclose(coef[s], c_ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("unbias", [True, False])
@pytest.mark.parametrize("F", M.SR3_F)
def test_sr3_every_size(dev, F, unbias):
    """Every system's iteration count is compared: tests/test_library_matrix.py shows that with tol = 0.03 no
    stopping value of the restatement lies within 1e-6 (relative) of tol."""
    from insite_amd import ops
    G, b = M.solver_systems(F)
    coef, mask, iters = ops.sr3(_t(G, dev), _t(b, dev), M.SR3_THRESHOLD, tol=M.SR3_TOL, unbias=unbias)
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    worst = 0.0
    for s in range(G.shape[0]):
        c_ref, s_ref, it_ref, _ = WR.sr3(G[s], b[s], M.SR3_THRESHOLD, tol=M.SR3_TOL, unbias=unbias)
        assert np.array_equal(mask[s] != 0, s_ref), (s, mask[s], s_ref)
        assert iters[s] == it_ref, (s, iters[s], it_ref)
        worst = max(worst, float(np.abs(coef[s] - c_ref).max()))
    print(f"sr3 F={F} unbias={unbias}: coef Linf {worst:.3e}")
    assert worst < 1e-8


def test_sr3_refuses_ten_terms(dev):
    from insite_amd import ops
    from insite_amd._lib import InsiteError
    G, b = M.solver_systems(10)
    with pytest.raises(InsiteError) as e:
        ops.sr3(_t(G, dev), _t(b, dev), M.SR3_THRESHOLD, tol=M.SR3_TOL)
    assert e.value.code == -2


def test_sr3_default_tolerance_decides_one_term_counts_by_the_last_bit(dev):
    """With tol = threshold / nu (the defaults) and one term, the first stopping value IS tol up to rounding, so the
    iteration count of such a system is 1 or 2 by the last bit; masks and coefficients do not depend on it."""
    from insite_amd import ops
    G, b = M.solver_systems(1)
    coef, mask, iters = ops.sr3(_t(G, dev), _t(b, dev), M.SR3_THRESHOLD)
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    near = differ = 0
    for s in range(32):
        c_ref, s_ref, it_ref, stops = WR.sr3(G[s], b[s], M.SR3_THRESHOLD)
        assert np.array_equal(mask[s] != 0, s_ref) and np.abs(coef[s] - c_ref).max() < 1e-8
        if any(abs(v - 0.1) <= 1e-6 * 0.1 for v in stops):
            near += 1
            differ += int(iters[s] != it_ref)
            assert abs(int(iters[s]) - it_ref) <= 1
        else:
            assert iters[s] == it_ref
    print(f"sr3 F=1, default tol: {near} of 32 systems within 1e-6 of tol, {differ} iteration counts differ")
    assert near >= 8


# ---------------------------------------------------------------------------------------------------
# e. rollouts (affine_rates: alpha and beta folded from the table per patient)
# ---------------------------------------------------------------------------------------------------
def _arm_layout(arm, T, layout, dev):
    import torch
    if layout == "patient":
        return _t(arm, dev, torch.int8), "patient"
    N = arm.shape[0]
    tm = np.zeros((T, N + 3), np.int8)
    tm[:, :N] = arm[:, :T].T
    if layout == "bits":
        from insite_amd import ops
        return ops.pack_arm_bits(_t(tm, dev, torch.int8), N), "time_bits"
    return _t(tm, dev, torch.int8), "time"


@pytest.mark.parametrize("method", ["euler5", "rk4"])
@pytest.mark.parametrize("layout,n_arms", [("patient", 2), ("time", 2), ("bits", 2), ("patient", 4), ("time", 4)])
@pytest.mark.parametrize("name", M.ROLLOUT_LIBS)
def test_rollout(dev, name, layout, n_arms, method):
    from insite_amd import ops
    y0, u, arm, coef = M.rollout_inputs(name, n_arms)
    N, T = M.ROLLOUT_SHAPE
    ad, lay = _arm_layout(arm, T, layout, dev)
    y = ops.rollout(_t(y0, dev), _u(u, dev), ad, _t(coef, dev), M.LIBS[name], M.ROLLOUT_DT, method=method, T=T,
                    drop_below=M.DROP_BELOW, layout=lay)
    y = y.cpu().numpy()
    y = y if layout == "patient" else y.T
    y_ref = M.rollout_case_ref(name, n_arms, method)
    print(f"rollout {name} A={n_arms} {layout} {method}: worst relative error "
          f"{float(np.max(np.abs(y - y_ref) / np.maximum(np.abs(y_ref), 1e-300))):.3e}")
    np.testing.assert_allclose(y, y_ref, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("layout", ["time", "patient"])
@pytest.mark.parametrize("name", M.ROLLOUT_LIBS)
def test_rollout_rk45(dev, name, layout):
    """The bounds of tests/test_gpu_rk45.py: relative 1e-9 per sample, RMSE <= 1e-6, 99 % of the attempt counts
    equal."""
    from insite_amd import ops
    t, n_obs, u, arm, y0, coef = M.rk45_inputs(name)
    N, Tm = t.shape
    tn = np.nan_to_num(t, nan=0.0)
    if layout == "patient":
        tt = _t(tn, dev)
        bits = ops.pack_arm_bits(_t(arm, dev), Tm)
    else:
        tt = _t(tn.T, dev)
        bits = ops.pack_arm_bits(_t(arm.T, dev), N)
    y, steps = ops.rollout_rk45(_t(y0, dev), _u(u, dev), bits, tt, _t(n_obs, dev), _t(coef, dev), M.LIBS[name],
                                drop_below=M.DROP_BELOW, layout=layout)
    y = y.cpu().numpy()
    y = y if layout == "patient" else y.T
    ref, ref_steps = M.rk45_case_ref(name)
    valid = ~np.isnan(ref)
    assert np.array_equal(np.isnan(y), ~valid)
    rel = np.abs(y[valid] - ref[valid]) / np.abs(ref[valid])
    print(f"rk45 {name} {layout}: worst relative error {rel.max():.3e}")
    assert rel.max() < 1e-9, rel.max()
    assert np.sqrt(np.mean((y[valid] - ref[valid]) ** 2)) <= 1e-6
    assert np.mean(steps.cpu().numpy() == ref_steps) >= 0.99
