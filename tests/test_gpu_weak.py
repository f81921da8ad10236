"""GPU tests of the weak-form discovery (include/insite_weak.h: gram_weak_kernel, sr3_kernel and the three entry
points, ops.gram_weak / sr3 / sindy_fit_weak, SINDY.fit_weak) against the numpy restatement tests/weak_ref.py,
never against the code under test.  Tolerances: G | b and the moments at rtol 1e-10 of the largest entry (the
project's bar in tests/test_gpu_deferred.py), coefficients 1e-8 in L-infinity, supports equal."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

EXPS = R.poly_library(3, 2, True)
NAMES = R.library_names(EXPS, ["x0", "u0", "u1"])
DT = 10.0 / 60.0
THRESHOLD = 0.1
# (N, T, K): 4 full 64-patient tiles + 44 patients, T = 2 mod 4, K = 4 mod 16 | one test function, T below a
# chunk | one patient, K = 1 mod 16 | exact tiles | K > 128: two passes over x, the second 2 rows
SHAPES = [(300, 58, 100), (65, 5, 1), (1, 7, 17), (64, 64, 16), (20, 9, 130)]


def _lib():
    from insite_amd.library import polynomial_library
    return polynomial_library(2, 2, True)


def _close(got, ref, scale=None, rtol=1e-10):
    scale = float(np.abs(ref).max()) if scale is None else scale
    err = float(np.abs(got - ref).max())
    print(f"max abs err {err:.3e} of scale {scale:.3e}")
    assert err <= rtol * scale, (err, scale)


@functools.lru_cache(maxsize=None)
def _case(N, T, K, n_arms):
    """Inputs and the restatement's G, b, moments; read-only.  Some patients carry arm = -1 / n_arms or
    rows < T (their samples are NaN: they must reach no output); with n_arms = 3 no patient is in arm 2."""
    rng = np.random.default_rng(10007 * N + 101 * T + K + n_arms)
    x = rng.uniform(0.5, 3.0, (N, 1)) * np.exp(-rng.uniform(0.2, 1.0, (N, 1)) * np.arange(T) * DT) \
        + 0.01 * rng.normal(size=(N, T))
    u = rng.normal(0.5, 0.05, (N, 2))
    arm = rng.integers(0, 2, N)
    rows = np.full(N, T)
    if N > 1:
        k = np.arange(N)
        arm = np.where(k % 11 == 3, -1, np.where(k % 13 == 5, n_arms, arm))
        rows = np.where(k % 7 == 2, T - 1, np.where(k % 17 == 4, T + 3, rows))
    L = (T - 1) * DT
    H = max(L / 20.0, 1.5 * DT)
    W, D = WR.weights(T, DT, rng.uniform(H, L - H, K), H=H)
    G, b = WR.gram(x, u, arm, rows, W, D, EXPS, n_arms)
    mom = WR.moments(x, arm, rows, W, D, n_arms)
    off = ~WR.contributes(rows, arm, T, n_arms)
    x = x.copy()
    x[off] = np.nan
    for a in (x, u, arm, rows, W, D, G, b, mom):
        a.setflags(write=False)
    return x, u, arm, rows, W, D, G, b, mom


def _pad(a, ld, dev):
    """[R, C] array -> a device view with row stride ld."""
    import torch
    buf = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float64, device=dev)
    buf[:, :a.shape[1]] = torch.tensor(np.asarray(a), device=dev)
    return buf[:, :a.shape[1]]


def _up(dev, case, layout="patient", pad=0):
    import torch
    x, u, arm, rows, W, D = case[:6]
    xs = x if layout == "patient" else np.ascontiguousarray(x.T)
    xd = _pad(xs, xs.shape[1] + pad, dev) if pad else torch.tensor(xs, device=dev)
    Wd = _pad(W, W.shape[1] + pad, dev) if pad else torch.tensor(W, device=dev)
    Dd = _pad(D, D.shape[1] + pad, dev) if pad else torch.tensor(D, device=dev)
    return (xd, Wd, Dd, torch.tensor(u, device=dev), torch.tensor(arm.astype(np.int8), device=dev),
            torch.tensor(rows.astype(np.int32), device=dev))


def _check_gram(out, case, n_arms):
    G, b, mom = (o.cpu().numpy() for o in out)
    Gr, br, momr = case[6:9]
    scale = max(float(np.abs(Gr).max()), float(np.abs(br).max()))
    _close(G, Gr, scale)
    _close(b, br, scale)
    _close(mom, momr, float(np.abs(momr).max()))
    off = ~WR.contributes(case[3], case[2], case[4].shape[1], n_arms)
    assert np.all(mom[off] == 0)
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(b))


@pytest.mark.parametrize("N,T,K", SHAPES)
def test_gram_matches_restatement(dev, N, T, K):
    from insite_amd import ops
    case = _case(N, T, K, 2)
    _check_gram(ops.gram_weak(*_up(dev, case), _lib(), n_arms=2, moments=True), case, 2)


@pytest.mark.parametrize("n_arms", [2, 3])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("layout", ["patient", "time"])
def test_first_shape_layouts_strides_arms(dev, layout, pad, n_arms):
    """(300, 58, 100) in both layouts, with ldx / ldw at the minimum and larger and odd, two and three arms (arm 2
    is empty: G = b = 0), two calls bitwise equal."""
    import torch
    from insite_amd import ops
    case = _case(300, 58, 100, n_arms)
    args = _up(dev, case, layout, pad)
    if pad:
        assert args[0].stride(0) % 2 == 1 and args[1].stride(0) % 2 == 1
    out = ops.gram_weak(*args, _lib(), n_arms=n_arms, layout=layout, moments=True)
    _check_gram(out, case, n_arms)
    again = ops.gram_weak(*args, _lib(), n_arms=n_arms, layout=layout, moments=True)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    if n_arms == 3:
        assert not bool(out[0][2].any()) and not bool(out[1][2].any())


def test_empty_arm_is_reported_by_the_solvers(dev):
    """The all-zero arm of the three-arm case: STLSQ's answer is the strong form's (oracle stlsq_gram on zeros),
    SR3 reports iters = -1 and NaN coefficients."""
    from insite_amd import ops
    case = _case(300, 58, 100, 3)
    args = _up(dev, case)
    coef, mask, iters, G, b = ops.sindy_fit_weak(*args, _lib(), THRESHOLD, optimizer="stlsq", alpha=0.5, max_iter=100,
                                                 n_arms=3)
    for a in range(3):
        c_ref, s_ref, it_ref = R.stlsq_gram(case[6][a], case[7][a], THRESHOLD, 0.5)
        assert np.array_equal(mask[a].cpu().numpy() != 0, s_ref)
        assert int(iters[a]) == it_ref
        assert np.abs(coef[a].cpu().numpy() - c_ref).max() < 1e-8
    assert not bool(coef[2].any())
    coef, mask, iters, G, b = ops.sindy_fit_weak(*args, _lib(), THRESHOLD, optimizer="sr3", n_arms=3)
    assert int(iters[2]) == -1 and bool(coef[2].isnan().all()) and not bool(mask[2].any())
    assert int(iters[0]) > 0 and int(iters[1]) > 0


@pytest.mark.parametrize("N,T,K", SHAPES[:4])
def test_per_patient_weak_refit_from_the_moments(dev, N, T, K):
    """mom_out has insite_gram_moments_f64's layout (1 -> c, x -> a, x_dot -> d) and
    insite_fit_per_patient_moments_f64 uses slot 0 as a sum and ``rows`` only to gate short patients, so the
    per-patient weak refit is that call on the weak moments (rows = 0 for a patient that contributes nothing)."""
    import torch
    from insite_amd import ops
    case = _case(N, T, K, 2)
    x, u, arm, rows, W, D = case[:6]
    args = _up(dev, case)
    _, _, mom = ops.gram_weak(*args, _lib(), n_arms=2, moments=True)
    gcoef = np.zeros((2, EXPS.shape[0]))
    gcoef[0, [NAMES.index("x0"), NAMES.index("x0 u0")]] = (-0.05, -1.0)
    gcoef[1, [NAMES.index("x0"), NAMES.index("x0 u1")]] = (-0.15, -1.0)
    on = WR.contributes(rows, arm, T, 2)
    rows_fit = torch.tensor(np.where(on, np.maximum(rows, 5), 0).astype(np.int32), device=dev)
    coef, mask, iters = ops.fit_per_patient_moments(mom, args[3], args[4], rows_fit, max(T, 5), _lib(),
                                                    torch.tensor(gcoef, device=dev), THRESHOLD, 0.5)
    c_ref, m_ref, it_ref = WR.per_patient_fit(x, u, arm, rows, W, D, EXPS, gcoef, THRESHOLD, 0.5)
    valid = (arm >= 0) & (arm < 2)
    assert np.array_equal(iters.cpu().numpy(), it_ref)
    assert np.array_equal(mask.cpu().numpy()[valid], m_ref[valid])
    err = float(np.abs(coef.cpu().numpy() - c_ref).max())
    print(f"per-patient coef Linf {err:.3e}")
    assert err < 1e-8


def test_invalid_arguments_are_refused_with_device_pointers(dev):
    """Each INVALID_ARG / UNSUPPORTED / WORKSPACE case of the header on real device pointers: the calls return
    their status before any launch (the outputs keep their fill)."""
    import ctypes
    import torch
    from insite_amd import _lib as B
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    case = _case(65, 5, 1, 2)
    x, W, D, u, arm, rows = _up(dev, case)
    lib = _lib()
    L = B.load()
    with pytest.raises(B.InsiteError) as e:
        ops.gram_weak(x, W, D, u[:, :1].contiguous(), arm, rows, polynomial_library(1, 2, False))   # has x0^2
    assert e.value.code == -2
    Wk = torch.zeros((B.WEAK_MAX_K + 1, 5), dtype=torch.float64, device=dev)
    with pytest.raises(B.InsiteError) as e:
        ops.gram_weak(x, Wk, Wk, u, arm, rows, lib)
    assert e.value.code == -2
    G = torch.full((2, 7, 7), 7.0, dtype=torch.float64, device=dev)
    b = torch.full((2, 7), 7.0, dtype=torch.float64, device=dev)
    for kw in ({"threshold": -0.1}, {"nu": 0.0}, {"tol": float("nan")}, {"max_iter": -1}):
        args = {"threshold": 0.1, "nu": 1.0, "tol": 0.1, "max_iter": 10}
        args.update(kw)
        with pytest.raises(B.InsiteError) as e:
            ops.sr3(G, b, args["threshold"], nu=args["nu"], tol=args["tol"], max_iter=args["max_iter"])
        assert e.value.code == -1
    with pytest.raises(B.InsiteError) as e:
        ops.sindy_fit_weak(x, W, D, u, arm, rows, lib, 0.1, optimizer="stlsq", alpha=-1.0)
    assert e.value.code == -1
    # raw calls: leading dimension, layout, workspace
    tab = lib.ctypes_table()
    ep = tab.ctypes.data_as(ctypes.c_void_p)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    need = L.insite_gram_weak_workspace_bytes(65, 2, 7, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)

    def call(ldx=5, lay=0, ldw=5, wsn=need, n_arms=2):
        return L.insite_gram_weak_f64(p(x), ldx, lay, 5, p(W), p(D), ldw, 1, p(u), p(arm), p(rows), 65, 2, n_arms, ep,
                                      7, p(G), p(b), ctypes.c_void_p(0), p(ws), wsn, ctypes.c_void_p(0))

    assert call(ldx=4) == -1 and call(ldw=4) == -1 and call(lay=2) == -1 and call(lay=1) == -1 and call(n_arms=5) == -1
    assert call(wsn=need - 1) == -3
    torch.cuda.synchronize()
    assert bool((G == 7.0).all()) and bool((b == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((G == 7.0).any())


@functools.lru_cache(maxsize=None)
def _eq4a():
    tr = RC.make_collection("EQ_4_A", with_tests=False)["train"]
    x, u, arm, rows = R.de_format(tr.data, tr.scaling_params, 1)
    T = int(rows.max())
    return tr, x[:, :T].copy(), u, arm, rows, T


@functools.lru_cache(maxsize=None)
def _eq4a_system(seed):
    _, x, u, arm, rows, T = _eq4a()
    H = WR.half_width(T, DT)
    c = np.random.default_rng(seed).uniform(H, (T - 1) * DT - H, 100)
    W, D = WR.weights(T, DT, c)
    G, b = WR.gram(x, u, arm, rows, W, D, EXPS, 2)
    return c, W, D, G, b


@functools.lru_cache(maxsize=None)
def _sr3_systems():
    """EQ_4_A seeds 0 and 2 (two arms each), then 32 random well-conditioned 7 x 7 systems with a sparse truth."""
    Gs, bs = [], []
    for seed in (0, 2):
        _, _, _, G, b = _eq4a_system(seed)
        Gs += [G[0], G[1]]
        bs += [b[0], b[1]]
    rng = np.random.default_rng(42)
    for _ in range(32):
        A = rng.normal(size=(60, 7)) * rng.uniform(0.5, 2.0, 7)
        c = np.where(rng.random(7) < 0.4, rng.uniform(0.5, 2.0, 7) * rng.choice([-1.0, 1.0], 7), 0.0)
        y = A @ c + 0.05 * rng.normal(size=60)
        Gs.append(A.T @ A)
        bs.append(A.T @ y)
    return np.stack(Gs), np.stack(bs)


@pytest.mark.parametrize("unbias", [True, False])
def test_sr3_matches_restatement(dev, unbias):
    import torch
    from insite_amd import ops
    G, b = _sr3_systems()
    coef, mask, iters = ops.sr3(torch.as_tensor(G, device=dev), torch.as_tensor(b, device=dev), THRESHOLD,
                                unbias=unbias)
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    guarded = 0
    for s in range(G.shape[0]):
        c_ref, s_ref, it_ref, stops = WR.sr3(G[s], b[s], THRESHOLD, unbias=unbias)
        assert it_ref > 0
        assert np.array_equal(mask[s] != 0, s_ref), (s, mask[s], s_ref)
        err = float(np.abs(coef[s] - c_ref).max())
        assert err < 1e-8, (s, err)
        # the iteration count is comparable where no stopping value sits within 1e-6 (relative) of tol
        near = [abs(v - 0.1) <= 1e-6 * 0.1 for v in stops[-2:]]
        if any(near):
            guarded += s >= 4
            assert s >= 4, "the EQ_4_A systems are not near the threshold"
            continue
        assert iters[s] == it_ref, (s, iters[s], it_ref)
    print(f"systems skipped by the guard: {guarded} of 32")
    assert guarded <= 2


def test_sr3_singular_and_max_iter(dev):
    import torch
    from insite_amd import ops
    G = np.stack([np.ones((3, 3)), np.zeros((3, 3)), np.diag([4.0, 1.0, 9.0])])
    b = np.stack([np.ones(3), np.zeros(3), np.array([8.0, 0.01, -18.0])])
    coef, mask, iters = ops.sr3(torch.as_tensor(G, device=dev), torch.as_tensor(b, device=dev), THRESHOLD)
    assert iters.tolist()[:2] == [-1, -1]
    assert bool(coef[:2].isnan().all()) and not bool(mask[:2].any())
    c_ref, s_ref, it_ref, _ = WR.sr3(G[2], b[2], THRESHOLD)
    assert int(iters[2]) == it_ref and np.array_equal(mask[2].cpu().numpy() != 0, s_ref)
    assert np.abs(coef[2].cpu().numpy() - c_ref).max() < 1e-12
    coef0, _, iters0 = ops.sr3(torch.as_tensor(G[2:], device=dev), torch.as_tensor(b[2:], device=dev), THRESHOLD,
                               max_iter=0, unbias=False)
    assert int(iters0[0]) == 0
    np.testing.assert_allclose(coef0[0].cpu().numpy(), b[2] / np.diag(G[2]), rtol=1e-14)


@pytest.mark.parametrize("seed", [0, 2])
def test_sindy_fit_weak_on_eq_4_a(dev, seed):
    """End to end on the reference's EQ_4_A training cohort: weights from insite_amd.weak, the Gram pass and SR3
    in one call; the restatement's support ({x0 u0} / {x0 u1}) and coefficients."""
    import torch
    from insite_amd import ops, weak
    _, x, u, arm, rows, T = _eq4a()
    c, W, D, G_ref, b_ref = _eq4a_system(seed)
    assert np.array_equal(weak.draw_centres(T, DT, 100, seed), c)
    Wd, Dd = weak.test_function_weights(T, DT, c, device=dev)
    _close(Wd.cpu().numpy(), W, rtol=1e-13)
    _close(Dd.cpu().numpy(), D, rtol=1e-13)
    plan = ops.plan_sindy_fit_weak(torch.as_tensor(x, device=dev), Wd, Dd, torch.as_tensor(u, device=dev),
                                   torch.as_tensor(arm.astype(np.int8), device=dev),
                                   torch.as_tensor(rows.astype(np.int32), device=dev), _lib(), THRESHOLD)
    coef, mask, iters, G, b = plan()
    scale = max(float(np.abs(G_ref).max()), float(np.abs(b_ref).max()))
    _close(G.cpu().numpy(), G_ref, scale)
    _close(b.cpu().numpy(), b_ref, scale)
    for a, name in ((0, "x0 u0"), (1, "x0 u1")):
        c_ref, s_ref, it_ref, _ = WR.sr3(G_ref[a], b_ref[a], THRESHOLD)
        assert [NAMES[j] for j in np.nonzero(s_ref)[0]] == [name]
        assert np.array_equal(mask[a].cpu().numpy() != 0, s_ref)
        assert np.abs(coef[a].cpu().numpy() - c_ref).max() < 1e-8
        assert int(iters[a]) == it_ref


def test_plugin_weak_form(dev):
    """SINDY(weak_form=True).fit dispatches to fit_weak, sets the equation string, and the rollout runs."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    tr = _eq4a()[0]
    ov = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_A", "model.dataset_name=EQ_4_A", "model.sindy_threshold=0.1",
          "model.sindy_alpha=0.5", "model.lam=10.0"]
    m = SINDY(C.compose(["+backbone=weak", "model.weak_seed=0"] + ov), device=dev)
    assert m.fit(tr) is m
    assert m.global_equation_string.startswith("Treatment 0: x_dot = ") and "x0*u0" in m.global_equation_string \
        and "x0*u1" in m.global_equation_string
    c_ref = np.stack([WR.sr3(_eq4a_system(0)[3][a], _eq4a_system(0)[4][a], THRESHOLD)[0] for a in range(2)])
    assert np.abs(m.joint_coefs - c_ref).max() < 1e-8
    p = m.get_predictions(tr)
    assert p.shape == tr.data["outputs"].shape and np.all(np.isfinite(p))
    with pytest.raises(NotImplementedError):
        SINDY(C.compose(["+backbone=sindy", "model.wsindy=true"] + ov), device=dev)
