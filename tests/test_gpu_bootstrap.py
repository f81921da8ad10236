"""GPU tests of the patient-level bootstrap (include/insite_bootstrap.h: boot_gram_kernel and its two entry points,
ops.bootstrap_gram / sindy_bootstrap, SINDY.bootstrap / bootstrap_irregular / predict_interval) against the numpy
restatement tests/bootstrap_ref.py.  G | b at the project's Gram bar (GRAM_RTOL per entry scale), coefficients 1e-8
in L-infinity (the bar of tests/test_gpu_deferred.py), supports equal on every system."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_ref as BR  # noqa: E402
import library_matrix as M  # noqa: E402
import weak_ref as WR  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import ref_cohort as RC  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 3, 63, 64, 65, 130, 300)
RS = (1, 2, 16, 17, 33)
ARMS = (1, 2, 3, 4)
OFFSETS = (0, 1, 2 ** 32 + 5)      # the odd value: the pair parity; the large one: the counter's high word
MIN_ROWS = 5
COEF_TOL = 1e-8


@functools.lru_cache(maxsize=None)
def _inputs(name, N, n_arms):
    """(mom [N, 5], u [N, U], arm [N], rows [N]) straight from numpy, so every table runs (the ones the MFMA moment
    plan of the strong form refuses included); rows 3..8 against MIN_ROWS = 5."""
    exps = M.exps_of(name)
    rng = np.random.default_rng(M._seed("bootstrap", name, N, n_arms))
    out = (BR.numpy_moments(rng, N), rng.uniform(0.6, 1.6, (N, exps.shape[1] - 1)), rng.integers(0, n_arms, N),
           rng.integers(3, 9, N))
    for a in out:
        a.setflags(write=False)
    return out


def _up(dev, mom, u, arm, rows):
    import torch
    return (torch.tensor(mom, device=dev), torch.tensor(np.ascontiguousarray(u), device=dev),
            torch.tensor(np.asarray(arm, np.int8), device=dev),
            None if rows is None else torch.tensor(np.asarray(rows, np.int32), device=dev))


def _check(got, ref, what):
    """G | b of the device against (G, b, S_G, S_b) of the restatement, per entry scale."""
    for k, tag in ((0, "G"), (1, "b")):
        g = got[k].cpu().numpy()
        assert g.shape == ref[k].shape and np.all(np.isfinite(g)), (what, tag)
        ratio = M.worst_ratio(g, ref[k], ref[k + 2])
        print(f"{what} {tag}: {ratio:.2e}")
        assert ratio <= M.GRAM_RTOL, (what, tag, ratio)
    G = got[0].cpu().numpy()
    assert np.array_equal(G, np.swapaxes(G, -1, -2)), (what, "G is not symmetric")


def _case(dev, name, N, n_arms, Rn, off, seed=7):
    from insite_amd import ops
    mom, u, arm, rows = _inputs(name, N, n_arms)
    got = ops.bootstrap_gram(*_up(dev, mom, u, arm, rows), M.LIBS[name], Rn, seed=seed, n_arms=n_arms,
                             min_rows=MIN_ROWS, patient_offset=off)
    ref = BR.gram(mom, u, arm, rows, MIN_ROWS, M.exps_of(name), n_arms, Rn, seed, off)
    _check(got, ref, (name, N, n_arms, Rn, off))


@pytest.mark.parametrize("name", sorted(M.LIBS))
def test_gram_matches_reference_on_every_library(dev, name):
    """Every N with a rotating (R, n_arms, offset): the seven cases of a library cover every value of each."""
    li = sorted(M.LIBS).index(name)
    for i, N in enumerate(NS):
        _case(dev, name, N, ARMS[(i + li) % 4], RS[(i + li) % 5], OFFSETS[(i + li) % 3])


@pytest.mark.parametrize("n_arms", ARMS)
def test_gram_std7_every_replicate_count_and_offset(dev, n_arms):
    for Rn in RS:
        for off in OFFSETS:
            _case(dev, "std7", 130, n_arms, Rn, off)


@pytest.mark.parametrize("name,N,n_arms,Rn,off", [
    ("std7", 300, 2, 100, 1),          # 5 column tiles x 3 replicate tiles per wave: three replicate groups
    ("x_only", 300, 1, 100, 0),        # 1 column tile x 4 replicate tiles per wave: two replicate groups
    ("u3_first9", 300, 4, 100, 2),     # 216 columns: three column chunks
    ("u3_mixed9", 65, 3, 50, 2 ** 32 + 5),
    ("std7", 20000, 2, 17, 1),         # more 8-patient groups than waves: two groups per wave
])
def test_gram_more_groups_than_one(dev, name, N, n_arms, Rn, off):
    _case(dev, name, N, n_arms, Rn, off)


def test_patients_that_contribute_nothing(dev):
    """An arm out of range, an arm of -1 and a patient below min_rows, all with NaN moments (one with NaN statics
    too), and an arm without patients: finite outputs equal to the reference's, the empty arm exactly zero."""
    from insite_amd import ops
    mom, u, arm, rows = (a.copy() for a in _inputs("std7", 65, 3))
    arm[arm == 1] = 2
    rows[:] = np.maximum(rows, MIN_ROWS)
    arm[5], arm[9], rows[20] = 3, -1, MIN_ROWS - 1
    mom[[5, 9, 20]] = np.nan
    u[9] = np.nan
    got = ops.bootstrap_gram(*_up(dev, mom, u, arm, rows), M.LIBS["std7"], 17, seed=3, n_arms=3, min_rows=MIN_ROWS)
    ref = BR.gram(mom, u, arm, rows, MIN_ROWS, M.exps_of("std7"), 3, 17, 3)
    _check(got, ref, "nothing")
    assert not got[0][:, 1].any() and not got[1][:, 1].any() and bool(got[0][:, 0].any()) and bool(got[0][:, 2].any())
    # rows = None: min_rows is not read, the short patient counts (its moments must then be finite)
    mom[20] = _inputs("std7", 65, 3)[0][20]
    got = ops.bootstrap_gram(*_up(dev, mom, u, arm, None), M.LIBS["std7"], 17, seed=3, n_arms=3, min_rows=1000)
    _check(got, BR.gram(mom, u, arm, None, 1000, M.exps_of("std7"), 3, 17, 3), "rows=None")


def test_replicate_zero_shards_and_determinism(dev):
    """Replicate 0 is ops.gram's G | b on the std7 cohort; two shards with their offsets add up to the whole; two
    calls are bitwise equal."""
    import torch
    from insite_amd import ops
    lib = M.LIBS["std7"]
    x, u, arm, rows = M.strong_inputs("std7", 2, M.STRONG_T)
    xd, ud = torch.tensor(x, device=dev), torch.tensor(u, device=dev)
    ad, rd = torch.tensor(arm.astype(np.int8), device=dev), torch.tensor(rows.astype(np.int32), device=dev)
    G0, b0 = ops.gram(xd, ud, ad, rd, M.DT, lib, n_arms=2)
    mom = ops.gram_moments(xd, ud, ad, rd, M.DT, lib, n_arms=2)[5]
    whole = ops.bootstrap_gram(mom, ud, ad, rd, lib, 17, seed=5, n_arms=2, min_rows=MIN_ROWS)
    _, _, SG, Sb, _ = M.strong_ref("std7", 2, M.STRONG_T, "smoothed4")
    for got, ref, scale, tag in ((whole[0][0], G0, SG, "G"), (whole[1][0], b0, Sb, "b")):
        ratio = M.worst_ratio(got.cpu().numpy(), ref.cpu().numpy(), scale)
        print(f"replicate 0 vs ops.gram {tag}: {ratio:.2e}")
        assert ratio <= M.GRAM_RTOL, (tag, ratio)
    ref = BR.gram(mom.cpu().numpy(), u, arm, rows, MIN_ROWS, M.exps_of("std7"), 2, 17, 5)
    _check(whole, ref, "whole")
    for cut in (150, 149, 8, 299):
        lo = ops.bootstrap_gram(mom[:cut].contiguous(), ud[:cut].contiguous(), ad[:cut].contiguous(),
                                rd[:cut].contiguous(), lib, 17, seed=5, n_arms=2, min_rows=MIN_ROWS)
        hi = ops.bootstrap_gram(mom[cut:].contiguous(), ud[cut:].contiguous(), ad[cut:].contiguous(),
                                rd[cut:].contiguous(), lib, 17, seed=5, n_arms=2, min_rows=MIN_ROWS,
                                patient_offset=cut)
        for k, tag in ((0, "G"), (1, "b")):
            ratio = M.worst_ratio((lo[k] + hi[k]).cpu().numpy(), whole[k].cpu().numpy(), ref[k + 2])
            assert ratio <= M.GRAM_RTOL, (cut, tag, ratio)
    again = ops.bootstrap_gram(mom, ud, ad, rd, lib, 17, seed=5, n_arms=2, min_rows=MIN_ROWS)
    plan = ops.plan_bootstrap_gram(mom, ud, ad, rd, lib, 17, seed=5, n_arms=2, min_rows=MIN_ROWS)
    third = plan()
    torch.cuda.synchronize()
    for a, b, c in zip(whole, again, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    other = ops.bootstrap_gram(mom, ud, ad, rd, lib, 17, seed=6, n_arms=2, min_rows=MIN_ROWS)
    assert torch.equal(other[0][0], whole[0][0]) and not torch.equal(other[0][1:], whole[0][1:])


@pytest.mark.parametrize("optimizer", ["stlsq", "sr3"])
def test_sindy_bootstrap_on_eq_4_d(dev, optimizer):
    """The reference's EQ_4_D cohort, R = 33: every system's support is the restatement's and its coefficients agree
    to 1e-8.  The thresholds sit far from every coefficient (0.1 against 0.197 and 1.0): no system is excused."""
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    _, u, arm, rows, exps, mom = BR.published_cohort("EQ_4_D")
    Rn, seed = 33, 7
    ref = BR.gram(mom, u, arm, rows, MIN_ROWS, exps, 2, Rn, seed)
    max_iter = 100 if optimizer == "stlsq" else 1000
    plan = ops.plan_sindy_bootstrap(*_up(dev, mom, u, arm, rows), polynomial_library(2, 2, True), Rn, 0.1,
                                    optimizer=optimizer, alpha=0.5, max_iter=max_iter, seed=seed, n_arms=2,
                                    min_rows=MIN_ROWS)
    coef, mask, iters, G, b = plan()
    torch.cuda.synchronize()
    _check((G, b), ref, ("EQ_4_D", optimizer))
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    assert coef.shape == (Rn, 2, 7) and mask.shape == (Rn, 2, 7) and iters.shape == (Rn, 2)
    worst = 0.0
    for r in range(Rn):
        for a in range(2):
            if optimizer == "stlsq":
                c_ref = R.stlsq_gram(ref[0][r, a], ref[1][r, a], 0.1, 0.5)[0]
                s_ref = c_ref != 0
            else:
                c_ref, s_ref = WR.sr3(ref[0][r, a], ref[1][r, a], 0.1)[:2]
            assert np.array_equal(mask[r, a] != 0, s_ref), (r, a, mask[r, a], s_ref)
            worst = max(worst, float(np.abs(coef[r, a] - c_ref).max()))
    print(f"{optimizer}: worst coefficient error {worst:.2e}")
    assert worst < COEF_TOL
    assert np.all(iters > 0)
    # the two-call composition gives the same bits
    G2, b2 = ops.bootstrap_gram(*_up(dev, mom, u, arm, rows), polynomial_library(2, 2, True), Rn, seed=seed, n_arms=2,
                                min_rows=MIN_ROWS)
    c2 = (ops.stlsq(G2, b2, 0.1, 0.5) if optimizer == "stlsq" else ops.sr3(G2, b2, 0.1))[0]
    assert np.array_equal(c2.cpu().numpy().reshape(Rn, 2, 7), coef)


OV = ["+dataset=pkpd_sim", "dataset.equation_str=EQ_4_D", "model.dataset_name=EQ_4_D", "model.sindy_threshold=0.1",
      "model.sindy_alpha=0.5"]


@functools.lru_cache(maxsize=None)
def _train():
    return RC.make_collection("EQ_4_D", with_tests=False)["train"]


def _check_summary(res, Rn):
    coef, mask = res.coef.cpu().numpy(), res.mask.cpu().numpy()
    assert coef.shape == (Rn, 2, 7) and np.all(np.isfinite(coef))
    assert np.array_equal(res.point.cpu().numpy(), coef[0])
    assert np.array_equal(res.inclusion.cpu().numpy(), (mask[1:] != 0).mean(0))
    np.testing.assert_allclose(res.mean.cpu().numpy(), coef[1:].mean(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res.std.cpu().numpy(), coef[1:].std(0, ddof=1), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(res.quantiles.cpu().numpy(), np.quantile(coef[1:], list(res.q), axis=0), rtol=1e-12,
                               atol=1e-15)


@pytest.mark.parametrize("backbone", ["sindy", "weak"])
def test_plugin_bootstrap(dev, backbone):
    """SINDY.bootstrap under the strong and the weak keys: replicate 0 is the fitted model, the summary is numpy's
    on the kernel's own coefficients, and the fitted model is not touched."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    tr = _train()
    extra = ["model.weak_seed=0"] if backbone == "weak" else []
    m = SINDY(C.compose([f"+backbone={backbone}"] + extra + OV), device=dev).fit(tr)
    fitted, eq = m.joint_coefs.copy(), m.global_equation_string
    res = m.bootstrap(tr, n_replicates=33, seed=7)
    assert res is m.bootstrap_ and res.n_replicates == 33 and res.q == (0.025, 0.5, 0.975)
    err = float(np.abs(res.point.cpu().numpy() - fitted).max())
    print(f"{backbone}: point vs fitted {err:.2e}")
    assert err < COEF_TOL and np.array_equal(res.mask[0].cpu().numpy() != 0, m.coef_mask)
    _check_summary(res, 33)
    assert np.array_equal(m.joint_coefs, fitted) and m.global_equation_string == eq
    if backbone == "sindy":
        # the published support of EQ_4_D in every replicate, and a band of the width the issue's prototype saw
        inc = res.inclusion.cpu().numpy()
        assert np.array_equal(inc, (fitted != 0).astype(float)), inc
        j = m.feature_library_names.index("x0")
        lo, hi = res.quantiles[0, 0, j].item(), res.quantiles[2, 0, j].item()
        assert lo < fitted[0, j] < hi and hi - lo < 0.01


def test_plugin_bootstrap_irregular(dev):
    from insite_amd import cohort
    from insite_amd.sindy import SINDY
    coh = cohort.irregular_cohort(300, 3, dev, equation="EQ_4_A")   # noise-free: a sparse, well-conditioned fit
    cfg = {"model": {"sindy_threshold": 0.1, "sindy_alpha": 0.5, "dataset_name": "EQ_4_A"}}
    m = SINDY(cfg, device=dev).fit_irregular(coh.x, coh.t_obs, coh.n_obs, coh.u, coh.arm, fd="nonuniform4")
    res = m.bootstrap_irregular(coh.x, coh.t_obs, coh.n_obs, coh.u, coh.arm, fd="nonuniform4", n_replicates=17,
                                seed=1, quantiles=(0.1, 0.9))
    err = float(np.abs(res.point.cpu().numpy() - m.joint_coefs).max())
    print(f"irregular: point vs fitted {err:.2e}")
    assert err < COEF_TOL and res.q == (0.1, 0.9) and res.quantiles.shape == (2, 2, 7)
    _check_summary(res, 17)


def test_predict_interval(dev):
    """5 rows x R = 17: replicate 0's rollout is the model's own prediction, and the band is numpy.quantile of the
    oracle's rollouts under each replicate's coefficients."""
    from insite_amd import config as C
    from insite_amd.sindy import SINDY, rhs_coefficients
    tr = _train()
    m = SINDY(C.compose(["+backbone=sindy"] + OV), device=dev).fit(tr)
    with pytest.raises(RuntimeError, match="bootstrap"):
        m.predict_interval(tr)
    res = m.bootstrap(tr, n_replicates=17, seed=2)
    band, y = m.predict_interval(tr, quantiles=(0.025, 0.975), max_rows=5, return_replicates=True)
    T = tr.data["prev_outputs"].shape[1]
    assert band.shape == (2, 5, T) and y.shape == (5, 17, T)
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    # compared un-standardised (the volumes are positive): a pure relative bound, no absolute slack near zero
    own = m._predict_device(tr)[:5].cpu().numpy() * std + mean
    np.testing.assert_allclose(y[:, 0].cpu().numpy() * std + mean, own, rtol=1e-10, atol=0)
    prev, stat = R.unscale_inputs(tr.data, tr.scaling_params)
    arms = np.argmax(tr.data["current_treatments"][:5], axis=-1)
    coef = res.coef.cpu().numpy()
    exps = R.poly_library(3, 2, True)
    rolls = np.stack([R.rollout(prev[:5, 0], stat[:5], arms, rhs_coefficients(coef[r]), exps, m.dt, method="euler5")
                      for r in range(1, 17)])
    np.testing.assert_allclose(band.cpu().numpy() * std + mean, np.quantile(rolls, [0.025, 0.975], axis=0), rtol=1e-10,
                               atol=0)
    assert bool((band[0] <= band[1]).all())
    assert m.predict_interval(tr, max_rows=3).shape == (2, 3, T)
