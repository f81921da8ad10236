"""GPU tests of the patient-level bootstrap of the treatment-segment discovery (include/insite_segboot.h:
seg_moments_kernel, segboot_gram_kernel and their entry points, ops.segment_moments / segboot_gram /
sindy_bootstrap_segments, SINDY.bootstrap_segments and the ensemble methods it opens) against the numpy restatement
tests/segboot_ref.py.  Moments and G | b at the project's Gram bar (GRAM_RTOL per entry scale), coefficients 1e-8 in
L-infinity with every support equal (the bars of tests/test_gpu_bootstrap.py), the plugin's bands at the bars of
tests/test_gpu_effect.py and tests/test_gpu_regimen.py."""
import ctypes
import functools
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_ref as BR  # noqa: E402
import effect_ref as E  # noqa: E402
import library_matrix as M  # noqa: E402
import regimen_ref as G  # noqa: E402
import segboot_ref as SB  # noqa: E402
import workspace_matrix as W  # noqa: E402
from oracle import cancer_sim_ref as CS  # noqa: E402
from oracle import insite_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ARMS = (1, 2, 3, 4)
RS = (1, 2, 17, 48, 49, 64, 65, 200)          # 48 | 49 and 64 | 65: the 16 RT edges of RT = 3 and RT = 4
NS = (1, 7, 8, 9, 300)
OFFSETS = (0, 1, 7, 2 ** 33 + 3)              # the pair parity, the last slot of a group, the counter's high word
LOADS = ("pm_even", "pm_odd", "tm")           # patient-major ld = T + 1 | T + 2, time-major ld = N + 5
COEF_TOL = 1e-8
BAND_TOL = 1e-10                              # tests/test_gpu_effect.py, tests/test_gpu_regimen.py


def _t(dev, a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device=dev, dtype=dtype)


# ---------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------
def _load(dev, x, arm, load):
    """(x, arm, layout) on the device behind a padded leading dimension; the padding holds NaN / an arm of 7."""
    import torch
    N, T = x.shape
    if load == "tm":
        xb = torch.full((T, N + 5), float("nan"), dtype=torch.float64, device=dev)
        ab = torch.full((T - 1, N + 5), 7, dtype=torch.int8, device=dev)
        xb[:, :N] = _t(dev, x.T)
        ab[:, :N] = _t(dev, arm.T.astype(np.int8))
        return xb, ab, "time"
    ld = T + (1 if (T + 1) % 2 == 0 else 2) + (0 if load == "pm_even" else 1)
    assert ld % 2 == (0 if load == "pm_even" else 1)
    xb = torch.full((N, ld), float("nan"), dtype=torch.float64, device=dev)
    ab = torch.full((N, ld), 7, dtype=torch.int8, device=dev)
    xb[:, :T] = _t(dev, x)
    ab[:, :T - 1] = _t(dev, arm.astype(np.int8))
    return xb[:, :T], ab[:, :T - 1], "patient"


def _check_moments(got, mom, sc, what):
    got = got.cpu().numpy()
    assert got.shape == mom.shape and not np.isnan(got).any(), what
    ratio = M.worst_ratio(got, mom, sc)
    print(f"{what}: {ratio:.2e}")
    assert ratio <= M.GRAM_RTOL, (what, ratio)
    never = mom[:, :, 0] == 0
    assert np.array_equal(got[:, :, 0], mom[:, :, 0]) and not got[never].any(), (what, "a never-visited arm")


@pytest.mark.parametrize("load", LOADS)
@pytest.mark.parametrize("fd", M.SEG_FDS)
@pytest.mark.parametrize("n_arms", ARMS)
def test_moments(dev, n_arms, fd, load):
    """library_matrix.segment_inputs (N = 300, T = 23, seq_len 0, 1, 2, 3, T - 1, a switch at the last step, NaN past
    seq_len, changed arms from seq_len on): every entry within GRAM_RTOL of its scale, the counts exact, a
    never-visited arm exactly five zeros, no NaN."""
    import torch
    from insite_amd import ops
    x, _, arm, sl = SB.segment_inputs("std7", n_arms)
    assert {0, 1, 2, 3, x.shape[1] - 1} <= set(sl.tolist()) and np.isnan(x).any()
    mom, sc = SB.moments_case("std7", n_arms, fd)
    xd, ad, layout = _load(dev, x, arm, load)
    got = ops.segment_moments(xd, ad, _t(dev, sl.astype(np.int32)), M.DT, n_arms=n_arms, fd=fd, layout=layout)
    torch.cuda.synchronize()
    _check_moments(got, mom, sc, (n_arms, fd, load))


@pytest.mark.parametrize("N", [1, 65])
def test_moments_short_cohorts(dev, N):
    """One patient, and a second wave that holds one patient: every arm count, both fd, both layouts; seq_len beyond
    the stored steps is clamped and a negative one is 0."""
    import torch
    from insite_amd import ops
    for n_arms in ARMS:
        x, _, arm, sl = SB.segment_inputs("std7", n_arms)
        x, arm, sl = x[4:4 + N], arm[4:4 + N], sl[4:4 + N].copy()     # patient 4: seq_len T - 1, a switch at the end
        for fd in M.SEG_FDS:
            mom, sc = SB.moments(x, arm, sl, M.DT, n_arms, fd)
            for load in ("pm_odd", "tm"):
                xd, ad, layout = _load(dev, x, arm, load)
                got = ops.segment_moments(xd, ad, _t(dev, sl.astype(np.int32)), M.DT, n_arms=n_arms, fd=fd,
                                          layout=layout)
                _check_moments(got, mom, sc, (N, n_arms, fd, load))
        sl2 = sl.copy()
        sl2[0] = x.shape[1] + 5                                       # clamped to T - 1 = its own value
        if N > 1:
            sl2[1] = -3
        ref = SB.moments(x, arm, sl2, M.DT, n_arms, "order1")
        got = ops.segment_moments(_t(dev, x), _t(dev, arm.astype(np.int8)), _t(dev, sl2.astype(np.int32)), M.DT,
                                  n_arms=n_arms)
        _check_moments(got, *ref, (N, n_arms, "clamp"))
        if N > 1:
            assert not got[1].any()
    empty = ops.segment_moments(torch.zeros((0, 9), dtype=torch.float64, device=dev),
                                torch.zeros((0, 8), dtype=torch.int8, device=dev),
                                torch.zeros(0, dtype=torch.int32, device=dev), M.DT)
    assert tuple(empty.shape) == (0, 4, 5)


def test_moments_plan_and_determinism(dev):
    import torch
    from insite_amd import ops
    x, _, arm, sl = SB.segment_inputs("std7", 4)
    xd, ad, sd = _t(dev, x), _t(dev, arm.astype(np.int8)), _t(dev, sl.astype(np.int32))
    a = ops.segment_moments(xd, ad, sd, M.DT, fd="smoothed1")
    plan = ops.plan_segment_moments(xd, ad, sd, M.DT, fd="smoothed1")
    b = plan().clone()
    c = plan()
    torch.cuda.synchronize()
    assert W.same_bits(a, b) and W.same_bits(a, c)
    # the two layouts read the same numbers in the same order
    xt, at, _ = _load(dev, x, arm, "tm")
    assert W.same_bits(a, ops.segment_moments(xt, at, sd, M.DT, fd="smoothed1", layout="time"))


# ---------------------------------------------------------------------------------------------------
# Gram
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gram_inputs(name, N, n_arms):
    """(mom [N, A, 5], u [N, U]) straight from numpy, so every table runs."""
    exps = M.exps_of(name)
    rng = np.random.default_rng(M._seed("segboot", name, N, n_arms))
    out = (SB.numpy_moments(rng, N, n_arms), rng.uniform(0.6, 1.6, (N, exps.shape[1] - 1)))
    for a in out:
        a.setflags(write=False)
    return out


def _check(got, ref, what):
    """G | b of the device against (G, b, S_G, S_b) of the restatement, per entry scale."""
    for k, tag in ((0, "G"), (1, "b")):
        g = got[k].cpu().numpy()
        assert g.shape == ref[k].shape and np.all(np.isfinite(g)), (what, tag)
        ratio = M.worst_ratio(g, ref[k], ref[k + 2])
        print(f"{what} {tag}: {ratio:.2e}")
        assert ratio <= M.GRAM_RTOL, (what, tag, ratio)
    Gm = got[0].cpu().numpy()
    assert np.array_equal(Gm, np.swapaxes(Gm, -1, -2)), (what, "G is not symmetric")


def _case(dev, name, N, n_arms, Rn, off, seed=7):
    from insite_amd import ops
    mom, u = _gram_inputs(name, N, n_arms)
    got = ops.segboot_gram(_t(dev, mom), _t(dev, u), M.LIBS[name], Rn, seed=seed, patient_offset=off)
    ref = SB.gram(mom, u, M.exps_of(name), Rn, seed, off)
    _check(got, ref, (name, N, n_arms, Rn, off))
    return got, mom


@pytest.mark.parametrize("name", sorted(M.LIBS))
def test_gram_matches_reference_on_every_library(dev, name):
    """Every R with a rotating (N, n_arms, offset): the eight cases of a library cover every value of each."""
    li = sorted(M.LIBS).index(name)
    for i, Rn in enumerate(RS):
        _case(dev, name, NS[(i + li) % 5], ARMS[(i + li) % 4], Rn, OFFSETS[(i + 2 * li + i // 4) % 4])


@pytest.mark.parametrize("n_arms", ARMS)
def test_gram_std7_every_replicate_count(dev, n_arms):
    """std7 has 35 entries per arm: 3 column tiles (RT = 4), 5 (RT = 3), 7 in two chunks of 4 (RT = 4), 9 in two
    chunks of 5 (RT = 3, the EQ_5 shape); every R at N = 300, and every N and offset at the R past the tile edge.
    On this bias-first table G[r, a, 0, 0] is the weighted sample count, exact: sum_p w_rp count_pa with ONE weight
    per patient -- a weight drawn per (patient, arm) fails this."""
    for i, Rn in enumerate(RS):
        off = OFFSETS[i % 4]
        got, mom = _case(dev, "std7", 300, n_arms, Rn, off)
        w = BR.weights(7, Rn, 300, off).astype(np.float64)
        assert np.array_equal(got[0][:, :, 0, 0].cpu().numpy(), w @ mom[:, :, 0]), (n_arms, Rn)
    for N in NS:
        for off in OFFSETS:
            _case(dev, "std7", N, n_arms, 49 if n_arms in (2, 4) else 65, off)


@pytest.mark.parametrize("name,N,n_arms,Rn,off", [
    ("u3_first9", 300, 4, 100, 2),     # 216 columns: three column chunks
    ("bias_x", 20000, 4, 17, 1),       # more 8-patient groups than waves: two groups per wave
])
def test_gram_more_groups_than_one(dev, name, N, n_arms, Rn, off):
    _case(dev, name, N, n_arms, Rn, off)


@pytest.mark.parametrize("fd", M.SEG_FDS)
@pytest.mark.parametrize("n_arms", M.SEG_ARMS)
def test_replicate_zero_is_the_segment_gram(dev, n_arms, fd):
    """Moments on the device, then the Gram: replicate 0 is ops.gram_segments' G | b on the same inputs, at
    GRAM_RTOL of the literal's scale; the whole chain against the restatement too."""
    from insite_amd import ops
    lib = M.LIBS["std7"]
    x, u, arm, sl = M.segment_inputs("std7", n_arms)
    xd, ud = _t(dev, x), _t(dev, u)
    ad, sd = _t(dev, arm.astype(np.int8)), _t(dev, sl.astype(np.int32))
    G0, b0 = ops.gram_segments(xd, ad, sd, ud, M.DT, lib, n_arms=n_arms, fd=fd)
    mom = ops.segment_moments(xd, ad, sd, M.DT, n_arms=n_arms, fd=fd)
    whole = ops.segboot_gram(mom, ud, lib, 17, seed=5)
    _, _, SG, Sb = M.segment_case_ref("std7", n_arms, fd)
    for got, ref, scale, tag in ((whole[0][0], G0, SG, "G"), (whole[1][0], b0, Sb, "b")):
        ratio = M.worst_ratio(got.cpu().numpy(), ref.cpu().numpy(), scale)
        print(f"replicate 0 vs ops.gram_segments {tag}: {ratio:.2e}")
        assert ratio <= M.GRAM_RTOL, (tag, ratio)
    rm, rs = SB.moments_case("std7", n_arms, fd)
    _check(whole, SB.gram(rm, u, M.exps_of("std7"), 17, 5, scale_mom=rs), ("chain", n_arms, fd))


def test_shards_determinism_and_seed(dev):
    """Two shards with their offsets add up to the whole; two calls and a plan are bitwise equal; another seed keeps
    replicate 0 and changes the rest."""
    import torch
    from insite_amd import ops
    lib = M.LIBS["std7"]
    mom, u = _gram_inputs("std7", 300, 4)
    md, ud = _t(dev, mom), _t(dev, u)
    whole = ops.segboot_gram(md, ud, lib, 17, seed=5)
    ref = SB.gram(mom, u, M.exps_of("std7"), 17, 5)
    _check(whole, ref, "whole")
    for cut in (150, 149, 8, 299):
        lo = ops.segboot_gram(md[:cut].contiguous(), ud[:cut].contiguous(), lib, 17, seed=5)
        hi = ops.segboot_gram(md[cut:].contiguous(), ud[cut:].contiguous(), lib, 17, seed=5, patient_offset=cut)
        for k, tag in ((0, "G"), (1, "b")):
            ratio = M.worst_ratio((lo[k] + hi[k]).cpu().numpy(), whole[k].cpu().numpy(), ref[k + 2])
            assert ratio <= M.GRAM_RTOL, (cut, tag, ratio)
    again = ops.segboot_gram(md, ud, lib, 17, seed=5)
    third = ops.plan_segboot_gram(md, ud, lib, 17, seed=5)()
    torch.cuda.synchronize()
    for a, b, c in zip(whole, again, third):
        assert W.same_bits(a, b) and W.same_bits(a, c)
    other = ops.segboot_gram(md, ud, lib, 17, seed=6)
    assert torch.equal(other[0][0], whole[0][0]) and not torch.equal(other[0][1:], whole[0][1:])


def test_unvisited_arms_reach_nothing(dev):
    """NaN moments behind a count of 0 (and a NaN count) reach no output: a select, not a multiplication by zero.  An
    arm no patient visits is exactly zero in every replicate."""
    from insite_amd import ops
    mom, u = (a.copy() for a in _gram_inputs("std7", 65, 4))
    mom[:, 1] = 0.0                                # nobody visits arm 1
    never = mom[:, :, 0] == 0
    poisoned = mom.copy()
    poisoned[never, 1:] = np.nan
    poisoned[3, 1, 0] = np.nan                     # a NaN count is not > 0
    assert never[:, [0, 2, 3]].any() and not never[:, [0, 2, 3]].all()
    got = ops.segboot_gram(_t(dev, poisoned), _t(dev, u), M.LIBS["std7"], 17, seed=3)
    _check(got, SB.gram(mom, u, M.exps_of("std7"), 17, 3), "poisoned")
    assert not got[0][:, 1].any() and not got[1][:, 1].any() and bool(got[0][:, 0].any())


# ---------------------------------------------------------------------------------------------------
# the workspace contract (tests/workspace_matrix.py cannot gain a row: its export lists are pinned)
# ---------------------------------------------------------------------------------------------------
def test_workspace_contract(dev):
    """Too small: INSITE_E_WORKSPACE and untouched outputs; the 512-byte header is zero after a call; a body of NaN
    bytes (or of another pattern) before the call gives bitwise the same outputs and the guards stay clean;
    n_patients = 0 is a no-op."""
    import torch
    from insite_amd import _lib
    L = _lib.load()
    name, N, A, Rn = "std7", 300, 4, 50
    lib = M.LIBS[name]
    F = lib.n_terms
    mom, u = _gram_inputs(name, N, A)
    md, ud = _t(dev, mom), _t(dev, u)
    tab = lib.ctypes_table()
    need = L.insite_segboot_workspace_bytes(N, A, F, Rn)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def outs():
        return (W._full(dev, (Rn, A, F, F), torch.float64), W._full(dev, (Rn, A, F), torch.float64),
                W._full(dev, (Rn, A, F), torch.float64), W._full(dev, (Rn, A, F), torch.int8),
                W._full(dev, (Rn, A), torch.int32))

    def call(ws, nbytes, o, n=N, fit=False):
        head = (p(md), p(ud), 0, n, lib.n_statics, A, tab.ctypes.data_as(ctypes.c_void_p), F, Rn, 9)
        if fit:
            st = L.insite_segboot_fit_f64(*head, 0.1, 0.5, 100, 1, p(ws), nbytes, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                          p(o[4]), stream)
        else:
            st = L.insite_segboot_gram_f64(*head, p(ws), nbytes, p(o[0]), p(o[1]), stream)
        torch.cuda.synchronize()
        return st

    results = []
    for fit in (False, True):
        for pattern in W.PATTERNS:
            whole, view = W.make_guarded(need, "header512", pattern, dev)
            o = outs()
            assert call(view, need - 1, o, fit=fit) == -3 and call(view, 0, o, fit=fit) == -3
            assert W.untouched(o) and W.guards_clean(whole, need, pattern)
            assert bool((view[512:] == pattern).all()), "a refused call wrote scratch"
            assert call(view, need, o, n=0, fit=fit) == 0 and W.untouched(o)
            assert call(view, need, o, fit=fit) == 0
            assert W.header_zero(view, "header512") and W.guards_clean(whole, need, pattern)
            assert not W.untouched(o[:2])
            results.append(o if fit else o[:2])
    zero = torch.zeros(need, dtype=torch.uint8, device=dev)
    o = outs()
    assert call(zero, need, o) == 0
    for a, b, c in zip(o[:2], results[0], results[1]):
        assert W.same_bits(a, b) and W.same_bits(a, c)
    for a, b in zip(results[2], results[3]):
        assert W.same_bits(a, b)
    for a, b in zip(results[2][:2], o[:2]):
        assert W.same_bits(a, b)                   # the fit's G | b are the Gram call's
    _check(o[:2], SB.gram(mom, u, M.exps_of(name), Rn, 9), "workspace")


# ---------------------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------------------
def test_fit(dev):
    """oracle.segments_ref.synthetic_cohort (4 arms, noise-free, 300 patients, switches, ragged lengths), R = 33,
    moments and systems made on the device: every system's support is stlsq_gram's on the restated system and its
    coefficients agree to 1e-8; no system is excused.  Precondition (also tests/test_segboot_abi.py): no ridge iterate
    of any restated system lies within a relative 1e-3 of the threshold."""
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    x, u, arm, sl, exps, mom, Gr, br = SB.fit_case()
    Rn, thr, alpha = SB.FIT_R, SB.FIT_THRESHOLD, SB.FIT_ALPHA
    margin = min(SB.stlsq_margin(Gr[r, a], br[r, a], thr, alpha) for r in range(Rn) for a in range(4))
    assert margin > 1e-3, margin
    assert (np.diff(arm, axis=1) != 0).any() and len(set(sl.tolist())) > 1
    lib = polynomial_library(1, 2, True)
    assert np.array_equal(lib.exps.astype(np.int64), exps)
    md = ops.segment_moments(_t(dev, x), _t(dev, arm.astype(np.int8)), _t(dev, sl.astype(np.int32)), SB.FIT_DT)
    plan = ops.plan_sindy_bootstrap_segments(md, _t(dev, u), lib, Rn, thr, alpha=alpha, seed=SB.FIT_SEED)
    coef, mask, iters, Gd, bd = plan()
    torch.cuda.synchronize()
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    assert coef.shape == (Rn, 4, 4) and mask.shape == (Rn, 4, 4) and iters.shape == (Rn, 4)
    worst = 0.0
    for r in range(Rn):
        for a in range(4):
            c_ref, s_ref, _ = R.stlsq_gram(Gr[r, a], br[r, a], thr, alpha)
            assert np.array_equal(mask[r, a] != 0, s_ref), (r, a, mask[r, a], s_ref)
            worst = max(worst, float(np.abs(coef[r, a] - c_ref).max()))
    print(f"worst coefficient error {worst:.2e} (margin {margin:.2e})")
    assert worst < COEF_TOL and np.all(iters > 0)
    # the two-call composition gives the same bits
    G2, b2 = ops.segboot_gram(md, _t(dev, u), lib, Rn, seed=SB.FIT_SEED)
    c2 = ops.stlsq(G2.view(Rn * 4, 4, 4), b2.view(Rn * 4, 4), thr, alpha)[0]
    assert W.same_bits(G2, Gd) and np.array_equal(c2.cpu().numpy().reshape(Rn, 4, 4), coef)


# ---------------------------------------------------------------------------------------------------
# plugin
# ---------------------------------------------------------------------------------------------------
PLUGIN_R = 33


@functools.lru_cache(maxsize=None)
def _train():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return CS.make_collection(1, {"train": 200, "val": 20, "test": 10}, with_tests=False)["train"]


@pytest.fixture(scope="module")
def model(dev):
    from insite_amd import config as C
    from insite_amd.sindy import SINDY
    a = C.compose(["+backbone=sindy", "+dataset=pkpd_sim", "model.sindy_threshold=0.001", "model.sindy_alpha=0.5"])
    a["model"].update({"dataset_name": "cancer_sim", "dim_treatments": 4, "dim_static_features": 1, "dim_outcomes": 1})
    m = SINDY(a, device=dev).fit(_train())
    with pytest.raises(NotImplementedError, match="bootstrap_segments"):
        m.predict_bands(_train())
    m.bootstrap_segments(_train(), n_replicates=PLUGIN_R, seed=3)
    return m


def _worst(got, ref, scale):
    """max |got - ref| / scale over the entries (tests/test_gpu_effect.py's measure); a NaN on one side only, or an
    entry off where the scale is 0, is inf."""
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(got - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(scale, got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _stack(res):
    return np.concatenate([res.point.cpu().numpy()[:, None], res.mean.cpu().numpy()[:, None],
                           res.std.cpu().numpy()[:, None], res.quantiles.cpu().numpy()], axis=1)


def _plugin_inputs(model):
    from insite_amd.sindy import rhs_coefficients
    tr = _train()
    std, mean = float(tr.scaling_params["output_stds"]), float(tr.scaling_params["output_means"])
    prev, stat = R.unscale_inputs(tr.data, tr.scaling_params, 1, 1)
    arms = np.argmax(tr.data["current_treatments"], axis=-1)
    coef = np.stack([rhs_coefficients(c) for c in model.bootstrap_.coef.cpu().numpy()])
    return tr, std, mean, prev, stat, arms, coef, R.poly_library(2, 2, True)


def test_plugin_bootstrap_segments(dev, model):
    """Replicate 0 is the fitted model (1e-8, the support exactly), the summary is numpy's over the replicates
    1..R-1, the fitted model is not touched, and an arm without segments is refused as ``fit`` refuses it."""
    import copy
    tr = _train()
    res = model.bootstrap_
    assert model.bootstrap_mode_ == "segments" and res.n_replicates == PLUGIN_R and res.seed == 3
    coef, mask = res.coef.cpu().numpy(), res.mask.cpu().numpy()
    assert coef.shape == (PLUGIN_R, 4, 4) and np.all(np.isfinite(coef))
    err = float(np.abs(coef[0] - model.joint_coefs).max())
    print(f"point vs fitted {err:.2e}")
    assert err < COEF_TOL and np.array_equal(mask[0] != 0, model.coef_mask)
    assert np.array_equal(res.point.cpu().numpy(), coef[0])
    assert np.array_equal(res.inclusion.cpu().numpy(), (mask[1:] != 0).mean(0))
    np.testing.assert_allclose(res.mean.cpu().numpy(), coef[1:].mean(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(res.std.cpu().numpy(), coef[1:].std(0, ddof=1), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(res.quantiles.cpu().numpy(), np.quantile(coef[1:], list(res.q), axis=0), rtol=1e-12,
                               atol=1e-15)
    assert len({c.tobytes() for c in coef[1:]}) > 1
    m2 = copy.copy(model)
    fitted = model.joint_coefs.copy()
    data = dict(tr.data)
    ct = np.array(data["current_treatments"])
    ct[..., 0] += ct[..., 3]                       # arm 3 never given
    ct[..., 3] = 0
    data["current_treatments"] = ct
    with pytest.raises(ValueError, match=r"arm\(s\) \[3\]"):
        m2.bootstrap_segments(R.Subset("train", data, tr.scaling_params, None, tr.norm_const), n_replicates=5)
    assert np.array_equal(model.joint_coefs, fitted) and model.bootstrap_ is res


def test_plugin_bands_and_effect(dev, model):
    """``predict_bands`` and ``treatment_effect`` (plan B = arm 0 everywhere, plan A the cohort's own 4-arm plan)
    against tests/effect_ref.py at its bar, in standardised units."""
    tr, std, mean, prev, stat, arms, coef, exps = _plugin_inputs(model)
    q = (0.025, 0.5, 0.975)
    assert set(np.unique(arms)) == {0, 1, 2, 3}
    ref, scale = E.bands(prev[:, 0], stat, arms, np.zeros_like(arms), coef, exps, model.dt, q, "euler5")
    res = model.treatment_effect(tr, plan_b=0)
    assert res.series == ("a", "b", "effect")
    want = ref / std
    want[:2, [0, 1, 3, 4, 5]] = (ref[:2, [0, 1, 3, 4, 5]] - mean) / std
    w = _worst(_stack(res), want, scale / std)
    print(f"treatment_effect: worst |got - ref| / s = {w:.3e}")
    assert w <= BAND_TOL
    one = model.predict_bands(tr, quantiles=q)
    assert one.series == ("a",)
    w = _worst(_stack(one)[0], want[0], scale / std)
    print(f"predict_bands: {w:.3e}")
    assert w <= BAND_TOL
    band = model.predict_interval(tr, quantiles=(0.025, 0.975), max_rows=7)
    assert _worst(band.cpu().numpy(), want[0][[3, 5], :7], (scale / std)[:7]) <= BAND_TOL
    own = model._predict_device(tr).cpu().numpy()
    assert _worst(one.point[0].cpu().numpy(), own, scale / std) <= BAND_TOL


def test_plugin_choose_plan(dev, model):
    """``choose_plan`` over the four constant plans against tests/regimen_ref.py at its bar; the choice is compared
    on the rows whose margin in the restatement is at least 1e-8 s_p (a hundred times the bar, the input condition
    of tests/test_gpu_regimen.py)."""
    tr, std, mean, prev, stat, arms, coef, exps = _plugin_inputs(model)
    q = (0.025, 0.5, 0.975)
    N, T = arms.shape
    res = model.choose_plan(tr, [0, 1, 2, 3], objective="mean")
    plans = np.stack([np.full((N, T), j) for j in range(4)])
    ae = tr.data["active_entries"][..., 0].astype(np.float64)
    w = ae / ae.sum(axis=1, keepdims=True)
    ref = G.regimen(prev[:, 0], stat, plans, coef, exps, model.dt, q, w, None, 1, "euler5")
    clear = ref["margin"] >= 1e-8
    print(f"rows with a clear choice: {int(clear.sum())} of {N}; choices {np.bincount(ref['choice'], minlength=4)}")
    assert clear.sum() >= 0.9 * N
    assert np.array_equal(res.choice.cpu().numpy()[clear], ref["choice"][clear])
    o = ref["out"].transpose(2, 3, 0, 1)                          # [2, 3 + Q, N, K]
    want = o / std
    want[0, [0, 1, 3, 4, 5]] = (o[0, [0, 1, 3, 4, 5]] - mean * w.sum(axis=1)[None, :, None]) / std
    got = _stack(res)
    assert got.shape == want.shape == (2, 6, N, 4)
    # a row in a near tie may take the other plan in some replicate: its regret then differs, so the regret series
    # is compared on the clear rows; the value series on every row
    s = (ref["scale"] / std)[None, :, None]
    wv = _worst(got[0], want[0], s)
    wr = _worst(got[1][:, clear], want[1][:, clear], s[:, clear])
    print(f"choose_plan: value {wv:.3e} regret {wr:.3e}")
    assert wv <= BAND_TOL and wr <= BAND_TOL
    votes = np.stack([(ref["best"][1:] == j).mean(axis=0) for j in range(4)], axis=1)
    assert np.allclose(res.win.cpu().numpy()[clear], votes[clear], rtol=0, atol=1e-15)


def test_plugin_cohort_methods_run(dev, model):
    """``average_effect``, ``predict_average``, ``policy_value``, ``evaluate_rules`` and ``rule_value`` on the segment
    ensemble: finite results of the documented shapes."""
    import torch
    from insite_amd.effect import ThresholdRule as TR
    tr = _train()
    N, T = tr.data["current_treatments"].shape[:2]
    Q, K = 3, 4
    fin = lambda *ts: all(bool(torch.isfinite(t.double()).all()) for t in ts)   # noqa: E731
    ate = model.average_effect(tr, plan_b=0)
    assert ate.point.shape == (3, 1, T) and ate.quantiles.shape == (3, Q, 1, T)
    assert ate.weight_sum.shape == (PLUGIN_R, 1)
    assert fin(ate.point, ate.mean, ate.std, ate.quantiles, ate.weight_sum)
    avg = model.predict_average(tr, groups=np.arange(N) % 2)
    assert avg.point.shape == (1, 2, T) and fin(avg.point, avg.mean, avg.std, avg.quantiles)
    pv = model.policy_value(tr, [0, 1, 2, 3])
    S = len(pv.series)
    assert S == 2 * K + 6 and pv.point.shape == (S, 1) and pv.quantiles.shape == (S, Q, 1)
    assert pv.fixwin.shape == (1, K) and pv.rule.shape == (N,)
    assert fin(pv.point, pv.mean, pv.std, pv.quantiles, pv.fixwin)
    assert float(pv["gain_personalised"]["point"]) >= 0.0
    rules = [TR(0.0), TR(0.5, 0.2, arm_on=3), TR(-0.2, arm_on=2, arm_off=1, every=3)]
    fb = model.evaluate_rules(tr, rules)
    assert fb.choice.shape == (N,) and fb.win.shape == (N, 3) and fb.point.shape == (3, N, 3)
    assert fb.quantiles.shape == (3, Q, N, 3) and fin(fb.point, fb.mean, fb.std, fb.quantiles, fb.win)
    rv = model.rule_value(tr, rules)
    S = len(rv.series)
    assert S == 3 * 3 + 9 and rv.point.shape == (S, 1) and rv.quantiles.shape == (S, Q, 1)
    assert rv.fixwin.shape == (1, 3) and rv.assign.shape == (N,) and fin(rv.point, rv.mean, rv.std, rv.quantiles)
