"""The Gram kernels' telescoped derivative moments (gram_body) against the per-patient-loop oracle.

The body rows' sum x_dot and sum x_dot x reach the Gram only through one -lo term (the tile's first piece, from
x[0..7]) and one +hi term (the lane's tail piece, from x[L-8..L-1]); every row's x and x^2 are summed by the piece
that owns the row's step.  Each case below is a way that ownership could go wrong: lanes of one wave with different
row counts around every special length, pieces of a single 16-step group, mixed pieces, one wave's range crossing
several tiles (the fused / deferred steps with 1 and 3 gram blocks), every entry point, both layouts.

Tolerances are the existing parity tests': G and b rtol 1e-10 / atol 1e-8 against ``oracle.insite_ref.gram_moments``
(its per-patient ``rows``), support equal to the oracle's STLSQ; fused and deferred G|b bitwise equal for one split and
rtol 1e-12 / atol 1e-9 against the standalone fit (tests/test_gpu_fused.py); per-patient moments rtol 1e-12 /
atol 1e-9 (tests/test_gpu_moments.py)."""
import numpy as np
import pytest
import torch

from oracle import insite_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = [3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40]
_cache = {}


def _cohort(dev, N, T, seed, rows_kind):
    """Time-major cohort with ragged rows; cached with its numpy copies and oracle results."""
    key = (N, T, seed, rows_kind)
    if key in _cache:
        return _cache[key]
    from insite_amd import cohort
    coh = cohort.synthetic_pkpd(N, T, seed=seed, device=dev, equation="EQ_4_C", layout="time")
    rng = np.random.default_rng(seed)
    if rows_kind == "lengths":     # neighbouring lanes hold different lengths; every length present when N >= 19
        rows = np.array([LENGTHS[(3 * i + seed) % len(LENGTHS)] for i in range(N)], dtype=np.int32)
    else:                          # anything in [0, T], the tile edges and the special lengths forced in
        rows = rng.integers(0, T + 1, N).astype(np.int32)
        forced = [v for v in LENGTHS + [T, T - 1, T - 2, 47, 48, 49, 63, 64, 65] if v <= T]
        rows[rng.choice(N, len(forced), replace=False)] = forced
    coh.rows = torch.as_tensor(rows, device=dev)
    ent = {"coh": coh, "rows": rows, "x": coh.x[:, :N].t().contiguous().cpu().numpy(), "u": coh.u.cpu().numpy(),
           "arm": coh.arm.cpu().numpy().astype(np.int64), "exps": coh.lib.exps.astype(np.int64), "ref": {}}
    _cache[key] = ent
    return ent


def _oracle(ent, fd="smoothed4"):
    if fd not in ent["ref"]:
        G, b = R.gram_moments(ent["x"], ent["u"], ent["arm"], ent["rows"], ent["coh"].dt, ent["exps"], fd=fd)
        ent["ref"][fd] = (G, b, np.stack([R.stlsq_gram(G[a], b[a], 0.1, 0.5)[0] for a in range(2)]))
    return ent["ref"][fd]


def _oracle_moments(ent):
    if "mom" not in ent["ref"]:
        x, rows, dt = ent["x"], ent["rows"], ent["coh"].dt
        m = np.zeros((x.shape[0], 5))
        for i, L in enumerate(np.minimum(rows, x.shape[1])):
            if L < 5:
                continue
            xi = x[i, :L]
            _, d = R.smoothed_fd4(xi, dt)
            m[i] = (L, xi.sum(), (xi * xi).sum(), d.sum(), (d * xi).sum())
        ent["ref"]["mom"] = m
    return ent["ref"]["mom"]


def _check_gb(G, b, ref, what):
    for name, got, want in (("G", G, ref[0]), ("b", b, ref[1])):
        got = got.cpu().numpy()
        err = np.max(np.abs(got - want) / (1e-8 + 1e-10 * np.abs(want)))
        print(f"{what}: {name} worst |err| / (atol + rtol |ref|) = {err:.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-8, err_msg=f"{what}: {name}")


def _check_fit(out, ref, what):
    coef, mask, iters, G, b = out
    _check_gb(G, b, ref, what)
    assert np.array_equal(mask.cpu().numpy() != 0, ref[2] != 0), f"{what}: support"


def _patient_major(coh, N, T, ldx):
    xp = torch.zeros((N, ldx), dtype=torch.float64, device=coh.x.device)
    xp[:, :T] = coh.x[:, :N].t()
    return xp[:, :T]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_row_counts_in_one_wave(dev, N):
    """Lanes of one wave with L from LENGTHS (L < 5: nothing; 5..7: small_trajectory; 8: no body row, neither
    term; 9: a = b), standalone Gram and fit in the time-major and both patient-major (8- and 16-byte) instances,
    and the one-pass moments; every call twice, bitwise equal."""
    from insite_amd import ops
    T = 40
    ent = _cohort(dev, N, T, seed=3 + N, rows_kind="lengths")
    coh, ref = ent["coh"], _oracle(ent)
    calls = [("time", coh.x), ("patient", _patient_major(coh, N, T, T)), ("patient", _patient_major(coh, N, T, T + 1))]
    for layout, x in calls:
        what = f"N={N} {layout} ldx={x.stride(0)}"
        runs = [ops.sindy_fit(x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, 0.1, 0.5, layout=layout) for _ in range(2)]
        G, b = ops.gram(x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, layout=layout)
        torch.cuda.synchronize()
        _check_fit(runs[0], ref, "sindy_fit " + what)
        _check_gb(G, b, ref, "gram " + what)
        assert all(torch.equal(p, q) for p, q in zip(runs[0], runs[1])), what + ": not reproducible"
        moms = [ops.gram_moments(x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, 0.1, 0.5, layout=layout)
                for _ in range(2)]
        torch.cuda.synchronize()
        _check_fit(moms[0][:5], ref, "gram_moments " + what)
        np.testing.assert_allclose(moms[0][5].cpu().numpy(), _oracle_moments(ent), rtol=1e-12, atol=1e-9,
                                   err_msg="moments " + what)
        assert all(torch.equal(p, q) for p, q in zip(moms[0], moms[1])), what + ": moments not reproducible"


@pytest.mark.parametrize("N,T", [(130, 100), (6_400, 200)])
def test_piece_cuts_of_the_default_grid(dev, N, T):
    """The standalone time-major Gram at its default grid: 130 x 100 gives every wave a single 16-step group
    (interior pieces with no boundary term), 6,400 x 200 pieces of one and two groups."""
    from insite_amd import ops
    ent = _cohort(dev, N, T, seed=17, rows_kind="ragged")
    coh, ref = ent["coh"], _oracle(ent)
    runs = [ops.sindy_fit(coh.x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, 0.1, 0.5, layout="time") for _ in range(2)]
    mom = ops.gram_moments(coh.x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, 0.1, 0.5, layout="time")
    torch.cuda.synchronize()
    _check_fit(runs[0], ref, f"sindy_fit {N}x{T}")
    assert all(torch.equal(p, q) for p, q in zip(runs[0], runs[1]))
    _check_fit(mom[:5], ref, f"gram_moments {N}x{T}")
    np.testing.assert_allclose(mom[5].cpu().numpy(), _oracle_moments(ent), rtol=1e-12, atol=1e-9)
    # full-length rows too (no lane masked anywhere: the unmasked loop)
    full = _cohort(dev, N, T, seed=18, rows_kind="ragged")
    rows_full = torch.full_like(full["coh"].rows, T)
    G, b = ops.gram(full["coh"].x, full["coh"].u, full["coh"].arm, rows_full, full["coh"].dt, full["coh"].lib,
                    layout="time")
    torch.cuda.synchronize()
    Gr, br = R.gram_moments_vectorized(full["x"], full["u"], full["arm"], T, full["coh"].dt, full["exps"])
    _check_gb(G, b, (Gr, br), f"gram full rows {N}x{T}")


@pytest.mark.parametrize("gram_blocks", [1, 3])
def test_long_ranges_in_the_fused_and_deferred_steps(dev, gram_blocks):
    """One wave's range crosses several tiles (4 and 12 gram waves over 21 tiles x 7 groups): the fused step and
    the deferred step through both slots, against the oracle, bitwise equal to each other and run to run, and to
    rtol 1e-12 of the standalone fit."""
    from insite_amd import cohort, ops
    N, T = 1_300, 100
    ent = _cohort(dev, N, T, seed=29, rows_kind="ragged")
    coh, ref = ent["coh"], _oracle(ent)
    lib = coh.lib
    F = lib.n_terms
    rc = cohort.synthetic_pkpd(65, 33, seed=31, device=dev, equation="EQ_4_C", layout="time")
    bits = cohort.counterfactual_arms(rc.arm, 33, seed=32, layout="time_bits")
    cin = torch.zeros((2, F), dtype=torch.float64, device=dev)
    cin[0, 4], cin[1, 1], cin[1, 5] = -1.1107592869834308, -0.14540553723951796, -1.0234639833519243
    fused = [ops.fit_rollout(coh.x, coh.u, coh.arm, coh.rows, coh.dt, lib, 0.1, 0.5, rc.y0, rc.u, bits, cin, rc.dt,
                             method="rk4", gram_blocks=gram_blocks)[0] for _ in range(2)]
    torch.cuda.synchronize()
    _check_fit(fused[0], ref, f"fit_rollout gram_blocks={gram_blocks}")
    assert all(torch.equal(p, q) for p, q in zip(fused[0], fused[1]))
    ws = ops.Workspace()
    outs = [(torch.zeros((2, F), dtype=torch.float64, device=dev), torch.zeros((2, F), dtype=torch.int8, device=dev),
             torch.zeros((2,), dtype=torch.int32, device=dev), torch.zeros((2, F, F), dtype=torch.float64, device=dev),
             torch.zeros((2, F), dtype=torch.float64, device=dev)) for _ in range(2)]
    for k in range(3):   # call 1 finalises slot 0 into outs[0], call 2 slot 1 into outs[1]
        ops.fit_rollout_deferred(coh.x, coh.u, coh.arm, coh.rows, coh.dt, lib, 0.1, 0.5, rc.y0, rc.u, bits, cin,
                                 rc.dt, k % 2, k > 0, ws, method="rk4", T=33, out=outs[(k - 1) % 2],
                                 gram_blocks=gram_blocks)
    std = ops.sindy_fit(coh.x, coh.u, coh.arm, coh.rows, coh.dt, lib, 0.1, 0.5, layout="time")
    torch.cuda.synchronize()
    for slot in range(2):
        _check_fit(outs[slot], ref, f"fit_rollout_deferred slot {slot} gram_blocks={gram_blocks}")
        assert torch.equal(outs[slot][3], fused[0][3]) and torch.equal(outs[slot][4], fused[0][4])
        assert torch.equal(outs[slot][0], fused[0][0]) and torch.equal(outs[slot][1], fused[0][1])
    np.testing.assert_allclose(fused[0][3].cpu().numpy(), std[3].cpu().numpy(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(fused[0][4].cpu().numpy(), std[4].cpu().numpy(), rtol=1e-12, atol=1e-9)
    assert torch.equal(fused[0][1], std[1])


def test_unsmoothed_instance_unchanged(dev):
    """fd = order4 (the 5-tap form of the same telescoping): ragged rows against the oracle, both layouts."""
    from insite_amd import ops
    N, T = 1_300, 100
    ent = _cohort(dev, N, T, seed=29, rows_kind="ragged")
    coh, ref = ent["coh"], _oracle(ent, "order4")
    for layout, x in (("time", coh.x), ("patient", _patient_major(coh, N, T, T))):
        out = ops.sindy_fit(x, coh.u, coh.arm, coh.rows, coh.dt, coh.lib, 0.1, 0.5, fd="order4", layout=layout)
        torch.cuda.synchronize()
        _check_fit(out, ref, f"order4 {layout}")
