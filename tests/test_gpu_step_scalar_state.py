"""The deferred step on the smallest shapes at which the rollout role's step-mask ring and its per-chunk address and
descriptor updates can go wrong (csrc/insite_hip.hip, rollout_bits_range: one ring of kTG = 16 masks refilled in halves
of 8, clamped at the range's last step; an integrate-only loop before the stored one; rollout_units: the wave's
coefficient rows and column codes kept across its ranges).

Every case streams one cohort through ops.fit_rollout_deferred three times, as the bench does:

* call 0 streams the cohort into slot 0 and rolls it out with a fixed random model;
* call 1 streams it into slot 1, finalises slot 0 and rolls out with a second fixed model;
* call 2 finalises slot 1 and rolls out with the model call 1 finalised.

Both finalisations are compared with ops.sindy_fit on the same cohort -- G | b | coef | mask | iters -- and the three y
with ops.rollout(layout="time_bits") on the time-major bits under the same coefficients.  Every comparison is bitwise
(on the 64-bit patterns): include/insite_hip.h promises y_out bitwise, and G | b | coef as insite_sindy_fit_f64 with
the same block count, so the deferred calls are given the block count the standalone time-major gram takes for the
cohort (gram_blocks_of below restates launch_gram4's range mode).

Shapes: T in 5 .. 200 around the half ring (8), the chunk (16) and the 32-step arm group, with T not a multiple of 8
for the refills past the range's last step; N around one and two 64-patient tiles (N = 1, 32, 65, 130 in time-major
bits leave a last tile of <= 32 patients, which takes the per-lane form beside the scalar-mask tiles); time-major bits
and tile-major bits with more rows per tile than steps; ragged row counts (tests/library_matrix.cohort).  The last
cases give the gram every block but one, so that the four waves of one rollout block walk all the (tile, arm group)
ranges, most of them starting mid-trajectory; their discovery cohort is a single (tile, 16-step) unit, for which the
block partials are zero but one and the fixed-order sum does not depend on the block count."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
import step_matrix as SM  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = "std7"
T_CASES = (5, 8, 9, 15, 16, 17, 24, 31, 32, 33, 48, 49, 200)
N_CASES = (1, 32, 33, 64, 65, 130)
LAYOUTS = ("time_bits", "tile_bits")
TILE_PAD = 3          # rows per tile beyond T in the tile-major layout (S = T + 3 > T)
ONE_BLOCK = [(130, 200, lay) for lay in LAYOUTS] + [(65, 49, "time_bits"), (130, 33, "tile_bits")]
ONE_UNIT = (33, 16)   # the discovery cohort of the one-rollout-block cases: one tile, one 16-step group


def gram_blocks_of(N, T):
    """Blocks of the standalone time-major gram (launch_gram4, range mode) for cohorts far below a resident round."""
    units = SM.ceil_div(N, SM.WAVE) * SM.ceil_div(T, SM.GT)
    return max(1, SM.ceil_div(units, SM.WAVES_PER_BLOCK))


def _bits(t):
    """The 64-bit patterns of a float64 tensor (NaN compares equal to itself)."""
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _cohort(dev, N, T):
    """Device inputs of one cohort: x [T, N] time-major (NaN past rows), u, arm, rows; for its rollout y0 ~ U(0.5, 3)
    and random per-step arms as time-major bits and as tile-major bits with T + TILE_PAD rows a tile (garbage in the
    padding rows)."""
    import torch
    from insite_amd import ops
    lib = SM.LIBS[LIB]
    x, u, arm, rows = M.cohort(N, T, lib.n_statics, M._seed("scalar-state", N, T), 2)
    rng = np.random.default_rng(M._seed("scalar-state-roll", N, T))
    y0 = rng.uniform(0.5, 3.0, N)
    steps = rng.integers(0, 2, (T, N)).astype(np.int8)
    xt = torch.tensor(np.ascontiguousarray(x.T), device=dev)
    tm = ops.pack_arm_bits(torch.tensor(steps, device=dev), N)
    tile = ops.tile_major_bits(tm, N)
    padded = torch.full((tile.size(0), T + TILE_PAD, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    padded[:, :T] = tile
    return dict(x=xt, u=torch.tensor(u, device=dev), arm=torch.tensor(arm, dtype=torch.int8, device=dev),
                rows=torch.tensor(rows, dtype=torch.int32, device=dev), y0=torch.tensor(y0, device=dev),
                time_bits=tm, tile_bits=padded)


@functools.lru_cache(maxsize=None)
def _models(dev):
    """Two fixed models whose arms differ in every term, so that a wrong step mask moves y."""
    import torch
    rng = np.random.default_rng(M._seed("scalar-state-coef"))
    out = []
    for _ in range(2):
        c = rng.uniform(0.05, 0.15, (2, 7)) * rng.choice([-1.0, 1.0], (2, 7))
        c[1, 6] = 0.5 * SM.DROP_BELOW
        out.append(torch.tensor(c, device=dev))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _fit_ref(dev, N, T):
    from insite_amd import ops
    c = _cohort(dev, N, T)
    return ops.sindy_fit(c["x"], c["u"], c["arm"], c["rows"], SM.DT, SM.LIBS[LIB], SM.THRESHOLD, SM.ALPHA,
                         layout="time")


def _roll_ref(dev, N, T, coef):
    from insite_amd import ops
    c = _cohort(dev, N, T)
    return ops.rollout(c["y0"], c["u"], c["time_bits"], coef, SM.LIBS[LIB], SM.ROLLOUT_DT, method="rk4",
                       drop_below=SM.DROP_BELOW, T=T, layout="time_bits")


@functools.lru_cache(maxsize=None)
def _roll_ref_fixed(dev, N, T, k):
    return _roll_ref(dev, N, T, _models(dev)[k])


def _outs(dev):
    import torch
    return (torch.full((2, 7), 7.25, dtype=torch.float64, device=dev),
            torch.full((2, 7), 3, dtype=torch.int8, device=dev),
            torch.full((2,), -77, dtype=torch.int32, device=dev),
            torch.full((2, 7, 7), 7.25, dtype=torch.float64, device=dev),
            torch.full((2, 7), 7.25, dtype=torch.float64, device=dev))


def _stream(dev, disc, roll, layout, gram_blocks):
    """Three deferred launches: ``disc`` = (N, T) of the streamed cohort, ``roll`` = (N, T) of the rolled-out one.
    Returns the two finalisations and the three (y, coefficients it was rolled out with)."""
    import torch
    from insite_amd import ops
    d, r = _cohort(dev, *disc), _cohort(dev, *roll)
    Nr, Tr = roll
    ws = ops.Workspace()
    outs = [_outs(dev) for _ in range(3)]
    fixed = _models(dev)
    ys = []
    for k in range(3):
        cin = fixed[k] if k < 2 else outs[1][0]
        y = torch.full((Tr, Nr), -777.25, dtype=torch.float64, device=dev)
        ops.fit_rollout_deferred(d["x"], d["u"], d["arm"], d["rows"], SM.DT, SM.LIBS[LIB], SM.THRESHOLD, SM.ALPHA,
                                 r["y0"], r["u"], r[layout], cin, SM.ROLLOUT_DT, k % 2, k > 0, ws, method="rk4",
                                 drop_below=SM.DROP_BELOW, T=Tr, out=outs[k], y_out=y, gram_blocks=gram_blocks)
        ys.append((y, cin))
    return outs[1:], ys


def _check(dev, disc, roll, layout, gram_blocks):
    fins, ys = _stream(dev, disc, roll, layout, gram_blocks)
    ref = _fit_ref(dev, *disc)
    for k, fin in enumerate(fins):
        for name, got, want in zip(("coef", "mask", "iters", "G", "b"), fin, ref):
            assert _same(got, want), f"finalisation {k + 1}: {name} differs from sindy_fit"
    for k, (y, cin) in enumerate(ys):
        want = _roll_ref_fixed(dev, *roll, k) if k < 2 else _roll_ref(dev, *roll, cin)
        assert _same(y, want), f"call {k}: y differs from the standalone time-major rollout"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", N_CASES)
@pytest.mark.parametrize("T", T_CASES)
def test_deferred_step_small_shapes_bitwise(dev, T, N, layout):
    _check(dev, (N, T), (N, T), layout, gram_blocks_of(N, T))


@pytest.mark.parametrize("N,T,layout", ONE_BLOCK)
def test_one_rollout_block_walks_every_range_bitwise(dev, N, T, layout):
    _check(dev, ONE_UNIT, (N, T), layout, SM.GB_OVER)
