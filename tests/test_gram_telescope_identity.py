"""The smoothed Gram's telescoped derivative moments, restated in numpy and checked against the oracle's row sums.

savgol(5,3) (symmetric) followed by FD4 (antisymmetric) is one 9-tap antisymmetric filter on the raw samples,
d_k = sum_{j=1..4} c_j (x_{k+j} - x_{k-j}), for the rows k = 4..L-5 whose stencils are all interior ones.  Over those
rows sum d_k and sum d_k x_k collapse to the eight samples at either end of the trajectory (the kernel's tele9_lo on
x[0..7] and tele9_hi on x[L-8..L-1]).  Here: the taps, and lo / hi against ``oracle.insite_ref.smoothed_fd4`` for
L = 8..40 (L = 8: no such row, neither term; L = 9: one row) on a smooth decay and on pure noise, where sum d x
cancels heavily -- agreement to 1e-12 relative to sum |d x|."""
import numpy as np
import pytest

from oracle import insite_ref as R


def composite_taps(dt):
    """c_1..c_4 from the weights the kernels hold (GramW: sg0..2, fd1..2 with 1/dt folded in)."""
    sg0, sg1, sg2 = R.SAVGOL_5_3[2][2], R.SAVGOL_5_3[2][3], R.SAVGOL_5_3[2][4]
    fd1, fd2 = R.FD4[2][3] / dt, R.FD4[2][4] / dt
    return np.array([fd1 * sg0 + fd2 * sg1 - fd1 * sg2, fd1 * sg1 + fd2 * sg0, fd1 * sg2 + fd2 * sg1, fd2 * sg2])


def tele9_end(c, v):
    """One end's bracket term from v = x[m-3 .. m+4] (m = L-5 for hi, m = 3 for lo): (sum d, sum d x) parts."""
    s1 = v[3] + v[4]
    s2 = s1 + (v[2] + v[5])
    s3 = s2 + (v[1] + v[6])
    s4 = s3 + (v[0] + v[7])
    sd = c[0] * s1 + c[1] * s2 + c[2] * s3 + c[3] * s4
    sdx = (c[0] * (v[3] * v[4]) + c[1] * (v[2] * v[4] + v[3] * v[5])
           + c[2] * (v[1] * v[4] + v[2] * v[5] + v[3] * v[6])
           + c[3] * (v[0] * v[4] + v[1] * v[5] + v[2] * v[6] + v[3] * v[7]))
    return sd, sdx


def telescoped_body(x, dt):
    L = x.shape[0]
    if L <= 8:
        return 0.0, 0.0
    c = composite_taps(dt)
    hi, lo = tele9_end(c, x[L - 8:]), tele9_end(c, x[:8])
    return hi[0] - lo[0], hi[1] - lo[1]


@pytest.mark.parametrize("dt", [1.0, 0.05, 10.0 / 60])
def test_composite_taps(dt):
    want = np.array([148.0, 79.0, -36.0, 3.0]) / (420.0 * dt)
    got = composite_taps(dt)
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-15
    assert abs(np.sum(2.0 * np.arange(1, 5) * got) * dt - 1.0) <= 1e-15     # exact on a ramp
    # and they are the convolution of FD4's interior row with savgol's
    conv = np.convolve(R.FD4[2], R.SAVGOL_5_3[2]) / dt                     # coefficient of x[k-4 .. k+4]
    np.testing.assert_allclose(conv[5:], got, rtol=1e-14)
    np.testing.assert_allclose(conv[:4][::-1], -got, rtol=1e-14)
    assert abs(conv[4]) <= 1e-16 / dt


@pytest.mark.parametrize("kind", ["decay", "noise"])
def test_telescoped_sums_match_oracle_rows(kind):
    rng = np.random.default_rng(11 if kind == "decay" else 12)
    dt = 10.0 / 60
    for L in range(8, 41):
        for _ in range(8):
            if kind == "decay":
                t = np.arange(L) * dt
                x = rng.uniform(0.2, 2.0) * np.exp(-rng.uniform(0.05, 0.8) * t) + 1e-3 * rng.standard_normal(L)
            else:
                x = rng.standard_normal(L)
            _, d = R.smoothed_fd4(x, dt)
            body = slice(4, L - 4)
            sd_ref, sdx_ref = np.sum(d[body]), np.sum(d[body] * x[body])
            sd, sdx = telescoped_body(x, dt)
            scale_d = np.sum(np.abs(d)) + np.max(np.abs(x)) / dt   # either end's term is of size |x| / dt
            assert abs(sdx - sdx_ref) <= 1e-12 * np.sum(np.abs(d * x)), (L, kind)
            assert abs(sd - sd_ref) <= 1e-12 * scale_d, (L, kind)
            # with the head and tail rows (positional stencils, untouched) the whole-trajectory moments follow
            edge = np.r_[0:4, L - 4:L]
            assert abs(np.sum(d[edge]) + sd - np.sum(d)) <= 1e-12 * scale_d
            assert abs(np.sum(d[edge] * x[edge]) + sdx - np.sum(d * x)) <= 1e-12 * np.sum(np.abs(d * x))
