"""The step family -- insite_fit_rollout_f64 (step_kernel<SMOOTH, METHOD>), insite_fit_rollout_deferred_f64 and
insite_fit_rollout_lagged_f64 (step_deferred_kernel<SMOOTH, METHOD, DYN>) -- on the small edge shapes of
tests/step_matrix.py, against plain numpy references: both derivative kinds, rk4 / euler5 / euler with three
substeps, two 7-term libraries, the static and the claimed gram tail (ragged rows, a claimed tile without a usable
patient, a last piece of one group), trajectories of 5 .. 7 rows, row counts above n_steps, cohorts without a usable
patient, every bit layout of the rollout role (per-lane and wide last tile, tile-major), rollout ranges that start
mid-tile, padded outputs and the empty halves (n_rows = 0, n_patients = 0).

Every (discovery case, rollout case) pair of step_matrix.PAIRS runs through the three entry points:

* fused: one call, at the lower STLSQ threshold;
* deferred: call 0 streams the case into slot 0, call 1 streams the next case of the same library into slot 1 and
  finalises the first, call 2 (n_patients = 0, with a rollout) finalises the second; a fresh Workspace per stream;
* lagged: the same stream through plan_fit_rollout_lagged with red = (G, b); its solve role gets the reference G | b
  made symmetric.

Against the references first: per entry |G - G_ref| <= 1e-10 S_G and |b - b_ref| <= 1e-10 S_b; support, iteration count
and |coef - coef_ref| < 1e-8 for every case whose fit the reference decides (all but step_matrix.GB_ONLY, see
tests/test_step_matrix.py); y at rtol 1e-11 / atol 1e-12; the padding of y and the outputs of a call that does not
finalise keep their fill values.  Then the equalities insite_hip.h promises, bitwise: y across the entry points, the
bit layouts and ops.rollout; deferred G | b and the fused ones for an explicit gram_blocks on the static path; lagged
red and deferred G | b; two independent claimed streams.

Which instantiation a launch took is read from the slot header it wrote (words kSlotRec + 1 = the gram blocks after
the planner's clamps, kDynRecP = the claimed pieces, 0 for a static launch, kDynRecDone = the pieces processed),
through the Workspace buffer: the claimed-tail predicate of step_matrix is evaluated with the recorded block count and
must agree with both the case list and the recorded piece count.

Measured worst |error| / scale on an MI355X (G, b): fused 1.7e-15, 1.3e-15; deferred static 1.7e-15, 9.5e-16; deferred
claimed 1.8e-15, 1.2e-15; lagged 1.8e-15, 1.2e-15.  The 192 tests take about 2 s (4 s with the imports); run with -s to
print these figures and the wall time."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import library_matrix as M  # noqa: E402
import step_matrix as SM  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}   # family -> worst |error| / scale seen
Y_FILL = -777.25
OUT_FILL = (7.25, 3, -77, 7.25, 7.25)   # coef, mask, iters, G, b of a call that must not write them
SLOT_MAGIC = 0x1E5D0A7E
BITWISE_GB = (1, 2, 7)   # explicit gram_blocks below any grid: the fused and the deferred launch cut the same blocks


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for fam in sorted(WORST):
        print(f"\n[step-matrix] worst error / scale, {fam}: {WORST[fam]:.3e}", end="")
    print(f"\n[step-matrix] wall time of the file: {time.perf_counter() - t0:.1f} s")


def _t(a, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    if not a.size:   # (an empty array converts to a tensor with zero strides, which the wrappers refuse)
        return torch.zeros(a.shape, device=dev, dtype=dtype or torch.float64)
    return torch.tensor(a, device=dev, dtype=dtype)


def _outs(dev, fill=None):
    import torch
    f = fill or (0, 0, 0, 0, 0)
    return (torch.full((2, 7), f[0], dtype=torch.float64, device=dev),
            torch.full((2, 7), f[1], dtype=torch.int8, device=dev),
            torch.full((2,), f[2], dtype=torch.int32, device=dev),
            torch.full((2, 7, 7), f[3], dtype=torch.float64, device=dev),
            torch.full((2, 7), f[4], dtype=torch.float64, device=dev))


def _untouched(outs, fill):
    return all(bool((t == v).all()) for t, v in zip(outs, fill))


# ---------------------------------------------------------------------------------------------------
# device inputs, cached per case
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _disc_dev(dev, lib, N, T, pattern):
    """(x [T, N] view of a [T, N + 5] buffer with NaN padding, u, arm, rows)."""
    import torch
    x, u, arm, rows = SM._cohort(lib, N, T, pattern)
    buf = torch.full((T, N + 5), float("nan"), dtype=torch.float64, device=dev)
    buf[:, :N] = _t(x.T, dev)
    return buf, _t(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32)


def _disc_args(dev, name, empty=False):
    c = SM.DISC[name]
    x, u, arm, rows = _disc_dev(dev, c.lib, c.N, c.T, c.pattern)
    return (x[:, :0], u[:0], arm[:0], rows[:0]) if empty else (x, u, arm, rows)


@functools.lru_cache(maxsize=None)
def _roll_dev(dev, rname, lib):
    """y0, u, coef and the arm bits in the three layouts: {"tm", "tm_even", "tile"} -> tensor."""
    import torch
    from insite_amd import ops
    c = SM.ROLL[rname]
    y0, u, arm, coef = SM.roll_inputs(rname, lib)
    W = SM.ceil_div(c.Nr, 32)
    if c.Nr:
        tm = ops.pack_arm_bits(_t(arm.T, dev, torch.int8), c.Nr)
        assert tuple(tm.shape) == (c.Tr, W) and tm.stride(0) == W
        ldp = W + 1 if W % 2 else W + 2
        even = torch.full((c.Tr, ldp), 0x5A5A5A5A, dtype=torch.int32, device=dev)   # garbage in the padding words
        even[:, :W] = tm
        tile = ops.tile_major_bits(tm, c.Nr)
    else:
        tm = even = tile = torch.zeros((c.Tr, 1), dtype=torch.int32, device=dev)
    return _t(y0, dev), _t(u, dev), _t(coef, dev), {"tm": tm, "tm_even": even, "tile": tile}


def _roll_args(dev, rname, lib, alt=False):
    """(y0, ru, bits, coef_in, keyword arguments) with the case's bit layout, or -- alt -- the other family's
    (tile-major for a time-major case and the other way round)."""
    c = SM.ROLL[rname]
    y0, u, coef, bits = _roll_dev(dev, rname, lib)
    lay = c.bits if not alt else ("tm" if c.bits == "tile" else "tile")
    meth, sub = SM.METHODS[c.method]
    return y0, u, bits[lay], coef, dict(method=meth, substeps=sub, drop_below=SM.DROP_BELOW, T=c.Tr)


def _ybuf(dev, rname):
    """The output two rows taller than Tr and five columns wider than Nr; the call gets the [Tr, Nr + 5] view."""
    import torch
    c = SM.ROLL[rname]
    buf = torch.full((c.Tr + 2, c.Nr + 5), Y_FILL, dtype=torch.float64, device=dev)
    return buf, buf[:c.Tr]


@functools.lru_cache(maxsize=None)
def _rollout_baseline(dev, rname, lib):
    from insite_amd import ops
    c = SM.ROLL[rname]
    y0, u, coef, bits = _roll_dev(dev, rname, lib)
    meth, sub = SM.METHODS[c.method]
    return ops.rollout(y0, u, bits["tm"], coef, SM.LIBS[lib], SM.ROLLOUT_DT, method=meth, substeps=sub,
                       drop_below=SM.DROP_BELOW, T=c.Tr, layout="time_bits")


def _header(ws, slot, dev):
    """The 128 words of a slot's header."""
    from insite_amd import _lib
    import torch
    one = _lib.load().insite_gram_workspace_bytes(1, 2, 7)
    buf = next(iter(ws._buf.values()))
    off = SM.DEF_AREA_BYTES + slot * one
    return buf[off:off + 512].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------
# the three entry points, each run once per pair
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused(dev, d, r):
    from insite_amd import ops
    c = SM.DISC[d]
    y0, ru, bits, cin, kw = _roll_args(dev, r, c.lib)
    buf, yv = _ybuf(dev, r)
    out = _outs(dev, OUT_FILL)
    ops.fit_rollout(*_disc_args(dev, d), SM.DT, SM.LIBS[c.lib], SM.THRESHOLD_LOW, SM.ALPHA, y0, ru, bits, cin,
                    SM.ROLLOUT_DT, fd=c.fd, out=out, y_out=yv, gram_blocks=c.gram_blocks, **kw)
    return out, buf


def _stream_calls(d):
    """(streamed case or None, the case whose shapes the call takes, slot, finalises) of the three calls."""
    nxt = SM.next_in_stream(d)
    return [(d, d, 0, False), (nxt, nxt, 1, True), (None, d, 0, True)]


def _deferred_stream(dev, d, r, calls=3):
    from insite_amd import ops
    c = SM.DISC[d]
    lib = SM.LIBS[c.lib]
    ws = ops.Workspace()
    outs = [_outs(dev, OUT_FILL) for _ in range(3)]
    thresholds = (SM.THRESHOLD, SM.THRESHOLD, SM.THRESHOLD_LOW)
    ys, hdrs = [], []
    for k, (streamed, shape, slot, fin) in enumerate(_stream_calls(d)[:calls]):
        s = SM.DISC[shape]
        y0, ru, bits, cin, kw = _roll_args(dev, r, c.lib, alt=k == 1)
        buf, yv = _ybuf(dev, r)
        ops.fit_rollout_deferred(*_disc_args(dev, shape, empty=streamed is None), SM.DT, lib, thresholds[k], SM.ALPHA,
                                 y0, ru, bits, cin, SM.ROLLOUT_DT, slot, fin, ws, fd=s.fd, out=outs[k], y_out=yv,
                                 gram_blocks=s.gram_blocks, **kw)
        ys.append(buf)
        hdrs.append(_header(ws, slot, dev))
    return outs, ys, hdrs


@functools.lru_cache(maxsize=None)
def _deferred(dev, d, r):
    return _deferred_stream(dev, d, r)


def _sym(G):
    return np.ascontiguousarray(np.tril(G) + np.transpose(np.tril(G, -1), (0, 2, 1)))


@functools.lru_cache(maxsize=None)
def _lagged(dev, d, r):
    import torch
    from insite_amd import ops
    c = SM.DISC[d]
    lib = SM.LIBS[c.lib]
    ws = ops.Workspace()
    reds = [(torch.full((2, 7, 7), OUT_FILL[3], dtype=torch.float64, device=dev),
             torch.full((2, 7), OUT_FILL[4], dtype=torch.float64, device=dev)) for _ in range(3)]
    fits = [_outs(dev, OUT_FILL)[:3] for _ in range(3)]
    thresholds = (SM.THRESHOLD, SM.THRESHOLD_LOW, SM.THRESHOLD)
    calls = _stream_calls(d)
    ys, hdrs = [], []
    for k, (streamed, shape, slot, fin) in enumerate(calls):
        s = SM.DISC[shape]
        y0, ru, bits, cin, kw = _roll_args(dev, r, c.lib, alt=k == 1)
        buf, yv = _ybuf(dev, r)
        fit_in = None
        if k > 0:   # the solve role: the reference G | b of the cohort this call reduces
            Gr, br = SM.disc_ref(calls[k - 1][0])[:2]
            fit_in = (_t(_sym(Gr), dev), _t(br, dev))
        ops.plan_fit_rollout_lagged(*_disc_args(dev, shape, empty=streamed is None), SM.DT, lib, thresholds[k],
                                    SM.ALPHA, y0, ru, bits, cin, SM.ROLLOUT_DT, slot, fin, ws, reds[k], fit_in=fit_in,
                                    fit_out=fits[k], fd=s.fd, y_out=yv, gram_blocks=s.gram_blocks, **kw)()
        ys.append(buf)
        hdrs.append(_header(ws, slot, dev))
    return reds, fits, ys, hdrs


# ---------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------
def _check_gram(family, G, b, name, what):
    Gr, br, SG, Sb = SM.disc_ref(name)
    for tag, got, ref, scale in (("G", G, Gr, SG), ("b", b, br, Sb)):
        got = got.cpu().numpy()
        assert np.all(np.isfinite(got)), (family, tag, what)
        ratio = M.worst_ratio(got, ref, scale)
        key = f"{family} {tag}"
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        print(f"{key} {what}: worst |error| / scale {ratio:.3e}")
        assert ratio <= SM.GRAM_RTOL, (family, tag, what, ratio)
    G = G.cpu().numpy()
    assert np.array_equal(G, np.transpose(G, (0, 2, 1))), (family, what)


def _check_fit(coef, mask, iters, G_ref, b_ref, name, threshold, what):
    """Support, iteration count and coefficients against oracle.insite_ref.stlsq_gram on the reference G | b."""
    if not SM.asserts_fit(name, threshold):
        return
    cr, sr, ir = SM.fit_ref(G_ref, b_ref, threshold)
    coef, mask, iters = coef.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()
    assert np.array_equal(mask != 0, sr), (what, mask, sr)
    assert set(np.unique(mask).tolist()) <= {0, 1}
    assert np.array_equal(iters, ir), (what, iters, ir)
    err = float(np.max(np.abs(coef - cr)))
    print(f"{what} thr {threshold}: coefficient L-inf {err:.3e}")
    assert err < SM.COEF_ATOL, (what, err)


def _check_y(buf, r, lib, what):
    c = SM.ROLL[r]
    got = buf.cpu().numpy()
    assert np.all(got[c.Tr:] == Y_FILL) and np.all(got[:, c.Nr:] == Y_FILL), (what, "padding written")
    if not c.Nr:
        return
    y, ref = got[:c.Tr, :c.Nr].T, SM.roll_ref(r, lib)
    assert np.all(np.isfinite(y)), what
    print(f"{what}: rollout worst relative error "
          f"{float(np.max(np.abs(y - ref) / np.maximum(np.abs(ref), 1e-300))):.3e}")
    np.testing.assert_allclose(y, ref, rtol=SM.Y_RTOL, atol=SM.Y_ATOL, err_msg=what)


def _check_header(hdr, name, what):
    """The launch that streamed ``name`` took the instantiation the case list says."""
    c = SM.DISC[name]
    assert hdr[SM.SLOT_REC] == SLOT_MAGIC, what
    gb, P, done = int(hdr[SM.SLOT_REC + 1]), int(hdr[SM.DYN_REC_P]), int(hdr[SM.DYN_REC_DONE])
    assert 1 <= gb <= SM.GRAM_MAX_BLOCKS
    if c.gram_blocks in BITWISE_GB:
        assert gb == c.gram_blocks, (what, gb)
    elif c.gram_blocks == SM.GB_OVER:
        assert gb >= 64, (what, gb)     # the grid less two
    claimed = SM.claimed_tail(c.N, c.T, gb)
    assert claimed is (c.path == "claimed"), (what, gb)
    if claimed:
        assert P == done == SM.tail_geometry(c.N, c.T)[2] > 0, (what, P, done)
    else:
        assert P == 0, (what, P)


def _family(name):
    return "deferred " + SM.DISC[name].path


IDS = [f"{d}-{r}" for d, r in SM.PAIRS]


@pytest.mark.parametrize("d,r", SM.PAIRS, ids=IDS)
def test_fused(dev, d, r):
    (coef, mask, iters, G, b), ybuf = _fused(dev, d, r)
    _check_gram("fused", G, b, d, f"{d}-{r}")
    Gr, br = SM.disc_ref(d)[:2]
    _check_fit(coef, mask, iters, Gr, br, d, SM.THRESHOLD_LOW, f"fused {d}")
    _check_y(ybuf, r, SM.DISC[d].lib, f"fused {d}-{r}")


@pytest.mark.parametrize("d,r", SM.PAIRS, ids=IDS)
def test_deferred_stream(dev, d, r):
    outs, ys, hdrs = _deferred(dev, d, r)
    nxt = SM.next_in_stream(d)
    assert _untouched(outs[0], OUT_FILL), "call 0 does not finalise: its outputs must keep their fill"
    for k, name, thr in ((1, d, SM.THRESHOLD), (2, nxt, SM.THRESHOLD_LOW)):
        coef, mask, iters, G, b = outs[k]
        _check_gram(_family(name), G, b, name, f"{name} (stream of {d})")
        Gr, br = SM.disc_ref(name)[:2]
        _check_fit(coef, mask, iters, Gr, br, name, thr, f"deferred {name}")
    for k in range(3):
        _check_y(ys[k], r, SM.DISC[d].lib, f"deferred call {k} {d}-{r}")
    _check_header(hdrs[0], d, f"call 0 {d}")
    _check_header(hdrs[1], nxt, f"call 1 {nxt}")
    assert hdrs[2][SM.SLOT_REC] == SLOT_MAGIC and hdrs[2][SM.DYN_REC_P] == 0    # the flush streams nothing: static


@pytest.mark.parametrize("d,r", SM.PAIRS, ids=IDS)
def test_lagged_stream(dev, d, r):
    reds, fits, ys, hdrs = _lagged(dev, d, r)
    nxt = SM.next_in_stream(d)
    assert _untouched(reds[0], OUT_FILL[3:]) and _untouched(fits[0], OUT_FILL[:3]), "call 0 neither reduces nor solves"
    for k, name, thr in ((1, d, SM.THRESHOLD_LOW), (2, nxt, SM.THRESHOLD)):
        _check_gram("lagged", reds[k][0], reds[k][1], name, f"{name} (stream of {d})")
        Gr, br = SM.disc_ref(name)[:2]
        _check_fit(*fits[k], Gr, br, name, thr, f"lagged solve {name}")
    for k in range(3):
        _check_y(ys[k], r, SM.DISC[d].lib, f"lagged call {k} {d}-{r}")
    _check_header(hdrs[0], d, f"call 0 {d}")
    _check_header(hdrs[1], nxt, f"call 1 {nxt}")


@pytest.mark.parametrize("d,r", SM.PAIRS, ids=IDS)
def test_entry_points_agree_bitwise(dev, d, r):
    import torch
    c, q = SM.DISC[d], SM.ROLL[r]
    nxt = SM.next_in_stream(d)
    fo, fy = _fused(dev, d, r)
    do, dys, _ = _deferred(dev, d, r)
    lr, lf, lys, _ = _lagged(dev, d, r)
    # y: every call of every entry point (call 1 of the streams reads the other bit layout) and ops.rollout
    if q.Nr:
        base = _rollout_baseline(dev, r, c.lib)
        assert torch.equal(fy[:q.Tr, :q.Nr], base), "fused y differs from insite_rollout_f64"
    for k in range(3):
        assert torch.equal(dys[k], fy), f"deferred call {k}: y differs from the fused call's"
        assert torch.equal(lys[k], fy), f"lagged call {k}: y differs from the fused call's"
    # deferred G | b == fused G | b: the same blocks, the same order of the partials
    if c.path == "static" and c.gram_blocks in BITWISE_GB:
        assert torch.equal(do[1][3], fo[3]) and torch.equal(do[1][4], fo[4]), "deferred G|b differ from the fused ones"
    # lagged red == deferred G | b, claimed launches included
    for k in (1, 2):
        assert torch.equal(lr[k][0], do[k][3]) and torch.equal(lr[k][1], do[k][4]), \
            f"call {k}: lagged red differs from the deferred G|b"
    # two independent claimed streams
    if "claimed" in (c.path, SM.DISC[nxt].path):
        again, _, _ = _deferred_stream(dev, d, r)
        for k in (1, 2):
            for a, b in zip(again[k], do[k]):
                assert torch.equal(a, b), f"call {k}: two claimed streams differ"
