"""The workspace contract of every entry point that takes a caller-owned workspace, on the rows and shape cases of
tests/workspace_matrix.py (its docstring derives the cases and states the contract, W1 .. W5).

Per row and case, in one process and with few launches:

1. anchor: the call on a fresh, generous torch.zeros workspace; the outputs match the row's oracle at the tolerance
   that operation's own GPU test uses (the only tolerance in this file);
2. W1 / W2: the same call on an exact-size view between two 4 KiB guards, everything filled with 0xFF and then with
   0x5A except the header the contract requires to be zero: the outputs equal the anchor's bit for bit, both guards
   keep their pattern, and the wrapper asked for no more than the query (the injected view is still the workspace's
   buffer);
3. W3: after every call the contract's header is zero.

Per row, on one guarded buffer sized for the largest query of the sequence (never re-zeroed between the calls):

4. W4: largest, smallest, no-op, too-few-rows, smallest, largest: every output equals that case's anchor bit for
   bit; a no-op that the header documents as one leaves the poison the outputs held;
5. W5: the last call once more: the same bits.

The view goes in through the public path, an ops.Workspace whose buffer for the device is preset, so the size each
wrapper computes is exercised too (insite_rk45_order_i32, whose wrapper takes no workspace, is called through _lib).
Nothing is ever put where a contract requires zero, and every write that could go astray lands in the test's own
allocation.  Run with -s to print every anchor's error against its oracle and the wall time."""
import functools
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_matrix as W  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}   # row -> worst (error / bar) of its anchors


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    for name in (r.name for r in W.ROWS if r.name in WORST):
        print(f"\n[workspace-matrix] {name}: anchors' worst error / bar {WORST[name]:.3e} "
              f"({W.BY_NAME[name].tolerance})", end="")
    print(f"\n[workspace-matrix] wall time of the file: {time.perf_counter() - t0:.1f} s")


def _workspace(buf, dev):
    from insite_amd import ops
    ws = ops.Workspace()
    ws._buf[dev.index] = buf
    return ws


def _call(row, dev, case, ws):
    """One call (a two-call stream for the deferred and lagged rows) with poisoned outputs -> the outputs."""
    import torch
    outs = row.run(dev, case, ws, row.alloc(dev, case))
    torch.cuda.synchronize()
    return tuple(outs)


def _bits(row, dev, case, outs):
    return tuple(row.canonical_outs(dev, case, outs)) if row.canonical else outs


def _is_noop(row, case):
    return case == "noop" and not row.noop_writes


@functools.lru_cache(maxsize=None)
def _anchor(dev, rname, case):
    import torch
    row = W.BY_NAME[rname]
    buf = torch.zeros(row.need(case) + (1 << 20), dtype=torch.uint8, device=dev)
    ws = _workspace(buf, dev)
    outs = _call(row, dev, case, ws)
    assert ws._buf[dev.index] is buf
    if _is_noop(row, case):
        assert W.untouched(outs), f"{rname}: the header documents n = 0 as a no-op, the outputs were written"
        ratio = 0.0
    else:
        ratio = row.check(case, W._np(outs))
    WORST[rname] = max(WORST.get(rname, 0.0), ratio)
    print(f"{rname} {case}: anchor error / bar {ratio:.3e}")
    assert W.header_zero(buf, row.contract), f"{rname} {case}: header not zero after the call"
    return _bits(row, dev, case, outs)


def _same(row, dev, case, outs, anchor, what):
    got = _bits(row, dev, case, outs)
    assert len(got) == len(anchor), what
    for k, (a, b) in enumerate(zip(got, anchor)):
        assert W.same_bits(a, b), f"{what}: output {k} differs from the anchor's"
    if _is_noop(row, case):
        assert W.untouched(outs), f"{what}: a documented no-op wrote its outputs"


IDS = [f"{r}-{c}" for r, c in W.CASES]


@pytest.mark.parametrize("rname,case", W.CASES, ids=IDS)
def test_exact_size_poisoned_workspace(dev, rname, case):
    row = W.BY_NAME[rname]
    anchor = _anchor(dev, rname, case)
    need = row.need(case)
    for pattern in W.PATTERNS:
        what = f"{rname} {case} pattern {pattern:#x}"
        whole, view = W.make_guarded(need, row.contract, pattern, dev)
        ws = _workspace(view, dev)
        outs = _call(row, dev, case, ws)
        assert ws._buf[dev.index] is view, f"{what}: the wrapper asked for more than the query's {need} bytes"
        assert W.guards_clean(whole, need, pattern), f"{what}: a write outside the queried size"
        _same(row, dev, case, outs, anchor, what)
        assert W.header_zero(view, row.contract), f"{what}: header not zero after the call"


@pytest.mark.parametrize("rname", [r.name for r in W.ROWS])
def test_shape_change_sequence(dev, rname):
    row = W.BY_NAME[rname]
    seq = row.sequence()
    need = max(row.need(c) for c in seq)
    pattern = 0x5A
    whole, view = W.make_guarded(need, row.contract, pattern, dev)
    ws = _workspace(view, dev)
    for k, case in enumerate(seq + seq[-1:]):        # W5: the last call once more
        what = f"{rname} call {k} ({case})"
        outs = _call(row, dev, case, ws)
        assert ws._buf[dev.index] is view, what
        _same(row, dev, case, outs, _anchor(dev, rname, case), what)
        assert W.header_zero(view, row.contract), f"{what}: header not zero after the call"
        assert W.guards_clean(whole, need, pattern), f"{what}: a write outside the buffer"
