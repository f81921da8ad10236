"""CPU checks of tests/workspace_matrix.py: every entry point that takes a workspace has a row, every case's query
answers on the host, the block counts the module docstring derives are what the launchers' arithmetic gives, the
segment query covers the ranged grid, and the checkers of the GPU file can fail."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_matrix as W  # noqa: E402


def _exports():
    from insite_amd import _lib
    out = []
    for name in ("EXPORTS", "EXT_EXPORTS", "WEAK_EXPORTS", "BOOT_EXPORTS", "EFFECT_EXPORTS", "COHORT_EXPORTS",
                 "REGIMEN_EXPORTS", "POLICY_EXPORTS"):
        out += list(getattr(_lib, name))
    assert {n for n in dir(_lib) if n.endswith("EXPORTS")} == {"EXPORTS", "EXT_EXPORTS", "WEAK_EXPORTS", "BOOT_EXPORTS",
                                                                "EFFECT_EXPORTS", "COHORT_EXPORTS", "REGIMEN_EXPORTS",
                                                                "POLICY_EXPORTS"}, "a new export list: add it here"
    return out


# the entry points whose workspace arguments are not used (their queries are in NO_WORKSPACE)
UNUSED_WORKSPACE = {"insite_effect_bands_f64", "insite_regimen_choice_f64"}


def test_every_workspace_query_has_a_row_or_a_reason():
    queries = {n for n in _exports() if n.endswith("_workspace_bytes")}
    in_rows = {r.query for r in W.ROWS}
    assert in_rows <= queries and set(W.NO_WORKSPACE) <= queries
    assert not in_rows & set(W.NO_WORKSPACE)
    missing = queries - in_rows - set(W.NO_WORKSPACE)
    assert not missing, f"no row in tests/workspace_matrix.py for {sorted(missing)}"
    assert all(W.NO_WORKSPACE.values())


def test_every_entry_point_with_a_workspace_argument_has_a_row():
    """An entry point takes a workspace when its signature ends (void* workspace, size_t workspace_bytes, void*
    stream)."""
    from insite_amd import _lib
    takes = {n for n, (_, a) in _lib._SIGNATURES.items()
             if len(a) >= 3 and a[-1] is ctypes.c_void_p and a[-2] is ctypes.c_size_t and a[-3] is ctypes.c_void_p}
    assert takes <= set(_exports())
    rows = {r.export for r in W.ROWS}
    assert rows <= takes
    missing = takes - rows - UNUSED_WORKSPACE
    assert not missing, f"no row in tests/workspace_matrix.py for {sorted(missing)}"


def test_rows_are_well_formed():
    from insite_amd import multistate, ops
    for r in W.ROWS:
        mod, fn = r.wrapper.split(".")
        assert callable(getattr({"ops": ops, "multistate": multistate}[mod], fn)), r.wrapper
        assert r.contract in W.CONTRACTS and r.tolerance, r.name
        assert {"noop", "short"} <= set(r.cases) and len(r.cases) >= 4, r.name
        assert r.smallest not in ("noop", "short") and r.largest in r.cases, r.name
        assert set(r.query_zero) <= set(r.cases)
        assert set(r.sequence()) <= set(r.cases)


@pytest.mark.parametrize("rname,case", W.CASES, ids=[f"{r}-{c}" for r, c in W.CASES])
def test_query_of_every_case(rname, case):
    row = W.BY_NAME[rname]
    need = row.need(case)
    if case in row.query_zero:
        assert need == 0
    else:
        assert need >= max(W.CONTRACTS[row.contract], 1), need
        assert need % 4 == 0


@pytest.mark.parametrize("query,args", W.ZERO_QUERIES, ids=[f"{q}{a}" for q, a in W.ZERO_QUERIES])
def test_documented_zero_queries(query, args):
    from insite_amd import _lib
    assert getattr(_lib.load(), query)(*args) == 0


# ---------------------------------------------------------------------------------------------------
# the block counts of the module docstring, from the launchers' arithmetic restated
# ---------------------------------------------------------------------------------------------------
def _cd(a, b):
    return -(-a // b)


def test_block_counts_of_the_cases():
    """The launchers' formulas restated (tests/workspace_matrix.py derives them with source lines): this checks the
    restatement, not the launched grid, which cannot be seen from outside.  Re-read the formulas when a launcher
    changes."""
    want = {"b1": 1, "b16": 16, "b17": 17, "b33": 33}
    for k, blocks in want.items():
        assert _cd(_cd(W.DISC_N[k], 64), 4) == blocks          # gram_plan, one segment; seg_grid
        assert _cd(W.WEAK_N[k], 64) == blocks                  # wk_grid
    seg = W.BY_NAME["gram_segments"].cases
    for k, blocks in dict(want, tall=62).items():
        c = seg[k]
        assert _cd(_cd(c["N"], 64) * _cd(c["T"] - 1, 4), 4) == blocks
    for rname, cases in (("sindy_fit_segments", seg), ("sindy_fit_irregular", None), ("sindy_fit", None),
                         ("gram_moments", None), ("gram_irregular", None)):
        rc = W.BY_NAME[rname].cases
        assert set(want) <= set(rc), rname                     # every gram_tail row has the four block counts
        for k, blocks in want.items():
            c = rc[k]
            got = _cd(_cd(c["N"], 64) * _cd(c["T"] - 1, 4), 4) if cases else _cd(_cd(c["N"], 64), 4)
            assert got == blocks, (rname, k)
    assert _cd(62, 16) == 4 and W.DISC_T < 96 and W.DISC_T <= 16
    pp = W.BY_NAME["per_patient"].cases
    assert _cd(_cd(pp["b1"]["N"], 64), 4) == 1 and _cd(_cd(pp["b17"]["N"], 64), 4) == 17
    assert [W.STEP_GB[k] for k in ("gb1", "gb16", "gb17", "gb33")] == [1, 16, 17, 33]
    # bootstrap: 70 columns = 5 column tiles -> 3 replicate tiles of 16 per wave
    assert _cd(2 * 35, 16) == 5 and _cd(17, 48) == 1 and _cd(50, 48) == 2
    # cohort / policy: chunks = min(8192 / (replicate tiles x groups), ceil(N / 64))
    for k, chunks in (("c1_r2", 1), ("c1_r65", 1), ("c3_r2", 3), ("c3_r65", 3)):
        c = W.ENS_CASES[k]
        assert min(8192 // (_cd(c["R"], 64) * W.ENS_G), _cd(c["N"], 64)) == chunks
    assert _cd(1234, 64) == 20 and _cd(5000, 4096) == 2 and _cd(_cd(300, 64), 4) == 2


@pytest.mark.parametrize("rname", ["gram_segments", "sindy_fit_segments"])
def test_segment_query_covers_the_ranged_grid(rname):
    """gram_seg_kernel stores one partial of n_arms x nE doubles per block and one per group of 16 blocks after the
    512-byte header; the ranged launch takes ceil(units / 4) blocks (capped by the resident blocks), units =
    ceil(N / 64) x ceil((n_steps - 1) / 4), whatever seg_grid(N) is."""
    import library_matrix as M
    row = W.BY_NAME[rname]
    for case, c in row.cases.items():
        F = M.TABLE[c["name"]][0]
        n_ent = c["n_arms"] * (F * (F + 1) // 2 + F)
        blocks = max(1, _cd(_cd(c["N"], 64) * _cd(max(c["T"] - 1, 1), 4), 4))
        assert row.need(case) >= 512 + (blocks + _cd(blocks, 16)) * n_ent * 8, (case, blocks)


# ---------------------------------------------------------------------------------------------------
# the checkers can fail (this stands in for a kernel that misbehaves)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", W.PATTERNS)
@pytest.mark.parametrize("contract", sorted(W.CONTRACTS))
def test_guards_notice_one_byte(contract, pattern):
    need = 5000
    whole, view = W.make_guarded(need, contract, pattern, "cpu")
    assert whole.numel() == need + 2 * W.GUARD and view.numel() == need
    assert view.data_ptr() == whole.data_ptr() + W.GUARD
    assert W.guards_clean(whole, need, pattern) and W.header_zero(view, contract)
    h = W.CONTRACTS[contract]
    assert bool((view[h:] == pattern).all()), "only the contract's header is zeroed"
    view.fill_(0x11)                       # writes inside the view are allowed
    assert W.guards_clean(whole, need, pattern)
    for pos in (0, W.GUARD - 1, W.GUARD + need, whole.numel() - 1):
        w2 = whole.clone()
        w2[pos] = (pattern + 1) & 0xFF
        assert not W.guards_clean(w2, need, pattern), pos
    assert not W.guards_clean(whole[:-1], need, pattern)


@pytest.mark.parametrize("contract", ["header512", "claim4k"])
def test_header_check_notices_one_byte(contract):
    _, view = W.make_guarded(8192, contract, 0x5A, "cpu")
    h = W.CONTRACTS[contract]
    for pos in (0, 4, h - 1):
        v = view.clone()
        v[pos] = 1
        assert not W.header_zero(v, contract), pos
    v = view.clone()
    v[h] = 1
    assert W.header_zero(v, contract)      # past the header anything goes
    assert W.header_zero(view[:0], "none") and W.header_zero(view, "self_zeroed")


def test_same_bits_is_bitwise():
    import torch
    for dt in (torch.float64, torch.float32):
        a = torch.tensor([1.0, 0.0, float("nan"), -2.5], dtype=dt)
        assert W.same_bits(a, a.clone())
        b = a.clone()
        b[0] = torch.nextafter(a[0], torch.tensor(2.0, dtype=dt))
        assert not W.same_bits(a, b), "one ulp"
        b = a.clone()
        b[1] = -0.0
        assert not W.same_bits(a, b), "0.0 against -0.0"
        assert W.same_bits(torch.tensor([float("nan")], dtype=dt), torch.tensor([float("nan")], dtype=dt))
    i = torch.tensor([1, 2, 3], dtype=torch.int32)
    assert W.same_bits(i, i.clone()) and not W.same_bits(i, i + 1)
    assert not W.same_bits(i, i.to(torch.int64)) and not W.same_bits(i, i[:2])


def test_untouched_and_rel_err():
    import torch
    outs = (W._full("cpu", (2, 3), torch.float64), W._full("cpu", (4,), torch.int8), W._full("cpu", (0,), torch.int32))
    assert W.untouched(outs)
    outs[1][2] = 0
    assert not W.untouched(outs)
    assert W.rel_err(np.array([1.0, np.nan]), np.array([1.0, np.nan]), 1.0) == 0.0
    assert W.rel_err(np.array([1.0, np.nan]), np.array([1.0, 2.0]), 1.0) == np.inf
    assert W.rel_err(np.array([1e-3]), np.array([0.0]), 0.0) == np.inf
    assert abs(W.rel_err(np.array([1.5]), np.array([1.0]), 2.0) - 0.25) < 1e-15
