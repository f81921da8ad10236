"""The workspace matrix: one row per entry point of the C ABI that takes a caller-owned workspace, shared by
tests/test_workspace_matrix.py (CPU) and tests/test_gpu_workspace_matrix.py (GPU).  Helper only: no tests here.

What the eight headers promise about a workspace, in one place:

  W1  a buffer of exactly ``*_workspace_bytes(...)`` bytes is enough, nothing is written outside it;
  W2  only a documented header must be zero before the first use (the contract class of the row), the rest may hold
      anything;
  W3  every call leaves that header zero;
  W4  the outputs do not depend on what an earlier call of another shape left in the buffer;
  W5  fixed-order sums: a repeated call gives the same bits.

Contract classes (CONTRACTS): "header512" the first 512 bytes (gram_tail's arrival counters, or a reserved header);
"claim4k" the 4 KiB claim areas of the deferred and lagged steps; "none" nothing (scratch written before it is read);
"self_zeroed" nothing (insite_rk45_order_i32 clears its histogram itself).

Shape cases.  Every row has the degenerate cases "noop" (n_patients / n_rows = 0) and "short" (no patient has enough
rows, or no row contributes) and the smallest cohorts that reach each path of its reduction.  The block counts are
the launcher's (line numbers of csrc/insite_hip.hip unless another file is named); where a grid is capped by the
resident blocks of the device the cap is at least 256 on the MI355X's 256 CUs (resident_waves, 4268-4284: CUs x
blocks per CU, at least one), which none of the cases reaches:

* gram_tail (185-360): groups of kTailGroup = 16 blocks, at most kTailMaxGroups = 64 groups; the cases are 1 block,
  16 blocks (one full group), 17 blocks (a second group with one member) and 33 blocks (three groups).
  - insite_gram_f64, patient-major (launch_gram4 4347-4372, gram_plan 4289-4311): n_steps = 9 < 96 gives one
    segment, grid = ceil(ceil(N / 64) / 4): N = 200, 3900, 4100, 8200 -> 1, 16, 17, 33 blocks.
    Every row that goes through gram_tail has all four, the fused-STLSQ instantiations included (STF = 7 for
    insite_sindy_fit_f64, insite_gram_moments_f64, insite_sindy_fit_irregular_f64 and the step, STF = 4 for
    insite_sindy_fit_segments_f64): with exactly 16 blocks the only group reducer is also the final reducer that
    solves the fits.
  - insite_sindy_fit_f64 and insite_gram_moments_f64, time-major: ranged mode (4360-4367) with n_steps = 9 <= 16 has
    ceil(N / 64) units, the moments launch (4351-4359) ceil(N / 64) tiles; both give the same grids for the same N.
  - insite_gram_irregular_f64 / insite_sindy_fit_irregular_f64: grid = seg_grid(N) = ceil(ceil(N / 64) / 4)
    (4483-4487, 4582): the same N.
  - insite_gram_segments_f64 / insite_sindy_fit_segments_f64 (launch_gram_seg 4489-4508, INSITE_SEG_RANGED): units
    = ceil(N / 64) x ceil((n_steps - 1) / 4), grid = ceil(units / 4).  n_steps = 9 (two chunks): N = 100, 2000, 2100,
    4130 -> 2, 64, 66, 130 units -> 1, 16, 17, 33 blocks.  The case "tall" (N = 256, n_steps = 246, nine terms, one
    arm) has 4 x 62 = 248 units = 62 blocks in four groups: 66 rows of 54 partials, one more than seg_grid(256) +
    kTailMaxGroups = 65.  The grid grows with n_steps, which the query is not given, so the query has to size the
    partials for the most blocks a ranged launch takes (kSegRangedBlocks), not for seg_grid(N): this case is the
    smallest in which the two differ by less than a guard.
  - insite_fit_rollout_f64 (step_plan 4225-4239): an explicit gram_blocks is the block count of the tail whatever N
    (blocks without a unit store zero partials): gram_blocks = 1, 16, 17, 33 on one 300-patient cohort, and 0 (the
    default split, half the resident blocks).  insite_fit_rollout_deferred_f64 / _lagged_f64 (4898-4904) take the
    same gram_blocks; their finalisation (deferred_finalize 366-397) sums the same groups without counters.
* insite_sindy_fit_per_patient_f64 (launch_moments 4405-4410, the moments launch of 4351-4359): 1 and 17 blocks.
  Two sizes only: the moments launch (MOM = 1) never calls gram_tail, every block writes its own patients' moments.
* insite_gram_weak_f64 / insite_sindy_fit_weak_f64 (csrc/insite_weak.hip, wk_grid 57-61: one block per 64
  patients; weak_finalize_kernel 248-: groups of kWkGroup = 16): N = 50, 1000, 1050, 2100 -> 1, 16, 17, 33 blocks.
  insite_sindy_fit_weak_f64 has 1 and 17 blocks only: its Gram pass is insite_gram_weak_f64's, finalised by a
  separate launch without counters, and the solve is one more launch on G | b.
* insite_bootstrap_gram_f64 / insite_sindy_bootstrap_f64 (csrc/insite_boot.hip, bt_plan 53-70): std7 with two arms
  has 70 columns = 5 column tiles, so 3 replicate tiles of 16 per wave: R = 17 is one replicate group, R = 50 two.
* insite_cohort_effect_*_f64 (csrc/insite_cohort.hip, co_plan 61-84) and insite_policy_*_f64 (csrc/insite_policy.hip,
  po_plan 58-78): patient chunks = min(8192 / (replicate tiles x groups [x time tiles]), ceil(N / 64)): N = 40 is
  one chunk, N = 130 three; R = 2 and R = 65 (one replicate past a tile of 64).  The chunking comes from the plan
  (co_plan / po_plan of the shape), never from workspace_bytes, which is only compared with plan.bytes (411), so the
  bits do not depend on the size of the buffer.
* insite_gen_gram_f64 / insite_gen_gram_segments_f64 (csrc/insite_gen.hip 576-674): kGenChunks = 256 fixed patient
  chunks; N = 70 (chunks of one patient, most empty) and N = 600 (three patients per chunk).
* insite_masked_sse_f64 (sse_grid 4318-4323: ceil(N / 64) blocks): N = 50 and 1234.
* insite_gram_ms_f32 (csrc/insite_ms.hip, ms_grid 1497-1505): N = 67 (one block) and 300 (two).
* insite_rk45_order_i32 (5399-5414): 4096 rows per block: N = 100 and 5000.

The grids cannot be seen from outside a launch: the block counts above are the launchers' formulas restated, and
tests/test_workspace_matrix.py checks the restatement, not the launched grid.  Whoever changes launch_gram4,
gram_plan, launch_gram_seg, seg_grid, wk_grid, bt_plan, co_plan, po_plan or step_plan must re-read the formulas and
line numbers here and move the cases, or they silently stop reaching the 16-, 17- and 33-block paths.

No call's result depends on the byte count it is given: every launcher reads workspace_bytes only to refuse a buffer
that is too small.  insite_rk45_order_i32 orders the rows of one bin by arrival (LDS and global atomics; the header
calls the order "scheduling only"), so its bits are compared on the canonical form (the keys in output order, the
sorted permutation).

Oracles and tolerances are the ones each operation's own GPU test uses (the ``tolerance`` of a row cites it).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bootstrap_ref as BR  # noqa: E402
import cohort_effect_ref as CR  # noqa: E402
import irregular_ref as IR  # noqa: E402
import library_matrix as M  # noqa: E402
import policy_ref as P  # noqa: E402
import step_matrix as SM  # noqa: E402
from oracle import insite_ref as R  # noqa: E402
from oracle import multistate_ref as MSR  # noqa: E402
from oracle import segments_ref as S  # noqa: E402

# ---------------------------------------------------------------------------------------------------
# a. buffers and comparisons: plain functions over tensors on any device
# ---------------------------------------------------------------------------------------------------
GUARD = 4096
CONTRACTS = {"header512": 512, "claim4k": 4096, "none": 0, "self_zeroed": 0}   # bytes that must be zero
PATTERNS = (0xFF, 0x5A)   # NaN as f64, -1 as int32, a saturated counter | the project's usual poison
FILL_F, FILL_I8, FILL_I32 = -7.25, 3, -77   # what the outputs hold before a call


def make_guarded(need, contract, pattern, device):
    """(whole, view): need + 2 * GUARD bytes filled with ``pattern``; view = the ``need`` bytes at offset GUARD (which
    keeps the alignment of the allocation), its contract header zeroed and nothing else."""
    import torch
    whole = torch.full((int(need) + 2 * GUARD,), pattern, dtype=torch.uint8, device=device)
    view = whole[GUARD:GUARD + int(need)]
    view[:min(CONTRACTS[contract], int(need))] = 0
    return whole, view


def guards_clean(whole, need, pattern):
    lo, hi = whole[:GUARD], whole[GUARD + int(need):]
    return hi.numel() == GUARD and bool((lo == pattern).all()) and bool((hi == pattern).all())


def header_zero(view, contract):
    return not bool(view[:min(CONTRACTS[contract], view.numel())].any())


def same_bits(a, b):
    """Equal shapes, dtypes and bit patterns: NaN equals NaN of the same payload, -0.0 differs from 0.0."""
    import torch
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    elif a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def rel_err(got, ref, scale):
    """max |got - ref| / scale (broadcast); a NaN on one side only is inf, an entry of scale 0 must be exact."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    if not np.array_equal(nan_g, nan_r):
        return np.inf
    err = np.where(nan_r, 0.0, np.abs(np.where(nan_g, 0.0, got) - np.where(nan_r, 0.0, ref)))
    s = np.broadcast_to(scale, got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, err / s, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def _t(a, dev, dtype=None):
    """numpy -> device tensor (an empty array: a fresh tensor, whose strides the wrappers accept)."""
    import torch
    a = np.ascontiguousarray(a)
    if not a.size:
        return torch.zeros(a.shape, device=dev, dtype=dtype or getattr(torch, a.dtype.name))
    return torch.tensor(a, device=dev, dtype=dtype)


def _full(dev, shape, dtype):
    import torch
    fill = {torch.float64: FILL_F, torch.float32: FILL_F, torch.int8: FILL_I8, torch.int32: FILL_I32}[dtype]
    return torch.full(tuple(shape), fill, dtype=dtype, device=dev)


def untouched(outs):
    """Every output still holds what _full wrote."""
    import torch
    fill = {torch.float64: FILL_F, torch.float32: FILL_F, torch.int8: FILL_I8, torch.int32: FILL_I32}
    return all(bool((o == fill[o.dtype]).all()) for o in outs)


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _np(outs):
    return [o.cpu().numpy() for o in outs]


# ---------------------------------------------------------------------------------------------------
# b. shared checks (each returns the worst error / bar ratio it saw, after asserting it)
# ---------------------------------------------------------------------------------------------------
THRESHOLD, ALPHA = SM.THRESHOLD, SM.ALPHA
COEF_TOL = 1e-8        # tests/test_gpu_parity.py, tests/test_gpu_bootstrap.py, tests/step_matrix.py (COEF_ATOL)
ENSEMBLE_TOL = 1e-10   # tests/test_gpu_cohort_effect.py, tests/test_gpu_policy.py (TOL)


def check_gram(G, b, Gr, br, SG, Sb, what):
    """Per entry |G - G_ref| <= GRAM_RTOL S_G, |b - b_ref| <= GRAM_RTOL S_b; G symmetric.  -> worst error / bar."""
    worst = 0.0
    for tag, got, ref, scale in (("G", G, Gr, SG), ("b", b, br, Sb)):
        assert got.shape == ref.shape and np.all(np.isfinite(got)), (what, tag)
        r = M.worst_ratio(got, ref, scale)
        assert r <= M.GRAM_RTOL, (what, tag, r)
        worst = max(worst, r)
    assert np.array_equal(G, np.swapaxes(G, -1, -2)), (what, "G is not symmetric")
    return worst / M.GRAM_RTOL


def check_stlsq(coef, mask, iters, G, b, what, threshold=THRESHOLD):
    """Support, iteration count and coefficients against oracle.insite_ref.stlsq_gram on the call's own G | b (the
    form of tests/test_gpu_general.py and test_sindy_fit_fused_matches_oracle).  -> L-inf error of the coefficients."""
    F = G.shape[-1]
    worst = 0.0
    for s, (Gs, bs) in enumerate(zip(G.reshape(-1, F, F), b.reshape(-1, F))):
        cr, sr, ir = R.stlsq_gram(Gs, bs, threshold, ALPHA)
        assert np.array_equal(mask.reshape(-1, F)[s] != 0, sr), (what, s)
        assert int(iters.reshape(-1)[s]) == ir, (what, s, int(iters.reshape(-1)[s]), ir)
        worst = max(worst, float(np.max(np.abs(coef.reshape(-1, F)[s] - cr))))
    assert worst < COEF_TOL, (what, worst)
    return worst


# ---------------------------------------------------------------------------------------------------
# c. the rows
# ---------------------------------------------------------------------------------------------------
class Row:
    """One entry point.  ``cases``: name -> shape parameters, in the order small to large, then "noop" and "short";
    ``query_zero``: the cases for which the header documents a query result of 0."""
    name = wrapper = export = query = tolerance = ""
    contract = "header512"
    noop_writes = False      # n_patients = 0 still runs the finalisation: the outputs are the oracle's (zeros)
    canonical = False        # bits are compared on canonical(outs) (insite_rk45_order_i32)
    query_zero = ()
    cases: dict = {}

    @property
    def smallest(self):
        return next(iter(self.cases))

    @property
    def largest(self):
        return [c for c in self.cases if c not in ("noop", "short")][-1]

    def sequence(self):
        """W4: largest, smallest, no-op, too few rows, smallest, largest (the buffer is sized for the largest query
        among them)."""
        return [self.largest, self.smallest, "noop", "short", self.smallest, self.largest]

    def need(self, case):
        from insite_amd import _lib
        return int(getattr(_lib.load(), self.query)(*self.query_args(case)))

    # per row: query_args(case), alloc(dev, case), run(dev, case, ws, outs), check(case, outs as numpy) -> float


def _lib7():
    return M.LIBS["std7"]


# ---- the strong-form discovery family on one std7 / two-arm cohort recipe --------------------------------------
DISC_T = 9
DISC_N = {"b1": 200, "b16": 3900, "b17": 4100, "b33": 8200, "noop": 0, "short": 300}
FD = "smoothed4"


@functools.lru_cache(maxsize=None)
def disc_cohort(N, T=DISC_T, short=False):
    """(x [N, T] NaN past rows, u [N, 2], arm [N], rows [N]): library_matrix.cohort; short: rows = p % 5."""
    x, u, arm, rows = M.cohort(max(N, 1), T, 2, M._seed("ws-disc", N, T, short), 2)
    x, u, arm, rows = x[:N], u[:N], arm[:N], rows[:N]
    if short:
        rows = (np.arange(N) % 5).astype(np.int64)
        x = x.copy()
        x[np.arange(T)[None, :] >= rows[:, None]] = np.nan
    return _freeze(x, u, arm, rows)


@functools.lru_cache(maxsize=None)
def disc_ref(N, T=DISC_T, short=False):
    return _freeze(*M.gram_ref(*disc_cohort(N, T, short), M.DT, M.exps_of("std7"), 2, FD))


@functools.lru_cache(maxsize=None)
def _disc_dev(dev, N, T, short, layout):
    """Device inputs; time-major x is the [T, N] view of a [T, N + 5] buffer with NaN padding."""
    import torch
    x, u, arm, rows = disc_cohort(N, T, short)
    if layout == "time":
        buf = torch.full((T, N + 5), float("nan"), dtype=torch.float64, device=dev)
        if N:
            buf[:, :N] = _t(x.T, dev)
        xd = buf[:, :N]
    else:
        xd = _t(x, dev)
    return xd, _t(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32)


class _DiscRow(Row):
    layout = "patient"
    cases = {k: dict(N=v, short=k == "short") for k, v in DISC_N.items()}
    noop_writes = True   # run_discovery has no early return: the tail reduces zero partials, G = b = 0

    def query_args(self, case):
        return (self.cases[case]["N"], 2, 7)

    def _args(self, dev, case):
        c = self.cases[case]
        return _disc_dev(dev, c["N"], DISC_T, c["short"], self.layout)

    def _ref(self, case):
        c = self.cases[case]
        return disc_ref(c["N"], DISC_T, c["short"])


class GramRow(_DiscRow):
    name, wrapper, export, query = "gram", "ops.gram", "insite_gram_f64", "insite_gram_workspace_bytes"
    tolerance = "library_matrix.GRAM_RTOL per entry scale (tests/test_gpu_library_matrix.py::test_strong_gram)"

    def alloc(self, dev, case):
        import torch
        return (_full(dev, (2, 7, 7), torch.float64), _full(dev, (2, 7), torch.float64))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        ops.gram(*self._args(dev, case), M.DT, _lib7(), n_arms=2, fd=FD, workspace=ws, out=outs, layout=self.layout)
        return outs

    def check(self, case, outs):
        Gr, br, SG, Sb, _ = self._ref(case)
        return check_gram(outs[0], outs[1], Gr, br, SG, Sb, (self.name, case))


class SindyFitRow(_DiscRow):
    """Time-major with seven terms: the STLSQ runs in the tail's last block (launch mode 3)."""
    name, wrapper, export, query = "sindy_fit", "ops.sindy_fit", "insite_sindy_fit_f64", "insite_gram_workspace_bytes"
    layout = "time"
    tolerance = "GRAM_RTOL per entry scale; support, iterations, |coef| < 1e-8 (test_sindy_fit_fused_matches_oracle)"

    def alloc(self, dev, case):
        import torch
        return (_full(dev, (2, 7), torch.float64), _full(dev, (2, 7), torch.int8), _full(dev, (2,), torch.int32),
                _full(dev, (2, 7, 7), torch.float64), _full(dev, (2, 7), torch.float64))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        ops.sindy_fit(*self._args(dev, case), M.DT, _lib7(), THRESHOLD, ALPHA, n_arms=2, fd=FD, workspace=ws, out=outs,
                      layout=self.layout)
        return outs

    def check(self, case, outs):
        coef, mask, iters, G, b = outs[:5]
        Gr, br, SG, Sb, _ = self._ref(case)
        w = check_gram(G, b, Gr, br, SG, Sb, (self.name, case))
        check_stlsq(coef, mask, iters, G, b, (self.name, case))
        return w


class GramMomentsRow(SindyFitRow):
    name, wrapper, export = "gram_moments", "ops.gram_moments", "insite_gram_moments_f64"
    tolerance = ("GRAM_RTOL per entry scale; moments 1e-10 of the column maximum "
                 "(test_gram_moments_succeeds_exactly_where_the_plan_fits)")

    def alloc(self, dev, case):
        import torch
        return SindyFitRow.alloc(self, dev, case) + (_full(dev, (self.cases[case]["N"], 5), torch.float64),)

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        ops.gram_moments(*self._args(dev, case), M.DT, _lib7(), THRESHOLD, ALPHA, n_arms=2, fd=FD, workspace=ws,
                         out=outs, layout=self.layout)
        return outs

    def check(self, case, outs):
        w = SindyFitRow.check(self, case, outs)
        mom, momr = outs[5], self._ref(case)[4]
        assert np.array_equal(mom[:, 0], momr[:, 0])
        if mom.size:
            assert np.all(np.abs(mom - momr).max(axis=0) <= 1e-10 * np.abs(momr).max(axis=0))
        return w


class PerPatientRow(_DiscRow):
    name, wrapper = "per_patient", "ops.sindy_fit_per_patient"
    export, query = "insite_sindy_fit_per_patient_f64", "insite_per_patient_workspace_bytes"
    cases = {k: dict(N=DISC_N[k], short=k == "short") for k in ("b1", "b17", "noop", "short")}
    noop_writes = False   # returns before anything is launched
    tolerance = "mask and iterations equal, |coef - ref| < 1e-8 (tests/test_gpu_parity.py::test_per_patient_fit_*)"

    def query_args(self, case):
        return (self.cases[case]["N"],)

    @staticmethod
    def global_coef():
        g = np.zeros((2, 7))
        g[:, 1] = -0.5        # support {x0} for both arms
        g[1, 4] = 0.2         # arm 1: {x0, x0 u0}
        return g

    def alloc(self, dev, case):
        import torch
        N = self.cases[case]["N"]
        return (_full(dev, (N, 2, 7), torch.float64), _full(dev, (N, 7), torch.int8), _full(dev, (N,), torch.int32))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        ops.sindy_fit_per_patient(*self._args(dev, case), M.DT, _lib7(), _t(self.global_coef(), dev), THRESHOLD, ALPHA,
                                  fd=FD, workspace=ws, out=outs, layout=self.layout)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        x, u, arm, rows = disc_cohort(c["N"], DISC_T, c["short"])
        cr, mr, ir = R.per_patient_fit(np.nan_to_num(x), u, arm, np.minimum(rows, DISC_T), M.DT, M.exps_of("std7"),
                                       self.global_coef(), THRESHOLD, ALPHA)
        assert np.array_equal(outs[1], mr) and np.array_equal(outs[2], ir), (self.name, case)
        err = float(np.max(np.abs(outs[0] - cr))) if cr.size else 0.0
        assert err < COEF_TOL, (self.name, case, err)
        if c["short"]:   # the header: patients with < 5 rows keep the global model (iters 0)
            assert np.array_equal(outs[0], np.repeat(self.global_coef()[None], c["N"], 0)) and not outs[2].any()
        return err / COEF_TOL


# ---- the step family --------------------------------------------------------------------------------------------
STEP_N = 300
STEP_GB = {"gb1": 1, "gb16": 16, "gb17": 17, "gb33": 33, "gb0": 0}
STEP_ROLL = "r65_t33_lane"
Y_FILL = -777.25


@functools.lru_cache(maxsize=None)
def _roll_dev(dev):
    import torch
    from insite_amd import ops
    c = SM.ROLL[STEP_ROLL]
    y0, u, arm, coef = SM.roll_inputs(STEP_ROLL, "std7")
    bits = ops.pack_arm_bits(_t(arm.T, dev, torch.int8), c.Nr)
    return _t(y0, dev), _t(u, dev), bits, _t(coef, dev)


class _StepRow(_DiscRow):
    layout = "time"
    query = "insite_gram_workspace_bytes"
    cases = dict([(k, dict(N=STEP_N, short=False, gb=v)) for k, v in STEP_GB.items()]
                 + [("noop", dict(N=0, short=False, gb=0)), ("short", dict(N=STEP_N, short=True, gb=7))])

    def alloc(self, dev, case):
        import torch
        c = SM.ROLL[STEP_ROLL]
        return SindyFitRow.alloc(self, dev, case) + (torch.full((c.Tr, c.Nr), Y_FILL, dtype=torch.float64, device=dev),)

    def _roll_kw(self):
        c = SM.ROLL[STEP_ROLL]
        meth, sub = SM.METHODS[c.method]
        return dict(method=meth, substeps=sub, drop_below=SM.DROP_BELOW, T=c.Tr)

    def _check_y(self, y):
        ref = SM.roll_ref(STEP_ROLL, "std7")
        np.testing.assert_allclose(y.T, ref, rtol=SM.Y_RTOL, atol=SM.Y_ATOL)

    def check(self, case, outs):
        w = SindyFitRow.check(self, case, outs)
        self._check_y(outs[5])
        return w


class FitRolloutRow(_StepRow):
    name, wrapper, export = "fit_rollout", "ops.fit_rollout", "insite_fit_rollout_f64"
    tolerance = "GRAM_RTOL per entry scale, |coef| < 1e-8, y at rtol 1e-11 / atol 1e-12 (tests/test_gpu_step_matrix.py)"

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        y0, ru, bits, cin = _roll_dev(dev)
        ops.fit_rollout(*self._args(dev, case), M.DT, _lib7(), THRESHOLD, ALPHA, y0, ru, bits, cin, SM.ROLLOUT_DT,
                        fd=FD, workspace=ws, out=outs[:5], y_out=outs[5], gram_blocks=self.cases[case]["gb"],
                        **self._roll_kw())
        return outs


class DeferredRow(_StepRow):
    """A stream of two calls on one workspace: call 0 streams the cohort into slot 0, call 1 (n_patients = 0, slot 1)
    finalises it.  The outputs are call 1's."""
    name, wrapper, export = "fit_rollout_deferred", "ops.fit_rollout_deferred", "insite_fit_rollout_deferred_f64"
    query = "insite_fit_rollout_deferred_workspace_bytes"
    contract = "claim4k"
    tolerance = FitRolloutRow.tolerance

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        y0, ru, bits, cin = _roll_dev(dev)
        scratch = self.alloc(dev, case)
        common = (M.DT, _lib7(), THRESHOLD, ALPHA, y0, ru, bits, cin, SM.ROLLOUT_DT)
        kw = dict(fd=FD, gram_blocks=self.cases[case]["gb"], **self._roll_kw())
        ops.fit_rollout_deferred(*self._args(dev, case), *common, 0, False, ws, out=scratch[:5], y_out=scratch[5], **kw)
        assert untouched(scratch[:5]), "a call that does not finalise wrote its outputs"
        ops.fit_rollout_deferred(*_disc_dev(dev, 0, DISC_T, False, "time"), *common, 1, True, ws, out=outs[:5],
                                 y_out=outs[5], **kw)
        return outs


class LaggedRow(_StepRow):
    """The same stream through plan_fit_rollout_lagged: call 1 reduces slot 0 into (G, b); no solve role."""
    name, wrapper, export = "fit_rollout_lagged", "ops.plan_fit_rollout_lagged", "insite_fit_rollout_lagged_f64"
    query = "insite_fit_rollout_deferred_workspace_bytes"
    contract = "claim4k"
    tolerance = "GRAM_RTOL per entry scale, y at rtol 1e-11 / atol 1e-12 (tests/test_gpu_step_matrix.py)"

    def alloc(self, dev, case):
        import torch
        c = SM.ROLL[STEP_ROLL]
        return (_full(dev, (2, 7, 7), torch.float64), _full(dev, (2, 7), torch.float64),
                torch.full((c.Tr, c.Nr), Y_FILL, dtype=torch.float64, device=dev))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        y0, ru, bits, cin = _roll_dev(dev)
        scratch = self.alloc(dev, case)
        common = (M.DT, _lib7(), THRESHOLD, ALPHA, y0, ru, bits, cin, SM.ROLLOUT_DT)
        kw = dict(fd=FD, gram_blocks=self.cases[case]["gb"], **self._roll_kw())
        ops.plan_fit_rollout_lagged(*self._args(dev, case), *common, 0, False, ws, scratch[:2], y_out=scratch[2],
                                    **kw)()
        assert untouched(scratch[:2]), "a call that does not reduce wrote its outputs"
        ops.plan_fit_rollout_lagged(*_disc_dev(dev, 0, DISC_T, False, "time"), *common, 1, True, ws, outs[:2],
                                    y_out=outs[2], **kw)()
        return outs

    def check(self, case, outs):
        Gr, br, SG, Sb, _ = self._ref(case)
        w = check_gram(outs[0], outs[1], Gr, br, SG, Sb, (self.name, case))
        self._check_y(outs[2])
        return w


# ---- treatment segments -----------------------------------------------------------------------------------------
SEG_T = 9


@functools.lru_cache(maxsize=None)
def seg_cohort(N, T, U, n_arms, short=False, p_switch=0.3):
    """library_matrix.segment_inputs at any shape: (x [N, T] NaN past seq_len, u [N, U], arm_steps [N, T - 1],
    seq_len); short: seq_len = 0 everywhere (one sample, no row for an order-1 estimator)."""
    rng = np.random.default_rng(M._seed("ws-seg", N, T, U, n_arms, short))
    x = M._decay(rng, np.arange(T) * M.DT, N)
    u = rng.uniform(0.6, 1.6, (N, U))
    arm = np.empty((N, T - 1), dtype=np.int64)
    if N:
        arm[:, 0] = rng.integers(0, n_arms, N)
    for k in range(1, T - 1):
        other = (arm[:, k - 1] + rng.integers(1, max(n_arms, 2), N)) % n_arms
        arm[:, k] = np.where(rng.random(N) < p_switch, other, arm[:, k - 1])
    sl = rng.integers(0, T, N)
    if N >= 6:
        sl[:6] = [0, 1, 2, 3, T - 1, T - 2]
    if short:
        sl[:] = 0
    for p in range(N):
        x[p, sl[p] + 1:] = np.nan
    return _freeze(x, u, arm, sl)


@functools.lru_cache(maxsize=None)
def seg_ref(N, T, name, n_arms, short, p_switch, fd):
    return _freeze(*M.segments_ref(*seg_cohort(N, T, M.TABLE[name][1], n_arms, short, p_switch), M.DT, M.exps_of(name),
                                   n_arms, fd))


@functools.lru_cache(maxsize=None)
def _seg_dev(dev, key):
    import torch
    x, u, arm, sl = seg_cohort(*key)
    ud = _t(u, dev) if u.shape[1] else None
    return _t(x, dev), _t(arm, dev, torch.int8), _t(sl, dev, torch.int32), ud


def _seg_case(N, name="lin3", n_arms=2, T=SEG_T, short=False, p_switch=0.3):
    return dict(N=N, T=T, name=name, n_arms=n_arms, short=short, p_switch=p_switch)


class GramSegmentsRow(Row):
    name, wrapper, export = "gram_segments", "ops.gram_segments", "insite_gram_segments_f64"
    query = "insite_gram_segments_workspace_bytes"
    noop_writes = True   # run_segment_discovery: "G = b = 0 (and the fit of an all-zero system)" through the tail
    fd = "order1"
    tolerance = "GRAM_RTOL per entry scale (tests/test_gpu_library_matrix.py::test_segment_gram)"
    cases = {"b1": _seg_case(100), "b16": _seg_case(2000), "b17": _seg_case(2100), "b33": _seg_case(4130),
             "tall": _seg_case(256, "u3_x9", 1, 246, p_switch=0.03),
             "noop": _seg_case(0), "short": _seg_case(300, short=True)}

    @property
    def largest(self):
        return "b33"

    def _key(self, case):
        c = self.cases[case]
        return (c["N"], c["T"], M.TABLE[c["name"]][1], c["n_arms"], c["short"], c["p_switch"])

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], c["n_arms"], M.TABLE[c["name"]][0])

    def alloc(self, dev, case):
        import torch
        c = self.cases[case]
        A, F = c["n_arms"], M.TABLE[c["name"]][0]
        return (_full(dev, (A, F, F), torch.float64), _full(dev, (A, F), torch.float64))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        c = self.cases[case]
        x, arm, sl, u = _seg_dev(dev, self._key(case))
        ops.gram_segments(x, arm, sl, u, M.DT, M.LIBS[c["name"]], n_arms=c["n_arms"], fd=self.fd, workspace=ws,
                          out=outs)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        Gr, br, SG, Sb = seg_ref(c["N"], c["T"], c["name"], c["n_arms"], c["short"], c["p_switch"], self.fd)
        return check_gram(outs[-2], outs[-1], Gr, br, SG, Sb, (self.name, case))


class SindyFitSegmentsRow(GramSegmentsRow):
    """Four terms: the STLSQ runs in the tail (run_segment_discovery, fuse)."""
    name, wrapper, export = "sindy_fit_segments", "ops.sindy_fit_segments", "insite_sindy_fit_segments_f64"
    fd = "smoothed1"
    tolerance = "GRAM_RTOL per entry scale; support, iterations, |coef| < 1e-8 (tests/test_gpu_segments.py)"
    cases = {"b1": _seg_case(100, "high_pow"), "b16": _seg_case(2000, "high_pow"), "b17": _seg_case(2100, "high_pow"),
             "b33": _seg_case(4130, "high_pow"), "noop": _seg_case(0, "high_pow"),
             "short": _seg_case(300, "high_pow", short=True)}

    def alloc(self, dev, case):
        import torch
        c = self.cases[case]
        A, F = c["n_arms"], M.TABLE[c["name"]][0]
        return (_full(dev, (A, F), torch.float64), _full(dev, (A, F), torch.int8), _full(dev, (A,), torch.int32),
                _full(dev, (A, F, F), torch.float64), _full(dev, (A, F), torch.float64))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        c = self.cases[case]
        x, arm, sl, u = _seg_dev(dev, self._key(case))
        ops.sindy_fit_segments(x, arm, sl, u, M.DT, M.LIBS[c["name"]], THRESHOLD, ALPHA, n_arms=c["n_arms"], fd=self.fd,
                               workspace=ws, out=outs)
        return outs

    def check(self, case, outs):
        w = GramSegmentsRow.check(self, case, outs)
        check_stlsq(outs[0], outs[1], outs[2], outs[3], outs[4], (self.name, case))
        return w


class GenGramSegmentsRow(GramSegmentsRow):
    name, wrapper, export = "gen_gram_segments", "ops.gen_gram_segments", "insite_gen_gram_segments_f64"
    query = "insite_gen_gram_segments_workspace_bytes"
    contract = "none"
    tolerance = "rtol 1e-9, b atol 1e-9 max |b| (tests/test_gpu_segments_degree4.py), against oracle.segments_ref"
    cases = {"n70": _seg_case(70, "deg4", 4), "n600": _seg_case(600, "deg4", 4), "noop": _seg_case(0, "deg4", 4),
             "short": _seg_case(300, "deg4", 4, short=True)}

    @property
    def largest(self):
        return "n600"

    @staticmethod
    def lib():
        from insite_amd.library import polynomial_library
        return polynomial_library(1, 4, False)

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], c["n_arms"], self.lib().n_terms)

    def _key(self, case):
        c = self.cases[case]
        return (c["N"], c["T"], 1, c["n_arms"], c["short"], c["p_switch"])

    def alloc(self, dev, case):
        import torch
        A, F = self.cases[case]["n_arms"], self.lib().n_terms
        return (_full(dev, (A, F, F), torch.float64), _full(dev, (A, F), torch.float64))

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        x, arm, sl, u = _seg_dev(dev, self._key(case))
        ops.gen_gram_segments(x, arm, sl, u, M.DT, self.lib(), n_arms=self.cases[case]["n_arms"], fd=self.fd,
                              workspace=ws, out=outs)
        return outs

    def check(self, case, outs):
        x, u, arm, sl = seg_cohort(*self._key(case))
        Gr, br, _ = S.gram_segments(np.nan_to_num(x), u, arm, sl, M.DT, self.lib().exps.astype(np.int64),
                                    n_arms=self.cases[case]["n_arms"], fd=self.fd)
        np.testing.assert_allclose(outs[0], Gr, rtol=1e-9, atol=0)
        np.testing.assert_allclose(outs[1], br, rtol=1e-9, atol=1e-9 * np.abs(br).max())
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(outs[0] - Gr) / np.abs(Gr)
        return float(np.nanmax(r, initial=0.0)) / 1e-9


# ---- irregular grids --------------------------------------------------------------------------------------------
IRR_T = 12


@functools.lru_cache(maxsize=None)
def irr_cohort(N, short=False):
    """(x, t_obs [N, IRR_T] NaN past n_obs, n_obs, u [N, 2], arm): increasing times with steps in [0.5, 1.5] DT, the
    decay recipe on every patient's own times, n_obs in [0, IRR_T] with the edge lengths 0, 4, 5, 6, IRR_T planted;
    short: n_obs = p % 5 (below the five-sample window)."""
    rng = np.random.default_rng(M._seed("ws-irr", N, short))
    t = np.cumsum(rng.uniform(0.5, 1.5, (N, IRR_T)) * M.DT, axis=1)
    x = M._decay(rng, t, N)
    u = rng.uniform(0.6, 1.6, (N, 2))
    arm = rng.integers(0, 2, N)
    n_obs = rng.integers(0, IRR_T + 1, N)
    if N >= 5:
        n_obs[:5] = [0, 4, 5, 6, IRR_T]
    if short:
        n_obs = np.arange(N) % 5
    past = np.arange(IRR_T)[None, :] >= n_obs[:, None]
    x[past] = np.nan
    t[past] = np.nan
    return _freeze(x, t, n_obs.astype(np.int64), u, arm.astype(np.int64))


@functools.lru_cache(maxsize=None)
def irr_ref(N, short):
    return _freeze(*M.irregular_ref(*irr_cohort(N, short), M.exps_of("std7"), 2, "nonuniform4"))


@functools.lru_cache(maxsize=None)
def _irr_dev(dev, N, short):
    import torch
    x, t, n_obs, u, arm = irr_cohort(N, short)
    return _t(x, dev), _t(t, dev), _t(n_obs, dev, torch.int32), _t(u, dev), _t(arm, dev, torch.int8)


class GramIrregularRow(Row):
    name, wrapper, export = "gram_irregular", "ops.gram_irregular", "insite_gram_irregular_f64"
    query = "insite_gram_irregular_workspace_bytes"
    tolerance = ("GRAM_RTOL per entry scale, moments 1e-10 of the column maximum "
                 "(tests/test_gpu_library_matrix.py::test_irregular_gram)")
    cases = {k: dict(N=v, short=k == "short") for k, v in DISC_N.items()}
    fit = False

    def query_args(self, case):
        return (self.cases[case]["N"], 2, 7)

    def alloc(self, dev, case):
        import torch
        gb = (_full(dev, (2, 7, 7), torch.float64), _full(dev, (2, 7), torch.float64))
        fit = (_full(dev, (2, 7), torch.float64), _full(dev, (2, 7), torch.int8), _full(dev, (2,), torch.int32))
        return (fit if self.fit else ()) + gb + (_full(dev, (self.cases[case]["N"], 5), torch.float64),)

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        c = self.cases[case]
        args = _irr_dev(dev, c["N"], c["short"])
        if self.fit:
            ops.sindy_fit_irregular(*args, _lib7(), THRESHOLD, ALPHA, n_arms=2, fd="nonuniform4", workspace=ws,
                                    out=outs, moments=True)
        else:
            ops.gram_irregular(*args, _lib7(), n_arms=2, fd="nonuniform4", workspace=ws, out=outs, moments=True)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        Gr, br, SG, Sb, momr = irr_ref(c["N"], c["short"])
        G, b, mom = outs[-3], outs[-2], outs[-1]
        w = check_gram(G, b, Gr, br, SG, Sb, (self.name, case))
        assert np.array_equal(mom[:, 0], momr[:, 0])
        assert np.all(np.abs(mom - momr).max(axis=0) <= 1e-10 * np.abs(momr).max(axis=0))
        if self.fit:
            check_stlsq(outs[0], outs[1], outs[2], G, b, (self.name, case))
        return w


class SindyFitIrregularRow(GramIrregularRow):
    name, wrapper, export = "sindy_fit_irregular", "ops.sindy_fit_irregular", "insite_sindy_fit_irregular_f64"
    cases = {k: dict(N=v, short=k == "short") for k, v in DISC_N.items()}
    fit = True
    tolerance = GramIrregularRow.tolerance + "; support, iterations, |coef| < 1e-8 (tests/test_gpu_irregular.py)"


# ---- weak form --------------------------------------------------------------------------------------------------
WEAK_T = 23
WEAK_N = {"b1": 50, "b16": 1000, "b17": 1050, "b33": 2100, "noop": 0, "short": 300}


@functools.lru_cache(maxsize=None)
def weak_cohort(N, short=False):
    """library_matrix.weak_inputs at any N (std7, two arms): every 7th patient has rows = T - 1 and contributes
    nothing; short: every patient has."""
    rng = np.random.default_rng(M._seed("ws-weak", N, short))
    x = M._decay(rng, np.arange(WEAK_T) * M.DT, N)
    u = rng.uniform(0.6, 1.6, (N, 2))
    arm = rng.integers(0, 2, N)
    k = np.arange(N)
    rows = np.where(k % 7 == 2, WEAK_T - 1, WEAK_T)
    if short:
        rows[:] = WEAK_T - 1
    W, D = M.weak_weights(WEAK_T)
    x[rows < WEAK_T] = np.nan
    return _freeze(x, u, arm.astype(np.int64), rows.astype(np.int64), W, D)


@functools.lru_cache(maxsize=None)
def weak_ref(N, short):
    return _freeze(*M.weak_ref(*weak_cohort(N, short), M.exps_of("std7"), 2))


@functools.lru_cache(maxsize=None)
def _weak_dev(dev, N, short):
    import torch
    x, u, arm, rows, W, D = weak_cohort(N, short)
    return _t(x, dev), _t(W, dev), _t(D, dev), _t(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32)


class GramWeakRow(Row):
    name, wrapper, export = "gram_weak", "ops.gram_weak", "insite_gram_weak_f64"
    query = "insite_gram_weak_workspace_bytes"
    tolerance = "GRAM_RTOL per entry scale, moments too (tests/test_gpu_library_matrix.py::test_weak_gram)"
    cases = {k: dict(N=v, short=k == "short") for k, v in WEAK_N.items()}
    fit = False

    def query_args(self, case):
        return (self.cases[case]["N"], 2, 7, 33)

    alloc = GramIrregularRow.alloc

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        c = self.cases[case]
        args = _weak_dev(dev, c["N"], c["short"])
        if self.fit:
            ops.sindy_fit_weak(*args, _lib7(), THRESHOLD, optimizer="stlsq", alpha=ALPHA, max_iter=100, n_arms=2,
                               workspace=ws, out=outs, moments=True)
        else:
            ops.gram_weak(*args, _lib7(), n_arms=2, workspace=ws, out=outs, moments=True)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        Gr, br, SG, Sb, momr, Sm = weak_ref(c["N"], c["short"])
        G, b, mom = outs[-3], outs[-2], outs[-1]
        w = check_gram(G, b, Gr, br, SG, Sb, (self.name, case))
        r = M.worst_ratio(mom, momr, Sm)
        assert r <= M.GRAM_RTOL, (self.name, case, "moments", r)
        if self.fit:
            check_stlsq(outs[0], outs[1], outs[2], G, b, (self.name, case))
        return max(w, r / M.GRAM_RTOL)


class SindyFitWeakRow(GramWeakRow):
    name, wrapper, export = "sindy_fit_weak", "ops.sindy_fit_weak", "insite_sindy_fit_weak_f64"
    cases = {k: dict(N=WEAK_N[k], short=k == "short") for k in ("b1", "b17", "noop", "short")}
    fit = True
    tolerance = GramWeakRow.tolerance + "; support, iterations, |coef| < 1e-8 (tests/test_gpu_weak.py)"


# ---- bootstrap --------------------------------------------------------------------------------------------------
BOOT_MIN_ROWS, BOOT_SEED = 5, 7


@functools.lru_cache(maxsize=None)
def boot_cohort(N, short=False):
    """tests/test_gpu_bootstrap._inputs at any N: (mom [N, 5], u [N, 2], arm, rows in 3..8; short: rows = 3)."""
    rng = np.random.default_rng(M._seed("ws-boot", N, short))
    mom = BR.numpy_moments(rng, N) if N else np.zeros((0, 5))
    rows = rng.integers(3, 9, N)
    if short:
        rows[:] = 3
    return _freeze(mom, rng.uniform(0.6, 1.6, (N, 2)), rng.integers(0, 2, N), rows)


@functools.lru_cache(maxsize=None)
def boot_ref(N, Rn, short):
    return _freeze(*BR.gram(*boot_cohort(N, short), BOOT_MIN_ROWS, M.exps_of("std7"), 2, Rn, BOOT_SEED, 0))


class BootstrapGramRow(Row):
    name, wrapper, export = "bootstrap_gram", "ops.bootstrap_gram", "insite_bootstrap_gram_f64"
    query = "insite_bootstrap_workspace_bytes"
    tolerance = "GRAM_RTOL per entry scale (tests/test_gpu_bootstrap.py)"
    cases = {"rg1": dict(N=65, R=17, short=False), "rg2": dict(N=300, R=50, short=False),
             "noop": dict(N=0, R=17, short=False), "short": dict(N=130, R=17, short=True)}
    fit = False

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], 2, 7, c["R"])

    def alloc(self, dev, case):
        import torch
        Rn = self.cases[case]["R"]
        gb = (_full(dev, (Rn, 2, 7, 7), torch.float64), _full(dev, (Rn, 2, 7), torch.float64))
        fit = (_full(dev, (Rn, 2, 7), torch.float64), _full(dev, (Rn, 2, 7), torch.int8),
               _full(dev, (Rn, 2), torch.int32))
        return (fit if self.fit else ()) + gb

    def run(self, dev, case, ws, outs):
        import torch
        from insite_amd import ops
        c = self.cases[case]
        mom, u, arm, rows = boot_cohort(c["N"], c["short"])
        args = (_t(mom, dev), _t(u, dev), _t(arm, dev, torch.int8), _t(rows, dev, torch.int32), _lib7(), c["R"])
        kw = dict(seed=BOOT_SEED, n_arms=2, min_rows=BOOT_MIN_ROWS, workspace=ws, out=outs)
        if self.fit:
            ops.sindy_bootstrap(*args, THRESHOLD, optimizer="stlsq", alpha=ALPHA, **kw)
        else:
            ops.bootstrap_gram(*args, **kw)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        Gr, br, SG, Sb = boot_ref(c["N"], c["R"], c["short"])
        w = check_gram(outs[-2], outs[-1], Gr, br, SG, Sb, (self.name, case))
        if self.fit:
            check_stlsq(outs[0], outs[1], outs[2], outs[3], outs[4], (self.name, case))
        return w


class SindyBootstrapRow(BootstrapGramRow):
    name, wrapper, export = "sindy_bootstrap", "ops.sindy_bootstrap", "insite_sindy_bootstrap_f64"
    fit = True
    tolerance = BootstrapGramRow.tolerance + "; supports equal, |coef| < 1e-8 on every system"


# ---- the general one-state path -----------------------------------------------------------------------------------
class GenGramRow(Row):
    """The degree-4 library (35 terms) with two regressions; "nosteps": n_steps = 0 with patients (G = b = 0)."""
    name, wrapper, export = "gen_gram", "ops.gen_gram", "insite_gen_gram_f64"
    query = "insite_gen_gram_workspace_bytes"
    contract, noop_writes = "none", True
    tolerance = ("rtol 1e-11, atol 1e-13 of the largest entry "
                 "(tests/test_gpu_general.py::test_degree4_gram_matches_oracle)")
    cases = {"n70": dict(N=70, T=DISC_T, short=False), "n600": dict(N=600, T=DISC_T, short=False),
             "nosteps": dict(N=70, T=0, short=False),
             "noop": dict(N=0, T=DISC_T, short=False), "short": dict(N=300, T=DISC_T, short=True)}

    @property
    def largest(self):
        return "n600"

    @staticmethod
    def lib():
        from insite_amd.library import polynomial_library
        return polynomial_library(2, 4, False)

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], c["T"], 2, self.lib().n_terms)

    def alloc(self, dev, case):
        import torch
        F = self.lib().n_terms
        return (_full(dev, (2, F, F), torch.float64), _full(dev, (2, F), torch.float64))

    def run(self, dev, case, ws, outs):
        import torch
        from insite_amd import ops
        c = self.cases[case]
        x, u, arm, rows = disc_cohort(c["N"], DISC_T, c["short"])
        xd = _t(x, dev) if c["T"] else torch.zeros((c["N"], 0), dtype=torch.float64, device=dev)
        ops.gen_gram(xd, _t(u, dev), _t(rows, dev, torch.int32), M.DT, self.lib(), group=_t(arm, dev, torch.int8),
                     n_groups=2, fd=FD, workspace=ws, out=outs)
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        x, u, arm, rows = disc_cohort(c["N"], DISC_T, c["short"])
        F = self.lib().n_terms
        if c["T"] == 0 or c["N"] == 0:
            Gr, br = np.zeros((2, F, F)), np.zeros((2, F))
        else:
            Gr, br = R.gram_moments(np.nan_to_num(x), u, arm, np.minimum(rows, DISC_T), M.DT,
                                    self.lib().exps.astype(np.int64))
        worst = 0.0
        for a in range(2):
            for got, ref in ((outs[0][a], Gr[a]), (outs[1][a], br[a])):
                atol = 1e-13 * np.abs(ref).max()
                np.testing.assert_allclose(got, ref, rtol=1e-11, atol=atol)
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.abs(got - ref) / (atol + 1e-11 * np.abs(ref))
                worst = max(worst, float(np.nanmax(r, initial=0.0)))
            assert np.array_equal(outs[0][a], outs[0][a].T)
        return worst


# ---- metrics, multi-state, lane order -------------------------------------------------------------------------------
class MaskedSseRow(Row):
    name, wrapper, export = "masked_sse", "ops.masked_sse", "insite_masked_sse_f64"
    query = "insite_masked_sse_workspace_bytes"
    contract, noop_writes = "none", True   # n_rows = 0: one block sums nothing, the outputs are zeros
    tolerance = "rtol 1e-12, counts exact (tests/test_gpu_parity.py::test_masked_sse_matches_numpy)"
    T = 7
    cases = {"b1": dict(N=50, short=False), "b20": dict(N=1234, short=False), "noop": dict(N=0, short=False),
             "short": dict(N=300, short=True)}

    def query_args(self, case):
        return (self.cases[case]["N"], self.T)

    @functools.lru_cache(maxsize=None)
    def _inputs(self, N, short):
        rng = np.random.default_rng(M._seed("ws-sse", N, short))
        pred = rng.normal(size=(N, self.T + 3))
        target = rng.normal(size=(N, self.T))
        sl = rng.integers(1, self.T + 1, size=N) * (0 if short else 1)
        active = (np.arange(self.T)[None, :] < sl[:, None]).astype(np.float64)
        return _freeze(pred, target, active)

    def alloc(self, dev, case):
        return ()

    def run(self, dev, case, ws, outs):
        from insite_amd import ops
        c = self.cases[case]
        pred, target, active = self._inputs(c["N"], c["short"])
        return ops.masked_sse(_t(pred, dev), _t(target, dev), _t(active, dev), scale=2.0, shift=0.5, workspace=ws)

    def check(self, case, outs):
        c = self.cases[case]
        pred, target, active = self._inputs(c["N"], c["short"])
        T = self.T
        e = ((pred[:, :T] * 2.0 + 0.5 - target) ** 2) * active
        np.testing.assert_allclose(outs[0], e.sum(0), rtol=1e-12)
        np.testing.assert_allclose(outs[1], active.sum(0), rtol=0)
        lw = active - np.concatenate([active[:, 1:], np.zeros((c["N"], 1))], axis=1)
        want = [(((pred[:, :T] * 2 + 0.5 - target) ** 2) * lw).sum(), lw.sum()]
        np.testing.assert_allclose(outs[2], want, rtol=1e-12)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.abs(outs[0] - e.sum(0)) / np.abs(e.sum(0))
        return float(np.nanmax(r, initial=0.0)) / 1e-12


class GramMsRow(Row):
    name, wrapper, export = "gram_ms", "multistate.gram_ms", "insite_gram_ms_f32"
    query = "insite_gram_ms_workspace_bytes"
    contract, noop_writes = "none", True   # n_patients = 0: the partials are cleared and finalised, G = B = 0
    tolerance = "rtol 1e-10, atol 1e-8 (tests/test_gpu_multistate.py::test_gram_ms_matches_oracle)"
    T = 48
    cases = {"b1": dict(N=67, short=False), "b2": dict(N=300, short=False), "noop": dict(N=0, short=False),
             "short": dict(N=130, short=True)}

    def query_args(self, case):
        return (self.cases[case]["N"],)

    @functools.lru_cache(maxsize=None)
    def _inputs(self, N, short):
        x, a = MSR.c3_cohort(max(N, 1), self.T, seed=11)
        rng = np.random.default_rng(M._seed("ws-ms", N, short))
        rows = rng.integers(0, self.T + 1, max(N, 1)).astype(np.int32)
        rows[:10] = [0, 4, 5, 6, 7, 8, 9, 10, self.T, self.T - 1][:rows.size]
        if short:
            rows = (np.arange(N) % 5).astype(np.int32)
        return _freeze(x[:N], a[:N], rows[:N])

    @staticmethod
    def lib():
        from insite_amd.multistate import ms_library
        return ms_library(5, 1, True)

    def alloc(self, dev, case):
        import torch
        F = self.lib().exps.shape[0]
        return (_full(dev, (F, F), torch.float64), _full(dev, (F, 5), torch.float64))

    def run(self, dev, case, ws, outs):
        import torch
        from insite_amd import multistate as MS
        from insite_amd.ops import pack_arm_bits
        c = self.cases[case]
        N = c["N"]
        x, a, rows = self._inputs(N, c["short"])
        xd = np.full((self.T, 5, N + 3), np.nan, dtype=np.float32)
        xd[:, :, :N] = np.transpose(x, (1, 2, 0))
        bits = pack_arm_bits(_t(np.ascontiguousarray(a.T) if N else np.zeros((self.T, 1), a.dtype), dev), max(N, 1))
        return MS.gram_ms(torch.tensor(xd, device=dev), bits, self.lib(), MSR.DT_C3, rows=_t(rows, dev, torch.int32),
                          n_patients=N, workspace=ws, out=outs)

    def check(self, case, outs):
        c = self.cases[case]
        x, a, rows = self._inputs(c["N"], c["short"])
        ex = self.lib().exps.astype(np.int64)
        if c["N"]:
            Gr, Br = MSR.ms_gram(x, a, rows, MSR.DT_C3, ex)
        else:
            Gr, Br = np.zeros((ex.shape[0],) * 2), np.zeros((ex.shape[0], 5))
        assert np.allclose(outs[0], Gr, rtol=1e-10, atol=1e-8) and np.allclose(outs[1], Br, rtol=1e-10, atol=1e-8)
        return float(np.max(np.abs(outs[0] - Gr) / (1e-8 + 1e-10 * np.abs(Gr))))


class Rk45OrderRow(Row):
    """ops.rk45_order takes no workspace argument: the export is called through _lib with the matrix's buffer."""
    name, wrapper, export = "rk45_order", "ops.rk45_order", "insite_rk45_order_i32"
    query = "insite_rk45_order_workspace_bytes"
    contract, canonical = "self_zeroed", True
    tolerance = ("the key sequence of numpy's stable sort, exactly "
                 "(tests/test_gpu_rk45.py::test_rk45_order_is_a_binned_permutation)")
    T_MAX = 24
    cases = {"b1": dict(N=100, short=False), "b2": dict(N=5000, short=False), "noop": dict(N=0, short=False),
             "short": dict(N=300, short=True)}

    def query_args(self, case):
        return (self.T_MAX,)

    @functools.lru_cache(maxsize=None)
    def _inputs(self, N, short):
        rng = np.random.default_rng(M._seed("ws-order", N, short))
        n = rng.integers(-2, self.T_MAX + 5, N).astype(np.int32)
        if short:
            n = (np.arange(N) % 2).astype(np.int32)
        return _freeze(n)[0]

    def keys(self, n):
        return np.clip(n, 0, min(self.T_MAX, 1023))

    def alloc(self, dev, case):
        import torch
        return (_full(dev, (self.cases[case]["N"],), torch.int32),)

    def run(self, dev, case, ws, outs):
        import ctypes
        import torch
        from insite_amd import _lib
        c = self.cases[case]
        n = _t(self._inputs(c["N"], c["short"]), dev, torch.int32)
        buf = ws.get(self.need(case), dev)
        st = _lib.load().insite_rk45_order_i32(ctypes.c_void_p(n.data_ptr()), c["N"], self.T_MAX,
                                               ctypes.c_void_p(outs[0].data_ptr()), ctypes.c_void_p(buf.data_ptr()),
                                               buf.numel(),
                                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _lib.check(self.export, st)
        return outs

    def canonical_outs(self, dev, case, outs):
        """(the keys in output order, the sorted permutation): what every valid order of the rows shares."""
        import torch
        c = self.cases[case]
        o = outs[0].cpu().numpy()
        if not c["N"]:
            return outs
        key = self.keys(self._inputs(c["N"], c["short"]))[np.clip(o, 0, c["N"] - 1)]
        return (_t(key, dev, torch.int32), _t(np.sort(o), dev, torch.int32))

    def check(self, case, outs):
        c = self.cases[case]
        n = self._inputs(c["N"], c["short"])
        o = outs[0]
        assert np.array_equal(np.sort(o), np.arange(c["N"]))
        key = self.keys(n)
        assert np.array_equal(key[o], key[np.argsort(-key, kind="stable")])
        return 0.0


# ---- the ensemble calls: cohort effect and policy value -----------------------------------------------------------
ENS_T, ENS_G, ENS_Q = 8, 3, (0.0, 1.0, 0.5, 0.025)
ENS_CASES = {"c1_r2": dict(N=40, R=2, short=False), "c1_r65": dict(N=40, R=65, short=False),
             "c3_r2": dict(N=130, R=2, short=False), "c3_r65": dict(N=130, R=65, short=False),
             "noop": dict(N=0, R=65, short=False), "short": dict(N=70, R=65, short=True)}


def _ens_plans(rng, N, T, A, pad=3):
    """Per-step arms [N, T + pad] of two plans (the recipe of tests/test_gpu_effect.py): random, with a switch at step
    1 and at step T - 1 in every row; the columns past T hold out-of-range arms, which no call may read."""
    out = []
    for _ in range(2):
        arm = rng.integers(0, A, (N, T + pad))
        if A > 1 and T >= 2:
            arm[:, 1] = (arm[:, 0] + 1) % A
            arm[:, T - 1] = (arm[:, T - 2] + 1) % A
        arm[:, T:] = [A + 3, -2, 127][:pad]
        out.append(arm.astype(np.int8))
    return out


def _ens_coef(rng, name, Rn, A):
    """[R, A, F] (the recipe of tests/test_gpu_effect.py): a decaying model (state-exponent-1 terms negative, |c| in
    [0.05, 0.15]) and bootstrap-like replicates of it: every coefficient scaled by 1 + 0.3 z, one term in five outside
    the replicate's support, the last column of the last arm below drop_below in replicate 1."""
    exps = M.exps_of(name)
    F = exps.shape[0]
    base = rng.uniform(0.05, 0.15, (A, F)) * np.where(exps[:, 0] > 0, -1.0, rng.choice([-1.0, 1.0], (A, F)))
    coef = base[None] * (1.0 + 0.3 * rng.normal(size=(Rn, A, F)))
    coef[rng.random((Rn, A, F)) < 0.2] = 0.0
    coef[0] = base
    coef[1, A - 1, F - 1] = 0.5 * M.DROP_BELOW
    return coef


@functools.lru_cache(maxsize=None)
def cohort_inputs(N, Rn, short):
    """The inputs of tests/test_gpu_cohort_effect.py at any shape (std7, two arms), group = p % 3; short: every group
    id is -1, so no row contributes."""
    rng = np.random.default_rng(M._seed("ws-cohort", N, Rn, short))
    y0 = rng.uniform(0.5, 3.0, N)
    u = rng.uniform(0.6, 1.6, (N, 2))
    arm_a, arm_b = _ens_plans(rng, N, ENS_T, 2)
    coef = _ens_coef(rng, "std7", Rn, 2)
    group = (np.arange(N) % ENS_G).astype(np.int32)
    if short:
        group[:] = -1
    return _freeze(y0, u, arm_a, arm_b, coef, group)


@functools.lru_cache(maxsize=None)
def cohort_ref(N, Rn, short):
    y0, u, arm_a, arm_b, coef, group = cohort_inputs(N, Rn, short)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _freeze(*CR.cohort(y0, u, arm_a[:, :ENS_T], arm_b[:, :ENS_T], coef, M.exps_of("std7"), 0.1, ENS_Q, group,
                                  ENS_G, "poisson", BOOT_SEED, 0, "euler", 5))


class CohortSumsRow(Row):
    name, wrapper, export = "cohort_effect_sums", "ops.cohort_effect_sums", "insite_cohort_effect_sums_f64"
    query = "insite_cohort_effect_workspace_bytes"
    contract = "none"
    query_zero = ("noop",)   # insite_cohort.h: the query is 0 for n_rows = 0 (nothing is launched)
    tolerance = "1e-10 of the trajectory scale, wsum exact (tests/test_gpu_cohort_effect.py::test_parity)"
    cases = ENS_CASES
    full = False

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], ENS_T, 2, 7, c["R"], ENS_G)

    def alloc(self, dev, case):
        import torch
        Rn = self.cases[case]["R"]
        sums = (_full(dev, (Rn, ENS_G, 2, ENS_T), torch.float64), _full(dev, (Rn, ENS_G), torch.float64))
        return ((_full(dev, (ENS_G, 3, 3 + len(ENS_Q), ENS_T), torch.float64),) if self.full else ()) + sums

    def run(self, dev, case, ws, outs):
        import torch
        from insite_amd import ops
        c = self.cases[case]
        y0, u, arm_a, arm_b, coef, group = cohort_inputs(c["N"], c["R"], c["short"])
        args = (_t(y0, dev), _t(u, dev), _t(arm_a, dev, torch.int8), _t(arm_b, dev, torch.int8), _t(coef, dev), _lib7(),
                0.1)
        kw = dict(group=_t(group, dev, torch.int32), n_groups=ENS_G, weighting="poisson", seed=BOOT_SEED,
                  method="euler", substeps=5, drop_below=M.DROP_BELOW, T=ENS_T, workspace=ws)
        if not self.full:
            ops.cohort_effect_sums(*args, out=outs, **kw)
            return outs
        # ops.cohort_effect allocates sums / wsum itself: they are copied into the matrix's outputs
        got = ops.cohort_effect(*args, ENS_Q, out=outs[0], **kw)
        if c["N"]:
            outs[1].copy_(got[1])
            outs[2].copy_(got[2])
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        ref, S_ref, w_ref, scale = cohort_ref(c["N"], c["R"], c["short"])
        sums, wsum = outs[-2], outs[-1]
        assert np.array_equal(wsum, w_ref), (self.name, case)
        w = rel_err(sums, S_ref, (scale[None, :, None, :] * np.maximum(w_ref, 1.0)[:, :, None, None]))
        if self.full:
            w = max(w, rel_err(outs[0], ref, scale[:, None, None, :]))
        assert w <= ENSEMBLE_TOL, (self.name, case, w)
        return w / ENSEMBLE_TOL


class CohortEffectRow(CohortSumsRow):
    name, wrapper, export = "cohort_effect", "ops.cohort_effect", "insite_cohort_effect_f64"
    full = True


POL_K = 3


@functools.lru_cache(maxsize=None)
def policy_inputs(N, Rn, short):
    y0, u, plans, w, cost, coef, group, _ = P.inputs(("ws-policy", N, Rn, short), Rn, N, ENS_T, 2, POL_K, ENS_G, "std7")
    if short:
        group = np.full(N, -1, dtype=np.int32)
    return _freeze(y0, u, plans, w, cost, coef, group)


@functools.lru_cache(maxsize=None)
def policy_ref(N, Rn, short):
    import regimen_ref as G
    y0, u, plans, w, cost, coef, group = policy_inputs(N, Rn, short)
    with np.errstate(invalid="ignore", divide="ignore"):
        return P.policy(y0, u, G.full_plans(plans, N, ENS_T), coef, M.exps_of("std7"), P.DT, ENS_Q, w[..., :ENS_T],
                        cost, 1, None, group, ENS_G, "poisson", P.SEED, 0, "euler", 5)


class PolicySumsRow(Row):
    name, wrapper, export = "policy_sums", "ops.policy_sums", "insite_policy_sums_f64"
    query = "insite_policy_workspace_bytes"
    contract = "none"
    query_zero = ("noop",)   # insite_policy.h: the query is 0 for n_rows = 0
    tolerance = ("1e-10 of the objective scale, wsum exact, the rule exact where the reference's argmin margin is "
                 "at least 1e-8 (tests/test_gpu_policy.py::test_parity)")
    cases = ENS_CASES
    full = False

    def query_args(self, case):
        c = self.cases[case]
        return (c["N"], ENS_T, 2, 7, c["R"], ENS_G, POL_K)

    def alloc(self, dev, case):
        import torch
        c = self.cases[case]
        sums = (_full(dev, (c["R"], ENS_G, 2 * POL_K + 2), torch.float64), _full(dev, (c["R"], ENS_G), torch.float64))
        rule = (_full(dev, (c["N"],), torch.int32),)
        return ((_full(dev, (ENS_G, 2 * POL_K + 6, 3 + len(ENS_Q)), torch.float64),) if self.full else ()) + sums + rule

    def run(self, dev, case, ws, outs):
        import torch
        from insite_amd import ops
        c = self.cases[case]
        y0, u, plans, w, cost, coef, group = policy_inputs(c["N"], c["R"], c["short"])
        args = (_t(y0, dev), _t(u, dev), _t(plans, dev, torch.int8), _t(coef, dev), _lib7(), P.DT)
        kw = dict(cost=_t(cost, dev), group=_t(group, dev, torch.int32), n_groups=ENS_G, weighting="poisson",
                  seed=P.SEED, method="euler", substeps=5, drop_below=M.DROP_BELOW, T=ENS_T, workspace=ws)
        # the wrappers allocate the rule (and, for policy_value, sums / wsum): copied into the matrix's outputs
        if not self.full:
            got = ops.policy_sums(*args, _t(w, dev), out=outs[:2], **kw)
            if c["N"]:
                outs[2].copy_(got[2])
            return outs
        got = ops.policy_value(*args, ENS_Q, _t(w, dev), out=outs[0], **kw)
        if c["N"]:
            outs[1].copy_(got[4])
            outs[2].copy_(got[5])
            outs[3].copy_(got[3])
        return outs

    def check(self, case, outs):
        c = self.cases[case]
        ref = policy_ref(c["N"], c["R"], c["short"])
        sums, wsum, rule = outs[-3], outs[-2], outs[-1]
        K, s = POL_K, ref["scale"]
        assert np.array_equal(wsum, ref["wsum"]), (self.name, case)
        if ref["row_margin"] >= 1e-8:
            assert np.array_equal(rule, ref["rule"]), (self.name, case)
        w = rel_err(sums[:, :, :K + 2], ref["sums"][:, :, :K + 2],
                    (s[None, :] * np.maximum(ref["wsum"], 1.0))[:, :, None])
        if self.full and ref["row_margin"] >= 1e-8 and ref["fixed_margin"] >= 1e-8:
            w = max(w, rel_err(outs[0][:, :K + 6], ref["out"][:, :K + 6], s[:, None, None]))
        assert w <= ENSEMBLE_TOL, (self.name, case, w)
        return w / ENSEMBLE_TOL


class PolicyValueRow(PolicySumsRow):
    name, wrapper, export = "policy_value", "ops.policy_value", "insite_policy_value_f64"
    full = True


ROWS = [GramRow(), SindyFitRow(), GramMomentsRow(), FitRolloutRow(), DeferredRow(), LaggedRow(), GramSegmentsRow(),
        SindyFitSegmentsRow(), PerPatientRow(), GenGramSegmentsRow(), GenGramRow(), MaskedSseRow(), GramMsRow(),
        Rk45OrderRow(), GramIrregularRow(), SindyFitIrregularRow(), GramWeakRow(), SindyFitWeakRow(),
        BootstrapGramRow(), SindyBootstrapRow(), CohortSumsRow(), CohortEffectRow(), PolicySumsRow(), PolicyValueRow()]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# every *_workspace_bytes export without a row, with its reason
NO_WORKSPACE = {
    "insite_effect_workspace_bytes": "insite_effect.h: this version needs no workspace, the query returns 0",
    "insite_regimen_workspace_bytes": "insite_regimen.h: this version needs no workspace, the query returns 0",
}
# arguments for which a header documents a query result of 0: (query, arguments)
ZERO_QUERIES = [
    ("insite_gram_workspace_bytes", (-1, 2, 7)), ("insite_gram_workspace_bytes", (10, 5, 7)),
    ("insite_gram_segments_workspace_bytes", (10, 0, 4)), ("insite_gram_irregular_workspace_bytes", (-1, 2, 7)),
    ("insite_gram_weak_workspace_bytes", (10, 2, 7, 0)), ("insite_bootstrap_workspace_bytes", (10, 2, 7, 0)),
    ("insite_per_patient_workspace_bytes", (-1,)), ("insite_cohort_effect_workspace_bytes", (0, 8, 2, 7, 65, 3)),
    ("insite_policy_workspace_bytes", (0, 8, 2, 7, 65, 3, 3)), ("insite_effect_workspace_bytes", (10, 8, 2, 7, 65, 4)),
    ("insite_regimen_workspace_bytes", (10, 8, 2, 7, 65, 4, 3)), ("insite_gen_gram_workspace_bytes", (10, 9, 0, 35)),
    ("insite_masked_sse_workspace_bytes", (-1, 7)),
]

CASES = [(r.name, c) for r in ROWS for c in r.cases]
