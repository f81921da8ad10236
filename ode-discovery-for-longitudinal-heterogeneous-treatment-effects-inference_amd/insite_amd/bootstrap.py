"""Patient-level Poisson bootstrap of the discovered equations (include/insite_bootstrap.h).

The hot path is ``ops.sindy_bootstrap`` (the weights are generated inside the kernel and never exist in memory).
This module holds what surrounds it: the threshold table and a restatement of the weights for users who want to
inspect a draw (``weights``: small N only, it materialises [R, N]), and the summary of the replicates' coefficients
(``summarize``: torch reductions on the device the coefficients live on).

The resampling unit is the patient, not the row: replicate r weighs every row of patient p with the same Poisson(1)
count w_rp.  Replicate 0 has weight 1 everywhere, so it is the point estimate; the statistics run over the
replicates 1..R-1.
"""
from __future__ import annotations

import dataclasses
from fractions import Fraction

import numpy as np
import torch

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
N_THRESHOLDS = 12


def poisson_thresholds() -> np.ndarray:
    """T_k = floor(2^32 sum_{i <= k} e^-1 / i!), k = 0..11, as uint64 (every value is below 2^32): the table of
    insite_bootstrap.h.  A weight is w = #{k : v >= T_k} for a uniform 32-bit word v.  1 / e is summed as the
    alternating series in exact rationals (80 terms: far below the gap between any 2^32 CDF_k and an integer)."""
    inv_e = sum(Fraction((-1) ** n, _factorial(n)) for n in range(80))
    out, cdf = [], Fraction(0)
    for k in range(N_THRESHOLDS):
        cdf += inv_e / _factorial(k)
        out.append((cdf * 2 ** 32).__floor__())
    return np.array(out, dtype=np.uint64)


def _factorial(n: int) -> int:
    f = 1
    for i in range(2, n + 1):
        f *= i
    return f


def _threefry2x32(k0, k1, x0, x1):
    """Threefry-2x32-20 (Salmon et al., SC'11; the block function of csrc/insite_rng.hip) on uint32 arrays."""
    k0 = np.uint32(k0)
    k1 = np.asarray(k1, dtype=np.uint32)
    ks = (k0, k1, (k0 ^ k1 ^ np.uint32(0x1BD11BDA)).astype(np.uint32))
    with np.errstate(over="ignore"):
        a = (np.asarray(x0, dtype=np.uint32) + ks[0]).astype(np.uint32)
        b = (np.asarray(x1, dtype=np.uint32) + ks[1]).astype(np.uint32)
        for g in range(5):
            for r in _ROT[g % 2]:
                a = (a + b).astype(np.uint32)
                b = (((b << np.uint32(r)) | (b >> np.uint32(32 - r))).astype(np.uint32)) ^ a
            a = (a + ks[(g + 1) % 3]).astype(np.uint32)
            b = (b + ks[(g + 2) % 3] + np.uint32(g + 1)).astype(np.uint32)
    return a, b


def weights(seed: int, n_replicates: int, n_patients: int, patient_offset: int = 0) -> np.ndarray:
    """The weights the kernel draws, int64 [R, N]: row 0 all ones; for r >= 1 and g = patient_offset + p the word
    v = (a if g even else b) of Threefry-2x32-20(key (seed, r), counter (q & 0xffffffff, q >> 32)), q = g >> 1,
    counted against ``poisson_thresholds()``.  Integer work only: equal to the device's bit for bit."""
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed must be a uint32")
    R, N = int(n_replicates), int(n_patients)
    if R < 1 or N < 0 or int(patient_offset) < 0:
        raise ValueError("n_replicates >= 1, n_patients >= 0 and patient_offset >= 0 expected")
    g = int(patient_offset) + np.arange(N, dtype=np.uint64)
    q = g >> np.uint64(1)
    x0 = (q & np.uint64(0xFFFFFFFF)).astype(np.uint32)[None, :]
    x1 = (q >> np.uint64(32)).astype(np.uint32)[None, :]
    r = np.arange(R, dtype=np.uint32)[:, None]
    a, b = _threefry2x32(seed, r, np.broadcast_to(x0, (R, N)), np.broadcast_to(x1, (R, N)))
    v = np.where((g & np.uint64(1))[None, :] == 0, a, b).astype(np.uint64)
    w = (v[..., None] >= poisson_thresholds()[None, None, :]).sum(-1).astype(np.int64)
    w[0] = 1
    return w


@dataclasses.dataclass
class BootstrapResult:
    """``point`` [A, F]: replicate 0 (every weight 1).  ``inclusion`` [A, F]: the share of the replicates 1..R-1
    whose support holds the term.  ``mean``, ``std`` [A, F] (std with the n - 1 divisor) and ``quantiles`` [Q, A, F]
    (linear interpolation, ``torch.quantile``) over the coefficients of the replicates 1..R-1 (a term outside a
    replicate's support counts with its coefficient 0).  ``coef`` [R, A, F], ``mask`` [R, A, F]: every replicate.
    With R = 1 there is no resample: inclusion, mean, std and quantiles are NaN."""
    point: torch.Tensor
    inclusion: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    quantiles: torch.Tensor
    coef: torch.Tensor
    mask: torch.Tensor
    q: tuple
    seed: int | None = None

    @property
    def n_replicates(self) -> int:
        return int(self.coef.size(0))


def summarize(coef: torch.Tensor, mask: torch.Tensor, quantiles=(0.025, 0.5, 0.975), seed: int | None = None):
    """Summary of bootstrap coefficients coef [R, A, F] and supports mask [R, A, F] (``ops.sindy_bootstrap``)."""
    if coef.dim() != 3 or tuple(mask.shape) != tuple(coef.shape):
        raise ValueError("coef and mask must both be [R, n_arms, F]")
    q = tuple(float(v) for v in quantiles)
    if any(not 0.0 <= v <= 1.0 for v in q):
        raise ValueError("quantiles must lie in [0, 1]")
    R = coef.size(0)
    rep = coef[1:]
    qt = torch.as_tensor(q, dtype=coef.dtype, device=coef.device)
    if R > 1:
        inclusion = (mask[1:] != 0).to(coef.dtype).mean(0)
        mean = rep.mean(0)
        std = rep.std(0, unbiased=True) if R > 2 else torch.full_like(mean, float("nan"))
        quant = torch.quantile(rep, qt, dim=0)
    else:
        nan = torch.full_like(coef[0], float("nan"))
        inclusion, mean, std = nan, nan.clone(), nan.clone()
        quant = nan[None].expand(len(q), -1, -1).clone()
    return BootstrapResult(point=coef[0], inclusion=inclusion, mean=mean, std=std, quantiles=quant, coef=coef,
                           mask=mask, q=q, seed=seed)
