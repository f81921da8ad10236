"""Test functions of the weak-form discovery (``include/insite_weak.h``).

The grid is uniform, t_i = i dt for i = 0..T-1, L = (T - 1) dt.  Subdomain k has centre c_k and half-width H;
its test function is phi_k(t) = (1 - tau^2)^p with tau = (t - c_k) / H, integrated over the grid points with
|t_i - c_k| <= H by the rectangle rule:

    W[k, i] = dt (1 - tau^2)^p                       (weights of phi_k)
    D[k, i] = dt (-2 p tau (1 - tau^2)^(p-1)) / H    (weights of phi_k')

and zero outside the subdomain.  The defaults are the reference's (pysindy ``WeakPDELibrary(K=100)``): p = 4,
H = L / 20, centres uniform in [H, L - H].  The C entry points take W and D as dense matrices, so any other
test function or quadrature can be passed instead.
"""
from __future__ import annotations

import numpy as np
import torch

DEFAULT_K, DEFAULT_P = 100, 4


def default_half_width(T: int, dt: float) -> float:
    """H = L / 20 with L = (T - 1) dt."""
    return (int(T) - 1) * float(dt) / 20.0


def draw_centres(T: int, dt: float, K: int = DEFAULT_K, seed=None, H: float | None = None) -> np.ndarray:
    """K subdomain centres: exactly ``numpy.random.default_rng(seed).uniform(H, L - H, K)``."""
    L = (int(T) - 1) * float(dt)
    H = default_half_width(T, dt) if H is None else float(H)
    return np.random.default_rng(seed).uniform(H, L - H, int(K))


def test_function_weights(T: int, dt: float, centres, H: float | None = None, p: int = DEFAULT_P, device=None):
    """(W, D), float64 tensors [K, T], for the given centres (array or tensor [K]) on ``device`` (default: the
    device of ``centres`` when it is a tensor, else the current HIP device, else the CPU)."""
    if T < 2 or not dt > 0 or p < 1:
        raise ValueError("test_function_weights needs T >= 2, dt > 0 and p >= 1")
    if device is None:
        device = centres.device if isinstance(centres, torch.Tensor) else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    c = torch.as_tensor(np.asarray(centres, dtype=np.float64) if not isinstance(centres, torch.Tensor) else centres,
                        dtype=torch.float64, device=device).reshape(-1)
    H = default_half_width(T, dt) if H is None else float(H)
    if not H > 0:
        raise ValueError("the half-width H must be positive")
    t = torch.arange(int(T), dtype=torch.float64, device=device) * float(dt)
    tau = (t[None, :] - c[:, None]) / H
    inside = (t[None, :] - c[:, None]).abs() <= H
    q = 1.0 - tau * tau
    zero = torch.zeros((), dtype=torch.float64, device=device)
    W = torch.where(inside, float(dt) * q ** p, zero)
    D = torch.where(inside, float(dt) * (-2.0 * p * tau * q ** (p - 1)) / H, zero)
    return W.contiguous(), D.contiguous()


test_function_weights.__test__ = False   # (not a pytest test, whatever module imports it)
