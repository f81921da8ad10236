#!/usr/bin/env python
"""Time the patient-level bootstrap (ops.sindy_bootstrap: Poisson weights made on chip, R x N x entries on the f64
MFMA, batched STLSQ) beside the composition it replaces, in one process.

Workload: N patients (default 1M and 100k), R = 1024 replicates, the std7 library, 2 arms; the per-patient moments
come from one ops.gram_moments pass over a synthetic cohort (T = 60).  Prepared plans, device events, warm-up then
``--steps`` rounds.  Timed:
  bootstrap   ops.plan_sindy_bootstrap (Gram pass + STLSQ of the R n_arms systems), and ops.plan_bootstrap_gram alone
  torch       the same weights MATERIALISED as an f64 [R, N] tensor (built once on the device by a torch restatement
              of the Threefry block; its build time is reported, not counted), the per-patient entries [N, A nE]
              (built once, not counted), then per call torch.matmul(W, E), the unpacking to G | b and ops.stlsq.
              Leaving the weight and entry builds out favours the composition: it is the bar.
The tool checks that the materialised weights are the package's (``bootstrap.weights``) on a slice and that G | b of
both paths agree (largest difference over the largest entry <= 1e-10), and exits non-zero otherwise.
Dense flops of the kernel: 2 R_pad N 16 n_tiles (the MFMAs it issues; useful: 2 R N A nE) against the 78.6 TF f64
MFMA peak the project uses; Threefry blocks: one per replicate row, patient pair and column chunk.  One JSON line per
shape, also written to ``--out`` (default ``profiles/bootstrap/bench_bootstrap.jsonl``, rewritten by every full run;
``--bootstrap-only`` writes nothing).

    python tools/bench_bootstrap.py [--patients 1000000 100000] [--replicates 1024] [--steps 20] [--warmup 5] [--bootstrap-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

MFMA_F64_PEAK = 78.6e12  # flop/s, MI355X f64 matrix
_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
_M32 = 0xFFFFFFFF


def timed(call, steps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def device_weights(seed, R, N, offset, dev, chunk=32):
    """``insite_amd.bootstrap.weights`` as an f64 [R, N] device tensor (int64 torch arithmetic, ``chunk`` replicates
    at a time)."""
    import torch
    from insite_amd import bootstrap
    g = offset + torch.arange(N, device=dev, dtype=torch.int64)
    q = g >> 1
    x0, x1, odd = (q & _M32)[None], ((q >> 32) & _M32)[None], (g & 1).bool()[None]
    thr = [int(v) for v in bootstrap.poisson_thresholds()]
    W = torch.empty((R, N), dtype=torch.float64, device=dev)
    for r0 in range(0, R, chunk):
        k1 = torch.arange(r0, min(R, r0 + chunk), device=dev, dtype=torch.int64)[:, None]
        k0 = torch.full_like(k1, int(seed))
        ks = (k0, k1, k0 ^ k1 ^ 0x1BD11BDA)
        a, b = (x0 + ks[0]) & _M32, (x1 + ks[1]) & _M32
        for i in range(5):
            for rot in _ROT[i % 2]:
                a = (a + b) & _M32
                b = (((b << rot) | (b >> (32 - rot))) & _M32) ^ a
            a = (a + ks[(i + 1) % 3]) & _M32
            b = (b + ks[(i + 2) % 3] + (i + 1)) & _M32
        v = torch.where(odd, b, a)
        w = torch.zeros_like(v)
        for t in thr:
            w += v >= t
        W[r0:r0 + k1.numel()] = w.to(torch.float64)
    W[0] = 1.0
    return W


def entries(mom, u, arm, rows, min_rows, lib, n_arms):
    """E [N, n_arms nE] (arm-major; upper triangle then b, as the kernel's columns) and the unpacking indices."""
    import torch
    dev = mom.device
    F = lib.n_terms
    ex = torch.as_tensor(lib.exps[:, 0].astype("int64"), device=dev)
    m = torch.ones((mom.size(0), F), dtype=torch.float64, device=dev)
    for j in range(F):
        for i in range(lib.n_statics):
            for _ in range(int(lib.exps[j, 1 + i])):
                m[:, j] = m[:, j] * u[:, i]
    ii, kk = torch.triu_indices(F, F, device=dev)
    g = m[:, ii] * m[:, kk] * mom[:, ex[ii] + ex[kk]]
    h = m * mom[:, 3 + ex]
    e = torch.cat([g, h], dim=1)                                                   # [N, nE]
    on = (arm >= 0) & (arm < n_arms) & (rows >= min_rows)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    E = torch.cat([torch.where((on & (arm == a))[:, None], e, zero) for a in range(n_arms)], dim=1)
    return E.contiguous(), ii, kk


def one_shape(N, R, a, dev):
    import torch
    from insite_amd import _lib, bootstrap, cohort, ops
    c = cohort.synthetic_pkpd(N, 60, 500, dev, layout="time")
    lib, n_arms, seed, min_rows = c.lib, 2, 7, 5
    mom = ops.gram_moments(c.x, c.u, c.arm, c.rows, c.dt, lib, n_arms=n_arms, layout="time")[5]
    F = lib.n_terms
    nE = F * (F + 1) // 2 + F
    ncol = n_arms * nE
    n_tiles = (ncol + 15) // 16
    n_z = (n_tiles + 4) // 5
    ct = (n_tiles + n_z - 1) // n_z
    rt = 3 if ct == 5 else 4
    r_pad = (R + 16 * rt - 1) // (16 * rt) * 16 * rt
    res = {"tool": "bench_bootstrap", "patients": N, "replicates": R, "library": "std7", "n_arms": n_arms,
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "workspace_bytes": int(_lib.load().insite_bootstrap_workspace_bytes(N, n_arms, F, R))}

    plan = ops.plan_sindy_bootstrap(mom, c.u, c.arm, c.rows, lib, R, a.threshold, alpha=a.alpha, seed=seed,
                                    n_arms=n_arms, min_rows=min_rows)
    ms = timed(plan, a.steps, a.warmup)
    gplan = ops.plan_bootstrap_gram(mom, c.u, c.arm, c.rows, lib, R, seed=seed, n_arms=n_arms, min_rows=min_rows)
    ms_g = timed(gplan, a.steps, a.warmup)
    dense = 2.0 * r_pad * N * 16 * n_z * ct
    res["bootstrap"] = {"ms_per_call": ms, "gram_only_ms": ms_g, "dense_flops": dense,
                        "useful_flops": 2.0 * R * N * ncol,
                        "dense_fraction_of_f64_mfma_peak": dense / (ms_g * 1e-3) / MFMA_F64_PEAK,
                        "threefry_blocks": r_pad * (N / 2.0) * n_z,
                        "threefry_blocks_per_s": r_pad * (N / 2.0) * n_z / (ms_g * 1e-3)}

    if a.bootstrap_only:
        print(json.dumps(res), flush=True)
        return
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    W = device_weights(seed, R, N, 0, dev)
    t1.record()
    torch.cuda.synchronize()
    n_chk = min(N, 300)
    import numpy as np
    if not np.array_equal(W[:, :n_chk].cpu().numpy(), bootstrap.weights(seed, R, n_chk).astype(np.float64)):
        raise SystemExit("the materialised weights are not bootstrap.weights")
    E, ii, kk = entries(mom, c.u, c.arm, c.rows, min_rows, lib, n_arms)
    G = torch.zeros((R, n_arms, F, F), dtype=torch.float64, device=dev)
    nT = ii.numel()

    def torch_run():
        P = torch.matmul(W, E).view(R, n_arms, nE)
        G[:, :, ii, kk] = P[:, :, :nT]
        G[:, :, kk, ii] = P[:, :, :nT]
        b = P[:, :, nT:].contiguous()
        return G, b, ops.stlsq(G, b, a.threshold, a.alpha)

    ms_t = timed(torch_run, a.steps, a.warmup)
    ms_mm = timed(lambda: torch.matmul(W, E), a.steps, a.warmup)
    G_t, b_t, (coef_t, mask_t, _) = torch_run()
    coef, mask, _, G_k, b_k = plan()
    torch.cuda.synchronize()
    agree = float(max((G_t - G_k).abs().max(), (b_t - b_k).abs().max()) / G_k.abs().max())
    res["torch_composition"] = {"ms_per_call": ms_t, "matmul_only_ms": ms_mm, "weights_build_ms": t0.elapsed_time(t1),
                                "weights_bytes": float(R) * N * 8, "speedup_of_bootstrap": ms_t / ms,
                                "gram_max_diff_of_largest_entry": agree,
                                "masks_equal": bool(torch.equal(mask.view(-1, F), mask_t)),
                                "coef_max_diff": float((coef.view(-1, F) - coef_t).abs().max())}
    res["inclusion"] = (mask[1:] != 0).double().mean(0).cpu().numpy().tolist()
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    if not agree <= 1e-10:
        raise SystemExit(f"G | b of the two paths differ by {agree:.3e} of the largest entry")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--replicates", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--bootstrap-only", action="store_true", help="time the kernel path only (A/B builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap", "bench_bootstrap.jsonl"),
                    help="file that receives the JSON lines of a full run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bootstrap needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.bootstrap_only:
        a.out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for N in a.patients:
        one_shape(N, a.replicates, a, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
