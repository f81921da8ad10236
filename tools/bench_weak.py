#!/usr/bin/env python
"""Time the weak-form discovery (ops.sindy_fit_weak: test-function projections on the f64 MFMA, per-arm Gram, SR3)
beside the composition it replaces and the strong-form fit at the same shape, in one process.

Workload: N patients x T steps f64 time-major, K test functions (default 100k x 200, K = 100), two cohorts
rotating (together larger than the 256 MiB Infinity Cache), prepared plans, device events, warm-up then
``--steps`` rounds.  Timed, in this order:
  weak        ops.plan_sindy_fit_weak (one Gram pass + SR3; a, d never reach HBM), rows of W | D sorted by centre
              (the kernel skips all-zero 16-row tiles), and the same with the rows in the draw's order
  torch       a = W @ x, d = -(D @ x) (torch.matmul, [K, N] each written to HBM), the five moment reductions over
              k, the per-arm expansion to G | b (the statics' monomials, one small matmul) and ops.stlsq
  uniform     ops.plan_sindy_fit (strong form, smoothed4) on the same arrays, as context
Useful flops of the weak pass: 2 matrices x 2 K T N; the f64 MFMA peak is the 78.6 TF the project uses for C3
(DESIGN.md §5); algorithmic bytes: 8 N T (x read once) + the per-patient statics, arm and rows.  Prints one JSON
line.

    python tools/bench_weak.py [--patients 100000] [--T 200] [--K 100] [--steps 20] [--warmup 5] [--weak-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

HBM_PEAK = 8.0e12        # B/s, MI355X
MFMA_F64_PEAK = 78.6e12  # flop/s, MI355X f64 matrix


def timed(calls, steps, warmup):
    """ms per call of the callables called round robin: ``steps`` rounds after ``warmup`` rounds."""
    import torch
    for _ in range(warmup):
        for c in calls:
            c()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        for c in calls:
            c()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (steps * len(calls))


def torch_composition(c, x, W, D, lib, n_arms, threshold, alpha):
    """The unfused form: both projections to HBM, moment reductions, per-arm expansion, STLSQ."""
    import torch
    from insite_amd import ops
    N = c.arm.numel()
    exps = torch.as_tensor(lib.exps.astype("int64"), device=x.device)
    ex = exps[:, 0]
    cvec = W.sum(dim=1)
    onehot = torch.stack([(c.arm == a) for a in range(n_arms)]).to(torch.float64)      # [A, N]
    F = lib.n_terms
    ii, jj = torch.meshgrid(torch.arange(F, device=x.device), torch.arange(F, device=x.device), indexing="ij")

    def run():
        xs = x[:, :N]
        a = torch.matmul(W, xs)
        d = -torch.matmul(D, xs)
        mom = torch.stack([(cvec * cvec).sum().expand(N), (cvec[:, None] * a).sum(0), (a * a).sum(0),
                           (cvec[:, None] * d).sum(0), (a * d).sum(0)])               # [5, N]
        m = torch.ones((F, N), dtype=torch.float64, device=x.device)
        for j in range(F):
            for i in range(lib.n_statics):
                for _ in range(int(lib.exps[j, 1 + i])):
                    m[j] = m[j] * c.u[:, i]
        mm = m[ii] * m[jj] * mom[(ex[ii] + ex[jj])]                                    # [F, F, N]
        G = torch.einsum("an,ijn->aij", onehot, mm).contiguous()
        b = torch.einsum("an,in->ai", onehot, m * mom[3 + ex]).contiguous()
        return G, b, ops.stlsq(G, b, threshold, alpha)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=100_000)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cohorts", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--weak-only", action="store_true", help="time the weak pass only (A/B builds)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_weak needs the GPU: there is no CPU fallback to time")
    from insite_amd import cohort, ops, weak
    dev = torch.device("cuda:0")
    N, T, K = a.patients, a.T, a.K
    cs = [cohort.synthetic_pkpd(N, T, 300 + i, dev, layout="time") for i in range(max(2, a.cohorts))]
    lib = cs[0].lib
    dt = cs[0].dt
    import numpy as np
    centres = weak.draw_centres(T, dt, K, 0)
    W, D = weak.test_function_weights(T, dt, np.sort(centres), device=dev)    # sorted rows, as SINDY.fit_weak
    Wu, Du = weak.test_function_weights(T, dt, centres, device=dev)           # the draw's own order
    full = torch.full((N,), T, dtype=torch.int32, device=dev)
    res = {"tool": "bench_weak", "patients": N, "T": T, "K": K, "cohorts": len(cs), "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    per_patient = lib.n_statics * 8 + 1 + 4
    nbytes = float(N) * T * 8 + N * per_patient
    flops = 2.0 * 2.0 * K * T * N

    plans = [ops.plan_sindy_fit_weak(c.x, W, D, c.u, c.arm, full, lib, a.threshold, layout="time") for c in cs]
    ms = timed(plans, a.steps, a.warmup)
    res["weak"] = {"ms_per_fit": ms, "useful_flops": flops,
                   "fraction_of_f64_mfma_peak": flops / (ms * 1e-3) / MFMA_F64_PEAK,
                   "algorithmic_bytes": nbytes, "fraction_of_8TBs": nbytes / (ms * 1e-3) / HBM_PEAK,
                   "support": plans[0].out[1].cpu().numpy().tolist(), "iters": plans[0].out[2].cpu().numpy().tolist()}
    gplans = [ops.plan_gram_weak(c.x, W, D, c.u, c.arm, full, lib, layout="time") for c in cs]
    res["weak_gram_only"] = {"ms_per_call": timed(gplans, a.steps, a.warmup)}
    uplans_w = [ops.plan_sindy_fit_weak(c.x, Wu, Du, c.u, c.arm, full, lib, a.threshold, layout="time") for c in cs]
    res["weak_unsorted_rows"] = {"ms_per_fit": timed(uplans_w, a.steps, a.warmup)}

    if a.weak_only:
        print(json.dumps(res))
        return
    runs = [torch_composition(c, c.x, W, D, lib, 2, a.threshold, a.alpha) for c in cs]
    ms_t = timed(runs, a.steps, a.warmup)
    plans[0]()
    G_t, b_t, _ = runs[0]()
    G_w, b_w = plans[0].out[3], plans[0].out[4]
    agree = float(max((G_t - G_w).abs().max(), (b_t - b_w).abs().max()) / G_w.abs().max())
    res["torch_composition"] = {"ms_per_fit": ms_t, "hbm_bytes_of_a_and_d": 2.0 * K * N * 8,
                                "speedup_of_weak": ms_t / ms, "gram_max_diff_of_largest_entry": agree}

    uplans = [ops.plan_sindy_fit(c.x, c.u, c.arm, c.rows, c.dt, lib, a.threshold, a.alpha, fd="smoothed4",
                                 layout="time") for c in cs]
    ms_u = timed(uplans, a.steps, a.warmup)
    res["uniform_sindy_fit"] = {"ms_per_fit": ms_u, "fraction_of_8TBs": nbytes / (ms_u * 1e-3) / HBM_PEAK}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
