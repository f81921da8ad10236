#!/usr/bin/env python
"""Time the paired treatment-effect bands (ops.effect_bands: R replicate trajectories of both plans in one wave's
registers, order statistics by a register bitonic network) beside the composition it replaces, in one process.

Workload: N patients (default 1M and 100k) x T = 60 steps, R = 256 replicates (replicate 0 the point model), the std7
library, 2 arms, three series (A, B, A - B), Q = 3 quantiles; synthetic inputs (a decaying model and bootstrap-like
perturbations of it).  Prepared plans, device events, warm-up then ``--steps`` rounds, ``--runs`` runs of each side.
Timed:
  kernel       ops.plan_effect_bands at every N
  composition  at ``--composition-rows`` patients (default 4096: [n R, T] f64 is 503 MB per plan there): two prepared
               ops.rollout launches on [n R] rows with per-row coefficients, the subtraction, and per series
               torch.quantile, mean and std over the replicates 1..R-1.  The repeated inputs ([n R] rows, [n R, A, F]
               coefficients) are built once and not counted, which favours the composition: it is the bar.
Both sides are reported per patient.  The tool checks that the two paths agree at the composition's rows (largest
difference over the largest |trajectory| there <= 1e-10) and exits non-zero otherwise.  One JSON line per shape, also
written to ``--out`` (default ``profiles/effect/bench_effect.jsonl``, rewritten by every full run; ``--kernel-only``
writes nothing).

    python tools/bench_effect.py [--patients 1000000 100000] [--replicates 256] [--steps 20] [--warmup 5] [--runs 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

T_STEPS, DT, QUANTILES = 60, 10.0 / 60.0, (0.025, 0.5, 0.975)


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


def inputs(N, R, lib, dev, seed=0):
    """y0 [N], u [N, 2], two random per-step plans int8 [N, T], coef [R, 2, F]: a decaying model (state terms
    negative) and replicates scaled by 1 + 0.1 z."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    y0 = torch.rand(N, generator=g, device=dev, dtype=torch.float64) * 2.5 + 0.5
    u = torch.rand((N, 2), generator=g, device=dev, dtype=torch.float64) + 0.6
    arm_a = torch.randint(0, 2, (N, T_STEPS), generator=g, device=dev).to(torch.int8)
    arm_b = torch.randint(0, 2, (N, T_STEPS), generator=g, device=dev).to(torch.int8)
    F = lib.n_terms
    base = torch.rand((2, F), generator=g, device=dev, dtype=torch.float64) * 0.1 + 0.05
    state = torch.as_tensor(lib.exps[:, 0] > 0, device=dev)
    sign = torch.where(torch.rand((2, F), generator=g, device=dev) < 0.5, -1.0, 1.0).to(torch.float64)
    base = torch.where(state[None], -base, base * sign)
    coef = base[None] * (1.0 + 0.1 * torch.randn((R, 2, F), generator=g, device=dev, dtype=torch.float64))
    coef[0] = base
    return y0, u, arm_a, arm_b, coef.contiguous()


def composition(n, R, y0, u, arm_a, arm_b, coef, lib):
    """The prepared composition on the first n rows: (callable -> [3, 3 + Q, n, T], bytes of its [n R, T] tensors)."""
    import torch
    from insite_amd import ops
    dev = y0.device
    y0r = y0[:n].repeat_interleave(R).contiguous()
    ur = u[:n].repeat_interleave(R, 0).contiguous()
    ar = arm_a[:n].repeat_interleave(R, 0).contiguous()
    br = arm_b[:n].repeat_interleave(R, 0).contiguous()
    cr = coef.repeat(n, 1, 1).contiguous()
    pa = ops.plan_rollout(y0r, ur, ar, cr, lib, DT, method="euler5", T=T_STEPS)
    pb = ops.plan_rollout(y0r, ur, br, cr, lib, DT, method="euler5", T=T_STEPS)
    qt = torch.as_tensor(QUANTILES, dtype=torch.float64, device=dev)

    def run():
        ya, yb = pa().view(n, R, T_STEPS), pb().view(n, R, T_STEPS)
        out = []
        for v in (ya, yb, ya - yb):
            rep = v[:, 1:]
            out.append(torch.cat([v[:, :1].transpose(0, 1), rep.mean(1)[None], rep.std(1, unbiased=True)[None],
                                  torch.quantile(rep, qt, dim=1)]))
        return torch.stack(out)

    return run, 3 * n * R * T_STEPS * 8


def one_shape(N, R, a, dev, comp):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0, u, arm_a, arm_b, coef = inputs(N, R, lib, dev)
    res = {"tool": "bench_effect", "patients": N, "T": T_STEPS, "replicates": R, "library": "std7", "n_arms": 2,
           "n_series": 3, "quantiles": list(QUANTILES), "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    plan = ops.plan_effect_bands(y0, u, arm_a, arm_b, coef, lib, DT, QUANTILES, method="euler5", T=T_STEPS)
    ms = [timed(plan, a.steps, a.warmup) for _ in range(a.runs)]
    res["kernel"] = {"ms_per_call": ms, "us_per_patient": [m * 1e3 / N for m in ms],
                     "out_bytes": plan.out.numel() * 8,
                     "sorted_keys_per_s": [3.0 * N * T_STEPS * (R - 1) / (m * 1e-3) for m in ms]}
    if comp is not None:
        n = min(comp, N)
        run, nbytes = composition(n, R, y0, u, arm_a, arm_b, coef, lib)
        ms_c = [timed(run, a.steps, a.warmup) for _ in range(a.runs)]
        small = ops.plan_effect_bands(y0[:n], u[:n], arm_a[:n], arm_b[:n], coef, lib, DT, QUANTILES, method="euler5",
                                      T=T_STEPS)
        ms_s = [timed(small, a.steps, a.warmup) for _ in range(a.runs)]
        want, got = run(), small()
        torch.cuda.synchronize()
        agree = float((got - want).abs().max() / want[:2].abs().max())
        spread = max(max(ms_c) - min(ms_c), max(ms_s) - min(ms_s)) * 1e3 / n
        res["composition"] = {"rows": n, "ms_per_call": ms_c, "us_per_patient": [m * 1e3 / n for m in ms_c],
                              "replicate_tensor_bytes": nbytes,
                              "kernel_ms_at_rows": ms_s, "kernel_us_per_patient_at_rows": [m * 1e3 / n for m in ms_s],
                              "speedup_of_kernel_at_rows": min(ms_c) / min(ms_s),
                              "run_to_run_spread_us_per_patient": spread,
                              "kernel_no_slower": bool(min(ms_s) * 1e3 / n <= min(ms_c) * 1e3 / n + spread),
                              "max_diff_of_largest_trajectory": agree}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    if comp is not None and not agree <= 1e-10:
        raise SystemExit(f"the two paths differ by {agree:.3e} of the largest trajectory value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--composition-rows", type=int, default=4096,
                    help="patients of the composition (its [n R, T] tensors must fit comfortably)")
    ap.add_argument("--kernel-only", action="store_true", help="time the kernel only (A/B builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effect", "bench_effect.jsonl"),
                    help="file that receives the JSON lines of a full run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_effect needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.kernel_only:
        a.out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for i, N in enumerate(a.patients):
        # the composition runs once, beside the last (smallest) shape
        one_shape(N, a.replicates, a, dev, None if a.kernel_only or i + 1 < len(a.patients) else a.composition_rows)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
