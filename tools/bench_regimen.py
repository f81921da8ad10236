#!/usr/bin/env python
"""Time the regimen choice (ops.regimen_choice: K plans per row rolled from one prologue, the argmin inside each
bootstrap replicate, votes and objective / regret bands on chip) beside the only route to comparable numbers without
it, in one process: K - 1 prepared ops.effect_bands launches, plan 0 against every other plan.  That route gives the
per-step bands of every pair, from which a per-plan value and a pairwise difference can be read, but not the votes.

Workload: N rows (default 4096, 100k and 1M) x T = 60 steps, R = 256 replicates (replicate 0 the point model), the
std7 library, 2 arms, Euler with 5 sub-steps, Q = 3 quantiles, K in {2, 8} random per-row plans, per-row weights;
synthetic inputs (a decaying model and bootstrap-like perturbations of it).  Prepared plans, device events, warm-up
then ``--steps`` rounds, ``--runs`` runs of each side.  One JSON line per (N, K), also written to ``--out`` (default
``profiles/regimen/bench_regimen.jsonl``, rewritten by every full run; ``--kernel-only`` writes nothing).

    python tools/bench_regimen.py [--rows 4096 100000 1000000] [--plans 2 8] [--replicates 256] [--steps 20]
                                  [--warmup 5] [--runs 3]
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


def inputs(N, R, K, lib, dev, seed=0):
    """y0 [N], u [N, 2], K random per-step plans int8 [K, N, T], weights [N, T], cost [K], coef [R, 2, F]: a decaying
    model (state terms negative) and replicates scaled by 1 + 0.1 z (tools/bench_effect.py's)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    y0 = torch.rand(N, generator=g, device=dev, dtype=torch.float64) * 2.5 + 0.5
    u = torch.rand((N, 2), generator=g, device=dev, dtype=torch.float64) + 0.6
    plans = torch.randint(0, 2, (K, N, T_STEPS), generator=g, device=dev).to(torch.int8)
    w = torch.rand((N, T_STEPS), generator=g, device=dev, dtype=torch.float64)
    cost = torch.rand(K, generator=g, device=dev, dtype=torch.float64) * 0.1 - 0.05
    F = lib.n_terms
    base = torch.rand((2, F), generator=g, device=dev, dtype=torch.float64) * 0.1 + 0.05
    state = torch.as_tensor(lib.exps[:, 0] > 0, device=dev)
    sign = torch.where(torch.rand((2, F), generator=g, device=dev) < 0.5, -1.0, 1.0).to(torch.float64)
    base = torch.where(state[None], -base, base * sign)
    coef = base[None] * (1.0 + 0.1 * torch.randn((R, 2, F), generator=g, device=dev, dtype=torch.float64))
    coef[0] = base
    return y0, u, plans, w, cost, coef.contiguous()


def one_shape(N, R, K, a, dev):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0, u, plans, w, cost, coef = inputs(N, R, K, lib, dev)
    res = {"tool": "bench_regimen", "rows": N, "T": T_STEPS, "replicates": R, "plans": K, "library": "std7",
           "n_arms": 2, "method": "euler5", "quantiles": list(QUANTILES), "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    plan = ops.plan_regimen_choice(y0, u, plans, coef, lib, DT, QUANTILES, w, cost=cost, method="euler5", T=T_STEPS)
    ms = [timed(plan, a.steps, a.warmup) for _ in range(a.runs)]
    res["kernel"] = {"ms_per_call": ms, "us_per_row": [m * 1e3 / N for m in ms],
                     "us_per_row_and_plan": [m * 1e3 / N / K for m in ms],
                     "out_bytes": sum(t.numel() * t.element_size() for t in plan.out),
                     # two FMAs per (row, plan, step, replicate slot): 4 flop
                     "fma_tflops": [4.0 * N * K * T_STEPS * R / (m * 1e-3) / 1e12 for m in ms]}
    if not a.kernel_only and K > 1:
        out = torch.empty((3, 3 + len(QUANTILES), N, T_STEPS), dtype=torch.float64, device=dev)
        pairs = [ops.plan_effect_bands(y0, u, plans[0], plans[j], coef, lib, DT, QUANTILES, method="euler5", T=T_STEPS,
                                       out=out) for j in range(1, K)]

        def pairwise():
            for p in pairs:
                p()

        ms_p = [timed(pairwise, a.steps, a.warmup) for _ in range(a.runs)]
        spread = max(max(ms) - min(ms), max(ms_p) - min(ms_p))
        res["pairwise"] = {"launches": K - 1, "ms_per_call": ms_p, "us_per_row": [m * 1e3 / N for m in ms_p],
                           "speedup_of_kernel": min(ms_p) / min(ms),
                           "run_to_run_spread_ms": spread,
                           "kernel_faster": bool(min(ms) + spread < min(ms_p))}
        # the two routes agree where they overlap: the point model's terminal value of plan 0 under a terminal weight
        wt = torch.zeros(T_STEPS, dtype=torch.float64, device=dev)
        wt[-1] = 1.0
        n = min(N, 4096)
        _, _, o = ops.regimen_choice(y0[:n], u[:n], plans[:2, :n].contiguous(), coef, lib, DT, QUANTILES, wt,
                                     method="euler5", T=T_STEPS)
        e = ops.effect_bands(y0[:n], u[:n], plans[0, :n].contiguous(), plans[1, :n].contiguous(), coef, lib, DT,
                             QUANTILES, method="euler5", T=T_STEPS)
        torch.cuda.synchronize()
        agree = float((o[:, :, 0, :].permute(1, 2, 0) - e[:2, :, :, -1]).abs().max() / e[:2].abs().max())
        res["pairwise"]["max_diff_of_largest_trajectory"] = agree
        del out, pairs
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    if "pairwise" in res and not res["pairwise"]["max_diff_of_largest_trajectory"] <= 1e-10:
        raise SystemExit("the two routes differ in the terminal value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 100_000, 1_000_000])
    ap.add_argument("--plans", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="time the kernel only (A/B builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regimen", "bench_regimen.jsonl"),
                    help="file that receives the JSON lines of a full run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_regimen needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.kernel_only:
        a.out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for N in a.rows:
        for K in a.plans:
            one_shape(N, a.replicates, K, a, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
