#!/usr/bin/env python
"""Time the policy value (ops.policy_value: K plans per row rolled from one prologue, the argmin inside each
bootstrap replicate, 2 K + 2 weighted sums per (replicate, group) and the statistics of 2 K + 6 series) beside two
yardsticks built from the calls the tree had before it, in one process:

  (a) at 4096 rows, the materialised composition: K prepared ``ops.rollout`` launches on [n R] rows (every replicate's
      trajectory of every plan in memory) plus the torch reduction to the same sums and statistics; its inputs (the
      repeated rows, the Poisson weights, the group one-hot) are built once and not timed;
  (b) at every size, ceil(K / 2) prepared two-plan ``ops.cohort_effect`` calls: they roll the same K plans and average
      them per step, but cannot give the personalised, rule or share series.

Workload: N rows (default 4096, 100k and 1M) x T = 60 steps, R = 256 replicates (replicate 0 the point model), the
std7 library, 2 arms, Euler with 5 sub-steps, Q = 3 quantiles, Poisson row weights, K in {2, 8} random per-row plans,
G in {1, 8} groups; synthetic inputs (tools/bench_regimen.py's).  Prepared plans, device events, warm-up then
``--steps`` rounds, ``--runs`` runs of each side.  One JSON line per (N, K, G), also written to ``--out`` (default
``profiles/policy/bench_policy.jsonl``, rewritten by every full run; ``--kernel-only`` writes nothing).

    python tools/bench_policy.py [--rows 4096 100000 1000000] [--plans 2 8] [--groups 1 8] [--replicates 256]
                                 [--steps 20] [--warmup 5] [--runs 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

from bench_regimen import DT, QUANTILES, T_STEPS, inputs, timed  # noqa: E402

SEED = 5
MATERIALISED_ROWS = 4096


def materialised(y0, u, plans, w, cost, coef, group, G, lib, dev):
    """Yardstick (a): (the timed call, its result getter).  Everything the call does not compute per round is built
    here, once."""
    import torch
    from insite_amd import bootstrap, ops
    N, (R, A, F), K = y0.numel(), coef.shape, plans.size(0)
    y0r = y0.repeat_interleave(R).contiguous()
    ur = u.repeat_interleave(R, 0).contiguous()
    cr = coef.repeat(N, 1, 1).contiguous()
    rolls = [ops.plan_rollout(y0r, ur, plans[j].repeat_interleave(R, 0).contiguous(), cr, lib, DT, method="euler5",
                              drop_below=1e-3, T=T_STEPS) for j in range(K)]
    om = torch.as_tensor(bootstrap.weights(SEED, R, N, 0), dtype=torch.float64, device=dev).t().contiguous()  # [N, R]
    onehot = torch.nn.functional.one_hot(group.long(), G).to(torch.float64)                                   # [N, G]
    qt = torch.tensor(QUANTILES, dtype=torch.float64, device=dev)
    box = {}

    def call():
        J = torch.stack([(p().view(N, R, T_STEPS) * w[:, None, :]).sum(dim=2) + cost[j]
                         for j, p in enumerate(rolls)], dim=2)                                              # [N, R, K]
        best = J.argmin(dim=2)
        pick = torch.nn.functional.one_hot(best, K).to(torch.float64)
        rule = best[:, 0]
        cols = torch.cat([J, J.gather(2, best[:, :, None]), J.gather(2, rule[:, None, None].expand(N, R, 1)), pick],
                         dim=2)                                                                             # [N, R, 2K+2]
        sums = torch.einsum("ng,nr,nrc->rgc", onehot, om, cols)
        wsum = torch.einsum("ng,nr->rg", onehot, om)
        m = sums / wsum[:, :, None]
        bf = m[:, :, :K].min(dim=2).values
        ser = torch.cat([m[:, :, :K + 2], bf[:, :, None], (bf - m[:, :, K])[:, :, None],
                         (bf - m[:, :, K + 1])[:, :, None], (m[:, :, K + 1] - m[:, :, K])[:, :, None], m[:, :, K + 2:]],
                        dim=2)                                                                              # [R, G, S]
        rep = ser[1:]
        box["out"] = torch.cat([ser[:1], rep.mean(0, keepdim=True), rep.std(0, keepdim=True),
                                torch.quantile(rep, qt, dim=0)], dim=0).permute(1, 2, 0)                    # [G, S, 3+Q]
        return box["out"]

    return call, box


def one_shape(N, R, K, G, a, dev):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0, u, plans, w, cost, coef = inputs(N, R, K, lib, dev)
    group = (torch.arange(N, device=dev) % G).to(torch.int32)
    res = {"tool": "bench_policy", "rows": N, "T": T_STEPS, "replicates": R, "plans": K, "groups": G,
           "library": "std7", "n_arms": 2, "method": "euler5", "quantiles": list(QUANTILES), "weighting": "poisson",
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    plan = ops.plan_policy_value(y0, u, plans, coef, lib, DT, QUANTILES, w, cost=cost, group=group, n_groups=G,
                                 weighting="poisson", seed=SEED, method="euler5", T=T_STEPS)
    ms = [timed(plan, a.steps, a.warmup) for _ in range(a.runs)]
    res["kernel"] = {"ms_per_call": ms, "us_per_row": [m * 1e3 / N for m in ms],
                     # two FMAs per (row, plan, step, replicate): 4 flop
                     "fma_tflops": [4.0 * N * K * T_STEPS * R / (m * 1e-3) / 1e12 for m in ms]}
    if not a.kernel_only:
        # (b) the same K plans through two-plan cohort_effect calls
        pairs = [ops.plan_cohort_effect(y0, u, plans[j], plans[min(j + 1, K - 1)], coef, lib, DT, QUANTILES,
                                        group=group, n_groups=G, weighting="poisson", seed=SEED, method="euler5",
                                        T=T_STEPS) for j in range(0, K, 2)]

        def cohort_pairs():
            for p in pairs:
                p()

        ms_b = [timed(cohort_pairs, a.steps, a.warmup) for _ in range(a.runs)]
        spread = max(max(ms) - min(ms), max(ms_b) - min(ms_b))
        res["cohort_effect_pairs"] = {"launches": len(pairs), "ms_per_call": ms_b,
                                      "ratio_to_kernel": min(ms_b) / min(ms), "run_to_run_spread_ms": spread,
                                      "kernel_not_slower": bool(min(ms) <= min(ms_b) + spread)}
        del pairs
        if N <= MATERIALISED_ROWS:
            call, box = materialised(y0, u, plans, w, cost, coef, group, G, lib, dev)
            ms_a = [timed(call, a.steps, a.warmup) for _ in range(a.runs)]
            spread = max(max(ms) - min(ms), max(ms_a) - min(ms_a))
            got = plan()[0]
            torch.cuda.synchronize()
            # the two routes agree (torch.quantile's interpolation is the header's), relative to the largest value
            keep = [0, 1, 3, 4, 5]
            diff = float((got[:, :, keep] - box["out"][:, :, keep]).abs().max() / box["out"][:, :K].abs().max())
            res["materialised"] = {"launches": K, "trajectory_bytes": K * N * R * T_STEPS * 8, "ms_per_call": ms_a,
                                   "speedup_of_kernel": min(ms_a) / min(ms), "run_to_run_spread_ms": spread,
                                   "kernel_faster": bool(min(ms) + spread < min(ms_a)),
                                   "max_diff_of_largest_value": diff}
            del call, box
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    if "materialised" in res and not res["materialised"]["max_diff_of_largest_value"] <= 1e-9:
        raise SystemExit("the two routes differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 100_000, 1_000_000])
    ap.add_argument("--plans", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="time the kernel only (A/B builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy", "bench_policy.jsonl"),
                    help="file that receives the JSON lines of a full run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.kernel_only:
        a.out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for N in a.rows:
        for K in a.plans:
            for G in a.groups:
                one_shape(N, a.replicates, K, G, a, dev)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
