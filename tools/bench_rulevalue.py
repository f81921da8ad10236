#!/usr/bin/env python
"""Time the rule value (ops.rule_value: K closed-loop rules per row rolled from one prologue inside each bootstrap
replicate, their argmin, 3 K + 4 weighted sums per (replicate, group) and the statistics of 3 K + 9 series) beside two
yardsticks, neither of them the code under test, in one process:

  (a) at 4096 rows, the torch composition that is the only route without the kernel: tools/bench_feedback.py's
      ``torch_route`` (the replicates' interval maps folded with torch, a Python loop over the T steps on [R, n] tensors
      with torch.where between them) followed by the weighted sums per replicate and group and torch's mean / std /
      quantile; its inputs that do not change per round (the Poisson weights, the group one-hot) are built once and
      not timed; checked for agreement with the kernel;
  (b) at every size, ops.policy_value on the same shape under K constant plans: the open-loop kernel with the same
      skeleton, whose step is the two FMAs the closed loop adds its decision to.

Workload: tools/bench_feedback.py's -- N rows (default 4096, 100k and 1M) x T = 60 steps, R = 256 replicates
(replicate 0 the point model), the std7 library, 2 arms, Euler with 5 sub-steps, Q = 3 quantiles, K in {2, 8} rules with
per-row thresholds, periods cycling through 1, 1, 2, 5, per-row weights, a cost per rule and per arm -- with Poisson
row weights and G in {1, 8} groups.  Prepared plans, device events, warm-up then ``--steps`` rounds, ``--runs`` runs of
each side.  One JSON line per (N, K, G), also written to ``--out`` (default ``profiles/rulevalue/bench_rulevalue.jsonl``,
rewritten by every full run; ``--kernel-only`` writes nothing).

    python tools/bench_rulevalue.py [--rows 4096 100000 1000000] [--rules 2 8] [--groups 1 8] [--replicates 256]
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

from bench_feedback import ARM_COST, rule_inputs, torch_route  # noqa: E402
from bench_regimen import DT, QUANTILES, T_STEPS, inputs, timed  # noqa: E402

SEED = 5
TORCH_ROWS = 4096


def torch_composition(y0, u, theta, rules, w, cost, coef, group, G, lib, dev):
    """Yardstick (a): (the timed call, its results)."""
    import torch
    from insite_amd import bootstrap
    N, R, K = y0.numel(), coef.size(0), len(rules)
    om = torch.as_tensor(bootstrap.weights(SEED, R, N, 0), dtype=torch.float64, device=dev)   # [R, N]
    onehot = torch.nn.functional.one_hot(group.long(), G).to(torch.float64)                   # [N, G]
    qt = torch.tensor(QUANTILES, dtype=torch.float64, device=dev)
    box = {}

    def call():
        _, _, J, E, _ = torch_route(y0, u, theta, rules, w, cost, coef, lib, QUANTILES)       # [R, N, K]
        best = J.argmin(dim=2)
        pick = torch.nn.functional.one_hot(best, K).to(torch.float64)
        asg = best[0][None, :, None].expand(R, N, 1)
        bi = best[:, :, None]
        cols = torch.cat([J, J.gather(2, bi), J.gather(2, asg), pick, E, E.gather(2, bi), E.gather(2, asg)], dim=2)
        sums = torch.einsum("ng,rn,rnc->rgc", onehot, om, cols)                               # [R, G, 3K+4]
        wsum = torch.einsum("ng,rn->rg", onehot, om)
        m = sums / wsum[:, :, None]
        bf, jf = m[:, :, :K].min(dim=2)
        ebf = m[:, :, 2 * K + 2:3 * K + 2].gather(2, jf[:, :, None])
        ser = torch.cat([m[:, :, :K + 2], bf[:, :, None], (bf - m[:, :, K])[:, :, None],
                         (bf - m[:, :, K + 1])[:, :, None], (m[:, :, K + 1] - m[:, :, K])[:, :, None], m[:, :, K + 2:],
                         ebf], dim=2)                                                          # [R, G, S]
        rep = ser[1:]
        box["out"] = torch.cat([ser[:1], rep.mean(0, keepdim=True), rep.std(0, keepdim=True),
                                torch.quantile(rep, qt, dim=0)], dim=0).permute(1, 2, 0)       # [G, S, 3+Q]
        box["sums"], box["wsum"], box["assign"] = sums, wsum, best[0]
        return box["out"]

    return call, box


def one_shape(N, R, K, G, a, dev):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0, u, _, w, cost, coef = inputs(N, R, K, lib, dev)
    theta, rules = rule_inputs(y0, K, dev)
    group = (torch.arange(N, device=dev) % G).to(torch.int32)
    res = {"tool": "bench_rulevalue", "rows": N, "T": T_STEPS, "replicates": R, "rules": K, "groups": G,
           "library": "std7", "n_arms": 2, "method": "euler5", "quantiles": list(QUANTILES), "weighting": "poisson",
           "periods": [int(r[2]) for r in rules], "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    plan = ops.plan_rule_value(y0, u, theta, rules, coef, lib, DT, QUANTILES, w, cost=cost, arm_cost=ARM_COST,
                               group=group, n_groups=G, weighting="poisson", seed=SEED, method="euler5", T=T_STEPS)
    ms = [timed(plan, a.steps, a.warmup) for _ in range(a.runs)]
    res["kernel"] = {"ms_per_call": ms, "ns_per_row_and_rule": [m * 1e6 / N / K for m in ms]}
    if not a.kernel_only:
        # yardstick (b): the open-loop cohort kernel on K constant plans
        plans = torch.as_tensor(rules[:, 0:1].repeat(T_STEPS, axis=1).astype("int8"), device=dev).contiguous()
        pv = ops.plan_policy_value(y0, u, plans, coef, lib, DT, QUANTILES, w, cost=cost, group=group, n_groups=G,
                                   weighting="poisson", seed=SEED, method="euler5", T=T_STEPS)
        ms_p = [timed(pv, a.steps, a.warmup) for _ in range(a.runs)]
        spread = max(max(ms) - min(ms), max(ms_p) - min(ms_p))
        res["policy_constant_plans"] = {"ms_per_call": ms_p, "ns_per_row_and_plan": [m * 1e6 / N / K for m in ms_p],
                                        "kernel_over_policy": min(ms) / min(ms_p), "run_to_run_spread_ms": spread}
        del pv
        if N <= TORCH_ROWS:
            call, box = torch_composition(y0, u, theta, rules, w, cost, coef, group, G, lib, dev)
            ms_t = [timed(call, max(a.steps // 4, 2), 1) for _ in range(a.runs)]
            spread_t = max(max(ms) - min(ms), max(ms_t) - min(ms_t))
            out, _, _, assign, sums, wsum = plan()
            call()
            torch.cuda.synchronize()
            keep = [0, 1, 3, 4, 5]
            scale = float(box["out"][:, :K].abs().max())
            res["torch_composition"] = {
                "ms_per_call": ms_t, "ns_per_row_and_rule": [m * 1e6 / N / K for m in ms_t],
                "speedup_of_kernel": min(ms_t) / min(ms), "run_to_run_spread_ms": spread_t,
                "kernel_faster": bool(min(ms) + spread_t < min(ms_t)),
                "assign_mismatches": int((assign.long() != box["assign"]).sum()),
                "wsum_mismatches": int((wsum != box["wsum"]).sum()),
                "max_diff_objective_series_of_scale":
                    float((out[:, :K + 6][:, :, keep] - box["out"][:, :K + 6][:, :, keep]).abs().max() / scale),
                "max_diff_share_series": float((out[:, K + 6:2 * K + 6][:, :, keep]
                                                - box["out"][:, K + 6:2 * K + 6][:, :, keep]).abs().max()),
                "max_diff_exposure_series_of_T":
                    float((out[:, 2 * K + 6:][:, :, keep] - box["out"][:, 2 * K + 6:][:, :, keep]).abs().max()
                          / T_STEPS)}
            del call, box
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    t = res.get("torch_composition")
    if t and not (t["max_diff_objective_series_of_scale"] <= 1e-9 and t["wsum_mismatches"] == 0
                  and t["assign_mismatches"] <= N // 1000):
        raise SystemExit("the torch composition and the kernel disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 100_000, 1_000_000])
    ap.add_argument("--rules", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="time the kernel only (A/B builds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rulevalue", "bench_rulevalue.jsonl"),
                    help="file that receives the JSON lines of a full run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rulevalue needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.kernel_only:
        a.out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for N in a.rows:
        for K in a.rules:
            for G in a.groups:
                one_shape(N, a.replicates, K, G, a, dev)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
