#!/usr/bin/env python
"""Time the cohort / subgroup average effects (ops.cohort_effect: lane = replicate, the weighted trajectory sums in
lane-private registers, then a reduce over the patient chunks and an LDS sort per (group, step)) beside the
composition it replaces, in one process.

Workload: N patients (default 1M and 100k) x T = 60 steps, R = 256 replicates (replicate 0 the point model), the std7
library, 2 arms, three series (A, B, A - B), Q = 3 quantiles, Poisson weights, G = 1 and G = 8 groups (group = p % G);
synthetic inputs (tools/bench_effect.py's).  Prepared plans, device events, warm-up then ``--steps`` rounds, ``--runs``
runs of each side.  Timed:
  kernel       ops.plan_cohort_effect at every N and G, and at the composition's rows (G = 1)
  composition  at ``--composition-rows`` patients (default 4096, G = 1): two prepared ops.rollout launches on [n R]
               rows with per-row coefficients, the weighted means with a materialised weight tensor
               (``bootstrap.weights``: built once, not counted, like the repeated inputs), the paired difference and
               per series torch.quantile, mean and std over the replicates 1..R-1.  What is not counted favours the
               composition: it is the bar.
Both sides are reported per patient.  The tool checks that the two paths agree at the composition's rows (largest
difference over the largest |trajectory| there <= 1e-10) and exits non-zero otherwise.  One JSON line per shape, also
written to ``--out`` (default ``profiles/cohort_effect/bench_cohort_effect.jsonl``, rewritten by every full run;
``--kernel-only`` writes nothing unless ``--out`` is given).

    python tools/bench_cohort_effect.py [--patients 1000000 100000] [--replicates 256] [--groups 1 8] [--steps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_effect import DT, QUANTILES, T_STEPS, inputs, timed  # noqa: E402

SEED = 7


def composition(n, R, y0, u, arm_a, arm_b, coef, lib):
    """The prepared composition on the first n rows, one group: callable -> [1, 3, 3 + Q, T]."""
    import torch
    from insite_amd import bootstrap, ops
    dev = y0.device
    y0r = y0[:n].repeat_interleave(R).contiguous()
    ur = u[:n].repeat_interleave(R, 0).contiguous()
    ar = arm_a[:n].repeat_interleave(R, 0).contiguous()
    br = arm_b[:n].repeat_interleave(R, 0).contiguous()
    cr = coef.repeat(n, 1, 1).contiguous()
    pa = ops.plan_rollout(y0r, ur, ar, cr, lib, DT, method="euler5", T=T_STEPS)
    pb = ops.plan_rollout(y0r, ur, br, cr, lib, DT, method="euler5", T=T_STEPS)
    w = torch.as_tensor(bootstrap.weights(SEED, R, n).T.copy(), dtype=torch.float64, device=dev)   # [n, R]
    qt = torch.as_tensor(QUANTILES, dtype=torch.float64, device=dev)

    def run():
        ya, yb = pa().view(n, R, T_STEPS), pb().view(n, R, T_STEPS)
        wsum = w.sum(0)                                                  # [R]
        ma = (w[:, :, None] * ya).sum(0) / wsum[:, None]                 # [R, T]
        mb = (w[:, :, None] * yb).sum(0) / wsum[:, None]
        out = []
        for v in (ma, mb, ma - mb):
            rep = v[1:]
            out.append(torch.cat([v[:1], rep.mean(0)[None], rep.std(0, unbiased=True)[None],
                                  torch.quantile(rep, qt, dim=0)]))
        return torch.stack(out)[None]

    return run, 2 * n * R * T_STEPS * 8


def one_shape(N, R, groups, a, dev, comp):
    import torch
    from insite_amd import ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(2, 2, True)
    y0, u, arm_a, arm_b, coef = inputs(N, R, lib, dev)
    res = {"tool": "bench_cohort_effect", "patients": N, "T": T_STEPS, "replicates": R, "library": "std7",
           "n_arms": 2, "n_series": 3, "quantiles": list(QUANTILES), "weighting": "poisson", "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernel": {}}
    for G in groups:
        group = (torch.arange(N, device=dev) % G).to(torch.int32) if G > 1 else None
        plan = ops.plan_cohort_effect(y0, u, arm_a, arm_b, coef, lib, DT, QUANTILES, group=group, n_groups=G,
                                      weighting="poisson", seed=SEED, method="euler5", T=T_STEPS)
        ms = [timed(plan, a.steps, a.warmup) for _ in range(a.runs)]
        res["kernel"][f"G{G}"] = {"ms_per_call": ms, "us_per_patient": [m * 1e3 / N for m in ms],
                                  "weighted_steps_per_s": [2.0 * N * R * T_STEPS / (m * 1e-3) for m in ms]}
        del plan
    if comp is not None:
        n = min(comp, N)
        run, nbytes = composition(n, R, y0, u, arm_a, arm_b, coef, lib)
        ms_c = [timed(run, a.steps, a.warmup) for _ in range(a.runs)]
        small = ops.plan_cohort_effect(y0[:n], u[:n], arm_a[:n], arm_b[:n], coef, lib, DT, QUANTILES,
                                       weighting="poisson", seed=SEED, method="euler5", T=T_STEPS)
        ms_s = [timed(small, a.steps, a.warmup) for _ in range(a.runs)]
        want, got = run(), small()[0]
        torch.cuda.synchronize()
        agree = float((got - want).abs().max() / want[0, :2].abs().max())
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
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--composition-rows", type=int, default=4096,
                    help="patients of the composition (its [n R, T] tensors must fit comfortably)")
    ap.add_argument("--kernel-only", action="store_true", help="time the kernel only (A/B builds)")
    ap.add_argument("--out", default=None, help="file that receives the JSON lines (default: "
                    "profiles/cohort_effect/bench_cohort_effect.jsonl for a full run, none with --kernel-only)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cohort_effect needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.out is None and not a.kernel_only:
        a.out = os.path.join(ROOT, "profiles", "cohort_effect", "bench_cohort_effect.jsonl")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for i, N in enumerate(a.patients):
        # the composition runs once, beside the last (smallest) shape
        one_shape(N, a.replicates, a.groups, a, dev,
                  None if a.kernel_only or i + 1 < len(a.patients) else a.composition_rows)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
