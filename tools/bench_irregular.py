#!/usr/bin/env python
"""Time the discovery on irregular observation grids (ops.sindy_fit_irregular, both derivative kinds) beside the
closest uniform-grid path (the patient-major ops.sindy_fit at the same cohort size and T = 60), in one process.

Every timed window is warmed up, runs prepared plans only, rotates over several cohorts (each far larger than the
256 MiB Infinity Cache at the default size, so no call finds its input cached) and is bracketed by device events.
Algorithmic bytes are what the pass has to read: 16 B (x and t) per sample inside n_obs for the irregular kernel,
8 B per stored sample for the uniform one, plus the per-patient statics, arm and length.  Prints one JSON line.

    python tools/bench_irregular.py [--patients 1000000] [--steps 20] [--warmup 5] [--cohorts 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

HBM_PEAK = 8.0e12   # B/s, MI355X


def timed(plans, steps, warmup):
    """ms per call of the plans called round robin: ``steps`` rounds after ``warmup`` rounds."""
    import torch
    for _ in range(warmup):
        for p in plans:
            p()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        for p in plans:
            p()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (steps * len(plans))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cohorts", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--alpha", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_irregular needs the GPU: there is no CPU fallback to time")
    from insite_amd import cohort, ops
    dev = torch.device("cuda:0")
    N, T = a.patients, 60
    irr = [cohort.irregular_cohort(N, 100 + i, dev) for i in range(max(2, a.cohorts))]
    uni = [cohort.synthetic_pkpd(N, T, 200 + i, dev, layout="patient") for i in range(max(2, a.cohorts))]
    lib = irr[0].lib
    per_patient = lib.n_statics * 8 + 1 + 4
    res = {"tool": "bench_irregular", "patients": N, "T_max": T, "cohorts": len(irr), "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    samples = sum(int(c.n_obs.sum()) for c in irr) / len(irr)
    irr_bytes = samples * 16 + N * per_patient
    for fd in ("nonuniform2", "nonuniform4"):
        plans = [ops.plan_sindy_fit_irregular(c.x, c.t_obs, c.n_obs, c.u, c.arm, lib, a.threshold, a.alpha, fd=fd)
                 for c in irr]
        ms = timed(plans, a.steps, a.warmup)
        res[fd] = {"ms_per_fit": ms, "algorithmic_bytes": irr_bytes, "bytes_per_s": irr_bytes / (ms * 1e-3),
                   "fraction_of_8TBs": irr_bytes / (ms * 1e-3) / HBM_PEAK,
                   "support": plans[0].out[1].cpu().numpy().tolist()}
    plans = [ops.plan_sindy_fit(c.x, c.u, c.arm, c.rows, c.dt, lib, 0.1, a.alpha, fd="smoothed4", layout="patient")
             for c in uni]
    ms = timed(plans, a.steps, a.warmup)
    uni_bytes = float(N) * T * 8 + N * per_patient
    res["uniform_patient_major"] = {"ms_per_fit": ms, "algorithmic_bytes": uni_bytes,
                                    "bytes_per_s": uni_bytes / (ms * 1e-3),
                                    "fraction_of_8TBs": uni_bytes / (ms * 1e-3) / HBM_PEAK}
    res["samples_in_n_obs"] = samples
    print(json.dumps(res))


if __name__ == "__main__":
    main()
