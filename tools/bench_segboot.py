#!/usr/bin/env python
"""Time the patient-level bootstrap of the treatment-segment discovery (include/insite_segboot.h)
beside its yardsticks, in one process.

Workload: the EQ_5 shape -- N patients (default 1M and 100k), T = 60 steps, 4 arms that switch over time, the std7
library (2 statics), R = 1024 replicates -- on ``cohort.synthetic_segments`` (time-major).  Prepared plans, device
events, ``--warmup`` rounds then ``--steps`` timed rounds, ``--runs`` such runs per figure (all reported, the median
is the figure).  Timed:
  moments     ops.plan_segment_moments, beside ops.plan_gram_segments on the same cohort: the existing kernel that
              reads the same bytes and contracts the moments instead of writing them.  Bytes of the moments pass:
              (T + 1) N 8 + T N + 4 N read, N n_arms 40 written.
  bootstrap   ops.plan_sindy_bootstrap_segments (Gram + STLSQ of the R n_arms systems) and ops.plan_segboot_gram alone
  torch       the composition it replaces: the weights MATERIALISED as an f64 [R, N] tensor (built once by
              tools/bench_bootstrap.py's torch restatement of the Threefry block; build time reported, not counted),
              the per-(patient, arm) entries [N, A nE] (built once, not counted), then per call torch.matmul(W, E),
              the unpacking to G | b and ops.stlsq.  Leaving the two builds out favours the composition: it is the bar.
              Skipped (and said so) where [R, N] f64 does not fit ``--max-weight-bytes``.
The tool checks that the materialised weights are the package's on a slice, that replicate 0 of the bootstrap is
ops.gram_segments' G | b, and that G | b of the two paths agree (largest difference over the largest entry of its
system <= 1e-10); it exits non-zero otherwise.  One JSON line per shape, also written to ``--out`` (default
``profiles/segboot/bench_segboot.jsonl``, rewritten by every run).

    python tools/bench_segboot.py [--patients 1000000 100000] [--replicates 1024] [--steps 20] [--warmup 5] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_bootstrap as BB  # noqa: E402  (timed, device_weights, the f64 MFMA peak)

T_STEPS, N_ARMS, N_STATICS = 60, 4, 2


def planted_coef(lib):
    """A 4-arm model over std7 in the manner of oracle.segments_ref.TRUE_COEF_U1: growth without treatment, three kill
    terms."""
    import numpy as np
    names = list(lib.get_feature_names())
    c = np.zeros((N_ARMS, lib.n_terms))
    c[0, names.index("x0")] = 0.20
    c[1, names.index("x0 u0")] = -0.60
    c[2, names.index("x0")] = -0.30
    c[3, names.index("x0")] = -0.25
    c[3, names.index("x0 u1")] = -0.90
    return c


def runs_of(call, a):
    ms = [BB.timed(call, a.steps, a.warmup) for _ in range(a.runs)]
    return {"ms_runs": ms, "ms": statistics.median(ms)}


def entries(mom, u, lib):
    """E [N, n_arms nE] (arm-major; upper triangle then b, as the kernel's columns) and the unpacking indices; a
    (patient, arm) without rows (count 0) is a zero row by a select."""
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
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    cols = []
    for a in range(mom.size(1)):
        ma = mom[:, a]
        e = torch.cat([m[:, ii] * m[:, kk] * ma[:, ex[ii] + ex[kk]], m * ma[:, 3 + ex]], dim=1)
        cols.append(torch.where((ma[:, 0] > 0)[:, None], e, zero))
    return torch.cat(cols, dim=1).contiguous(), ii, kk


def one_shape(N, R, a, dev):
    import numpy as np
    import torch
    from insite_amd import _lib, bootstrap, cohort, ops
    from insite_amd.library import polynomial_library
    lib = polynomial_library(N_STATICS, 2, True)
    c = cohort.synthetic_segments(N, T_STEPS, 500, dev, planted_coef(lib), n_statics=N_STATICS, dt=0.1)
    seed, fd = 7, a.fd
    F = lib.n_terms
    nE = F * (F + 1) // 2 + F
    ncol = N_ARMS * nE
    n_tiles = (ncol + 15) // 16
    n_z = (n_tiles + 4) // 5
    ct = (n_tiles + n_z - 1) // n_z
    rt = 3 if ct == 5 else 4
    r_pad = (R + 16 * rt - 1) // (16 * rt) * 16 * rt
    res = {"tool": "bench_segboot", "patients": N, "replicates": R, "library": "std7", "n_arms": N_ARMS, "T": T_STEPS,
           "fd": fd, "layout": "time", "steps": a.steps, "warmup": a.warmup, "runs": a.runs,
           "device": torch.cuda.get_device_name(0), "column_tiles": n_tiles, "column_chunks": n_z, "ct": ct, "rt": rt,
           "workspace_bytes": int(_lib.load().insite_segboot_workspace_bytes(N, N_ARMS, F, R))}

    # ---- the moments pass beside the segment Gram it is cut from
    mplan = ops.plan_segment_moments(c.x, c.arm, c.seq_len, c.dt, n_arms=N_ARMS, fd=fd, layout="time")
    gplan = ops.plan_gram_segments(c.x, c.arm, c.seq_len, c.u, c.dt, lib, n_arms=N_ARMS, fd=fd, layout="time")
    t_m, t_g = runs_of(mplan, a), runs_of(gplan, a)
    rd, wr = float((T_STEPS + 1) * N * 8 + T_STEPS * N + 4 * N), float(N * N_ARMS * 40)
    res["moments"] = dict(t_m, bytes_read=rd, bytes_written=wr, bytes_per_s=(rd + wr) / (t_m["ms"] * 1e-3),
                          gram_segments_ms_runs=t_g["ms_runs"], gram_segments_ms=t_g["ms"],
                          ratio_to_gram_segments=t_m["ms"] / t_g["ms"])
    mom = mplan()
    G_seg, b_seg = gplan()

    # ---- Gram + fit
    plan = ops.plan_sindy_bootstrap_segments(mom, c.u, lib, R, a.threshold, alpha=a.alpha, seed=seed)
    bplan = ops.plan_segboot_gram(mom, c.u, lib, R, seed=seed)
    t_f, t_b = runs_of(plan, a), runs_of(bplan, a)
    dense = 2.0 * r_pad * N * 16 * n_z * ct
    res["bootstrap"] = dict(t_f, gram_only_ms_runs=t_b["ms_runs"], gram_only_ms=t_b["ms"], dense_flops=dense,
                            useful_flops=2.0 * R * N * ncol,
                            dense_fraction_of_f64_mfma_peak=dense / (t_b["ms"] * 1e-3) / BB.MFMA_F64_PEAK,
                            threefry_blocks=r_pad * (N / 2.0) * n_z)
    coef, mask, _, G_k, b_k = plan()
    torch.cuda.synchronize()
    scale = G_seg.abs().amax(dim=(1, 2))                                   # the largest entry of each arm's system
    rep0 = float(max(((G_k[0] - G_seg).abs().amax(dim=(1, 2)) / scale).max(),
                     ((b_k[0] - b_seg).abs().amax(dim=1) / scale).max()))
    res["replicate0_vs_gram_segments"] = rep0
    res["inclusion"] = (mask[1:] != 0).double().mean(0).cpu().numpy().tolist() if R > 1 else None

    agree = 0.0
    if float(R) * N * 8 > a.max_weight_bytes:
        res["torch_composition"] = {"skipped": f"[R, N] f64 weights need {float(R) * N * 8:.3e} bytes"}
    else:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        W = BB.device_weights(seed, R, N, 0, dev)
        t1.record()
        torch.cuda.synchronize()
        n_chk = min(N, 300)
        if not np.array_equal(W[:, :n_chk].cpu().numpy(), bootstrap.weights(seed, R, n_chk).astype(np.float64)):
            raise SystemExit("the materialised weights are not bootstrap.weights")
        E, ii, kk = entries(mom, c.u, lib)
        G = torch.zeros((R, N_ARMS, F, F), dtype=torch.float64, device=dev)
        nT = ii.numel()

        def torch_run():
            P = torch.matmul(W, E).view(R, N_ARMS, nE)
            G[:, :, ii, kk] = P[:, :, :nT]
            G[:, :, kk, ii] = P[:, :, :nT]
            b = P[:, :, nT:].contiguous()
            return G, b, ops.stlsq(G, b, a.threshold, a.alpha)

        t_t, t_mm = runs_of(torch_run, a), runs_of(lambda: torch.matmul(W, E), a)
        G_t, b_t, (coef_t, mask_t, _) = torch_run()
        torch.cuda.synchronize()
        sys_scale = G_k.abs().amax(dim=(2, 3))
        agree = float(max(((G_t - G_k).abs().amax(dim=(2, 3)) / sys_scale).max(),
                          ((b_t - b_k).abs().amax(dim=2) / sys_scale).max()))
        res["torch_composition"] = dict(t_t, matmul_only_ms_runs=t_mm["ms_runs"], matmul_only_ms=t_mm["ms"],
                                        weights_build_ms=t0.elapsed_time(t1), weights_bytes=float(R) * N * 8,
                                        speedup_of_bootstrap=t_t["ms"] / t_f["ms"],
                                        gram_max_diff_of_largest_entry=agree,
                                        masks_equal=bool(torch.equal(mask.view(-1, F), mask_t)),
                                        coef_max_diff=float((coef.view(-1, F) - coef_t).abs().max()))
        del W, E
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    if not rep0 <= 1e-10:
        raise SystemExit(f"replicate 0 differs from ops.gram_segments by {rep0:.3e} of the largest entry")
    if not agree <= 1e-10:
        raise SystemExit(f"G | b of the two paths differ by {agree:.3e} of the largest entry")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, nargs="+", default=[1_000_000, 100_000])
    ap.add_argument("--replicates", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fd", default="order1", choices=["order1", "smoothed1"])
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--max-weight-bytes", type=float, default=64e9,
                    help="the composition is skipped where its [R, N] f64 weights are larger")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segboot", "bench_segboot.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segboot needs the GPU: there is no CPU fallback to time")
    dev = torch.device("cuda:0")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    for N in a.patients:
        one_shape(N, a.replicates, a, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
