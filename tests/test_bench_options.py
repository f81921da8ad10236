"""bench.py's run options (host logic, no GPU): a run without --full is lean -- everything measured beside the
headline figure is switched off -- and --dump-outputs writes float32 / float64 arrays within its size budget, a large
output as the same seeded sample of its slices on every run."""
import argparse
import os
import sys

import numpy as np
import torch

import bench

EXTRAS = ("no_cpu_baseline", "no_parity", "no_north_star", "no_c3_block", "no_fused", "insite_only_binned")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_the_extras_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 3, None)
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_run_keeps_the_extras_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = _parse(monkeypatch, "--full", "--no-parity")
    assert a.no_parity and not a.no_cpu_baseline


def test_headline_has_the_result_fields(monkeypatch):
    a = _parse(monkeypatch, "--steps", "7", "--warmup", "3")
    line = bench.headline(a, 2.0e6, 0.5, 1, "weak", "f64", "data", "workload")
    assert line["metric"] == bench.METRIC and line["unit"] == "patient-trajectories/s"
    assert (line["value"], line["ms_per_step"], line["steps"], line["warmup"]) == (2.0e6, 0.5, 7, 3)
    assert line["higher_is_better"] is True and line["dtype"] == "f64"


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    y = torch.arange(200 * 100_000, dtype=torch.float64).view(200, 100_000)       # 160 MB: sampled
    z = torch.ones((5, 3, 70_001), dtype=torch.float32)                          # under its share: whole
    arrays = {"coef": torch.full((2, 7), 0.5, dtype=torch.float64), "mask": torch.ones((2, 7), dtype=torch.int8),
              "iters": torch.tensor([3, 4], dtype=torch.int32), "y": (y, 1), "z": (z, 2)}
    dirs = [str(tmp_path / "a"), str(tmp_path / "b" / "nested")]
    for d in dirs:
        bench.dump_outputs(argparse.Namespace(dump_outputs=d), arrays)
    got = {f[:-4]: np.load(os.path.join(dirs[0], f)) for f in sorted(os.listdir(dirs[0]))}
    assert sorted(got) == ["coef", "iters", "mask", "y", "y_index", "z"]
    assert all(v.dtype == (np.float32 if k == "z" else np.float64) for k, v in got.items())
    assert sum(v.nbytes for v in got.values()) <= 64e6
    idx = got["y_index"].astype(np.int64)
    assert idx.size > 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 100_000
    assert np.array_equal(got["y"], y[:, idx].numpy())
    assert np.array_equal(got["z"], z.numpy()) and np.array_equal(got["iters"], [3.0, 4.0])
    for f in os.listdir(dirs[0]):       # the same arrays, the same sample, on every run
        assert np.array_equal(np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f)))


def test_dump_outputs_is_off_without_the_option(tmp_path):
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), {"coef": torch.zeros(2)})
    assert os.listdir(tmp_path) == []
