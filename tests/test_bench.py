"""bench.py --dump-outputs and --steps: what the timed path computed, written for output-for-output comparison."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_sample_is_fixed_and_bounded():
    small = torch.randn(3, 4)
    assert torch.equal(bench.dump_sample(small), small)
    big = torch.randn(bench.DUMP_MAX_ELEMS + 12345)
    a, b = bench.dump_sample(big), bench.dump_sample(big.clone())
    assert a.shape == (bench.DUMP_MAX_ELEMS,) and torch.equal(a, b)
    p = bench.dump_sample(big, 1000)
    assert p.shape == (1000,) and np.isin(p.numpy(), big.numpy()).all()


def test_dump_outputs_dtypes_and_budget(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"a": torch.ones(2, 3, dtype=torch.bfloat16), "b": torch.zeros(4, dtype=torch.float64),
                                             "c": torch.tensor(0.5)})
    got = {f: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert {k: (v.dtype, v.shape) for k, v in got.items()} == {
        "a.npy": (np.float32, (2, 3)), "b.npy": (np.float64, (4,)), "c.npy": (np.float32, ())}
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "e"), {"x": torch.zeros(bench.DUMP_BUDGET_BYTES // 4 + 1)})
    assert not (tmp_path / "e").exists() or not os.listdir(tmp_path / "e")


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "7"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_full_is_off_by_default():
    assert not bench.parse_args([]).full
    assert bench.parse_args(["--full"]).full


@pytest.mark.gpu
def test_full_adds_what_a_plain_run_leaves_out():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "cfg2-64"]
    lines = []
    for extra in ([], ["--full"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, full = lines
    for line in lines:
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0
    assert plain["infer"] is None and plain["phases_ms"] is None and "cpu_baseline" not in plain
    assert full["infer"]["ms_per_step"] > 0 and full["phases_ms"]
    assert full["cpu_baseline"]["value"] > 0 and "max_abs_prob_diff_vs_cpu" in full["dice"]
    # --full adds work after the timed steps, never changes them
    assert abs(plain["final_loss"] - full["final_loss"]) <= 1e-5 * max(1.0, abs(full["final_loss"]))
    assert abs(plain["dice"]["gpu_soft_dice_loss_step0"] - full["dice"]["gpu_soft_dice_loss_step0"]) <= 1e-6


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", "cfg2-64", "--no-cpu-baseline", "--no-cfg3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    files = sorted(os.listdir(out))
    assert files == ["infer_y_pred.npy", "train_dice_loss.npy", "train_logistic_loss.npy", "train_loss.npy",
                     "train_params_sample.npy", "train_y_pred.npy"], files
    arrs = {f: np.load(out / f) for f in files}
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_BUDGET_BYTES
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert arrs["train_y_pred.npy"].shape == arrs["infer_y_pred.npy"].shape == (1, 3, 64, 64, 64)
    assert arrs["train_params_sample.npy"].shape == (bench.DUMP_PARAM_ELEMS,)
    # the dumped loss is the one the JSON line reports for the last timed step
    assert abs(float(arrs["train_loss.npy"]) - line["final_loss"]) <= 1e-6 * max(1.0, abs(line["final_loss"]))
    # probabilities: softmax over the class axis
    assert np.abs(arrs["infer_y_pred.npy"].sum(1) - 1).max() < 1e-4
