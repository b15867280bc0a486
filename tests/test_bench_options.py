"""bench.py's plain run and its two output options: a plain run times exactly ``--steps`` steps in one window and prints
the headline line only; ``--full`` brings back everything else (repeated windows, roofline, CPU baseline, the other
configs' legs); ``--dump-outputs DIR`` writes what the last timed step returned as ``DIR/<name>.npy``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
STEP_OUTPUTS = ("d_loss", "gp", "rec_loss", "loss_g", "sup_loss", "tot_loss", "preds", "out_labels", "sup_fvs")
FULL_ONLY_KEYS = ("roofline", "cpu_baseline", "parity_mode", "with_batcher", "gpu_sections", "sweep", "infer", "c5",
                  "ref_default", "dp_emulated", "loop", "dp_legs")


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pcaa_bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_windows_default_to_one_and_to_five_with_full(monkeypatch):
    b = _bench_module()
    for argv, full, windows in ((["--steps", "7"], False, 1), (["--full"], True, 5), (["--full", "--windows", "3"], True, 3),
                                (["--windows", "2"], False, 2)):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        a = b.parse()
        assert (a.full, a.windows, a.dump_outputs) == (full, windows, None), argv
    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", "out"])
    assert b.parse().dump_outputs == "out"


def test_dump_outputs_writes_float_arrays_and_samples_oversize(tmp_path, monkeypatch):
    b = _bench_module()
    out = {"tot_loss": torch.tensor(1.5), "out_labels": torch.randn(4, 8, dtype=torch.bfloat16),
           "sup_fvs": torch.randn(4, 32, dtype=torch.float64), "preds": torch.tensor([3, 0, 7, 1]), "gp": 0.25,
           "supervised": True}
    shapes = b.dump_outputs(out, str(tmp_path / "d"))
    assert shapes == {"tot_loss": [], "out_labels": [4, 8], "sup_fvs": [4, 32], "preds": [4], "gp": []}
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in shapes}
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{n}.npy" for n in shapes)
    assert got["tot_loss"].dtype == np.float32 and float(got["tot_loss"]) == 1.5
    assert got["out_labels"].dtype == np.float32 and np.array_equal(got["out_labels"], out["out_labels"].float().numpy())
    assert got["sup_fvs"].dtype == np.float64 and np.array_equal(got["sup_fvs"], out["sup_fvs"].numpy())
    assert got["preds"].dtype == np.float64 and got["preds"].tolist() == [3.0, 0.0, 7.0, 1.0]
    assert got["gp"].dtype == np.float64 and float(got["gp"]) == 0.25
    # over the limit: each array above an equal share keeps a fixed sample of its elements, the same on every call
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 100)
    first = b.dump_outputs(out, str(tmp_path / "e"))
    assert first == {"tot_loss": [], "out_labels": [5], "sup_fvs": [2], "preds": [2], "gp": []}
    assert sum(np.load(tmp_path / "e" / f"{n}.npy").nbytes for n in first) <= 100
    fv = np.load(tmp_path / "e" / "sup_fvs.npy")
    assert np.isin(fv, out["sup_fvs"].numpy().reshape(-1)).all()
    b.dump_outputs(out, str(tmp_path / "f"))
    assert all(np.array_equal(np.load(tmp_path / "e" / f"{n}.npy"), np.load(tmp_path / "f" / f"{n}.npy")) for n in first)


def test_dump_outputs_outside_the_train_workload_exits_before_any_gpu_call(tmp_path):
    res = subprocess.run([sys.executable, BENCH, "--workload", "infer", "--dump-outputs", str(tmp_path / "d")], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--dump-outputs" in res.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_line_times_exactly_the_steps_and_dumps_the_last_step(tmp_path):
    """Small shape: this test is about the line and the files, the timed workload's numerics are the parity tests'.
    Two runs with the same arguments must dump the same bits: the inputs are seeded and the fp32 sums of the timed step
    do not depend on the order its workgroups finish in."""
    B, N, K, steps = 8, 32, 8, 3

    def run(d):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B),
                            "--points", str(N), "--classes", str(K), "--dump-outputs", str(d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=500)
        assert r.returncode == 0, r.stderr[-3000:]
        return r
    res = run(tmp_path / "d")
    run(tmp_path / "again")
    for n in STEP_OUTPUTS:
        assert np.array_equal(np.load(tmp_path / "d" / f"{n}.npy"), np.load(tmp_path / "again" / f"{n}.npy")), n
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "gait sequences/sec (train step)" and d["unit"] == "sequences/s" and d["higher_is_better"]
    assert d["dtype"] == "bf16" and d["steps"] == steps and d["warmup"] == 1
    assert len(d["config"]["windows_ms_per_step"]) == 1 and d["config"]["windows_ms_per_step"][0] == d["ms_per_step"]
    assert abs(d["value"] - B / d["ms_per_step"] * 1e3) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY_KEYS if k in d], "a plain run measures the headline figure only"
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in STEP_OUTPUTS}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in got.values())
    assert got["out_labels"].shape == (B, K) and got["sup_fvs"].shape == (B, 32) and got["preds"].shape == (B,)
    assert np.array_equal(got["preds"], got["out_labels"].argmax(1))
    assert abs(float(got["tot_loss"]) - float(got["rec_loss"] + got["loss_g"] + got["sup_loss"])) <= 1e-4 * abs(float(got["tot_loss"]))
