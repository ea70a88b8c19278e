"""CPU: what a plain `bench.py` run does and what `--dump-outputs` writes.  A plain run is the headline alone -- everything else the
benchmark measures or checks waits for `--full` (tests/test_bench_guard.py runs that side with a stand-in for the measurement) --
and the dump is what a caller of the timed step received, as float32 / float64 arrays, frames sampled, at most 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _line(args):
    env = dict(os.environ, MEMGYM_BENCH_FAKE="1")
    env.pop("MEMGYM_BENCH_TEST_FAULT", None)
    p = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-400:]
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", ["1", "2"])
def test_plain_run_is_the_headline_alone(gpus):
    j = _line(["--gpus", gpus, "--backend", "gloo", "--steps", "10", "--warmup", "2"])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 10 and j["warmup"] == 2 and j["full"] is False and j["n_gpus"] == int(gpus)
    for k in ("config5", "value_windows", "value_2000", "roofline", "cpu_baseline", "c1", "secondary_workloads", "other_workloads"):
        assert k not in j, k


def test_full_run_keeps_the_rest():
    j = _line(["--gpus", "2", "--backend", "gloo", "--steps", "10", "--warmup", "2", "--full"])
    assert j["full"] is True and "value_windows" in j and "value_2000" in j and "config5" in j


def test_host_outputs_names_dtypes_and_sample():
    n = 1000
    obs = torch.arange(n * 84 * 84 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(n, 84, 84, 3)
    rew = torch.linspace(0, 1, n, dtype=torch.float32)
    done = torch.arange(n) % 7 == 0
    info = {"done_mask": done, "length": torch.arange(n, dtype=torch.int32), "ground_truth": torch.ones(n, 3, dtype=torch.float64),
            "final_observation": obs, "_final_observation": done, "final_info": {"reward": rew}, "note": "not an array"}
    out = bench.host_outputs((obs, rew, done, torch.zeros(n, dtype=torch.bool), info), n)
    rows = out["sample_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0) and rows.max() < n
    assert np.array_equal(rows, bench.host_outputs((obs,), n)["sample_rows"])  # the same rows every time
    assert sorted(out) == sorted(["sample_rows", "obs", "reward", "terminated", "truncated", "info_done_mask", "info_length", "info_ground_truth",
                                  "info_final_observation", "info__final_observation", "info_final_info_reward"])
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["obs"].shape == (bench.DUMP_ROWS, 84, 84, 3) and out["obs"].dtype == np.float32
    assert np.array_equal(out["obs"], obs.numpy()[rows].astype(np.float32))
    assert out["reward"].shape == (n,) and np.array_equal(out["reward"], rew.numpy())
    assert out["info_length"].dtype == np.float64 and out["info_ground_truth"].dtype == np.float64
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_LIMIT


def test_write_outputs(tmp_path):
    bench.write_outputs({"obs": np.ones((2, 3), np.float32)}, str(tmp_path / "d"), "_rank1")
    assert np.array_equal(np.load(tmp_path / "d" / "obs_rank1.npy"), np.ones((2, 3), np.float32))
