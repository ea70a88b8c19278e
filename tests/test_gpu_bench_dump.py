"""GPU (-m gpu): `bench.py --dump-outputs DIR` on a plain run -- two runs with the same arguments write the same outputs, array for
array (seeds, actions and step counts do not depend on timing), the frames are what a caller of the step received (uint8 values
as float32), and the plain line is the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(d):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs-per-gpu", "2048", "--steps", "16", "--warmup", "4",
                          "--settle", "20", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-500:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    j = _run(tmp_path / "a")
    assert j["steps"] == 16 and j["value"] > 1e5 and j["ms_per_step"] > 0 and j["full"] is False
    assert "roofline" not in j and "value_windows" not in j and "cpu_baseline" not in j
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert {"obs.npy", "reward.npy", "terminated.npy", "truncated.npy", "sample_rows.npy"} <= set(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    obs = a["obs.npy"]
    assert obs.shape == (256, 84, 84, 3) and obs.min() >= 0 and obs.max() <= 255 and np.array_equal(obs, np.round(obs)) and obs.max() > 0
    assert a["reward.npy"].shape == (2048,) and set(np.unique(a["terminated.npy"])) <= {0.0, 1.0}
    _run(tmp_path / "b")
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), f
