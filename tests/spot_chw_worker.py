"""Worker of tests/test_gpu_spot_chw.py::test_plain_autoreset_fused_launch_forced (a process of its own: the lab library and its switches are
chosen by the environment before the package loads).  usage: spot_chw_worker.py N STEPS ENV_ID:OBS_FORMAT [ENV_ID:OBS_FORMAT ...]

final_observation=False, short episodes (tests/test_spot_chw_inputs.py); after every step all N frames are turned back into bytes on the device
-- exactly: every value must be the table's value of its byte -- and their digests compared with the oracle's, rewards, dones and ground truth
too.  Every step must have gone out as the fused raster / reset launch."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "endless-memory-gym_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frame_digest as fd  # noqa: E402
import memory_gym_amd  # noqa: E402
from test_gpu_chw_final import converted, rows_to_bytes  # noqa: E402
from test_spot_chw_inputs import SHORT, oracle_run  # noqa: E402

n, steps = int(sys.argv[1]), int(sys.argv[2])

for case in sys.argv[3:]:
    env_id, fmt = case.split(":")

    def exact_bytes(rows, what):
        b = rows_to_bytes(fmt, rows)
        assert torch.equal(converted(fmt, b), rows), "%s %s, %s: a value no byte maps to" % (env_id, fmt, what)
        return b

    seeds, first, run = oracle_run(env_id, n, steps, True, False)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt)
    obs = env.reset(seed=seeds, options=SHORT[env_id])[0]
    assert len(fd.differing(fd.digest_torch(exact_bytes(obs, "reset")), first)) == 0, "%s %s: reset frames differ from the oracle's" % (env_id, fmt)
    n_done = 0
    for t, (a, _, dg, _, rew, done, gt) in enumerate(run):
        obs, r, d, _, info = env.step(a)
        assert np.array_equal(d.cpu().numpy(), done.astype(bool)) and np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), \
            "%s %s: rewards / dones differ at step %d" % (env_id, fmt, t)
        bad = fd.differing(fd.digest_torch(exact_bytes(obs, "step %d" % t)), dg)
        assert len(bad) == 0, "%s %s: frames of instances %s differ from the oracle's at step %d" % (env_id, fmt, bad[:8], t)
        if gt is not None:
            assert np.array_equal(info["ground_truth"].cpu().numpy(), gt), "%s %s: ground truth differs at step %d" % (env_id, fmt, t)
        n_done += int(done.sum())
    env.check_errors()
    assert n_done > n, n_done
    assert env.debug_counter("spot_fused_steps") == steps, env.debug_counter("spot_fused_steps")
    env.close()
    print("ok:", env_id, n, steps, fmt, n_done)
