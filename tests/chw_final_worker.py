"""Worker of tests/test_gpu_chw_final.py::test_rescue_path_in_a_float_kernel (a process of its own: the lab library and its switches are
chosen by the environment before the package loads).  usage: chw_final_worker.py ENV_ID N STEPS OBS_FORMAT

final_observation=True, short episodes; after every step all N frames and the terminal frames of the finished instances are turned back into
bytes on the device -- exactly: every value must be the table's value of its byte -- and their digests compared with the oracle's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "endless-memory-gym_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frame_digest as fd  # noqa: E402
import memory_gym_amd  # noqa: E402
import oracle_lib  # noqa: E402
from test_gpu_chw_final import SHORT, converted, rows_to_bytes  # noqa: E402

env_id, n, steps, fmt = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]


def exact_bytes(rows, what):
    b = rows_to_bytes(fmt, rows)
    assert torch.equal(converted(fmt, b), rows), "%s: a value no byte maps to" % what
    return b


ref = oracle_lib.OracleBatch(env_id, n, options=SHORT[env_id])
env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=True)
seeds = np.arange(n, dtype=np.int64)
obs = env.reset(seed=seeds, options=SHORT[env_id])[0]
assert len(fd.differing(fd.digest_torch(exact_bytes(obs, "reset")), ref.reset_digest(seeds))) == 0, "reset frames differ from the oracle's"
prng = np.random.Generator(np.random.PCG64(8))
n_done = 0
for t in range(steps):
    a = (prng.integers(0, 4, n) if ref.discrete else prng.integers(0, 3, (n, 2))).astype(np.int32)
    obs, r, d, _, info = env.step(a)
    dg, fdg, rew, done = ref.step_digest(a, autoreset=True)
    d_host = d.cpu().numpy()
    assert np.array_equal(d_host, done.astype(bool)) and np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), "rewards / dones differ at step %d" % t
    bad = fd.differing(fd.digest_torch(exact_bytes(obs, "step %d" % t)), dg)
    assert len(bad) == 0, "frames of instances %s differ from the oracle's at step %d" % (bad[:8], t)
    if d_host.any():
        bad = fd.differing(fd.digest_torch(exact_bytes(info["final_observation"][d], "terminal rows, step %d" % t)), fdg[d_host])
        assert len(bad) == 0, "terminal frames differ from the oracle's at step %d" % t
    n_done += int(d_host.sum())
env.check_errors()
assert n_done > n, n_done
assert env.debug_counter("one_launch_steps") == steps and env.debug_counter("final_obs_generic_steps") == 0
print("RESCUES", env.debug_counter("one_launch_rescues"))
env.close()
ref.close()
print("ok:", env_id, n, steps, fmt, n_done)
