"""Worker of tests/test_gpu_chw_final.py::test_rescue_path_in_a_float_kernel and tests/test_gpu_spot_chw.py::
test_plain_autoreset_fused_launch_forced (a process of its own: the lab library and its switches are chosen by the environment before the
package loads).  usage: chw_worker.py N STEPS OPTIONS [--final] [--seed0 S] [--action-seed A] [--expect COUNTER=VALUE ...] [--rescues]
ENV_ID:OBS_FORMAT [ENV_ID:OBS_FORMAT ...]

Every case runs tests/chw_referee.py's lock_step_with_the_oracle under the reset options OPTIONS (JSON), frames by digest: after every step
all N frames (--final: and the terminal rows) are turned back into bytes on the device -- exactly: every value must be the table's value of
its byte -- and their digests compared with the oracle's.  More than N instances must finish, and every COUNTER must read VALUE afterwards."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "endless-memory-gym_amd")]

from chw_referee import lock_step_with_the_oracle  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("n", type=int)
p.add_argument("steps", type=int)
p.add_argument("options", type=json.loads)
p.add_argument("cases", nargs="+")
p.add_argument("--final", action="store_true")
p.add_argument("--seed0", type=int, default=31)
p.add_argument("--action-seed", type=int, default=6)
p.add_argument("--expect", action="append", default=[])
p.add_argument("--rescues", action="store_true")
args = p.parse_args()

for case in args.cases:
    env_id, fmt = case.split(":")
    n_done, _, _, env = lock_step_with_the_oracle(env_id, fmt, args.n, args.steps, args.options, frames=False, final=args.final,
                                                  seed0=args.seed0, action_seed=args.action_seed)
    assert n_done > args.n, n_done
    for counter, value in (e.split("=") for e in args.expect):
        assert env.debug_counter(counter) == int(value), (counter, env.debug_counter(counter))
    if args.rescues:
        print("RESCUES", env.debug_counter("one_launch_rescues"))
    env.close()
    print("ok:", env_id, args.n, args.steps, fmt, n_done)
