"""GPU (-m gpu): the spotlight family's fused raster / reset launch (spot_raster_serve_kernel<EN, BORDER, NT, FINAL, FMT>, csrc/mg_spot_serve.hpp) in
the image-order formats (bf16_chw, f16_chw, f32_chw, u8_chw), with and without kept terminal observations.

Comparisons are exact and made by tests/chw_referee.py: a float frame is the oracle's uint8 frame through its 256-entry table.  Which launches
ran is asserted from the host-side counters of mg_debug_counter: "final_obs_generic_steps" (mg_step's generic terminal-observation branch) and
"spot_fused_steps" (step() calls that went out as spot_raster_serve_kernel).  The inputs, and what the oracle alone says about them, are in
tests/test_spot_chw_inputs.py."""
import json
import os
import subprocess
import sys

import pytest

from chw_referee import (CHW, clones, converted, lock_step_with_a_twin, lock_step_with_the_oracle, replay_captured, same_steps,
                         two_option_sets_keep_the_generic_path)
from test_spot_chw_inputs import FORCED, IDS, IN_STEP, ONE_ROUND, ROUNDS, SHORT, TERMINAL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAB_LIB = os.path.join(ROOT, "endless-memory-gym_amd", "lib", "lab", "libmemgym_hip_lab.so")
FINITE, ENDLESS = IDS


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in CHW])  # (id by id: oracle_run is shared)
def test_terminal_frames_against_the_oracle(env_id, fmt):
    n, steps = TERMINAL["n"], TERMINAL["steps"]
    n_done, n_running, _, env = lock_step_with_the_oracle(env_id, fmt, n, steps, SHORT[env_id])
    assert n_done >= 6 * n and n_running >= n, (n_done, n_running)
    assert env.debug_counter("final_obs_generic_steps") == 0  # the step's own launches kept the terminal observations
    assert env.debug_counter("spot_fused_steps") == steps
    env.close()


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in ("bf16_chw", "u8_chw")])
def test_more_than_one_service_round(env_id, fmt):
    """4,163 instances, nearly all truncated in the same step (9 and 18): more than 512 x 8 queue entries, so workgroups 0 .. 8 serve a second
    round at batch 8 (base += SPOT_SVC_WGS * batch); and a count that is no multiple of 64 or of the batch."""
    n, steps = ROUNDS["n"], ROUNDS["steps"]
    assert n % 64 != 0
    _, _, most, env = lock_step_with_the_oracle(env_id, fmt, n, steps, IN_STEP[env_id], frames=False)
    assert most > ONE_ROUND, most  # otherwise the run did not reach the second round
    assert env.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("spot_fused_steps") == steps
    env.close()


@pytest.mark.parametrize("env_id,fmt", [(FINITE, "bf16_chw"), (FINITE, "f32_chw"), (FINITE, "u8_chw"), (ENDLESS, "bf16_chw")])
def test_the_batch_of_eight_regime(env_id, fmt):
    """Beyond 12,288 instances a service workgroup takes eight queue entries per round whatever the count (batch_min = 8); 12,355 is no
    multiple of 64.  Against a u8_xyc twin handle stepped with the same actions.  With terminal observations kept both ids defer at this size."""
    n, steps = 12288 + 67, 12
    finished, xyc, env = lock_step_with_a_twin(env_id, fmt, n, steps, SHORT[env_id])
    n_done = sum(finished)
    assert n_done >= n, n_done  # (max_steps = 9: every instance finished within the 12 steps)
    assert env.debug_counter("final_obs_generic_steps") == 0 and xyc.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("spot_fused_steps") == steps
    for e in (xyc, env):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("batch", [None, 3])
def test_plain_autoreset_fused_launch_forced(batch):
    """Lab library, MEMGYM_SPOT_FUSE=1: the fused launch without kept terminal observations, whatever fuse_resets() would choose for the size;
    once more with MEMGYM_SPOT_SVC_BATCH=3, a batch that divides neither 8 nor the counts.  tests/chw_worker.py runs both ids in bf16_chw
    and u8_chw against the oracle in one process."""
    env = dict(os.environ, MEMGYM_HIP_LIB=LAB_LIB, MEMGYM_SPOT_FUSE="1")
    if batch:
        env["MEMGYM_SPOT_SVC_BATCH"] = str(batch)
    cases = ["%s:%s" % (e, f) for e in IDS for f in ("bf16_chw", "u8_chw")]
    assert SHORT[FINITE] == SHORT[ENDLESS]  # (the worker takes one set of options)
    # four runs of 40 steps of 96 instances next to ~10 s of imports and oracle; 300 s is far beyond any run that makes progress
    r = subprocess.run([sys.executable, os.path.join(HERE, "chw_worker.py"), str(FORCED["n"]), str(FORCED["steps"]), json.dumps(SHORT[FINITE]),
                        "--expect", "spot_fused_steps=%d" % FORCED["steps"]] + cases, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("ok:") == len(cases), r.stdout[-2000:] + r.stderr[-4000:]


def test_two_option_sets_keep_the_generic_path():
    """Per-instance option sets: the plain arrangement and mg_step's generic path for terminal observations, and the counters say so.
    (A guard: this holds before and after the fused launch learnt the image-order formats.)"""
    two_option_sets_keep_the_generic_path(FINITE, SHORT[FINITE], dict(SHORT[FINITE], max_steps=5), 12, "spot_fused_steps")


def test_graph_replay_of_a_bf16_handle_keeps_the_plain_arrangement():
    """Under capture a bf16_chw handle takes the two plain launches as before; the replay equals a u8_xyc twin's eager steps."""
    import memory_gym_amd
    import torch

    n, K = 512, 8
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = [torch.randint(0, 3, (n, 2), device="cuda", generator=g, dtype=torch.int32) for _ in range(K)]
    twin = memory_gym_amd.make(FINITE, num_envs=n, device=0, obs_format="u8_xyc")
    twin.reset(seed=9, options=SHORT[FINITE])
    want = []
    for a in acts:
        o, r, d, _, _ = twin.step(a)
        want.append((converted("bf16_chw", o), r.clone(), d.clone()))
    assert sum(int(d.sum()) for _, _, d in want) > 0
    env = memory_gym_amd.make(FINITE, num_envs=n, device=0, obs_format="bf16_chw")
    env.reset(seed=9, options=SHORT[FINITE])
    before = []
    same_steps(want, replay_captured(env, acts, clones, lambda: before.append(env.debug_counter("spot_fused_steps"))))
    assert env.debug_counter("spot_fused_steps") == before[0]  # captured steps are not the fused launch
    env.check_errors()
    twin.close()
    env.close()
