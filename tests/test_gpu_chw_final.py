"""GPU (-m gpu): terminal observations kept inside the step's own launches in the image-order formats (bf16_chw, f16_chw, f32_chw, u8_chw) on the
mortar family (mortar_step_raster_kernel<false, FINAL, FMT>, csrc/mg_mortar_one_launch.hpp) and the finite Mystery Path ids
(mystery_raster_paths_kernel<FMT, true>, csrc/mg_mystery_finite.hpp).

Floats are compared EXACTLY: a float observation is the oracle's uint8 [x][y][c] frame / np.float32(255) transposed to [c][y][x], the 16-bit
formats that quotient rounded -- a table of 256 values (tests/chw_referee.py, which holds every comparison made here), no tolerance.  Which
path ran is asserted from the host-side counters of mg_debug_counter: "final_obs_generic_steps" (mg_step's generic terminal-observation
branch; must stay 0) and, on the mortar ids, "one_launch_steps"."""
import json
import os
import subprocess
import sys

import pytest

from chw_referee import (FLOATS, SHORT, clones, lock_step_with_a_twin, lock_step_with_the_oracle, replay_captured, same_steps,
                         two_option_sets_keep_the_generic_path)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAB_LIB = os.path.join(ROOT, "endless-memory-gym_amd", "lib", "lab", "libmemgym_hip_lab.so")

MORTAR = ("MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0")
MYSTERY = ("MysteryPath-Grid-v0", "MysteryPath-v0")

FINAL_CASES = [(e, f) for e in MORTAR for f in FLOATS] + [(e, f) for e in MYSTERY for f in FLOATS + ("u8_chw",)]  # (id by id: oracle_run is shared)


@pytest.mark.parametrize("env_id,fmt", FINAL_CASES)
def test_terminal_frames_against_the_oracle(env_id, fmt):
    n, steps = 48, 60
    n_done, n_running, _, env = lock_step_with_the_oracle(env_id, fmt, n, steps, SHORT[env_id])
    assert n_done > n and n_running > n, (n_done, n_running)  # both kinds of row were seen, many times
    assert env.debug_counter("final_obs_generic_steps") == 0  # the step's own launches kept the terminal observations
    if env_id in MORTAR:
        assert env.debug_counter("one_launch_steps") == steps
    env.close()


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in MORTAR for f in FLOATS])
def test_plain_autoreset_steps_against_the_oracle(env_id, fmt):
    n, steps = 96, 40
    n_done, _, _, env = lock_step_with_the_oracle(env_id, fmt, n, steps, SHORT[env_id], final=False)
    assert n_done > n
    assert env.debug_counter("one_launch_steps") == steps  # every float format ships in the one-launch form (profiles/chw_final.md)
    assert env.debug_counter("final_obs_generic_steps") == 0
    env.close()


@pytest.mark.parametrize("env_id,fmt", [("MortarMayhem-Grid-v0", "bf16_chw"), ("MortarMayhem-Grid-v0", "f32_chw"), ("MysteryPath-Grid-v0", "bf16_chw")])
def test_more_than_one_frame_per_workgroup(env_id, fmt):
    """Just above the raster grid (14,336 persistent workgroups, mg_raster_v1.hpp RASTER_GRID) and no multiple of 64: 67 workgroups draw two
    frames (and their terminal frames), the last 64-instance claim slot of the one-launch step holds 3 instances.  Against a u8_xyc twin handle."""
    n, steps = 14336 + 67, 12
    assert n % 64 != 0
    finished, xyc, env = lock_step_with_a_twin(env_id, fmt, n, steps, SHORT[env_id])
    n_done = sum(finished)
    assert n_done >= n, n_done  # (episodes under SHORT last 7 steps at the most: every instance finished within the 12, so every workgroup drew terminal frames)
    assert env.debug_counter("final_obs_generic_steps") == 0 and xyc.debug_counter("final_obs_generic_steps") == 0
    if env_id in MORTAR:
        assert env.debug_counter("one_launch_steps") == steps
    for e in (xyc, env):
        e.check_errors()
        e.close()


def test_rescue_path_in_a_float_kernel():
    """The step workgroups at the END of the grid (lab build, MEMGYM_LAB_LOGIC_LAST=1; tests/test_gpu_one_launch.py): frame waves of the bf16
    FINAL kernel step the slots themselves.  tests/chw_worker.py compares every frame and every terminal frame with the oracle (inputs of its
    own: seeds arange(n), actions from PCG64(8))."""
    env_id, n, steps = "MortarMayhem-Grid-v0", 4096, 30
    env = dict(os.environ, MEMGYM_HIP_LIB=LAB_LIB, MEMGYM_LAB_LOGIC_LAST="1")
    # 30 steps of 4,096 instances: three rounds of frame workgroups per step, each waiting RESCUE_AFTER_TICKS (200 us) at most once, next
    # to ~10 s of imports, oracle and digests; 300 s is far beyond any run that makes progress
    r = subprocess.run([sys.executable, os.path.join(HERE, "chw_worker.py"), str(n), str(steps), json.dumps(SHORT[env_id]), "--final", "--seed0", "0",
                        "--action-seed", "8", "--expect", "one_launch_steps=%d" % steps, "--expect", "final_obs_generic_steps=0", "--rescues",
                        env_id + ":bf16_chw"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rescues = int(r.stdout.split("RESCUES")[1].split()[0])
    assert rescues > 0, "the frame waves never had to step a slot themselves: the test did not exercise the path"


def test_graph_replay_of_a_bf16_handle_equals_eager():
    """Under capture the mortar family keeps its two-launch form in the float formats as well: captured steps are not one-launch steps."""
    import memory_gym_amd
    import torch

    env_id, n, K = "MortarMayhem-Grid-v0", 512, 8
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = [torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32) for _ in range(K)]
    eager = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="bf16_chw")
    eager.reset(seed=9)
    want = [clones(eager.step(a)) for a in acts]
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="bf16_chw")
    env.reset(seed=9)
    before = []
    same_steps(want, replay_captured(env, acts, clones, lambda: before.append(env.debug_counter("one_launch_steps"))))
    assert env.debug_counter("one_launch_steps") == before[0]  # captured steps are not the one-launch kernel
    env.check_errors()
    eager.close()
    env.close()


def test_two_option_sets_keep_the_generic_path():
    """Per-instance option sets: mg_step keeps terminal observations on its generic path, and the counter says so."""
    env_id = "MortarMayhem-Grid-v0"
    two_option_sets_keep_the_generic_path(env_id,SHORT[env_id], dict(SHORT[env_id], command_count=[3]), 10, "one_launch_steps")
