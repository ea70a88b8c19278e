"""GPU (-m gpu): Endless-MysteryPath-v0's fused raster / service launch (emp_raster_serve_kernel<FMT, EMP_NT, FINAL>,
csrc/mg_mystery_endless_launch.hpp) in the image-order formats (bf16_chw, f16_chw, f32_chw, u8_chw), with and without kept terminal observations,
and what comes with the fused arrangement: lazy initial segments, records ahead of time, the fast masked reset.

Comparisons are exact and made by tests/chw_referee.py: a float frame is the oracle's uint8 frame through its 256-entry table.  Which launches
ran is asserted from the host-side counters of mg_debug_counter: "final_obs_generic_steps" (mg_step's generic terminal-observation branch) and
"emp_fused_steps" (step() calls that went out as emp_raster_serve_kernel).  The inputs, and what the oracle alone says about them, are in
tests/test_emp_chw_inputs.py."""
import numpy as np
import pytest

from chw_referee import (CHW, SENTINEL, clones, converted, lock_step_with_a_twin, lock_step_with_the_oracle, replay_captured, rows_to_bytes,
                         same_steps, two_option_sets_keep_the_generic_path)
from test_emp_chw_inputs import ENV_ID, FORCED, IN_STEP, LANES, ONE_ROUND, ONE_ROUND_PRE, ROUNDS, SHORT, TERMINAL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", CHW)
def test_terminal_frames_against_the_oracle(fmt):
    n, steps = TERMINAL["n"], TERMINAL["steps"]
    n_done, n_running, _, env = lock_step_with_the_oracle(ENV_ID, fmt, n, steps, SHORT)
    assert n_done >= 6 * n and n_running >= n, (n_done, n_running)
    assert env.debug_counter("final_obs_generic_steps") == 0  # the step's own launches kept the terminal observations
    assert env.debug_counter("emp_fused_steps") == steps
    env.close()


def test_terminal_frames_of_a_single_instance():
    """n = 1: one frame workgroup, and a service workgroup whose other three waves have no entry."""
    import frame_digest as fd
    import memory_gym_amd
    import oracle_lib
    import torch

    fmt, steps = "bf16_chw", 40
    ref = oracle_lib.OracleBatch(ENV_ID, 1, options=SHORT)
    env = memory_gym_amd.make(ENV_ID, num_envs=1, device=0, obs_format=fmt, final_observation=True)
    seeds = np.array([31], dtype=np.int64)
    first = ref.reset_digest(seeds)
    obs = env.reset(seed=seeds, options=SHORT)[0]
    assert len(fd.differing(fd.digest_torch(rows_to_bytes(fmt, obs)), first)) == 0
    prng = np.random.Generator(np.random.PCG64(6))
    n_done = 0
    for t in range(steps):
        a = prng.integers(0, 4, (1,)).astype(np.int32)
        dg, fdg, rew, done = ref.step_digest(a, autoreset=True)
        env.final_obs.fill_(SENTINEL[fmt])
        obs, r, d, _, info = env.step(a)
        assert np.array_equal(d.cpu().numpy(), done.astype(bool)) and np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), "step %d" % t
        b = rows_to_bytes(fmt, obs)
        assert torch.equal(converted(fmt, b), obs) and len(fd.differing(fd.digest_torch(b), dg)) == 0, "the frame differs from the oracle's at step %d" % t
        rows = info["final_observation"]
        if done[0]:
            fb = rows_to_bytes(fmt, rows)
            assert torch.equal(converted(fmt, fb), rows) and len(fd.differing(fd.digest_torch(fb), fdg)) == 0, "the terminal frame differs at step %d" % t
        else:
            assert bool((rows == SENTINEL[fmt]).all()), "the row of the running instance was written at step %d" % t
        n_done += int(done[0])
    assert n_done >= 4, n_done
    assert env.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("emp_fused_steps") == steps
    env.check_errors()
    env.close()
    ref.close()


@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
def test_more_than_one_service_round(fmt):
    """4,163 instances, nearly all truncated in the same step (9 and 18): more than 768 x 4 queue entries, so service waves fetch a second
    entry through QC_HEAD; and a count that is no multiple of 64."""
    n, steps = ROUNDS["n"], ROUNDS["steps"]
    _, _, most, env = lock_step_with_the_oracle(ENV_ID, fmt, n, steps, IN_STEP, frames=False)
    assert most > ONE_ROUND, most  # otherwise the run did not reach the second round
    assert env.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("emp_fused_steps") == steps
    env.close()


@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
def test_the_lane_regime(fmt):
    """20,481 instances: the handle leaves bg_coop -- the lane generator in background workgroups, records ahead of time (EMP_PRE), 64 service
    workgroups, plain stores -- and more than 64 x 4 instances finish in one step."""
    n, steps = LANES["n"], LANES["steps"]
    _, _, most, env = lock_step_with_the_oracle(ENV_ID, fmt, n, steps, IN_STEP, frames=False)
    assert most > ONE_ROUND_PRE, most
    assert env.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("emp_fused_steps") == steps
    assert env.debug_counter("emp_ahead_records") > 0  # background workgroups generated next episodes' first segments
    env.close()


@pytest.mark.parametrize("fmt", CHW)
def test_plain_autoreset_steps_against_the_oracle(fmt):
    """final_observation=False: the fused launch in its plain form.  No format is excluded from the fused arrangement (profiles/emp_chw.md,
    csrc/mg_mystery.hip steps_fused()), so the product library runs it for all four."""
    n, steps = FORCED["n"], FORCED["steps"]
    n_done, _, _, env = lock_step_with_the_oracle(ENV_ID, fmt, n, steps, SHORT, final=False)
    assert n_done > n
    assert env.debug_counter("emp_fused_steps") == steps
    env.close()


@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
def test_masked_reset_in_mid_run(fmt):
    """reset(seed=None, mask=...) between steps: the fast path (emp_masked_reset_kernel: lazy segments, records ahead of time where there are any).
    Against a u8_xyc twin given the same actions and masks: the frames right after each reset and over 20 further steps, rewards, dones."""
    import torch

    n = 160

    def masked_resets(t, twin, env, g):
        if t in (7, 12):  # two masked resets five steps apart: the second meets instances the first one left with owed segments
            mask = torch.rand(n, device="cuda", generator=g) < 0.4
            assert 0 < int(mask.sum()) < n
            o_x, o_c = twin.reset(mask=mask)[0], env.reset(mask=mask)[0]
            assert torch.equal(o_c, converted(fmt, o_x)), "%s: frames differ right after the masked reset before step %d" % (fmt, t)

    finished, twin, env = lock_step_with_a_twin(ENV_ID, fmt, n, 7 + 5 + 5 + 15, SHORT, final=False, seed=3, action_seed=11, between=masked_resets)
    assert sum(finished[-15:]) > 0
    for e in (twin, env):
        e.check_errors()
        e.close()


def test_two_option_sets_keep_the_generic_path():
    """Per-instance option sets: the plain arrangement and mg_step's generic path for terminal observations, and the counters say so.
    (A guard: this holds before and after the fused launch learnt the image-order formats.)"""
    two_option_sets_keep_the_generic_path(ENV_ID, SHORT, dict(SHORT, max_steps=5), 12, "emp_fused_steps")


def test_graph_replay_of_a_bf16_handle_equals_a_u8_xyc_twin():
    """Under capture this id steps fused in u8_xyc (tests/test_gpu_graph_capture.py); the image-order formats do the same.  The replay of 30
    captured bf16_chw steps equals a u8_xyc twin's eager steps, terminal rows included."""
    import memory_gym_amd
    import torch

    n, K, fmt = 512, 30, "bf16_chw"
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = [torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32) for _ in range(K)]
    twin = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, obs_format="u8_xyc", final_observation=True)
    twin.reset(seed=9, options=IN_STEP)
    want, finished = [], 0
    for a in acts:
        o, r, d, _, info = twin.step(a)
        want.append((converted(fmt, o), r.clone(), d.clone(), converted(fmt, info["final_observation"][d])))
        finished += int(d.sum())
    assert finished > n
    env = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, obs_format=fmt, final_observation=True)
    env.reset(seed=9, options=IN_STEP)
    before = []
    outs = replay_captured(env, acts, lambda out: clones(out, final=True), lambda: before.append(env.debug_counter("emp_fused_steps")))
    same_steps(want, outs)
    for k, ((_, _, d1, f1), (_, _, _, f2)) in enumerate(zip(want, outs)):
        assert torch.equal(f1, f2[d1]), "terminal observations of step %d differ in the replay" % k
    assert env.debug_counter("emp_fused_steps") == before[0] + K  # the captured steps were the fused launch
    assert env.debug_counter("final_obs_generic_steps") == 0
    env.check_errors()
    twin.close()
    env.close()


def test_checkpoint_in_mid_run_carries_owed_segments_and_records():
    """A bf16_chw handle's state_dict taken at step 15 of 30 loads into a fresh handle, which finishes the run like the first: handles in the
    image-order formats now carry owed segments (lazy resets) and records ahead of time in their state."""
    import memory_gym_amd
    import torch

    n, steps, fmt = 160, 30, "bf16_chw"
    g = torch.Generator(device="cuda").manual_seed(13)
    acts = [torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32) for _ in range(steps)]
    env = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, obs_format=fmt)
    env.reset(seed=17, options=SHORT)
    for a in acts[:steps // 2]:
        env.step(a)
    snap = env.state_dict()
    want, finished = [], 0
    for a in acts[steps // 2:]:
        o, r, d, _, info = env.step(a)
        want.append((o.clone(), r.clone(), d.clone(), info["ground_truth"].clone()))
        finished += int(d.sum())
    assert finished > n
    fresh = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, obs_format=fmt)
    fresh.load_state_dict(snap)
    for k, (a, (o1, r1, d1, g1)) in enumerate(zip(acts[steps // 2:], want)):
        o2, r2, d2, _, info = fresh.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(g1, info["ground_truth"]), "step %d after the restore differs" % k
    assert fresh.debug_counter("emp_fused_steps") == steps - steps // 2
    for e in (env, fresh):
        e.check_errors()
        e.close()
