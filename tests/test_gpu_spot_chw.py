"""GPU (-m gpu): the spotlight family's fused raster / reset launch (spot_raster_serve_kernel<EN, BORDER, NT, FINAL, FMT>, csrc/mg_spot_serve.hpp) in
the image-order formats (bf16_chw, f16_chw, f32_chw, u8_chw), with and without kept terminal observations.

Comparisons are exact, as in tests/test_gpu_chw_final.py: a float frame is the oracle's uint8 frame through the 256-entry table of
tests/test_float_bytes.py.  Which launches ran is asserted from the host-side counters of mg_debug_counter: "final_obs_generic_steps" (mg_step's
generic terminal-observation branch) and "spot_fused_steps" (step() calls that went out as spot_raster_serve_kernel).  The inputs, and what the
oracle alone says about them, are in tests/test_spot_chw_inputs.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_chw_final import SENTINEL, converted, rows_to_bytes
from test_spot_chw_inputs import FORCED, IDS, IN_STEP, ONE_ROUND, ROUNDS, SHORT, TERMINAL, oracle_run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAB_LIB = os.path.join(ROOT, "endless-memory-gym_amd", "lib", "lab", "libmemgym_hip_lab.so")
FINITE, ENDLESS = IDS
CHW = ("bf16_chw", "f16_chw", "f32_chw", "u8_chw")


def lock_step_with_the_oracle(env_id, fmt, n, steps, short, frames):
    """final_observation=True, every step against the oracle: frames (frames=True: byte for byte, else by digest), rewards, dones, ground truth,
    terminal rows by digest, sentinel rows.  -> (finished rows seen, running rows seen, most finished in one step, the handle, still open)"""
    import frame_digest as fd
    import memory_gym_amd
    import torch

    opts = (SHORT if short else IN_STEP)[env_id]
    seeds, first, run = oracle_run(env_id, n, steps, short, frames)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=True)
    what = "%s %s" % (env_id, fmt)

    def same_frames(obs, want_frames, want_digest):
        if frames:
            return torch.equal(obs.cpu(), converted(fmt, want_frames))
        b = rows_to_bytes(fmt, obs)
        return torch.equal(converted(fmt, b), obs) and len(fd.differing(fd.digest_torch(b), want_digest)) == 0

    obs = env.reset(seed=seeds, options=opts)[0]
    assert same_frames(obs, first, first), "%s: reset frames differ from the oracle's" % what
    n_done = n_running = most = 0
    for t, (a, fr, dg, fdg, rew, done, gt) in enumerate(run):
        env.final_obs.fill_(SENTINEL[fmt])
        obs, r, d, _, info = env.step(a)
        d_host = d.cpu().numpy()
        assert np.array_equal(d_host, done.astype(bool)), "%s: dones differ at step %d" % (what, t)
        assert np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), "%s: rewards differ at step %d" % (what, t)
        assert same_frames(obs, fr, dg), "%s: frames differ from the oracle's at step %d" % (what, t)
        if gt is not None:
            assert np.array_equal(info["ground_truth"].cpu().numpy(), gt), "%s: ground truth differs at step %d" % (what, t)
        rows = info["final_observation"]
        if d_host.any():
            b = rows_to_bytes(fmt, rows[d])
            assert len(fd.differing(fd.digest_torch(b), fdg[d_host])) == 0, "%s: terminal frames differ from the oracle's at step %d" % (what, t)
            assert torch.equal(converted(fmt, b), rows[d]), "%s: a terminal row holds a value no byte maps to (step %d)" % (what, t)
        assert bool((rows[~d] == SENTINEL[fmt]).all()), "%s: a row of a running instance was written at step %d" % (what, t)
        n_done += int(d_host.sum())
        n_running += int((~d_host).sum())
        most = max(most, int(d_host.sum()))
    env.check_errors()
    return n_done, n_running, most, env


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in IDS for f in CHW])  # (id by id: oracle_run is shared)
def test_terminal_frames_against_the_oracle(env_id, fmt):
    n, steps = TERMINAL["n"], TERMINAL["steps"]
    n_done, n_running, _, env = lock_step_with_the_oracle(env_id, fmt, n, steps, short=True, frames=True)
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
    _, _, most, env = lock_step_with_the_oracle(env_id, fmt, n, steps, short=False, frames=False)
    assert most > ONE_ROUND, most  # otherwise the run did not reach the second round
    assert env.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("spot_fused_steps") == steps
    env.close()


@pytest.mark.parametrize("env_id,fmt", [(FINITE, "bf16_chw"), (FINITE, "f32_chw"), (FINITE, "u8_chw"), (ENDLESS, "bf16_chw")])
def test_the_batch_of_eight_regime(env_id, fmt):
    """Beyond 12,288 instances a service workgroup takes eight queue entries per round whatever the count (batch_min = 8); 12,355 is no
    multiple of 64.  Against a u8_xyc twin handle stepped with the same actions.  With terminal observations kept both ids defer at this size."""
    import memory_gym_amd
    import torch

    n, steps = 12288 + 67, 12
    xyc = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_xyc", final_observation=True)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=True)
    g = torch.Generator(device="cuda").manual_seed(4)
    o_x, o_c = xyc.reset(seed=21, options=SHORT[env_id])[0], env.reset(seed=21, options=SHORT[env_id])[0]
    assert torch.equal(o_c, converted(fmt, o_x))
    n_done = 0
    for t in range(steps):
        a = torch.randint(0, 3, (n, 2), device="cuda", generator=g, dtype=torch.int32)
        env.final_obs.fill_(SENTINEL[fmt])
        (o_x, r_x, d_x, _, i_x), (o_c, r_c, d_c, _, i_c) = xyc.step(a), env.step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c), "%s %s: rewards / dones differ after step %d" % (env_id, fmt, t)
        assert torch.equal(o_c, converted(fmt, o_x)), "%s %s: frames differ after step %d" % (env_id, fmt, t)
        f_x, f_c = i_x["final_observation"], i_c["final_observation"]
        assert torch.equal(f_c[d_c], converted(fmt, f_x[d_x])), "%s %s: terminal frames differ after step %d" % (env_id, fmt, t)
        assert bool((f_c[~d_c] == SENTINEL[fmt]).all()), "%s %s: a row of a running instance was written at step %d" % (env_id, fmt, t)
        n_done += int(d_c.sum())
    assert n_done >= n, n_done  # (max_steps = 9: every instance finished within the 12 steps)
    assert env.debug_counter("final_obs_generic_steps") == 0 and xyc.debug_counter("final_obs_generic_steps") == 0
    assert env.debug_counter("spot_fused_steps") == steps
    for e in (xyc, env):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("batch", [None, 3])
def test_plain_autoreset_fused_launch_forced(batch):
    """Lab library, MEMGYM_SPOT_FUSE=1: the fused launch without kept terminal observations, whatever fuse_resets() would choose for the size;
    once more with MEMGYM_SPOT_SVC_BATCH=3, a batch that divides neither 8 nor the counts.  tests/spot_chw_worker.py runs both ids in bf16_chw
    and u8_chw against the oracle in one process."""
    env = dict(os.environ, MEMGYM_HIP_LIB=LAB_LIB, MEMGYM_SPOT_FUSE="1")
    if batch:
        env["MEMGYM_SPOT_SVC_BATCH"] = str(batch)
    cases = ["%s:%s" % (e, f) for e in IDS for f in ("bf16_chw", "u8_chw")]
    # four runs of 40 steps of 96 instances next to ~10 s of imports and oracle; 300 s is far beyond any run that makes progress
    r = subprocess.run([sys.executable, os.path.join(HERE, "spot_chw_worker.py"), str(FORCED["n"]), str(FORCED["steps"])] + cases,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("ok:") == len(cases), r.stdout[-2000:] + r.stderr[-4000:]


def test_two_option_sets_keep_the_generic_path():
    """Per-instance option sets: the plain arrangement and mg_step's generic path for terminal observations, and the counters say so.
    (A guard: this holds before and after the fused launch learnt the image-order formats.)"""
    import memory_gym_amd
    import torch

    n, steps = 64, 12
    envs = [memory_gym_amd.make(FINITE, num_envs=n, device=0, obs_format=f, final_observation=True) for f in ("u8_xyc", "bf16_chw")]
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[n // 2:] = 1
    for e in envs:
        e.reset(seed=5, options=SHORT[FINITE])
        e.reset(options=dict(SHORT[FINITE], max_steps=5), mask=mask)  # the second half runs under a second option set
    g = torch.Generator(device="cuda").manual_seed(7)
    n_done = 0
    for t in range(steps):
        a = torch.randint(0, 3, (n, 2), device="cuda", generator=g, dtype=torch.int32)
        (o_x, r_x, d_x, _, i_x), (o_c, r_c, d_c, _, i_c) = envs[0].step(a), envs[1].step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c) and torch.equal(o_c, converted("bf16_chw", o_x)), "step %d" % t
        assert torch.equal(i_c["final_observation"][d_c], converted("bf16_chw", i_x["final_observation"][d_x])), "terminal frames, step %d" % t
        n_done += int(d_c.sum())
    assert n_done > 0
    for e in envs:
        assert e.debug_counter("final_obs_generic_steps") == steps
        assert e.debug_counter("spot_fused_steps") == 0
        e.check_errors()
        e.close()


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
    snap = env.state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe asks
        env.step(acts[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    before = env.debug_counter("spot_fused_steps")
    outs = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for a in acts:
            o, r, d, _, _ = env.step(a)
            outs.append((o.clone(), r.clone(), d.clone()))
    env.load_state_dict(snap)
    graph.replay()
    torch.cuda.synchronize()
    for k, ((o1, r1, d1), (o2, r2, d2)) in enumerate(zip(want, outs)):
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), "step %d of the replay differs" % k
    assert env.debug_counter("spot_fused_steps") == before  # captured steps are not the fused launch
    env.check_errors()
    twin.close()
    env.close()
