"""GPU (-m gpu): terminal observations kept inside the step's own launches in the image-order formats (bf16_chw, f16_chw, f32_chw, u8_chw) on the
mortar family (mortar_step_raster_kernel<false, FINAL, FMT>, csrc/mg_mortar_one_launch.hpp) and the finite Mystery Path ids
(mystery_raster_paths_kernel<FMT, true>, csrc/mg_mystery_finite.hpp).

Floats are compared EXACTLY: a float observation is the oracle's uint8 [x][y][c] frame / np.float32(255) transposed to [c][y][x], the 16-bit
formats that quotient rounded -- a table of 256 values (tests/test_float_bytes.py), no tolerance.  Which path ran is asserted from the host-side
counters of mg_debug_counter: "final_obs_generic_steps" (mg_step's generic terminal-observation branch; must stay 0) and, on the mortar ids,
"one_launch_steps"."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_float_bytes import float_rows_to_bytes, unit_values
from test_gpu_u8_chw import SHORT as SHORT_U8_CHW

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAB_LIB = os.path.join(ROOT, "endless-memory-gym_amd", "lib", "lab", "libmemgym_hip_lab.so")

# reset options under which episodes end within a few steps (MortarMayhem-v0: the grid variant's; MysteryPath-v0: max_steps, like the grid variant)
SHORT = dict(SHORT_U8_CHW)
SHORT["MortarMayhem-v0"] = SHORT_U8_CHW["MortarMayhem-Grid-v0"]
SHORT["MysteryPath-v0"] = {"max_steps": 7}

MORTAR = ("MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0")
MYSTERY = ("MysteryPath-Grid-v0", "MysteryPath-v0")
FLOATS = ("bf16_chw", "f16_chw", "f32_chw")
SENTINEL = {"u8_chw": 0x5A, "bf16_chw": -3.0, "f16_chw": -3.0, "f32_chw": -3.0}  # (no observation holds either value)


def converted(fmt, frames):
    """uint8 [k][x][y][c] (numpy array or tensor, any device) -> what the format holds for these frames, a tensor [k][3][y][x] on the same
    device: the table's value for every byte (in chunks: the index tensor is 8 bytes per element)"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    t = t.permute(0, 3, 2, 1)
    if fmt == "u8_chw":
        return t.contiguous()
    lut = unit_values(fmt).to(t.device)
    out = torch.empty(t.shape, dtype=lut.dtype, device=t.device)
    for i in range(0, t.shape[0], 2048):
        out[i:i + 2048] = lut[t[i:i + 2048].long()]
    return out


def rows_to_bytes(fmt, rows):
    """rows in format `fmt` [k][3][y][x] -> uint8 [k][x][y][c], what tests/frame_digest.py digests"""
    return rows.permute(0, 3, 2, 1).contiguous() if fmt == "u8_chw" else float_rows_to_bytes(rows)


def _actions_np(prng, n, disc):
    return (prng.integers(0, 4, n) if disc else prng.integers(0, 3, (n, 2))).astype(np.int32)


@functools.lru_cache(maxsize=1)
def oracle_run(env_id, n, steps):
    """The oracle's run of `steps` auto-reset steps under SHORT[env_id], computed once per (id, n, steps) and shared by the formats: the reset
    frames and, per step, (actions, frames, final_digest, reward, done).  Two batches in lock step: one returns the frames, one the digests."""
    import oracle_lib

    refs = [oracle_lib.OracleBatch(env_id, n, options=SHORT[env_id]) for _ in range(2)]
    seeds = np.arange(n, dtype=np.int64) + 31
    first = refs[0].reset(seeds)
    refs[1].reset_digest(seeds)
    prng = np.random.Generator(np.random.PCG64(6))
    out = []
    for _ in range(steps):
        a = _actions_np(prng, n, refs[0].discrete)
        frames, rew, done = refs[0].step(a, autoreset=True)
        _, fdg, rew2, done2 = refs[1].step_digest(a, autoreset=True)
        assert np.array_equal(rew, rew2) and np.array_equal(done, done2)
        out.append((a, frames, fdg, rew, done))
    for r in refs:
        r.close()
    return seeds, first, out


def lock_step_with_the_oracle(env_id, fmt, n, steps, final):
    """-> (finished rows seen, running rows seen, the handle -- still open, for the caller's counter asserts)"""
    import frame_digest as fd
    import memory_gym_amd
    import torch

    seeds, first, run = oracle_run(env_id, n, steps)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=final)
    obs = env.reset(seed=seeds, options=SHORT[env_id])[0]
    assert torch.equal(obs.cpu(), converted(fmt, first)), "%s %s: reset frames differ from the oracle's" % (env_id, fmt)
    n_done = n_running = 0
    for t, (a, frames, fdg, rew, done) in enumerate(run):
        if final:
            env.final_obs.fill_(SENTINEL[fmt])
        obs, r, d, _, info = env.step(a)
        d_host = d.cpu().numpy()
        assert np.array_equal(d_host, done.astype(bool)), "%s %s: dones differ at step %d" % (env_id, fmt, t)
        assert np.array_equal(r.cpu().numpy(), rew.astype(np.float32)), "%s %s: rewards differ at step %d" % (env_id, fmt, t)
        assert torch.equal(obs.cpu(), converted(fmt, frames)), "%s %s: frames differ from the oracle's at step %d" % (env_id, fmt, t)
        if final:
            rows = info["final_observation"]
            if d_host.any():
                got = fd.digest_torch(rows_to_bytes(fmt, rows[d]))
                assert len(fd.differing(got, fdg[d_host])) == 0, "%s %s: terminal frames differ from the oracle's at step %d" % (env_id, fmt, t)
                assert torch.equal(converted(fmt, rows_to_bytes(fmt, rows[d])), rows[d]), "%s %s: a terminal row holds a value no byte maps to (step %d)" % (env_id, fmt, t)
            assert bool((rows[~d] == SENTINEL[fmt]).all()), "%s %s: a row of a running instance was written at step %d" % (env_id, fmt, t)
        n_done += int(d_host.sum())
        n_running += int((~d_host).sum())
    env.check_errors()
    return n_done, n_running, env


FINAL_CASES = [(e, f) for e in MORTAR for f in FLOATS] + [(e, f) for e in MYSTERY for f in FLOATS + ("u8_chw",)]  # (id by id: oracle_run is shared)


@pytest.mark.parametrize("env_id,fmt", FINAL_CASES)
def test_terminal_frames_against_the_oracle(env_id, fmt):
    n, steps = 48, 60
    n_done, n_running, env = lock_step_with_the_oracle(env_id, fmt, n, steps, final=True)
    assert n_done > n and n_running > n, (n_done, n_running)  # both kinds of row were seen, many times
    assert env.debug_counter("final_obs_generic_steps") == 0  # the step's own launches kept the terminal observations
    if env_id in MORTAR:
        assert env.debug_counter("one_launch_steps") == steps
    env.close()


@pytest.mark.parametrize("env_id,fmt", [(e, f) for e in MORTAR for f in FLOATS])
def test_plain_autoreset_steps_against_the_oracle(env_id, fmt):
    n, steps = 96, 40
    n_done, _, env = lock_step_with_the_oracle(env_id, fmt, n, steps, final=False)
    assert n_done > n
    assert env.debug_counter("one_launch_steps") == steps  # every float format ships in the one-launch form (profiles/chw_final.md)
    assert env.debug_counter("final_obs_generic_steps") == 0
    env.close()


@pytest.mark.parametrize("env_id,fmt", [("MortarMayhem-Grid-v0", "bf16_chw"), ("MortarMayhem-Grid-v0", "f32_chw"), ("MysteryPath-Grid-v0", "bf16_chw")])
def test_more_than_one_frame_per_workgroup(env_id, fmt):
    """Just above the raster grid (14,336 persistent workgroups, mg_raster_v1.hpp RASTER_GRID) and no multiple of 64: 67 workgroups draw two
    frames (and their terminal frames), the last 64-instance claim slot of the one-launch step holds 3 instances.  Against a u8_xyc twin handle."""
    import memory_gym_amd
    import torch

    n, steps = 14336 + 67, 12
    assert n % 64 != 0
    xyc = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_xyc", final_observation=True)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=fmt, final_observation=True)
    g = torch.Generator(device="cuda").manual_seed(4)
    o_x, o_c = xyc.reset(seed=21, options=SHORT[env_id])[0], env.reset(seed=21, options=SHORT[env_id])[0]
    assert torch.equal(o_c, converted(fmt, o_x))
    n_done = 0
    for t in range(steps):
        a = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32)
        env.final_obs.fill_(SENTINEL[fmt])
        (o_x, r_x, d_x, _, i_x), (o_c, r_c, d_c, _, i_c) = xyc.step(a), env.step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c), "%s %s: rewards / dones differ after step %d" % (env_id, fmt, t)
        assert torch.equal(o_c, converted(fmt, o_x)), "%s %s: frames differ after step %d" % (env_id, fmt, t)
        f_x, f_c = i_x["final_observation"], i_c["final_observation"]
        assert torch.equal(f_c[d_c], converted(fmt, f_x[d_x])), "%s %s: terminal frames differ after step %d" % (env_id, fmt, t)
        assert bool((f_c[~d_c] == SENTINEL[fmt]).all()), "%s %s: a row of a running instance was written at step %d" % (env_id, fmt, t)
        n_done += int(d_c.sum())
    assert n_done >= n, n_done  # (episodes under SHORT last 7 steps at the most: every instance finished within the 12, so every workgroup drew terminal frames)
    assert env.debug_counter("final_obs_generic_steps") == 0 and xyc.debug_counter("final_obs_generic_steps") == 0
    if env_id in MORTAR:
        assert env.debug_counter("one_launch_steps") == steps
    for e in (xyc, env):
        e.check_errors()
        e.close()


def test_rescue_path_in_a_float_kernel():
    """The step workgroups at the END of the grid (lab build, MEMGYM_LAB_LOGIC_LAST=1; tests/test_gpu_one_launch.py): frame waves of the bf16
    FINAL kernel step the slots themselves.  tests/chw_final_worker.py compares every frame and every terminal frame with the oracle."""
    env = dict(os.environ, MEMGYM_HIP_LIB=LAB_LIB, MEMGYM_LAB_LOGIC_LAST="1")
    # 30 steps of 4,096 instances: three rounds of frame workgroups per step, each waiting RESCUE_AFTER_TICKS (200 us) at most once, next
    # to ~10 s of imports, oracle and digests; 300 s is far beyond any run that makes progress
    r = subprocess.run([sys.executable, os.path.join(HERE, "chw_final_worker.py"), "MortarMayhem-Grid-v0", "4096", "30", "bf16_chw"],
                       env=env, capture_output=True, text=True, timeout=300)
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
    want = []
    for a in acts:
        o, r, d, _, _ = eager.step(a)
        want.append((o.clone(), r.clone(), d.clone()))
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="bf16_chw")
    env.reset(seed=9)
    snap = env.state_dict()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe asks
        env.step(acts[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    before = env.debug_counter("one_launch_steps")
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
    assert env.debug_counter("one_launch_steps") == before  # captured steps are not the one-launch kernel
    env.check_errors()
    eager.close()
    env.close()


def test_two_option_sets_keep_the_generic_path():
    """Per-instance option sets: mg_step keeps terminal observations on its generic path, and the counter says so."""
    import memory_gym_amd
    import torch

    env_id, n, steps = "MortarMayhem-Grid-v0", 64, 10
    envs = [memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format=f, final_observation=True) for f in ("u8_xyc", "bf16_chw")]
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[n // 2:] = 1
    for e in envs:
        e.reset(seed=5, options=SHORT[env_id])
        e.reset(options=dict(SHORT[env_id], command_count=[3]), mask=mask)  # the second half runs under a second option set
    g = torch.Generator(device="cuda").manual_seed(7)
    n_done = 0
    for t in range(steps):
        a = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32)
        (o_x, r_x, d_x, _, i_x), (o_c, r_c, d_c, _, i_c) = envs[0].step(a), envs[1].step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c) and torch.equal(o_c, converted("bf16_chw", o_x)), "step %d" % t
        assert torch.equal(i_c["final_observation"][d_c], converted("bf16_chw", i_x["final_observation"][d_x])), "terminal frames, step %d" % t
        n_done += int(d_c.sum())
    assert n_done > 0
    for e in envs:
        assert e.debug_counter("final_obs_generic_steps") == steps
        assert e.debug_counter("one_launch_steps") == 0
        e.check_errors()
        e.close()
