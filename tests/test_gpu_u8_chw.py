"""GPU (-m gpu): the uint8 image-order stream-out of the raster kernels (include/memgym.h MG_OBS_U8_CYX, obs_format="u8_chw").

The format is a fixed permutation of the frame the oracle referees: out[i][c][y][x] == xyc[i][x][y][c].  Checked against this
library's own uint8 frames (all ten ids, rewards / dones / render / vector observation as well), against the oracle directly, past
one frame per workgroup on the mortar family's one-launch step (mg_debug_counter "one_launch_steps" shows that launch ran), with
terminal observations kept, under a masked reset, through mg_render, under graph capture and on the single-instance path."""
import ctypes as C

import numpy as np
import pytest

from chw_referee import SHORT, clones, lock_step_with_a_twin, replay_captured, same_steps

pytestmark = pytest.mark.gpu

CASES = [("MortarMayhem-Grid-v0", 4), ("MortarMayhem-v0", 3), ("Endless-MortarMayhem-v0", 3), ("MysteryPath-v0", 3),
         ("Endless-MysteryPath-v0", 4), ("MysteryPath-Grid-v0", 4), ("SearingSpotlights-v0", 3),
         ("Endless-SearingSpotlights-v0", 3), ("MortarMayhemB-Grid-v0", 4), ("MortarMayhemB-v0", 3)]


def _actions(torch, g, env, n, n_act):
    return torch.randint(0, n_act, (n,) if env.action_dim == 1 else (n, 2), device="cuda", generator=g, dtype=torch.int32)


@pytest.mark.parametrize("env_id,n_act", CASES)
def test_u8_chw_is_the_permuted_u8_xyc(env_id, n_act):
    import torch

    n, steps = 96, 50

    def same_render(t, xyc, chw, g):
        assert torch.equal(chw.render(), xyc.render()), "%s: render() differs at step %d" % (env_id, t)

    _, xyc, chw = lock_step_with_a_twin(env_id, "u8_chw", n, steps + 1, final=False, seed=11, action_seed=3, between=same_render)
    assert chw.obs.shape == (n, 3, 84, 84) and chw.obs.dtype == torch.uint8
    assert xyc.action_space.n == n_act if xyc.action_dim == 1 else list(xyc.action_space.nvec) == [n_act, n_act]
    if env_id.startswith("MortarMayhemB"):
        assert xyc.vector_obs is not None  # (observations are the reference's Dict: the twin loop compared the vector observation too)
    for e in (xyc, chw):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id,n_act", [("MortarMayhem-Grid-v0", 4), ("MysteryPath-v0", 3), ("Endless-MysteryPath-v0", 4),
                                          ("SearingSpotlights-v0", 3), ("Endless-SearingSpotlights-v0", 3)])
def test_u8_chw_matches_the_oracle(env_id, n_act):
    """Against the ORACLE's frames, not this library's own uint8 output: obs == oracle [x][y][c] transposed to [c][y][x], at every step."""
    import memory_gym_amd
    import oracle_lib

    n, steps = 64, 40
    ref = oracle_lib.OracleBatch(env_id, n)
    seeds = np.arange(n, dtype=np.int64) + 77
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    obs = env.reset(seed=seeds)[0]
    want = ref.reset(seeds)
    prng = np.random.Generator(np.random.PCG64(5))
    disc = env.action_dim == 1
    for t in range(steps + 1):
        assert np.array_equal(obs.cpu().numpy(), want.transpose(0, 3, 2, 1)), "%s: frames differ from the oracle's at step %d" % (env_id, t)
        a = (prng.integers(0, n_act, n) if disc else prng.integers(0, n_act, (n, 2))).astype(np.int32)
        obs, r, d, _, _ = env.step(a)
        want, r2, d2 = ref.step(a, autoreset=True)
        assert np.array_equal(d.cpu().numpy(), d2.astype(bool)) and np.array_equal(r.cpu().numpy(), r2.astype(np.float32))
    env.check_errors()
    env.close()
    ref.close()


@pytest.mark.parametrize("env_id,n_act", [("MortarMayhem-Grid-v0", 4), ("Endless-MortarMayhem-v0", 3)])
def test_more_than_one_frame_per_workgroup(env_id, n_act):
    """Just above the raster grid (14,336 persistent workgroups, mg_raster_v1.hpp RASTER_GRID) and no multiple of 64: 67 workgroups
    draw two frames, the last 64-instance claim slot of the one-launch step holds 3 instances."""
    n, steps = 14336 + 67, 12
    assert n % 64 != 0
    _, xyc, chw = lock_step_with_a_twin(env_id, "u8_chw", n, steps, final=False)
    assert chw.debug_counter("one_launch_steps") == steps
    assert xyc.debug_counter("one_launch_steps") == steps
    for e in (xyc, chw):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id,n_act", [("MortarMayhem-Grid-v0", 4), ("Endless-MortarMayhem-v0", 3), ("MysteryPath-Grid-v0", 4),
                                          ("SearingSpotlights-v0", 3)])
def test_terminal_observations(env_id, n_act):
    """final_observation=True: rows of finished instances hold the permuted terminal frame, every other row is left alone; on the mortar
    family every such step is ONE launch (the FINAL form of the one-launch step)."""
    n, steps = 48, 60
    finished, xyc, chw = lock_step_with_a_twin(env_id, "u8_chw", n, steps, SHORT[env_id], seed=31, action_seed=6)
    n_done = sum(finished)
    n_running = n * steps - n_done
    assert n_done > n and n_running > n, (n_done, n_running)  # both kinds of row were seen, many times
    if "MortarMayhem" in env_id:
        assert chw.debug_counter("one_launch_steps") == steps
    else:
        with pytest.raises(RuntimeError):
            chw.debug_counter("one_launch_steps")
    for e in (xyc, chw):
        e.check_errors()
        e.close()


def test_masked_reset_leaves_other_frames():
    """mg_reset with a mask writes only the reset instances' frames."""
    import memory_gym_amd
    import torch

    env = memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=8, device=0, obs_format="u8_chw")
    twin = memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=8, device=0, obs_format="u8_xyc")
    env.reset(seed=0)
    twin.reset(seed=0)
    env.obs.fill_(0x5A)
    mask = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.uint8, device="cuda")
    obs, _ = env.reset(seed=5, mask=mask)
    want, _ = twin.reset(seed=5, mask=mask)
    assert bool((obs[[1, 2, 4, 5, 6, 7]] == 0x5A).all())
    assert torch.equal(obs[[0, 3]], want[[0, 3]].permute(0, 3, 2, 1))
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id,n_act", [("MortarMayhem-Grid-v0", 4), ("Endless-SearingSpotlights-v0", 3), ("Endless-MysteryPath-v0", 4)])
def test_render_into_a_second_buffer(env_id, n_act):
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    n = 80
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    g = torch.Generator(device="cuda").manual_seed(8)
    env.reset(seed=41)
    for t in range(6):
        obs = env.step(_actions(torch, g, env, n, n_act))[0]
        again = torch.full_like(obs, 0x5A)
        _native.check(_native.LIB.mg_render(env._h, again.data_ptr(), env._stream()), "mg_render")
        assert torch.equal(again, obs), "%s: mg_render differs after step %d" % (env_id, t)
    env.check_errors()
    env.close()


def test_graph_replay_equals_eager():
    """Under capture the mortar family steps in its two-launch form: the plain raster launch with the new stream-out."""
    import memory_gym_amd
    import torch

    env_id, n, K = "MortarMayhem-Grid-v0", 512, 8
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = [torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32) for _ in range(K)]
    eager = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    eager.reset(seed=9)
    want = [clones(eager.step(a)) for a in acts]
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    env.reset(seed=9)
    before = []
    same_steps(want, replay_captured(env, acts, clones, lambda: before.append(env.debug_counter("one_launch_steps"))))
    assert env.debug_counter("one_launch_steps") == before[0]  # captured steps are not the one-launch kernel
    env.check_errors()
    eager.close()
    env.close()


@pytest.mark.parametrize("env_id,n_act", [("MortarMayhem-Grid-v0", 4), ("MysteryPath-Grid-v0", 4)])
def test_single_instance_path(env_id, n_act):
    """mg_single_reset / mg_single_step with the format set on the handle: the mapped host frame is the permuted one."""
    import memory_gym_amd
    from memory_gym_amd import _native

    one = memory_gym_amd.make(env_id)
    twin = memory_gym_amd.make(env_id)
    _native.check(_native.LIB.mg_set_obs_format(one._h, 4), "mg_set_obs_format")
    assert _native.LIB.mg_obs_bytes(one._h) == 84 * 84 * 3
    chw = lambda e: np.ctypeslib.as_array(C.cast(e._io.obs, C.POINTER(C.c_uint8)), shape=(3, 84, 84))  # noqa: E731
    one.reset(seed=3)
    want, _ = twin.reset(seed=3)
    assert np.array_equal(chw(one), want.transpose(2, 1, 0))
    prng = np.random.Generator(np.random.PCG64(9))
    for t in range(12):
        a = int(prng.integers(0, n_act))
        _, r1, d1, _, _ = one.step(a)
        want, r2, d2, _, _ = twin.step(a)
        assert np.array_equal(chw(one), want.transpose(2, 1, 0)), "%s: single step %d" % (env_id, t)
        assert r1 == r2 and d1 == d2
        if d2:
            one.reset()
            twin.reset()
    one.close()
    twin.close()
