"""GPU (-m gpu): the uint8 image-order stream-out of the raster kernels (include/memgym.h MG_OBS_U8_CYX, obs_format="u8_chw").

The format is a fixed permutation of the frame the oracle referees: out[i][c][y][x] == xyc[i][x][y][c].  Checked against this
library's own uint8 frames (all ten ids, rewards / dones / render / vector observation as well), against the oracle directly, past
one frame per workgroup on the mortar family's one-launch step (mg_debug_counter "one_launch_steps" shows that launch ran), with
terminal observations kept, under a masked reset, through mg_render, under graph capture and on the single-instance path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [("MortarMayhem-Grid-v0", 4), ("MortarMayhem-v0", 3), ("Endless-MortarMayhem-v0", 3), ("MysteryPath-v0", 3),
         ("Endless-MysteryPath-v0", 4), ("MysteryPath-Grid-v0", 4), ("SearingSpotlights-v0", 3),
         ("Endless-SearingSpotlights-v0", 3), ("MortarMayhemB-Grid-v0", 4), ("MortarMayhemB-v0", 3)]

# reset options under which episodes end within a few steps (terminal observations, resets inside the run)
SHORT = {"MortarMayhem-Grid-v0": {"command_count": [2], "command_show_duration": [1], "command_show_delay": [0], "explosion_delay": [2],
                                  "explosion_duration": [1]},
         "Endless-MortarMayhem-v0": {"command_show_duration": [1], "command_show_delay": [0], "explosion_delay": [2], "explosion_duration": [1],
                                     "max_steps": 14},
         "MysteryPath-Grid-v0": {"max_steps": 7},
         "SearingSpotlights-v0": {"max_steps": 9, "agent_health": 1}}


def _actions(torch, g, env, n, n_act):
    return torch.randint(0, n_act, (n,) if env.action_dim == 1 else (n, 2), device="cuda", generator=g, dtype=torch.int32)


def _vis(o):
    return o["visual_observation"] if isinstance(o, dict) else o


@pytest.mark.parametrize("env_id,n_act", CASES)
def test_u8_chw_is_the_permuted_u8_xyc(env_id, n_act):
    import memory_gym_amd
    import torch

    n, steps = 96, 50
    xyc = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_xyc")
    chw = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    assert chw.obs.shape == (n, 3, 84, 84) and chw.obs.dtype == torch.uint8
    g = torch.Generator(device="cuda").manual_seed(3)
    o_x, o_c = xyc.reset(seed=11)[0], chw.reset(seed=11)[0]
    for t in range(steps + 1):
        assert torch.equal(_vis(o_c), _vis(o_x).permute(0, 3, 2, 1)), "%s: frames differ at step %d" % (env_id, t)
        assert torch.equal(chw.render(), xyc.render()), "%s: render() differs at step %d" % (env_id, t)
        if isinstance(o_x, dict):
            assert torch.equal(o_c["vector_observation"], o_x["vector_observation"]), "%s: vector observation differs at step %d" % (env_id, t)
        a = _actions(torch, g, xyc, n, n_act)
        (o_x, r_x, d_x, _, _), (o_c, r_c, d_c, _, _) = xyc.step(a), chw.step(a)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c), "%s: rewards / dones differ at step %d" % (env_id, t)
    if env_id.startswith("MortarMayhemB"):
        assert isinstance(o_x, dict)
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
    import memory_gym_amd
    import torch

    n, steps = 14336 + 67, 12
    assert n % 64 != 0
    xyc = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_xyc")
    chw = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
    g = torch.Generator(device="cuda").manual_seed(4)
    o_x, o_c = xyc.reset(seed=21)[0], chw.reset(seed=21)[0]
    assert torch.equal(o_c, o_x.permute(0, 3, 2, 1))
    for t in range(steps):
        a = _actions(torch, g, xyc, n, n_act)
        (o_x, r_x, d_x, _, _), (o_c, r_c, d_c, _, _) = xyc.step(a), chw.step(a)
        assert torch.equal(o_c, o_x.permute(0, 3, 2, 1)), "%s: frames differ after step %d" % (env_id, t)
        assert torch.equal(r_x, r_c) and torch.equal(d_x, d_c)
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
    import memory_gym_amd
    import torch

    n, steps, sentinel = 48, 60, 0x5A
    xyc = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_xyc", final_observation=True)
    chw = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw", final_observation=True)
    g = torch.Generator(device="cuda").manual_seed(6)
    xyc.reset(seed=31, options=SHORT[env_id])
    chw.reset(seed=31, options=SHORT[env_id])
    n_done = n_running = 0
    for t in range(steps):
        a = _actions(torch, g, xyc, n, n_act)
        xyc.final_obs.fill_(sentinel)
        chw.final_obs.fill_(sentinel)
        (o_x, _, d_x, _, i_x), (o_c, _, d_c, _, i_c) = xyc.step(a), chw.step(a)
        assert torch.equal(d_x, d_c) and torch.equal(o_c, o_x.permute(0, 3, 2, 1)), "%s: step %d" % (env_id, t)
        f_x, f_c = i_x["final_observation"], i_c["final_observation"]
        assert torch.equal(f_c[d_c], f_x[d_x].permute(0, 3, 2, 1)), "%s: terminal frames differ at step %d" % (env_id, t)
        assert bool((f_c[~d_c] == sentinel).all()), "%s: a row of a running instance was written at step %d" % (env_id, t)
        n_done += int(d_c.sum())
        n_running += int((~d_c).sum())
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
    want = []
    for a in acts:
        o, r, d, _, _ = eager.step(a)
        want.append((o.clone(), r.clone(), d.clone()))
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, obs_format="u8_chw")
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
