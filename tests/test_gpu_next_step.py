"""GPU (-m gpu): next-step auto-reset -- mg_step_next, make(..., autoreset_mode="next_step"), GymnasiumVectorEnv(autoreset_mode="next_step") -- all ten env ids.

DEFINITION under test (include/memgym.h): an instance whose restart flag is set is reset instead of stepped -- its random stream continues, it keeps
its option set, reward 0, done 0 -- every other instance steps without auto-reset, and the frame of the step that ends an episode is the terminal frame.
By definition the call is the pair  step(a, mask=~restart) of a handle without auto-reset, then reset(mask=restart).  Referees: the CPU oracle stepped one
instance at a time (1, 4), a twin handle that runs the pair with public calls (2, 6, 7), a second handle of the same kind (3, 5, 7, 9).  Inputs and the
short-episode options: tests/masked_step_inputs.py.  The episode counts in the docstrings were measured with the oracle ALONE on the CPU with exactly these
inputs (tests/next_step_inputs.py run as a program prints them); every test asserts its condition so that a run in which nothing ever ends cannot pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

import masked_step_inputs as mi
import next_step_inputs as ni

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_IDS = mi.MORTAR + mi.SPOT  # the ids whose family has a NEXT form of its step kernel; the Mystery Path ids run the pair itself


def vis(o):
    return o["visual_observation"] if isinstance(o, dict) else o


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def make(env_id, n, options=None, **kw):
    """a handle after the seeded reset every test here starts from (seeds arange(n) + 1000, the id's short-episode options unless given)"""
    import memory_gym_amd

    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    env.reset(seed=mi.seeds(n), options=mi.SHORT[env_id] if options is None else options)
    return env


def same_frames(got, want, what):
    g = vis(got).cpu().numpy()
    if not np.array_equal(g, want):
        bad = np.nonzero((g != want).reshape(len(want), -1).any(1))[0]
        raise AssertionError("%s: frames of %d instances differ, first %s" % (what, len(bad), bad[:8]))


def check_against_oracle(env, t, out, r2, d2, i2, what):
    _, reward, done, _, info = out
    assert np.array_equal(done.cpu().numpy(), d2), "%s: done differs at step %d" % (what, t)
    assert np.array_equal(env.reward64.cpu().numpy(), r2), "%s: reward64 differs at step %d" % (what, t)
    assert np.array_equal(reward.cpu().numpy(), r2.astype(np.float32)), "%s: reward differs at step %d" % (what, t)
    assert np.array_equal(info["done_mask"].cpu().numpy(), d2)
    assert "final_observation" not in info and "final_frames" not in info
    if d2.any():
        assert np.array_equal(info["reward"].cpu().numpy()[d2], i2["reward"][d2]), "%s: info['reward'] differs at step %d" % (what, t)
        assert np.array_equal(info["length"].cpu().numpy()[d2], i2["length"][d2].astype(np.int32)), "%s: info['length'] differs at step %d" % (what, t)
        for nm in env.info_names:
            assert np.array_equal(info[nm].cpu().numpy()[d2], i2[nm][d2].astype(np.float32)), "%s: info[%r] differs at step %d" % (what, nm, t)


def twin_pair(twin, a, restart):
    """the definition with public calls on a handle without auto-reset -> what step() returned; its obs / gt rows are complete after the reset"""
    out = twin.step(a, mask=~restart)
    twin.reset(mask=restart)
    return out


def same_handles(env, twin, out, out2, t, what):
    """everything a call leaves, handle against handle"""
    import torch

    (o, r, d, _, i), (o2, r2, d2, _, i2) = out, out2
    assert torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(env.reward64, twin.reward64), "%s: reward / done at step %d" % (what, t)
    assert torch.equal(vis(env.obs), vis(twin.obs)), "%s: obs at step %d" % (what, t)
    if env.gt_dim:
        assert torch.equal(env.gt, twin.gt), "%s: ground truth at step %d" % (what, t)
    if env.vector_obs is not None:
        assert torch.equal(env.vector_obs, twin.vector_obs), "%s: vector observation at step %d" % (what, t)
    for nm in ("reward", "length") + tuple(env.info_names):
        assert torch.equal(i[nm], i2[nm]), "%s: info[%r] at step %d" % (what, nm, t)
    assert np.array_equal(env.state_dict()["blob"], twin.state_dict()["blob"]), "%s: state after step %d" % (what, t)


# ---- 1. against the oracle

@pytest.mark.parametrize("env_id", mi.ALL_IDS)
def test_next_step_rollout_equals_the_oracle(env_id):
    """n = 67 (four full 16-instance spotlight workgroups and three instances; one mortar wave and three lanes), 40 steps of step() in next_step mode:
    the oracle's envs[i].reset(None) where the previous done is set, else envs[i].step(a[i]).  After every step all 67 frames, reward64, done and the
    episode record where done; at the end the RNG words of instances 0 and 66.  Oracle alone (ni.EPISODES): 464 / 322 / 361 / 561 / 361 episodes end
    on the mortar ids, 201 on each Mystery Path and spotlight id -- at least 67 are asserted."""
    n, T = ni.N, ni.T
    env = make(env_id, n, autoreset_mode="next_step")
    assert env.autoreset_mode == "next_step"
    ref = ni.NextOracle(env_id, n, env.info_names)
    act = ni.rollout_actions(env.action_dim == 1, T, n)
    same_frames(env.obs, ref.frames(), env_id + ": reset frames")
    prev = np.zeros(n, bool)
    for t in range(T):
        out = env.step(act[t])
        r2, d2, i2 = ref.step(act[t], prev)
        check_against_oracle(env, t, out, r2, d2, i2, env_id)
        same_frames(out[0], ref.frames(), "%s: step %d" % (env_id, t))
        prev = d2
    for i in (0, n - 1):
        assert np.array_equal(env.rng_words(i), ref.rng_words(i)), "%s: RNG words of instance %d" % (env_id, i)
    env.check_errors()
    print("%s: %d episodes" % (env_id, ref.episodes.sum()))
    assert ref.episodes.sum() == ni.EPISODES[env_id] and ref.episodes.sum() >= n, ref.episodes.sum()
    assert env.debug_counter("next_steps") == T
    assert env.debug_counter("next_fused_steps") == (T if env_id in FUSED_IDS else 0)
    env.close()
    ref.close()


# ---- 2. against the definition, caller-chosen flags

@pytest.mark.parametrize("env_id,n", [(e, 67) for e in mi.ALL_IDS] + [("MortarMayhem-v0", 1), ("MortarMayhem-v0", 257),
                                                                       ("Endless-SearingSpotlights-v0", 1), ("Endless-SearingSpotlights-v0", 17)])
def test_next_step_equals_the_pair_of_its_definition(env_id, n):
    """42 calls with caller-chosen flags, written into the handle's pending flags before each call -- all clear, all set, ten Bernoulli(1/2) rows, sixteen
    rows of block_masks (whole waves and whole 16-lane groups beside partial ones), fourteen rows all clear -- each OR-ed with the previous done, so that
    no instance is stepped past its end.  The twin is an autoreset_mode="disabled" handle that runs step(a, mask=~restart), reset(mask=restart).  After
    every call: obs, reward, done, reward64, ground truth, the vector observation (MortarMayhemB ids), every info row and the checkpoint blob.
    In the last fourteen rows every instance of a Mystery Path or spotlight id reaches its max_steps = 12 unless it ended earlier: n episodes end."""
    import torch

    T = 42
    env, twin = make(env_id, n, autoreset_mode="next_step"), make(env_id, n, autoreset_mode="disabled")
    assert twin.autoreset is False
    rng = np.random.default_rng(5)
    flags = np.concatenate([np.zeros((1, n), bool), np.ones((1, n), bool), rng.random((10, n)) < 0.5, mi.block_masks(16, n), np.zeros((14, n), bool)])
    act = mi.actions(rng, env.action_dim == 1, T, n)
    prev = torch.zeros(n, dtype=torch.bool, device="cuda")
    finished = restarted = 0
    for t in range(T):
        restart = dev(flags[t]) | prev
        env.done_u8.copy_(restart.to(torch.uint8))
        a = dev(act[t])
        out, out2 = env.step(a), twin_pair(twin, a, restart)
        same_handles(env, twin, out, out2, t, "%s x%d" % (env_id, n))
        assert not bool(out[2][restart].any()) and not bool(out[1][restart].any()), "a restarted instance reports reward 0 and done 0"
        prev = out[2].clone()
        finished += int(prev.sum())
        restarted += int(restart.sum())
    assert restarted >= 8 * n, restarted
    assert finished >= (n if env_id in mi.MYSTERY + mi.SPOT else (1 if n >= 17 else 0)), finished
    assert env.debug_counter("next_steps") == T and env.debug_counter("next_fused_steps") == (T if env_id in FUSED_IDS else 0)
    for e in (env, twin):
        e.check_errors()
        e.close()


# ---- 3. aliasing

@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY)
def test_restart_flags_may_be_the_done_buffer(env_id):
    """mg_step_next through the binding, 30 calls, n = 67: handle A gets restart_dev == done_dev (one tensor), handle B the same flags in a tensor of
    their own.  Everything the calls leave is equal, and episodes end (so the flags are not all clear)."""
    import torch
    from memory_gym_amd import _native

    n, T = 67, 30
    A, B = make(env_id, n), make(env_id, n)
    act = dev(ni.rollout_actions(A.action_dim == 1, T, n))
    flags_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
    finished = 0
    for t in range(T):
        flags_b.copy_(B.done_u8)
        for e, restart in ((A, A.done_u8), (B, flags_b)):
            rc = _native.LIB.mg_step_next(e._h, act[t].data_ptr(), restart.data_ptr(), e.obs.data_ptr(), e._p_reward, e._p_done, e._p_gt, e._p_info, e._raw_stream())
            assert rc == 0, _native.last_error()
        assert torch.equal(A.done_u8, B.done_u8) and torch.equal(A.reward, B.reward) and torch.equal(A.reward64, B.reward64), "step %d" % t
        assert torch.equal(vis(A.obs), vis(B.obs)), "%s: obs at step %d" % (env_id, t)
        assert np.array_equal(A.state_dict()["blob"], B.state_dict()["blob"]), "%s: state after step %d" % (env_id, t)
        finished += int(A.done_u8.sum())
    assert finished >= n, finished
    for e in (A, B):
        e.check_errors()
        e.close()


# ---- 4. two option sets in one handle (the PS forms)

@pytest.mark.parametrize("env_id", ["SearingSpotlights-v0", "MortarMayhem-Grid-v0"])
def test_next_step_with_two_option_sets(env_id):
    """n = 64, the halves under two option sets (ni.TWO_SETS; the handle's per-set kernels), 40 steps in next_step mode: each half against its own oracle
    batch.  Oracle alone (ni.TWO_SET_EPISODES): 96 / 128 episodes end in the halves of SearingSpotlights-v0, 218 / 173 in those of MortarMayhem-Grid-v0."""
    import memory_gym_amd
    import oracle_lib
    import torch

    n, T = 64, ni.T
    half = n // 2
    opt_a, opt_b = ni.TWO_SETS[env_id]
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="next_step")
    refs = ni.two_set_oracles(env_id, n, env.info_names)
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds)  # (SearingSpotlights: every instance gets an exit first -- use_exit = False keeps drawing the earlier one)
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    act = ni.rollout_actions(env.action_dim == 1, T, n)
    prev = np.zeros(n, bool)
    for t in range(T):
        obs, _, done, _, _ = env.step(act[t])
        got_d, got_r, got_o = done.cpu().numpy(), env.reward64.cpu().numpy(), vis(obs).cpu().numpy()
        for k, (ref, sl) in enumerate(zip(refs, (slice(0, half), slice(half, n)))):
            r2, d2, _ = ref.step(act[t][sl], prev[sl])
            assert np.array_equal(got_d[sl], d2) and np.array_equal(got_r[sl], r2), "half %d, step %d" % (k, t)
            assert np.array_equal(got_o[sl], ref.frames()), "%s: frames of half %d at step %d" % (env_id, k, t)
        prev = got_d
    assert [int(r.episodes.sum()) for r in refs] == list(ni.TWO_SET_EPISODES[env_id])
    assert env.debug_counter("next_fused_steps") == T
    env.check_errors()
    env.close()
    for r in refs:
        r.close()


# ---- 5. formats

@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY)
def test_next_step_in_image_order_formats(env_id, fmt):
    """n = 67, 30 steps in next_step mode: every row of the handle's obs is at every step what tests/chw_referee.py makes of the u8_xyc twin's."""
    import chw_referee
    import torch

    n, T = 67, 30
    twin, env = make(env_id, n, autoreset_mode="next_step"), make(env_id, n, autoreset_mode="next_step", obs_format=fmt)
    act = dev(ni.rollout_actions(env.action_dim == 1, T, n))
    finished = 0
    for t in range(T):
        (o, r, d, _, _), (o2, r2, d2, _, _) = twin.step(act[t]), env.step(act[t])
        assert torch.equal(r, r2) and torch.equal(d, d2), "%s %s: step %d" % (env_id, fmt, t)
        assert torch.equal(vis(o2), chw_referee.converted(fmt, vis(o))), "%s %s: frames at step %d" % (env_id, fmt, t)
        finished += int(d.sum())
    assert finished >= n, finished
    for e in (twin, env):
        e.check_errors()
        e.close()


# ---- 6. captured graph

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0"])
def test_next_step_replays_from_a_graph(env_id):
    """mg_step_next captured after a first eager call (which allocates the handle's scratch) and replayed three times, the action and the flag tensor
    rewritten between the replays, against a twin that makes the same four calls eagerly.  n = 67; two ids with a NEXT kernel, one on the pair."""
    import torch
    from memory_gym_amd import _native

    n = 67
    env, twin = make(env_id, n), make(env_id, n)
    rng = np.random.default_rng(9)
    acts = dev(mi.actions(rng, env.action_dim == 1, 4, n))
    flags = dev((rng.random((4, n)) < 0.5).astype(np.uint8))
    A, R = acts[0].clone(), flags[0].clone()

    def call(e, a, r):
        rc = _native.LIB.mg_step_next(e._h, a.data_ptr(), r.data_ptr(), e.obs.data_ptr(), e._p_reward, e._p_done, e._p_gt, e._p_info, e._raw_stream())
        assert rc == 0, _native.last_error()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(env, A, R)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    call(twin, acts[0], flags[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(env, A, R)
    for k in (1, 2, 3):
        A.copy_(acts[k])
        R.copy_(flags[k])
        graph.replay()
        call(twin, acts[k], flags[k])
        torch.cuda.synchronize()
        assert torch.equal(env.reward, twin.reward) and torch.equal(env.done_u8, twin.done_u8), "%s: replay %d" % (env_id, k)
        assert torch.equal(vis(env.obs), vis(twin.obs)), "%s: obs after replay %d" % (env_id, k)
        assert np.array_equal(env.state_dict()["blob"], twin.state_dict()["blob"]), "%s: state after replay %d" % (env_id, k)
    assert env.debug_counter("next_steps") == 2  # (the eager call and the capture: a replay does not pass through the host)
    for e in (env, twin):
        e.check_errors()
        e.close()


# ---- 7. pending flags

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_reset_and_advance_clear_the_pending_flags(env_id):
    """n = 67.  Steps until instances have finished; the caller then resets exactly those by hand (a masked reset): the next step() restarts nobody a second
    time.  Later, with flags pending again, advance(3): the next step() restarts nobody.  The twin runs the same calls with the pair of the definition."""
    import torch

    n = 67
    env, twin = make(env_id, n, autoreset_mode="next_step"), make(env_id, n, autoreset_mode="disabled")
    act = dev(ni.rollout_actions(env.action_dim == 1, 40, n))
    prev = torch.zeros(n, dtype=torch.bool, device="cuda")
    t = 0

    def until_some_finish():
        nonlocal t, prev
        while True:
            out, out2 = env.step(act[t]), twin_pair(twin, act[t], prev)
            same_handles(env, twin, out, out2, t, env_id)
            prev = out[2].clone()
            t += 1
            if int(prev.sum()) >= 3:
                return
            assert t < 30, "nothing finishes"

    until_some_finish()
    env.reset(mask=prev)
    twin.reset(mask=prev)
    assert not bool(env.done_u8.any())
    none = torch.zeros(n, dtype=torch.bool, device="cuda")
    out, out2 = env.step(act[t]), twin_pair(twin, act[t], none)
    same_handles(env, twin, out, out2, t, env_id + ": after the masked reset")
    prev = out[2].clone()
    t += 1
    until_some_finish()
    env.advance(3, eps=0.5, seed=3, step=0, render=False)
    twin.advance(3, eps=0.5, seed=3, step=0, render=False)
    assert not bool(env.done_u8.any())
    out, out2 = env.step(act[t]), twin_pair(twin, act[t], none)
    same_handles(env, twin, out, out2, t, env_id + ": after advance()")
    for e in (env, twin):
        e.close()


@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY)
def test_checkpoint_in_the_middle_of_a_next_step_rollout(env_id):
    """n = 67: state_dict() after 12 steps in next_step mode -- flags are pending, asserted -- loaded into a fresh handle: both continue 14 steps bit for
    bit.  The dictionary carries the flags under one extra key in this mode only."""
    import memory_gym_amd
    import torch

    n = 67
    A = make(env_id, n, autoreset_mode="next_step")
    act = dev(ni.rollout_actions(A.action_dim == 1, 40, n))
    t = 0
    while t < 12 or not bool(A.done_u8.any()):
        A.step(act[t])
        t += 1
    sd = A.state_dict()
    assert sd["next_step_pending"].any() and sd["next_step_pending"].dtype == np.uint8
    B = memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="next_step")
    B.load_state_dict(sd)
    finished = 0
    for k in range(t, t + 14):
        (o, r, d, _, i), (o2, r2, d2, _, i2) = A.step(act[k]), B.step(act[k])
        assert torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(vis(o), vis(o2)), "%s: step %d" % (env_id, k)
        assert np.array_equal(A.state_dict()["blob"], B.state_dict()["blob"])
        finished += int(d.sum())
    assert finished >= n // 4, finished
    C = make(env_id, n)
    assert "next_step_pending" not in C.state_dict()
    for e in (A, B, C):
        e.close()


# ---- 8. refusals

def test_refusals():
    import ctypes as C
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    env_id, n = "MortarMayhem-Grid-v0", 67
    for kw in (dict(final_observation=True), dict(final_frames=True)):
        with pytest.raises(ValueError):
            memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="next_step", **kw)
    with pytest.raises(ValueError):
        memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="sometimes")
    step_next = _native.LIB.mg_step_next
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="next_step")
    a = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags = torch.ones(n, dtype=torch.uint8, device="cuda")
    args = [env._h, a.data_ptr(), flags.data_ptr(), env.obs.data_ptr(), env._p_reward, env._p_done, env._p_gt, env._p_info, env._raw_stream()]
    assert step_next(*args) == -1 and "before the first" in _native.last_error()
    env.reset(seed=mi.seeds(n), options=mi.SHORT[env_id])
    words = [env.rng_words(i).copy() for i in (0, n - 1)]
    for k in (1, 2, 3, 4, 5):  # a NULL actions_dev, restart_dev, obs_dev, reward_dev or done_dev
        bad = list(args)
        bad[k] = None
        assert step_next(*bad) == -1 and "NULL buffer" in _native.last_error()
    scratch = torch.zeros((n, 84 * 84 * 3), dtype=torch.uint8, device="cuda")
    for member in ("final_obs_dev", "final_frames_dev"):
        info = _native.InfoBuffers()
        C.memmove(C.byref(info), C.byref(env._info), C.sizeof(info))
        setattr(info, member, scratch.data_ptr())
        bad = list(args)
        bad[7] = C.byref(info)
        assert step_next(*bad) == -1 and "no terminal rows" in _native.last_error()
    with pytest.raises(ValueError):
        env.step(a, mask=flags)
    with pytest.raises(ValueError):
        env.step(a, render=False)
    assert env.debug_counter("next_steps") == 0 and env.debug_counter("masked_steps") == 0 and env.debug_counter("headless_steps") == 0
    for i, w in zip((0, n - 1), words):  # nothing was stepped, nobody was reset
        assert np.array_equal(env.rng_words(i), w)
    env.close()


# ---- 9. the gymnasium front end

def test_gymnasium_vector_env_in_next_step_mode():
    """In a subprocess whose path holds tests/fake_gymnasium: GymnasiumVectorEnv(autoreset_mode="next_step"), device and as_numpy layouts against a
    VecMemoryGym in the same mode; keys and masks; the default mode against a second default handle."""
    code = """
import numpy as np, torch
import gymnasium as gym
import memory_gym_amd
import masked_step_inputs as mi, next_step_inputs as ni
env_id, n, T = "MortarMayhem-Grid-v0", 9, 30
act = ni.rollout_actions(True, T, n)
ref = memory_gym_amd.make(env_id, num_envs=n, device=0, autoreset_mode="next_step", ground_truth64=True)
ref.reset(seed=5, options=mi.SHORT[env_id])
dv = memory_gym_amd.GymnasiumVectorEnv(env_id, n, autoreset_mode="next_step")
hv = memory_gym_amd.GymnasiumVectorEnv(env_id, n, autoreset_mode="next_step", as_numpy=True)
assert isinstance(dv, gym.vector.VectorEnv)
for v in (dv, hv):
    assert v.metadata["autoreset_mode"] == "next_step" and "autoreset_mode" not in memory_gym_amd.VecMemoryGym.metadata
    v.reset(seed=5, options=mi.SHORT[env_id])
keys = ["reward", "length"] + list(ref.info_names)
ended = 0
for t in range(T):
    o, r, d, _, i = ref.step(act[t])
    o1, r1, te1, tr1, i1 = dv.step(act[t])
    o2, r2, te2, tr2, i2 = hv.step(act[t])
    assert torch.equal(o1, o) and torch.equal(r1, r) and torch.equal(te1, d) and not bool(tr1.any())
    assert isinstance(o2, np.ndarray) and np.array_equal(o2, o.cpu().numpy()) and r2.dtype == np.float64 and np.array_equal(r2, ref.reward64.cpu().numpy())
    assert te2.dtype == np.bool_ and np.array_equal(te2, d.cpu().numpy()) and not tr2.any()
    for inf in (i1, i2):
        assert sorted(inf) == sorted(keys + ["_" + k for k in keys]), sorted(inf)
    for k in keys:
        assert torch.equal(i1[k], i[k]) and torch.equal(i1["_" + k], d)
        assert isinstance(i2[k], np.ndarray) and i2[k].shape == (n,) and np.array_equal(i2["_" + k], d.cpu().numpy())
        assert np.array_equal(i2[k][te2], i[k].cpu().numpy()[te2])
    ended += int(d.sum())
assert ended >= n, ended
for e in (ref, dv, hv):
    e.close()
a, b = memory_gym_amd.GymnasiumVectorEnv(env_id, n), memory_gym_amd.GymnasiumVectorEnv(env_id, n, autoreset_mode="same_step")
assert a.metadata["autoreset_mode"] == "same_step"
for v in (a, b):
    v.reset(seed=5, options=mi.SHORT[env_id])
ended = 0
for t in range(T):
    (o1, r1, te1, tr1, i1), (o2, r2, te2, tr2, i2) = a.step(act[t]), b.step(act[t])
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(te1, te2)
    assert sorted(i1) == sorted(i2) == ["_final_info", "_final_observation", "final_info", "final_observation"], sorted(i1)
    assert torch.equal(i1["final_observation"][te1], i2["final_observation"][te2])
    ended += int(te1.sum())
assert ended >= n
try:
    memory_gym_amd.GymnasiumVectorEnv(env_id, n, autoreset_mode="next_step", final_frames=True)
    raise SystemExit("final_frames=True in next_step mode did not raise")
except ValueError:
    pass
print("ok")
"""
    paths = os.pathsep.join([os.path.join(ROOT, "tests", "fake_gymnasium"), os.path.join(ROOT, "endless-memory-gym_amd"), os.path.join(ROOT, "tests")])
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=paths), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]
