"""GPU (-m gpu): caller-supplied action tapes played without a frame -- mg_play (VecMemoryGym.play) -- against the CPU oracle and against twin
handles that run the loop of its definition with device calls (step(render=False, mask=...)), all ten env ids.

The inputs are those of FINISHED in tests/test_gpu_headless.py: n = 200 (three full waves and a partial one), seeds 0..199, and as the tape the
ORACLE's expert at eps 0.3, hash seed 7, recorded while the oracle plays it with auto-reset.  The oracle alone gives, per id, the episodes of
200 steps in FINISHED and between 11 and 196 instances that have finished an episode by step 64, so a 64-step play "until done" has finished
AND unfinished instances on every id; each test asserts such conditions, so that a run in which nothing ends or nothing pauses cannot pass."""
import functools

import numpy as np
import pytest
from test_gpu_headless import EPS, FINISHED, HASH_SEED, MORTAR, N, _full, pair, same_frames, same_rng, vis

pytestmark = pytest.mark.gpu

SUMS = ("reward", "episodes", "episode_reward", "episode_length")


@functools.lru_cache(maxsize=None)
def recording(env_id, steps=200):
    """The oracle alone: -> dict(tape int32 [steps, N(, 2)], reward float64 [steps, N], done bool [steps, N], frames after the last step,
    RNG words of instances 0 and N - 1 after the last step).  Computed once per id and never written to."""
    import oracle_lib

    ref = oracle_lib.OracleBatch(env_id, N)
    ref.reset(np.arange(N, dtype=np.int64))
    tape, reward, done = [], [], []
    for t in range(steps):
        a = ref.expert_actions(EPS, HASH_SEED, t).copy()
        _, r, d = ref.step(a, autoreset=True, want_obs=False)
        tape.append(a)
        reward.append(r.copy())
        done.append(d.astype(bool))
    rec = dict(tape=np.stack(tape), reward=np.stack(reward), done=np.stack(done), frames=ref.frames(range(N)),
               rng={i: ref.envs[i].rng_words() for i in (0, N - 1)})
    ref.close()
    for v in (rec["tape"], rec["reward"], rec["done"], rec["frames"]):
        v.setflags(write=False)
    return rec


def handles(env_id, count, n=N, seed0=0, **kw):
    import memory_gym_amd

    out = []
    for _ in range(count):
        e = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
        e.reset(seed=np.arange(n, dtype=np.int64) + seed0)
        out.append(e)
    return out


def device_tape(env_id, tape):
    import torch

    return torch.as_tensor(np.array(tape), device="cuda")  # (a writable copy: the recording itself is read-only)


def definition(twin, tape, until_done=False, mask=None):
    """the loop of mg_play's definition with device calls -> the stats dictionary play(trace=True) returns"""
    import torch

    n, dev, K = twin.num_envs, twin.device, int(tape.shape[0])
    st = {"reward": torch.zeros(n, dtype=torch.float64, device=dev), "episodes": torch.zeros(n, dtype=torch.int32, device=dev),
          "episode_reward": torch.zeros(n, dtype=torch.float64, device=dev), "episode_length": torch.zeros(n, dtype=torch.int64, device=dev),
          "steps": torch.zeros(n, dtype=torch.int32, device=dev), "reward_trace": torch.zeros((K, n), dtype=torch.float32, device=dev),
          "done_trace": torch.zeros((K, n), dtype=torch.bool, device=dev)}
    for nm in twin.info_names:
        st[nm] = torch.zeros(n, dtype=torch.float64, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev) if mask is None else mask.to(dev).bool().clone()
    masked = until_done or mask is not None
    was = twin.autoreset
    twin.autoreset = not until_done
    for t in range(K):
        _, r, done, _, info = twin.step(tape[t], render=False, mask=alive.clone() if masked else None)
        st["reward_trace"][t], st["done_trace"][t] = r, done
        st["reward"] += twin.reward64
        st["episodes"] += done.to(torch.int32)
        st["episode_reward"] += torch.where(done, info["reward"], torch.zeros_like(info["reward"]))
        st["episode_length"] += torch.where(done, info["length"], torch.zeros_like(info["length"])).to(torch.int64)
        for nm in twin.info_names:
            st[nm] += torch.where(done, info[nm], torch.zeros_like(info[nm])).double()
        st["steps"] += alive.to(torch.int32)
        if until_done:
            alive &= ~done
    twin.autoreset = was
    return st


def same_stats(got, want, what):
    import torch

    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), what + ": stats[%r] differs from the definition's" % k


def same_state(env, twin, which, what):
    import torch

    for i in which:
        assert np.array_equal(env.rng_words(i), twin.rng_words(i)), what + ": RNG words of instance %d" % i
    if env.gt_dim:
        assert torch.equal(env.gt, twin.gt), what + ": ground truth"
    if env.vector_obs is not None:
        assert torch.equal(env.vector_obs, twin.vector_obs), what + ": vector observation"
    same_frames(env.redraw(), twin.redraw(), what + ": redraw()")


def close(*envs):
    for e in envs:
        e.check_errors()
        e.close()


# ---- 1. MG_PLAY_THROUGH against the oracle and against the definition

@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_play_through_equals_the_oracle_and_the_definition(env_id):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin, split = handles(env_id, 3)
    c0 = (env.debug_counter("play_fused_steps"), env.debug_counter("headless_steps"))
    obs, st = env.play(tape, trace=True)
    c1 = (env.debug_counter("play_fused_steps"), env.debug_counter("headless_steps"))
    assert (c1[0] - c0[0], c1[1] - c0[1]) == ((200, 0) if env_id in MORTAR else (0, 200))
    reward = np.zeros(N)
    for t in range(200):
        reward += rec["reward"][t]
    assert np.array_equal(st["reward"].cpu().numpy(), reward), "reward sums against the oracle's loop"
    assert np.array_equal(st["episodes"].cpu().numpy(), rec["done"].sum(0).astype(np.int32)), "episodes against the oracle's loop"
    assert int(st["episodes"].sum()) == FINISHED[env_id]
    assert np.array_equal(st["done_trace"].cpu().numpy(), rec["done"]) and np.array_equal(st["reward_trace"].cpu().numpy(), rec["reward"].astype(np.float32))
    same_frames(obs, rec["frames"], env_id + ": frames after play(200)")
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), rec["rng"][i]), "RNG words of instance %d against the oracle" % i
    assert bool((st["steps"] == 200).all())
    same_stats(st, definition(twin, tape), env_id)
    same_state(env, twin, (0, N // 2, N - 1), env_id)
    parts, at = [], 0
    for k in (1, 7, 56, 136):
        o2, s2 = split.play(tape[at:at + k])
        parts.append({key: s2[key].clone() for key in ("episodes", "episode_length", "steps")})
        at += k
    same_frames(o2, obs, env_id + ": as 1 + 7 + 56 + 136")
    for key in ("episodes", "episode_length", "steps"):
        assert torch.equal(sum(p[key] for p in parts), st[key]), "as 1 + 7 + 56 + 136: stats[%r]" % key
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), split.rng_words(i)), "as 1 + 7 + 56 + 136: RNG words of instance %d" % i
    close(env, twin, split)


# ---- 2. MG_PLAY_EPISODE

@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_play_until_done_equals_the_definition_and_the_oracle(env_id):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin = handles(env_id, 2)
    _, st = env.play(tape[:64], until_done=True, trace=True, render=False)
    same_stats(st, definition(twin, tape[:64], until_done=True), env_id)
    same_state(env, twin, range(N), env_id)  # (terminal frames of the finished instances, current frames of the others)
    finished = st["done_trace"].any(0)
    fin = finished.cpu().numpy()
    print("%s: %d of %d finished within 64 steps" % (env_id, int(fin.sum()), N))
    assert 11 <= int(fin.sum()) <= 196, int(fin.sum())
    first = rec["done"][:64].argmax(0)  # the oracle's first-done step (where it has one within 64 steps)
    assert np.array_equal(fin, rec["done"][:64].any(0)), "who finished, against the oracle"
    steps = st["steps"].cpu().numpy()
    assert np.array_equal(steps[fin] - 1, first[fin]) and bool((steps[~fin] == 64).all())
    rt = st["reward_trace"].cpu().numpy()
    for i in np.nonzero(fin)[0]:
        want = rec["reward"][:first[i] + 1, i].astype(np.float32)
        assert np.array_equal(rt[:first[i] + 1, i], want) and not rt[first[i] + 1:, i].any(), "reward trace of instance %d against the oracle" % i
        assert float(st["reward"][i]) == float(np.add.accumulate(rec["reward"][:first[i] + 1, i])[-1]), "reward sum of instance %d against the oracle" % i
    assert bool((st["episodes"] == finished.to(torch.int32)).all())
    # the finished instances re-started by a masked reset, then a second play
    for e in (env, twin):
        e.reset(mask=finished)
    _, st = env.play(tape[64:96], until_done=True, trace=True, render=False)
    same_stats(st, definition(twin, tape[64:96], until_done=True), env_id + ", second play")
    same_state(env, twin, range(0, N, 7), env_id + ", second play")
    close(env, twin)


# ---- 3. an initial mask

@pytest.mark.parametrize("until_done", [False, True])
@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"])
def test_play_with_an_initial_mask(env_id, until_done):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin = handles(env_id, 2)
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[::3] = True
    before = env.redraw().clone() if not isinstance(env.redraw(), dict) else None
    words = {i: env.rng_words(i) for i in (1, 2, N - 1)}  # (N - 1 = 199: no multiple of three)
    m0 = env.debug_counter("masked_steps")
    _, st = env.play(tape[:64], until_done=until_done, mask=mask, trace=True, render=False)
    if env_id not in MORTAR:
        assert env.debug_counter("masked_steps") - m0 == 64
    same_stats(st, definition(twin, tape[:64], until_done=until_done, mask=mask), env_id)
    same_state(env, twin, range(0, N, 3), env_id)
    off = ~mask
    for i, w in words.items():
        assert np.array_equal(env.rng_words(i), w), "a paused instance's RNG stream moved"
    if before is not None:
        assert torch.equal(env.redraw()[off], before[off]), "a paused instance's frame changed"
    assert not bool(st["steps"][off].any()) and not bool(st["reward_trace"][:, off].any()) and not bool(st["done_trace"][:, off].any())
    for k in SUMS + tuple(env.info_names):
        assert not bool(st[k][off].any()), "stats[%r] of a paused instance" % k
    # the active instances against the oracle's own run of the tape (instances are independent: the paused ones change nothing for them)
    on, steps, episodes = mask.cpu().numpy(), st["steps"].cpu().numpy(), st["episodes"].cpu().numpy()
    fin, first = rec["done"][:64].any(0), rec["done"][:64].argmax(0)
    if until_done:
        assert np.array_equal(steps[on], np.where(fin, first + 1, 64)[on]) and np.array_equal(episodes[on], fin[on].astype(np.int32))
    else:
        assert bool((steps[on] == 64).all()) and np.array_equal(episodes[on], rec["done"][:64].sum(0)[on].astype(np.int32))
    assert np.array_equal(st["done_trace"].cpu().numpy()[:, on].any(0), fin[on])
    close(env, twin)


# ---- 4. more steps than one launch takes

def test_play_beyond_the_per_launch_cap():
    """MortarMayhem-Grid-v0, a 1,500-step tape: two launches of the in-launch form (1,024 + 476 steps), against the oracle; the same tape until done."""
    env_id = "MortarMayhem-Grid-v0"
    rec = recording(env_id, 1500)
    tape = device_tape(env_id, rec["tape"])
    env, epi = handles(env_id, 2)
    obs, st = env.play(tape, trace=True)
    reward = np.zeros(N)
    for t in range(1500):
        reward += rec["reward"][t]
    episodes = rec["done"].sum(0).astype(np.int32)
    assert np.array_equal(st["reward"].cpu().numpy(), reward) and np.array_equal(st["episodes"].cpu().numpy(), episodes)
    assert int(episodes.sum()) >= 1500, int(episodes.sum())  # (508 in 200 steps)
    assert np.array_equal(st["done_trace"].cpu().numpy(), rec["done"]) and bool((st["steps"] == 1500).all())
    same_frames(obs, rec["frames"], "play(1500)")
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), rec["rng"][i])
    assert env.debug_counter("play_fused_steps") == 1500 and env.debug_counter("headless_steps") == 0
    _, st = epi.play(tape, until_done=True, trace=True, render=False)
    steps = st["steps"].cpu().numpy()
    assert int(steps.max()) <= 118, int(steps.max())  # (the oracle's last first-done step is 117)
    assert bool(st["done_trace"].any(0).all()) and bool((st["episodes"] == 1).all())
    assert np.array_equal(steps - 1, rec["done"].argmax(0)) and not bool(st["done_trace"][118:].any()) and not bool(st["reward_trace"][118:].any())
    close(env, epi)


# ---- 5. save -> play -> load -> play

@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "Endless-MysteryPath-v0"])
def test_a_reloaded_state_replays_a_tape(env_id):
    import torch

    env, twin = handles(env_id, 2)
    for e in (env, twin):
        e.advance(40, eps=0.1, seed=1, render=False, stats=False)
    snap, snap2 = env.save_instances(), twin.save_instances()
    g = torch.Generator(device="cpu").manual_seed(5)
    shape, high = ((60, N), 4) if env.action_dim == 1 else ((60, N, 2), 3)
    tapes = [torch.randint(0, high, shape, generator=g, dtype=torch.int32).cuda() for _ in range(2)]
    assert not torch.equal(tapes[0], tapes[1])
    runs = []
    for tape in (tapes[0], tapes[1], tapes[0]):
        env.load_instances(snap, render=False)
        _, st = env.play(tape, trace=True, render=False)
        runs.append({k: v.clone() for k, v in st.items()})
    assert all(torch.equal(runs[0][k], runs[2][k]) for k in runs[0]), "the first tape played again after the second"
    assert not torch.equal(runs[0]["reward_trace"], runs[1]["reward_trace"]), "two different tapes gave the same rewards"
    twin.load_instances(snap2, render=False)
    same_stats(runs[2], definition(twin, tapes[0]), env_id)
    same_state(env, twin, (0, N - 1), env_id)
    close(env, twin)


@pytest.mark.parametrize("env_id,opt_a,opt_b", [("SearingSpotlights-v0", dict(num_coins=[3], use_exit=True), dict(num_coins=[1, 2], use_exit=False, max_steps=90)),
                                                ("MortarMayhem-Grid-v0", dict(command_count=[3]), dict(command_count=[8, 10]))])
@pytest.mark.parametrize("until_done", [False, True])
def test_play_with_two_option_sets(env_id, opt_a, opt_b, until_done):
    """the halves of one handle under two option sets (the handle's per-set kernels): play() against the definition on a twin set up alike"""
    import torch

    n = 256
    env, twin = handles(env_id, 2, n=n, seed0=3)
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:n // 2] = True
    for e in (env, twin):
        e.reset(seed=seeds, options=opt_a, mask=mask_a)
        e.reset(seed=seeds, options=opt_b, mask=~mask_a)
    tape = torch.stack([twin.expert_actions(0.1, HASH_SEED, t) for t in range(120)])  # (the teacher in the FIRST states throughout: some competent tape)
    g = torch.Generator(device="cpu").manual_seed(9)
    tape = torch.where(torch.rand(tape.shape, generator=g).cuda() < 0.5, tape, torch.randint(0, 3, tape.shape, generator=g, dtype=torch.int32).cuda())
    _, st = env.play(tape, until_done=until_done, trace=True, render=False)
    same_stats(st, definition(twin, tape, until_done=until_done), env_id)
    same_state(env, twin, (0, n // 2 - 1, n // 2, n - 1), env_id)
    assert int(st["episodes"].sum()) > 0
    close(env, twin)


# ---- 6. image-order formats and capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "MysteryPath-v0"])
def test_play_in_an_image_order_format(env_id):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin = handles(env_id, 2, obs_format="bf16_chw")
    obs, st = env.play(tape[:60])
    for t in range(60):
        o, _, _, _, _ = twin.step(tape[t])
    assert torch.equal(vis(obs), vis(o)), "%s bf16_chw: frames after play(60) against a twin that drew every step" % env_id
    assert int(st["episodes"].sum()) > 0
    close(env, twin)


@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_play_replays_from_a_graph(env_id):
    """The handle's first call under capture is refused; after an eager call, play(8 steps, until done, a mask) is captured once and replayed three times
    with the tape and mask tensors overwritten between the replays, against a twin that makes the same three calls eagerly."""
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin, fresh = handles(env_id, 3)
    T = tape[:8].clone()
    M = torch.ones(N, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="first call"):
        with torch.cuda.graph(refused):
            fresh.play(T, until_done=True, mask=M, trace=True, render=False)
    torch.cuda.synchronize()
    fresh.close()  # (its stats tensors belong to the capture that failed: the handle is not used again)
    for e in (env, twin):
        e.play(tape[:8], trace=True, render=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, st = env.play(T, until_done=True, mask=M, trace=True, render=False)
    assert obs is None
    for r in range(3):
        T.copy_(tape[8 + 8 * r:16 + 8 * r])
        M.copy_(torch.arange(N, device="cuda") % (r + 2) != 0)
        graph.replay()
        _, want = twin.play(T.clone(), until_done=True, mask=M.clone(), trace=True, render=False)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(st[k], want[k]), "replay %d: stats[%r]" % (r, k)
        assert not bool(st["steps"][::r + 2].any()) and int(st["steps"].sum()) > 0
        same_frames(env.redraw(), twin.redraw(), "%s: redraw() after replay %d" % (env_id, r))
        finished = st["done_trace"].any(0).clone()
        for e in (env, twin):  # (an instance that has finished is re-started before the next replay steps it again)
            e.reset(mask=finished)
    same_state(env, twin, range(0, N, 9), env_id)
    close(env, twin)


# ---- 7. refusals

def test_refusals():
    import ctypes as C

    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    env_id, n = "MortarMayhem-Grid-v0", 70
    fresh = memory_gym_amd.make(env_id, num_envs=n, device=0)
    tape = torch.zeros((5, n), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="before the first mg_reset"):
        fresh.play(tape)
    fresh.close()
    env, twin = handles(env_id, 2, n=n)
    with pytest.raises(ValueError):
        env.play(torch.zeros((0, n), dtype=torch.int32, device="cuda"))
    for shape in ((n,), (5, n + 1), (5, n, 2), (5, n, 1)):
        with pytest.raises(ValueError):
            env.play(torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        env.play(tape, mask=torch.ones(n + 1, dtype=torch.bool, device="cuda"))
    lib, null = _native.LIB, None
    assert lib.mg_play(env._h, tape.data_ptr(), 0, 0, null, null, null, null, null, None, env._raw_stream()) == -1 and "steps < 1" in _native.last_error()
    assert lib.mg_play(env._h, null, 5, 0, null, null, null, null, null, None, env._raw_stream()) == -1 and "tape_dev" in _native.last_error()
    assert lib.mg_play(env._h, tape.data_ptr(), 5, 2, null, null, null, null, null, None, env._raw_stream()) == -1 and "mode" in _native.last_error()
    out = _native.AdvanceOut()
    out.struct_size = 12
    assert lib.mg_play(env._h, tape.data_ptr(), 5, 0, null, null, null, null, null, C.byref(out), env._raw_stream()) == -1 and "struct_size" in _native.last_error()
    a = twin.expert_actions(EPS, HASH_SEED, 0)
    (o1, r1, d1, _, _), (o2, r2, d2, _, _) = env.step(a), twin.step(a)  # nothing was stepped
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and np.array_equal(env.rng_words(0), twin.rng_words(0))
    assert env.debug_counter("play_fused_steps") == 0 and env.debug_counter("headless_steps") == 0
    arr = (C.c_double * 1)(4.0)
    assert lib.mg_set_option(env._h, b"arena_size", arr, 1) == 0  # a geometry option: a reset is needed first
    with pytest.raises(RuntimeError, match="geometry"):
        env.play(tape)
    env.close()
    twin.close()


# ---- 8. the gymnasium front end

def test_vector_front_end_passes_play_through():
    import memory_gym_amd
    from memory_gym_amd.vector import GymnasiumVectorEnv

    env_id, n = "MortarMayhemB-Grid-v0", 70
    venv = GymnasiumVectorEnv(env_id, n, device=0, as_numpy=True)
    plain = memory_gym_amd.make(env_id, num_envs=n, device=0)
    venv.reset(seed=4)
    plain.reset(seed=4)
    tape = np.random.Generator(np.random.PCG64(3)).integers(0, 4, (50, n)).astype(np.int32)
    obs, st = venv.play(tape, trace=True)
    o2, s2 = plain.play(tape, trace=True)
    assert isinstance(obs, dict) and isinstance(obs["visual_observation"], np.ndarray) and isinstance(st["steps"], np.ndarray)
    assert np.array_equal(obs["visual_observation"], o2["visual_observation"].cpu().numpy())
    assert np.array_equal(obs["vector_observation"], o2["vector_observation"].cpu().numpy())
    assert sorted(st) == sorted(s2) and all(np.array_equal(st[k], s2[k].cpu().numpy()) for k in st) and int(st["episodes"].sum()) > 0
    assert st["done_trace"].dtype == np.bool_ and st["done_trace"].shape == (50, n)
    assert venv.play(tape, until_done=True, render=False, stats=False) == (None, None)
    venv.close()
    plain.close()
