"""GPU (-m gpu): rollout traces -- mg_advance_traced / mg_play_traced (VecMemoryGym.advance_traced(ro) / play(trace=ro), RolloutTrace.draw) -- against
the CPU oracle and against twin handles that run the loop of the definition with device calls (expert_actions, step(render=False, mask=...),
save_frames(out=store[t])), all ten env ids.

The inputs are those of tests/test_gpu_headless.py / tests/test_gpu_play.py: n = 200 (three full waves and a partial one), seeds 0..199, the
oracle's expert at eps 0.3, hash seed 7.  The oracle alone gives, per id, FINISHED episodes in 200 steps and between 11 and 196 instances that
have finished an episode by step 64; the tests assert such conditions again, so that a run in which nothing ends or nothing pauses cannot pass."""
import ctypes as C
import functools

import numpy as np
import pytest
from test_gpu_headless import EPS, FINISHED, HASH_SEED, MORTAR, N, same_frames, vis
from test_gpu_play import close, device_tape, handles, recording, same_state

pytestmark = pytest.mark.gpu

K = 64
SUMS = ("reward", "episodes", "episode_reward", "episode_length")


@functools.lru_cache(maxsize=None)
def oracle_rollout(env_id, steps=K):
    """The oracle alone plays its own expert with step_digest: -> dict(digest uint64 [steps + 1, N] (row 0: the reset frames), actions, labels (the
    expert at eps 0 in the same states), reward float64 [steps, N], done bool [steps, N]).  Computed once per id and never written to."""
    import oracle_lib

    ref = oracle_lib.OracleBatch(env_id, N)
    digest, actions, labels, reward, done = [ref.reset_digest(np.arange(N, dtype=np.int64)).copy()], [], [], [], []
    for t in range(steps):
        labels.append(ref.expert_actions(0.0, HASH_SEED, t).copy())
        a = ref.expert_actions(EPS, HASH_SEED, t).copy()
        dg, _, r, d = ref.step_digest(a, autoreset=True)
        actions.append(a)
        digest.append(dg.copy())
        reward.append(r.copy())
        done.append(d.astype(bool))
    ref.close()
    out = dict(digest=np.stack(digest), actions=np.stack(actions), labels=np.stack(labels), reward=np.stack(reward), done=np.stack(done))
    for v in out.values():
        v.setflags(write=False)
    return out


def advance_definition(twin, steps, eps, seed, step0, labels=True):
    """the loop of mg_advance_traced's definition with device calls -> dict of the trace's tensors"""
    import torch

    B = twin.frame_record_bytes
    n, dev = twin.num_envs, twin.device
    acts = (steps, n) if twin.action_dim == 1 else (steps, n, 2)
    w = dict(frames=torch.zeros((steps + 1, n, B), dtype=torch.uint8, device=dev), actions=torch.zeros(acts, dtype=torch.int32, device=dev),
             reward=torch.zeros((steps, n), dtype=torch.float32, device=dev), done=torch.zeros((steps, n), dtype=torch.bool, device=dev))
    if labels:
        w["labels"] = torch.zeros(acts, dtype=torch.int32, device=dev)
    was = twin.autoreset
    twin.autoreset = True
    twin.save_frames(out=w["frames"][0])
    for t in range(steps):
        if labels:
            twin.expert_actions(0.0, seed, step0 + t, out=w["labels"][t])
        twin.expert_actions(eps, seed, step0 + t, out=w["actions"][t])
        _, r, d, _, _ = twin.step(w["actions"][t], render=False)
        w["reward"][t], w["done"][t] = r, d
        twin.save_frames(out=w["frames"][t + 1])
    twin.autoreset = was
    return w


def play_definition(twin, tape, until_done=False, mask=None):
    """the loop of mg_play_traced's definition with device calls: step(render=False, mask=...) plus save_frames(out=store[t]) -> dict of the trace's tensors
    and "steps", the steps each instance took"""
    import torch

    B = twin.frame_record_bytes
    n, dev, steps = twin.num_envs, twin.device, int(tape.shape[0])
    w = dict(frames=torch.zeros((steps + 1, n, B), dtype=torch.uint8, device=dev), reward=torch.zeros((steps, n), dtype=torch.float32, device=dev),
             done=torch.zeros((steps, n), dtype=torch.bool, device=dev), steps=torch.zeros(n, dtype=torch.int32, device=dev))
    alive = torch.ones(n, dtype=torch.bool, device=dev) if mask is None else mask.to(dev).bool().clone()
    masked = until_done or mask is not None
    was = twin.autoreset
    twin.autoreset = not until_done
    twin.save_frames(out=w["frames"][0])
    for t in range(steps):
        _, r, d, _, _ = twin.step(tape[t], render=False, mask=alive.clone() if masked else None)
        w["reward"][t], w["done"][t] = r, d
        w["steps"] += alive.to(torch.int32)
        twin.save_frames(out=w["frames"][t + 1])
        if until_done:
            alive &= ~d
    twin.autoreset = was
    return w


def same_trace(ro, want, keys, what):
    import torch

    for k in keys:
        got = getattr(ro, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (what, k, got.dtype, tuple(got.shape))
        if not torch.equal(got, want[k]):
            flat = (got != want[k]).reshape(got.shape[0], got.shape[1], -1).any(2)
            t, i = (int(v) for v in flat.nonzero()[0])
            raise AssertionError("%s: trace.%s differs from the definition's, first at (t, i) = (%d, %d) of %d entries" % (what, k, t, i, int(flat.sum())))


def counters(env):
    return tuple(env.debug_counter(k) for k in ("traced_steps", "traced_fused_steps", "advance_fused_steps", "play_fused_steps", "headless_steps"))


def delta(env, before):
    return tuple(a - b for a, b in zip(counters(env), before))


# ---- 1. advance_traced(ro) against the oracle

@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_traced_advance_equals_the_oracle(env_id):
    import torch
    from frame_digest import as_uint64, digest_torch

    rec = oracle_rollout(env_id)
    fin = rec["done"].any(0)
    print("%s: %d of %d finished within %d steps, %d episodes" % (env_id, int(fin.sum()), N, K, int(rec["done"].sum())))
    assert 11 <= int(fin.sum()) <= 196, int(fin.sum())  # finished AND unfinished instances by step 64, by the oracle alone
    assert int(recording(env_id)["done"].sum()) == FINISHED[env_id]
    assert not np.array_equal(rec["actions"], rec["labels"]), "eps 0.3 never replaced the teacher's action"
    env, twin = handles(env_id, 2)
    ro = env.new_rollout(K, labels=True)
    c0 = counters(env)
    _, st = env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=0, render=False)
    assert delta(env, c0) == ((K, K, K, 0, 0) if env_id in MORTAR else (K, 0, 0, 0, K))
    _, st2 = twin.advance(K, eps=EPS, seed=HASH_SEED, step=0, render=False)
    for k in SUMS + tuple(env.info_names):
        assert torch.equal(st[k], st2[k]), "stats[%r] differs from an untraced twin's" % k
    assert np.array_equal(ro.actions.cpu().numpy(), rec["actions"]), "actions against the oracle's"
    assert np.array_equal(ro.labels.cpu().numpy(), rec["labels"]), "labels against the oracle's eps-0 actions"
    assert np.array_equal(ro.reward.cpu().numpy(), rec["reward"].astype(np.float32)) and np.array_equal(ro.done.cpu().numpy(), rec["done"])
    assert ro.frame_layout == env.frame_layout() and ro.steps == K and ro.num_envs == N
    t = torch.arange(K + 1, device="cuda").repeat_interleave(N)
    i = torch.arange(N, device="cuda").repeat(K + 1)
    got = as_uint64(digest_torch(ro.draw(env, t, i))).reshape(K + 1, N)
    bad = np.argwhere(got != rec["digest"])
    assert not len(bad), "%s: %d frames of the trace differ from the oracle's, first at (row, i) = %s (row 0: the reset frames, row t + 1: step t)" % (
        env_id, len(bad), tuple(bad[0]))
    same_state(env, twin, (0, N // 2, N - 1), env_id)
    close(env, twin)


# ---- 2. play(trace=ro) against the definition

@pytest.mark.parametrize("episode", [False, True], ids=["through", "until_done_masked"])
@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_traced_play_equals_the_definition(env_id, episode):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])[:K]
    env, twin = handles(env_id, 2)
    mask = None
    if episode:
        mask = torch.zeros(N, dtype=torch.bool, device="cuda")
        mask[::3] = True
    on = np.ones(N, bool) if mask is None else mask.cpu().numpy()
    fin, first = rec["done"][:K].any(0), rec["done"][:K].argmax(0)
    assert (fin & on).any() and (~fin & on).any(), "the oracle's tape must finish some of the playing instances and leave some unfinished"
    ro = env.new_rollout(K)
    marker = torch.full_like(ro.actions, -7)
    ro.actions.copy_(marker)
    c0 = counters(env)
    _, st = env.play(tape, until_done=episode, mask=mask, trace=ro, render=False)
    assert delta(env, c0) == ((K, K, 0, K, 0) if env_id in MORTAR else (K, 0, 0, 0, K))
    want = play_definition(twin, tape, until_done=episode, mask=mask)
    same_trace(ro, want, ("frames", "reward", "done"), env_id)
    assert torch.equal(st["steps"], want["steps"]) and "reward_trace" not in st
    assert torch.equal(ro.actions, marker), "play() wrote trace.actions: the tape is the caller's"
    same_state(env, twin, range(0, N, 3) if episode else (0, N // 2, N - 1), env_id)
    done = ro.done.cpu().numpy()
    if not episode:
        assert np.array_equal(done, rec["done"][:K]) and np.array_equal(ro.reward.cpu().numpy(), rec["reward"][:K].astype(np.float32))
    else:
        frames, reward = ro.frames.cpu().numpy(), ro.reward.cpu().numpy()
        assert np.array_equal(done.any(0), fin & on), "who finished, against the oracle"
        for i in range(N):
            if not on[i]:  # never alive: every row repeats the record from before the call
                assert (frames[:, i] == frames[0, i]).all() and not done[:, i].any() and not reward[:, i].any(), "paused instance %d" % i
            elif fin[i]:   # rows after its own done repeat the terminal record
                f = first[i]
                assert done[f, i] and done[:, i].sum() == 1 and (frames[f + 1:, i] == frames[f + 1, i]).all(), "finished instance %d" % i
                assert not reward[f + 1:, i].any()
        # the terminal record draws the terminal frame: what redraw() shows for a finished instance
        pick = np.nonzero(fin & on)[0]
        got = ro.draw(env, [K] * len(pick), pick.tolist())
        assert torch.equal(got, vis(env.redraw())[torch.as_tensor(pick, device="cuda")])
    close(env, twin)


# ---- 3. a trace drawn in another format

@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "MysteryPath-v0", "SearingSpotlights-v0"])
def test_a_trace_draws_in_another_format(env_id, fmt):
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])[:K]
    (env,), (twin,) = handles(env_id, 1), handles(env_id, 1, obs_format=fmt)
    ro = env.new_rollout(K)
    env.play(tape, trace=ro, render=False)
    assert bool(ro.done.any())
    every = list(range(N))
    assert torch.equal(ro.draw(env, [0] * N, every, obs_format=fmt), vis(twin.redraw())), "row 0 against the twin's reset frames"
    for t in range(K):
        o, _, _, _, _ = twin.step(tape[t])
        if t in (0, 12, 25, 38, 51, 63):
            got = ro.draw(env, [t + 1] * N, every, obs_format=fmt)
            assert got.dtype == vis(o).dtype and torch.equal(got, vis(o)), "%s %s: frames of step %d against a twin that drew them" % (env_id, fmt, t)
    close(env, twin)


# ---- 4. beyond the per-launch cap

def test_traces_beyond_the_per_launch_cap():
    """MortarMayhem-v0, 64 instances, 1,030 steps: two launches of each in-launch form (1,024 + 6 steps), the second one's rows offset by the host."""
    import torch

    env_id, n, steps = "MortarMayhem-v0", 64, 1030
    env, twin, epi, epi_twin = handles(env_id, 4, n=n)
    ro = env.new_rollout(steps, labels=True)
    c0 = counters(env)
    env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=0, render=False)
    assert delta(env, c0) == (steps, steps, steps, 0, 0)
    want = advance_definition(twin, steps, EPS, HASH_SEED, 0)
    assert bool(want["done"][:1024].any()) and bool((want["frames"][1025:] != want["frames"][1024]).any()), "nothing happens on one side of step 1,024"
    same_trace(ro, want, ("frames", "actions", "labels", "reward", "done"), env_id)
    same_state(env, twin, (0, n - 1), env_id)
    tape = ro.actions.clone()
    ro2 = epi.new_rollout(steps)
    _, st = epi.play(tape, until_done=True, trace=ro2, render=False)
    want = play_definition(epi_twin, tape, until_done=True)
    same_trace(ro2, want, ("frames", "reward", "done"), env_id + " until done")
    early = want["done"][:1024].any(0)  # finished inside the first launch: the second one only repeats their terminal records
    print("until done: %d of %d finished before step 1,024, %d after it" % (int(early.sum()), n, int(want["done"][1024:].sum())))
    assert torch.equal(st["steps"], want["steps"]) and bool(early.any())
    assert bool((ro2.frames[1025:, early] == ro2.frames[1024, early]).all())
    close(env, twin, epi, epi_twin)


# ---- 5. two workgroups with a partial last wave

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-MortarMayhem-v0"])
def test_two_workgroups_and_a_partial_wave(env_id):
    import torch

    n, steps = 321, 32
    env, twin, epi, epi_twin = handles(env_id, 4, n=n)
    ro = env.new_rollout(steps, labels=True)
    env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=5, render=False)
    same_trace(ro, advance_definition(twin, steps, EPS, HASH_SEED, 5), ("frames", "actions", "labels", "reward", "done"), env_id)
    same_state(env, twin, (0, 255, 256, n - 1), env_id)
    mask = torch.arange(n, device="cuda") % 5 != 0
    ro2 = epi.new_rollout(steps)
    epi.play(ro.actions, until_done=True, mask=mask, trace=ro2, render=False)
    same_trace(ro2, play_definition(epi_twin, ro.actions, until_done=True, mask=mask), ("frames", "reward", "done"), env_id + " until done")
    same_state(epi, epi_twin, (0, 255, 256, n - 1), env_id)
    assert bool((ro2.frames[:, n - 1] != 0).any()) and bool((ro2.frames[:, 320] == ro2.frames[0, 320]).all())  # (320 = 5 x 64: paused)
    close(env, twin, epi, epi_twin)


# ---- 6. trace offsets beyond 4 GiB inside one launch

def test_trace_offsets_beyond_4_gib():
    """MortarMayhem-Grid-v0, 270,336 instances, 1,024 steps, frames only: 16 x 270,336 x 1,024 B = 4.43 GB written by ONE launch; rows 1,000 and 1,023
    (byte offsets 4.33 and 4.42 GB) against a twin's records saved at those steps."""
    import memory_gym_amd
    import torch

    env_id, n, steps = "MortarMayhem-Grid-v0", 270336, 1024
    free = torch.cuda.mem_get_info(0)[0]
    if free < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory for a 4.43 GB trace and two handles, %.1f GiB are free" % (free / 2.0 ** 30))
    env, twin = handles(env_id, 2, n=n)
    B = env.frame_record_bytes
    assert B == 16 and n * steps * B > 1 << 32 and 1000 * n * B > 1 << 32
    ro = memory_gym_amd.RolloutTrace(torch.zeros((steps + 1, n, B), dtype=torch.uint8, device="cuda"), 0, None, None, None, None)
    c0 = counters(env)
    env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=0, render=False, stats=False)
    assert delta(env, c0) == (steps, steps, steps, 0, 0)
    assert torch.equal(ro.frames[steps], env.save_frames().records), "the last row against save_frames() after the call"
    twin.advance(1001, eps=EPS, seed=HASH_SEED, step=0, render=False, stats=False)
    assert torch.equal(ro.frames[1001], twin.save_frames().records), "row 1,000 (the frame after step 1,000) against the twin's"
    twin.advance(23, eps=EPS, seed=HASH_SEED, step=1001, render=False, stats=False)
    assert torch.equal(ro.frames[1024], twin.save_frames().records), "row 1,023 against the twin's"
    assert not torch.equal(ro.frames[1001], ro.frames[1024]) and not torch.equal(ro.frames[1], ro.frames[1001])
    pick = [0, 77, n // 2, n - 1]
    assert torch.equal(ro.draw(env, [steps] * 4, pick), env.redraw()[pick])
    del ro
    close(env, twin)


# ---- 7. per-instance option sets

@pytest.mark.parametrize("env_id,opt_a,opt_b", [("SearingSpotlights-v0", dict(num_coins=[3], use_exit=True), dict(num_coins=[1, 2], use_exit=False, max_steps=90)),
                                                ("MortarMayhem-Grid-v0", dict(command_count=[3]), dict(command_count=[8, 10]))])
def test_traces_with_two_option_sets(env_id, opt_a, opt_b):
    import torch

    n, steps = 256, 120
    env, twin, epi, epi_twin = handles(env_id, 4, n=n, seed0=3)
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:n // 2] = True
    for e in (env, twin, epi, epi_twin):
        e.reset(seed=seeds, options=opt_a, mask=mask_a)
        e.reset(seed=seeds, options=opt_b, mask=~mask_a)
    ro = env.new_rollout(steps, labels=True)
    c0 = counters(env)
    env.advance_traced(ro, eps=0.1, seed=HASH_SEED, step=0, render=False)
    assert delta(env, c0)[:2] == ((steps, steps) if env_id in MORTAR else (steps, 0))
    same_trace(ro, advance_definition(twin, steps, 0.1, HASH_SEED, 0), ("frames", "actions", "labels", "reward", "done"), env_id)
    same_state(env, twin, (0, n // 2 - 1, n // 2, n - 1), env_id)
    assert bool(ro.done.any())
    ro2 = epi.new_rollout(steps)
    epi.play(ro.actions, until_done=True, trace=ro2, render=False)
    same_trace(ro2, play_definition(epi_twin, ro.actions, until_done=True), ("frames", "reward", "done"), env_id + " until done")
    close(env, twin, epi, epi_twin)


# ---- 8. right after load_instances

@pytest.mark.parametrize("env_id", ["MortarMayhemB-v0", "Endless-MysteryPath-v0"])
def test_a_trace_started_from_a_loaded_record(env_id):
    import torch

    env, twin = handles(env_id, 2)
    snaps = []
    for e in (env, twin):
        e.advance(40, eps=0.1, seed=1, render=False, stats=False)
        snaps.append(e.save_instances())
        e.advance(25, eps=0.5, seed=2, render=False, stats=False)
        e.load_instances(snaps[-1], render=False)
    ro = env.new_rollout(K, labels=True)
    env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=40, render=False)
    want = advance_definition(twin, K, EPS, HASH_SEED, 40)
    same_trace(ro, want, ("frames", "actions", "labels", "reward", "done"), env_id)
    same_state(env, twin, (0, N - 1), env_id)
    env.load_instances(snaps[0], render=False)
    ro2 = env.new_rollout(K)
    env.play(ro.actions, trace=ro2, render=False)
    assert torch.equal(ro2.frames, ro.frames) and torch.equal(ro2.done, ro.done), "the recorded actions replayed from the same record"
    assert bool((ro.frames[1:] != ro.frames[:-1]).any())
    close(env, twin)


# ---- 9. capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_traced_calls_replay_from_a_graph(env_id):
    """After one eager call each, advance_traced() and play(trace=) are captured into one graph and replayed twice with the tape overwritten between the
    replays; each replay's traces against a twin that makes the same calls eagerly."""
    import torch

    rec = recording(env_id)
    tape = device_tape(env_id, rec["tape"])
    env, twin = handles(env_id, 2)
    steps = 16
    ro_a, ro_p, tw_a, tw_p = env.new_rollout(steps, labels=True), env.new_rollout(steps), twin.new_rollout(steps, labels=True), twin.new_rollout(steps)
    T = tape[:steps].clone()
    for e, a, p in ((env, ro_a, ro_p), (twin, tw_a, tw_p)):
        e.advance_traced(a, eps=EPS, seed=HASH_SEED, step=0, render=False)
        e.play(tape[:steps], trace=p, render=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.advance_traced(ro_a, eps=EPS, seed=HASH_SEED, step=100, render=False)
        env.play(T, trace=ro_p, render=False)
    for r in range(2):
        T.copy_(tape[steps * (r + 1):steps * (r + 2)])
        for t in (ro_a.frames, ro_a.actions, ro_a.labels, ro_p.frames, ro_p.reward):
            t.zero_()
        graph.replay()
        twin.advance_traced(tw_a, eps=EPS, seed=HASH_SEED, step=100, render=False)
        twin.play(T.clone(), trace=tw_p, render=False)
        torch.cuda.synchronize()
        for k in ("frames", "actions", "labels", "reward", "done"):
            assert torch.equal(getattr(ro_a, k), getattr(tw_a, k)), "replay %d: advance's trace.%s" % (r, k)
        for k in ("frames", "reward", "done"):
            assert torch.equal(getattr(ro_p, k), getattr(tw_p, k)), "replay %d: play's trace.%s" % (r, k)
        assert bool(ro_a.frames[1:].any()) and bool((ro_a.frames[0] != ro_p.frames[steps]).any())
        same_frames(env.redraw(), twin.redraw(), "%s: redraw() after replay %d" % (env_id, r))
    same_state(env, twin, range(0, N, 9), env_id)
    close(env, twin)


# ---- 10. refusals

def test_refusals():
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native
    from memory_gym_amd.vector import GymnasiumVectorEnv

    env_id, n, steps = "MortarMayhem-Grid-v0", 70, 8
    fresh = memory_gym_amd.make(env_id, num_envs=n, device=0)
    assert _native.LIB.mg_advance_traced(fresh._h, steps, 0.0, 0, 0, None, None, None, fresh._raw_stream()) == -1 and "before the first mg_reset" in _native.last_error()
    fresh.close()
    env, twin, first = handles(env_id, 3, n=n)
    B = env.frame_record_bytes
    tape = torch.zeros((steps, n), dtype=torch.int32, device="cuda")
    good = env.new_rollout(steps, labels=True)

    def variant(**kw):
        ro = memory_gym_amd.RolloutTrace(good.frames, 0, good.actions, good.labels, good.reward, good.done)
        for k, v in kw.items():
            setattr(ro, k, v)
        return ro

    buf = torch.zeros((steps + 1) * n * B + 16, dtype=torch.uint8, device="cuda")
    bad = {"misaligned frames": variant(frames=buf[8:8 + (steps + 1) * n * B].view(steps + 1, n, B)),
           "another K": env.new_rollout(steps - 1), "another N": variant(reward=torch.zeros((steps, n + 1), device="cuda")),
           "frames without row 0": variant(frames=good.frames[1:]), "float64 reward": variant(reward=good.reward.double()),
           "uint8 done": variant(done=good.done.view(torch.uint8)), "int64 actions": variant(actions=good.actions.long()),
           "host tensors": variant(done=good.done.cpu()), "a strided view": variant(reward=torch.zeros((steps, 2 * n), device="cuda")[:, ::2]),
           "no trace": good.frames}
    assert bad["misaligned frames"].frames.data_ptr() % 16 == 8
    for what, ro in bad.items():
        if what != "another K":  # (advance_traced takes K from the trace: a whole trace of another K is legal there, an inconsistent one is not)
            with pytest.raises(ValueError):
                env.advance_traced(ro, render=False)
        if what != "int64 actions":  # (play does not look at trace.actions)
            with pytest.raises(ValueError):
                env.play(tape, trace=ro, render=False)
    # the C ABI's own refusals, through ctypes
    lib, null, st = _native.LIB, None, env._raw_stream()
    rows = _native.RolloutTraceRows()
    rows.struct_size = 12
    rows.frames_dev = good.frames[1:].data_ptr()
    assert lib.mg_advance_traced(env._h, steps, 0.0, 0, 0, null, None, C.byref(rows), st) == -1 and "struct_size" in _native.last_error()
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 0, null, null, null, None, C.byref(rows), st) == -1 and "struct_size" in _native.last_error()
    rows.struct_size = C.sizeof(_native.RolloutTraceRows)
    rows.frames_dev = good.frames[1:].data_ptr() + 8
    assert lib.mg_advance_traced(env._h, steps, 0.0, 0, 0, null, None, C.byref(rows), st) == -1 and "16-byte aligned" in _native.last_error()
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 0, null, null, null, None, C.byref(rows), st) == -1 and "16-byte aligned" in _native.last_error()
    rows.frames_dev = good.frames[1:].data_ptr()
    rows.actions_dev = good.actions.data_ptr()
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 0, null, null, null, None, C.byref(rows), st) == -1 and "no teacher" in _native.last_error()
    rows.actions_dev, rows.labels_dev = None, good.labels.data_ptr()
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 0, null, null, null, None, C.byref(rows), st) == -1 and "no teacher" in _native.last_error()
    rows.labels_dev = None
    assert lib.mg_advance_traced(env._h, 0, 0.0, 0, 0, null, None, C.byref(rows), st) == -1 and "steps < 1" in _native.last_error()
    assert lib.mg_advance_traced(env._h, steps, 1.5, 0, 0, null, None, C.byref(rows), st) == -1 and "eps" in _native.last_error()
    assert lib.mg_play_traced(env._h, null, steps, 0, null, null, null, None, C.byref(rows), st) == -1 and "tape_dev" in _native.last_error()
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 2, null, null, null, None, C.byref(rows), st) == -1 and "mode" in _native.last_error()
    # capture of a handle's first call
    torch.cuda.synchronize()
    ro_first = first.new_rollout(steps)
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="first call"):
        with torch.cuda.graph(refused):
            first.advance_traced(ro_first, render=False, stats=False)
    torch.cuda.synchronize()
    first.close()
    # nothing was stepped: the handle against a twin that saw none of this
    assert counters(env) == (0, 0, 0, 0, 0)
    a = twin.expert_actions(EPS, HASH_SEED, 0)
    (o1, r1, d1, _, _), (o2, r2, d2, _, _) = env.step(a), twin.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and np.array_equal(env.rng_words(0), twin.rng_words(0))
    # trace == NULL is the untraced sibling
    assert lib.mg_advance_traced(env._h, steps, 0.0, 0, 0, null, None, None, st) == 0 and lib.mg_advance(twin._h, steps, 0.0, 0, 0, null, None, st) == 0
    assert lib.mg_play_traced(env._h, tape.data_ptr(), steps, 0, null, null, null, None, None, st) == 0
    assert lib.mg_play(twin._h, tape.data_ptr(), steps, 0, null, null, null, null, null, None, st) == 0
    assert counters(env) == (0, 0, steps, steps, 0)
    same_frames(env.redraw(), twin.redraw(), "trace == NULL against the untraced calls")
    # a stale layout in draw(), too many records for one draw
    env.advance_traced(good, render=False)
    assert good.draw(env, 1, 2).shape == (1, 84, 84, 3)
    with pytest.raises(ValueError, match="one length"):
        good.draw(env, [1, 2], [0])
    other = good.frame_layout
    env.reset(seed=1, options={"arena_size": 4})  # a rebuild of the geometry: a new frame layout
    assert env.frame_layout() != other
    with pytest.raises(ValueError, match="layout"):
        good.draw(env, [1], [2])
    huge = memory_gym_amd.RolloutTrace(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(1 << 16, 1 << 15, B), env.frame_layout(), None, None, None, None)
    with pytest.raises(ValueError, match="at most"):
        huge.draw(env, [0], [0])
    env.close()
    twin.close()
    # the gymnasium front end passes trace= through
    venv = GymnasiumVectorEnv("MortarMayhemB-Grid-v0", n, device=0, as_numpy=True)
    plain = memory_gym_amd.make("MortarMayhemB-Grid-v0", num_envs=n, device=0)
    venv.reset(seed=4)
    plain.reset(seed=4)
    ro_v, ro_p = venv.new_rollout(steps, labels=True), plain.new_rollout(steps, labels=True)
    _, sv = venv.advance_traced(ro_v, eps=EPS, seed=HASH_SEED, step=0, render=False)
    plain.advance_traced(ro_p, eps=EPS, seed=HASH_SEED, step=0, render=False)
    assert isinstance(sv["episodes"], np.ndarray) and isinstance(ro_v, memory_gym_amd.RolloutTrace)
    for k in ("frames", "actions", "labels", "reward", "done"):
        assert torch.equal(getattr(ro_v, k), getattr(ro_p, k)), k
    ro_v2 = venv.new_rollout(steps)
    venv.play(ro_p.actions.cpu().numpy(), trace=ro_v2, render=False)
    plain.play(ro_p.actions, trace=ro_p, render=False)
    assert torch.equal(ro_v2.frames, ro_p.frames) and bool(ro_p.frames[1:].any())
    venv.close()
    plain.close()
