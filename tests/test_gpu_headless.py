"""GPU (-m gpu): stepping without drawing -- mg_step with obs_dev == NULL (VecMemoryGym.step(render=False), redraw()) and mg_advance
(VecMemoryGym.advance) -- against the CPU oracle and against twin handles that draw every step, all ten env ids.

A headless step must leave everything but the frames as a drawn step leaves it: state, PCG64 streams, reward, done, infos, error bits and
the frame descriptors, so that redraw() gives the frame the last step would have drawn.  mg_advance is checked against its definition,
the loop of expert_actions + headless step.

The figures in FINISHED were measured with the oracle ALONE on the CPU (n = 200, seeds 0..199, 200 steps of its expert at eps 0.3, hash
seed 7, auto-reset): each id asserts at least half of its figure, so that a run in which nothing ever resets cannot pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, HASH_SEED, EPS = 200, 200, 7, 0.3  # 200 is no multiple of 64: the last wave is partial
FINISHED = {"MortarMayhem-Grid-v0": 508, "MortarMayhem-v0": 68, "Endless-MortarMayhem-v0": 99, "MortarMayhemB-Grid-v0": 1450, "MortarMayhemB-v0": 93,
            "MysteryPath-Grid-v0": 1491, "MysteryPath-v0": 605, "Endless-MysteryPath-v0": 42, "SearingSpotlights-v0": 914,
            "Endless-SearingSpotlights-v0": 354}
MORTAR = ("MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0")
REDRAW_AFTER = (0, 49, 50, 99, 100, 149, 199)


def _full(env_id, opts):
    from memory_gym_amd.reset_params import process_reset_params
    return process_reset_params(env_id, opts)


def vis(o):
    return o["visual_observation"] if isinstance(o, dict) else o


def same_frames(got, want, what):
    """got: a device tensor of frames, want: the oracle's uint8 array (or a tensor)"""
    g = vis(got).cpu().numpy()
    w = vis(want).cpu().numpy() if not isinstance(want, np.ndarray) else want
    if not np.array_equal(g, w):
        bad = np.nonzero((g != w).reshape(len(w), -1).any(1))[0]
        raise AssertionError("%s: frames of %d instances differ, first %s" % (what, len(bad), bad[:8]))


def pair(env_id, n, options=None, seed0=0, **kw):
    """a handle and an oracle batch after the same seeded reset"""
    import memory_gym_amd
    import oracle_lib

    seeds = np.arange(n, dtype=np.int64) + seed0
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    ref = oracle_lib.OracleBatch(env_id, n, options=_full(env_id, options) if options else None)
    env.reset(seed=seeds, options=options)
    ref.reset(seeds)
    return env, ref


def same_rng(env, ref, which, what=""):
    for i in which:
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words()), "%sRNG words of instance %d" % (what, i)


# ---- 1. headless against the oracle

@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_headless_steps_equal_the_oracle(env_id):
    """n = 200, 200 headless steps under the oracle's policy at eps 0.3: no observation comes back, reward64 and done equal the oracle's at
    every step, the episode record (reward summed in step order, length) where done; redraw() after steps 0, 49, 50, 99, 100, 149 and 199 equals
    the oracle's screens on all 200 instances."""
    env, ref = pair(env_id, N)
    ep_sum, ep_len, finished = np.zeros(N), np.zeros(N, np.int64), 0
    for t in range(STEPS):
        a = ref.expert_actions(EPS, HASH_SEED, t)
        obs, _, done, _, info = env.step(a, render=False)
        assert obs is None
        o2, r2, d2 = ref.step(a, autoreset=True, want_obs=(t == 0))
        if t == 0:  # the oracle draws its screen on every step, asked for or not
            assert np.array_equal(o2, ref.frames(range(N))), "the oracle's screens are not the frames its step returns"
        d2 = d2.astype(bool)
        assert np.array_equal(done.cpu().numpy(), d2), "done differs at step %d" % t
        assert np.array_equal(env.reward64.cpu().numpy(), r2), "reward differs at step %d" % t
        ep_sum += r2
        ep_len += 1
        if d2.any():
            assert np.array_equal(info["reward"].cpu().numpy()[d2], ep_sum[d2]) and np.array_equal(info["length"].cpu().numpy()[d2], ep_len[d2]), \
                "episode record differs at step %d" % t
            ep_sum[d2], ep_len[d2] = 0.0, 0
            finished += int(d2.sum())
        if t in REDRAW_AFTER:
            same_frames(env.redraw(), ref.frames(range(N)), "%s: redraw() after step %d" % (env_id, t))
    print("%s: %d finished episodes" % (env_id, finished))
    assert 2 * finished >= FINISHED[env_id], (finished, FINISHED[env_id])
    same_rng(env, ref, (0, N - 1))
    env.check_errors()
    assert env.debug_counter("headless_steps") == STEPS
    env.close()
    ref.close()


# ---- 2. headless and drawn steps mixed

@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_headless_and_drawn_steps_mix(env_id):
    """Two handles, the same seeds and actions, 160 steps: A draws every step, B one step in four for the first 80 and every second one after
    that.  B's drawn frames are A's bytes, after B's headless steps B.redraw() is A's obs; reward, done and the infos where done are equal
    at every step; then 40 drawn steps on both.  (Observables only: an Endless-MysteryPath handle may hold other owed records.)"""
    import memory_gym_amd
    import torch

    seeds = np.arange(N, dtype=np.int64) + 11
    A, B = (memory_gym_amd.make(env_id, num_envs=N, device=0) for _ in range(2))
    A.reset(seed=seeds)
    B.reset(seed=seeds)
    headless = 0
    for t in range(200):
        a = A.expert_actions(EPS, HASH_SEED, t)
        draw = t >= 160 or (t % 4 == 0 if t < 80 else t % 2 == 0)
        oa, ra, da, _, ia = A.step(a)
        ob, rb, db, _, ib = B.step(a, render=draw)
        headless += not draw
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(A.reward64, B.reward64), "step %d" % t
        if bool(da.any()):
            for k in ia:
                if k != "done_mask" and k != "ground_truth":
                    assert torch.equal(ia[k][da], ib[k][da]), "info[%r] differs at step %d" % (k, t)
        if A.gt_dim:
            assert torch.equal(ia["ground_truth"], ib["ground_truth"]), "ground truth differs at step %d" % t
        if draw:
            same_frames(ob, oa, "%s: drawn step %d" % (env_id, t))
        else:
            assert ob is None
            same_frames(B.redraw(), oa, "%s: redraw() after headless step %d" % (env_id, t))
        if A.vector_obs is not None:
            assert torch.equal(A.vector_obs, B.vector_obs), "vector observation differs at step %d" % t
    for i in (0, N // 2, N - 1):
        assert np.array_equal(A.rng_words(i), B.rng_words(i))
    assert B.debug_counter("headless_steps") == headless and A.debug_counter("headless_steps") == 0
    for e in (A, B):
        e.check_errors()
        e.close()


# ---- 3. the step that resets everybody

def test_whole_batch_truncation_headless():
    """MysteryPath-Grid-v0, n = 2,048, max_steps = 12: 40 headless steps against the oracle, redraw() after steps 11, 12 and 13 -- the step
    that truncates and resets the whole batch (its paths generated in the step kernel), and its neighbours."""
    n = 2048
    env, ref = pair("MysteryPath-Grid-v0", n, options=dict(max_steps=12))
    finished = 0
    for t in range(40):
        a = ref.expert_actions(EPS, HASH_SEED, t)
        _, _, done, _, _ = env.step(a, render=False)
        _, r2, d2 = ref.step(a, autoreset=True, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), d2.astype(bool)) and np.array_equal(env.reward64.cpu().numpy(), r2), "step %d" % t
        finished += int(d2.sum())
        if t in (11, 12, 13):
            same_frames(env.redraw(), ref.frames(range(n)), "redraw() after step %d" % t)
    assert finished >= 3 * n * 7 // 10, finished  # three truncations of (nearly) everybody
    same_rng(env, ref, (0, n - 1))
    env.check_errors()
    env.close()
    ref.close()


# ---- 4. per-instance option sets

@pytest.mark.parametrize("env_id,opt_a,opt_b", [("SearingSpotlights-v0", dict(num_coins=[3], use_exit=True), dict(num_coins=[1, 2], use_exit=False, max_steps=90)),
                                                ("MortarMayhem-Grid-v0", dict(command_count=[3]), dict(command_count=[8, 10]))])
def test_headless_with_two_option_sets(env_id, opt_a, opt_b):
    """n = 256, the halves under two option sets (the handle's per-set kernels), 120 headless steps: each half against its own oracle batch,
    redraw() at the end.  (The actions are the device's teacher at eps 0.1, checked elsewhere: the oracle numbers its random actions by the
    index in ITS batch.)"""
    import memory_gym_amd
    import oracle_lib
    import torch

    n = 256
    half = n // 2
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref_a = oracle_lib.OracleBatch(env_id, half, options=_full(env_id, opt_a))
    ref_b = oracle_lib.OracleBatch(env_id, half, options=_full(env_id, opt_b))
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds)  # (SearingSpotlights: every instance gets an exit first -- use_exit = False keeps drawing the earlier one)
    ref_b.set_options(_full(env_id, dict()))
    ref_b.reset(seeds[half:])
    ref_b.set_options(_full(env_id, opt_b))
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    ref_a.reset(seeds[:half])
    ref_b.reset(seeds[half:])
    finished = [0, 0]
    for t in range(120):
        a = env.expert_actions(0.1, HASH_SEED, t)
        obs, _, done, _, _ = env.step(a, render=False)
        assert obs is None
        a = a.cpu().numpy()
        for k, (ref, sl) in enumerate(((ref_a, slice(0, half)), (ref_b, slice(half, n)))):
            _, r2, d2 = ref.step(a[sl], autoreset=True, want_obs=False)
            assert np.array_equal(done[sl].cpu().numpy(), d2.astype(bool)) and np.array_equal(env.reward64[sl].cpu().numpy(), r2), "half %d, step %d" % (k, t)
            finished[k] += int(d2.sum())
    assert min(finished) >= half // 2, finished
    same_frames(env.redraw(), np.concatenate([ref_a.frames(range(half)), ref_b.frames(range(half))]), "%s: redraw() after 120 headless steps" % env_id)
    env.check_errors()
    env.close()
    ref_a.close()
    ref_b.close()


def test_masked_reset_after_headless_steps_draws_everybody():
    """MortarMayhem-Grid-v0: a masked reset right after headless steps leaves the CURRENT frame in every row -- the new episode's first frame in
    the masked rows, the frame the last headless step would have drawn in the others (VecMemoryGym keeps a flag for "obs is stale")."""
    import torch

    env, ref = pair("MortarMayhem-Grid-v0", N)
    for t in range(20):
        a = ref.expert_actions(EPS, HASH_SEED, t)
        env.step(a, render=False)
        ref.step(a, autoreset=True, want_obs=False)
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[::3] = True
    obs, _ = env.reset(mask=mask)
    for i in range(0, N, 3):
        ref.envs[i].reset(None, want_obs=False)
    same_frames(obs, ref.frames(range(N)), "masked reset after headless steps")
    env.check_errors()
    env.close()
    ref.close()


@pytest.mark.parametrize("env_id", ["Endless-MortarMayhem-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"])
def test_headless_without_autoreset_and_with_the_optional_buffers(env_id):
    """autoreset = 0, capacity_dev (on_capacity="truncate") and gt64_dev (ground_truth64) bound: 80 headless steps against a twin that draws,
    the finished instances re-started by a masked reset after every step -- whose frames, after headless steps, come with everybody's
    current frame."""
    import memory_gym_amd
    import torch

    seeds = np.arange(N, dtype=np.int64) + 21
    twin, env = (memory_gym_amd.make(env_id, num_envs=N, device=0, on_capacity="truncate", ground_truth64=True) for _ in range(2))
    restarted = 0
    for e in (twin, env):
        e.autoreset = False
        e.reset(seed=seeds)
    for t in range(80):
        a = twin.expert_actions(EPS, HASH_SEED, t)
        o, r, d, tr, i = twin.step(a)
        o2, r2, d2, tr2, i2 = env.step(a, render=False)
        assert o2 is None and torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(tr, tr2) and torch.equal(twin.reward64, env.reward64), "step %d" % t
        if twin.gt_dim:
            assert i["ground_truth"].dtype == torch.float64 and torch.equal(i["ground_truth"], i2["ground_truth"]), "ground truth at step %d" % t
        if bool(d.any()):
            mask = d.clone()
            (o, _), (o2, _) = twin.reset(mask=mask), env.reset(mask=mask)
            same_frames(o2, o, "%s: masked reset after headless step %d" % (env_id, t))
            restarted += int(mask.sum())
    assert restarted > 0
    same_frames(env.redraw(), o, "%s: redraw() at the end" % env_id)
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), twin.rng_words(i))
    for e in (twin, env):
        e.check_errors()
        e.close()


# ---- 5. observation formats

@pytest.mark.parametrize("fmt", ["bf16_chw", "u8_chw"])
@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "SearingSpotlights-v0", "MysteryPath-v0", "Endless-MysteryPath-v0"])
def test_headless_in_image_order_formats(env_id, fmt):
    """60 headless steps, then redraw() equals the obs of a twin that drew every step in that format."""
    import memory_gym_amd
    import torch

    seeds = np.arange(N, dtype=np.int64) + 5
    twin, env = (memory_gym_amd.make(env_id, num_envs=N, device=0, obs_format=fmt) for _ in range(2))
    twin.reset(seed=seeds)
    env.reset(seed=seeds)
    for t in range(60):
        a = twin.expert_actions(EPS, HASH_SEED, t)
        o, r, d, _, _ = twin.step(a)
        o2, r2, d2, _, _ = env.step(a, render=False)
        assert o2 is None and torch.equal(r, r2) and torch.equal(d, d2), "step %d" % t
    assert torch.equal(vis(env.redraw()), vis(o)), "%s %s: redraw() after 60 headless steps" % (env_id, fmt)
    for e in (twin, env):
        e.check_errors()
        e.close()


# ---- 6. capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_headless_step_replays_from_a_graph(env_id):
    """expert_actions(out=A) + step(A, render=False) captured once and replayed 20 times, against a twin that ran the same 20 pairs eagerly."""
    import memory_gym_amd
    import torch

    seeds = np.arange(N, dtype=np.int64)
    twin, env = (memory_gym_amd.make(env_id, num_envs=N, device=0) for _ in range(2))
    twin.reset(seed=seeds)
    env.reset(seed=seeds)
    for _ in range(20):
        _, r, d, _, _ = twin.step(twin.expert_actions(EPS, HASH_SEED, 5), render=False)
    A = torch.zeros((N,) if env.action_dim == 1 else (N, 2), dtype=torch.int32, device="cuda")

    def one():
        return env.step(env.expert_actions(EPS, HASH_SEED, 5, out=A), render=False)

    snap = env.state_dict()
    side = torch.cuda.Stream()  # torch's recipe: a warm-up on a side stream, back to the snapshot, capture, replay
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, r2, d2, _, _ = one()
    env.load_state_dict(snap)
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(d, d2)
    same_frames(env.redraw(), twin.redraw(), "%s: redraw() after 20 replays" % env_id)
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), twin.rng_words(i))
    for e in (twin, env):
        e.check_errors()
        e.close()


# ---- 7. refusals

def test_refusals():
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    env_id, n = "MortarMayhem-Grid-v0", 70
    env, twin = (memory_gym_amd.VecMemoryGym(env_id, num_envs=n, device=0, final_observation=True) for _ in range(2))
    env.reset(seed=1)
    twin.reset(seed=1)
    a = twin.expert_actions(EPS, HASH_SEED, 0)
    with pytest.raises(ValueError):
        env.step(a, render=False)
    # the C entry point itself: obs_dev NULL together with final_obs_dev
    assert _native.LIB.mg_step(env._h, a.data_ptr(), None, env._p_reward, env._p_done, env._p_gt, env._p_info, 1, env._raw_stream()) == -1
    assert "final_obs_dev" in _native.last_error()
    (o1, r1, d1, _, _), (o2, r2, d2, _, _) = env.step(a), twin.step(a)  # nothing was stepped
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    assert env.debug_counter("headless_steps") == 0
    with pytest.raises(RuntimeError, match="steps < 1"):
        env.advance(0)
    with pytest.raises(RuntimeError, match="eps"):
        env.advance(3, eps=1.5)
    env.close()
    twin.close()
    fresh = memory_gym_amd.make(env_id, num_envs=n, device=0)
    with pytest.raises(RuntimeError, match="before the first mg_reset"):
        fresh.advance(3)
    fresh.close()


def test_vector_front_end_passes_advance_through():
    """GymnasiumVectorEnv.advance on its final_observation handle: numpy with as_numpy, the Dict observation of MortarMayhemB, step=None
    continuing the numbering of expert_actions(), and a drawn step() afterwards that goes on from the advanced state like a plain handle's."""
    import memory_gym_amd
    from memory_gym_amd.vector import GymnasiumVectorEnv

    env_id, n = "MortarMayhemB-Grid-v0", 70
    venv = GymnasiumVectorEnv(env_id, n, device=0, as_numpy=True)
    plain = memory_gym_amd.make(env_id, num_envs=n, device=0)
    venv.reset(seed=4)
    plain.reset(seed=4)
    obs, st = venv.advance(50, eps=EPS, seed=HASH_SEED)
    o2, s2 = plain.advance(50, eps=EPS, seed=HASH_SEED)
    assert isinstance(obs, dict) and isinstance(obs["visual_observation"], np.ndarray) and isinstance(st["episodes"], np.ndarray)
    assert np.array_equal(obs["visual_observation"], o2["visual_observation"].cpu().numpy())
    assert np.array_equal(obs["vector_observation"], o2["vector_observation"].cpu().numpy())
    assert sorted(st) == sorted(s2) and all(np.array_equal(st[k], s2[k].cpu().numpy()) for k in st) and int(st["episodes"].sum()) > 0
    assert venv.env._expert_calls == 50
    a = venv.expert_actions(EPS, HASH_SEED)  # call number 50
    assert np.array_equal(a, plain.expert_actions(EPS, HASH_SEED, step=50).cpu().numpy())
    o, r, term, trunc, infos = venv.step(a)
    o2, r2, d2, _, _ = plain.step(a)
    assert np.array_equal(o["visual_observation"], o2["visual_observation"].cpu().numpy()) and np.array_equal(term, d2.cpu().numpy())
    assert venv.advance(3, render=False, stats=False) == (None, None)
    venv.close()
    plain.close()


# ---- 8. mg_advance against its definition

PARAMS = ((1, 0.0, 0), (7, 0.3, 0), (64, 0.3, 1000), (200, 1.0, 0))  # (steps, eps, step0)


def oracle_loop(ref, steps, eps, step0):
    """the loop of mg_advance's definition played by the oracle -> (reward summed in step order, episodes ended)"""
    reward, episodes = np.zeros(ref.n), np.zeros(ref.n, np.int32)
    for t in range(steps):
        _, r, d = ref.step(ref.expert_actions(eps, HASH_SEED, step0 + t), autoreset=True, want_obs=False)
        reward += r
        episodes += d.astype(np.int32)
    return reward, episodes


def device_loop(twin, steps, eps, step0):
    """the same loop with device calls -> the stats dictionary advance() returns"""
    import torch

    n, dev = twin.num_envs, twin.device
    st = {"reward": torch.zeros(n, dtype=torch.float64, device=dev), "episodes": torch.zeros(n, dtype=torch.int32, device=dev),
          "episode_reward": torch.zeros(n, dtype=torch.float64, device=dev), "episode_length": torch.zeros(n, dtype=torch.int64, device=dev)}
    for nm in twin.info_names:
        st[nm] = torch.zeros(n, dtype=torch.float64, device=dev)
    for t in range(steps):
        _, _, done, _, info = twin.step(twin.expert_actions(eps, HASH_SEED, step0 + t), render=False)
        st["reward"] += twin.reward64
        st["episodes"] += done.to(torch.int32)
        st["episode_reward"] += torch.where(done, info["reward"], torch.zeros_like(info["reward"]))
        st["episode_length"] += torch.where(done, info["length"], torch.zeros_like(info["length"])).to(torch.int64)
        for nm in twin.info_names:
            st[nm] += torch.where(done, info[nm], torch.zeros_like(info[nm])).double()
    return st


@pytest.mark.parametrize("env_id,n", [(e, N) for e in sorted(FINISHED)] + [(e, 520) for e in MORTAR])
def test_advance_equals_its_definition(env_id, n):
    """advance(steps, eps, seed 7, step0) for four parameter sets in a row, on three handles and an oracle batch after the same reset: the
    oracle plays the loop (reward sums exact, episodes, frames, RNG words), a twin handle runs the loop with device calls (every sum, the ground
    truth), and a third handle takes the 64 steps as 40 + 24.  n = 520: two full workgroups and a partial one of the mortar ids' kernel."""
    import memory_gym_amd
    import torch

    env, ref = pair(env_id, n)
    seeds = np.arange(n, dtype=np.int64)
    twin, split = (memory_gym_amd.make(env_id, num_envs=n, device=0) for _ in range(2))
    twin.reset(seed=seeds)
    split.reset(seed=seeds)
    fused = env_id in MORTAR
    for steps, eps, step0 in PARAMS:
        what = "%s n=%d advance(%d, %g, step0 %d)" % (env_id, n, steps, eps, step0)
        c0 = (env.debug_counter("advance_fused_steps"), env.debug_counter("headless_steps"))
        obs, st = env.advance(steps, eps=eps, seed=HASH_SEED, step=step0)
        c1 = (env.debug_counter("advance_fused_steps"), env.debug_counter("headless_steps"))
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((steps, 0) if fused else (0, steps)), what
        reward, episodes = oracle_loop(ref, steps, eps, step0)
        assert np.array_equal(st["reward"].cpu().numpy(), reward), what + ": reward sums"
        assert np.array_equal(st["episodes"].cpu().numpy(), episodes), what + ": episodes"
        same_frames(obs, ref.frames(range(n)), what)
        same_rng(env, ref, (0, n - 1), what + ": ")
        want = device_loop(twin, steps, eps, step0)
        assert sorted(st) == sorted(want)
        for k in want:
            assert torch.equal(st[k], want[k]), what + ": stats[%r] differs from the loop's" % k
        if env.gt_dim:
            assert torch.equal(env.gt, twin.gt), what + ": ground truth"
        if env.vector_obs is not None:
            assert torch.equal(env.vector_obs, twin.vector_obs), what + ": vector observation"
        if steps != 64:
            split.advance(steps, eps=eps, seed=HASH_SEED, step=step0, render=False, stats=False)
            continue
        _, s1 = split.advance(40, eps=eps, seed=HASH_SEED, step=step0, render=False)
        s1 = {k: v.clone() for k, v in s1.items()}
        o2, s2 = split.advance(24, eps=eps, seed=HASH_SEED, step=step0 + 40)
        same_frames(o2, obs, what + ", as 40 + 24")
        for k in ("episodes", "episode_length"):
            assert torch.equal(s1[k] + s2[k], st[k]), what + ", as 40 + 24: stats[%r]" % k
        for k in st:  # float sums: the two partial sums added once more -- one rounding of a sum of at most 64 terms apart
            assert torch.allclose(s1[k].double() + s2[k].double(), st[k].double(), rtol=0, atol=1e-12), what + ", as 40 + 24: stats[%r]" % k
        if env.gt_dim:
            assert torch.equal(env.gt, split.gt)
        for i in (0, n - 1):
            assert np.array_equal(env.rng_words(i), split.rng_words(i)), what + ", as 40 + 24"
    for i in (0, n - 1):
        assert np.array_equal(env.rng_words(i), split.rng_words(i)) and np.array_equal(env.rng_words(i), twin.rng_words(i))
    for e in (env, twin, split):
        e.check_errors()
        e.close()
    ref.close()


# ---- 9. more steps than one launch takes

def test_advance_beyond_the_per_launch_cap():
    """MortarMayhem-Grid-v0, advance(1500, eps 0.3): two launches of the in-launch form (1,024 + 476 steps), against the oracle."""
    env, ref = pair("MortarMayhem-Grid-v0", N)
    obs, st = env.advance(1500, eps=EPS, seed=HASH_SEED, step=0)
    reward, episodes = oracle_loop(ref, 1500, EPS, 0)
    assert np.array_equal(st["reward"].cpu().numpy(), reward) and np.array_equal(st["episodes"].cpu().numpy(), episodes)
    assert int(episodes.sum()) >= 1500, int(episodes.sum())  # (508 in 200 steps)
    same_frames(obs, ref.frames(range(N)), "advance(1500)")
    same_rng(env, ref, (0, N - 1))
    assert env.debug_counter("advance_fused_steps") == 1500 and env.debug_counter("headless_steps") == 0
    env.check_errors()
    env.close()
    ref.close()


# ---- 10. mg_advance under capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_advance_replays_from_a_graph(env_id):
    """After a first eager call (the one that allocates): advance(8, ..., render=False) captured, replayed three times, against three eager
    calls with the captured arguments on a twin."""
    import memory_gym_amd
    import torch

    seeds = np.arange(N, dtype=np.int64)
    twin, env = (memory_gym_amd.make(env_id, num_envs=N, device=0) for _ in range(2))
    for e in (twin, env):
        e.reset(seed=seeds)
        e.advance(8, eps=EPS, seed=HASH_SEED, step=0, render=False)
    for _ in range(3):
        _, want = twin.advance(8, eps=EPS, seed=HASH_SEED, step=8, render=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obs, st = env.advance(8, eps=EPS, seed=HASH_SEED, step=8, render=False)
    assert obs is None
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(st[k], want[k]), "stats[%r] of the last replay" % k
    same_frames(env.redraw(), twin.redraw(), "%s: redraw() after three replays" % env_id)
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), twin.rng_words(i))
    for e in (twin, env):
        e.check_errors()
        e.close()
