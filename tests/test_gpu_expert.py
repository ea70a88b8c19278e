"""GPU (-m gpu): the device-side scripted teacher (include/memgym.h mg_expert_actions, VecMemoryGym.expert_actions) against its
definition, the CPU oracle's expert hooks mixed with mgo_batch_expert's counter-based random actions -- every instance, every step.

The figures in FINISHED / REWARD were measured with the oracle ALONE on the CPU (n = 200, seeds 0..199, 400 steps of its own expert
at eps 0, auto-reset): each case asserts at least half of its id's figure, so that a policy that stands still cannot pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, HASH_SEED = 200, 400, 7  # 200 is no multiple of 64: the last wave is partial
# finished episodes of the oracle alone at eps 0 (memory_gym/__init__.py order of the mortar ids)
FINISHED = {"MortarMayhem-Grid-v0": 600, "MortarMayhem-v0": 200, "Endless-MortarMayhem-v0": 0, "MortarMayhemB-Grid-v0": 1000, "MortarMayhemB-v0": 200,
            "MysteryPath-Grid-v0": 5878, "MysteryPath-v0": 2227, "Endless-MysteryPath-v0": 3, "SearingSpotlights-v0": 2678,
            "Endless-SearingSpotlights-v0": 809}
# the two ids whose episodes do not end under competent play: reward per instance instead (measured 1.5 and 10.0)
REWARD = {"Endless-MortarMayhem-v0": 1.0, "Endless-MysteryPath-v0": 5.0}
CHORDED = {"MysteryPath-Grid-v0": 40, "MysteryPath-v0": 25}  # chorded paths in that run (measured 118 and 56)
EPS = (0.0, 0.1)


def _full(env_id, opts):
    from memory_gym_amd.reset_params import process_reset_params
    return process_reset_params(env_id, opts)


def has_chord(path):
    """path: the oracle's get_list("path"), x0 y0 x1 y1 ... (end first).  A chord: two cells adjacent in the grid that are not
    consecutive in the list (the reference's `neighbor.g = g` typo lets A* return such paths) -- the cell mask alone does not give the order."""
    p = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    d = np.abs(p[:, None, :] - p[None, :, :]).sum(-1)
    k = np.arange(len(p))
    return bool(((d == 1) & (np.abs(k[:, None] - k[None, :]) > 1)).any())


def count_chorded(ref, which):
    return sum(has_chord(ref.envs[int(i)].get_list("path")) for i in which)


def same_actions(env, ref, t, what="", eps_list=EPS):
    """the device's expert actions equal the oracle's in the current states, for every eps of the list; -> {eps: the oracle's actions}"""
    out = {}
    for eps in eps_list:
        want = ref.expert_actions(eps, HASH_SEED, t)
        got = env.expert_actions(eps, HASH_SEED, t).cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
            raise AssertionError("%sstep %d, eps %g: %d instances differ, first %d: device %s, oracle %s"
                                 % (what, t, eps, len(bad), bad[0], got[bad[0]], want[bad[0]]))
        out[eps] = want
    return out


def lock_step(env, ref, steps, play_eps, chords=False, what="", eps_list=EPS):
    """`steps` steps of both sides under the oracle's actions at play_eps, the expert actions compared at every step for every eps ->
    (finished episodes, summed reward, chorded paths among all episodes begun)"""
    n = ref.n
    finished, reward, chorded = 0, 0.0, count_chorded(ref, range(n)) if chords else 0
    for t in range(steps):
        a = same_actions(env, ref, t, what, eps_list)[play_eps]
        _, rew, done, _, _ = env.step(a)
        _, r2, d2 = ref.step(a, autoreset=True, want_obs=False)
        d2 = d2.astype(bool)
        assert np.array_equal(done.cpu().numpy(), d2), "%sdone differs at step %d" % (what, t)
        assert np.array_equal(env.reward64.cpu().numpy(), r2), "%sreward differs at step %d" % (what, t)
        finished += int(d2.sum())
        reward += float(r2.sum())
        if chords and d2.any():
            chorded += count_chorded(ref, np.nonzero(d2)[0])
    same_actions(env, ref, steps, what, eps_list)
    return finished, reward, chorded


@pytest.mark.parametrize("play_eps", [0.0, 0.3], ids=["play_eps0", "play_eps0.3"])
@pytest.mark.parametrize("env_id", sorted(FINISHED))
def test_expert_equals_the_oracle_in_lock_step(env_id, play_eps):
    """All ten ids, n = 200, 400 steps.  play_eps 0: both sides play the expert itself, the run the figures above were measured on (and the
    chorded paths of the two finite Mystery Path ids are counted); play_eps 0.3 (200 steps): they play the oracle's policy with 30 % random
    actions, which takes the instances where the expert alone never goes -- off the path, into failed commands, away from the coin."""
    import memory_gym_amd
    import oracle_lib

    seeds = np.arange(N, dtype=np.int64)
    env = memory_gym_amd.make(env_id, num_envs=N, device=0)
    ref = oracle_lib.OracleBatch(env_id, N)
    env.reset(seed=seeds)
    ref.reset(seeds)
    finished, reward, chorded = lock_step(env, ref, STEPS if not play_eps else STEPS // 2, play_eps, chords=env_id in CHORDED and not play_eps,
                                          eps_list=EPS if not play_eps else (0.0, play_eps))
    print("%s play_eps %g: %d finished episodes, reward per instance %.3f, %d chorded paths" % (env_id, play_eps, finished, reward / N, chorded))
    if not play_eps:
        if env_id in REWARD:
            assert reward / N >= REWARD[env_id], (reward / N, REWARD[env_id])
        else:
            assert 2 * finished >= FINISHED[env_id], (finished, FINISHED[env_id])
        if env_id in CHORDED:
            assert chorded >= CHORDED[env_id], (chorded, CHORDED[env_id])
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words())
    env.check_errors()
    env.close()
    ref.close()


@pytest.mark.parametrize("env_id", sorted(CHORDED))
def test_mass_resets_through_the_lane_generator(env_id):
    """n = 2,048 with max_steps = 12: the whole batch is truncated in one step, every 12 steps -- queues of up to 2,048 (Grid) and 1,474
    entries, above PATH_MASS, so the raster launch's helpers generate the paths one per LANE (lane_path) and store their order from there."""
    import memory_gym_amd
    import oracle_lib

    n, opts = 2048, dict(max_steps=12)
    seeds = np.arange(n, dtype=np.int64)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref = oracle_lib.OracleBatch(env_id, n, options=_full(env_id, opts))
    env.reset(seed=seeds, options=opts)
    ref.reset(seeds)
    finished, _, chorded = lock_step(env, ref, 60, 0.0, chords=True)
    print("%s: %d finished episodes, %d chorded paths" % (env_id, finished, chorded))
    assert finished >= 5 * n * 7 // 10  # five truncations of (nearly) everybody
    assert chorded >= 150, chorded  # measured 227 on either id
    env.check_errors()
    env.close()
    ref.close()


def test_two_option_sets_in_one_handle():
    """SearingSpotlights-v0, the halves under option sets that differ in use_exit / num_coins: each half against its own oracle batch.  (The
    oracle's random actions are numbered by the instance's index in ITS batch: eps 0.1 is compared on the first half, whose indices agree.)"""
    import memory_gym_amd
    import oracle_lib
    import torch

    env_id, n = "SearingSpotlights-v0", 256
    half = n // 2
    opt_a, opt_b = dict(num_coins=[3], use_exit=True), dict(num_coins=[1, 2], use_exit=False, max_steps=90)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref_a = oracle_lib.OracleBatch(env_id, half, options=_full(env_id, opt_a))
    ref_b = oracle_lib.OracleBatch(env_id, half, options=_full(env_id, opt_b))
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds)  # every instance gets an exit first: use_exit = False keeps drawing the earlier one
    ref_b.set_options(_full(env_id, dict()))
    ref_b.reset(seeds[half:])
    ref_b.set_options(_full(env_id, opt_b))
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    ref_a.reset(seeds[:half])
    ref_b.reset(seeds[half:])
    finished = [0, 0]
    for t in range(200):
        got0 = env.expert_actions(0.0, HASH_SEED, t).cpu().numpy()
        got1 = env.expert_actions(0.1, HASH_SEED, t).cpu().numpy()
        assert np.array_equal(got0[:half], ref_a.expert_actions(0.0, HASH_SEED, t)), "first half, eps 0, step %d" % t
        assert np.array_equal(got0[half:], ref_b.expert_actions(0.0, HASH_SEED, t)), "second half, eps 0, step %d" % t
        assert np.array_equal(got1[:half], ref_a.expert_actions(0.1, HASH_SEED, t)), "first half, eps 0.1, step %d" % t
        _, rew, done, _, _ = env.step(got1)
        for k, (ref, sl) in enumerate(((ref_a, slice(0, half)), (ref_b, slice(half, n)))):
            _, r2, d2 = ref.step(got1[sl], autoreset=True, want_obs=False)
            assert np.array_equal(done[sl].cpu().numpy(), d2.astype(bool)) and np.array_equal(env.reward64[sl].cpu().numpy(), r2), "half %d, step %d" % (k, t)
            finished[k] += int(d2.sum())
    assert min(finished) >= half, finished  # both halves play: at least an episode per instance
    env.check_errors()
    env.close()


def test_checkpoint_carries_the_path_order():
    """MysteryPath-v0: state_dict() mid-episode into a FRESH handle; the expert actions of the next 20 steps equal the first handle's and
    the oracle's (the order of a path cannot be rebuilt from the restored cell mask)."""
    import memory_gym_amd
    import oracle_lib
    import torch

    env_id, n = "MysteryPath-v0", 200
    seeds = np.arange(n, dtype=np.int64)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref = oracle_lib.OracleBatch(env_id, n)
    env.reset(seed=seeds)
    ref.reset(seeds)
    lock_step(env, ref, 30, 0.1)
    assert count_chorded(ref, range(n)) >= 1, "no chorded path among the episodes under way: the test would not see a rebuilt order"
    other = memory_gym_amd.make(env_id, num_envs=n, device=0)
    other.load_state_dict(env.state_dict())
    for t in range(30, 50):
        want = same_actions(env, ref, t)
        for eps in EPS:
            assert np.array_equal(other.expert_actions(eps, HASH_SEED, t).cpu().numpy(), want[eps]), "restored handle, step %d, eps %g" % (t, eps)
        a = want[0.1]
        o1, _, d1, _, _ = env.step(a)
        o2, _, d2, _, _ = other.step(a)
        ref.step(a, autoreset=True, want_obs=False)
        assert torch.equal(o1, o2) and torch.equal(d1, d2), "step %d after the restore" % t
    env.close()
    other.close()
    ref.close()


def test_expert_and_step_replay_from_a_graph():
    """MortarMayhem-v0: three (expert, step) pairs captured into one graph -- eps, seed and step are baked into the captured launches --
    replayed from the snapshot, against the same pairs run eagerly."""
    import memory_gym_amd
    import torch
    from chw_referee import clones

    env_id, n, k = "MortarMayhem-v0", 200, 3
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    env.reset(seed=np.arange(n, dtype=np.int64))
    for t in range(9):  # past the display phase of the first commands: the expert moves
        env.step(env.expert_actions(0.1, HASH_SEED, t))
    snap = env.state_dict()
    want = []
    for j in range(k):
        a = env.expert_actions(0.1, HASH_SEED, 100 + j)
        want.append((a.clone(),) + clones(env.step(a)))
    assert any(bool(w[0].any()) for w in want), "the expert stands still in every captured step"
    env.load_state_dict(snap)
    bufs = [torch.zeros_like(want[0][0]) for _ in range(k)]

    def pair(j):
        return clones(env.step(env.expert_actions(0.1, HASH_SEED, 100 + j, out=bufs[j])))

    side = torch.cuda.Stream()  # torch's recipe: a warm-up on a side stream, back to the snapshot, capture, back to the snapshot, replay
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [pair(j) for j in range(k)]
    env.load_state_dict(snap)
    for b in bufs:
        b.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for j in range(k):
        assert torch.equal(bufs[j], want[j][0]), "captured expert actions, pair %d" % j
        for x, y in zip(outs[j], want[j][1:]):
            assert torch.equal(x, y), "captured step, pair %d" % j
    env.check_errors()
    env.close()


@pytest.mark.parametrize("env_id", ["Endless-MortarMayhem-v0", "Endless-MysteryPath-v0", "MysteryPath-Grid-v0", "SearingSpotlights-v0"])
def test_calling_the_expert_changes_nothing(env_id):
    """Three handles run the same 64 steps: one never asks the expert, one asks once per step, one twice.  Frames, rewards, dones and the
    RNG words are equal -- the call draws from no instance's stream and changes no state (Endless-MysteryPath: owed segments stay owed)."""
    import memory_gym_amd
    import torch

    n = 128
    seeds = np.arange(n, dtype=np.int64) + 40
    envs = [memory_gym_amd.make(env_id, num_envs=n, device=0) for _ in range(3)]
    for e in envs:
        e.reset(seed=seeds)
    vis = (lambda o: o["visual_observation"] if isinstance(o, dict) else o)
    for t in range(64):
        a = envs[1].expert_actions(0.1, HASH_SEED, t)
        b = envs[2].expert_actions(0.1, HASH_SEED, t)
        c = envs[2].expert_actions(0.1, HASH_SEED, t)
        assert torch.equal(a, b) and torch.equal(b, c), "step %d" % t
        outs = [e.step(a) for e in envs]
        for o in outs[1:]:
            assert torch.equal(vis(o[0]), vis(outs[0][0])) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2]), "step %d" % t
    for i in (0, n // 2, n - 1):
        w = [e.rng_words(i) for e in envs]
        assert np.array_equal(w[0], w[1]) and np.array_equal(w[0], w[2])
    for e in envs:
        e.check_errors()
        e.close()


def test_python_surface():
    """step=None counts the handle's calls; `out` is written in place and checked; the gymnasium-style vector env and the single-instance
    env pass the call through."""
    import memory_gym_amd
    import torch
    from memory_gym_amd.vec_env import MemoryGymEnv
    from memory_gym_amd.vector import GymnasiumVectorEnv

    env = memory_gym_amd.make("MortarMayhem-v0", num_envs=70, device=0)
    with pytest.raises(RuntimeError, match="before the first mg_reset"):
        env.expert_actions()
    env.reset(seed=1)
    a0, a1 = env.expert_actions(0.5, 3), env.expert_actions(0.5, 3)
    assert a0.dtype == torch.int32 and tuple(a0.shape) == (70, 2)
    assert torch.equal(a0, env.expert_actions(0.5, 3, step=0)) and torch.equal(a1, env.expert_actions(0.5, 3, step=1)) and not torch.equal(a0, a1)
    out = torch.full((70, 2), -1, dtype=torch.int32, device="cuda")
    assert env.expert_actions(0.5, 3, step=1, out=out) is out and torch.equal(out, a1)
    with pytest.raises(ValueError):
        env.expert_actions(out=torch.zeros(70, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="eps"):
        env.expert_actions(eps=1.5)
    env.close()
    venv = GymnasiumVectorEnv("MysteryPath-Grid-v0", 5, device=0, as_numpy=True)
    venv.reset(seed=2)
    a = venv.expert_actions()
    assert isinstance(a, np.ndarray) and a.shape == (5,) and a.dtype == np.int32
    venv.step(a)
    venv.close()
    one = MemoryGymEnv("SearingSpotlights-v0", device=0)
    one.reset(seed=3)
    a = one.expert_action()
    assert a.shape == (2,)
    one.step(a)
    one.close()
    one = MemoryGymEnv("Endless-MysteryPath-v0", device=0)
    one.reset(seed=3)
    assert isinstance(one.expert_action(), int)
    one.close()
