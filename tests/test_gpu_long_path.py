"""GPU (-m gpu): Endless-MysteryPath-v0 far out, in lock-step with the oracle.  The agent's absolute x passes 32,768 px after ~341
segments (a path follower: ~15,500 steps); rounds 1-6 kept it in 16 bits (MysteryCore::ax), so past that point the step kernel read
segment records at a negative index and ended the episode as a fall behind the frontier, with no error bit.  Their fall-off keys held
16 bits of the column (two cells 65,536 columns apart collided; no test walks that far, see FAR).  Every case here makes the segment
store large enough (make(capacity={"path_segments": 512})), walks past 32,768 px and asserts that it got there.

The policy is a path follower that reads the environment's own ground truth (the direction to the next node, as
tools/emp_policy_bench.py does); half of the instances take a seeded random action with probability EPS per step instead, so that some
episodes fall off far out (fall-off list, the return to the start, camera and past-path window from far away)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ENV_ID = "Endless-MysteryPath-v0"
CAP = {"path_segments": 512}
WRAP = 32768      # where a 16-bit x wrapped
NEAR = 300        # frames on every step for an instance whose x lies this close to WRAP
EPS = 1e-4
MIN_STEPS, MAX_STEPS = 15000, 20000
# Half of the followers without random actions must end beyond FAR px.  Not more: a path may step LEFT (A* around walls), and no action
# moves left -- there every agent, the reference's too, falls off or runs out of stamina.  Measured on the oracle: roughly one such dead
# end per 4,700 columns; after 15,000 steps ~2/3 of 256 followers were past 33,000 px, none after 13,000.
FAR = 33000


def _policy(n, eps_mask, seed):
    """follower(gt) -> int32 actions on the device: argmax of the one-hot direction (right / up / down) + 1; an instance of eps_mask
    takes a uniformly random action with probability EPS instead"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    eps = torch.as_tensor(eps_mask, device="cuda") * EPS

    def act(gt):
        a = gt.argmax(1).to(torch.int32) + 1
        r = torch.rand(n, device="cuda", generator=g) < eps
        return torch.where(r, torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32), a)
    return act


def _oracle_gt(ref):
    return np.stack([ref.get_all("gt%d" % k) for k in range(3)], 1)


def _far_enough(ax, eps_mask):
    follow = ax[~eps_mask]
    return (follow > FAR).sum() * 2 >= follow.size


def _check_far(ref, env, eps_mask):
    ax = ref.get_all("ax")
    assert _far_enough(ax, eps_mask), "the followers did not get past %d px: %s" % (FAR, np.sort(ax[~eps_mask]))
    assert env.debug_counter("emp_segments_max") >= 345, env.debug_counter("emp_segments_max")
    return ax


def _lock_step(env, ref, n, eps_mask, convert=None, stop=None):
    """env: a VecMemoryGym; ref: OracleBatch of the same seeds.  Rewards (float64), dones and ground truth on every step; frames every
    50 steps and, on every step, of each instance within NEAR px of WRAP.  Runs until the followers are far out, or until
    stop(oracle x) holds; returns (steps, ground truth, policy) to go on from there."""
    import torch

    act = _policy(n, eps_mask, 5)
    seeds = np.arange(n, dtype=np.int64) + 101
    obs, info = env.reset(seed=seeds)
    want = ref.reset(seeds)
    assert torch.equal(obs.cpu(), convert(want) if convert else torch.from_numpy(want))
    gt = info["ground_truth"]
    ax = ref.get_all("ax")
    buf = np.empty_like(want)
    t = 0
    while True:
        near = np.abs(ax - WRAP) < NEAR
        frames = t % 50 == 0 or near.any()
        a = act(gt)
        obs, rew, done, _, info = env.step(a)
        gt = info["ground_truth"]
        o2, r2, d2 = ref.step(a.cpu().numpy(), autoreset=True, want_obs=frames, out=(buf, np.empty(n), np.empty(n, np.uint8)) if frames else None)
        assert np.array_equal(env.reward64.cpu().numpy(), r2), "rewards, step %d" % t
        assert np.array_equal(done.cpu().numpy(), d2.astype(bool)), "dones, step %d" % t
        assert np.array_equal(gt.cpu().numpy(), _oracle_gt(ref)), "ground truth, step %d" % t
        if frames:
            sel = np.arange(n) if t % 50 == 0 else np.nonzero(near)[0]
            got = obs[torch.as_tensor(sel, device=obs.device)].cpu()
            exp = convert(o2[sel]) if convert else torch.from_numpy(o2[sel])
            assert torch.equal(got, exp), "frames of instances %s, step %d" % (sel[:8], t)
        ax = ref.get_all("ax")
        t += 1
        if stop is not None:
            if stop(ax):
                return t, gt, act
            assert t < MAX_STEPS, "no instance came near %d px" % WRAP
        elif t >= MIN_STEPS and (_far_enough(ax, eps_mask) or t >= MAX_STEPS):
            return t, gt, act


def _rng_parity(env, ref, idx, of=None):
    """generator words of env instance of[j] (default: j) against oracle instance j, for j in idx"""
    for j in idx:
        i = int(j if of is None else of[j])
        assert np.array_equal(env.rng_words(i), ref.envs[int(j)].rng_words()), "generator words of instance %d" % i


def test_a_small_launch_arrangement_past_32768_px():
    """256 instances, uint8 frames: the arrangement of small launches (bg_coop, n <= 20,480)."""
    import memory_gym_amd
    import oracle_lib

    n = 256
    eps_mask = np.arange(n) >= n // 2
    env = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, capacity=CAP)
    ref = oracle_lib.OracleBatch(ENV_ID, n)
    _lock_step(env, ref, n, eps_mask)
    _check_far(ref, env, eps_mask)
    _rng_parity(env, ref, [0, 1, n // 2, n - 1])
    env.check_errors()


def test_c_float_observations_past_32768_px():
    """256 instances, obs_format="bf16_chw": the step kernel and a separate raster launch instead of the fused one."""
    import memory_gym_amd
    import oracle_lib
    import torch

    n = 256
    eps_mask = np.arange(n) >= n // 2
    env = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, capacity=CAP, obs_format="bf16_chw")
    ref = oracle_lib.OracleBatch(ENV_ID, n)

    def convert(u8):  # as tests/test_gpu_obs_format.py: [x][y][c] uint8 -> [c][y][x] / 255
        return torch.from_numpy(u8.transpose(0, 3, 2, 1).astype(np.float32) / np.float32(255)).to(torch.bfloat16)
    _lock_step(env, ref, n, eps_mask, convert=convert)
    _check_far(ref, env, eps_mask)
    _rng_parity(env, ref, [0, n - 1])
    env.check_errors()


def test_b_the_arrangement_at_scale_with_terminal_observations():
    """32,768 instances behind the gymnasium vector front end (final observations): background workgroups, the next episode's first
    segment ahead of time, the FINAL step kernel and the sparse raster of terminal frames.  An oracle subset of 257 instances referees
    (0, n - 1, every 128th): terminal frames of its finished episodes and the first frames of the next ones."""
    import torch
    from memory_gym_amd.vector import GymnasiumVectorEnv
    import oracle_lib

    n = 32768
    idx = np.array(sorted(set(range(0, n, 128)) | {n - 1}))
    m = idx.size
    eps_all = (np.arange(n) // 128) % 2 == 1
    eps_mask = eps_all[idx]
    assert eps_mask.any() and not eps_mask.all()
    idx_t = torch.as_tensor(idx, device="cuda")
    envs = GymnasiumVectorEnv(ENV_ID, n, device=0, capacity=CAP)
    ref = oracle_lib.OracleBatch(ENV_ID, m)
    seeds = np.arange(n, dtype=np.int64) + 7
    obs, info = envs.reset(seed=seeds)
    want = ref.reset(seeds[idx])
    assert np.array_equal(obs[idx_t].cpu().numpy(), want)
    act = _policy(n, eps_all, 9)
    gt = info["ground_truth"]
    buf, rbuf, dbuf = np.empty_like(want), np.empty(m), np.empty(m, np.uint8)
    t, finals = 0, 0
    while True:
        a = act(gt)
        obs, rew, term, trunc, infos = envs.step(a)
        gt = infos["ground_truth"]
        o2, r2, d2 = ref.step(a[idx_t].cpu().numpy(), autoreset=False, out=(buf, rbuf, dbuf))
        done = (term | trunc)[idx_t].cpu().numpy()
        assert np.array_equal(envs.env.reward64[idx_t].cpu().numpy(), r2), "rewards, step %d" % t
        assert np.array_equal(done, d2.astype(bool)), "dones, step %d" % t
        ax = ref.get_all("ax")
        fin = np.nonzero(done)[0]
        if fin.size:  # the terminal frames, then the oracle's resets: the next episodes' first frames and ground truth
            got = infos["final_observation"][idx_t[torch.as_tensor(fin, device="cuda")]].cpu().numpy()
            assert np.array_equal(got, o2[fin]), "terminal frames of %s, step %d" % (idx[fin], t)
            for j in fin:
                o2[j] = ref.envs[j].reset(None)
            finals += fin.size
        assert np.array_equal(gt[idx_t].cpu().numpy(), _oracle_gt(ref)), "ground truth, step %d" % t
        near = np.abs(ax - WRAP) < NEAR
        sel = np.arange(m) if t % 50 == 0 else np.union1d(np.nonzero(near)[0], fin)
        if sel.size:
            got = obs[idx_t[torch.as_tensor(sel, device="cuda")]].cpu().numpy()
            assert np.array_equal(got, o2[sel]), "frames of %s, step %d" % (idx[sel[:8]], t)
        t += 1
        if t >= MIN_STEPS and (_far_enough(ax, eps_mask) or t >= MAX_STEPS):
            break
    assert finals > 0, "no episode of the subset ended: the terminal frames went unchecked"
    _check_far(ref, envs.env, eps_mask)
    _rng_parity(envs.env, ref, [0, 1, m - 1], of=idx)
    envs.env.check_errors()


def test_d_single_instance_past_32768_px():
    """mg_single_* through make(id, capacity=...): one perfect follower, frames on every step."""
    import memory_gym_amd
    import oracle_lib

    e = memory_gym_amd.make(ENV_ID, capacity=CAP)
    assert e.vec.capacity == CAP
    r = oracle_lib.OracleEnv(ENV_ID)
    o, info = e.reset(seed=3)  # (a path without a dead end before 33,200 px: ~14,400 steps)
    assert np.array_equal(o, r.reset(3))
    t = 0
    while r.get("ax") <= FAR + 200 and t < MAX_STEPS:
        a = int(np.argmax(info["ground_truth"])) + 1
        o, rw, d, _, info = e.step(a)
        o2, r2, d2 = r.step([a, 0])
        assert np.array_equal(o, o2) and rw == r2 and d == d2 and not d, "step %d" % t
        assert np.array_equal(info["ground_truth"], r.gt()), "step %d" % t
        t += 1
    assert r.get("ax") > FAR, r.get("ax")
    assert e.vec.debug_counter("emp_segments_max") >= 345
    assert np.array_equal(e.vec.rng_words(0), r.rng_words())
    e.close()


def test_e_checkpoint_across_the_wrap():
    """state_dict() just before the first instance reaches 32,768 px, loaded into a fresh handle of the same capacity: both handles
    run 2,000 steps further, equal to each other and to the oracle.  A blob of state version 7 (16-bit x) is refused."""
    import memory_gym_amd
    import oracle_lib
    import torch

    n = 64
    eps_mask = np.arange(n) >= n // 2
    env = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, capacity=CAP)
    ref = oracle_lib.OracleBatch(ENV_ID, n)
    # up to the step before the first instance comes within 2 * NEAR px of the wrap
    _, gt, act = _lock_step(env, ref, n, eps_mask, stop=lambda ax: ax.max() >= WRAP - 2 * NEAR)
    assert ref.get_all("ax").max() < WRAP
    sd = env.state_dict()
    blob = sd["blob"]
    assert int(np.frombuffer(blob[8:12].tobytes(), np.uint32)[0]) == 8
    other = memory_gym_amd.make(ENV_ID, num_envs=n, device=0, capacity=CAP)
    old = dict(sd, blob=blob.copy())
    old["blob"][8:12] = np.frombuffer(np.uint32(7).tobytes(), np.uint8)
    with pytest.raises(RuntimeError, match="state version 7"):
        other.load_state_dict(old)
    other.load_state_dict(sd)
    buf = np.empty((n, 84, 84, 3), np.uint8)
    for k in range(2000):
        a = act(gt)
        o_a, _, d_a, _, info = env.step(a)
        o_b, _, d_b, _, info_b = other.step(a)
        gt = info["ground_truth"]
        assert torch.equal(o_a, o_b) and torch.equal(d_a, d_b) and torch.equal(env.reward64, other.reward64), "step %d after the load" % k
        assert torch.equal(gt, info_b["ground_truth"]), "step %d after the load" % k
        ax = ref.get_all("ax")
        frames = k % 50 == 0 or (np.abs(ax - WRAP) < NEAR).any()
        o2, r2, d2 = ref.step(a.cpu().numpy(), autoreset=True, want_obs=frames, out=(buf, np.empty(n), np.empty(n, np.uint8)) if frames else None)
        assert np.array_equal(env.reward64.cpu().numpy(), r2) and np.array_equal(d_a.cpu().numpy(), d2.astype(bool)), "step %d after the load" % k
        assert np.array_equal(gt.cpu().numpy(), _oracle_gt(ref)), "ground truth, step %d after the load" % k
        if frames:
            assert np.array_equal(o_a.cpu().numpy(), o2), "frames, step %d after the load" % k
    ax = ref.get_all("ax")
    assert (ax[~eps_mask] > WRAP).sum() * 3 >= (~eps_mask).sum(), "the run after the load did not cross %d px: %s" % (WRAP, np.sort(ax))
    _rng_parity(other, ref, [0, n - 1])
    env.check_errors()
    other.check_errors()
