"""GPU (-m gpu): stepping a subset of a handle's instances -- mg_step_masked, VecMemoryGym.step(mask=...) -- all ten env ids.

DEFINITION under test: take the subsequence of calls in which instance i was active; its results are exactly what a handle stepped with plain
step() gives instance i for the same actions in the same order, and an inactive instance keeps everything -- state, stream, descriptor, its rows
of obs / ground truth / episode record -- but reward = 0 and done = 0.  Referees: the CPU oracle stepped one instance at a time (a, c, h) and
twin handles that step everybody (b, c, d, e, f).  Inputs and short-episode options: tests/masked_step_inputs.py -- instance i's k-th ACTIVE step
uses act[k, i].  The episode counts in the docstrings were measured with the oracle ALONE on the CPU with exactly these inputs; every test
asserts its condition so that a run in which nothing ever ends cannot pass."""
import os
import sys

import numpy as np
import pytest

import masked_step_inputs as mi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_IDS = ("MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0")


def vis(o):
    return o["visual_observation"] if isinstance(o, dict) else o


def dev_mask(m):
    import torch
    return torch.as_tensor(np.ascontiguousarray(m), device="cuda")


def make(env_id, n, options=None, **kw):
    """a handle after the seeded reset every test here starts from (seeds arange(n) + 1000, the id's short-episode options unless given)"""
    import memory_gym_amd

    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    env.reset(seed=mi.seeds(n), options=mi.SHORT[env_id] if options is None else options)
    return env


def same_rows(got, want, rows, what):
    """got: a device tensor [n, ...]; want: the frames of `rows` (numpy array or tensor [len(rows), ...])"""
    import torch

    g = vis(got)[torch.as_tensor(rows, device=vis(got).device)].cpu().numpy()
    w = want if isinstance(want, np.ndarray) else vis(want).cpu().numpy()
    if not np.array_equal(g, w):
        bad = np.asarray(rows)[np.nonzero((g != w).reshape(len(w), -1).any(1))[0]]
        raise AssertionError("%s: frames of %d instances differ, first %s" % (what, len(bad), bad[:8]))


def check_against_oracle(env, ref, t, out, r2, d2, i2, what):
    """reward64 / done of the call for everybody (the oracle's for active instances, 0 for the others) and the episode record where done"""
    _, _, done, _, info = out
    assert np.array_equal(done.cpu().numpy(), d2), "%s: done differs at step %d" % (what, t)
    assert np.array_equal(env.reward64.cpu().numpy(), r2), "%s: reward64 differs at step %d" % (what, t)
    assert np.array_equal(out[1].cpu().numpy(), r2.astype(np.float32)), "%s: reward differs at step %d" % (what, t)
    if d2.any():
        assert np.array_equal(info["reward"].cpu().numpy()[d2], i2["reward"][d2]), "%s: info['reward'] differs at step %d" % (what, t)
        assert np.array_equal(info["length"].cpu().numpy()[d2], i2["length"][d2].astype(np.int32)), "%s: info['length'] differs at step %d" % (what, t)
        for nm in env.info_names:
            assert np.array_equal(info[nm].cpu().numpy()[d2], i2[nm][d2].astype(np.float32)), "%s: info[%r] differs at step %d" % (what, nm, t)


# ---- (a) against the oracle

@pytest.mark.parametrize("env_id", mi.ALL_IDS)
def test_masked_steps_equal_the_oracle(env_id):
    """N = 1,100 (no multiple of 16, 64 or 256: the last 16-lane group, wave and workgroup are partial), T = 96, a Bernoulli(1/2) mask per step.
    Every step: done / reward64 / the episode record against the oracle, the active rows of obs equal the oracle's screens, the inactive rows what
    they held.  After steps 0, 47 and 95: redraw() on all 1,100, RNG words, error bits.  Oracle alone: every instance finishes at least two
    episodes (10,909 / 7,242 / 8,493 / 14,070 / 8,606 on the mortar ids, 3,882 / 3,882 / 4,068 on MysteryPath-v0 / -Grid / Endless, 3,883 / 3,882 on the
    spotlight ids), 32-63 active steps per instance."""
    import torch

    N, T = 1100, 96
    env = make(env_id, N)
    ref = mi.MaskedOracle(env_id, N, mi.SHORT[env_id], env.info_names)
    mask, act = mi.bernoulli_inputs(env.action_dim == 1, T, N)
    same_rows(env.obs, ref.frames(range(N)), np.arange(N), env_id + ": reset frames")
    counts = np.zeros(N, np.int64)
    for t in range(T):
        m = mask[t]
        a = mi.pick(act, counts)
        before = vis(env.obs).clone()
        out = env.step(a, mask=dev_mask(m))
        r2, d2, i2 = ref.step(a, m)
        check_against_oracle(env, ref, t, out, r2, d2, i2, env_id)
        on, off = np.nonzero(m)[0], np.nonzero(~m)[0]
        same_rows(out[0], ref.frames(on), on, "%s: active rows at step %d" % (env_id, t))
        off_t = torch.as_tensor(off, device="cuda")
        assert torch.equal(vis(out[0])[off_t], before[off_t]), "%s: an inactive row of obs was written at step %d" % (env_id, t)
        counts += m
        if t in (0, 47, 95):
            same_rows(env.redraw(), ref.frames(range(N)), np.arange(N), "%s: redraw() after step %d" % (env_id, t))
            for i in (0, 1, N - 1, int(off[len(off) // 2])):
                assert np.array_equal(env.rng_words(i), ref.rng_words(i)), "%s: RNG words of instance %d after step %d" % (env_id, i, t)
            env.check_errors()
    assert env.debug_counter("masked_steps") == T
    print("%s: %d episodes, at least %d per instance, %d-%d active steps" % (env_id, ref.episodes.sum(), ref.episodes.min(), counts.min(), counts.max()))
    assert ref.episodes.min() >= 2, ref.episodes.min()
    env.close()
    ref.close()


# ---- (b) twin handles, digests on the device

def twin_record(env_id, n, act, steps):
    """handle B steps everybody with act[k], k = 0 .. steps-1 -> per step reward64, done, the frame digest and the episode record, [steps, n] each"""
    import frame_digest as fd
    import torch

    B = make(env_id, n)
    rec = {"first": fd.digest_torch(vis(B.obs)), "reward": [], "done": [], "digest": [], "info": {k: [] for k in ("reward", "length") + tuple(B.info_names)}}
    for k in range(steps):
        obs, _, done, _, info = B.step(act[k])
        rec["reward"].append(B.reward64.clone())
        rec["done"].append(done.clone())
        rec["digest"].append(fd.digest_torch(vis(obs)))
        for nm in rec["info"]:
            rec["info"][nm].append(info[nm].clone())
    B.check_errors()
    B.close()
    for key in ("reward", "done", "digest"):
        rec[key] = torch.stack(rec[key])
    rec["info"] = {nm: torch.stack(v) for nm, v in rec["info"].items()}
    return rec


@pytest.mark.parametrize("masks", ["blocks", "sparse"])
@pytest.mark.parametrize("env_id", mi.ALL_IDS)
def test_masked_steps_equal_a_twin_that_steps_everybody(env_id, masks):
    """N = 4,160 (65 waves), T = 160.  For every active (t, i) handle A's reward64, done, frame digest and episode record equal handle B's at
    (count_i, i); inactive rows of A's obs keep their digest.  blocks: whole waves and whole 16-lane groups go silent beside partial ones at the seam
    -- oracle alone: every instance is active 80 times and finishes >= 1 episode (24,960 episodes on the ids with max_steps 12).  sparse: one instance in
    eight, rows 5 and 6 all False, rows 50 and 51 all True -- oracle alone: 9-39 active steps per instance, 4,118-4,160 of the 4,160 instances
    finish >= 1 episode depending on the id; at rows 5 and 6 nothing moves."""
    import frame_digest as fd
    import torch

    N, T = 4160, 160
    mask = mi.block_masks(T, N) if masks == "blocks" else mi.sparse_masks(T, N)
    total = mask.sum(0)
    A = make(env_id, N)
    act = mi.actions(np.random.default_rng(7), A.action_dim == 1, T, N)
    rec = twin_record(env_id, N, act, int(total.max()))
    what = "%s, %s" % (env_id, masks)
    digest = fd.digest_torch(vis(A.obs))
    assert torch.equal(digest, rec["first"]), what + ": reset frames"
    counts = torch.zeros(N, dtype=torch.int64, device="cuda")
    cols = torch.arange(N, device="cuda")
    episodes = torch.zeros(N, dtype=torch.int64, device="cuda")
    act_t = torch.as_tensor(act, device="cuda")
    words = None
    for t in range(T):
        m = dev_mask(mask[t])
        if masks == "sparse" and t == 5:
            words = [A.rng_words(i) for i in (0, N // 2, N - 1)]
        obs, reward, done, _, info = A.step(act_t[counts.clamp(max=T - 1), cols].contiguous(), mask=m)
        now = fd.digest_torch(vis(obs))
        k = counts.clamp(max=rec["reward"].shape[0] - 1)
        want = lambda x: x[k, cols]
        assert torch.equal(A.reward64[m], want(rec["reward"])[m]) and torch.equal(done[m], want(rec["done"])[m]), "%s: reward / done of active instances at step %d" % (what, t)
        assert not bool(A.reward64[~m].any()) and not bool(done[~m].any()) and not bool(reward[~m].any()), "%s: reward / done of inactive instances at step %d" % (what, t)
        assert torch.equal(now[m], want(rec["digest"])[m]), "%s: frames of active instances at step %d" % (what, t)
        assert torch.equal(now[~m], digest[~m]), "%s: an inactive row of obs changed at step %d" % (what, t)
        for nm, rows in rec["info"].items():
            assert torch.equal(info[nm][done], want(rows)[done]), "%s: info[%r] at step %d" % (what, nm, t)
        if masks == "sparse" and t in (5, 6):
            assert not bool(reward.any()) and not bool(done.any()) and torch.equal(now, digest), "%s: something moved under an all-zero mask (step %d)" % (what, t)
        digest = now
        counts += m.to(torch.int64)
        episodes += done.to(torch.int64)
        if masks == "sparse" and t == 6:
            for w, i in zip(words, (0, N // 2, N - 1)):
                assert np.array_equal(A.rng_words(i), w), "%s: the stream of instance %d moved under an all-zero mask" % (what, i)
    assert np.array_equal(counts.cpu().numpy(), total)
    finished = int((episodes >= 1).sum())
    print("%s: %d episodes, %d instances finished one, %d-%d active steps" % (what, int(episodes.sum()), finished, total.min(), total.max()))
    if masks == "blocks":
        assert int(total.min()) == 80 and int(total.max()) == 80 and finished == N, (finished, total.min(), total.max())
    else:
        assert finished >= 4000, finished
    assert A.debug_counter("masked_steps") == T
    A.check_errors()
    A.close()


# ---- (c) the definition at the edges

@pytest.mark.parametrize("env_id", EDGE_IDS)
def test_no_mask_and_a_mask_of_ones_equal_the_plain_step(env_id):
    """N = 200, 40 steps, three handles: step(a), step(a, mask=None) and step(a, mask=ones) give the same frames, rewards, dones, infos and RNG
    words; only the third counts masked steps (it takes the plain arrangement, the other two the handle's own)."""
    import torch

    N, T = 200, 40
    plain, none, ones = (make(env_id, N) for _ in range(3))
    act = mi.actions(np.random.default_rng(7), plain.action_dim == 1, T, N)
    all_on = torch.ones(N, dtype=torch.bool, device="cuda")
    finished = 0
    for t in range(T):
        o = [plain.step(act[t]), none.step(act[t], mask=None), ones.step(act[t], mask=all_on)]
        for k, e in ((1, none), (2, ones)):
            what = "%s, handle %d, step %d" % (env_id, k, t)
            assert torch.equal(vis(o[k][0]), vis(o[0][0])), what + ": frames"
            assert torch.equal(o[k][1], o[0][1]) and torch.equal(o[k][2], o[0][2]) and torch.equal(e.reward64, plain.reward64), what + ": reward / done"
            d = o[0][2]
            for nm in ("reward", "length") + tuple(plain.info_names):
                assert torch.equal(o[k][4][nm][d], o[0][4][nm][d]), what + ": info[%r]" % nm
            if plain.gt_dim:
                assert torch.equal(o[k][4]["ground_truth"], o[0][4]["ground_truth"]), what + ": ground truth"
        finished += int(o[0][2].sum())
    assert finished >= N, finished
    for i in (0, N // 2, N - 1):
        assert np.array_equal(none.rng_words(i), plain.rng_words(i)) and np.array_equal(ones.rng_words(i), plain.rng_words(i))
    assert (plain.debug_counter("masked_steps"), none.debug_counter("masked_steps"), ones.debug_counter("masked_steps")) == (0, 0, T)
    for e in (plain, none, ones):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("render", [True, False])
@pytest.mark.parametrize("env_id", EDGE_IDS)
def test_masked_steps_without_autoreset_and_without_frames(env_id, render):
    """N = 200, 40 masked steps with autoreset off against the oracle: a finished instance shows its terminal frame and is re-started by a masked
    reset.  render=False: the masked headless step -- no frame comes back, redraw() after steps 0, 20 and 39 equals the oracle's screens, and
    the calls count as masked and as headless steps."""
    N, T = 200, 40
    env = make(env_id, N)
    env.autoreset = False
    ref = mi.MaskedOracle(env_id, N, mi.SHORT[env_id], env.info_names)
    mask, act = mi.bernoulli_inputs(env.action_dim == 1, T, N)
    counts = np.zeros(N, np.int64)
    what = "%s, render=%s" % (env_id, render)
    for t in range(T):
        m = mask[t]
        a = mi.pick(act, counts)
        out = env.step(a, render=render, mask=dev_mask(m))
        r2, d2, i2 = ref.step(a, m, autoreset=False)
        check_against_oracle(env, ref, t, out, r2, d2, i2, what)
        on = np.nonzero(m)[0]
        if render:
            same_rows(out[0], ref.frames(on), on, "%s: active rows (terminal frames among them) at step %d" % (what, t))
        else:
            assert out[0] is None
            if t in (0, 20, 39):
                same_rows(env.redraw(), ref.frames(range(N)), np.arange(N), "%s: redraw() after step %d" % (what, t))
        if d2.any():
            obs, _ = env.reset(mask=dev_mask(d2))
            for i in np.nonzero(d2)[0]:
                ref.ref.envs[i].reset(None, want_obs=False)
            same_rows(obs, ref.frames(range(N)), np.arange(N), "%s: masked reset after step %d" % (what, t))
        counts += m
    assert ref.episodes.sum() >= N, ref.episodes.sum()
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), ref.rng_words(i))
    assert env.debug_counter("masked_steps") == T and env.debug_counter("headless_steps") == (0 if render else T)
    env.check_errors()
    env.close()
    ref.close()


@pytest.mark.parametrize("env_id", ["Endless-MortarMayhem-v0", "Endless-MysteryPath-v0", "Endless-SearingSpotlights-v0"])
def test_ground_truth_rows_of_inactive_instances_stay(env_id):
    """The three ids with a ground truth, handles with the float64 ground truth and capacity_dev bound (ground_truth64=True,
    on_capacity="truncate"), N = 200, 40 masked steps: the ground-truth rows (float64 and float32) of active instances are a twin's at
    (count_i, i), the rows of inactive ones are not written -- they hold what they held -- and `truncated` is False for them."""
    import torch

    N, T = 200, 40
    A, B = (make(env_id, N, on_capacity="truncate", ground_truth64=True) for _ in range(2))
    mask, act = mi.bernoulli_inputs(A.action_dim == 1, T, N)
    gt64, gt32 = [], []
    for k in range(int(mask.sum(0).max())):
        info = B.step(act[k])[4]
        assert info["ground_truth"].dtype == torch.float64
        gt64.append(info["ground_truth"].clone())
        gt32.append(B.gt.clone())
    gt64, gt32 = torch.stack(gt64), torch.stack(gt32)
    counts = torch.zeros(N, dtype=torch.int64, device="cuda")
    cols = torch.arange(N, device="cuda")
    act_t = torch.as_tensor(act, device="cuda")
    moved = 0
    for t in range(T):
        m = dev_mask(mask[t])
        before64, before32 = A.gt64.clone(), A.gt.clone()
        _, _, _, truncated, info = A.step(act_t[counts.clamp(max=T - 1), cols].contiguous(), mask=m)
        k = counts.clamp(max=gt64.shape[0] - 1)
        assert torch.equal(info["ground_truth"][m], gt64[k, cols][m]) and torch.equal(A.gt[m], gt32[k, cols][m]), "%s: ground truth of active instances at step %d" % (env_id, t)
        assert torch.equal(info["ground_truth"][~m], before64[~m]) and torch.equal(A.gt[~m], before32[~m]), "%s: a ground-truth row of an inactive instance was written at step %d" % (env_id, t)
        assert not bool(truncated[~m].any())
        moved += int((info["ground_truth"][m] != before64[m]).any(1).sum())
        counts += m.to(torch.int64)
    assert moved >= N, moved  # (the ground truth does change under these actions: the comparison above is not one of constants)
    for e in (A, B):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id,opt_a,opt_b", [("SearingSpotlights-v0", dict(num_coins=[3], use_exit=True), dict(num_coins=[1, 2], use_exit=False, max_steps=90)),
                                                ("MortarMayhem-Grid-v0", dict(command_count=[3]), dict(command_count=[8, 10]))])
def test_masked_steps_with_two_option_sets(env_id, opt_a, opt_b):
    """n = 256, the halves under two option sets (the option pairs of tests/test_gpu_headless.py, the handle's per-set kernels), 120 drawn masked
    steps under the device's teacher at eps 0.1: each half against its own oracle batch stepped one active instance at a time.  Oracle alone, under
    its own teacher's numbering of the random actions: 92 / 257 and 156 / 26 episodes end in the two halves; at least 8 per half are asserted."""
    import memory_gym_amd
    import oracle_lib
    import torch

    n, T = 256, 120
    half = n // 2
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    ref_a = oracle_lib.OracleBatch(env_id, half, options=mi.full(env_id, opt_a))
    ref_b = oracle_lib.OracleBatch(env_id, half, options=mi.full(env_id, opt_b))
    seeds = np.arange(n, dtype=np.int64) + 3
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds)  # (SearingSpotlights: every instance gets an exit first -- use_exit = False keeps drawing the earlier one)
    ref_b.set_options(mi.full(env_id, dict()))
    ref_b.reset(seeds[half:])
    ref_b.set_options(mi.full(env_id, opt_b))
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    ref_a.reset(seeds[:half])
    ref_b.reset(seeds[half:])
    refs = [mi.MaskedOracle(env_id, half, None, env.info_names, ref=r) for r in (ref_a, ref_b)]
    mask = np.random.default_rng(7).random((T, n)) < 0.5
    for t in range(T):
        m = mask[t]
        a = env.expert_actions(0.1, 7, t)
        obs, _, done, _, _ = env.step(a, mask=dev_mask(m))
        a = a.cpu().numpy()
        for k, (ref, sl) in enumerate(zip(refs, (slice(0, half), slice(half, n)))):
            r2, d2, _ = ref.step(a[sl], m[sl])
            assert np.array_equal(done[sl].cpu().numpy(), d2) and np.array_equal(env.reward64[sl].cpu().numpy(), r2), "half %d, step %d" % (k, t)
            on = np.nonzero(m[sl])[0]
            same_rows(obs, ref.frames(on), on + sl.start, "%s: active rows of half %d at step %d" % (env_id, k, t))
    assert min(int(r.episodes.sum()) for r in refs) >= 8, [int(r.episodes.sum()) for r in refs]
    same_rows(env.redraw(), np.concatenate([r.frames(range(half)) for r in refs]), np.arange(n), env_id + ": redraw() at the end")
    env.check_errors()
    env.close()
    for r in refs:
        r.close()


@pytest.mark.parametrize("fmt", ["bf16_chw", "f16_chw", "f32_chw", "u8_chw"])
@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY)
def test_masked_steps_in_image_order_formats(env_id, fmt):
    """N = 200, 30 masked steps: every row of the handle's obs, active or not, is at every step what tests/chw_referee.py makes of the uint8 twin's."""
    import chw_referee
    import torch

    N, T = 200, 30
    twin, env = make(env_id, N), make(env_id, N, obs_format=fmt)
    mask, act = mi.bernoulli_inputs(env.action_dim == 1, T, N)
    counts = np.zeros(N, np.int64)
    finished = 0
    for t in range(T):
        m, a = dev_mask(mask[t]), mi.pick(act, counts)
        (o, r, d, _, _), (o2, r2, d2, _, _) = twin.step(a, mask=m), env.step(a, mask=m)
        assert torch.equal(r, r2) and torch.equal(d, d2), "%s %s: step %d" % (env_id, fmt, t)
        assert torch.equal(vis(o2), chw_referee.converted(fmt, vis(o))), "%s %s: frames at step %d" % (env_id, fmt, t)
        counts += mask[t]
        finished += int(d.sum())
    assert finished >= N // 2, finished
    for e in (twin, env):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id", EDGE_IDS)
def test_masked_step_after_headless_steps_leaves_no_old_bytes(env_id):
    """N = 200: 12 headless steps of everybody (obs goes stale), then ONE drawn masked step -- every row of obs is the oracle's current screen, the
    inactive ones included."""
    N = 200
    env = make(env_id, N)
    ref = mi.MaskedOracle(env_id, N, mi.SHORT[env_id], env.info_names)
    mask, act = mi.bernoulli_inputs(env.action_dim == 1, 13, N)
    for t in range(12):
        env.step(act[t], render=False)
        ref.step(act[t], np.ones(N, bool))
    obs = env.step(act[12], mask=dev_mask(mask[12]))[0]
    ref.step(act[12], mask[12])
    same_rows(obs, ref.frames(range(N)), np.arange(N), env_id + ": a masked step after headless steps")
    env.check_errors()
    env.close()
    ref.close()


# ---- (d) terminal observations

@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY)
def test_masked_steps_keep_terminal_observations(env_id):
    """final_observation=True, N = 200, 60 masked steps: the final_observation rows of finished instances are the terminal frames a twin that steps
    everybody keeps at (count_i, i), every other row is untouched, obs and done follow the twin too, and the calls go mg_step's generic way."""
    import torch

    N, T = 200, 60
    A, B = (make(env_id, N, final_observation=True) for _ in range(2))
    mask, act = mi.bernoulli_inputs(A.action_dim == 1, T, N)
    total = mask.sum(0)
    finals, dones, frames = [], [], []
    for k in range(int(total.max())):
        obs, _, done, _, info = B.step(act[k])
        finals.append(info["final_observation"].clone())
        dones.append(done.clone())
        frames.append(vis(obs).clone())
    finals, dones, frames = torch.stack(finals), torch.stack(dones), torch.stack(frames)
    counts = torch.zeros(N, dtype=torch.int64, device="cuda")
    cols = torch.arange(N, device="cuda")
    act_t = torch.as_tensor(act, device="cuda")
    before = A.final_obs.clone()
    finished = 0
    for t in range(T):
        m = dev_mask(mask[t])
        obs, _, done, _, info = A.step(act_t[counts.clamp(max=T - 1), cols].contiguous(), mask=m)
        k = counts.clamp(max=finals.shape[0] - 1)
        assert torch.equal(done[m], dones[k, cols][m]) and not bool(done[~m].any()), "%s: done at step %d" % (env_id, t)
        assert torch.equal(vis(obs)[m], frames[k, cols][m]), "%s: frames of active instances at step %d" % (env_id, t)
        final = info["final_observation"]
        assert torch.equal(final[done], finals[k, cols][done]), "%s: terminal frames at step %d" % (env_id, t)
        assert torch.equal(final[~done], before[~done]), "%s: a final_observation row of an inactive or unfinished instance was written at step %d" % (env_id, t)
        before = final.clone()
        counts += m.to(torch.int64)
        finished += int(done.sum())
    assert finished >= N, finished
    assert A.debug_counter("final_obs_generic_steps") == T and A.debug_counter("masked_steps") == T
    for e in (A, B):
        e.check_errors()
        e.close()


# ---- (e) checkpoint

@pytest.mark.parametrize("env_id", mi.ONE_PER_FAMILY + ("Endless-MysteryPath-v0",))
def test_checkpoint_between_masked_steps(env_id):
    """state_dict() after 30 masked steps, loaded into a fresh handle: both continue 30 masked steps identically -- reward, done, infos, the active
    rows of obs at every step, redraw() and the RNG words at the end (N = 200; every instance is active at least once in the second half, asserted)."""
    import memory_gym_amd
    import torch

    N, T = 200, 60
    A = make(env_id, N)
    mask, act = mi.bernoulli_inputs(A.action_dim == 1, T, N)
    assert mask[30:].any(0).all()
    counts = np.zeros(N, np.int64)
    for t in range(30):
        A.step(mi.pick(act, counts), mask=dev_mask(mask[t]))
        counts += mask[t]
    B = memory_gym_amd.make(env_id, num_envs=N, device=0)
    B.load_state_dict(A.state_dict())
    finished = 0
    for t in range(30, T):
        m, a = dev_mask(mask[t]), mi.pick(act, counts)
        (o, r, d, _, i), (o2, r2, d2, _, i2) = A.step(a, mask=m), B.step(a, mask=m)
        assert torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(A.reward64, B.reward64), "%s: step %d" % (env_id, t)
        assert torch.equal(vis(o)[m], vis(o2)[m]), "%s: frames of active instances at step %d" % (env_id, t)
        for nm in ("reward", "length") + tuple(A.info_names):
            assert torch.equal(i[nm][d], i2[nm][d]), "%s: info[%r] at step %d" % (env_id, nm, t)
        counts += mask[t]
        finished += int(d.sum())
    assert finished >= N // 2, finished
    assert torch.equal(vis(A.redraw()), vis(B.redraw())), env_id + ": redraw() at the end"
    for i in (0, N // 2, N - 1):
        assert np.array_equal(A.rng_words(i), B.rng_words(i))
    for e in (A, B):
        e.check_errors()
        e.close()


# ---- (f) capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0"])
def test_masked_step_replays_from_a_graph(env_id):
    """expert_actions(out=A) + step(A, mask=M) captured once and replayed 20 times, the mask tensor rewritten between the replays, against a twin
    that ran the same 20 masked steps eagerly (the recipe of tests/test_gpu_headless.py: side-stream warm-up, snapshot, capture, replay)."""
    import torch

    N = 200
    twin, env = make(env_id, N), make(env_id, N)
    masks = torch.as_tensor((np.random.default_rng(7).random((20, N)) < 0.5).astype(np.uint8), device="cuda")
    for k in range(20):
        o, r, d, _, _ = twin.step(twin.expert_actions(0.3, 7, 5), mask=masks[k])
    A = torch.zeros((N,) if env.action_dim == 1 else (N, 2), dtype=torch.int32, device="cuda")
    M = torch.ones(N, dtype=torch.uint8, device="cuda")

    def one():
        return env.step(env.expert_actions(0.3, 7, 5, out=A), mask=M)

    snap = env.state_dict()
    first = vis(env.obs).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.load_state_dict(snap)
    vis(env.obs).copy_(first)  # (the warm-up drew everybody: back to the reset frames, which the twin's inactive rows still hold)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o2, r2, d2, _, _ = one()
    env.load_state_dict(snap)
    for k in range(20):
        M.copy_(masks[k])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(r, r2) and torch.equal(d, d2)
    assert torch.equal(vis(o2), vis(o)), env_id + ": obs after 20 replays"
    assert torch.equal(vis(env.redraw()), vis(twin.redraw())), env_id + ": redraw() after 20 replays"
    for i in (0, N - 1):
        assert np.array_equal(env.rng_words(i), twin.rng_words(i))
    for e in (twin, env):
        e.check_errors()
        e.close()


# ---- (g) refusals

def test_refusals():
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    env_id, n = "MortarMayhem-Grid-v0", 70
    step_masked = _native.LIB.mg_step_masked
    env, twin = (memory_gym_amd.VecMemoryGym(env_id, num_envs=n, device=0, final_observation=True) for _ in range(2))
    a = torch.zeros(n, dtype=torch.int32, device="cuda")
    on = torch.ones(n, dtype=torch.uint8, device="cuda")
    # before the first reset
    assert step_masked(env._h, a.data_ptr(), on.data_ptr(), env.obs.data_ptr(), env._p_reward, env._p_done, env._p_gt, env._p_info, 1, env._raw_stream()) == -1
    assert "before the first" in _native.last_error()
    env.reset(seed=1)
    twin.reset(seed=1)
    a = twin.expert_actions(0.3, 7, 0)
    args = [env._h, a.data_ptr(), on.data_ptr(), env.obs.data_ptr(), env._p_reward, env._p_done, env._p_gt, env._p_info, 1, env._raw_stream()]
    for k in (1, 4, 5):  # a NULL actions_dev, reward_dev or done_dev
        bad = list(args)
        bad[k] = None
        assert step_masked(*bad) == -1 and "NULL buffer" in _native.last_error()
    bad = list(args)
    bad[3] = None  # obs_dev NULL together with final_obs_dev
    assert step_masked(*bad) == -1 and "final_obs_dev" in _native.last_error()
    with pytest.raises(ValueError):
        env.step(a, render=False, mask=on)
    for wrong in (torch.ones(n - 1, dtype=torch.bool, device="cuda"), np.ones(n + 1, bool), torch.ones((n, 1), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            env.step(a, mask=wrong)
    assert env.debug_counter("masked_steps") == 0 and env.debug_counter("headless_steps") == 0
    (o1, r1, d1, _, _), (o2, r2, d2, _, _) = env.step(a, mask=on), twin.step(a)  # nothing was stepped
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    env.close()
    twin.close()


# ---- (h) examples/evaluate_seeds.py as a function

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "SearingSpotlights-v0"])
def test_evaluate_seeds_plays_one_episode_per_seed(env_id):
    """64 seeds, default options, the teacher at eps 0.1: per-seed return and length equal the oracle's -- an OracleBatch of 64 under
    expert_actions(0.1, seed, t) each step, of which only the unfinished envs[i] are stepped --, every instance reports exactly one episode and the
    loop ends within max_episode_steps."""
    import memory_gym_amd
    import oracle_lib

    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_seeds

    n, hash_seed = 64, 3
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    res = evaluate_seeds.evaluate(env, mi.seeds(n), eps=0.1, hash_seed=hash_seed)
    ref = oracle_lib.OracleBatch(env_id, n)
    ref.reset(mi.seeds(n))
    ret, length, finished, t = np.zeros(n), np.zeros(n, np.int64), np.zeros(n, bool), 0
    while not finished.all():
        a = ref.expert_actions(0.1, hash_seed, t)
        for i in np.nonzero(~finished)[0]:
            _, r, d = ref.envs[i].step(a[i], want_obs=False)
            ret[i] += r
            length[i] += 1
            finished[i] = d
        t += 1
    assert res["steps"] == t and t <= env.max_episode_steps, (res["steps"], t, env.max_episode_steps)
    assert np.array_equal(res["episodes"].cpu().numpy(), np.ones(n, np.int32))
    assert np.array_equal(res["return"].cpu().numpy(), ret) and np.array_equal(res["length"].cpu().numpy(), length.astype(np.int32))
    assert env.debug_counter("masked_steps") == t and env.debug_counter("headless_steps") == t
    env.close()
    ref.close()
