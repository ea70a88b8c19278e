"""GPU (-m gpu): single instances saved to and loaded from device memory -- mg_save_instances / mg_load_instances (include/memgym.h),
VecMemoryGym.save_instances / load_instances / copy_instances -- against the CPU oracle and against twin handles that never saw a save or a load.

DEFINITION under test: after a load of record r (saved from instance s) into instance d, d gives for the same actions bit for bit what s gave
from the moment of the save; every instance the load does not name keeps everything; a save changes nothing.

Sizes: 200 instances (no multiple of 64), counts 1, 63, 65 and 200.  Actions: the handle's own teacher at eps 0.3 (oracle-equal:
tests/test_gpu_expert.py), copied to the host where the oracle needs them.  OPTIONS makes episodes end inside the windows.  With the oracle ALONE on
the CPU (seeds 300 .. 499, 40 + 30 steps, then 60 steps of the permuted batch) these options gave, per id, instances whose RNG words moved between
the save and the load / episodes that ended in the last window: MortarMayhem-Grid 140 / 206, MortarMayhem 200 / 502, Endless-MortarMayhem 200 / 201,
MortarMayhemB-Grid 145 / 390, MortarMayhemB 172 / 399, MysteryPath-Grid 171 / 473, MysteryPath 165 / 248, Endless-MysteryPath 200 / 599,
SearingSpotlights 152 / 300, Endless-SearingSpotlights 161 / 200 -- at least half of the instances and at least N / 4 episodes everywhere."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, EPS, HASH = 200, 0.3, 7
SHORT_MORTAR = {"command_count": [3], "command_show_duration": [1], "command_show_delay": [1], "explosion_delay": [6], "explosion_duration": [2]}
OPTIONS = {"MortarMayhem-v0": SHORT_MORTAR, "MortarMayhemB-v0": {"command_count": [3], "explosion_delay": [8], "explosion_duration": [3]},
           "MysteryPath-v0": {"max_steps": 60}, "Endless-MysteryPath-v0": {"max_steps": 25}, "Endless-MortarMayhem-v0": {"max_steps": 40},
           "Endless-SearingSpotlights-v0": {"max_steps": 40}}
ALL_IDS = ["MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0", "MysteryPath-Grid-v0",
           "MysteryPath-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0", "Endless-SearingSpotlights-v0"]
PER_ARRANGEMENT = ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0"]
PERM = np.roll(np.arange(N), 7)  # a fixed permutation without fixed points


def _full(env_id, opts):
    from memory_gym_amd.reset_params import process_reset_params
    return process_reset_params(env_id, opts) if opts else None


def vis(o):
    return o["visual_observation"] if isinstance(o, dict) else o


def make(env_id, n=N, seed0=300, options="default", **kw):
    import memory_gym_amd

    options = OPTIONS.get(env_id) if options == "default" else options
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    seeds = np.arange(n, dtype=np.int64) + seed0
    env.reset(seed=seeds, options=options)
    return env, seeds, options


def oracle(env_id, seeds, options):
    import oracle_lib

    ref = oracle_lib.OracleBatch(env_id, len(seeds), options=_full(env_id, options))
    ref.reset(seeds)
    return ref


def teacher(env, t):
    return env.expert_actions(EPS, HASH, step=t)


def digests(obs):
    import frame_digest as fd
    return fd.digest_torch(vis(obs)).cpu().numpy().view(np.uint64)


def same_rows(got, want, what):
    import torch

    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).reshape(got.shape[0], -1).any(1)).flatten().cpu().numpy()
        raise AssertionError("%s: %d rows differ, first %s" % (what, len(bad), bad[:8]))


def lock_step_with_twin(env, twin, steps, perm=None, t0=1000, rows=None, final=False, what=""):
    """`steps` steps: the twin plays its teacher's actions, env the same actions (row i of env takes row perm[i] of the twin); frames, reward64, done, the
    ground truth and the episode records where done must be equal on `rows` (default: all).  -> episodes that ended"""
    import torch

    p = torch.arange(env.num_envs, device="cuda") if perm is None else torch.as_tensor(perm, device="cuda")
    r = torch.arange(env.num_envs, device="cuda") if rows is None else torch.as_tensor(rows, device="cuda")
    ended = 0
    for t in range(steps):
        a = teacher(twin, t0 + t)
        o2, _, d2, _, i2 = twin.step(a)
        o1, _, d1, _, i1 = env.step(a[p].contiguous())
        w = "%s step %d" % (what, t)
        same_rows(vis(o1)[r], vis(o2)[p][r], w + " frames")
        assert torch.equal(env.reward64[r], twin.reward64[p][r]) and torch.equal(d1[r], d2[p][r]), w + " reward / done"
        if env.gt_dim:
            assert torch.equal(env.gt[r], twin.gt[p][r]), w + " ground truth"
        if env.vector_obs is not None:
            assert torch.equal(env.vector_obs[r], twin.vector_obs[p][r]), w + " vector observation"
        m = d1[r]
        if bool(m.any()):
            for k in ("reward", "length") + tuple(env.info_names):
                assert torch.equal(i1[k][r][m], i2[k][p][r][m]), w + " info " + k
            if final:
                same_rows(i1["final_observation"][r][m], i2["final_observation"][p][r][m], w + " terminal frames")
        ended += int(m.sum())
    return ended


def same_rng(env, twin, pairs, what=""):
    for i, j in pairs:
        assert np.array_equal(env.rng_words(int(i)), twin.rng_words(int(j))), "%s RNG words of instance %d" % (what, i)


def detour(env, steps, t0=5000):
    """steps the twin does not take: other actions (another hash seed), so that env leaves the twin's trajectory"""
    for t in range(steps):
        env.step(env.expert_actions(0.6, HASH + 1, step=t0 + t))


# ---- 1. rewind and branch against the oracle, all ten ids

@pytest.mark.parametrize("env_id", ALL_IDS)
def test_rewind_and_branch_equals_the_oracle(env_id):
    import torch

    env, seeds, options = make(env_id)
    acts = []
    for t in range(40):
        a = teacher(env, t)
        acts.append(a.cpu().numpy())
        env.step(a)
    snap = env.save_instances()
    assert snap.count == N and snap.records.shape[1] == env.instance_bytes and env.instance_bytes % 16 == 0
    w40 = [env.rng_words(i) for i in range(0, N, 8)]
    for t in range(40, 70):
        env.step(teacher(env, t))
    moved = sum(not np.array_equal(env.rng_words(i), w) for i, w in zip(range(0, N, 8), w40))
    obs = env.load_instances(snap, idx=torch.arange(N, dtype=torch.int32), rec=torch.as_tensor(PERM, dtype=torch.int32))
    ref = oracle(env_id, seeds[PERM], options)
    for t in range(40):
        ref.step(acts[t][PERM], autoreset=True, want_obs=False)
    assert np.array_equal(vis(obs).cpu().numpy(), ref.frames(range(N))), "frames of the load itself"
    ended = 0
    for t in range(60):
        a = teacher(env, 100 + t)
        obs, _, done, _, _ = env.step(a)
        dg, _, r2, d2 = ref.step_digest(a.cpu().numpy(), autoreset=True)
        bad = np.nonzero(digests(obs) != dg)[0]
        assert len(bad) == 0, "step %d: frames of instances %s differ from the oracle's" % (t, bad[:8])
        assert np.array_equal(env.reward64.cpu().numpy(), r2), "reward at step %d" % t
        assert np.array_equal(done.cpu().numpy(), d2.astype(bool)), "done at step %d" % t
        ended += int(d2.sum())
    print("%s: %d of %d sampled streams moved between save and load, %d episodes ended after the load" % (env_id, moved, len(w40), ended))
    assert 4 * ended >= N
    if env.gt_dim:
        assert np.array_equal(env.gt.cpu().numpy(), np.stack([e.gt() for e in ref.envs]).astype(np.float32)), "ground truth"
    assert np.array_equal(teacher(env, 999).cpu().numpy(), ref.expert_actions(EPS, HASH, 999)), "the teacher's action"
    for i in range(0, N, 8):
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words()), "RNG words of instance %d" % i
    env.check_errors()
    assert env.debug_counter("instance_saves") == 1 and env.debug_counter("instance_loads") == 1
    env.close()
    ref.close()


# ---- 2. frames of the load itself

@pytest.mark.parametrize("fmt", ["u8_xyc", "bf16_chw", "u8_chw"])
@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0"])
def test_frames_of_the_load(env_id, fmt):
    import torch
    from chw_referee import converted

    env, seeds, options = make(env_id, obs_format=fmt)
    ref = oracle(env_id, seeds, options)
    rows = (lambda f: torch.from_numpy(f) if fmt == "u8_xyc" else converted(fmt, f))
    for t in range(40):
        a = teacher(env, t)
        env.step(a)
        ref.step(a.cpu().numpy(), autoreset=True, want_obs=False)
    snap = env.save_instances()
    at40 = rows(ref.frames(range(N)))
    for t in range(40, 55):
        a = teacher(env, t)
        obs = env.step(a)[0]
        ref.step(a.cpu().numpy(), autoreset=True, want_obs=False)
    at55 = rows(ref.frames(range(N)))
    assert torch.equal(obs.cpu(), at55)
    sub = np.arange(0, N, 3)  # 67 instances
    idx = torch.as_tensor(sub, dtype=torch.int32)
    obs = env.load_instances(snap, idx=idx, rec=idx)
    mix = at55.clone()
    mix[sub] = at40[sub]
    same_rows(obs.cpu(), mix, "obs after a load of a subset (loaded rows: the save's frames, the others' bytes as they were)")
    env.obs.fill_(0)
    same_rows(env.redraw().cpu(), mix, "redraw() after the load")
    env.check_errors()
    env.close()
    ref.close()


# ---- 3. subsets, padding, one-to-many, bad indices

@pytest.mark.parametrize("env_id,count", [("MortarMayhem-Grid-v0", 1), ("Endless-SearingSpotlights-v0", 63), ("MysteryPath-v0", 65), ("Endless-MysteryPath-v0", 65),
                                          ("MortarMayhemB-v0", 200)])
def test_instances_not_named_keep_everything(env_id, count):
    """A load of `count` instances through an index array padded with -1: the instances it names are back at the save, every other one is bit for bit the
    twin's over 80 steps (frames, reward, done, infos, RNG words)."""
    import torch

    env, _, _ = make(env_id)
    twin, _, _ = make(env_id)
    lock_step_with_twin(env, twin, 40, t0=0, what="before the save")
    snap = env.save_instances()
    back = make(env_id)[0]  # a second twin that stops here: what the loaded instances return to
    for t in range(40):
        back.step(teacher(back, t))
    lock_step_with_twin(env, twin, 30, t0=40, what="before the load")
    named = np.sort(np.random.Generator(np.random.PCG64(count)).permutation(N)[:count])
    idx = np.full(N, -1, np.int64)
    idx[named] = named
    env.load_instances(snap, idx=torch.as_tensor(idx), rec=torch.as_tensor(np.maximum(idx, 0)))
    others = np.setdiff1d(np.arange(N), named)
    same_rng(env, back, [(i, i) for i in named[:6]], "loaded")
    if len(others):
        # equal actions for the instances that were not named: the twin's teacher; the named ones take them too (their results are not compared)
        lock_step_with_twin(env, twin, 80, t0=70, rows=others, what="%s, not named," % env_id)
        same_rng(env, twin, [(i, i) for i in others[:4]] + [(others[-1], others[-1])], "not named")
    else:
        lock_step_with_twin(env, back, 80, t0=70, what="%s, all loaded," % env_id)
    env.check_errors()
    for e in (env, twin, back):
        e.close()


@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-SearingSpotlights-v0", "MysteryPath-Grid-v0"])
def test_one_record_into_fifty_instances(env_id):
    """Record 0 loaded into instances 50 .. 99: they stay equal to each other and to the oracle's instance 0 under equal actions."""
    import torch

    env, seeds, options = make(env_id)
    ref = oracle(env_id, seeds[:1], options)
    for t in range(40):
        a = teacher(env, t)
        env.step(a)
        ref.step(a[:1].cpu().numpy(), autoreset=True, want_obs=False)
    snap = env.save_instances(idx=[0, 1, 2])
    env.step(teacher(env, 40))
    obs = env.load_instances(snap, idx=torch.arange(50, 100, dtype=torch.int32), rec=torch.zeros(50, dtype=torch.int32))
    want = torch.from_numpy(ref.frames([0]))
    same_rows(vis(obs)[50:100].cpu(), want.expand(50, -1, -1, -1), "frames of the load")
    ended = 0
    for t in range(60):
        a1 = ref.expert_actions(EPS, HASH, 500 + t)
        a = torch.as_tensor(np.repeat(a1, N, axis=0), device="cuda")
        obs, _, done, _, _ = env.step(a)
        o2, r2, d2 = ref.step(a1, autoreset=True)
        same_rows(vis(obs)[50:100].cpu(), torch.from_numpy(o2).expand(50, -1, -1, -1), "step %d frames" % t)
        assert bool((env.reward64[50:100] == float(r2[0])).all()) and bool((done[50:100] == bool(d2[0])).all()), "step %d" % t
        ended += int(d2[0])
    assert ended > 0
    for i in (50, 99):
        assert np.array_equal(env.rng_words(i), ref.envs[0].rng_words())
    env.check_errors()
    env.close()
    ref.close()


def test_bad_indices_are_skipped_and_flagged():
    """An instance index of num_envs and one of 2^31 - 1 are skipped, bit 512 is raised, check_errors reports and clears it, nothing else changed: the
    handle's state equals that of a twin whose load names the two valid instances alone."""
    import torch

    env, _, _ = make("MortarMayhem-Grid-v0")
    twin, _, _ = make("MortarMayhem-Grid-v0")
    for e in (env, twin):
        for t in range(20):
            e.step(teacher(e, t))
    snaps = [e.save_instances(idx=[3, 4, 5, 6]) for e in (env, twin)]
    for e in (env, twin):
        for t in range(20, 30):
            e.step(teacher(e, t))
    env.load_instances(snaps[0], idx=torch.tensor([3, N, 2 ** 31 - 1, 6], dtype=torch.int32))
    twin.load_instances(snaps[1], idx=torch.tensor([3, -1, -1, 6], dtype=torch.int32))
    twin.check_errors()
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    env.check_errors()  # cleared
    assert np.array_equal(env.state_dict()["blob"], twin.state_dict()["blob"])
    assert torch.equal(env.obs, twin.obs)
    # a record index outside the call's records, and a save from beyond the handle: flagged as well, the record keeps its bytes
    env.load_instances(snaps[0], idx=torch.tensor([3, 4, 5, 6], dtype=torch.int32), rec=torch.tensor([0, 4, -1, 3], dtype=torch.int32))
    twin.load_instances(snaps[1], idx=torch.tensor([3, -1, -1, 6], dtype=torch.int32), rec=torch.tensor([0, 0, 0, 3], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    assert np.array_equal(env.state_dict()["blob"], twin.state_dict()["blob"])
    before = snaps[0].records.clone()
    env.save_instances(idx=[-1, N, 2 ** 31 - 1, -5], out=snaps[0])
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    assert torch.equal(before, snaps[0].records)
    lock_step_with_twin(env, twin, 20, t0=30)
    env.close()
    twin.close()


# ---- 4. a save is read-only and nothing leaves the fused arrangement

@pytest.mark.parametrize("env_id,counter", zip(PER_ARRANGEMENT, ["one_launch_steps", "spot_fused_steps", None, "emp_fused_steps"]))
def test_a_save_every_step_changes_nothing(env_id, counter):
    env, _, _ = make(env_id)
    twin, _, _ = make(env_id)
    c0 = env.debug_counter(counter) if counter else 0
    snap = None
    ended = 0
    for t in range(100):
        snap = env.save_instances(out=snap)
        ended += lock_step_with_twin(env, twin, 1, t0=t, what="with a save per step, step %d:" % t)
    assert ended > 0
    same_rng(env, twin, [(0, 0), (N - 1, N - 1)])
    env.load_instances(snap)
    for t in range(10):
        env.step(teacher(env, 200 + t))
    if counter:  # every unmasked drawn step after a save and after a load went out as the fused launch
        assert env.debug_counter(counter) - c0 == 110
    assert env.debug_counter("instance_saves") == 100
    env.check_errors()
    env.close()
    twin.close()


# ---- 5. arrangements

def round_trip(env_id, perm=None, pre=30, away=20, post=60, options="default", render=True, n=N, final=False, eps_pre=None, at_save=None, **kw):
    """env and twin play `pre` steps, env saves all, leaves the twin's trajectory for `away` steps, loads (instance i <- record perm[i]) and must then be
    the twin (row i: the twin's row perm[i]) for `post` steps.  -> (env, twin, obs of the load)"""
    import torch

    env, _, _ = make(env_id, n=n, options=options, **kw)
    twin, _, _ = make(env_id, n=n, options=options, **kw)
    for t in range(pre):
        a = twin.expert_actions(EPS if eps_pre is None else eps_pre, HASH, step=t)
        twin.step(a)
        env.step(a)
    if at_save:
        at_save(env)
    snap = env.save_instances()
    detour(env, away)
    p = np.arange(n) if perm is None else perm
    obs = env.load_instances(snap, idx=torch.arange(n, dtype=torch.int32), rec=torch.as_tensor(p, dtype=torch.int32), render=render)
    if render:
        same_rows(vis(obs), vis(twin.obs)[torch.as_tensor(p, device="cuda")], "frames of the load")
    ended = lock_step_with_twin(env, twin, post, perm=p, final=final, what=env_id)
    assert ended > 0 or post == 0
    same_rng(env, twin, [(0, p[0]), (n - 1, p[n - 1])])
    env.check_errors()
    return env, twin, obs


def test_two_option_sets_travel_with_the_instances():
    """Two option sets in one handle, the halves swapped by a load: the loaded instance runs under the SAVED instance's set (oracle halves)."""
    import torch

    env_id, half = "MortarMayhem-Grid-v0", N // 2
    opt_a, opt_b = {"command_count": [3]}, {"command_count": [2], "explosion_delay": [3], "explosion_duration": [1]}
    env, seeds, _ = make(env_id, options=None)
    mask_a = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    ref_a, ref_b = oracle(env_id, seeds[:half], opt_a), oracle(env_id, seeds[half:], opt_b)
    for t in range(30):
        a = teacher(env, t)
        env.step(a)
        ref_a.step(a[:half].cpu().numpy(), autoreset=True, want_obs=False)
        ref_b.step(a[half:].cpu().numpy(), autoreset=True, want_obs=False)
    snap = env.save_instances()
    assert snap.set_of is not None
    detour(env, 10)
    swap = np.roll(np.arange(N), half)
    env.load_instances(snap, idx=torch.arange(N, dtype=torch.int32), rec=torch.as_tensor(swap, dtype=torch.int32))
    ended = 0
    for t in range(60):
        a = teacher(env, 100 + t)
        obs, _, done, _, _ = env.step(a)
        for ref, rows in ((ref_b, slice(0, half)), (ref_a, slice(half, N))):
            o2, r2, d2 = ref.step(a[rows].cpu().numpy(), autoreset=True)
            assert np.array_equal(obs[rows].cpu().numpy(), o2), "frames at step %d" % t
            assert np.array_equal(env.reward64[rows].cpu().numpy(), r2) and np.array_equal(done[rows].cpu().numpy(), d2.astype(bool)), "step %d" % t
            ended += int(d2.sum())
    assert ended > 0
    env.check_errors()
    env.close()


@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "Endless-MysteryPath-v0"])
def test_final_observation_handle(env_id):
    env, twin, _ = round_trip(env_id, perm=PERM, final=True, final_observation=True)
    snap = env.save_instances()
    with pytest.raises(ValueError):
        env.load_instances(snap, render=False)  # as step(render=False): terminal observations are frames
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id", PER_ARRANGEMENT)
def test_headless_steps_then_save_load_redraw(env_id):
    import torch

    env, _, _ = make(env_id)
    twin, _, _ = make(env_id)
    for t in range(30):
        a = teacher(twin, t)
        twin.step(a)
        assert env.step(a, render=False)[0] is None
    snap = env.save_instances()
    for t in range(20):
        env.step(env.expert_actions(0.6, HASH + 1, step=t), render=False)
    assert env.load_instances(snap, render=False) is None
    same_rows(vis(env.redraw()), vis(twin.obs), "redraw() after headless steps, save, load")
    detour(env, 5)
    env.step(teacher(env, 0), render=False)  # `obs` is stale: a drawn load draws everybody
    obs = env.load_instances(snap, idx=torch.arange(0, N, 2, dtype=torch.int32), rec=torch.arange(0, N, 2, dtype=torch.int32))
    same_rows(vis(obs)[0::2], vis(twin.obs)[0::2], "a drawn load on a stale handle, loaded rows")
    mine = vis(obs).clone()
    same_rows(vis(env.redraw()), mine, "a drawn load on a stale handle draws every row's CURRENT frame")
    env.check_errors()
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "Endless-SearingSpotlights-v0", "MysteryPath-v0"])
def test_copy_instances_rotation_by_one(env_id):
    """copy_instances with overlapping sets: instance (i + 1) % N <- instance i for every i at once."""
    import torch

    env, _, _ = make(env_id)
    twin, _, _ = make(env_id)
    lock_step_with_twin(env, twin, 30, t0=0)
    src = torch.arange(N, dtype=torch.int32)
    obs = env.copy_instances(src, torch.roll(src, -1))  # dst[j] = j + 1
    back = np.roll(np.arange(N), 1)  # row i of env is now the twin's row i - 1
    same_rows(vis(obs), vis(twin.obs)[torch.as_tensor(back, device="cuda")], "frames of the copy")
    assert lock_step_with_twin(env, twin, 60, perm=back, t0=30) > 0
    same_rng(env, twin, [(0, N - 1), (1, 0), (N - 1, N - 2)])
    env.check_errors()
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "MysteryPath-v0", "Endless-MysteryPath-v0"])
def test_debug_view_after_a_load(env_id):
    import torch

    p = np.roll(np.arange(40), 7)
    env, twin, _ = round_trip(env_id, perm=p, post=0, n=40)
    assert torch.equal(env.render_debug(), twin.render_debug()[torch.as_tensor(p, device="cuda")])
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id", ["MortarMayhemB-Grid-v0", "MortarMayhemB-v0"])
def test_vector_observation_rows(env_id):
    import torch

    env, twin, obs = round_trip(env_id, perm=PERM, post=0)
    p = torch.as_tensor(PERM, device="cuda")
    assert bool(twin.vector_obs.any()) and not torch.equal(twin.vector_obs, twin.vector_obs[p])
    assert torch.equal(obs["vector_observation"], twin.vector_obs[p]), "the loaded instances' vector rows"
    assert lock_step_with_twin(env, twin, 60, perm=PERM) > 0  # (compares the vector rows at every step)
    env.close()
    twin.close()


@pytest.mark.parametrize("env_id", ["SearingSpotlights-v0", "Endless-MysteryPath-v0"])
def test_checkpoint_after_a_load_continues_equal(env_id):
    import memory_gym_amd

    env, twin, _ = round_trip(env_id, perm=PERM, post=5)
    sd = env.state_dict()
    fresh = memory_gym_amd.make(env_id, num_envs=N, device=0)
    fresh.load_state_dict(sd)
    fresh.redraw()
    assert lock_step_with_twin(fresh, twin, 60, perm=PERM, t0=2000) > 0
    for e in (env, twin, fresh):
        e.close()


def test_capacity_row_that_is_no_multiple_of_16_bytes():
    """Endless-MysteryPath path_segments 6: a segment row of 312 bytes, moved 8 bytes per lane."""
    env, twin, _ = round_trip("Endless-MysteryPath-v0", perm=PERM, capacity={"path_segments": 6}, on_capacity="truncate")
    assert env.instance_bytes % 16 == 0
    env.close()
    twin.close()


def test_long_rows_under_a_follower():
    """Endless-MysteryPath path_segments 1,024 (rows of 53 KB, shared by four waves each) under the teacher at eps 0: paths that grow."""
    def grown(env):
        assert env.debug_counter("emp_segments_max") > 3, "the follower's paths did not grow before the save"

    env, twin, _ = round_trip("Endless-MysteryPath-v0", perm=PERM, pre=120, away=30, post=40, options={"max_steps": 150}, eps_pre=0.0,
                              capacity={"path_segments": 1024}, at_save=grown)
    env.close()
    twin.close()


def test_endless_mortar_mayhem_commands_8():
    env, twin, _ = round_trip("Endless-MortarMayhem-v0", perm=PERM, capacity={"commands": 8}, on_capacity="truncate")
    env.close()
    twin.close()


# ---- 6. graph capture

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"])
def test_save_and_load_are_graph_capturable(env_id):
    """save + load captured once, replayed three times with other contents of idx / rec: equal to the twin that makes the same calls eagerly."""
    import torch

    env, _, _ = make(env_id)
    twin, _, _ = make(env_id)
    K = 65
    src, dst, rec = (torch.zeros(K, dtype=torch.int32, device="cuda") for _ in range(3))
    snap = env.save_instances(idx=src)
    env.load_instances(snap, idx=torch.full((K,), -1, dtype=torch.int32))  # the handle's first load allocates: eagerly, naming nobody
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.save_instances(idx=src, out=snap)
        env.load_instances(snap, idx=dst, rec=rec)
    g = np.random.Generator(np.random.PCG64(3))
    for k in range(3):
        lock_step_with_twin(env, twin, 15, t0=100 * k, what="replay %d:" % k)
        s = g.permutation(N)[:K]
        d = g.permutation(N)[:K]
        d[k::7] = -1  # padding
        r = g.integers(0, K, K)
        src.copy_(torch.as_tensor(s, dtype=torch.int32))
        dst.copy_(torch.as_tensor(d, dtype=torch.int32))
        rec.copy_(torch.as_tensor(r, dtype=torch.int32))
        graph.replay()
        tsnap = twin.save_instances(idx=src)
        twin.load_instances(tsnap, idx=dst, rec=rec)
        torch.cuda.synchronize()
        same_rows(vis(env.obs), vis(twin.obs), "frames after replay %d" % k)
    assert lock_step_with_twin(env, twin, 40, t0=900) > 0
    same_rng(env, twin, [(i, i) for i in (0, 77, N - 1)])
    env.check_errors()
    env.close()
    twin.close()


# ---- 7. refusals

def test_refusals():
    import memory_gym_amd
    import torch

    env = memory_gym_amd.make("SearingSpotlights-v0", num_envs=8, device=0)
    with pytest.raises(ValueError):
        env.save_instances()  # before the first reset
    buf = torch.zeros(8 * 16384, dtype=torch.uint8, device="cuda")
    lib = memory_gym_amd._native.LIB
    assert lib.mg_save_instances(env._h, None, 8, buf.data_ptr(), None) == -1 and "before the first" in memory_gym_amd._native.last_error()
    env.reset(seed=1)
    assert lib.mg_save_instances(env._h, None, -1, buf.data_ptr(), None) == -1
    assert lib.mg_save_instances(env._h, None, 8, None, None) == -1
    assert lib.mg_save_instances(env._h, None, 8, buf.data_ptr() + 8, None) == -1
    assert lib.mg_load_instances(env._h, None, None, 8, buf.data_ptr() + 4, None, None) == -1
    assert lib.mg_save_instances(env._h, None, 0, buf.data_ptr(), None) == 0  # count == 0 is legal and does nothing
    snap = env.save_instances()
    other = memory_gym_amd.make("SearingSpotlights-v0", num_envs=8, device=0)
    other.reset(seed=1)
    with pytest.raises(ValueError, match="another handle"):
        other.load_instances(snap)
    for bad in (dict(idx=torch.arange(9)), dict(idx=torch.arange(8).float()), dict(idx=torch.arange(8), rec=torch.arange(7)),
                dict(idx=torch.zeros((2, 4), dtype=torch.int32))):
        with pytest.raises(ValueError):
            env.load_instances(snap, **bad)
    with pytest.raises(ValueError):
        env.load_instances(memory_gym_amd.InstanceSnapshot(snap.records[:, :-16].contiguous(), snap.layout))
    with pytest.raises(ValueError):
        env.save_instances(idx=[0, 1], out=snap)
    # a geometry option: the C calls refuse between the option and the reset, the snapshot is stale after the reset
    v = (memory_gym_amd._native.C.c_double * 1)(0.5)
    assert lib.mg_set_option(env._h, b"coin_scale", v, 1) == 0
    assert lib.mg_save_instances(env._h, None, 8, buf.data_ptr(), None) == -1 and "geometry" in memory_gym_amd._native.last_error()
    layout = env.instance_layout
    env.reset(seed=1, options={"coin_scale": 0.5})
    assert env.instance_layout != layout
    with pytest.raises(ValueError, match="geometry"):
        env.load_instances(snap)
    env.load_instances(env.save_instances())
    env.check_errors()
    env.close()
    other.close()


def test_single_instance_snapshot_and_restore():
    import memory_gym_amd

    env = memory_gym_amd.make("Endless-MortarMayhem-v0")
    o, _ = env.reset(seed=4)
    for t in range(12):
        env.step(env.expert_action(step=t))
    snap = env.snapshot()
    first = [env.step(env.expert_action(eps=1.0, seed=3, step=t)) for t in range(25)]
    o = env.restore(snap)
    again = [env.step(env.expert_action(eps=1.0, seed=3, step=t)) for t in range(25)]
    for (o1, r1, d1, _, i1), (o2, r2, d2, _, i2) in zip(first, again):
        assert np.array_equal(o1, o2) and r1 == r2 and d1 == d2 and np.array_equal(i1["ground_truth"], i2["ground_truth"])
        if d1:
            break
    env.close()


# ---- 8. through C

def test_c_host_program_saves_and_loads():
    import __graft_entry__

    exe = __graft_entry__.build_c_abi_instances_test()
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "endless-memory-gym_amd", "lib"), "/opt/rocm/lib", env.get("LD_LIBRARY_PATH", "")])
    for env_id in ("MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"):
        out = subprocess.run([exe, env_id, "200", "60"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("OK " + env_id), out.stdout
