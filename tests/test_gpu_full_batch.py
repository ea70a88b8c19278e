"""GPU (-m gpu): EVERY instance of the BASELINE.json configurations against the CPU oracle -- rewards, dones and the digest of every
frame after EVERY step, the frames themselves after the reset and at the end -- so that neither a mis-indexed tail workgroup or a wrong
grid stride beyond the first few thousand instances (round 1 compared 6-7 sampled instances at these sizes) nor a rare wrong frame
(round 6: one reset frame in ~10^7, which frames compared every 20th - 80th step met with a few per cent per run) can hide.  The digest:
tests/frame_digest.py, one 64-bit value per frame that the oracle computes from its own screens (no [n, 84, 84, 3] array is written) and
torch ops compute on the device (21 KB per frame stay there; 8 bytes cross).  Instance i is seeded i; same-step auto-reset on both sides.
Two policies: uniform random actions (`test_every_instance`), under which episodes are short and shallow (three of four
MortarMayhem-Grid episodes die at the first verification), and COMPETENT play (`test_every_instance_competent`, round 6: the oracle's
expert action for every instance's current state, a random one with probability 0.1) -- ten-command successes, command lists of a dozen
entries, path segments appended far beyond the initial three, opened exits -- on the launch arrangements that only exist at these sizes.
What the competent runs reached is asserted from the HIP side: the end-of-episode info the kernels wrote and mg_debug_counter scans of
the device's state records.  Both once more with final_observation=True (`..._final_observation`): every terminal frame of every step
against the oracle, at the sizes where the FINAL instantiations of the fused launches are selected."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (label, env id, instances, steps, compare frames every, options)
CONFIGS = [
    ("C2", "MortarMayhem-Grid-v0", 65536, 130, 26, None),
    ("C3", "MysteryPath-v0", 32768, 120, 20, dict(max_steps=24)),          # short episodes: thousands of A* resets inside the run
    ("C4", "Endless-SearingSpotlights-v0", 16384, 240, 30, None),
    ("C5 per-GPU shard", "Endless-MortarMayhem-v0", 32768, 160, 32, None),
    # the ids that are in no BASELINE config, at the sizes bench.py measures them ("other_workloads"); Endless-MysteryPath long enough
    # for several episodes per instance: lazy segments, records ahead of time and the instances' own resets on every instance
    ("Endless-MysteryPath", "Endless-MysteryPath-v0", 32768, 300, 30, None),
    ("SearingSpotlights", "SearingSpotlights-v0", 16384, 200, 25, dict(max_steps=40)),      # (every instance is reset inside the raster launch)
    ("MysteryPath-Grid", "MysteryPath-Grid-v0", 32768, 120, 20, dict(max_steps=24)),
    ("MortarMayhem", "MortarMayhem-v0", 32768, 160, 32, None),
    ("MortarMayhemB-Grid", "MortarMayhemB-Grid-v0", 32768, 100, 25, None),  # (Dict observation: the visual part here, the one-hot vector in test_gpu_mortar_b.py)
    ("MortarMayhemB", "MortarMayhemB-v0", 16384, 100, 25, None),
]


# What a run of _lock_step showed the oracle, per case: filled by the run, printed with `pytest -s` (profiles/oracle_every_frame.md)
SEEN = {}


def _lock_step(label, env_id, n, steps, every, options, eps=None, stats=None, final=False):
    """eps None: uniform random actions drawn on the device; else the oracle's expert actions with eps random ones.  `stats`:
    a dict the run fills from the HIP side's end-of-episode info (sums / maxima over the finished episodes) and its counters.

    Frames: after the reset and after EVERY step the 64-bit digests (tests/frame_digest.py) of all n device frames are compared
    with the n digests the oracle computed from its own screens (mgo_batch_step_digest) -- nothing is sampled, no instance is
    left out.  (`every` is what the periodic full-frame compare used to be; it only enters the record of what was seen before.)
    The frames themselves are compared after the reset and after the last step, and the reset's also prove that the device
    digest of a frame is the numpy digest of the same bytes on the host.

    final: the handle is made with final_observation=True.  Same-step auto-reset, uint8, one option set, no graph capture: every
    family then keeps the terminal observations inside its own launches (the FINAL instantiations), and after every step the
    digests of info["final_observation"] where done must be the oracle's digests of the frames its instances showed before
    their resets.  Every finished instance of every step; the run asserts that it compared as many as it counted dones."""
    import frame_digest as fd
    import memory_gym_amd
    import oracle_lib
    import torch

    env = memory_gym_amd.make(env_id, num_envs=n, device=0, final_observation=final)
    ref = oracle_lib.OracleBatch(env_id, n, options=options)
    seeds = np.arange(n, dtype=np.int64)
    all_instances = np.arange(n, dtype=np.int32)
    want = np.zeros((n, 84, 84, 3), np.uint8)
    rew, done = np.zeros(n, np.float64), np.zeros(n, np.uint8)
    want_dg, want_fdg = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    host = torch.empty((n, 84, 84, 3), dtype=torch.uint8).pin_memory()

    def frames_equal(where):
        host.copy_(obs)
        got = host.numpy()
        if not np.array_equal(got, want):
            env.check_errors()  # a capacity error flagged by the kernels explains a mismatch better than pixels do
            bad = np.nonzero((got != want).reshape(n, -1).any(1))[0]
            raise AssertionError("%s %s: %d of %d frames differ %s; first instances %s" % (label, env_id, len(bad), n, where, bad[:10]))

    def digests_equal(got_dg, want_u64, frames_dev, where, dones, mask=None, what="frames"):
        bad = fd.differing(got_dg, want_u64, mask)
        if len(bad):
            env.check_errors()
            first = bad[:8]
            pixels = -1
            if what == "frames":  # the oracle's screens still hold these frames (terminal ones are gone after its reset)
                dev = frames_dev[torch.as_tensor(first, device=frames_dev.device)].cpu().numpy()
                pixels = int((dev[0] != ref.frames(first)[0]).any(-1).sum())
            raise AssertionError("%s %s: the digests of %d of %d %s differ from the oracle's %s; instances %s, done %s, differing pixels of "
                                 "instance %d: %s" % (label, env_id, len(bad), n, what, where, first, np.asarray(dones)[first].astype(int), first[0],
                                                      pixels if pixels >= 0 else "not counted (the oracle's screen holds the next episode by now)"))

    def visual(o):
        return o["visual_observation"] if isinstance(o, dict) else o

    obs, _ = env.reset(seed=seeds, options=options)
    obs = visual(obs)
    dg = fd.digest_torch(obs)
    ref.reset(seeds, out=want)
    frames_equal("after reset")
    assert np.array_equal(fd.as_uint64(dg), fd.digest_numpy(want)), "%s: device digests of the reset frames != numpy digests of the same bytes" % label
    g = torch.Generator(device="cuda").manual_seed(17)
    disc = env.action_dim == 1
    a_host = np.empty((n,) if disc else (n, 2), np.int32)
    n_done = n_final = 0
    acc = {}
    for t in range(steps):
        if eps is None:
            a = torch.randint(0, 4 if disc else 3, (n,) if disc else (n, 2), device="cuda", generator=g, dtype=torch.int32)
            a_np = a.cpu().numpy()
        else:
            a_np = ref.expert_actions(eps, 4711, t, out=a_host)
            a = torch.from_numpy(a_np).to("cuda")
        obs, r, d, _, info = env.step(a)
        obs = visual(obs)
        dg = fd.digest_torch(obs)  # (queued behind the step: the device works while the oracle steps)
        fdg = fd.digest_torch(info["final_observation"]) if final else None
        ref.step_digest(a_np, autoreset=True, out=(want_dg, want_fdg, rew, done))
        dg_host = d.cpu().numpy()
        assert np.array_equal(dg_host, done.astype(bool)), "%s: done differs at step %d for instances %s" % (label, t, np.nonzero(dg_host != done.astype(bool))[0][:10])
        assert np.array_equal(env.reward64.cpu().numpy(), rew), "%s: reward differs at step %d for instances %s" % (
            label, t, np.nonzero(env.reward64.cpu().numpy() != rew)[0][:10])
        n_done += int(dg_host.sum())
        if stats is not None and dg_host.any():  # what the finished episodes reached, as the kernels reported it
            for name in env.info_names:
                v = info[name][d].double()
                s, m = acc.get(name, (0.0, -np.inf))
                acc[name] = (s + float(v.sum()), max(m, float(v.max())))
        digests_equal(dg, want_dg, obs, "at step %d" % t, dg_host)
        if final:
            digests_equal(fdg, want_fdg, info["final_observation"], "at step %d" % t, dg_host, mask=dg_host, what="terminal frames")
            n_final += int(dg_host.sum())
        if t == steps - 1:  # the frames themselves once more at the end
            ref.frames(all_instances, out=want)
            frames_equal("at step %d" % t)
    for i in (0, 1, n // 2, min(14335, n - 1), min(14336, n - 1), n - 2, n - 1):  # around the persistent grid's size and at both ends
        assert np.array_equal(env.rng_words(i), ref.envs[i].rng_words()), "%s: RNG words of instance %d" % (label, i)
    env.check_errors()
    if final:
        assert n_final == n_done and n_final > 0, "%s: %d terminal frames compared, %d dones counted" % (label, n_final, n_done)
    if stats is not None:
        stats["episodes"] = n_done
        for name, (s, m) in acc.items():
            stats["sum_" + name], stats["max_" + name] = s, m
        for name in stats.pop("counters", ()):
            stats[name] = env.debug_counter(name)
    seen = dict(frames=n * (steps + 1), terminal=n_final, before=n * (steps // every + 2))
    if final:  # which arrangement ran, where the shipped build can tell (the per-kernel counters "emp_own_resets" / "emp_final_served" exist in the lab build only)
        for name in {"Endless-MysteryPath-v0": ("emp_ahead_records",), "MysteryPath-v0": ("path_gen_paths",), "MysteryPath-Grid-v0": ("path_gen_paths",)}.get(env_id, ()):
            seen[name] = env.debug_counter(name)
            assert seen[name] > 0, "%s: %s = 0 -- the launches that generate paths / records inside the step did not run" % (label, name)
    SEEN[(label, "competent" if eps is not None else "random", "final" if final else "plain")] = seen
    print("oracle saw %s %s%s: %s" % (label, "competent" if eps is not None else "random", " final" if final else "", seen))
    env.close()
    ref.close()
    return n_done


@pytest.mark.parametrize("label,env_id,n,steps,every,options", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_instance(label, env_id, n, steps, every, options):
    assert _lock_step(label, env_id, n, steps, every, options) > 0


# Competent play at the sizes bench.py measures.  (label, env id, instances, steps, compare frames every,
# options, counters to read at the end, what the HIP side must report having reached)
COMPETENT = [
    ("C2", "MortarMayhem-Grid-v0", 65536, 170, 34, None, (),
     lambda s, n: s["sum_success"] > n // 4),                                           # full ten-command episodes
    ("C3", "MysteryPath-v0", 32768, 150, 30, None, (),
     lambda s, n: s["sum_success"] > n),                                                # goals reached along the A* path
    ("C4", "Endless-SearingSpotlights-v0", 16384, 260, 26, None, (),
     lambda s, n: s["max_coins_collected"] >= 12 and s["sum_coins_collected"] > 4 * n),
    ("C5 per-GPU shard", "Endless-MortarMayhem-v0", 32768, 560, 80, None, ("cmd_list_max",),
     lambda s, n: s["cmd_list_max"] >= 6),                                              # (a dozen entries: the slow variant below)
    ("Endless-MysteryPath", "Endless-MysteryPath-v0", 32768, 400, 40, None, ("emp_segments_sum", "emp_segments_max"),
     lambda s, n: s["emp_segments_sum"] > 6 * n and s["emp_segments_max"] >= 10),       # > 3 n segments appended beyond the initial three
    ("SearingSpotlights", "SearingSpotlights-v0", 16384, 200, 25, None, (),
     lambda s, n: s["sum_success"] > 2 * n),                                            # every coin, then the opened exit
    ("MysteryPath-Grid", "MysteryPath-Grid-v0", 32768, 120, 20, None, (),
     lambda s, n: s["sum_success"] > 4 * n),                                            # ~2,000 finished paths per step: the lane generator inside the raster launch
    ("MortarMayhem", "MortarMayhem-v0", 32768, 290, 58, None, (),
     lambda s, n: s["sum_success"] > n // 2),
]


@pytest.mark.parametrize("label,env_id,n,steps,every,options,counters,reached", COMPETENT, ids=[c[0] for c in COMPETENT])
def test_every_instance_competent(label, env_id, n, steps, every, options, counters, reached):
    stats = {"counters": counters}
    assert _lock_step(label, env_id, n, steps, every, options, eps=0.1, stats=stats) > 0 or env_id == "Endless-MysteryPath-v0"
    assert reached(stats, n), "%s: the competent run stayed shallow: %s" % (label, stats)


# final_observation=True at these sizes (same-step auto-reset, uint8, one option set, no graph capture): the kernel that writes the terminal
# frames which each case puts against the oracle.  (MortarMayhemB*: Dict observations, their terminal observations are not kept by the launches.)
FINAL_KERNEL = {
    "C2": "mortar_step_raster_kernel<false, true>: the one-launch step, the frame workgroup draws the terminal frame first",
    "C5 per-GPU shard": "mortar_step_raster_kernel<false, true>",
    "MortarMayhem": "mortar_step_raster_kernel<false, true>",
    "C3": "mystery_raster_paths_kernel<u8, true>: paths generated beside the raster, terminal frames drawn by the same launch",
    "MysteryPath-Grid": "mystery_raster_paths_kernel<u8, true>",
    "C4": "spot_raster_serve_kernel<..., FINAL> behind the deferring step kernel (16,384 instances: resets in the step kernel otherwise)",
    "SearingSpotlights": "spot_raster_serve_kernel<..., FINAL>: resets served inside the raster launch",
    "Endless-MysteryPath": "emp_step_kernel<false, true> + the sparse raster launch over the terminal descriptors behind it",
}
# Which kernel ran cannot be read from the shipped library: its per-kernel counters ("emp_own_resets", "emp_final_served") are compiled into the
# lab build only.  What the shipped build does count is asserted in _lock_step: "path_gen_paths" (finite Mystery Path: paths generated inside the
# step's launches) and "emp_ahead_records" (Endless-MysteryPath: first segments of next episodes generated ahead of time by the fused launch).
FINAL_CONFIGS = [c for c in CONFIGS if c[0] in FINAL_KERNEL]
FINAL_COMPETENT = [c for c in COMPETENT if c[0] in FINAL_KERNEL]


@pytest.mark.parametrize("label,env_id,n,steps,every,options", FINAL_CONFIGS, ids=[c[0] for c in FINAL_CONFIGS])
def test_every_instance_final_observation(label, env_id, n, steps, every, options):
    """test_every_instance with terminal observations kept: the digest of every finished instance's info["final_observation"] row against the
    oracle's digest of the frame that instance showed before its reset, after every step (FINAL_KERNEL: what writes those rows)."""
    assert len(FINAL_CONFIGS) == 8
    assert _lock_step(label, env_id, n, steps, every, options, final=True) > 0


@pytest.mark.parametrize("label,env_id,n,steps,every,options,counters,reached", FINAL_COMPETENT, ids=[c[0] for c in FINAL_COMPETENT])
def test_every_instance_competent_final_observation(label, env_id, n, steps, every, options, counters, reached):
    """Terminal frames of deep episodes: successes, emptied arenas, long paths.  Endless-MysteryPath: a competent agent ends an episode only
    through one of its random moves (eps = 0.1) -- on the oracle alone, 63 of the first 4,096 instances fall off the path or time out within
    these 400 steps (1.5 %, first at step 15), so some 500 terminal frames at 32,768; _lock_step asserts that there were some."""
    assert len(FINAL_COMPETENT) == 8
    stats = {"counters": counters}
    assert _lock_step(label, env_id, n, steps, every, options, eps=0.1, stats=stats, final=True) > 0
    assert reached(stats, n), "%s: the competent run stayed shallow: %s" % (label, stats)


def test_the_digest_compare_reports_exactly_the_altered_instance():
    """The comparison proves that it can fail: one byte of one instance altered in a CLONE of a real observation tensor (and of one
    final_observation row) is reported, that instance and no other."""
    import frame_digest as fd
    import memory_gym_amd
    import oracle_lib
    import torch

    n, env_id, options = 9001, "SearingSpotlights-v0", dict(max_steps=12)  # (three chunks of the device digest, the last one partial)
    env = memory_gym_amd.make(env_id, num_envs=n, device=0, final_observation=True)
    ref = oracle_lib.OracleBatch(env_id, n, options=options)
    seeds = np.arange(n, dtype=np.int64)
    obs, _ = env.reset(seed=seeds, options=options)
    assert len(fd.differing(fd.digest_torch(obs), ref.reset_digest(seeds))) == 0
    g = np.random.Generator(np.random.PCG64(4))
    for t in range(12):
        a = g.integers(0, 3, (n, 2)).astype(np.int32)
        obs, _, d, _, info = env.step(a)
        want, want_final, _, done = ref.step_digest(a)
        assert np.array_equal(d.cpu().numpy(), done.astype(bool))
    ended = np.nonzero(done)[0]  # max_steps = 12: all but the few that died a step earlier end in the twelfth step
    assert len(ended) > n // 2
    picks = [int(ended[0]), int(ended[ended > 4096][0]), int(ended[-1])]  # (one per chunk of the device digest)
    final = info["final_observation"]
    assert len(fd.differing(fd.digest_torch(obs), want)) == 0 and len(fd.differing(fd.digest_torch(final), want_final, mask=done)) == 0
    for tensor, expected in ((obs, want), (final, want_final)):
        for i, byte in zip(picks, (0, 84 * 84 * 3 - 1, 10001)):
            bad = tensor.clone()
            flat = bad.view(n, -1)
            flat[i, byte] ^= 1
            assert list(fd.differing(fd.digest_torch(bad), expected, mask=done)) == [i], "a changed byte %d of instance %d went unnoticed" % (byte, i)
    mask = done.astype(bool).copy()
    mask[picks[1]] = False  # ... and an instance outside the mask is not compared
    bad = final.clone()
    bad.view(n, -1)[picks[1], 5] ^= 0x80
    assert len(fd.differing(fd.digest_torch(bad), want_final, mask=mask)) == 0
    env.close()
    ref.close()


@pytest.mark.slow
def test_endless_mortar_lists_of_a_dozen():
    """Endless-MortarMayhem-v0 under competent play until command lists hold a dozen entries and more on over
    1 % of the instances (endless_mortar_mayhem.py:311-333: every completed list grows by one command and is executed again from the
    start -- 1,628 steps for the eleven lists before the twelfth with the default timings)."""
    if os.environ.get("MEMGYM_FAST"):
        pytest.skip("MEMGYM_FAST")
    n = 16384  # (the mortar family's one launch is the same arrangement at every size; the C5 shard size itself: the competent run above)
    stats = {"counters": ("cmd_list_max", "cmd_list_ge12")}
    _lock_step("C5 long", "Endless-MortarMayhem-v0", n, 1760, 220, None, eps=0.1, stats=stats)
    assert stats["cmd_list_ge12"] > n // 100 and stats["max_max_command_sequence"] >= 11, stats


# The arrangement that raced (tests/test_gpu_every_step.py runs these two cases HIP against HIP for 3,000 / 1,500 steps): resets served inside the
# raster launch, refereed by the oracle after every step, with and without terminal observations.  Steps: 1,000 of the 3,000 and 600 of the 1,500
# -- the oracle's spotlight step is the slowest of the three families and the GPU suite has a ceiling of 900 s for everything (profiles/
# oracle_every_frame.md has the measured durations); 2 x (16.4 + 12.0) million frames, each one seen by the oracle.
RACED = [("SearingSpotlights-v0", 16385, 1000), ("Endless-SearingSpotlights-v0", 20001, 600)]


@pytest.mark.slow
@pytest.mark.parametrize("final", [False, True], ids=["plain", "final_observation"])
@pytest.mark.parametrize("env_id,n,steps", RACED, ids=[c[0] for c in RACED])
def test_resets_inside_the_raster_launch_refereed_by_the_oracle(env_id, n, steps, final):
    assert _lock_step("raced", env_id, n, steps, steps, None, final=final) > 0
