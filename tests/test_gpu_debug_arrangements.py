"""GPU (-m gpu): render("debug_rgb_array") -- mg_render_debug -- against the oracle's debug view in every arrangement that writes
the state ONLY the view reads: the mortar family's clone of the glyph schedule (dbg_pops) and its stored (sprite, rect) pair, the
finite Mystery Path ids' walls, the spotlight family's stale (sprite, rect) pair.  tests/test_gpu_debug_render.py referees the view
at n = 24 under drawn steps with one option set; here: headless steps, mg_advance, every path generator, two option sets in one
handle, a checkpoint into a never-reset handle, the terminal-frame forms in two observation formats, several renders per step,
masked resets, and n from 1 to 1,094 (debug_stretch_kernel's grid-stride loop runs from n = 149 on).

Every comparison is exact, and the oracle's instance i renders exactly as often as the handle does: every render pops the mortar
clone.  At SCALE 0.25 a view is its [::4, ::4] sample repeated 4 x 4; where many views are taken that is checked ON THE DEVICE
(and on the oracle's side) and only the samples are compared on the host -- the same pixels, a sixteenth of the copy.

The witness figures (FIRST_RESET, FINISHED, LANE_N, TERMINAL_RUN, ...) were measured with the oracle ALONE on the CPU (seeds
0 .. n - 1, its expert at eps 0.3, hash seed 7, auto-reset) and are asserted from the oracle before a view is compared, so that a run
in which nothing resets, no clone empties or no wall is generated cannot pass."""
import numpy as np
import pytest

from test_gpu_headless import EPS, FINISHED, HASH_SEED, MORTAR, _full, oracle_loop, pair

pytestmark = pytest.mark.gpu

ALL_IDS = sorted(FINISHED)
# n = 200: (the first step, 0-based, in which an instance finishes and is auto-reset; how many do)
FIRST_RESET = {"MortarMayhem-Grid-v0": (45, 43), "MortarMayhem-v0": (57, 1), "Endless-MortarMayhem-v0": (21, 3), "MortarMayhemB-Grid-v0": (6, 51),
               "MortarMayhemB-v0": (18, 2), "MysteryPath-Grid-v0": (5, 1), "MysteryPath-v0": (26, 1), "Endless-MysteryPath-v0": (16, 2),
               "SearingSpotlights-v0": (9, 1), "Endless-SearingSpotlights-v0": (33, 1)}


def view_full(env):
    got = env.render_debug().cpu().numpy()
    assert got.shape == (env.num_envs, 336, 336, 3) and got.dtype == np.uint8
    return got


def view_sampled(env):
    """-> (the view on the device, its [::4, ::4] sample on the host), the view checked on the device to be the sample repeated 4 x 4"""
    v = env.render_debug()
    n = env.num_envs
    s = v[:, ::4, ::4]
    assert bool((v.view(n, 84, 4, 84, 4, 3) == s[:, :, None, :, None, :]).all()), "a debug view is not its 84 x 84 sample repeated 4 x 4"
    return v, s.cpu().numpy()


def oracle_views(refs, sampled, which=None):
    """One render of instance i of every batch in `refs` (all of them, or `which`), in order; sampled: the [::4, ::4] sample."""
    out = []
    for ref in refs:
        for i in (range(ref.n) if which is None else which):
            w = ref.envs[i].debug_view()
            if sampled:
                s = w[::4, ::4]
                assert np.array_equal(np.repeat(np.repeat(s, 4, 0), 4, 1), w)
                w = s
            out.append(w)
    return np.stack(out)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
        px = np.argwhere((got[bad[0]] != want[bad[0]]).any(-1))
        raise AssertionError("%s: debug views of %d instances differ, first %s; instance %d in %d px, first (y, x) = %s: hip %s oracle %s" % (
            what, len(bad), bad[:8], bad[0], len(px), px[0], got[bad[0]][tuple(px[0])], want[bad[0]][tuple(px[0])]))


def check_full(env, refs, what, which=None):
    got = view_full(env)
    same(got if which is None else got[list(which)], oracle_views(refs, False, which), what)


def check_sampled(env, refs, what, which=None):
    v, s = view_sampled(env)
    same(s if which is None else s[list(which)], oracle_views(refs, True, which), what)
    return v


def lock_step(env, ref, t, render=True):
    """one step of the oracle's policy on both sides -> the oracle's done flags"""
    a = ref.expert_actions(EPS, HASH_SEED, t)
    _, _, done, _, _ = env.step(a, render=render)
    _, r2, d2 = ref.step(a, autoreset=True, want_obs=False)
    d2 = d2.astype(bool)
    assert np.array_equal(done.cpu().numpy(), d2) and np.array_equal(env.reward64.cpu().numpy(), r2), "step %d" % t
    return d2


# ---- 1. headless steps

@pytest.mark.parametrize("env_id", ALL_IDS)
def test_view_after_headless_steps(env_id):
    """n = 200, 120 headless steps: the view after the reset, after steps 1, 49, 50 and 119 and at the first step that auto-reset an
    instance -- which is then rendered between its auto-reset and its next step: the stored pair is a finished episode's."""
    n = 200
    env, ref = pair(env_id, n)
    check_full(env, [ref], "%s after the reset" % env_id)
    first, count = FIRST_RESET[env_id]
    seen = None
    for t in range(120):
        d2 = lock_step(env, ref, t, render=False)
        if seen is None and d2.any():
            seen = (t, int(d2.sum()))
            assert seen == (first, count), seen
        if t in (1, 49, 50, 119, first):
            check_full(env, [ref], "%s after headless step %d" % (env_id, t))
    assert seen == (first, count), seen
    assert env.debug_counter("headless_steps") == 120
    env.check_errors()
    env.close()
    ref.close()


# ---- 2. mg_advance

@pytest.mark.parametrize("env_id", list(MORTAR) + ["MysteryPath-v0", "SearingSpotlights-v0"])
def test_view_after_advance(env_id):
    """advance(200, eps 0.3) after a seeded reset (the mortar ids inside mortar_advance_kernel, the others launch by launch), the view
    against an oracle batch that played the loop of the definition; then one drawn step and the view again."""
    n = 200
    env, ref = pair(env_id, n)
    env.advance(200, eps=EPS, seed=HASH_SEED, step=0, render=False, stats=False)
    _, episodes = oracle_loop(ref, 200, EPS, 0)
    assert int(episodes.sum()) == FINISHED[env_id], int(episodes.sum())  # episodes ended inside the call
    fused = env_id in MORTAR
    assert (env.debug_counter("advance_fused_steps"), env.debug_counter("headless_steps")) == ((200, 0) if fused else (0, 200))
    check_full(env, [ref], "%s after advance(200)" % env_id)
    lock_step(env, ref, 200)
    check_full(env, [ref], "%s one drawn step after advance(200)" % env_id)
    env.check_errors()
    env.close()
    ref.close()


# ---- 3. walls from every generator

PATH_MASS = 2 * 4 * 128  # csrc/mg_mystery_finite.hpp: a queue LONGER than this is served by the lane-per-path generator (MEMGYM_PATH_HELP unset)
# max_steps = 12: the smallest n at which step 11 QUEUES more than PATH_MASS resets for the raster / path-service launch.  MysteryPath-Grid-v0 queues
# every reset (defer 1): 1,025 of its first 1,094 instances are truncated then.  MysteryPath-v0 (defer 2, csrc/mg_mystery.hip defer_mode) queues a wave's
# resets only when the wave -- 16 instances -- has more than HYBRID_INLINE = 2 of them, and all of its instances are truncated in step 11: 1,025 and
# 1,026 instances queue 1,024 (the last wave serves its one or two itself, with the cooperative generator), 1,027 queue 1,027.
LANE_N = {"MysteryPath-Grid-v0": 1094, "MysteryPath-v0": 1027}
HYBRID_INLINE, WAVE_INSTANCES = 2, 16


def queued(env_id, done):
    """how many of the finished instances the step kernel queues (csrc/mg_mystery_finite.hpp mystery_step_kernel: queue_mine)"""
    if env_id == "MysteryPath-Grid-v0":
        return int(done.sum())
    per_wave = [int(done[k:k + WAVE_INSTANCES].sum()) for k in range(0, len(done), WAVE_INSTANCES)]
    return sum(c for c in per_wave if c > HYBRID_INLINE)


@pytest.mark.parametrize("env_id", sorted(LANE_N))
def test_walls_from_every_generator(env_id):
    """max_steps = 12: step 11 truncates and resets more than 1,024 instances at once.  The drawn handle's raster / path-service launch
    generates the queued paths and walls with the lane generator ("path_lane_paths" counts exactly the queue, and nothing with one
    instance fewer), the headless handle's step kernel all of them with the cooperative one ("path_lane_paths" stays 0); before that step
    the walls are those of mystery_reset_kernel.  Views after steps 11, 12 and 13 on both handles."""
    import memory_gym_amd

    n = LANE_N[env_id]
    drawn, ref = pair(env_id, n, options=dict(max_steps=12))
    headless = memory_gym_amd.make(env_id, num_envs=n, device=0)
    headless.reset(seed=np.arange(n, dtype=np.int64), options=dict(max_steps=12))
    for t in range(14):
        c0 = [(e.debug_counter("path_gen_paths"), e.debug_counter("path_lane_paths")) for e in (drawn, headless)] if t == 11 else None
        a = ref.expert_actions(EPS, HASH_SEED, t)
        _, _, d_a, _, _ = drawn.step(a)
        _, _, d_b, _, _ = headless.step(a, render=False)
        _, _, d2 = ref.step(a, autoreset=True, want_obs=False)
        d2 = d2.astype(bool)
        assert np.array_equal(d_a.cpu().numpy(), d2) and np.array_equal(d_b.cpu().numpy(), d2), "step %d" % t
        if t == 11:
            q = queued(env_id, d2)
            assert q > PATH_MASS and queued(env_id, d2[:-1]) <= PATH_MASS and c0[0][1] == 0, (q, queued(env_id, d2[:-1]))  # the smallest such n
            assert q == {"MysteryPath-Grid-v0": 1025, "MysteryPath-v0": 1027}[env_id] and int(d2.sum()) == q
            made = [(e.debug_counter("path_gen_paths") - c[0], e.debug_counter("path_lane_paths") - c[1]) for e, c in zip((drawn, headless), c0)]
            assert made == [(q, q), (q, 0)], made  # (paths, of which by the lane generator): the whole queue on the drawn handle, none on the headless one
        if t in (11, 12, 13):
            want = oracle_views([ref], True)
            for name, e in (("drawn", drawn), ("headless", headless)):
                _, s = view_sampled(e)
                same(s, want, "%s, %s handle, after step %d" % (env_id, name, t))
    for e in (drawn, headless):
        e.check_errors()
        e.close()
    ref.close()


# ---- 4. two option sets in one handle

SHORT = dict(command_count=[3], explosion_delay=[6], explosion_duration=[2])  # episodes of at most 42 steps
SETS = [("MortarMayhem-v0", dict(SHORT, command_show_duration=[2], command_show_delay=[3], visual_feedback=False),
         dict(SHORT, command_show_duration=[5], command_show_delay=[1], visual_feedback=True)),
        ("Endless-MysteryPath-v0", dict(show_stamina=True, show_background=False), dict(show_stamina=False, show_background=True)),
        ("SearingSpotlights-v0", dict(use_exit=True, coins_visible=True), dict(use_exit=False, coins_visible=False))]


@pytest.mark.parametrize("env_id,opt_a,opt_b", SETS, ids=[s[0] for s in SETS])
def test_view_under_two_option_sets(env_id, opt_a, opt_b):
    """n = 256, the halves under two option sets that differ in what the view shows (the period the mortar clone is read with, the
    tile colours; stamina bar and background; exit and coins), 80 steps of which every fourth is headless: each half against its own
    oracle batch.  (The actions are the device's teacher at eps 0.1, checked elsewhere: the oracle numbers its random actions by the
    index in ITS batch.)"""
    import memory_gym_amd
    import oracle_lib
    import torch

    n = 256
    half = n // 2
    env = memory_gym_amd.make(env_id, num_envs=n, device=0)
    seeds = np.arange(n, dtype=np.int64) + 3
    refs = []
    env.reset(seed=seeds)  # (SearingSpotlights: every instance gets an exit first -- use_exit = False keeps drawing the earlier one)
    for opts, sl in ((opt_a, slice(0, half)), (opt_b, slice(half, n))):
        ref = oracle_lib.OracleBatch(env_id, half, options=_full(env_id, dict()))
        ref.reset(seeds[sl])
        ref.set_options(_full(env_id, opts))
        ref.reset(seeds[sl])
        refs.append(ref)
    mask_a = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds, options=opt_a, mask=mask_a)
    env.reset(seed=seeds, options=opt_b, mask=~mask_a)
    if env_id == "MortarMayhem-v0":
        assert (refs[0].get_all("show_dur") == 2).all() and (refs[1].get_all("show_dur") == 5).all()
    check_sampled(env, refs, "%s after the masked resets" % env_id)
    finished, shown = [0, 0], [0, 0]
    for t in range(80):
        a = env.expert_actions(0.1, HASH_SEED, t)
        _, _, done, _, _ = env.step(a, render=t % 4 != 3)
        a = a.cpu().numpy()
        for k, (ref, sl) in enumerate(zip(refs, (slice(0, half), slice(half, n)))):
            _, r2, d2 = ref.step(a[sl], autoreset=True, want_obs=False)
            assert np.array_equal(done[sl].cpu().numpy(), d2.astype(bool)) and np.array_equal(env.reward64[sl].cpu().numpy(), r2), "half %d, step %d" % (k, t)
            finished[k] += int(d2.sum())
        if t % 8 in (3, 6):  # (t % 8 == 3: right after a headless step)
            if env_id == "MortarMayhem-v0":
                for k in range(2):
                    shown[k] += int((refs[k].get_all("vis_len") > 0).sum())  # instances whose view reads the clone at this render
            check_sampled(env, refs, "%s after step %d" % (env_id, t))
    print("%s: finished %s, renders inside a display %s" % (env_id, finished, shown))
    assert min(finished) > 0 or env_id == "Endless-MysteryPath-v0", finished  # (its episodes outlast 80 steps of a teacher at eps 0.1)
    assert env_id != "MortarMayhem-v0" or min(shown) > 0, shown
    env.check_errors()
    env.close()
    for ref in refs:
        ref.close()


# ---- 5. checkpoint

CHECKPOINT = [("MortarMayhem-v0", dict(command_show_duration=[4], explosion_delay=[6])), ("MysteryPath-Grid-v0", None), ("SearingSpotlights-v0", None)]


@pytest.mark.parametrize("env_id,options", CHECKPOINT, ids=[c[0] for c in CHECKPOINT])
def test_view_across_a_checkpoint(env_id, options):
    """40 steps with debug renders after steps 10 and 20 (MortarMayhem-v0 under these options shows glyphs for 49 steps: every instance is
    inside the display at the checkpoint, two entries of its clone popped), state_dict() into a fresh, never-reset handle: both handles'
    views equal each other and the oracle's, at once (t = 39 below) and after each of 30 more steps, across auto-resets."""
    import memory_gym_amd
    import torch

    n = 160
    env, ref = pair(env_id, n, options=options)
    for t in range(40):
        lock_step(env, ref, t)
        if t in (10, 20):
            check_sampled(env, [ref], "%s after step %d" % (env_id, t))
    if env_id == "MortarMayhem-v0":
        assert (ref.get_all("clone_pops") == 2).all() and (ref.get_all("vis_len") > 0).all()
    fresh = memory_gym_amd.make(env_id, num_envs=n, device=0)
    fresh.load_state_dict(env.state_dict())
    finished = 0
    for t in range(39, 70):
        if t >= 40:
            a = ref.expert_actions(EPS, HASH_SEED, t)
            (_, r_a, d_a, _, _), (_, r_b, d_b, _, _) = env.step(a), fresh.step(a)
            _, r2, d2 = ref.step(a, autoreset=True, want_obs=False)
            assert torch.equal(r_a, r_b) and torch.equal(d_a, d_b) and np.array_equal(d_a.cpu().numpy(), d2.astype(bool)), "step %d" % t
            finished += int(d2.sum())
        v_a = check_sampled(env, [ref], "%s, the checkpointed handle at step %d" % (env_id, t))
        v_b = fresh.render_debug()
        assert torch.equal(v_a, v_b), "%s: the restored handle's view differs at step %d" % (env_id, t)
    print("%s: %d episodes finished behind the checkpoint" % (env_id, finished))
    assert finished > 0
    for e in (env, fresh):
        e.check_errors()
        e.close()
    ref.close()


# ---- 6. terminal-frame forms and formats

# n = 160: steps to run so that three steps with a finishing instance (and the step after the third) lie inside the run
TERMINAL_RUN = {"MortarMayhem-Grid-v0": 56, "MortarMayhem-v0": 61, "Endless-MortarMayhem-v0": 29, "MortarMayhemB-Grid-v0": 15, "MortarMayhemB-v0": 25,
                "SearingSpotlights-v0": 24}


@pytest.mark.parametrize("fmt", ["u8_xyc", "f32_chw"])
@pytest.mark.parametrize("env_id", sorted(TERMINAL_RUN))
def test_view_with_terminal_frames_kept(env_id, fmt):
    """final_observation=True: the step's own launches draw the terminal frame and the new episode's first one, and the mortar family's
    hand-over word reuses the view's ring bit to mark terminal frames.  The view is uint8 image order whatever the format, and equals the
    oracle's at every step in which an instance finished and at the step after."""
    n = 160
    env, ref = pair(env_id, n, final_observation=True, obs_format=fmt)
    steps, after, checks, finishing = TERMINAL_RUN[env_id], False, 0, 0
    for t in range(steps):
        d2 = lock_step(env, ref, t)
        if d2.any() or after:
            check_sampled(env, [ref], "%s %s at step %d" % (env_id, fmt, t))
            checks += 1
        finishing += int(d2.any())
        after = bool(d2.any())
    assert finishing >= 3 and checks >= 4, (finishing, checks)
    name = "one_launch_steps" if env_id in MORTAR else "spot_fused_steps"
    assert env.debug_counter(name) > 0 and env.debug_counter("final_obs_generic_steps") == 0
    env.check_errors()
    env.close()
    ref.close()


# ---- 7. a render changes nothing else

@pytest.mark.parametrize("env_id", ["MortarMayhem-v0", "MysteryPath-v0", "SearingSpotlights-v0"])
def test_a_render_changes_nothing_else(env_id):
    """Three handles run the same 64 steps with 0, 1 and 3 debug renders behind every step: frames, rewards, dones, infos and the
    random streams are equal.  The handle with 3 renders per step equals the oracle rendered 3 times per step, on the first and the
    last 16 instances (the oracle's other instances are never rendered) -- more renders than steps: MortarMayhem-v0's clone of 40 entries
    is empty after 14 steps while the display lasts 39, and no glyph is drawn from then on (oracle/mgo_mortar.c mm_debug)."""
    import memory_gym_amd
    import torch

    n = 160
    which = list(range(16)) + list(range(n - 16, n))
    env, ref = pair(env_id, n)
    envs = [env] + [memory_gym_amd.make(env_id, num_envs=n, device=0) for _ in range(2)]  # 0, 1 and 3 renders per step
    for e in envs[1:]:
        e.reset(seed=np.arange(n, dtype=np.int64))
    emptied = 0
    for t in range(64):
        a = ref.expert_actions(EPS, HASH_SEED, t)
        outs = [e.step(a) for e in envs]
        _, _, d2 = ref.step(a, autoreset=True, want_obs=False)
        assert np.array_equal(outs[0][2].cpu().numpy(), d2.astype(bool)), "step %d" % t
        for k in (1, 2):
            (o, r, d, tr, info), (o2, r2, dd, tr2, info2) = outs[0], outs[k]
            assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, dd) and torch.equal(tr, tr2), "handle %d, step %d" % (k, t)
            assert torch.equal(envs[0].reward64, envs[k].reward64) and sorted(info) == sorted(info2)
            for key in info:
                assert torch.equal(info[key], info2[key]), "handle %d: info[%r] differs at step %d" % (k, key, t)
        envs[1].render_debug()
        for k in range(3):
            if env_id == "MortarMayhem-v0":  # a render that finds the clone empty while glyphs are still being shown
                emptied += int(((ref.get_all("clone_pops") >= ref.get_all("vis_total")) & (ref.get_all("vis_len") > 0))[which].sum())
            check_sampled(envs[2], [ref], "%s: render %d after step %d" % (env_id, k, t), which)
    print("%s: %d renders found the clone empty" % (env_id, emptied))
    assert env_id != "MortarMayhem-v0" or emptied > 32 * 20 * 3, emptied  # 32 instances, steps 14 .. 38, three renders each
    for i in range(n):
        w = envs[0].rng_words(i)
        assert np.array_equal(w, envs[1].rng_words(i)) and np.array_equal(w, envs[2].rng_words(i)) and np.array_equal(w, ref.envs[i].rng_words())
    for e in envs:
        e.check_errors()
        e.close()
    ref.close()


# ---- 8. sizes and masked resets

# reset instances whose stored pair is not the new agent's (sprite, rect) / that step 29 had auto-reset already
MOVED = {("Endless-MortarMayhem-v0", 5): 2, ("Endless-MortarMayhem-v0", 149): 50, ("Endless-MortarMayhem-v0", 257): 86,
         ("SearingSpotlights-v0", 5): 2, ("SearingSpotlights-v0", 149): 50, ("SearingSpotlights-v0", 257): 86}
TWICE = {("Endless-MortarMayhem-v0", 5): 0, ("Endless-MortarMayhem-v0", 149): 1, ("Endless-MortarMayhem-v0", 257): 3,
         ("SearingSpotlights-v0", 5): 0, ("SearingSpotlights-v0", 149): 2, ("SearingSpotlights-v0", 257): 2}


@pytest.mark.parametrize("n", [1, 5, 149, 257])
@pytest.mark.parametrize("env_id", ["Endless-MortarMayhem-v0", "MysteryPath-v0", "SearingSpotlights-v0"])
def test_view_at_every_size_and_after_a_masked_reset(env_id, n):
    """30 steps (views after the reset and after steps 0, 14 and 29), then a masked reset() of every third instance and a view: the reset
    instances show the pair their finished episode left (Endless-MortarMayhem-v0: the old agent's sprite at its old rect), the others what
    they showed.  n = 149: the first size at which debug_stretch_kernel's capped grid strides; 257: two strides for some workgroups."""
    import torch

    env, ref = pair(env_id, n)
    check_full(env, [ref], "%s n=%d after the reset" % (env_id, n))
    last_done = np.full(n, -1)
    for t in range(30):
        last_done[lock_step(env, ref, t, render=t % 2 == 0)] = t
        if t in (0, 14, 29):
            check_full(env, [ref], "%s n=%d after step %d" % (env_id, n, t))
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[::3] = True
    before = view_full(env)
    before_ref = oracle_views([ref], False)
    same(before, before_ref, "%s n=%d before the masked reset" % (env_id, n))
    env.reset(mask=mask)
    for i in range(0, n, 3):
        ref.envs[i].reset(None, want_obs=False)
    if env_id != "MysteryPath-v0" and n >= 5:  # the stale pair: the view's agent is not where the new episode's agent is
        moved = sum(1 for i in range(0, n, 3) if (ref.envs[i].get("disp_x"), ref.envs[i].get("disp_y")) != (ref.envs[i].get("ax"), ref.envs[i].get("ay")))
        assert moved == MOVED[env_id, n], moved
        # ... and instances that step 29 had auto-reset are reset twice in a row: the pair is still the one of the agent that stepped last
        assert int((last_done[::3] == 29).sum()) == TWICE[env_id, n]
    got = view_full(env)
    same(got, oracle_views([ref], False), "%s n=%d after the masked reset" % (env_id, n))
    if env_id != "Endless-MortarMayhem-v0":  # (a mortar render pops the clone: the next view may show another glyph)
        keep = np.ones(n, bool)
        keep[::3] = False
        assert np.array_equal(got[keep], before[keep]), "a masked reset changed the view of an instance it did not reset"
    env.check_errors()
    env.close()
    ref.close()
