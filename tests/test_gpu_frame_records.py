"""GPU (-m gpu): frame records -- mg_save_frames / mg_draw_frames (include/memgym.h), VecMemoryGym.save_frames / draw_frames -- against the frames the
handle itself wrote, against handles of the other observation formats and against the CPU oracle.

DEFINITION under test: a record saved from instance i after a call that wrote row i of the observation buffer in format F draws, in F, exactly those
bytes; in any other format the bytes a handle of that format would have shown.  Every comparison is bit for bit (torch.equal / np.array_equal).

Sizes: 48 instances (no multiple of 64) and 121 moments = 5,808 records for the whole-run cases; picks of 1, 3, 1,009 (a prime), 3,001 and 20,000 rows (the
last beyond the 16,384 frames at which generation 2 changes its store flavour and beyond both generations' grids, so that a workgroup draws several rows);
256 listed instances for the fused arrangements; 50,800 float32 rows = 4.30 GB for the offsets beyond 4 GiB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, T, EPS, HASH = 48, 120, 0.3, 11
ALL_IDS = ["MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0", "MysteryPath-Grid-v0",
           "MysteryPath-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0", "Endless-SearingSpotlights-v0"]
PER_FAMILY = ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "Endless-MysteryPath-v0"]  # generation 1 / generation 2 / generation 1 with a template per phase
RECORD_BYTES = {"Mortar": 16, "Mystery": 64, "Searing": 128}
FORMATS = ["u8_xyc", "f32_chw", "f16_chw", "bf16_chw", "u8_chw"]
PATTERN = 0xA5


def record_bytes(env_id):
    return next(v for k, v in RECORD_BYTES.items() if k in env_id)


def make(env_id, n=N, seed0=500, options=None, **kw):
    import memory_gym_amd

    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    seeds = np.arange(n, dtype=np.int64) * 3 + seed0
    env.reset(seed=seeds, options=options)
    return env, seeds


def same_rows(got, want, what):
    import torch

    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).reshape(got.shape[0], -1).any(1)).flatten().cpu().numpy()
        raise AssertionError("%s: %d of %d rows differ, first %s" % (what, len(bad), got.shape[0], bad[:8]))


def new_store(env, moments, n=None):
    import torch

    return torch.zeros((moments, env.num_envs if n is None else n, env.frame_record_bytes), dtype=torch.uint8, device="cuda")


def whole(env, store):
    import memory_gym_amd

    return memory_gym_amd.FrameRecords(store, env.frame_layout())


def rollout(env, steps, twins=(), keep=True, t0=0, **step_kw):
    """`steps` steps under env's own teacher; the twins take the same actions (with step_kw).  After the reset that came before and after each step:
    a clone of env.obs and env's records.  -> (store [steps + 1, N, bytes], clones [steps + 1, N, ...], the twins' stores)"""
    import torch

    store, tstores, clones = new_store(env, steps + 1), [new_store(w, steps + 1) for w in twins], []
    for t in range(steps + 1):
        if t:
            a = env.expert_actions(EPS, HASH, step=t0 + t)
            env.step(a)
            for w in twins:
                w.step(a, **step_kw)
        if keep:
            clones.append(env.obs.clone())
        rec = env.save_frames(out=store[t])
        assert rec.records.data_ptr() == store[t].data_ptr() and rec.layout == env.frame_layout()
        for w, ws in zip(twins, tstores):
            w.save_frames(out=ws[t])
    return store, (torch.stack(clones) if keep else None), tstores


# ---- 1. every frame of a run, all ten ids, against the handle's own frames and against the oracle

@pytest.mark.parametrize("env_id", ALL_IDS)
def test_every_frame_of_a_run(env_id):
    import oracle_lib
    import torch

    env, seeds = make(env_id)
    assert env.frame_record_bytes == record_bytes(env_id)
    ref = oracle_lib.OracleBatch(env_id, N)
    store, clones, want = new_store(env, T + 1), [], [ref.reset(seeds).copy()]
    for t in range(T + 1):
        if t:
            a = env.expert_actions(EPS, HASH, step=t)
            env.step(a)
            want.append(ref.step(a.cpu().numpy(), autoreset=True)[0].copy())
        clones.append(env.obs.clone())
        env.save_frames(out=store[t])
    drawn = env.draw_frames(whole(env, store))  # ONE call: 121 x 48 rows
    assert tuple(drawn.shape) == ((T + 1) * N, 84, 84, 3) and drawn.dtype == torch.uint8
    same_rows(drawn, torch.stack(clones).reshape(drawn.shape), env_id + ": drawn records against the frames of the run")
    got, want = drawn.cpu().numpy().reshape((T + 1, N, 84, 84, 3)), np.stack(want)
    for t in range(T + 1):
        assert np.array_equal(got[t], want[t]), "%s: records of moment %d differ from the oracle's frames for instances %s" % (
            env_id, t, np.nonzero((got[t] != want[t]).reshape(N, -1).any(1))[0][:8])
    assert env.debug_counter("frame_saves") == T + 1 and env.debug_counter("frame_draws") == 1
    env.check_errors()
    env.close()
    ref.close()


# ---- 2. headless: nothing was ever rastered at step time

@pytest.mark.parametrize("env_id", ALL_IDS)
def test_records_of_a_headless_twin(env_id):
    env, _ = make(env_id)
    twin, _ = make(env_id)
    _, clones, (tstore,) = rollout(env, T, twins=(twin,), render=False)
    assert twin.debug_counter("headless_steps") == T
    drawn = twin.draw_frames(whole(twin, tstore))
    same_rows(drawn, clones.reshape(drawn.shape), env_id + ": the headless twin's records against the drawn handle's frames")
    twin.check_errors()
    env.close()
    twin.close()


# ---- 3. formats: records carry none

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "MortarMayhem-v0", "SearingSpotlights-v0", "Endless-SearingSpotlights-v0", "Endless-MysteryPath-v0"])
def test_records_drawn_in_every_format(env_id):
    import torch

    steps = 30  # (the command glyphs of the mortar ids are shown in the first steps of an episode)
    env, _ = make(env_id)
    others = {f: make(env_id, obs_format=f)[0] for f in FORMATS[1:]}
    store, clones = new_store(env, steps + 1), {f: [] for f in FORMATS}
    for t in range(steps + 1):
        if t:
            a = env.expert_actions(EPS, HASH, step=t)
            for e in [env] + list(others.values()):
                e.step(a)
        env.save_frames(out=store[t])
        clones["u8_xyc"].append(env.obs.clone())
        for f, e in others.items():
            clones[f].append(e.obs.clone())
    for f in FORMATS:
        drawn = env.draw_frames(whole(env, store), obs_format=f)
        want = torch.stack(clones[f])
        assert drawn.dtype == want.dtype
        same_rows(drawn, want.reshape(drawn.shape), "%s: records of a u8_xyc handle drawn as %s" % (env_id, f))
    # and the other way round: records of a bf16_chw handle are the same bytes, drawn in the handle's own format by default
    rec = others["bf16_chw"].save_frames()
    assert torch.equal(rec.records, store[steps])
    same_rows(others["bf16_chw"].draw_frames(rec), clones["bf16_chw"][-1], env_id + ": default format")
    for e in [env] + list(others.values()):
        e.close()


# ---- 4. picks

@pytest.fixture(scope="module", params=PER_FAMILY)
def kept(request):
    """A handle, its store of 21 x 48 records and the identity draw of all of them (computed once, left unchanged)."""
    env, _ = make(request.param)
    store, clones, _ = rollout(env, 20)
    recs = whole(env, store)
    identity = env.draw_frames(recs)
    same_rows(identity, clones.reshape(identity.shape), request.param + ": identity draw")
    yield env, recs, identity
    env.close()


@pytest.mark.parametrize("case", ["permutation", "duplicates", "subset", "count_1", "count_3", "count_1009", "count_3001", "count_20000"])
def test_picks(kept, case):
    import torch

    env, recs, identity = kept
    n = recs.count
    g = torch.Generator().manual_seed(5)
    if case == "permutation":
        pick = torch.randperm(n, generator=g)
    elif case == "duplicates":
        pick = torch.randint(0, 7, (n,), generator=g) * 100  # seven records, each many times
    elif case == "subset":
        pick = torch.randperm(n, generator=g)[:200].sort().values
    else:
        pick = torch.randint(0, n, (int(case.split("_")[1]),), generator=g)
    drawn = env.draw_frames(recs, pick=pick.to(torch.int32 if case != "subset" else torch.int64))
    same_rows(drawn, identity[pick.cuda()], case)
    drawn = env.draw_frames(recs.records, pick=pick.tolist()[:50], obs_format="u8_chw")  # a plain tensor, a list of indices, another format
    same_rows(drawn, identity[pick[:50].cuda()].permute(0, 3, 2, 1).contiguous(), case + " as u8_chw")
    env.check_errors()


def test_picks_out_of_range_leave_their_rows(kept):
    import torch

    env, recs, identity = kept
    n = recs.count
    pick = torch.arange(0, 300, dtype=torch.int32) * 3
    pick[7], pick[100], pick[299] = -1, n, 2 ** 31 - 1
    bad = torch.tensor([7, 100, 299])
    out = torch.full((300, 84, 84, 3), PATTERN, dtype=torch.uint8, device="cuda")
    assert env.draw_frames(recs, pick=pick, out=out) is out
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    env.check_errors()  # cleared
    assert bool((out[bad.cuda()] == PATTERN).all()), "a pick outside the records wrote its row"
    good = torch.ones(300, dtype=torch.bool)
    good[bad] = False
    same_rows(out[good.cuda()], identity[pick[good].long().cuda()], "the rows next to picks out of range")
    # the save's side: an entry < 0 is skipped silently, one >= num_envs is skipped and flagged; both records keep their bytes
    before = recs.records[0].clone()
    env.save_frames(idx=[-1] * N, out=recs.records[0])
    env.check_errors()
    env.save_frames(idx=[N, 2 ** 31 - 1] + [-1] * (N - 2), out=recs.records[0])
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    assert torch.equal(before, recs.records[0])


# ---- 5. skip records: what a masked reset leaves for the instances it did not reset

@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_records_of_a_masked_reset_leave_rows_untouched(env_id):
    import torch

    env, _ = make(env_id)
    for t in range(10):
        env.step(env.expert_actions(EPS, HASH, step=t))
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[::5] = True
    env.reset(mask=mask)
    rec = env.save_frames()
    out = torch.full((N, 84, 84, 3), PATTERN, dtype=torch.uint8, device="cuda")
    env.draw_frames(rec, out=out)
    assert bool((out[~mask] == PATTERN).all()), "a record of an instance the masked reset left alone drew a frame"
    same_rows(out[mask], env.obs[mask], env_id + ": the reset instances' records")
    env.obs.fill_(PATTERN)
    env.redraw()  # the same thing: mg_render skips them as well
    same_rows(out, env.obs, env_id + ": draw_frames against redraw()")
    env.check_errors()
    env.close()


# ---- 6. the fused arrangements: the descriptor rows they leave are the rows a record needs

# Smallest handle that takes the fused launch and has 256 instances to list: the mortar one-launch step (MortarFamily::one_launch), the finite spotlight id's fused
# resets (SpotFamily::fuse_resets: n <= 65,536) and the endless Mystery Path launch (steps_fused) have no lower bound; the endless spotlight id fuses beyond
# RASTER_PLAIN_MAX = 16,384 instances in the one-byte formats.
@pytest.mark.parametrize("env_id,n,counter", [("MortarMayhem-Grid-v0", 256, "one_launch_steps"), ("SearingSpotlights-v0", 256, "spot_fused_steps"),
                                             ("Endless-SearingSpotlights-v0", 16385, "spot_fused_steps"), ("Endless-MysteryPath-v0", 256, "emp_fused_steps")])
def test_records_out_of_the_fused_launches(env_id, n, counter):
    import torch

    env, _ = make(env_id, n=n)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(2))[:256].to(torch.int32).cuda()
    c0 = env.debug_counter(counter)
    store, clones = new_store(env, 20, 256), []
    for t in range(20):
        env.step(env.expert_actions(EPS, HASH, step=t))
        env.save_frames(idx=idx, out=store[t])
        clones.append(env.obs[idx.long()])
    assert env.debug_counter(counter) - c0 == 20, "the steps did not take the fused launch"
    drawn = env.draw_frames(whole(env, store))
    same_rows(drawn, torch.stack(clones).reshape(drawn.shape), env_id + ": records out of the fused launch")
    env.check_errors()
    env.close()


# ---- 7. other arrangements

@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_records_after_masked_steps_loads_and_tapes(env_id):
    import torch

    env, _ = make(env_id)
    g = torch.Generator().manual_seed(9)
    for t in range(15):  # masked steps: inactive instances keep descriptor and row
        env.step(env.expert_actions(EPS, HASH, step=t), mask=torch.rand(N, generator=g) < 0.5)
        same_rows(env.draw_frames(env.save_frames()), env.obs, "%s: after masked step %d" % (env_id, t))
    snap = env.save_instances()
    frames = env.obs.clone()
    for t in range(10):
        env.step(env.expert_actions(0.6, HASH + 1, step=t))
    perm = torch.randperm(N, generator=g).to(torch.int32)
    env.load_instances(snap, idx=torch.arange(N, dtype=torch.int32), rec=perm, render=False)  # nothing drawn: the records alone know the frames
    same_rows(env.draw_frames(env.save_frames()), frames[perm.long().cuda()], env_id + ": after load_instances")
    shape = (12, N) if env.action_dim == 1 else (12, N, 2)
    tape = torch.randint(0, 3, shape, generator=g).to(torch.int32)
    env.play(tape, render=False)
    rec = env.save_frames()
    same_rows(env.draw_frames(rec), env.redraw(), env_id + ": after play()")
    env.check_errors()
    env.close()


def test_records_under_two_option_sets():
    import torch

    env_id, half = "MortarMayhem-Grid-v0", N // 2
    env, seeds = make(env_id)
    mask_a = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask_a[:half] = True
    env.reset(seed=seeds, options={"command_count": [3]}, mask=mask_a)
    env.reset(seed=seeds, options={"command_count": [2], "explosion_delay": [3], "explosion_duration": [1]}, mask=~mask_a)
    env.step(env.expert_actions(EPS, HASH, step=0))  # (the second masked reset left "leave the frame untouched" for the first half: a step, and every descriptor draws)
    store, clones, _ = rollout(env, 30)
    drawn = env.draw_frames(whole(env, store))
    same_rows(drawn, clones.reshape(drawn.shape), "two option sets in one handle")
    assert env.debug_counter("one_launch_steps") == 0  # (per-instance option sets: the two-launch form wrote these descriptors)
    env.close()


@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_save_and_draw_are_graph_capturable(env_id):
    """save + draw captured once, replayed with other contents of idx and pick: equal to the rows of `obs` they name."""
    import torch

    env, _ = make(env_id)
    K, M = 31, 77
    idx = torch.zeros(K, dtype=torch.int32, device="cuda")
    pick = torch.zeros(M, dtype=torch.int32, device="cuda")
    rec = env.save_frames(idx=idx)
    out = env.draw_frames(rec, pick=pick, obs_format="bf16_chw")  # (warm-up: both calls allocate nothing, but torch's side does)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.save_frames(idx=idx, out=rec)
        env.draw_frames(rec, pick=pick, out=out, obs_format="bf16_chw")
    g = torch.Generator().manual_seed(4)
    for k in range(3):
        for t in range(5):
            env.step(env.expert_actions(EPS, HASH, step=10 * k + t))
        i = torch.randperm(N, generator=g)[:K]
        p = torch.randint(0, K, (M,), generator=g)
        idx.copy_(i.to(torch.int32))
        pick.copy_(p.to(torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = (env.obs[i.cuda()][p.cuda()].permute(0, 3, 2, 1).to(torch.float32) / 255).to(torch.bfloat16)
        same_rows(out, want.contiguous(), "%s: replay %d" % (env_id, k))
    env.check_errors()
    env.close()


# ---- 8. layout, and a save changes nothing

def test_layout_follows_what_a_record_would_draw_differently():
    import memory_gym_amd
    import torch

    env, seeds = make("SearingSpotlights-v0")
    other, _ = make("SearingSpotlights-v0")
    assert env.frame_layout() != other.frame_layout() and env.frame_layout() != env.instance_layout
    rec = env.save_frames()
    with pytest.raises(ValueError, match="another handle"):
        other.draw_frames(rec)
    # the sticky background options travel IN the descriptor (its template field): no new layout, and an old record keeps drawing its own background
    # (sticky: an instance's backgrounds, once painted over, stay so -- the state keeps that, the descriptor names the template)
    layout, board_frames = env.frame_layout(), env.obs.clone()
    env.reset(seed=seeds, options={"hide_chessboard": True})
    assert env.frame_layout() == layout and not torch.equal(env.obs, board_frames)
    same_rows(env.draw_frames(rec), board_frames, "records saved with the chessboard, drawn after hide_chessboard")
    same_rows(env.draw_frames(env.save_frames()), env.obs, "records saved under hide_chessboard")
    # black_background for the first time: the border composer draws from now on (ordered_holes 0 -> 1) -- a new layout without a rebuild
    geometry = env.instance_layout
    env.reset(seed=seeds, options={"black_background": True})
    assert env.frame_layout() != layout and env.instance_layout == geometry
    with pytest.raises(ValueError, match="layout"):
        env.draw_frames(rec)
    layout = env.frame_layout()
    env.reset(seed=seeds, options={"black_background": False})  # (sticky: nothing changes back, and nothing changes again)
    env.reset(seed=seeds, options={"black_background": True})
    assert env.frame_layout() == layout
    # a geometry option + reset: a rebuild of the atlas
    rec = env.save_frames()
    env.reset(seed=seeds, options={"coin_scale": 0.5})
    assert env.frame_layout() != layout and env.instance_layout != geometry
    with pytest.raises(ValueError, match="layout"):
        env.draw_frames(rec)
    with pytest.raises(ValueError, match="layout"):
        env.draw_frames(memory_gym_amd.FrameRecords(rec.records, layout))
    same_rows(env.draw_frames(env.save_frames()), env.obs, "records of the new geometry")
    env.close()
    other.close()
    # the Mystery Path family's BIG-sprite composer is chosen by a rebuild: agent_scale is a geometry option
    env, seeds = make("MysteryPath-v0")
    layout = env.frame_layout()
    env.reset(seed=seeds, options={"agent_scale": 0.4})
    assert env.frame_layout() != layout
    for t in range(5):
        env.step(env.expert_actions(EPS, HASH, step=t))
    same_rows(env.draw_frames(env.save_frames()), env.obs, "records drawn by the BIG-sprite composer")
    env.close()


@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_a_save_changes_nothing(env_id):
    import torch

    env, _ = make(env_id)
    twin, _ = make(env_id)
    layout, geometry = env.frame_layout(), env.instance_layout
    for t in range(40):
        a = twin.expert_actions(EPS, HASH, step=t)
        env.save_frames()
        env.draw_frames(env.save_frames(idx=[t % N, 0]), obs_format="f16_chw")
        o1, r1, d1, _, _ = env.step(a)
        o2, r2, d2, _, _ = twin.step(a)
        same_rows(env.obs, twin.obs, "%s: step %d after a save" % (env_id, t))
        assert torch.equal(r1, r2) and torch.equal(d1, d2)
    for i in (0, N // 2, N - 1):
        assert np.array_equal(env.rng_words(i), twin.rng_words(i)), "RNG words of instance %d" % i
    assert np.array_equal(env.state_dict()["blob"], twin.state_dict()["blob"]), "state digest"
    assert env.frame_layout() == layout and env.instance_layout == geometry
    env.check_errors()
    env.close()
    twin.close()


# ---- 9. rows beyond 4 GiB

def test_rows_beyond_4_gib():
    import torch

    env, _ = make("MortarMayhem-Grid-v0")
    for t in range(6):
        env.step(env.expert_actions(EPS, HASH, step=t))
    rec = env.save_frames()
    direct = env.draw_frames(rec, obs_format="f32_chw")
    count, row_bytes = 50800, 84 * 84 * 3 * 4
    assert count * row_bytes > 2 ** 32 + 12 * row_bytes
    pick = (torch.arange(count, dtype=torch.int64) * 7 % N).to(torch.int32)  # a repeating pick that is no plain tiling of the store
    out = env.draw_frames(rec, pick=pick, obs_format="f32_chw")
    mark = 2 ** 32 // row_bytes  # the row that holds the 4-GiB mark
    rows = torch.tensor([0, count - 1] + list(range(mark - 12, mark + 13)))
    same_rows(out[rows.cuda()], direct[pick[rows].long().cuda()], "rows either side of the 4-GiB mark")
    del out
    env.check_errors()
    env.close()


# ---- 10. the C errors

def test_c_errors():
    import memory_gym_amd
    import torch

    lib, last = memory_gym_amd._native.LIB, memory_gym_amd._native.last_error
    env = memory_gym_amd.make("MysteryPath-Grid-v0", num_envs=8, device=0)
    B = 64
    assert lib.mg_frame_record_bytes(env._h) == B and lib.mg_frame_record_bytes(None) == 0 and lib.mg_frame_layout(None) == 0
    rec = torch.zeros((8, B), dtype=torch.uint8, device="cuda")
    obs = torch.full((8, 84, 84, 3), PATTERN, dtype=torch.uint8, device="cuda")
    r, o = rec.data_ptr(), obs.data_ptr()
    with pytest.raises(ValueError):
        env.save_frames()
    with pytest.raises(ValueError):
        env.draw_frames(rec)
    assert lib.mg_save_frames(env._h, None, 8, r, None) == -1 and "before the first" in last()
    assert lib.mg_draw_frames(env._h, r, 8, None, 8, 0, o, None) == -1 and "before the first" in last()
    env.reset(seed=1)
    pick = torch.zeros(16, dtype=torch.int32, device="cuda")
    refused = {"count < 0": lambda: lib.mg_save_frames(env._h, None, -1, r, None),
               "rec_dev is NULL": lambda: lib.mg_save_frames(env._h, None, 8, None, None),
               "not 16-byte aligned": lambda: lib.mg_save_frames(env._h, None, 8, r + 8, None)}
    drawn = {"count < 0": (r, 8, None, -1, 0, o), "rec_dev is NULL": (None, 8, None, 8, 0, o), "rec_dev is NULL or not": (r + 4, 8, None, 8, 0, o),
             "obs_dev is NULL": (r, 8, None, 8, 0, None), "obs_dev is NULL or not": (r, 8, None, 8, 0, o + 8), "n_records < 1": (r, 0, pick.data_ptr(), 8, 0, o),
             "unknown format": (r, 8, None, 8, 5, o), "unknown format ": (r, 8, None, 8, -1, o), "count > n_records": (r, 8, None, 9, 0, o),
             "n_records > INT32_MAX": (r, 2 ** 31, pick.data_ptr(), 8, 0, o)}
    for words, call in refused.items():
        assert call() == -1 and words in last(), words + ": " + last()
    for words, a in drawn.items():
        assert lib.mg_draw_frames(env._h, *a, None) == -1 and words.strip() in last(), words + ": " + last()
    v = (memory_gym_amd._native.C.c_double * 1)(0.3)
    assert lib.mg_set_option(env._h, b"agent_scale", v, 1) == 0  # a geometry option set since the last reset
    assert lib.mg_save_frames(env._h, None, 8, r, None) == -1 and "geometry" in last()
    assert lib.mg_draw_frames(env._h, r, 8, None, 8, 0, o, None) == -1 and "geometry" in last()
    env.reset(seed=1, options={"agent_scale": 0.3})
    assert lib.mg_save_frames(env._h, None, 0, r, None) == 0 and lib.mg_draw_frames(env._h, r, 8, None, 0, 0, o, None) == 0  # count == 0 is legal and does nothing
    torch.cuda.synchronize()
    assert bool((obs == PATTERN).all()) and bool((rec == 0).all()), "a refused call drew or saved something"
    assert env.debug_counter("frame_saves") == 0 and env.debug_counter("frame_draws") == 0
    for bad in (dict(pick=torch.zeros(3)), dict(pick=torch.zeros((2, 2), dtype=torch.int32)), dict(obs_format="rgb"), dict(out=obs[:7]), dict(out=obs.float()),
                dict(out=torch.zeros((9, 84, 84, 3), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            env.draw_frames(env.save_frames(), **bad)
    same_rows(env.draw_frames(env.save_frames()), env.obs, "after the refusals")
    env.check_errors()
    env.close()
