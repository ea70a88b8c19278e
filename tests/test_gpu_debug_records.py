"""GPU (-m gpu): debug-view records -- mg_save_debug_frames / mg_draw_debug_frames (include/memgym.h), VecMemoryGym.save_debug_frames /
draw_debug_frames -- against the CPU oracle's debug view, against twin handles that call render_debug(), and in the shapes where the draw can go wrong.

DEFINITION under test: a handle and a twin with the same history; every time render_debug() is called on the twin, save_debug_frames(S) is called on the
handle.  For every i in S the saved record drawn at size 336 is bit for bit row i of the twin's output at that moment, and an instance outside S behaves
like an instance of a handle on which no debug render was ever made (the mortar ids' clone of the glyph schedule is popped for the named instances alone).
Every comparison is exact.

Sizes: n = 24 and S = {0, 7, n - 1} throughout; draws of 0, 1, 3 x 14,336 + 1 (the grid both raster generations choose beyond 24,576 rows: a workgroup
draws its fourth row, one workgroup alone) and 12,700 rows (4.30 GB: row offsets beyond 4 GiB)."""
import numpy as np
import pytest

from test_gpu_debug_render import CASES

pytestmark = pytest.mark.gpu

N = 24
S = [0, 7, N - 1]
EPS, HASH = 0.3, 11
PATTERN = 0xA5
VIEW_BYTES = 336 * 336 * 3
ALL_IDS = ["MortarMayhem-Grid-v0", "MortarMayhem-v0", "Endless-MortarMayhem-v0", "MortarMayhemB-Grid-v0", "MortarMayhemB-v0", "MysteryPath-Grid-v0",
           "MysteryPath-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0", "Endless-SearingSpotlights-v0"]
PER_FAMILY = ["MortarMayhem-Grid-v0", "SearingSpotlights-v0", "Endless-MysteryPath-v0"]  # generation 1 / generation 2 / generation 1, owed segments
RASTER_GRID = 256 * 7 * 8  # csrc/mg_raster_v1.hpp, csrc/mg_raster.hpp: workgroups of a launch over more than 24,576 rows, both generations


def make(env_id, n=N, options=None, seed0=2, **kw):
    import memory_gym_amd

    env = memory_gym_amd.make(env_id, num_envs=n, device=0, **kw)
    seeds = np.arange(n, dtype=np.int64) * 5 + seed0
    env.reset(seed=seeds, options=options)
    return env, seeds


def same_rows(got, want, what):
    import torch

    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).reshape(got.shape[0], -1).any(1)).flatten().cpu().numpy()
        raise AssertionError("%s: %d of %d rows differ, first %s" % (what, len(bad), got.shape[0], bad[:8]))


def new_store(env, moments, k=len(S)):
    import torch

    return torch.zeros((moments, k, env.frame_record_bytes), dtype=torch.uint8, device="cuda")


def whole(env, store):
    import memory_gym_amd

    return memory_gym_amd.DebugFrameRecords(store, env.frame_layout())


def idx_dev(which=S):
    import torch

    return torch.tensor(list(which), dtype=torch.int32, device="cuda")


def saved_view(env, which=S):
    """one save of `which` and its draw at 336"""
    return env.draw_debug_frames(env.save_debug_frames(idx=idx_dev(which)))


# ---- 1. against the oracle, all ten ids

@pytest.mark.parametrize("env_id,options,steps", CASES, ids=["%s-%d" % (c[0], k) for k, c in enumerate(CASES)])
def test_records_equal_the_oracles_views(env_id, options, steps):
    """The run of tests/test_gpu_debug_render.py (its ids, options, step counts, seeds and actions).  After the reset and after every step S is saved
    into row t of a [T][3] store and the oracle's instances in S -- those alone -- give their debug view; ONE draw of all T x 3 records at the end."""
    import memory_gym_amd
    import oracle_lib

    env = memory_gym_amd.make(env_id, num_envs=N, device=0)
    ref = oracle_lib.OracleBatch(env_id, N, options=options)
    seeds = np.arange(N, dtype=np.int64) * 5 + 2
    env.reset(seed=seeds, options=options)
    ref.reset(seeds)
    disc = env.action_dim == 1
    prng = np.random.Generator(np.random.PCG64(7))
    store, want, idx = new_store(env, steps + 1), [], idx_dev()
    ended = 0
    for t in range(steps + 1):
        if t:
            a = (prng.integers(0, 4, N) if disc else prng.integers(0, 3, (N, 2))).astype(np.int32)
            _, _, done, _, _ = env.step(a)
            _, _, d2 = ref.step(a, autoreset=True, want_obs=False)
            assert np.array_equal(done.cpu().numpy(), d2.astype(bool))
            ended += int(d2[S].sum())
        rec = env.save_debug_frames(idx=idx, out=store[t])
        assert rec.records.data_ptr() == store[t].data_ptr() and rec.layout == env.frame_layout()
        want.append(np.stack([ref.envs[i].debug_view() for i in S]))
    drawn = env.draw_debug_frames(whole(env, store))  # ONE call: (steps + 1) x 3 rows
    assert tuple(drawn.shape) == ((steps + 1) * len(S), 336, 336, 3)
    got, want = drawn.cpu().numpy().reshape((steps + 1, len(S), 336, 336, 3)), np.stack(want)
    for t in range(steps + 1):
        for k, i in enumerate(S):
            if not np.array_equal(got[t, k], want[t, k]):
                bad = np.argwhere((got[t, k] != want[t, k]).any(-1))
                raise AssertionError("%s: record of instance %d at moment %d differs in %d px, first (y, x) = %s: hip %s oracle %s" % (
                    env_id, i, t, len(bad), bad[0], got[t, k][tuple(bad[0])], want[t, k][tuple(bad[0])]))
    print("%s: %d episodes ended in S" % (env_id, ended))
    assert ended > 0 or "Endless" in env_id or env_id.startswith("MortarMayhem")  # (the ids where that table's run ends episodes)
    assert env.debug_counter("debug_frame_saves") == steps + 1 and env.debug_counter("debug_frame_draws") == 1
    env.check_errors()
    env.close()
    ref.close()


# ---- 2. against a twin, and the pop rule

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "MortarMayhemB-v0", "Endless-MortarMayhem-v0"])
def test_twin_and_the_pop_rule(env_id):
    """Twin A calls render_debug() after every step, handle B saves S after every step, handle C never renders.  The run lasts until an instance of S has
    been auto-reset and 12 more steps have passed (the command display of the new episode), so it covers the first 12 steps after the reset and the 12
    after an auto-reset.  P, a fourth handle, is loaded from C's checkpoint at every step and rendered ONCE: what a handle that never rendered shows.
    (With the oracle alone, seeds 2, 7, 12, ... and this teacher: the first auto-reset in S is at step 47 / 69 / 83.)"""
    import memory_gym_amd
    import torch

    (A, _), (B, _), (C, _) = make(env_id), make(env_id), make(env_id)
    P = memory_gym_amd.make(env_id, num_envs=N, device=0)
    idx, sl = idx_dev(), torch.tensor(S, device="cuda")
    limit, until, first_reset = 200, None, None
    store, want, differ = new_store(B, limit + 1), [], 0
    t = 0
    while True:
        if t:
            a = A.expert_actions(EPS, HASH, step=t)
            dones = [e.step(a)[2] for e in (A, B, C)]
            assert torch.equal(dones[0], dones[1]) and torch.equal(dones[0], dones[2])
            if until is None and bool(dones[0][sl].any()):
                first_reset, until = t, t + 12
        want.append(A.render_debug()[sl])
        B.save_debug_frames(idx=idx, out=store[t])
        P.load_state_dict(C.state_dict())
        never = P.render_debug()[sl]
        differ += int((never != want[-1]).reshape(len(S), -1).any(1).sum())
        if t == until:
            break
        t += 1
        assert t <= limit, "no instance of S was auto-reset within %d steps" % limit
    assert first_reset is not None and t == first_reset + 12
    drawn = B.draw_debug_frames(whole(B, store[:t + 1].contiguous()))
    same_rows(drawn, torch.stack(want).reshape(drawn.shape), env_id + ": B's records of S against A's rows")
    # B and C differ in S at some step (else this run would show nothing about popping) ...
    print("%s: %d steps, first auto-reset in S at step %d, (instance, step) pairs where a never-rendered handle differs: %d" % (env_id, t, first_reset, differ))
    if env_id.startswith("MortarMayhemB"):  # the B ids give their commands in the vector observation: no glyph schedule, nothing a render could pop
        assert differ == 0
    else:
        assert differ > 0
    # ... and afterwards agree on every instance outside S
    others = torch.tensor([i for i in range(N) if i not in S], device="cuda")
    same_rows(B.render_debug()[others], C.render_debug()[others], env_id + ": instances outside S, B against C")
    for e in (A, B, C, P):
        e.check_errors()
        e.close()


# ---- 3. size 84

@pytest.mark.parametrize("env_id", ALL_IDS)
def test_size_84_is_the_surface_before_the_stretch(env_id):
    env, _ = make(env_id)
    for t in range(10):
        env.step(env.expert_actions(EPS, HASH, step=t))
    rec = env.save_debug_frames()  # all instances, in order
    assert rec.count == N
    big, small = env.draw_debug_frames(rec), env.draw_debug_frames(rec, size=84)
    assert tuple(big.shape) == (N, 336, 336, 3) and tuple(small.shape) == (N, 84, 84, 3)
    want = small.permute(0, 2, 1, 3).repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)  # [x][y][c] -> [y][x][c], every pixel four times per axis
    same_rows(big, want.contiguous(), env_id + ": size 336 against the stretched, transposed size 84")
    assert bool((small != small[:, :1, :1]).any()), "the debug surfaces are blank"
    env.check_errors()
    env.close()


# ---- 4. shapes where the draw can go wrong

@pytest.fixture(scope="module", params=PER_FAMILY)
def kept(request):
    """A handle, records of all its instances after 10 steps and their views at 336 as the twin's render_debug() gives them (computed once, left unchanged)."""
    import torch

    env, _ = make(request.param)
    twin, _ = make(request.param)
    for t in range(10):
        a = env.expert_actions(EPS, HASH, step=t)
        env.step(a)
        twin.step(a)
    rec = env.save_debug_frames()
    views = twin.render_debug()
    same_rows(env.draw_debug_frames(rec), views, request.param + ": identity draw")
    twin.close()
    yield env, rec, views
    env.close()


def test_count_1_and_count_0(kept):
    import torch

    env, rec, views = kept
    same_rows(env.draw_debug_frames(rec, pick=[5]), views[5:6], "count = 1")
    same_rows(env.draw_debug_frames(rec, pick=[N - 1], size=84).permute(0, 2, 1, 3).repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).contiguous(),
              views[N - 1:], "count = 1 at size 84")
    draws = env.debug_counter("debug_frame_draws")
    out = env.draw_debug_frames(rec, pick=torch.zeros(0, dtype=torch.int32))
    assert tuple(out.shape) == (0, 336, 336, 3)
    lib = __import__("memory_gym_amd")._native.LIB  # and the C call itself: count == 0 with good pointers returns 0 and does nothing
    row = torch.full((1, 336, 336, 3), PATTERN, dtype=torch.uint8, device="cuda")
    assert lib.mg_draw_debug_frames(env._h, rec.records.data_ptr(), N, None, 0, 336, row.data_ptr(), None) == 0
    assert lib.mg_save_debug_frames(env._h, None, 0, rec.records.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((row == PATTERN).all())
    assert env.debug_counter("debug_frame_draws") == draws  # count == 0: a no-op
    env.check_errors()


def test_count_three_grids_and_one(kept):
    """3 x grid + 1 rows for the grid the launch chooses: every workgroup draws three rows, workgroup 0 a fourth."""
    import torch

    env, rec, views = kept
    count = 3 * RASTER_GRID + 1
    assert count > 24576  # (the size from which generation 2 takes RASTER_GRID as well)
    pick = (torch.arange(count, dtype=torch.int64) * 7 % N).to(torch.int32).cuda()
    out = env.draw_debug_frames(rec, pick=pick)
    for a in range(0, count, 2048):
        same_rows(out[a:a + 2048], views[pick[a:a + 2048].long()], "rows %d .. of %d" % (a, count))
    del out
    env.check_errors()


def test_picks_with_duplicates_in_reverse_and_out_of_range(kept):
    import torch

    env, rec, views = kept
    pick = torch.tensor([N - 1, N - 1, 9, 9, 9, 4, 0, 0], dtype=torch.int32)
    same_rows(env.draw_debug_frames(rec, pick=pick), views[pick.long().cuda()], "duplicates")
    pick = torch.arange(N - 1, -1, -1, dtype=torch.int64)
    same_rows(env.draw_debug_frames(rec.records, pick=pick.tolist()), views[pick.cuda()], "reverse order, a plain tensor of records, a list of picks")
    pick = torch.tensor([3, 2, N, 1, 0], dtype=torch.int32)  # one entry out of range
    out = torch.full((5, 336, 336, 3), PATTERN, dtype=torch.uint8, device="cuda")
    assert env.draw_debug_frames(rec, pick=pick, out=out) is out
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    env.check_errors()  # cleared
    assert bool((out[2] == PATTERN).all()), "a pick outside the records wrote its row"
    good = torch.tensor([0, 1, 3, 4])
    same_rows(out[good.cuda()], views[pick[good].long().cuda()], "the rows next to the pick out of range")


def test_idx_with_minus_one_and_num_envs(kept):
    import torch

    env, rec, views = kept
    fill = torch.full((4, env.frame_record_bytes), PATTERN, dtype=torch.uint8, device="cuda")
    got = env.save_debug_frames(idx=[2, -1, 11, -1], out=fill.clone())
    env.check_errors()  # an entry < 0: skipped silently
    assert bool((got.records[1] == PATTERN).all()) and bool((got.records[3] == PATTERN).all()), "a skipped entry's record was written"
    got2 = env.save_debug_frames(idx=torch.tensor([N, 5, 2 ** 31 - 1, 6], dtype=torch.int32, device="cuda"), out=fill.clone())
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    assert bool((got2.records[0] == PATTERN).all()) and bool((got2.records[2] == PATTERN).all()), "an entry >= num_envs wrote its record"
    if "Mortar" not in env.env_id:  # (a second save of a mortar instance is its second debug render: the clone has moved on)
        same_rows(env.draw_debug_frames(got, pick=[0, 2]), views[[2, 11]], "the entries next to the skipped ones")
        same_rows(env.draw_debug_frames(got2, pick=[1, 3]), views[[5, 6]], "the entries next to the flagged ones")
    # the mirror refuses a host sequence that names an instance twice, a size that is neither, and records of the other kind
    with pytest.raises(ValueError, match="more than once"):
        env.save_debug_frames(idx=[3, 4, 3])
    with pytest.raises(ValueError, match="size"):
        env.draw_debug_frames(rec, size=168)
    with pytest.raises(ValueError, match="draw_debug_frames"):
        env.draw_frames(rec)
    with pytest.raises(ValueError, match="draw_frames"):
        env.draw_debug_frames(env.save_frames())
    # and the C call refuses the size itself
    lib = __import__("memory_gym_amd")._native.LIB
    out = torch.full((1, 336, 336, 3), PATTERN, dtype=torch.uint8, device="cuda")
    for size in (0, 83, 168, 335, -336):
        assert lib.mg_draw_debug_frames(env._h, rec.records.data_ptr(), N, None, 1, size, out.data_ptr(), None) == -1
    assert lib.mg_save_debug_frames(env._h, None, N + 1, fill.data_ptr(), None) == -1  # idx_dev == NULL with count > num_envs
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all())
    env.check_errors()


# ---- 5. offsets beyond 4 GiB

def test_rows_beyond_4_gib():
    """One record picked 12,700 times at size 336: 4.30 GB of output.  The first, the last and a middle row (the one that holds the 4-GiB mark) are the
    record's view; the bytes just beyond the last row keep their fill pattern."""
    import torch

    env, _ = make("MortarMayhem-Grid-v0")
    for t in range(6):
        env.step(env.expert_actions(EPS, HASH, step=t))
    rec = env.save_debug_frames(idx=[7])
    one = env.draw_debug_frames(rec)
    count, guard = 12700, 4096
    assert count * VIEW_BYTES > 2 ** 32 + VIEW_BYTES
    buf = torch.full((count * VIEW_BYTES + guard,), PATTERN, dtype=torch.uint8, device="cuda")
    out = buf[:count * VIEW_BYTES].view(count, 336, 336, 3)
    assert env.draw_debug_frames(rec, pick=torch.zeros(count, dtype=torch.int32), out=out) is out
    mark = 2 ** 32 // VIEW_BYTES  # the row that holds the 4-GiB mark
    for row in (0, mark - 1, mark, mark + 1, count - 1):
        same_rows(out[row:row + 1], one, "row %d of %d" % (row, count))
    assert bool((buf[count * VIEW_BYTES:] == PATTERN).all()), "bytes beyond the last row were written"
    del out, buf
    env.check_errors()
    env.close()


# ---- 6. arrangements

@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_after_headless_steps_and_after_advance(env_id):
    import torch

    (env, _), (twin, _) = make(env_id), make(env_id)
    sl = torch.tensor(S, device="cuda")
    for t in range(10):
        a = env.expert_actions(EPS, HASH, step=t)
        env.step(a, render=False)
        twin.step(a, render=False)
        if t in (0, 4, 9):
            same_rows(saved_view(env), twin.render_debug()[sl], "%s after headless step %d" % (env_id, t))
    assert env.debug_counter("headless_steps") == 10
    for e in (env, twin):
        e.advance(16, eps=EPS, seed=HASH, step=100, render=False, stats=False)
    same_rows(saved_view(env), twin.render_debug()[sl], env_id + " after advance(16)")
    for e in (env, twin):
        e.check_errors()
        e.close()


SETS = [("MortarMayhem-v0", dict(command_count=[3], explosion_delay=[6], explosion_duration=[2], command_show_duration=[2], command_show_delay=[3], visual_feedback=False),
         dict(command_count=[3], explosion_delay=[6], explosion_duration=[2], command_show_duration=[5], command_show_delay=[1], visual_feedback=True)),
        ("Endless-MysteryPath-v0", dict(show_stamina=True, show_background=False), dict(show_stamina=False, show_background=True)),
        ("SearingSpotlights-v0", dict(use_exit=True, coins_visible=True), dict(use_exit=False, coins_visible=False))]


@pytest.mark.parametrize("env_id,opt_a,opt_b", SETS, ids=[s[0] for s in SETS])
def test_two_option_sets_in_one_handle(env_id, opt_a, opt_b):
    """The halves of the handle under two option sets that differ in what the view shows (tests/test_gpu_debug_arrangements.py: SETS); S has instances of both."""
    import torch

    (env, seeds), (twin, _) = make(env_id), make(env_id)
    mask_a = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask_a[:N // 2] = True
    for e in (env, twin):
        e.reset(seed=seeds, options=opt_a, mask=mask_a)
        e.reset(seed=seeds, options=opt_b, mask=~mask_a)
    sl, idx = torch.tensor(S, device="cuda"), idx_dev()
    store, want = new_store(env, 21), []
    for t in range(21):
        if t:
            a = env.expert_actions(0.1, HASH, step=t)
            env.step(a, render=t % 4 != 3)
            twin.step(a, render=t % 4 != 3)
        env.save_debug_frames(idx=idx, out=store[t])
        want.append(twin.render_debug()[sl])
    drawn = env.draw_debug_frames(whole(env, store))
    same_rows(drawn, torch.stack(want).reshape(drawn.shape), env_id + ": two option sets")
    assert not torch.equal(drawn[0], drawn[len(S) - 1])
    for e in (env, twin):
        e.check_errors()
        e.close()


ARRANGED = [("MysteryPath-v0", dict(agent_scale=0.4)),                 # above 0.28: the BIG-sprite composer
            ("Endless-MysteryPath-v0", dict(agent_scale=0.4)),
            ("SearingSpotlights-v0", dict(black_background=True)),     # ordered_holes: the border composer
            ("Endless-SearingSpotlights-v0", dict(black_background=True))]


@pytest.mark.parametrize("env_id,options", ARRANGED, ids=["%s-%s" % (a[0], list(a[1])[0]) for a in ARRANGED])
def test_option_selected_composers(env_id, options):
    import torch

    (env, _), (twin, _) = make(env_id, options=options), make(env_id, options=options)
    sl, idx = torch.tensor(S, device="cuda"), idx_dev()
    store, want = new_store(env, 16), []
    for t in range(16):
        if t:
            a = env.expert_actions(EPS, HASH, step=t)
            env.step(a)
            twin.step(a)
        env.save_debug_frames(idx=idx, out=store[t])
        want.append(twin.render_debug()[sl])
    drawn = env.draw_debug_frames(whole(env, store))
    same_rows(drawn, torch.stack(want).reshape(drawn.shape), "%s under %s" % (env_id, options))
    small = env.draw_debug_frames(whole(env, store), size=84)
    same_rows(drawn, small.permute(0, 2, 1, 3).repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).contiguous(), "%s under %s, size 84" % (env_id, options))
    for e in (env, twin):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id,options", [("MortarMayhem-v0", dict(command_show_duration=[4], explosion_delay=[6])), ("MysteryPath-Grid-v0", None),
                                            ("SearingSpotlights-v0", None)])
def test_right_after_load_state_dict(env_id, options):
    """A save on a handle that was never reset, right after load_state_dict (the finite Mystery Path ids have no frame descriptors then): the ids of
    tests/test_gpu_debug_arrangements.py's checkpoint case.  (Endless-MysteryPath-v0 is not among them: its debug descriptor starts from the frame
    descriptor row, which is no part of the state, so a never-reset handle shows another view than the source until its first step -- with
    render_debug() and with a record alike.)"""
    import memory_gym_amd
    import torch

    (env, _), (twin, _) = make(env_id, options=options), make(env_id, options=options)
    for t in range(15):
        a = env.expert_actions(EPS, HASH, step=t)
        env.step(a)
        twin.step(a)
    fresh = memory_gym_amd.make(env_id, num_envs=N, device=0)
    fresh.load_state_dict(env.state_dict())
    same_rows(saved_view(fresh), twin.render_debug()[torch.tensor(S, device="cuda")], env_id + ": right after load_state_dict")
    for e in (env, twin, fresh):
        e.check_errors()
        e.close()


@pytest.mark.parametrize("env_id", PER_FAMILY)
def test_save_and_draw_from_a_captured_graph(env_id):
    """save + draw captured after a first eager call, replayed three times with idx changed between the replays.  The reference of a replay: on the
    mortar id a probe handle loaded from the handle's checkpoint just before it and rendered once (so its clone stands where the handle's does); on
    the other ids, whose view has no state of its own, a twin that takes the same steps."""
    import memory_gym_amd
    import torch

    env, _ = make(env_id)
    mortar = "Mortar" in env_id
    probe = memory_gym_amd.make(env_id, num_envs=N, device=0) if mortar else make(env_id)[0]
    K = 5
    idx = torch.arange(K, dtype=torch.int32, device="cuda")
    pick = torch.arange(K - 1, -1, -1, dtype=torch.int32, device="cuda")
    rec = env.save_debug_frames(idx=idx)  # (the first call, eager)
    out = env.draw_debug_frames(rec, pick=pick)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.save_debug_frames(idx=idx, out=rec)
        env.draw_debug_frames(rec, pick=pick, out=out)
    g = torch.Generator().manual_seed(4)
    for k in range(3):
        for t in range(4):
            a = env.expert_actions(EPS, HASH, step=10 * k + t)
            env.step(a)
            if not mortar:
                probe.step(a)
        i = torch.randperm(N, generator=g)[:K]
        idx.copy_(i.to(torch.int32))
        if mortar:
            probe.load_state_dict(env.state_dict())
        want = probe.render_debug()[i.cuda()].flip(0)
        graph.replay()
        torch.cuda.synchronize()
        same_rows(out, want.contiguous(), "%s: replay %d" % (env_id, k))
    env.check_errors()
    env.close()
    probe.close()


def test_a_record_is_refused_after_a_geometry_rebuild():
    import memory_gym_amd

    env, seeds = make("MysteryPath-v0")
    rec = env.save_debug_frames(idx=S)
    env.draw_debug_frames(rec)
    env.reset(seed=seeds, options={"agent_scale": 0.4})
    with pytest.raises(ValueError, match="layout"):
        env.draw_debug_frames(rec)
    with pytest.raises(ValueError, match="layout"):
        env.draw_debug_frames(memory_gym_amd.DebugFrameRecords(rec.records, rec.layout), size=84)
    other, _ = make("MysteryPath-v0", options={"agent_scale": 0.4})
    with pytest.raises(ValueError, match="another handle"):
        other.draw_debug_frames(env.save_debug_frames(idx=S))
    env.close()
    other.close()


# ---- 7. Endless-MysteryPath-v0: owed path segments

def test_endless_mystery_path_owed_segments():
    """Fused drawn steps, then a save with no other call in between (even moments; at odd moments the segment count is read either side of the save and the
    segments the save generated are reported), against the oracle."""
    import memory_gym_amd
    import oracle_lib

    env_id, steps = "Endless-MysteryPath-v0", 90
    env = memory_gym_amd.make(env_id, num_envs=N, device=0)
    ref = oracle_lib.OracleBatch(env_id, N)
    seeds = np.arange(N, dtype=np.int64) * 5 + 2
    env.reset(seed=seeds)
    ref.reset(seeds)
    idx, store, want, generated = idx_dev(), new_store(env, steps + 1), [], 0
    for t in range(steps + 1):
        if t:
            a = ref.expert_actions(EPS, HASH, t)
            env.step(a)
        if t % 2:
            before = env.debug_counter("emp_segments_sum")
        env.save_debug_frames(idx=idx, out=store[t])
        if t % 2:
            generated += env.debug_counter("emp_segments_sum") - before
        if t:
            ref.step(a, autoreset=True, want_obs=False)
        want.append(np.stack([ref.envs[i].debug_view() for i in S]))
    assert env.debug_counter("emp_fused_steps") == steps, "the steps did not take the fused launch"
    print("segments generated by the saves at odd moments: %d" % generated)  # (how many the step's own background jobs leave owed depends on timing: reported, not asserted)
    got = env.draw_debug_frames(whole(env, store)).cpu().numpy().reshape((steps + 1, len(S), 336, 336, 3))
    want = np.stack(want)
    for t in range(steps + 1):
        assert np.array_equal(got[t], want[t]), "moment %d: records differ from the oracle's views for %s" % (t, [S[k] for k in np.nonzero((got[t] != want[t]).reshape(len(S), -1).any(1))[0]])
    env.check_errors()
    env.close()
    ref.close()
