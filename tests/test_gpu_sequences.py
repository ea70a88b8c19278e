"""GPU (-m gpu): episode sequences -- mg_split_episodes / mg_sequence_picks / mg_draw_frames_padded (include/memgym.h), VecMemoryGym.split_episodes /
EpisodeSequences.picks / draw_frames_padded / draw_sequences -- against the header's definition in numpy (tests/sequence_definition.py), against
draw_frames / RolloutTrace.draw of the same records, and against the CPU oracle.  Every comparison is exact.

Tables and picks come from crafted `done` arrays: no stepping, one handle per family at the N the case needs.  The base cases are
done = default_rng(20261021).random((K, N)) < p for (K, N, p, L) = (64, 200, 0.06, 16), (64, 200, 0.06, 7), (64, 200, 0.06, 100), (1030, 257, 0.01, 64),
all from one generator; the counts the definition gives for them are asserted before the device is looked at.  (The stated counts -- 1,364 / 2,249 /
955 / 5,713 sequences -- are those of the generator drawing the [1030, 257] array THIRD and the L = 100 array last; in the order of the list the last two
would be 941 / 5,707.  The draws below are made in the order that gives the stated counts.)
Drawing: K = 64, N = 200 traces with the inputs of tests/test_gpu_rollout_trace.py, one id per composer, all five formats."""
import functools

import numpy as np
import pytest

import sequence_definition as sd

pytestmark = pytest.mark.gpu

FORMATS = ["u8_xyc", "f32_chw", "f16_chw", "bf16_chw", "u8_chw"]
SENTINEL = -7  # every int32 of a table / pick row the device must not write
PATTERN = 0xA5  # every byte of an observation row the device must not write
HANDLE_IDS = {200: "MortarMayhem-Grid-v0", 257: "SearingSpotlights-v0", 1: "Endless-MysteryPath-v0"}  # one id per family
# (K, N, p, L) -> sequences, full-length ones, shorter ones, the bound: from the definition alone
BASE = [((64, 200, 0.06, 16), (1364, 393, 971, 1617)), ((64, 200, 0.06, 7), (2249, 1455, 794, 2706)), ((64, 200, 0.06, 100), (955, 0, 955, 969)),
        ((1030, 257, 0.01, 64), (5713, 2865, 2848, 7001))]
DRAW_ORDER = (0, 1, 3, 2)


@functools.lru_cache(maxsize=None)
def base_cases():
    """-> [(done bool [K, N], L, the definition's table)] in the order of BASE.  Computed once, never written to."""
    g = np.random.default_rng(20261021)
    done = {}
    for k in DRAW_ORDER:
        K, N, p, _ = BASE[k][0]
        done[k] = g.random((K, N)) < p
    out = []
    for k, ((K, N, p, L), (total, full, shorter, limit)) in enumerate(BASE):
        table = sd.split(done[k], L)
        none = int((~done[k].any(0)).sum())
        print("(K, N, p, L) = %s: %d sequences, %d full, %d shorter, %d instances without a done, bound %d" % (
            (K, N, p, L), len(table), int((table[:, 2] == L).sum()), int((table[:, 2] < L).sum()), none, sd.bound(done[k], L)))
        assert (len(table), int((table[:, 2] == L).sum()), int((table[:, 2] < L).sum()), sd.bound(done[k], L)) == (total, full, shorter, limit)
        assert len(table) < limit
        if N == 200:
            assert none in (3, 4), none
        for a in (done[k], table):
            a.setflags(write=False)
        out.append((done[k], L, table))
    return out


_HANDLES = {}


def handle(n):
    """a started handle of n instances (HANDLE_IDS), shared by the tests of this module"""
    import memory_gym_amd

    if n not in _HANDLES:
        env = memory_gym_amd.make(HANDLE_IDS[n], num_envs=n, device=0)
        env.reset(seed=np.arange(n, dtype=np.int64))
        _HANDLES[n] = env
    return _HANDLES[n]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for env in _HANDLES.values():
        env.check_errors()
        env.close()
    _HANDLES.clear()
    for env, _ in _TRACES.values():
        env.close()
    _TRACES.clear()


def dev(a, dtype=None):
    import torch

    t = torch.as_tensor(np.array(a), device="cuda")  # (a writable copy: the base cases are read-only)
    return t if dtype is None else t.to(dtype)


def c_split(env, done, L, steps_of=None, start=None, capacity=None):
    """mg_split_episodes through the C ABI into a table filled with SENTINEL -> (table int32 [capacity, 4] on the host, count)"""
    import torch
    from memory_gym_amd import _native

    K, N = done.shape
    d = dev(done, torch.uint8)
    s = None if steps_of is None else dev(steps_of, torch.int32)
    b = None if start is None else dev(start, torch.uint8)
    cap = sd.bound(done, L) if capacity is None else capacity
    table = torch.full((cap + 3, 4), SENTINEL, dtype=torch.int32, device="cuda")  # (three rows past the capacity: nothing may land there)
    count = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = _native.LIB.mg_split_episodes(env._h, d.data_ptr(), K, None if s is None else s.data_ptr(), None if b is None else b.data_ptr(), L,
                                       table.data_ptr() if cap else None, cap, count.data_ptr(), env._stream())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return table.cpu().numpy(), int(count.item())


def check_split(env, done, L, steps_of=None, start=None, capacity=None, what=""):
    """the C call and the Python mirror against the definition: count, the written rows, SENTINEL everywhere else -> the definition's table"""
    import torch

    want = sd.split(done, L, steps_of, start)
    assert len(want) <= sd.bound(done, L)
    table, count = c_split(env, done, L, steps_of, start, capacity)
    cap = len(table) - 3
    held = min(len(want), cap)
    assert count == len(want), "%s: count %d, the definition has %d" % (what, count, len(want))
    bad = np.argwhere((table[:held] != want[:held]).any(1)).flatten()
    assert not len(bad), "%s: %d of %d entries differ, first entry %d: %s against %s" % (what, len(bad), held, bad[0], table[bad[0]], want[bad[0]])
    assert (table[held:] == SENTINEL).all(), "%s: something was written at or beyond entry %d (count %d, capacity %d)" % (what, held, count, cap)
    # the Python mirror
    seqs = env.split_episodes(dev(done), L, steps=None if steps_of is None else dev(steps_of, torch.int64), starts=None if start is None else dev(start),
                              capacity=capacity)
    assert seqs.table.shape == (sd.bound(done, L) if capacity is None else capacity, 4) and seqs.table.dtype == torch.int32
    assert (seqs.length, seqs.steps, seqs.num_envs) == (L, done.shape[0], done.shape[1])
    assert int(seqs.count.item()) == len(want) and np.array_equal(seqs.table[:held].cpu().numpy(), want[:held])
    return want, seqs


# ---- 1. tables and picks from crafted done arrays

@pytest.mark.parametrize("case", range(4), ids=["L16", "L7", "L100", "K1030_N257"])
def test_base_cases(case):
    done, L, want = base_cases()[case]
    K, N = done.shape
    env = handle(N)
    c0 = env.debug_counter("sequence_splits")
    got, seqs = check_split(env, done, L, what="base case %d" % case)
    assert env.debug_counter("sequence_splits") == c0 + 2 and np.array_equal(got, want)
    assert len(seqs) == len(want)
    pick, mask = seqs.picks()
    wp, wm, _ = sd.picks(want, None, len(want), L, N)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm)
    assert int(wm.sum()) == K * N  # every step of every instance, once
    env.check_errors()


CORNERS = ["all_done", "none_done", "done_at_the_last_step", "N_1", "K_1", "L_1", "starts_all_0", "starts_random", "steps_of_random"]


@pytest.mark.parametrize("corner", CORNERS)
def test_corners(corner):
    g = np.random.default_rng(CORNERS.index(corner) + 1)
    K, N, L = 64, 200, 16
    base = base_cases()[0][0]
    steps_of = start = None
    if corner == "all_done":
        done = np.ones((K, N), dtype=bool)
    elif corner == "none_done":
        done = np.zeros((K, N), dtype=bool)
    elif corner == "done_at_the_last_step":
        done = np.zeros((K, N), dtype=bool)
        done[K - 1] = True
    elif corner == "N_1":
        N, done = 1, base[:, 17:18].copy()
        assert done.any()
    elif corner == "K_1":
        K, done = 1, base[5:6].copy()
        assert done.any() and not done.all()
    elif corner == "L_1":
        L, done = 1, base
    else:
        done = base
        if corner == "starts_all_0":
            start = np.zeros(N, dtype=bool)
        elif corner == "starts_random":
            start = g.random(N) < 0.5
            assert start.any() and not start.all()
        else:
            steps_of = g.integers(-3, K + 4, N)
            assert (steps_of < 0).any() and (steps_of == 0).any() and (steps_of > K).any()
    env = handle(N)
    want, seqs = check_split(env, done, L, steps_of, start, what=corner)
    assert len(want) == {"all_done": K * N, "none_done": N * (K // L), "done_at_the_last_step": N * (K // L), "L_1": K * N}.get(corner, len(want))
    pick, mask = seqs.picks()
    wp, wm, _ = sd.picks(want, None, len(want), L, N)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm)
    env.check_errors()


def test_a_capacity_of_half_the_count():
    done, L, want = base_cases()[0]
    env = handle(200)
    half = len(want) // 2
    _, seqs = check_split(env, done, L, capacity=half, what="capacity %d of %d" % (half, len(want)))
    assert int(seqs.count.item()) == len(want) and seqs.capacity == half
    with pytest.raises(ValueError, match="capacity >= %d" % len(want)):
        len(seqs)
    # capacity 0 with no table only counts
    table, count = c_split(env, done, L, capacity=0)
    assert count == len(want) and (table == SENTINEL).all()
    # picks of a table that holds half: "all" with m = capacity is full, sequence `half` is out of range
    pick, mask = seqs.picks(m=half)
    wp, wm, _ = sd.picks(want[:half], None, half, L, 200)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm)
    env.check_errors()


def test_picks():
    import torch

    done, L, want = base_cases()[0]
    N, S = 200, len(base_cases()[0][2])
    env = handle(N)
    cap = S + 40
    seqs = env.split_episodes(dev(done), L, capacity=cap)
    # a shuffled selection with padding entries: rows of -1, no error
    g = np.random.default_rng(3)
    sel = g.permutation(S)[:300].astype(np.int64)
    sel[g.permutation(300)[:37]] = -1
    sel[0], sel[1], sel[2] = S - 1, 0, -5
    pick, mask = seqs.picks(sel=dev(sel))
    wp, wm, flagged = sd.picks(want, sel, 300, L, N)
    assert not flagged and (wp[sel < 0] == -1).all()
    assert pick.dtype == torch.int32 and mask.dtype == torch.bool and pick.shape == mask.shape == (300, L)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm)
    pick, _ = seqs.picks(sel=[int(v) for v in sel[:9]])  # (a list)
    assert np.array_equal(pick.cpu().numpy(), wp[:9])
    env.check_errors()
    # sel=None with m = capacity: rows beyond the count are padding, no error
    pick, mask = seqs.picks(m=cap)
    wp, wm, flagged = sd.picks(want, None, cap, L, N)
    assert not flagged and np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm) and (wp[S:] == -1).all()
    env.check_errors()
    # an entry equal to the count: a row of -1 and bit 512, reported and cleared
    sel = np.array([4, S, 5], dtype=np.int64)
    pick, mask = seqs.picks(sel=dev(sel))
    wp, wm, flagged = sd.picks(want, sel, 3, L, N)
    assert flagged and np.array_equal(pick.cpu().numpy(), wp) and (wp[1] == -1).all() and not mask[1].any()
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()
    env.check_errors()
    # gather: [K, N] and [K + 1, N, ...] data, zero at the pads
    x = torch.arange(64 * N, device="cuda", dtype=torch.float32).reshape(64, N) + 1
    got = seqs.gather(x, sel=dev(np.array([0, -1, 7])))
    wp, wm, _ = sd.picks(want, [0, -1, 7], 3, L, N)
    assert np.array_equal(got.cpu().numpy(), np.where(wm, wp + 1, 0).astype(np.float32))
    y = torch.arange(65 * N * 2, device="cuda", dtype=torch.int32).reshape(65, N, 2)
    got = seqs.gather(y, sel=[7])
    assert got.shape == (1, L, 2) and np.array_equal(got[0, :, 1].cpu().numpy(), np.where(wm[2], 2 * wp[2] + 1, 0))
    with pytest.raises(ValueError, match="not both"):
        seqs.picks(sel=[0], m=1)


def test_c_refusals():
    import memory_gym_amd
    import torch

    lib, last = memory_gym_amd._native.LIB, memory_gym_amd._native.last_error
    env = handle(200)
    done = torch.zeros((4, 200), dtype=torch.uint8, device="cuda")
    table = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    pick = torch.zeros(16, dtype=torch.int32, device="cuda")
    d, t, c = done.data_ptr(), table.data_ptr(), count.data_ptr()

    def split(done=d, steps=4, length=2, seq=t, capacity=64, count=c, h=None):
        return lib.mg_split_episodes(env._h if h is None else h, done, steps, None, None, length, seq, capacity, count, env._stream())

    assert split() == 0
    for what, kw in (("done_dev is NULL", dict(done=None)), ("count_dev is NULL", dict(count=None)), ("steps < 1", dict(steps=0)), ("length < 1", dict(length=0)),
                     ("capacity < 0", dict(capacity=-1)), ("16-byte aligned", dict(seq=None)), ("16-byte aligned", dict(seq=t + 8)),
                     ("INT32_MAX", dict(steps=(2**31 - 1) // 200))):
        assert split(**kw) == -1 and what in last(), (what, last())
    assert split(seq=None, capacity=0) == 0
    fresh = memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=200, device=0)
    assert split(h=fresh._h) == -1 and "before the first" in last()
    with pytest.raises(ValueError, match="before the first reset"):
        fresh.split_episodes(done, 2)
    fresh.close()
    assert lib.mg_sequence_picks(env._h, t, c, 64, None, 4, 4, pick.data_ptr(), None, env._stream()) == 0
    for what, args in (("count_dev is NULL", (t, None, 64, None, 4, 4, pick.data_ptr())), ("pick_dev is NULL", (t, c, 64, None, 4, 4, None)),
                       ("m < 0", (t, c, 64, None, -1, 4, pick.data_ptr())), ("length < 1", (t, c, 64, None, 4, 0, pick.data_ptr())),
                       ("capacity < 0", (t, c, -1, None, 4, 4, pick.data_ptr())), ("16-byte aligned", (t + 4, c, 64, None, 4, 4, pick.data_ptr())),
                       ("m * length > INT32_MAX", (t, c, 64, None, 1 << 16, 1 << 15, pick.data_ptr()))):
        assert lib.mg_sequence_picks(env._h, *args, None, env._stream()) == -1 and what in last(), (what, last())
    rec = env.save_frames()
    out = torch.zeros((4, 84, 84, 3), dtype=torch.uint8, device="cuda")
    pick.zero_()
    p4 = pick[:4].data_ptr()
    assert lib.mg_draw_frames_padded(env._h, rec.records.data_ptr(), 200, p4, 4, 0, out.data_ptr(), env._stream()) == 0
    for what, args in (("count < 0", (rec.records.data_ptr(), 200, p4, -1, 0, out.data_ptr())), ("rec_dev", (None, 200, p4, 4, 0, out.data_ptr())),
                       ("obs_dev", (rec.records.data_ptr(), 200, p4, 4, 0, out.data_ptr() + 4)), ("unknown format", (rec.records.data_ptr(), 200, p4, 4, 9, out.data_ptr())),
                       ("n_records < 1", (rec.records.data_ptr(), 0, p4, 4, 0, out.data_ptr())), ("count > n_records", (rec.records.data_ptr(), 2, None, 4, 0, out.data_ptr()))):
        assert lib.mg_draw_frames_padded(env._h, *args, env._stream()) == -1 and what in last() and "mg_draw_frames_padded" in last(), (what, last())
    torch.cuda.synchronize()
    env.check_errors()


# ---- 2. drawing

DRAW_IDS = ["MortarMayhem-Grid-v0", "MysteryPath-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"]  # one id per composer
_TRACES = {}


def traced(env_id):
    """-> (handle, its K = 64, N = 200 trace under the inputs of tests/test_gpu_rollout_trace.py); made once per id, the trace is never written to"""
    from test_gpu_rollout_trace import EPS, HASH_SEED, K, handles

    if env_id not in _TRACES:
        env, = handles(env_id, 1)
        ro = env.new_rollout(K)
        env.advance_traced(ro, eps=EPS, seed=HASH_SEED, step=0, render=False, stats=False)
        _TRACES[env_id] = (env, ro)
    return _TRACES[env_id]


def filled(rows, fmt, env):
    """a buffer of rows + 1 observation rows of the format, every byte PATTERN -> (the first `rows` rows, the row behind them)"""
    import torch

    _, dt, shape = env.OBS_FORMATS[fmt]
    buf = torch.empty((rows + 1,) + shape, dtype=dt, device="cuda")
    buf.view(torch.uint8).fill_(PATTERN)
    return buf[:rows], buf[rows]


def as_bytes(t):
    import torch

    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


def check_padded_rows(out, guard, pick, want_of, what):
    """rows with pick >= 0: the bytes of want_of(rows); rows with pick < 0: zero in every byte; the guard row: PATTERN in every byte"""
    import torch

    pick = pick.reshape(-1)
    flat = as_bytes(out.reshape((pick.numel(),) + tuple(out.shape[out.dim() - 3:])))
    valid = torch.nonzero(pick >= 0).flatten()
    pads = torch.nonzero(pick < 0).flatten()
    assert valid.numel() and pads.numel(), "%s: %d valid rows, %d padding rows" % (what, valid.numel(), pads.numel())
    want = as_bytes(want_of(valid))
    bad = torch.nonzero((flat[valid] != want).any(1)).flatten()
    assert not bad.numel(), "%s: %d of %d drawn rows differ, first row %d" % (what, bad.numel(), valid.numel(), int(valid[bad[0]]))
    dirty = torch.nonzero(flat[pads].any(1)).flatten()
    assert not dirty.numel(), "%s: %d of %d padding rows are not zero, first row %d" % (what, dirty.numel(), pads.numel(), int(pads[dirty[0]]))
    assert bool((guard.contiguous().view(torch.uint8) == PATTERN).all()), "%s: the row behind the last one was written" % what


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("env_id", DRAW_IDS)
def test_draw_sequences(env_id, fmt):
    import torch
    from test_gpu_rollout_trace import K, N

    env, ro = traced(env_id)
    L = 16
    seqs = env.split_episodes(ro.done, L)
    want = sd.split(ro.done.cpu().numpy(), L)
    S = len(seqs)
    assert S == len(want) and np.array_equal(seqs.table[:S].cpu().numpy(), want)
    assert (want[:, 2] < L).any() and (want[:, 2] == L).any(), "need padded and full sequences"
    out, guard = filled(S * L, fmt, env)
    c0 = env.debug_counter("padded_draws")
    obs, mask = env.draw_sequences(ro, seqs, out=out.view((S, L) + out.shape[1:]), obs_format=fmt)
    assert env.debug_counter("padded_draws") == c0 + 1
    assert obs.data_ptr() == out.data_ptr() and obs.shape == (S, L) + out.shape[1:] and mask.shape == (S, L)
    wp, wm, _ = sd.picks(want, None, S, L, N)
    assert np.array_equal(mask.cpu().numpy(), wm)
    pick = dev(wp).reshape(-1)
    check_padded_rows(obs, guard, pick, lambda rows: ro.draw(env, pick[rows] // N, pick[rows] % N, obs_format=fmt), "%s %s" % (env_id, fmt))
    if fmt == "bf16_chw":  # a selection with padding entries, drawn into a tensor of draw_sequences' own; actions and rewards beside it
        sel = dev(np.array([S - 1, -1, 0, 5, -1], dtype=np.int64))
        obs, mask = env.draw_sequences(ro, seqs, sel=sel, obs_format=fmt)
        sp, sm, _ = sd.picks(want, sel.cpu().numpy(), 5, L, N)
        assert obs.shape == (5, L, 3, 84, 84) and np.array_equal(mask.cpu().numpy(), sm) and not as_bytes(obs[1]).any() and not as_bytes(obs[4]).any()
        p = dev(sp).reshape(-1)
        rows = torch.nonzero(p >= 0).flatten()
        assert torch.equal(obs.reshape(-1, 3, 84, 84)[rows], ro.draw(env, p[rows] // N, p[rows] % N, obs_format=fmt))
        acts = seqs.gather(ro.actions, sel=sel)
        flat = ro.actions.reshape((K * N,) + tuple(ro.actions.shape[2:])).cpu().numpy()
        assert np.array_equal(acts.cpu().numpy().reshape((-1,) + flat.shape[1:])[sp.reshape(-1) >= 0], flat[sp.reshape(-1)[sp.reshape(-1) >= 0]])
    env.check_errors()


def test_draw_sequences_refuses_another_trace():
    import memory_gym_amd
    from test_gpu_rollout_trace import N

    env, ro = traced("MortarMayhem-Grid-v0")
    seqs = env.split_episodes(ro.done, 16)
    with pytest.raises(ValueError, match="steps of"):
        env.draw_sequences(memory_gym_amd.RolloutTrace(ro.frames[:33], ro.frame_layout, None, None, None, ro.done[:32]), seqs)
    with pytest.raises(ValueError, match="layout"):
        env.draw_sequences(memory_gym_amd.FrameRecords(ro.frames, ro.frame_layout + 1), seqs)
    with pytest.raises(ValueError, match="fewer than"):
        env.draw_sequences(ro.frames[:10], seqs)
    with pytest.raises(ValueError, match="EpisodeSequences"):
        env.draw_sequences(ro, seqs.table)
    with pytest.raises(ValueError, match="out must be"):
        env.draw_sequences(ro, seqs, sel=[0, 1], out=env.obs[:2 * 16].reshape(2, 16, 84, 84, 3)[:, :, :, :, :2])
    assert N == seqs.num_envs


@pytest.mark.parametrize("env_id", DRAW_IDS)
def test_padded_draw_equals_draw_frames(env_id):
    """pick=None and picks without a negative entry: draw_frames' rows; a pick at or beyond the records: its row untouched and bit 512"""
    import memory_gym_amd
    import torch
    from test_gpu_rollout_trace import N

    env, ro = traced(env_id)
    rec = memory_gym_amd.FrameRecords(ro.frames[7:9], ro.frame_layout)  # 2 N records
    for fmt in FORMATS:
        assert torch.equal(as_bytes(env.draw_frames_padded(rec, None, obs_format=fmt)), as_bytes(env.draw_frames(rec, obs_format=fmt))), fmt
        pick = (torch.arange(601, device="cuda") * 13 % (2 * N)).to(torch.int32)
        assert torch.equal(as_bytes(env.draw_frames_padded(rec, pick, obs_format=fmt)), as_bytes(env.draw_frames(rec, pick=pick, obs_format=fmt))), fmt
        env.check_errors()
        out, guard = filled(5, fmt, env)
        env.draw_frames_padded(rec, [3, 2 * N, -1, 2 * N + 9, 4], out=out, obs_format=fmt)
        direct = env.draw_frames(rec, pick=[3, 4], obs_format=fmt)
        got = as_bytes(out)
        assert torch.equal(got[[0, 4]], as_bytes(direct)) and not got[2].any() and bool((got[[1, 3]] == PATTERN).all()), fmt
        assert bool((guard.contiguous().view(torch.uint8) == PATTERN).all())
        with pytest.raises(RuntimeError, match="0x200"):
            env.check_errors()
    env.check_errors()


@pytest.mark.parametrize("arrangement", ["two_option_sets", "big_sprites", "border_composer"])
def test_padded_draw_of_the_other_composers(arrangement):
    import torch
    from test_gpu_frame_records import EPS, HASH, N, make

    if arrangement == "two_option_sets":
        env, seeds = make("MortarMayhem-Grid-v0")
        mask_a = torch.zeros(N, dtype=torch.bool, device="cuda")
        mask_a[:N // 2] = True
        env.reset(seed=seeds, options={"command_count": [3]}, mask=mask_a)
        env.reset(seed=seeds, options={"command_count": [2], "explosion_delay": [3], "explosion_duration": [1]}, mask=~mask_a)
    elif arrangement == "big_sprites":
        env, seeds = make("MysteryPath-v0")
        env.reset(seed=seeds, options={"agent_scale": 0.4})
    else:
        env, seeds = make("SearingSpotlights-v0")
        env.reset(seed=seeds, options={"black_background": True})
    for t in range(6):
        env.step(env.expert_actions(EPS, HASH, step=t))
    rec = env.save_frames()
    pick = torch.arange(3 * N, device="cuda", dtype=torch.int32) * 5 % N
    pick[::3] = -1
    pick[1] = -2**31
    for fmt in FORMATS:
        direct = env.draw_frames(rec, obs_format=fmt)
        if fmt == "u8_xyc":
            assert torch.equal(direct, env.obs), "the records do not draw the handle's own frames"
        out, guard = filled(3 * N, fmt, env)
        env.draw_frames_padded(rec, pick, out=out, obs_format=fmt)
        check_padded_rows(out, guard, pick, lambda rows: direct[pick[rows].long()], "%s %s" % (arrangement, fmt))
    env.check_errors()
    env.close()


# ---- 3. against the oracle

def test_sequences_of_the_oracles_rollout():
    import torch
    from frame_digest import as_uint64, digest_torch
    from test_gpu_rollout_trace import N, oracle_rollout

    env_id, L = "MortarMayhem-Grid-v0", 16
    rec = oracle_rollout(env_id)
    env, ro = traced(env_id)
    want = sd.split(rec["done"], L)
    assert rec["done"].any() and not rec["done"].any(0).all()  # finished and unfinished instances, by the oracle alone
    seqs = env.split_episodes(ro.done, L)
    S = len(seqs)
    assert S == len(want) and np.array_equal(seqs.table[:S].cpu().numpy(), want), "the table of the device's done against the definition on the oracle's"
    obs, mask = env.draw_sequences(ro, seqs, obs_format="u8_xyc")
    wp, wm, _ = sd.picks(want, None, S, L, N)
    assert np.array_equal(mask.cpu().numpy(), wm)
    got = as_uint64(digest_torch(obs.reshape(-1, 84, 84, 3)[dev(wm.reshape(-1))]))
    assert np.array_equal(got, rec["digest"].reshape(-1)[wp[wm]]), "digests of the drawn rows against the oracle's frames at the same (t, i)"
    env.check_errors()


# ---- 4. a captured graph

def test_split_picks_and_padded_draw_in_a_captured_graph():
    import memory_gym_amd
    import torch
    from test_gpu_rollout_trace import K, N

    env, ro = traced("MortarMayhem-Grid-v0")
    L = 16
    first = ro.done.cpu().numpy()
    second = np.random.default_rng(9).random((K, N)) < 0.05
    cap = max(sd.bound(first, L), sd.bound(second, L))
    done = ro.done.clone()
    frames = memory_gym_amd.FrameRecords(ro.frames, ro.frame_layout)
    out, guard = filled(cap * L, "u8_xyc", env)
    env.draw_frames_padded(frames, env.split_episodes(done, L, capacity=cap).picks(m=cap)[0].view(-1), out=out)  # (eager once: the handle's scratch, torch's side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seqs = env.split_episodes(done, L, capacity=cap)
        pick, mask = seqs.picks(m=cap)
        env.draw_frames_padded(frames, pick.view(-1), out=out)
    for k, content in enumerate((first, second)):
        done.copy_(dev(content))
        seqs.table.fill_(SENTINEL)
        out.view(torch.uint8).fill_(PATTERN)
        graph.replay()
        torch.cuda.synchronize()
        want = sd.split(content, L)
        S = len(want)
        assert int(seqs.count.item()) == S and np.array_equal(seqs.table[:S].cpu().numpy(), want), "replay %d: the table" % k
        assert bool((seqs.table[S:] == SENTINEL).all())
        wp, wm, _ = sd.picks(want, None, cap, L, N)
        assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm), "replay %d: picks and mask" % k
        p = pick.view(-1)
        check_padded_rows(out, guard, p, lambda rows: ro.draw(env, p[rows] // N, p[rows] % N), "replay %d" % k)
    env.check_errors()


# ---- 5. rows beyond 4 GiB

def test_padded_rows_beyond_4_gib():
    import torch
    from test_gpu_frame_records import EPS, HASH, N, make

    count, row_bytes, tail = 50800, 84 * 84 * 3 * 4, 2000
    free, _ = torch.cuda.mem_get_info()
    if free < count * row_bytes + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory for one float32 draw of %d rows, %.1f GB are free" % (
            (count * row_bytes + (1 << 30)) / 1e9, count, free / 1e9))
    assert (count - tail) * row_bytes < 2 ** 32 < (count - 12) * row_bytes  # the 4-GiB mark lies inside the alternating tail
    env, _ = make("MortarMayhem-Grid-v0")
    for t in range(6):
        env.step(env.expert_actions(EPS, HASH, step=t))
    rec = env.save_frames()
    direct = env.draw_frames(rec, obs_format="f32_chw")
    pick = (torch.arange(count, dtype=torch.int64) * 7 % N).to(torch.int32)  # a repeating pick that is no plain tiling of the store
    pick[count - tail::2] = -1
    pick = pick.cuda()
    out = torch.empty((count, 3, 84, 84), dtype=torch.float32, device="cuda")
    out[count - tail:].view(torch.uint8).fill_(PATTERN)
    env.draw_frames_padded(rec, pick, out=out, obs_format="f32_chw")
    last = out[count - tail:]
    p = pick[count - tail:]
    assert torch.equal(last[1::2], direct[p[1::2].long()]), "drawn rows either side of the 4-GiB mark"
    assert not bool(last[0::2].view(torch.uint8).any()), "padding rows either side of the 4-GiB mark"
    assert torch.equal(out[:3], direct[pick[:3].long()])
    del out, last
    env.check_errors()
    env.close()
