"""GPU (-m gpu): memory windows -- mg_episode_positions / mg_window_picks / mg_gather_rows_padded (include/memgym.h), VecMemoryGym.episode_positions /
episode_windows / gather_rows / draw_windows -- against the header's definition in numpy (tests/window_definition.py), against torch's own indexing of
the same store, and against RolloutTrace.draw of the same records.  Every comparison is exact.

Positions and picks come from crafted `done` arrays: no stepping, one handle per family at N = 257, 200 and 1.  Drawing: two consecutive traced rollouts
of K = 24 at N = 48, one id per family."""
import functools

import numpy as np
import pytest

import window_definition as wd

pytestmark = pytest.mark.gpu

SENTINEL = -7   # every int32 the device must not write
PATTERN = 0xA5  # every byte the device must not write
HANDLE_IDS = {200: "MortarMayhem-Grid-v0", 257: "SearingSpotlights-v0", 1: "Endless-MysteryPath-v0"}  # one id per family
ERR_INDEX = 512
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


def dev(a, dtype=None):
    import torch

    t = torch.as_tensor(np.array(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def poll(env):
    """mg_poll_errors: the handle's error bits since the last poll (synchronises, clears them)"""
    import ctypes as C
    from memory_gym_amd import _native

    f = C.c_int()
    assert _native.LIB.mg_poll_errors(env._h, C.byref(f)) == 0, _native.last_error()
    return f.value


# ---- 1. positions

def done_cases(K, N, g):
    """name -> done bool [K, N]"""
    at_first, at_last = np.zeros((K, N), dtype=bool), np.zeros((K, N), dtype=bool)
    at_first[0], at_last[K - 1] = True, True
    return {"zeros": np.zeros((K, N), dtype=bool), "ones": np.ones((K, N), dtype=bool), "done at t = 0": at_first, "done at t = K - 1": at_last,
            "random": g.random((K, N)) < 0.1}


def c_positions(env, done, steps_of=None, pos0=None):
    """mg_episode_positions through the C ABI into [K + 2, N] rows filled with SENTINEL -> the rows on the host"""
    import torch
    from memory_gym_amd import _native

    K, N = done.shape
    d = dev(done, torch.uint8)
    s = None if steps_of is None else dev(steps_of, torch.int32)
    p = None if pos0 is None else dev(pos0, torch.int32)
    pos = torch.full((K + 2, N), SENTINEL, dtype=torch.int32, device="cuda")
    rc = _native.LIB.mg_episode_positions(env._h, d.data_ptr(), K, None if s is None else s.data_ptr(), None if p is None else p.data_ptr(), pos.data_ptr(),
                                          env._stream())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return pos.cpu().numpy()


@pytest.mark.parametrize("K,N", [(37, 257), (37, 200), (37, 1), (1030, 257), (1030, 1)])
def test_positions_equal_the_loops_in_every_entry(K, N):
    import torch

    env = handle(N)
    g = np.random.default_rng(1000 * K + N)
    before = env.debug_counter("episode_positions")
    calls = 0
    for name, done in done_cases(K, N, g).items():
        pos0 = g.integers(-5, 9, N)          # zeros, negatives, small values
        pos0[g.random(N) < 0.3] = 0
        pos0[g.random(N) < 0.2] = 5 * K + 11  # larger than any back
        steps_of = g.integers(-3, K + 4, N)   # 0, K, beyond K and negative entries among them
        steps_of[:4] = [0, K, K + 2, -1][:N]
        for so, p0 in ((None, None), (None, pos0), (steps_of, None), (steps_of, pos0)):
            want = wd.positions(done, so, p0)
            got = c_positions(env, done, so, p0)
            calls += 1
            bad = np.argwhere(got[:K + 1] != want)
            assert not len(bad), "%s (steps_of %s, pos0 %s): %d entries differ, first at %s: %d against %d" % (
                name, so is not None, p0 is not None, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
            assert (got[K + 1] == SENTINEL).all(), "%s: the row behind the carry row was written" % name
        # the Python mirror, int64 arguments, a bool done
        pos = env.episode_positions(dev(done), steps=dev(steps_of, torch.int64), pos0=dev(pos0, torch.int64))
        calls += 1
        assert pos.dtype == torch.int32 and tuple(pos.shape) == (K + 1, N) and np.array_equal(pos.cpu().numpy(), want), name  # (want: the last pair)
    assert env.debug_counter("episode_positions") == before + calls
    env.check_errors()


def test_positions_carry_across_two_traces():
    """the carry-out of the first half as pos0 of the second: the positions of the whole array"""
    K, N = 37, 257
    env = handle(N)
    done = np.random.default_rng(5).random((2 * K, N)) < 0.1
    first = env.episode_windows(dev(done[:K]), 4)
    second = env.episode_windows(dev(done[K:]), 4, lag=1, back=K, pos0=first.carry)
    whole = wd.positions(done)
    assert np.array_equal(first.pos.cpu().numpy(), whole[:K + 1]) and np.array_equal(second.pos.cpu().numpy(), whole[K:])
    assert np.array_equal(second.carry.cpu().numpy(), whole[2 * K])
    # and the windows of the second half are the whole array's, index for index
    sel = np.random.default_rng(6).permutation((K + 1) * N)[:500]
    pick, mask, length = second.picks(sel=dev(sel))
    wp, wm, wl, _ = wd.picks(whole, sel + K * N, len(sel), 4, 1, 0)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(length.cpu().numpy(), wl)
    env.check_errors()


def test_positions_refusals():
    import memory_gym_amd
    import torch
    from memory_gym_amd import _native

    lib, last = _native.LIB, _native.last_error
    fresh = memory_gym_amd.make(HANDLE_IDS[1], num_envs=1, device=0)
    d = torch.zeros((4, 1), dtype=torch.uint8, device="cuda")
    pos = torch.zeros((5, 1), dtype=torch.int32, device="cuda")
    assert lib.mg_episode_positions(fresh._h, d.data_ptr(), 4, None, None, pos.data_ptr(), None) == -1 and "before the first" in last()
    fresh.close()
    env = handle(1)
    for what, args in (("done_dev", (None, 4, None, None, pos.data_ptr())), ("pos_dev", (d.data_ptr(), 4, None, None, None)),
                       ("steps < 1", (d.data_ptr(), 0, None, None, pos.data_ptr()))):
        assert lib.mg_episode_positions(env._h, *args, env._stream()) == -1 and what in last() and "mg_episode_positions" in last(), (what, last())
    pk = torch.zeros((5, 3), dtype=torch.int32, device="cuda")
    for what, args in (("pos_dev", (None, 4, None, 5, 3, 0, 0, pk.data_ptr())), ("pick_dev", (pos.data_ptr(), 4, None, 5, 3, 0, 0, None)),
                       ("steps < 1", (pos.data_ptr(), 0, None, 5, 3, 0, 0, pk.data_ptr())), ("m < 0", (pos.data_ptr(), 4, None, -1, 3, 0, 0, pk.data_ptr())),
                       ("window < 1", (pos.data_ptr(), 4, None, 5, 0, 0, 0, pk.data_ptr())), ("lag < 0", (pos.data_ptr(), 4, None, 5, 3, -1, 0, pk.data_ptr())),
                       ("back < 0", (pos.data_ptr(), 4, None, 5, 3, 0, -1, pk.data_ptr())), ("sel_dev is NULL", (pos.data_ptr(), 4, None, 6, 3, 0, 0, pk.data_ptr())),
                       ("m * window", (pos.data_ptr(), 4, pk.data_ptr(), 1 << 16, 1 << 15, 0, 0, pk.data_ptr())),
                       ("(back + steps + 1)", (pos.data_ptr(), 4, None, 5, 3, 0, 2**31 - 1, pk.data_ptr()))):
        assert lib.mg_window_picks(env._h, *args, None, None, env._stream()) == -1 and what in last() and "mg_window_picks" in last(), (what, last())
    x = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for what, args in (("count < 0", (x.data_ptr(), 4, 64, None, -1, x.data_ptr() + 1024)), ("row_bytes < 1", (x.data_ptr(), 4, 0, None, 1, x.data_ptr() + 1024)),
                       ("count > n_rows", (x.data_ptr(), 4, 64, None, 5, x.data_ptr() + 1024)), ("dst_dev", (x.data_ptr(), 4, 64, None, 1, None)),
                       ("src_dev", (None, 4, 64, None, 1, x.data_ptr())), ("overlap", (x.data_ptr(), 4, 64, pk.data_ptr(), 9, x.data_ptr() + 255)),
                       ("overlap", (x.data_ptr() + 64, 4, 64, pk.data_ptr(), 2, x.data_ptr()))):
        assert lib.mg_gather_rows_padded(env._h, *args, env._stream()) == -1 and what in last() and "mg_gather_rows_padded" in last(), (what, last())
    assert lib.mg_gather_rows_padded(env._h, x.data_ptr(), 4, 64, pk.data_ptr(), 0, None, env._stream()) == 0  # nothing to do
    torch.cuda.synchronize()
    env.check_errors()


# ---- 2. picks

def c_picks(env, pos, sel, m, window, lag, back, with_mask=True):
    """mg_window_picks through the C ABI into m + 1 rows filled with SENTINEL / PATTERN -> (pick [m + 1, W], mask [m + 1, W], len [m + 1]) on the host"""
    import torch
    from memory_gym_amd import _native

    K = pos.shape[0] - 1
    pick = torch.full((m + 1, window), SENTINEL, dtype=torch.int32, device="cuda")
    mask = torch.full((m + 1, window), PATTERN, dtype=torch.uint8, device="cuda")
    length = torch.full((m + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = _native.LIB.mg_window_picks(env._h, pos.data_ptr(), K, None if sel is None else sel.data_ptr(), m, window, lag, back, pick.data_ptr(),
                                     mask.data_ptr() if with_mask else None, length.data_ptr() if with_mask else None, env._stream())
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    return pick.cpu().numpy(), mask.cpu().numpy(), length.cpu().numpy()


def check_picks(env, pos_host, pos, sel_host, m, window, lag, back, what):
    import torch

    sel = None if sel_host is None else dev(sel_host, torch.int32)
    wp, wm, wl, flagged = wd.picks(pos_host, sel_host, m, window, lag, back)
    pick, mask, length = c_picks(env, pos, sel, m, window, lag, back)
    bad = np.argwhere((pick[:m] != wp).any(1)).flatten()
    assert not len(bad), "%s: %d of %d rows differ, first row %d: %s against %s" % (what, len(bad), m, bad[0], pick[bad[0]], wp[bad[0]])
    assert np.array_equal(mask[:m], wm.astype(np.uint8)) and np.array_equal(length[:m], wl), what
    assert (pick[m] == SENTINEL).all() and (mask[m] == PATTERN).all() and length[m] == SENTINEL, "%s: the entry behind the last row was written" % what
    assert (poll(env) == ERR_INDEX) == flagged, what
    return wp, flagged


@functools.lru_cache(maxsize=None)
def pick_positions(K, N):
    """-> positions of a random done [K, N] whose episodes reach into the previous trace (pos0 up to K + 9); computed once, never written to"""
    g = np.random.default_rng(77 * K + N)
    pos = wd.positions(g.random((K, N)) < 0.1, None, g.integers(0, K + 10, N))
    pos.setflags(write=False)
    return pos


@pytest.mark.parametrize("back_of", ["0", "3", "K"])
@pytest.mark.parametrize("K,N", [(37, 200), (37, 257), (37, 1), (1030, 257)])
def test_picks_equal_the_loops(K, N, back_of):
    """window in {1, 2, 5, K + back + 3} x lag in {0, 1, window, window + 2}: sel = None over every sample (K = 37), a selection with duplicates and -1
    entries, and one with entries at and beyond (K + 1) * N -- bit 512, rows of -1"""
    import torch

    env = handle(N)
    back = {"0": 0, "3": 3, "K": K}[back_of]
    pos_host = pick_positions(K, N)
    pos = dev(pos_host)
    samples = (K + 1) * N
    g = np.random.default_rng(K + N + back)
    some = g.integers(0, samples, 300)
    some[5:40:3] = some[4]  # duplicates
    some[::7] = -1
    some[-1], some[-2] = samples - 1, 0
    beyond = g.integers(0, samples, 40)
    beyond[[3, 17, 39]] = [samples, samples + 12345, 2**31 - 1]
    beyond[8] = -1
    before = env.debug_counter("window_picks")
    calls = 0
    every = K == 37  # sel = None over every sample: where the loops take well under a second
    for window in (1, 2, 5, K + back + 3):
        for lag in (0, 1, window, window + 2):
            what = "K %d, N %d, window %d, lag %d, back %d" % (K, N, window, lag, back)
            if every:
                check_picks(env, pos_host, pos, None, samples, window, lag, back, what + ", every sample")
                calls += 1
            wp, _ = check_picks(env, pos_host, pos, some, len(some), window, lag, back, what + ", a selection")
            assert (wp[::7] == -1).all()
            wp, flagged = check_picks(env, pos_host, pos, beyond, len(beyond), window, lag, back, what + ", entries beyond the samples")
            assert flagged and (wp[[3, 17, 39, 8]] == -1).all()
            calls += 2
    # without a mask and a length; m = 0
    wp, _, _, _ = wd.picks(pos_host, some, len(some), 5, 1, back)
    assert np.array_equal(c_picks(env, pos, dev(some, torch.int32), len(some), 5, 1, back, with_mask=False)[0][:len(some)], wp)
    c_picks(env, pos, None, 0, 5, 1, back)
    assert env.debug_counter("window_picks") == before + calls + 2
    env.check_errors()


def test_picks_of_the_python_mirror():
    import torch

    K, N = 37, 200
    env = handle(N)
    g = np.random.default_rng(3)
    done = g.random((K, N)) < 0.1
    pos0 = g.integers(0, 30, N)
    win = env.episode_windows(dev(done), 5, lag=1, back=3, pos0=dev(pos0))
    pos_host = wd.positions(done, None, pos0)
    assert (win.window, win.lag, win.back, win.steps, win.num_envs) == (5, 1, 3, K, N) and np.array_equal(win.pos.cpu().numpy(), pos_host)
    pick, mask, length = win.picks()  # every sample
    wp, wm, wl, _ = wd.picks(pos_host, None, (K + 1) * N, 5, 1, 3)
    assert pick.dtype == torch.int32 and mask.dtype == torch.bool and length.dtype == torch.int32
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(length.cpu().numpy(), wl)
    pick, _, _ = win.picks(m=N + 3)
    assert np.array_equal(pick.cpu().numpy(), wp[:N + 3])
    sel = [5, 5, -1, K * N + 7]
    pick, mask, length = win.picks(sel=sel)  # (a list)
    wp, wm, wl, _ = wd.picks(pos_host, sel, 4, 5, 1, 3)
    assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(length.cpu().numpy(), wl)
    env.check_errors()
    with pytest.raises(ValueError):
        win.picks(m=(K + 1) * N + 1)
    with pytest.raises(ValueError):
        win.picks(sel=sel, m=4)
    win.picks(sel=[(K + 1) * N])
    with pytest.raises(RuntimeError, match="0x200"):
        env.check_errors()


# ---- 3. gather

def region(nbytes, offset, fill=None):
    """`nbytes` bytes that begin `offset` bytes behind a 256-byte aligned address, inside a larger uint8 tensor -> (the region, the whole tensor)"""
    import torch

    whole = torch.empty(nbytes + 512, dtype=torch.uint8, device="cuda")
    if fill is not None:
        whole.fill_(fill)
    lead = (-whole.data_ptr()) % 256 + offset
    part = whole[lead:lead + nbytes]
    assert part.data_ptr() % 256 == offset
    return part, whole


@pytest.mark.parametrize("row_bytes", [1, 2, 4, 6, 16, 48, 768, 4100])
def test_gathered_rows_equal_torchs_indexing(row_bytes):
    """bases aligned to 16 and offset by 2 and by 1 byte on either side (the narrow forms); pads are zero in every byte, a row whose pick is out of range
    is untouched and raises bit 512, the row behind the last one is untouched, pick = None equals a copy"""
    import torch

    env = handle(257)
    R, count = 301, 1003
    g = np.random.default_rng(row_bytes)
    before = env.debug_counter("row_gathers")
    calls = 0
    for src_off, dst_off in ((0, 0), (2, 0), (0, 2), (2, 2), (1, 0), (0, 1), (16, 8), (4, 0)):
        what = "%d-byte rows, src + %d, dst + %d" % (row_bytes, src_off, dst_off)
        src, _ = region(R * row_bytes, src_off)
        src.copy_(dev(g.integers(0, 256, R * row_bytes, dtype=np.uint8)))
        x = src.view(R, row_bytes)
        pick_host = g.integers(0, R, count)
        pick_host[g.random(count) < 0.1] = -1
        pick_host[[0, 1, count - 1]] = [R - 1, 0, -1]
        pick = dev(pick_host, torch.int32)
        dst, whole = region((count + 1) * row_bytes, dst_off, PATTERN)
        out = dst[:count * row_bytes].view(count, row_bytes)
        got = env.gather_rows(x, pick, out=out)
        calls += 1
        assert got.data_ptr() == out.data_ptr()
        valid, pads = torch.nonzero(pick >= 0).flatten(), torch.nonzero(pick < 0).flatten()
        assert valid.numel() > 800 and pads.numel() > 50
        assert torch.equal(out[valid], x[pick[valid].long()]), what + ": gathered rows"
        assert not bool(out[pads].any()), what + ": a pad row is not zero"
        lead = dst.data_ptr() - whole.data_ptr()
        assert bool((whole[:lead] == PATTERN).all()) and bool((whole[lead + count * row_bytes:] == PATTERN).all()), what + ": bytes around the rows were written"
        assert poll(env) == 0, what
        # picks at and beyond the rows: untouched, bit 512
        out.fill_(PATTERN)
        pick2 = pick.clone()
        pick2[[2, 500, count - 1]] = torch.tensor([R, R + 77, 2**31 - 1], dtype=torch.int32, device="cuda")
        env.gather_rows(x, pick2, out=out)
        calls += 1
        skipped = torch.tensor([2, 500, count - 1], device="cuda")
        assert bool((out[skipped] == PATTERN).all()), what + ": a row whose pick is out of range was written"
        ok = torch.nonzero((pick2 >= 0) & (pick2 < R)).flatten()
        assert torch.equal(out[ok], x[pick2[ok].long()]) and not bool(out[torch.nonzero(pick2 < 0).flatten()].any()), what
        assert bool((whole[lead + count * row_bytes:] == PATTERN).all()), what + ": the row behind the last one was written"
        assert poll(env) == ERR_INDEX, what + ": bit 512"
        # pick = None: a copy
        out.fill_(PATTERN)
        env.gather_rows(x, None, out=out[:R])
        calls += 1
        assert torch.equal(out[:R], x) and bool((out[R:] == PATTERN).all()), what + ": pick = None"
    assert env.debug_counter("row_gathers") == before + calls
    env.check_errors()


def test_gather_of_typed_rows_and_pick_shapes():
    """x of any dtype and trailing shape, a pick of any shape; the packed form beyond one grid of lanes (17 M four-byte rows)"""
    import torch

    env = handle(200)
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn((50, 3, 64), dtype=torch.float32, device="cuda", generator=g)  # 768-byte rows
    pick = torch.randint(-1, 50, (7, 11), device="cuda", generator=g)               # int64 [7, 11]
    out = env.gather_rows(x, pick)
    want = torch.where((pick >= 0)[:, :, None, None], x[pick.clamp(min=0)], torch.zeros((), device="cuda"))
    assert tuple(out.shape) == (7, 11, 3, 64) and out.dtype == x.dtype and torch.equal(out, want)
    assert tuple(env.gather_rows(x, torch.zeros((0,), dtype=torch.int32, device="cuda")).shape) == (0, 3, 64)
    h = torch.randn((40, 5), dtype=torch.bfloat16, device="cuda", generator=g)      # 10-byte rows
    assert torch.equal(env.gather_rows(h, [[0, 39], [-1, 7]]), torch.stack((h[[0, 39]], torch.stack((torch.zeros_like(h[0]), h[7])))))
    r = torch.arange(1000, dtype=torch.int32, device="cuda") * 3 + 1
    count = 17_000_001
    big = torch.randint(-1, 1000, (count,), dtype=torch.int32, device="cuda", generator=g)
    out = env.gather_rows(r, big)
    assert torch.equal(out, torch.where(big >= 0, big * 3 + 1, torch.zeros_like(big)))
    env.check_errors()


def test_gathered_rows_beyond_4_gib():
    """1,100,000 rows of 4,096 bytes (4.5 GB) gathered from a 1,000-row source; the last 2,000 rows alternate pad and record"""
    import torch

    count, row_bytes, R, tail = 1_100_000, 4096, 1000, 2000
    free, _ = torch.cuda.mem_get_info()
    if free < count * row_bytes + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory, %.1f GB are free" % ((count * row_bytes + (1 << 30)) / 1e9, free / 1e9))
    assert (count - tail) * row_bytes > 2 ** 32
    env = handle(200)
    x = torch.randint(0, 2**31 - 1, (R, row_bytes // 4), dtype=torch.int32, device="cuda")
    pick = (torch.arange(count, dtype=torch.int64) * 7 % R).to(torch.int32)
    pick[count - tail::2] = -1
    pick = pick.cuda()
    out = torch.empty((count, row_bytes // 4), dtype=torch.int32, device="cuda")
    out[count - tail:].fill_(SENTINEL)
    env.gather_rows(x, pick, out=out)
    last, p = out[count - tail:], pick[count - tail:]
    assert torch.equal(last[1::2], x[p[1::2].long()]), "gathered rows beyond the 4-GiB mark"
    assert not bool(last[0::2].any()), "pad rows beyond the 4-GiB mark"
    assert torch.equal(out[:3000], x[pick[:3000].long()])
    mid = (2 ** 32) // row_bytes
    assert torch.equal(out[mid - 50:mid + 50], x[pick[mid - 50:mid + 50].long()]), "rows either side of the 4-GiB mark"
    del out, last
    env.check_errors()


def test_window_gather_with_a_prefix():
    """EpisodeWindows.gather: hidden states of two consecutive rollouts, lag = 1, back = 8 -- the window of a sample holds the rows of the whole store"""
    import torch

    K, N, W, back = 37, 200, 6, 8
    env = handle(N)
    g = np.random.default_rng(8)
    done = g.random((2 * K, N)) < 0.1
    hidden = torch.randn((2 * K + 1, N, 24), device="cuda")  # the whole store: row K of the first rollout is row 0 of the second
    first = env.episode_windows(dev(done[:K]), W, lag=1)
    second = env.episode_windows(dev(done[K:]), W, lag=1, back=back, pos0=first.carry)
    sel = dev(g.permutation((K + 1) * N)[:400])
    sel[::9] = -1
    got = second.gather(hidden[K:], sel=sel, prefix=hidden[K - back:K])
    whole = wd.positions(done)
    sel_host = sel.cpu().numpy()
    wp, wm, wl, _ = wd.picks(whole[K:], sel_host, len(sel_host), W, 1, back)
    flat = hidden[K - back:].reshape(-1, 24)
    want = torch.where(dev(wm)[:, :, None], flat[dev(wp).clamp(min=0).long()], torch.zeros((), device="cuda"))
    assert tuple(got.shape) == (400, W, 24) and torch.equal(got, want)
    # the same rows named in the whole store
    wp2, _, _, _ = wd.picks(whole, np.where(sel_host >= 0, sel_host + K * N, -1), len(sel_host), W, 1, 0)
    assert torch.equal(got, torch.where(dev(wp2 >= 0)[:, :, None], hidden.reshape(-1, 24)[dev(wp2).clamp(min=0).long()], torch.zeros((), device="cuda")))
    env.check_errors()


# ---- 4. draw_windows

@pytest.mark.parametrize("env_id", ["MortarMayhem-Grid-v0", "Endless-MysteryPath-v0", "SearingSpotlights-v0"])
def test_drawn_windows_are_the_traces_frames(env_id):
    """two traced rollouts of K = 24 at N = 48, back = 8: every valid row of a window is bit for bit RolloutTrace.draw of the same record, in the first or
    the second trace according to its row; every pad row is zero; len equals the loops' value on the traces' own done"""
    import memory_gym_amd
    import torch

    K, N, W, back, M = 24, 48, 12, 8, 96
    env = memory_gym_amd.make(env_id, num_envs=N, device=0)
    try:
        env.reset(seed=np.arange(N, dtype=np.int64) + 100)
        ro = [env.new_rollout(K), env.new_rollout(K)]
        env.advance_traced(ro[0], eps=0.4, seed=11, step=0, render=False, stats=False)
        env.advance_traced(ro[1], eps=0.4, seed=11, step=K, render=False, stats=False)
        assert torch.equal(ro[1].frames[0], ro[0].frames[K])
        first = env.episode_windows(ro[0].done, W)
        win = env.episode_windows(ro[1].done, W, back=back, pos0=first.carry)
        store = memory_gym_amd.FrameRecords(torch.cat((ro[0].frames[K - back:K], ro[1].frames)), env.frame_layout())
        done = np.concatenate((ro[0].done.cpu().numpy(), ro[1].done.cpu().numpy()))
        whole = wd.positions(done)
        sel_host = np.random.default_rng(12).permutation((K + 1) * N)[:M]
        sel_host[:6] = np.arange(6)  # samples of row 0: their windows lie in the previous trace but for one row
        sel_host[6] = -1
        wp, wm, wl, _ = wd.picks(whole[K:], sel_host, M, W, 0, back)
        assert 0 < int(wm.sum()) < M * W and (wp[wm] < back * N).any() and (wp[wm] >= back * N).any()
        for fmt in ("u8_xyc", "bf16_chw"):
            _, dt, shape = env.OBS_FORMATS[fmt]
            buf = torch.empty((M * W + 1,) + shape, dtype=dt, device="cuda")
            buf.view(torch.uint8).fill_(PATTERN)
            obs, mask, length = env.draw_windows(store, win, sel=dev(sel_host), out=buf[:M * W].view((M, W) + shape), obs_format=fmt)
            assert np.array_equal(length.cpu().numpy(), wl) and np.array_equal(mask.cpu().numpy(), wm), fmt
            flat = obs.reshape((M * W,) + shape)
            p = dev(wp.reshape(-1)).long()
            valid, pads = torch.nonzero(p >= 0).flatten(), torch.nonzero(p < 0).flatten()
            row, inst = p[valid] // N, p[valid] % N
            for k, (rows_of, t_of) in enumerate(((row < back, row + (K - back)), (row >= back, row - back))):
                at = torch.nonzero(rows_of).flatten()
                assert at.numel()
                want = ro[k].draw(env, t_of[at], inst[at], obs_format=fmt)
                assert torch.equal(flat[valid[at]], want), "%s: rows of trace %d" % (fmt, k)
            assert not bool(flat[pads].view(torch.uint8).any()), fmt + ": a pad row is not zero"
            assert bool((buf[M * W].view(torch.uint8) == PATTERN).all()), fmt + ": the row behind the last one was written"
        # back = 0: the trace itself as frames
        inside = env.episode_windows(ro[1].done, 3, pos0=first.carry)
        obs, mask, length = env.draw_windows(ro[1], inside, sel=[K * N + 5, 0, -1])
        wp, wm, wl, _ = wd.picks(whole[K:], [K * N + 5, 0, -1], 3, 3, 0, 0)
        assert np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(length.cpu().numpy(), wl) and wl[1] == 1
        assert torch.equal(obs[1, 0], ro[1].draw(env, 0, 0)[0]) and not bool(obs[1, 1:].any()) and not bool(obs[2].any())
        assert torch.equal(obs[0, wl[0] - 1], ro[1].draw(env, K, 5)[0])
        with pytest.raises(ValueError):
            env.draw_windows(ro[1], win)  # a trace with back > 0
        env.check_errors()
    finally:
        env.close()


# ---- 5. a captured graph

def test_positions_picks_and_gather_in_a_captured_graph():
    """after one uncaptured call, positions, picks and gather are captured on the handle's stream and replayed with done and sel changed in place"""
    import torch

    K, N, W, back, M = 37, 257, 5, 3, 300
    env = handle(N)
    g = np.random.default_rng(21)
    contents = [(g.random((K, N)) < 0.1, g.integers(-1, (K + 1) * N, M)) for _ in range(2)]
    pos0_host = g.integers(0, 20, N)
    done, sel, pos0 = dev(contents[0][0]), dev(contents[0][1], torch.int32), dev(pos0_host, torch.int32)
    store = torch.randn(((back + K + 1) * N, 192), device="cuda")  # 768-byte rows

    def run():
        win = env.episode_windows(done, W, lag=1, back=back, pos0=pos0)
        pick, mask, length = win.picks(sel=sel)
        return win.pos, pick, mask, length, env.gather_rows(store, pick)

    run()  # eager once
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pos, pick, mask, length, rows = run()
    for k, (d, s) in enumerate(reversed(contents)):
        done.copy_(dev(d))
        sel.copy_(dev(s, torch.int32))
        rows.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        want = wd.positions(d, None, pos0_host)
        wp, wm, wl, flagged = wd.picks(want, s, M, W, 1, back)
        assert not flagged and np.array_equal(pos.cpu().numpy(), want), "replay %d: positions" % k
        assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(length.cpu().numpy(), wl), "replay %d: picks" % k
        assert torch.equal(rows, torch.where(dev(wm)[:, :, None], store[dev(wp).clamp(min=0).long()], torch.zeros((), device="cuda"))), "replay %d: rows" % k
    env.check_errors()
