"""CPU tests of the memory windows' boundary (no GPU): the numpy definition (tests/window_definition.py) agrees with an independent restatement by episode
ids and has the carry property across two traces; include/memgym.h declares mg_episode_positions / mg_window_picks / mg_gather_rows_padded in plain C,
the library built here exports them, a NULL handle is refused, the Python argument checks that need no handle refuse what they must, and the host part
of csrc/mg_windows.hpp (refusals, the gather's access width) passes its stand-alone program under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import window_definition as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (1, 2, 5, 100)
LAGS = (0, 1, 3)


def two_traces():
    """N = 7, 2 x 40 steps, done drawn with probability 0.1 -> done bool [80, 7]"""
    return np.random.default_rng(20261021).random((80, 7)) < 0.1


def windows_by_episode_id(done, t, i, window, lag, back):
    """The restatement: every store row u of instance i gets an episode id by counting done -- row u + 1 belongs to the next episode when done[u] is set
    -- and the window of (t, i) is the rows u in [t - lag - W + 1, t - lag] with u >= -back and the episode id of row t.  -> the rows, ascending.
    (Rows below 0 lie in front of `done`: the caller passes a done array that begins `back` rows earlier and shifts t.)"""
    K = done.shape[0]
    ids = np.zeros(K + 1, dtype=np.int64)
    ids[1:] = np.cumsum(done[:, i] != 0)
    return [u for u in range(t - lag - window + 1, t - lag + 1) if u >= -back and u >= 0 and u <= K and ids[u] == ids[t]]


def test_the_loops_agree_with_the_restatement_by_episode_ids():
    done = two_traces()
    K2, N = done.shape
    pos = wd.positions(done)
    # pos itself: the distance to the row behind the last done, or to row 0
    for i in range(N):
        for t in range(K2 + 1):
            before = [u for u in range(t) if done[u, i]]
            assert pos[t, i] == (t - (before[-1] + 1) if before else t)
    some = 0
    for window in WINDOWS:
        for lag in LAGS:
            pick, mask, length, flagged = wd.picks(pos, None, (K2 + 1) * N, window, lag, 0)
            assert not flagged and pick.shape == (81 * N, window)
            for s in range((K2 + 1) * N):
                t, i = divmod(s, N)
                rows = windows_by_episode_id(done, t, i, window, lag, 0)
                assert length[s] == len(rows) and pick[s, :len(rows)].tolist() == [u * N + i for u in rows], (window, lag, t, i)
                assert (pick[s, len(rows):] == -1).all() and mask[s].tolist() == [True] * len(rows) + [False] * (window - len(rows))
                some += len(rows) > 0
    assert some > 4000
    # a selection: duplicates, -1 and an entry beyond the samples
    pick, mask, length, flagged = wd.picks(pos, [5, 5, -1, 81 * N, 80 * N + 6], 5, 5, 0, 0)
    assert flagged and (pick[0] == pick[1]).all() and (pick[2] == -1).all() and (pick[3] == -1).all() and length.tolist()[2:4] == [0, 0] and pick[4, length[4] - 1] == 80 * N + 6


def test_the_carry_property_across_two_traces():
    """Positions and windows of the second half with pos0 = the first half's carry and back = K equal those of the whole array, index for index: a pick of
    the whole [2K + 1, N] store IS the pick of the second call's [back + K + 1, N] store, whose row `back` is the whole store's row K."""
    done = two_traces()
    K, N = 40, done.shape[1]
    whole = wd.positions(done)
    first = wd.positions(done[:K])
    second = wd.positions(done[K:], pos0=first[K])
    assert np.array_equal(first, whole[:K + 1]) and np.array_equal(second, whole[K:])
    sel = np.arange((K + 1) * N)
    for window in WINDOWS:
        for lag in LAGS:
            p2, m2, l2, _ = wd.picks(second, sel, len(sel), window, lag, K)
            pw, mw, lw, _ = wd.picks(whole, sel + K * N, len(sel), window, lag, 0)
            assert np.array_equal(p2, pw) and np.array_equal(m2, mw) and np.array_equal(l2, lw), (window, lag)
            # a smaller back cuts the window at the store's first row and shifts the picks
            p3, _, l3, _ = wd.picks(second, sel, len(sel), window, lag, 3)
            t = sel // N
            lo_whole = t - lag - lw + 1
            assert np.array_equal(l3, np.maximum(0, lw - np.maximum(0, -3 - lo_whole) * (lw > 0)))
            keep = l3 > 0
            assert np.array_equal(p3[keep, 0], ((3 + np.maximum(lo_whole, -3)) * N + sel % N)[keep])
    # steps_of freezes a position, negative pos0 counts as 0, a position stops at INT32_MAX
    pos = wd.positions(done[:6, :4], steps_of=[0, 3, 99, -5], pos0=[7, -2, 2**31 - 1, 4])
    assert pos[:, 0].tolist() == [7] * 7 and pos[0, 1] == 0 and pos[3, 1] == pos[6, 1] and pos[:, 3].tolist() == [4] * 7
    assert pos[1, 2] == (0 if done[0, 2] else 2**31 - 1)


PROGRAM = r"""
#include <stdio.h>
#include "memgym.h"
typedef int (*pos_fn)(mg_env*, const uint8_t*, int32_t, const int32_t*, const int32_t*, int32_t*, void*);
typedef int (*picks_fn)(mg_env*, const int32_t*, int32_t, const int32_t*, int32_t, int32_t, int32_t, int32_t, int32_t*, uint8_t*, int32_t*, void*);
typedef int (*gather_fn)(mg_env*, const void*, int64_t, int64_t, const int32_t*, int64_t, void*, void*);
int main(void) {
    pos_fn a = &mg_episode_positions;
    picks_fn b = &mg_window_picks;
    gather_fn c = &mg_gather_rows_padded;
    printf("%d %u\n", a != 0 && b != 0 && c != 0, (unsigned)MG_STATE_VERSION);
    return 0;
}
"""


def test_the_header_compiles_as_c99_and_declares_the_three_functions(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler installed")
    src = tmp_path / "use_windows.c"
    src.write_text(PROGRAM)
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_windows.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("int mg_episode_positions(", "int mg_window_picks(", "int mg_gather_rows_padded(", "lo  = max(e, hi - window + 1, -back)", "#define MG_STATE_VERSION 8u",
                  "OUT OF SCOPE: sliding memory windows", "continue across two traces", "windows of their own: mg_window_picks", "episode_positions", "window_picks",
                  "row_gathers", "PACKED form"):
        assert words in header, words


def test_exports_and_the_null_handle():
    from memory_gym_amd import _native

    v, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {"mg_episode_positions": [v, v, i32, v, v, v, v], "mg_window_picks": [v, v, i32, v, i32, i32, i32, i32, v, v, v, v],
            "mg_gather_rows_padded": [v, v, i64, i64, v, i64, v, v]}
    for name, argtypes in want.items():
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert list(getattr(_native.LIB, name).argtypes) == argtypes, name
    # a NULL handle: refused before a GPU is touched
    assert _native.LIB.mg_episode_positions(None, None, 1, None, None, None, None) == -1
    assert _native.LIB.mg_window_picks(None, None, 1, None, 0, 1, 0, 0, None, None, None, None) == -1
    assert _native.LIB.mg_gather_rows_padded(None, None, 0, 1, None, 0, None, None) == -1
    assert "null handle" in _native.last_error()


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import EpisodeSequences, EpisodeWindows, VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    assert memory_gym_amd.EpisodeWindows is EpisodeWindows
    assert EpisodeWindows.__slots__ == ("pos", "window", "lag", "back", "steps", "num_envs", "_env")
    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        p = inspect.signature(cls.episode_positions).parameters
        assert list(p)[1:] == ["done", "steps", "pos0"] and [p[k].default for k in list(p)[2:]] == [None, None]
        p = inspect.signature(cls.episode_windows).parameters
        assert list(p)[1:] == ["done", "window", "lag", "back", "steps", "pos0"] and [p[k].default for k in list(p)[3:]] == [0, 0, None, None]
        p = inspect.signature(cls.gather_rows).parameters
        assert list(p)[1:] == ["x", "pick", "out"] and p["out"].default is None
        p = inspect.signature(cls.draw_windows).parameters
        assert list(p)[1:] == ["frames", "windows", "sel", "out", "obs_format"] and [p[k].default for k in list(p)[3:]] == [None, None, None]
    assert list(inspect.signature(EpisodeWindows.picks).parameters)[1:] == ["sel", "m"]
    assert list(inspect.signature(EpisodeWindows.gather).parameters)[1:] == ["x", "sel", "prefix"]
    assert list(inspect.signature(EpisodeSequences.gather).parameters)[1:] == ["x", "sel"]  # (as it was)
    text = VecMemoryGym.ERROR_BITS[512]
    assert "gather_rows" in text and "EpisodeWindows.picks" in text and "draw_windows" in text


def test_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import (EpisodeWindows, FrameRecords, RolloutTrace, check_episode_windows, check_gather_rows, check_window_frames)

    K, N, B = 6, 70, 64
    done = torch.zeros((K, N), dtype=torch.bool)
    d8, k, window, lag, back, steps, pos0 = check_episode_windows(done, 4, N)
    assert d8.dtype == torch.uint8 and d8.data_ptr() == done.data_ptr() and (k, window, lag, back, steps, pos0) == (K, 4, 0, 0, None, None)
    _, _, window, lag, back, steps, pos0 = check_episode_windows(done.view(torch.uint8), np.int64(9), N, np.int32(1), 3, torch.zeros(N, dtype=torch.int64),
                                                                 torch.ones(N, dtype=torch.int32))
    assert (window, lag, back) == (9, 1, 3) and steps.dtype == torch.int32 and pos0.dtype == torch.int32
    bad = {"float done": lambda: check_episode_windows(torch.zeros((K, N)), 4, N),
           "one-dimensional done": lambda: check_episode_windows(torch.zeros(K * N, dtype=torch.bool), 4, N),
           "another N": lambda: check_episode_windows(done, 4, N + 1),
           "K = 0": lambda: check_episode_windows(torch.zeros((0, N), dtype=torch.bool), 4, N),
           "a strided done": lambda: check_episode_windows(torch.zeros((K, 2 * N), dtype=torch.bool)[:, ::2], 4, N),
           "a numpy done": lambda: check_episode_windows(done.numpy(), 4, N),
           "window 0": lambda: check_episode_windows(done, 0, N),
           "window 2.5": lambda: check_episode_windows(done, 2.5, N),
           "window True": lambda: check_episode_windows(done, True, N),
           "lag -1": lambda: check_episode_windows(done, 4, N, -1),
           "lag 1.0": lambda: check_episode_windows(done, 4, N, 1.0),
           "back -1": lambda: check_episode_windows(done, 4, N, 0, -1),
           "float steps": lambda: check_episode_windows(done, 4, N, 0, 0, torch.zeros(N)),
           "short steps": lambda: check_episode_windows(done, 4, N, 0, 0, torch.zeros(N - 1, dtype=torch.int32)),
           "float pos0": lambda: check_episode_windows(done, 4, N, 0, 0, None, torch.zeros(N)),
           "pos0 [K + 1, N]": lambda: check_episode_windows(done, 4, N, 0, 0, None, torch.zeros((K + 1, N), dtype=torch.int32)),
           "a back beyond the int32 of a pick": lambda: check_episode_windows(done, 4, N, 0, 2**31 // N),
           "another device": lambda: check_episode_windows(done, 4, N, device=torch.device("cuda", 0))}
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")
    with pytest.raises(ValueError, match="int32 of a pick"):
        check_episode_windows(torch.zeros(1, dtype=torch.bool).expand(4, 1 << 29), 4, 1 << 29)  # (a broadcast view, 1 byte of memory)

    # an EpisodeWindows on its own: carry is row K; picks() needs the handle; gather() checks x and the prefix first
    pos = torch.arange((K + 1) * N, dtype=torch.int32).view(K + 1, N)
    w0 = EpisodeWindows(pos, 4, 0, 0, K, N)
    w3 = EpisodeWindows(pos, 4, 1, 3, K, N)
    assert torch.equal(w0.carry, pos[K]) and (w3.window, w3.lag, w3.back, w3.steps, w3.num_envs) == (4, 1, 3, K, N)
    with pytest.raises(ValueError, match="no handle"):
        w0.picks()
    x = torch.zeros((K + 1, N, 5))
    with pytest.raises(ValueError, match="prefix"):
        w3.gather(x)  # back > 0 without a prefix
    with pytest.raises(ValueError, match="prefix"):
        w3.gather(x, prefix=torch.zeros((2, N, 5)))  # a prefix of another length
    with pytest.raises(ValueError, match="prefix"):
        w3.gather(x, prefix=torch.zeros((3, N, 5), dtype=torch.float64))  # of another dtype
    with pytest.raises(ValueError, match="prefix"):
        w0.gather(x, prefix=torch.zeros((3, N, 5)))  # back = 0 with one
    for wrong in (torch.zeros((K + 2, N)), torch.zeros((K, N + 1)), torch.zeros(K)):
        with pytest.raises(ValueError, match="x must be"):
            w0.gather(wrong)
    assert tuple(w3.store(x, torch.ones((3, N, 5))).shape) == ((3 + K + 1) * N, 5) and float(w3.store(x, torch.ones((3, N, 5)))[3 * N - 1, 0]) == 1.0
    with pytest.raises(ValueError, match="no handle"):
        w3.gather(x, prefix=torch.zeros((3, N, 5)))

    # draw_windows' layout checks
    frames = torch.zeros((K + 1, N, B), dtype=torch.uint8)
    trace = RolloutTrace(frames, 5, None, None, None, None)
    assert isinstance(check_window_frames(trace, w0, B), FrameRecords) and check_window_frames(frames, w0, B) is frames
    store = FrameRecords(torch.zeros((3 + K + 1, N, B), dtype=torch.uint8), 5)
    assert check_window_frames(store, w3, B) is store
    bad = {"a trace with back > 0": lambda: check_window_frames(trace, w3, B),
           "a [K + 1] store with back > 0": lambda: check_window_frames(frames, w3, B),
           "a [back + K + 1] store with back = 0": lambda: check_window_frames(store, w0, B),
           "a trace of another K": lambda: check_window_frames(RolloutTrace(torch.zeros((K + 2, N, B), dtype=torch.uint8), 5, None, None, None, None), w0, B),
           "a trace of another N": lambda: check_window_frames(RolloutTrace(torch.zeros((K + 1, N + 1, B), dtype=torch.uint8), 5, None, None, None, None), w0, B),
           "a trace without frames": lambda: check_window_frames(RolloutTrace(None, 5, None, None, torch.zeros((K, N)), None), w0, B),
           "records of another width": lambda: check_window_frames(frames, w0, 16),
           "an int32 store": lambda: check_window_frames(frames.to(torch.int32), w0, B),
           "a strided store": lambda: check_window_frames(torch.zeros((K + 1, N, 2 * B), dtype=torch.uint8)[:, :, ::2], w0, B),
           "sequences instead of windows": lambda: check_window_frames(frames, "windows", B)}
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")

    # gather_rows
    x = torch.arange(40, dtype=torch.float32).view(10, 2, 2)
    _, pick, shape, row_bytes = check_gather_rows(x, [[0, -1, 9], [3, 3, 3]])
    assert pick.dtype == torch.int32 and tuple(pick.shape) == (2, 3) and shape == (2, 3, 2, 2) and row_bytes == 16
    assert check_gather_rows(x, None)[2:] == ((10, 2, 2), 16) and check_gather_rows(x.view(torch.uint8).view(-1)[1:8], None)[3] == 1
    bad = {"a strided x": lambda: check_gather_rows(x[:, :, 0], [0]),
           "a scalar x": lambda: check_gather_rows(torch.zeros(()), [0]),
           "rows without a byte": lambda: check_gather_rows(torch.zeros((4, 0)), [0]),
           "a float pick": lambda: check_gather_rows(x, torch.zeros(3)),
           "a float list": lambda: check_gather_rows(x, [0.5]),
           "a numpy x": lambda: check_gather_rows(x.numpy(), [0]),
           "out of another dtype": lambda: check_gather_rows(x, [0, 1], torch.zeros((2, 2, 2), dtype=torch.float64)),
           "out of another shape": lambda: check_gather_rows(x, [0, 1], torch.zeros((3, 2, 2))),
           "a strided out": lambda: check_gather_rows(x, [0, 1], torch.zeros((2, 2, 4))[:, :, ::2]),
           "another device": lambda: check_gather_rows(x, [0], device=torch.device("cuda", 0))}
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")


def test_the_host_part_of_the_kernels_header_under_the_sanitizers(tmp_path):
    """tests/host/windows_check.cpp, a stand-alone program (its own main) over the HIP-free part of csrc/mg_windows.hpp, built with
    -fsanitize=address,undefined and run as a program: the three refusal functions, the gather's access width and its choice of form."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "windows_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "windows_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
