"""CPU tests of the episode sequences' boundary (no GPU): include/memgym.h declares mg_sequence / mg_split_episodes / mg_sequence_picks /
mg_draw_frames_padded in plain C, the library built here exports them, the ctypes mirror of the struct has the header's size and field offsets, the
argument checks that need no handle refuse what they must, and the numpy definition (tests/sequence_definition.py) reproduces a hand-written example."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sequence_definition as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["instance", "t0", "len", "flags"]

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "memgym.h"
typedef int (*split_fn)(mg_env*, const uint8_t*, int32_t, const int32_t*, const uint8_t*, int32_t, mg_sequence*, int32_t, int32_t*, void*);
typedef int (*picks_fn)(mg_env*, const mg_sequence*, const int32_t*, int32_t, const int32_t*, int32_t, int32_t, int32_t*, uint8_t*, void*);
typedef int (*draw_fn)(mg_env*, const void*, int64_t, const int32_t*, int64_t, int, void*, void*);
int main(void) {
    split_fn s = &mg_split_episodes;
    picks_fn p = &mg_sequence_picks;
    draw_fn d = &mg_draw_frames_padded;
    mg_sequence q;
    q.instance = 3;
    q.t0 = 16;
    q.len = 5;
    q.flags = MG_SEQ_FIRST | MG_SEQ_LAST;
    printf("%u %u %u %u %u %d %d\n", (unsigned)sizeof q, (unsigned)offsetof(mg_sequence, instance), (unsigned)offsetof(mg_sequence, t0),
           (unsigned)offsetof(mg_sequence, len), (unsigned)offsetof(mg_sequence, flags), q.flags, s != 0 && p != 0 && d != 0 && q.instance + q.t0 + q.len == 24);
    return 0;
}
"""


def test_the_ctypes_mirror_has_the_headers_layout(tmp_path):
    """A C99 program that includes nothing of HIP fills an mg_sequence, takes the addresses of the three entry points (their types are checked against
    the declarations; nothing is linked in) and prints the struct's size and field offsets: 16 bytes, and those of _native.Sequence."""
    from memory_gym_amd import _native

    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler installed")
    src = tmp_path / "use_sequences.c"
    src.write_text(PROGRAM)
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_sequences.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    # the layout: the same program with the three addresses left out, so that it links without the library
    src2, exe = tmp_path / "layout.c", tmp_path / "layout"
    src2.write_text(PROGRAM.replace("&mg_split_episodes", "(split_fn)1").replace("&mg_sequence_picks", "(picks_fn)1").replace("&mg_draw_frames_padded", "(draw_fn)1"))
    p = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [f[0] for f in _native.Sequence._fields_] == FIELDS
    assert out[0] == 16 == C.sizeof(_native.Sequence)
    assert out[1:5] == [getattr(_native.Sequence, f).offset for f in FIELDS] == [0, 4, 8, 12]
    assert out[5] == (_native.MG_SEQ_FIRST | _native.MG_SEQ_LAST) == 3 and (sd.MG_SEQ_FIRST, sd.MG_SEQ_LAST) == (1, 2)
    assert out[6] == 1


def test_header_and_exports_agree():
    from memory_gym_amd import _native

    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("int mg_split_episodes(", "int mg_sequence_picks(", "int mg_draw_frames_padded(", "typedef struct mg_sequence", "#define MG_SEQ_FIRST 1",
                  "#define MG_SEQ_LAST  2", "num_envs * ceil(steps / length)", "no atomic decides", "OUT OF SCOPE: sliding memory windows", "continue across two traces",
                  "#define MG_STATE_VERSION 8u", "sequence_splits", "padded_draws"):
        assert words in header, words
    v, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {"mg_split_episodes": [v, v, i32, v, v, i32, v, i32, v, v], "mg_sequence_picks": [v, v, v, i32, v, i32, i32, v, v, v],
            "mg_draw_frames_padded": [v, v, i64, v, i64, C.c_int, v, v]}
    for name, argtypes in want.items():
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert list(getattr(_native.LIB, name).argtypes) == argtypes, name
    assert list(_native.LIB.mg_draw_frames_padded.argtypes) == list(_native.LIB.mg_draw_frames.argtypes)
    # a NULL handle: refused before a GPU is touched
    assert _native.LIB.mg_split_episodes(None, None, 1, None, None, 1, None, 0, None, None) == -1
    assert _native.LIB.mg_sequence_picks(None, None, None, 0, None, 0, 1, None, None, None) == -1
    assert _native.LIB.mg_draw_frames_padded(None, None, 0, None, 0, 0, None, None) == -1


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import EpisodeSequences, VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    assert memory_gym_amd.EpisodeSequences is EpisodeSequences
    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        p = inspect.signature(cls.split_episodes).parameters
        assert list(p)[1:] == ["done", "length", "steps", "starts", "capacity"] and [p[k].default for k in list(p)[3:]] == [None, None, None]
        p = inspect.signature(cls.draw_frames_padded).parameters
        assert list(p)[1:] == ["records", "pick", "out", "obs_format"] and [p[k].default for k in list(p)[3:]] == [None, None]
        p = inspect.signature(cls.draw_sequences).parameters
        assert list(p)[1:] == ["frames", "seqs", "sel", "out", "obs_format"] and [p[k].default for k in list(p)[3:]] == [None, None, None]
    assert list(inspect.signature(VecMemoryGym.draw_frames).parameters)[1:] == ["records", "pick", "out", "obs_format"]  # (as it was)
    assert list(inspect.signature(EpisodeSequences.picks).parameters)[1:] == ["sel", "m"]
    assert list(inspect.signature(EpisodeSequences.gather).parameters)[1:] == ["x", "sel"]
    assert "synchronises" in VecMemoryGym.split_episodes.__doc__
    text = VecMemoryGym.ERROR_BITS[512]
    assert "draw_frames" in text and "draw_frames_padded" in text and "draw_sequences" in text and "picks" in text


def test_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import EpisodeSequences, check_split_episodes

    K, N = 6, 70
    done = torch.zeros((K, N), dtype=torch.bool)
    d8, k, length, steps, starts, cap = check_split_episodes(done, 4, N)
    assert d8.dtype == torch.uint8 and d8.data_ptr() == done.data_ptr() and (k, length, steps, starts, cap) == (K, 4, None, None, None)
    d8, k, length, steps, starts, cap = check_split_episodes(done.view(torch.uint8), np.int64(4), N, torch.zeros(N, dtype=torch.int64),
                                                              torch.ones(N, dtype=torch.bool), 17)
    assert steps.dtype == torch.int32 and starts.dtype == torch.uint8 and cap == 17
    bad = {"float done": lambda: check_split_episodes(torch.zeros((K, N)), 4, N),
           "one-dimensional done": lambda: check_split_episodes(torch.zeros(K * N, dtype=torch.bool), 4, N),
           "another N": lambda: check_split_episodes(done, 4, N + 1),
           "K = 0": lambda: check_split_episodes(torch.zeros((0, N), dtype=torch.bool), 4, N),
           "a strided done": lambda: check_split_episodes(torch.zeros((K, 2 * N), dtype=torch.bool)[:, ::2], 4, N),
           "a numpy done": lambda: check_split_episodes(done.numpy(), 4, N),
           "length 0": lambda: check_split_episodes(done, 0, N),
           "length 2.5": lambda: check_split_episodes(done, 2.5, N),
           "length True": lambda: check_split_episodes(done, True, N),
           "float steps": lambda: check_split_episodes(done, 4, N, torch.zeros(N)),
           "short steps": lambda: check_split_episodes(done, 4, N, torch.zeros(N - 1, dtype=torch.int32)),
           "int starts": lambda: check_split_episodes(done, 4, N, None, torch.zeros(N, dtype=torch.int32)),
           "short starts": lambda: check_split_episodes(done, 4, N, None, torch.zeros(N - 1, dtype=torch.bool)),
           "negative capacity": lambda: check_split_episodes(done, 4, N, None, None, -1),
           "float capacity": lambda: check_split_episodes(done, 4, N, None, None, 3.0),
           "another device": lambda: check_split_episodes(done, 4, N, device=torch.device("cuda", 0))}
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")

    # an EpisodeSequences on its own: len() reads the count and refuses one beyond the table; picks() needs the handle
    seqs = EpisodeSequences(torch.zeros((5, 4), dtype=torch.int32), torch.tensor([5], dtype=torch.int32), 4, K, N)
    assert len(seqs) == 5 and seqs.capacity == 5 and (seqs.length, seqs.steps, seqs.num_envs) == (4, K, N)
    seqs.count[0] = 6
    with pytest.raises(ValueError, match="capacity >= 6"):
        len(seqs)
    with pytest.raises(ValueError, match="no handle"):
        seqs.picks()
    with pytest.raises(ValueError, match="gather"):
        seqs.gather(torch.zeros((K + 2, N)))


def test_the_int32_limit_of_a_pick():
    import torch
    from memory_gym_amd.vec_env import MAX_PICK, check_split_episodes

    assert MAX_PICK == 2**31 - 1
    done = torch.zeros(1, dtype=torch.bool).expand(4, 1 << 29)  # (K + 1) * N = 5 * 2^29 > INT32_MAX; a broadcast view, 1 byte of memory
    with pytest.raises(ValueError, match="int32 of a pick"):
        check_split_episodes(done, 4, 1 << 29)


def test_the_definition_on_a_hand_written_example():
    """K = 8 steps, N = 3 instances, L = 3.  Instance 0 finishes at t = 1 and t = 5, instance 1 never, instance 2 at t = 2 (a full sequence that also
    ends its episode), t = 3 and t = 7."""
    K, N, L = 8, 3, 3
    done = np.zeros((K, N), dtype=bool)
    done[[1, 5], 0] = True
    done[[2, 3, 7], 2] = True
    F, E = sd.MG_SEQ_FIRST, sd.MG_SEQ_LAST
    want = [(0, 0, 2, F | E), (0, 2, 3, F), (0, 5, 1, E), (0, 6, 2, F),
            (1, 0, 3, F), (1, 3, 3, 0), (1, 6, 2, 0),
            (2, 0, 3, F | E), (2, 3, 1, F | E), (2, 4, 3, F), (2, 7, 1, E)]
    table = sd.split(done, L)
    assert table.dtype == np.int32 and table.tolist() == [list(r) for r in want]
    assert len(want) <= sd.bound(done, L) == 3 * 3 + 5
    # steps_of clamps and cuts; start only sets the first sequence's flag
    cut = sd.split(done, L, steps_of=[11, 4, -2], start=[0, 1, 1])
    assert cut.tolist() == [[0, 0, 2, E], [0, 2, 3, F], [0, 5, 1, E], [0, 6, 2, F], [1, 0, 3, F], [1, 3, 1, 0]]
    # picks: sequence 2 (one step), a padding row, sequence 10, and one beyond the table
    pick, mask, flagged = sd.picks(table, [2, -1, 10, 11], 4, L, N)
    assert pick.tolist() == [[5 * N + 0, -1, -1], [-1, -1, -1], [7 * N + 2, -1, -1], [-1, -1, -1]] and flagged
    assert mask.tolist() == [[True, False, False], [False] * 3, [True, False, False], [False] * 3]
    pick, mask, flagged = sd.picks(table, None, 13, L, N)
    assert not flagged and pick[1].tolist() == [2 * N, 3 * N, 4 * N] and pick[11:].tolist() == [[-1] * 3] * 2 and int(mask.sum()) == K * N
    # every step of every instance is named exactly once
    assert sorted(pick[mask].tolist()) == list(range(K * N))
