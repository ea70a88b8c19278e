"""CPU tests of the rollout traces' boundary (no GPU): include/memgym.h declares mg_advance_traced / mg_play_traced / mg_rollout_trace in plain C, the
library built here exports them, the ctypes mirror of the struct has the header's size and field offsets, and the argument checks of
advance_traced(ro) / play(trace=ro) / RolloutTrace.draw that need no handle refuse what they must."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["struct_size", "frames_dev", "actions_dev", "labels_dev", "reward_dev", "done_dev"]

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "memgym.h"
typedef int (*advance_fn)(mg_env*, int32_t, double, uint64_t, uint64_t, float*, const mg_advance_out*, const mg_rollout_trace*, void*);
typedef int (*play_fn)(mg_env*, const int32_t*, int32_t, int, const uint8_t*, int32_t*, float*, const mg_advance_out*, const mg_rollout_trace*, void*);
int main(void) {
    advance_fn a = &mg_advance_traced;
    play_fn p = &mg_play_traced;
    mg_rollout_trace t;
    t.struct_size = sizeof t;
    t.frames_dev = (void*)0;
    t.actions_dev = (int32_t*)0;
    t.labels_dev = (int32_t*)0;
    t.reward_dev = (float*)0;
    t.done_dev = (uint8_t*)0;
    printf("%u %u %u %u %u %u %u %d\n", (unsigned)sizeof t, (unsigned)offsetof(mg_rollout_trace, struct_size), (unsigned)offsetof(mg_rollout_trace, frames_dev),
           (unsigned)offsetof(mg_rollout_trace, actions_dev), (unsigned)offsetof(mg_rollout_trace, labels_dev), (unsigned)offsetof(mg_rollout_trace, reward_dev),
           (unsigned)offsetof(mg_rollout_trace, done_dev), a != 0 && p != 0 && t.struct_size != 0);
    return 0;
}
"""


def test_the_ctypes_mirror_has_the_headers_layout(tmp_path):
    """A C99 program that includes nothing of HIP fills an mg_rollout_trace, takes the addresses of the two entry points (their types are checked against
    the declarations; nothing is linked in) and prints the struct's size and field offsets: those of _native.RolloutTraceRows."""
    from memory_gym_amd import _native

    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler installed")
    src = tmp_path / "use_traces.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "use_traces"
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use_traces.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    # the layout: the same program with the two addresses left out, so that it links without the library
    src2 = tmp_path / "layout.c"
    src2.write_text(PROGRAM.replace("&mg_advance_traced", "(advance_fn)1").replace("&mg_play_traced", "(play_fn)1"))
    p = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [f[0] for f in _native.RolloutTraceRows._fields_] == FIELDS
    assert out[0] == C.sizeof(_native.RolloutTraceRows)
    assert out[1:7] == [getattr(_native.RolloutTraceRows, f).offset for f in FIELDS]
    assert out[7] == 1


def test_header_and_exports_agree():
    from memory_gym_amd import _native

    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("int mg_advance_traced(", "int mg_play_traced(", "typedef struct mg_rollout_trace", "STILL OUT OF SCOPE", "vector observation", "debug view",
                  "#define MG_STATE_VERSION 8u", "traced_steps"):
        assert words in header, words
    for name, n_args in (("mg_advance_traced", 9), ("mg_play_traced", 10)):
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert len(getattr(_native.LIB, name).argtypes) == n_args
        assert getattr(_native.LIB, name).argtypes[n_args - 2] is C.POINTER(_native.RolloutTraceRows)
    at = _native.LIB.mg_advance_traced.argtypes
    assert at[1] is C.c_int32 and at[2] is C.c_double and at[3] is C.c_uint64 and at[4] is C.c_uint64 and at[6] is C.POINTER(_native.AdvanceOut)
    assert _native.LIB.mg_play_traced.argtypes[2] is C.c_int32 and _native.LIB.mg_play_traced.argtypes[7] is C.POINTER(_native.AdvanceOut)
    # a NULL handle: refused before a GPU is touched
    assert _native.LIB.mg_advance_traced(None, 1, 0.0, 0, 0, None, None, None, None) == -1
    assert _native.LIB.mg_play_traced(None, None, 1, 0, None, None, None, None, None, None) == -1


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import RolloutTrace, VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    assert memory_gym_amd.RolloutTrace is RolloutTrace
    assert RolloutTrace.__slots__ == ("frames", "frame_layout", "actions", "labels", "reward", "done")
    assert list(inspect.signature(RolloutTrace.draw).parameters)[1:] == ["env", "t", "i", "out", "obs_format"]
    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        p = inspect.signature(cls.new_rollout).parameters
        assert list(p)[1:] == ["steps", "labels"] and p["labels"].default is False
        p = inspect.signature(cls.advance_traced).parameters
        assert list(p)[1:] == ["trace", "eps", "seed", "step", "render", "stats"]
        assert [p[k].default for k in list(p)[2:]] == [0.0, 0, None, True, True]
        assert list(inspect.signature(cls.advance).parameters)[1:] == ["steps", "eps", "seed", "step", "render", "stats"]  # (as it was)
        assert inspect.signature(cls.play).parameters["trace"].default is False  # (False / True keep their meaning; a RolloutTrace is the third value)


def test_trace_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import FrameRecords, RolloutTrace, check_rollout_trace

    K, N, B = 6, 70, 64

    def make(adim=1, with_labels=True, **kw):
        acts = (K, N) if adim == 1 else (K, N, 2)
        ro = RolloutTrace(torch.zeros((K + 1, N, B), dtype=torch.uint8), 5 << 24, torch.zeros(acts, dtype=torch.int32),
                          torch.zeros(acts, dtype=torch.int32) if with_labels else None, torch.zeros((K, N)), torch.zeros((K, N), dtype=torch.bool))
        for k, v in kw.items():
            setattr(ro, k, v)
        return ro

    for adim in (1, 2):
        for teacher in (True, False):
            check_rollout_trace(make(adim), K, N, adim, B, teacher)
            check_rollout_trace(make(adim, with_labels=False), K, N, adim, B, teacher)
    check_rollout_trace(RolloutTrace(torch.zeros((K + 1, N, B), dtype=torch.uint8), 0, None, None, None, None), K, N, 1, B, True)  # frames alone
    check_rollout_trace(make(actions=torch.zeros(3), labels="x"), K, N, 1, B, False)  # play does not look at actions / labels
    assert make().steps == K and make().num_envs == N and make(frames=None).steps == K and make(frames=None).num_envs == N
    buf = torch.zeros((K + 1) * N * B + 16, dtype=torch.uint8)
    bad = {"another K": lambda: check_rollout_trace(make(), K + 1, N, 1, B, True),
           "another N": lambda: check_rollout_trace(make(), K, N + 1, 1, B, True),
           "another record width": lambda: check_rollout_trace(make(), K, N, 1, 16, True),
           "frames without row 0": lambda: check_rollout_trace(make(frames=torch.zeros((K, N, B), dtype=torch.uint8)), K, N, 1, B, True),
           "misaligned frames": lambda: check_rollout_trace(make(frames=buf[8:8 + (K + 1) * N * B].view(K + 1, N, B)), K, N, 1, B, False),
           "Discrete actions on a MultiDiscrete id": lambda: check_rollout_trace(make(1), K, N, 2, B, True),
           "int64 actions": lambda: check_rollout_trace(make(actions=torch.zeros((K, N), dtype=torch.int64)), K, N, 1, B, True),
           "float labels": lambda: check_rollout_trace(make(labels=torch.zeros((K, N))), K, N, 1, B, True),
           "float64 reward": lambda: check_rollout_trace(make(reward=torch.zeros((K, N), dtype=torch.float64)), K, N, 1, B, False),
           "uint8 done": lambda: check_rollout_trace(make(done=torch.zeros((K, N), dtype=torch.uint8)), K, N, 1, B, False),
           "a strided view": lambda: check_rollout_trace(make(reward=torch.zeros((K, 2 * N))[:, ::2]), K, N, 1, B, False),
           "a numpy array": lambda: check_rollout_trace(make(reward=torch.zeros((K, N)).numpy()), K, N, 1, B, False),
           "another device": lambda: check_rollout_trace(make(), K, N, 1, B, True, device=torch.device("cuda", 0)),
           "FrameRecords": lambda: check_rollout_trace(FrameRecords(torch.zeros((K + 1, N, B), dtype=torch.uint8), 0), K, N, 1, B, True),
           "True": lambda: check_rollout_trace(True, K, N, 1, B, False)}
    for what, call in bad.items():
        with pytest.raises(ValueError):
            call()
            pytest.fail(what + " was accepted")

    # draw(): refused before the handle is touched (env=None would raise AttributeError if it were)
    with pytest.raises(ValueError, match="one length"):
        make().draw(None, [0, 1], [0])
    with pytest.raises(ValueError, match="integers"):
        make().draw(None, [0.5], [0])
    with pytest.raises(ValueError, match="keeps no frames"):
        make(frames=None).draw(None, [0], [0])
    huge = make(frames=torch.zeros(1, dtype=torch.uint8).expand(1 << 16, 1 << 15, B))
    with pytest.raises(ValueError, match="at most"):
        huge.draw(None, [0], [0])
