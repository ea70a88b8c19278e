"""CPU tests of the terminal frame records' boundary (no GPU): include/memgym.h declares mg_info_buffers.final_frames_dev in plain C, the ctypes mirror
of the struct has the header's size and field offsets, the library's reading of the struct (csrc/mg_info.hpp) still accepts a caller built against the
older, shorter header -- in a stand-alone program under the address and undefined-behaviour sanitizers -- and the Python surface has the new keyword,
last in its lists, with the signatures other tests pin left alone."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["struct_size", "ep_reward_dev", "ep_length_dev", "aux_dev", "final_obs_dev", "reward64_dev", "gt64_dev", "capacity_dev", "final_frames_dev"]

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "memgym.h"
int main(void) {
    mg_info_buffers b;
    b.struct_size = sizeof b;
    b.capacity_dev = (uint8_t*)0;
    b.final_frames_dev = (void*)0;
    printf("%u %u %u %u %u %u %u %u %u %u %d\n", (unsigned)sizeof b, (unsigned)offsetof(mg_info_buffers, struct_size), (unsigned)offsetof(mg_info_buffers, ep_reward_dev),
           (unsigned)offsetof(mg_info_buffers, ep_length_dev), (unsigned)offsetof(mg_info_buffers, aux_dev), (unsigned)offsetof(mg_info_buffers, final_obs_dev),
           (unsigned)offsetof(mg_info_buffers, reward64_dev), (unsigned)offsetof(mg_info_buffers, gt64_dev), (unsigned)offsetof(mg_info_buffers, capacity_dev),
           (unsigned)offsetof(mg_info_buffers, final_frames_dev), b.struct_size != 0 && MG_STATE_VERSION == 8u);
    return 0;
}
"""


def test_the_header_is_c99_and_the_ctypes_mirror_has_its_layout(tmp_path):
    """A C99 program that includes nothing of HIP fills the new member and prints the struct's size and offsets: those of _native.InfoBuffers.  The
    member is the LAST one, behind capacity_dev: a caller's older struct is a prefix of today's."""
    from memory_gym_amd import _native

    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler installed")
    src = tmp_path / "use_final_frames.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "use_final_frames"
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [f[0] for f in _native.InfoBuffers._fields_] == FIELDS
    assert out[0] == C.sizeof(_native.InfoBuffers)
    assert out[1:10] == [getattr(_native.InfoBuffers, f).offset for f in FIELDS]
    assert out[9] == out[8] + C.sizeof(C.c_void_p) and out[0] == out[9] + C.sizeof(C.c_void_p)
    assert out[10] == 1


def test_the_header_says_what_it_must():
    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("void* final_frames_dev;", "final_frame_steps", "BEFORE ANY RESET OF THIS CALL", "SAME NUMBER OF", "PLAIN arrangement, not the",
                  "final_frames_dev together with final_obs_dev", "obs_dev == NULL together with info->final_obs_dev", "OUT OF SCOPE", "debug view",
                  "vector observation", "STILL OUT OF SCOPE: the terminal frames of episodes that end inside a call", "#define MG_STATE_VERSION 8u"):
        assert words in header, words
    assert header.index("uint8_t* capacity_dev;") < header.index("void* final_frames_dev;") < header.index("} mg_info_buffers;")


def test_an_older_callers_struct_is_still_read(tmp_path):
    """tests/host/info_buffers_check.cpp, a stand-alone program over csrc/mg_info.hpp, built with -fsanitize=address,undefined: a struct of the OLD size
    (offsetof(mg_info_buffers, final_frames_dev)) whose memory ends there is accepted and reads the member as NULL; so are the shortest and a later layout;
    sizes that are no layout and the three refusals of the terminal-frame members are refused."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "info_buffers_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "info_buffers_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_python_surface():
    import memory_gym_amd
    from memory_gym_amd.vec_env import VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    for f in (memory_gym_amd.make, VecMemoryGym.__init__, GymnasiumVectorEnv.__init__):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "final_frames" and p["final_frames"].default is False, f
    assert inspect.signature(memory_gym_amd.make).parameters["final_observation"].default is False
    # the signatures other tests pin stay as they are
    assert list(inspect.signature(VecMemoryGym.step).parameters)[1:] == ["actions", "render", "mask"]
    assert list(inspect.signature(GymnasiumVectorEnv.step).parameters)[1:] == ["actions"]
    assert list(inspect.signature(VecMemoryGym.advance).parameters)[1:] == ["steps", "eps", "seed", "step", "render", "stats"]
    assert list(inspect.signature(GymnasiumVectorEnv.final_observations).parameters)[1:] == ["info", "out", "obs_format"]
    p = inspect.signature(GymnasiumVectorEnv.final_observations).parameters
    assert p["out"].default is None and p["obs_format"].default is None
    # the two conventions exclude each other, and that is said before a GPU is touched
    with pytest.raises(ValueError, match="pick one"):
        memory_gym_amd.make("MortarMayhem-Grid-v0", num_envs=4, final_observation=True, final_frames=True)
    with pytest.raises(ValueError, match="pick one"):
        VecMemoryGym("MortarMayhem-Grid-v0", num_envs=4, final_observation=True, final_frames=True)
    # the info keys of the convention without frames
    src = inspect.getsource(GymnasiumVectorEnv.step)
    assert '"final_frames"' in inspect.getsource(VecMemoryGym.step) and "final_frames=" in src and "_final_frames=" in src


def test_a_null_handle_is_refused_with_the_new_struct():
    from memory_gym_amd import _native

    ib = _native.InfoBuffers()
    ib.struct_size = C.sizeof(_native.InfoBuffers)
    ib.final_frames_dev = 16
    assert _native.LIB.mg_step(None, None, None, None, None, None, C.byref(ib), 1, None) == -1
    assert _native.LIB.mg_debug_counter(None, b"final_frame_steps", C.byref(C.c_int64())) == -1
