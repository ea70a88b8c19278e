"""CPU tests of mg_play's boundary (no GPU): include/memgym.h declares it in plain C, the library exports it, the Python mirror's ctypes
layer binds its eleven arguments, both front ends have play(), and the example scripts that use the surrounding workflow start without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "memgym.h"
int main(void) {
    mg_advance_out sums;
    int rc;
    memset(&sums, 0, sizeof sums);
    sums.struct_size = sizeof sums;
    rc = mg_play((mg_env*)0, (const int32_t*)0, 1, MG_PLAY_EPISODE, (const uint8_t*)0, (float*)0, (uint8_t*)0, (int32_t*)0, (float*)0, &sums, (void*)0);
    printf("%d %d %d\n", rc, MG_PLAY_THROUGH, MG_PLAY_EPISODE);
    return 0;
}
"""


def test_header_declares_mg_play_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "memgym.h")).read()
    m = re.search(r"\bint\s+mg_play\s*\(([^;]*)\)\s*;", text)
    assert m, "include/memgym.h does not declare mg_play"
    assert len(m.group(1).split(",")) == 11
    assert re.search(r"#define\s+MG_PLAY_THROUGH\s+0\b", text) and re.search(r"#define\s+MG_PLAY_EPISODE\s+1\b", text)
    assert re.search(r"#define\s+MG_STATE_VERSION\s+8u", text), "mg_play adds no state: the checkpoint version stays"
    from memory_gym_amd import _native

    assert hasattr(_native.LIB, "mg_play"), "libmemgym_hip.so does not export mg_play"


def test_a_plain_c_caller_of_mg_play_compiles(tmp_path):
    """A C99 translation unit that includes nothing of HIP calls mg_play with a zeroed mg_advance_out: it compiles under -Wall -Wextra -Werror
    -pedantic (the entry point itself is not linked in: -c)."""
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler on this machine"
    src = tmp_path / "use_play.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_play.o"
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()


def test_native_binds_eleven_arguments():
    from memory_gym_amd import _native

    at = _native.LIB.mg_play.argtypes
    assert at is not None and len(at) == 11
    assert at[2] is C.c_int32 and at[3] is C.c_int and at[9] is C.POINTER(_native.AdvanceOut)
    assert (_native.MG_PLAY_THROUGH, _native.MG_PLAY_EPISODE) == (0, 1)


def test_python_surface_has_play():
    """play() exists on both front ends with the documented signature (nothing is called: no GPU here)."""
    import inspect

    from memory_gym_amd.vec_env import VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        p = inspect.signature(cls.play).parameters
        assert list(p)[1:] == ["actions", "until_done", "mask", "render", "stats", "trace"]
        assert [p[k].default for k in list(p)[2:]] == [False, None, True, True, False]


def test_the_example_scripts_parse_help_without_a_gpu():
    for name in ("plan_random_shooting.py", "branch_from_state.py"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), "--help"], capture_output=True, text=True)
        assert p.returncode == 0, name + ": " + p.stderr
        assert "--env" in p.stdout and "usage" in p.stdout.lower(), name
