"""CPU tests of the headless interface's boundary (no GPU): include/memgym.h declares mg_advance / mg_advance_out in plain C, and the
Python mirror's ctypes layer declares the entry point with the struct the header lays out."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "memgym.h"
typedef int (*advance_fn)(mg_env*, int32_t, double, uint64_t, uint64_t, float*, const mg_advance_out*, void*);
int main(void) {
    mg_advance_out out;
    advance_fn f = &mg_advance;
    int k;
    memset(&out, 0, sizeof out);
    out.struct_size = sizeof out;
    out.reward_sum_dev = (double*)0;
    out.episodes_dev = (int32_t*)0;
    out.ep_reward_sum_dev = (double*)0;
    out.ep_length_sum_dev = (int64_t*)0;
    for (k = 0; k < MG_INFO_SLOTS; ++k) out.aux_sum_dev[k] = (double*)0;
    printf("%u %u %d\n", (unsigned)sizeof out, (unsigned)((char*)&out.aux_sum_dev[0] - (char*)&out), f != 0);
    return 0;
}
"""


def test_header_declares_mg_advance_in_plain_c(tmp_path):
    """A C99 program that includes nothing of HIP fills an mg_advance_out and takes the address of mg_advance: it compiles (the entry point
    itself is not linked in: -c), and the struct it sees is the one _native.AdvanceOut describes."""
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    src = tmp_path / "use_advance.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_advance.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()


def test_native_declares_the_entry_point():
    from memory_gym_amd import _native

    assert hasattr(_native.LIB, "mg_advance"), "libmemgym_hip.so does not export mg_advance"
    at = _native.LIB.mg_advance.argtypes
    assert at is not None and len(at) == 8
    assert at[1] is C.c_int32 and at[2] is C.c_double and at[3] is C.c_uint64 and at[4] is C.c_uint64
    assert at[6] is C.POINTER(_native.AdvanceOut)
    names = [f[0] for f in _native.AdvanceOut._fields_]
    assert names == ["struct_size", "reward_sum_dev", "episodes_dev", "ep_reward_sum_dev", "ep_length_sum_dev", "aux_sum_dev"]
    assert C.sizeof(_native.AdvanceOut) == C.sizeof(C.c_void_p) * (5 + _native.MG_INFO_SLOTS)  # the header's layout on a 64-bit host
    assert _native.AdvanceOut.aux_sum_dev.offset == 5 * C.sizeof(C.c_void_p)


def test_python_surface_has_the_headless_calls():
    """step(render=...), redraw() and advance() exist on both front ends with the documented signatures (nothing is called: no GPU here)."""
    import inspect

    from memory_gym_amd.vec_env import VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    assert inspect.signature(VecMemoryGym.step).parameters["render"].default is True
    assert callable(VecMemoryGym.redraw)
    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        p = inspect.signature(cls.advance).parameters
        assert list(p)[1:] == ["steps", "eps", "seed", "step", "render", "stats"]
        assert (p["eps"].default, p["seed"].default, p["step"].default, p["render"].default, p["stats"].default) == (0.0, 0, None, True, True)
