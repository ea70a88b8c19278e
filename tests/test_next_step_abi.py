"""CPU: mg_step_next is declared in include/memgym.h and exported by the library (tests/test_abi_symbols.py then covers it with every other symbol),
a plain C translation unit that calls it compiles against the header alone, and the Python mirror refuses what it must before any handle exists."""
import ctypes
import os
import shutil
import subprocess

import pytest

import test_abi_symbols as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mg_step_next_is_declared_and_exported():
    assert "mg_step_next" in abi.declared_symbols()
    if not os.path.exists(abi.LIB):
        import __graft_entry__
        __graft_entry__.build_hip()
    import torch  # noqa: F401  (same load order as the package: torch's HIP runtime first)
    assert hasattr(ctypes.CDLL(abi.LIB), "mg_step_next")
    h = open(os.path.join(ROOT, "include", "memgym.h")).read()
    assert "#define MG_STATE_VERSION 8u" in h  # no state is added


def test_a_c_caller_of_mg_step_next_compiles_against_the_header_alone(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    src = tmp_path / "use_next.c"
    src.write_text('#include "memgym.h"\n'
                   "int next(mg_env* e, const int32_t* a, uint8_t* done, void* obs, float* r, float* gt, const mg_info_buffers* info, void* s) {\n"
                   "    return mg_step_next(e, a, done, obs, r, done, gt, info, s); /* restart_dev == done_dev */\n}\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "o.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_make_refuses_terminal_rows_in_next_step_mode_before_it_needs_a_gpu():
    import memory_gym_amd

    for kw in (dict(final_observation=True), dict(final_frames=True)):
        with pytest.raises(ValueError, match="next_step"):
            memory_gym_amd.VecMemoryGym("MortarMayhem-Grid-v0", num_envs=4, autoreset_mode="next_step", **kw)
    with pytest.raises(ValueError, match="autoreset_mode"):
        memory_gym_amd.VecMemoryGym("MortarMayhem-Grid-v0", num_envs=4, autoreset_mode="later")
    with pytest.raises(ValueError, match="autoreset_mode"):
        memory_gym_amd.make("MortarMayhem-Grid-v0", autoreset_mode="next_step")  # the single-instance adapter has no such mode
