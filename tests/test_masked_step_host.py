"""CPU tests of the masked step's boundary (no GPU): include/memgym.h declares mg_step_masked in plain C with its ten arguments, the
Python mirror's ctypes layer declares the entry point, and VecMemoryGym.step takes mask=None behind render."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "memgym.h"
typedef int (*step_masked_fn)(mg_env*, const int32_t*, const uint8_t*, void*, float*, uint8_t*, float*, const mg_info_buffers*, int, void*);
int probe(void);
int probe(void) {
    step_masked_fn f = &mg_step_masked;
    return f != 0;
}
"""


def test_header_declares_mg_step_masked_in_plain_c(tmp_path):
    """A C99 translation unit that includes only memgym.h takes the address of mg_step_masked with the ten-argument type: it compiles with
    every warning an error (the entry point itself is not linked in: -c)."""
    cc = next((c for c in ("gcc", "cc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc is not None, "no C compiler found"
    src = tmp_path / "use_step_masked.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_step_masked.o"
    p = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()


def test_native_declares_the_entry_point():
    from memory_gym_amd import _native

    assert hasattr(_native.LIB, "mg_step_masked"), "libmemgym_hip.so does not export mg_step_masked"
    at = _native.LIB.mg_step_masked.argtypes
    assert at is not None and len(at) == 10
    assert at[7] is C.POINTER(_native.InfoBuffers) and at[8] is C.c_int
    assert all(t is C.c_void_p for k, t in enumerate(at) if k not in (7, 8))
    # mg_step's arguments with the mask behind the actions
    assert list(at[:2]) + list(at[3:]) == list(_native.LIB.mg_step.argtypes)


def test_step_takes_a_mask_behind_render():
    """(nothing is called: no GPU here)"""
    import inspect

    from memory_gym_amd.vec_env import VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    p = inspect.signature(VecMemoryGym.step).parameters
    assert list(p) == ["self", "actions", "render", "mask"]
    assert p["render"].default is True and p["mask"].default is None
    assert "mask" not in inspect.signature(GymnasiumVectorEnv.step).parameters  # gymnasium has no such call
