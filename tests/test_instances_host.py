"""CPU tests of the instance records' boundary (no GPU): include/memgym.h declares mg_save_instances / mg_load_instances in plain C, the
ctypes layer declares them, the argument checks of save_instances / load_instances that need no handle refuse what they must, and the host
half of csrc/mg_instances.hpp (row table, splits, the served / skipped / flagged rule) holds under the address and undefined-behaviour
sanitizers in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include "memgym.h"
typedef int (*save_fn)(mg_env*, const int32_t*, int32_t, void*, void*);
typedef int (*load_fn)(mg_env*, const int32_t*, const int32_t*, int32_t, const void*, void*, void*);
typedef size_t (*bytes_fn)(const mg_env*);
typedef uint64_t (*layout_fn)(const mg_env*);
int main(void) {
    save_fn s = &mg_save_instances;
    load_fn l = &mg_load_instances;
    bytes_fn b = &mg_instance_bytes;
    layout_fn y = &mg_instance_layout;
    printf("%d\n", s != 0 && l != 0 && b != 0 && y != 0);
    return 0;
}
"""


def test_header_declares_the_calls_in_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    src = tmp_path / "use_instances.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_instances.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()


def test_native_declares_the_entry_points():
    from memory_gym_amd import _native

    for name, n_args in (("mg_instance_bytes", 1), ("mg_instance_layout", 1), ("mg_save_instances", 5), ("mg_load_instances", 7)):
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert len(getattr(_native.LIB, name).argtypes) == n_args
    assert _native.LIB.mg_instance_bytes.restype is C.c_size_t and _native.LIB.mg_instance_layout.restype is C.c_uint64
    assert _native.LIB.mg_save_instances.argtypes[2] is C.c_int32 and _native.LIB.mg_load_instances.argtypes[3] is C.c_int32
    assert _native.LIB.mg_instance_bytes(None) == 0 and _native.LIB.mg_instance_layout(None) == 0  # a NULL handle: no GPU is touched


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import MemoryGymEnv, VecMemoryGym
    from memory_gym_amd.vector import GymnasiumVectorEnv

    for cls in (VecMemoryGym, GymnasiumVectorEnv):
        assert list(inspect.signature(cls.save_instances).parameters)[1:] == ["idx", "out"]
        p = inspect.signature(cls.load_instances).parameters
        assert list(p)[1:] == ["snap", "idx", "rec", "render"] and p["render"].default is True and p["idx"].default is None and p["rec"].default is None
        p = inspect.signature(cls.copy_instances).parameters
        assert list(p)[1:] == ["src", "dst", "render"] and p["render"].default is True
    assert callable(MemoryGymEnv.snapshot) and callable(MemoryGymEnv.restore)
    assert 512 in VecMemoryGym.ERROR_BITS and not (512 & VecMemoryGym.CAPACITY_BITS)
    assert memory_gym_amd.InstanceSnapshot.__slots__ == ("records", "layout", "set_of")


def test_load_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import InstanceSnapshot, check_instance_load

    n, width, layout = 200, 448, (5 << 24) | 2
    snap = InstanceSnapshot(torch.zeros((65, width), dtype=torch.uint8), layout)
    ok = lambda **kw: check_instance_load(snap, layout, width, n, **kw)
    idx, rec = ok(idx=torch.arange(65), rec=torch.arange(65, dtype=torch.int32))
    assert idx.dtype == torch.int32 and rec.dtype == torch.int32 and idx.is_contiguous() and idx.tolist() == list(range(65))
    idx, rec = ok(idx=list(range(0, 130, 2)))
    assert idx.dtype == torch.int32 and rec is None and idx[-1] == 128
    idx, rec = ok(idx=np.arange(100), rec=np.zeros(100, np.int64))  # one record into many: more entries than records, with rec
    assert idx.numel() == 100 and rec.numel() == 100
    assert ok(idx=torch.full((65,), -1)) [0].tolist() == [-1] * 65
    for what, bad in (("another handle", lambda: check_instance_load(snap, (6 << 24) | 2, width, n, idx=torch.arange(65))),
                      ("a stale layout", lambda: check_instance_load(snap, (5 << 24) | 3, width, n, idx=torch.arange(65))),
                      ("a wrong record width", lambda: check_instance_load(snap, layout, width + 16, n, idx=torch.arange(65))),
                      ("no snapshot", lambda: check_instance_load(snap.records, layout, width, n)),
                      ("float indices", lambda: ok(idx=torch.arange(65).float())),
                      ("bool indices", lambda: ok(idx=torch.ones(65, dtype=torch.bool))),
                      ("a list of floats", lambda: ok(idx=[0.5, 1.0])),
                      ("two dimensions", lambda: ok(idx=torch.zeros((5, 13), dtype=torch.int32))),
                      ("rec of another length", lambda: ok(idx=torch.arange(65), rec=torch.arange(64))),
                      ("more instances than records without rec", lambda: ok(idx=torch.arange(66))),
                      ("all instances from 65 records", lambda: ok()),
                      ("records of another dtype", lambda: check_instance_load(InstanceSnapshot(torch.zeros((65, width), dtype=torch.int8), layout), layout, width, n,
                                                                              idx=torch.arange(65))),
                      ("set_of of another length", lambda: check_instance_load(InstanceSnapshot(snap.records, layout, torch.zeros(64, dtype=torch.int32)), layout, width,
                                                                              n, idx=torch.arange(65)))):
        with pytest.raises(ValueError):
            bad()
            pytest.fail("accepted: " + what)


def test_save_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import InstanceSnapshot, check_instance_save

    n, width = 200, 448
    assert check_instance_save(width, n) == (None, n)
    idx, k = check_instance_save(width, n, idx=[3, -1, 5])
    assert k == 3 and idx.dtype == torch.int32 and idx.tolist() == [3, -1, 5]
    out = InstanceSnapshot(torch.zeros((3, width), dtype=torch.uint8), 1)
    assert check_instance_save(width, n, idx=[3, -1, 5], out=out)[1] == 3
    for bad in (lambda: check_instance_save(width, n, idx=[3, 4], out=out), lambda: check_instance_save(width, n, out=out),
                lambda: check_instance_save(width + 16, n, idx=[3, -1, 5], out=out), lambda: check_instance_save(width, n, idx=[3, -1, 5], out=out.records),
                lambda: check_instance_save(width, n, idx=torch.zeros(3))):
        with pytest.raises(ValueError):
            bad()


def test_row_table_under_the_sanitizers(tmp_path):
    """tests/host/instances_table_check.cpp, a stand-alone program over the host half of csrc/mg_instances.hpp, built with
    -fsanitize=address,undefined: every byte the kernels' walk would touch lies inside its row and its record."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "instances_table_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "instances_table_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
