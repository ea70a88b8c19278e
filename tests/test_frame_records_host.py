"""CPU tests of the frame records' boundary (no GPU): include/memgym.h declares the four calls in plain C, the library built here exports them and the
ctypes layer declares them, the argument checks of save_frames / draw_frames that need no handle refuse what they must, and the host code of
csrc/mg_frame_records.hpp (layout value, row bytes, refusals, the save's walk) holds under the address and undefined-behaviour sanitizers in a
stand-alone program."""
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
typedef size_t (*bytes_fn)(const mg_env*);
typedef uint64_t (*layout_fn)(const mg_env*);
typedef int (*save_fn)(mg_env*, const int32_t*, int32_t, void*, void*);
typedef int (*draw_fn)(mg_env*, const void*, int64_t, const int32_t*, int64_t, int, void*, void*);
int main(void) {
    bytes_fn b = &mg_frame_record_bytes;
    layout_fn y = &mg_frame_layout;
    save_fn s = &mg_save_frames;
    draw_fn d = &mg_draw_frames;
    printf("%d\n", b != 0 && y != 0 && s != 0 && d != 0);
    return 0;
}
"""


def test_header_declares_the_calls_in_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    src = tmp_path / "use_frames.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_frames.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()
    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("OUT OF SCOPE", "final_obs_dev", "debug view", "vector observation", "mg_play / mg_advance", "CANNOT check", "#define MG_STATE_VERSION 8u"):
        assert words in header, words


def test_native_declares_the_entry_points():
    from memory_gym_amd import _native

    for name, n_args in (("mg_frame_record_bytes", 1), ("mg_frame_layout", 1), ("mg_save_frames", 5), ("mg_draw_frames", 8)):
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert len(getattr(_native.LIB, name).argtypes) == n_args
    assert _native.LIB.mg_frame_record_bytes.restype is C.c_size_t and _native.LIB.mg_frame_layout.restype is C.c_uint64
    assert _native.LIB.mg_save_frames.argtypes[2] is C.c_int32
    assert _native.LIB.mg_draw_frames.argtypes[2] is C.c_int64 and _native.LIB.mg_draw_frames.argtypes[4] is C.c_int64
    assert _native.LIB.mg_frame_record_bytes(None) == 0 and _native.LIB.mg_frame_layout(None) == 0  # a NULL handle: no GPU is touched
    assert _native.LIB.mg_save_frames(None, None, 1, None, None) == -1 and _native.LIB.mg_draw_frames(None, None, 1, None, 1, 0, None, None) == -1


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import VecMemoryGym

    assert list(inspect.signature(VecMemoryGym.save_frames).parameters)[1:] == ["idx", "out"]
    p = inspect.signature(VecMemoryGym.draw_frames).parameters
    assert list(p)[1:] == ["records", "pick", "out", "obs_format"] and all(p[k].default is None for k in ("pick", "out", "obs_format"))
    assert isinstance(VecMemoryGym.frame_record_bytes, property) and callable(VecMemoryGym.frame_layout)
    assert memory_gym_amd.FrameRecords.__slots__ == ("records", "layout")
    assert "draw_frames" in VecMemoryGym.ERROR_BITS[512]


def test_draw_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import FrameRecords, check_frame_draw

    width, layout = 64, (1 << 63) | (5 << 24) | 2
    store = torch.zeros((7, 48, width), dtype=torch.uint8)
    recs = FrameRecords(store, layout)
    assert recs.count == 7 * 48
    ok = lambda **kw: check_frame_draw(recs, layout, width, **kw)
    rows, pick, count, (dt, shape) = ok()
    assert tuple(rows.shape) == (336, width) and rows.data_ptr() == store.data_ptr() and pick is None and count == 336 and dt == torch.uint8 and shape == (84, 84, 3)
    rows, pick, count, (dt, shape) = ok(pick=[5, 5, 335, 0], obs_format="bf16_chw")
    assert pick.dtype == torch.int32 and pick.tolist() == [5, 5, 335, 0] and count == 4 and dt == torch.bfloat16 and shape == (3, 84, 84)
    assert ok(pick=np.arange(1000) % 336)[2] == 1000  # more rows than records: with a pick
    assert ok(pick=torch.arange(3), out=torch.zeros((3, 3, 84, 84)), obs_format="f32_chw")[2] == 3
    assert check_frame_draw(store[2], layout ^ 1, width)[2] == 48  # a plain tensor carries no layout: nothing to compare
    for what, bad in (("a stale layout", lambda: check_frame_draw(recs, layout + 1, width)),
                      ("another handle", lambda: check_frame_draw(recs, layout + (1 << 24), width)),
                      ("records of another dtype", lambda: check_frame_draw(store.to(torch.int8), layout, width)),
                      ("records of another width", lambda: check_frame_draw(recs, layout, 128)),
                      ("one dimension", lambda: check_frame_draw(torch.zeros(width, dtype=torch.uint8), layout, width)),
                      ("a strided view", lambda: check_frame_draw(store[:, ::2], layout, width)),
                      ("a column block", lambda: check_frame_draw(torch.zeros((8, 128), dtype=torch.uint8)[:, :64], layout, width)),
                      ("no tensor", lambda: check_frame_draw(store.numpy(), layout, width)),
                      ("float picks", lambda: ok(pick=torch.arange(4).float())),
                      ("bool picks", lambda: ok(pick=torch.ones(4, dtype=torch.bool))),
                      ("picks in two dimensions", lambda: ok(pick=torch.zeros((2, 2), dtype=torch.int32))),
                      ("an unknown format", lambda: ok(obs_format="rgb")),
                      ("a count beyond the records without a pick", lambda: ok(out=torch.zeros((337, 84, 84, 3), dtype=torch.uint8))),
                      ("out of another dtype", lambda: ok(out=torch.zeros((336, 84, 84, 3), dtype=torch.float32))),
                      ("out of another format's shape", lambda: ok(out=torch.zeros((336, 3, 84, 84), dtype=torch.uint8))),
                      ("out of another length than the pick", lambda: ok(pick=[1, 2], out=torch.zeros((3, 84, 84, 3), dtype=torch.uint8))),
                      ("a non-contiguous out", lambda: ok(pick=[1, 2], out=torch.zeros((4, 84, 84, 3), dtype=torch.uint8)[::2])),
                      ("a permuted out", lambda: ok(pick=[1, 2], out=torch.zeros((2, 3, 84, 84), dtype=torch.uint8).permute(0, 3, 2, 1))),
                      ("no records", lambda: check_frame_draw(torch.zeros((0, width), dtype=torch.uint8), layout, width, pick=[0]))):
        with pytest.raises(ValueError):
            bad()
            pytest.fail("accepted: " + what)


def test_save_checks_that_need_no_handle():
    import torch
    from memory_gym_amd.vec_env import FrameRecords, check_frame_save

    n, width = 48, 16
    assert check_frame_save(width, n) == (None, n, None)
    idx, k, rows = check_frame_save(width, n, idx=[3, -1, 5])
    assert k == 3 and rows is None and idx.dtype == torch.int32 and idx.tolist() == [3, -1, 5]
    store = torch.zeros((4, n, width), dtype=torch.uint8)
    rows = check_frame_save(width, n, out=store[2])[2]  # a row block of a [T, N, bytes] store
    assert rows.data_ptr() == store[2].data_ptr() and tuple(rows.shape) == (n, width)
    assert check_frame_save(width, n, idx=[3, -1, 5], out=FrameRecords(torch.zeros((3, width), dtype=torch.uint8), 1))[1] == 3
    for bad in (lambda: check_frame_save(width, n, idx=[3, 4], out=store[0]), lambda: check_frame_save(width, n, out=store[0, :40]),
                lambda: check_frame_save(64, n, out=store[0]), lambda: check_frame_save(width, n, out=store[:, 0]),
                lambda: check_frame_save(width, n, out=store[0].to(torch.int32)), lambda: check_frame_save(width, n, idx=torch.zeros(3)),
                lambda: check_frame_save(width, n, idx=torch.zeros((2, 2), dtype=torch.int64))):
        with pytest.raises(ValueError):
            bad()


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/host/frame_records_check.cpp, a stand-alone program over csrc/mg_frame_records.hpp, built with -fsanitize=address,undefined."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "frame_records_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "frame_records_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
