"""CPU tests of the debug-view records' boundary (no GPU): include/memgym.h declares mg_save_debug_frames / mg_draw_debug_frames in plain C, the library
built here exports them and the ctypes layer declares them, the Python mirror's signatures match, and the x4 image-order stream-out's chunk-to-source-byte
mapping (csrc/mg_debug_stream_out.hpp: debug336_chunk, the function the kernel calls) expands a pseudo-random frame to numpy's x4 repeat of the
transposed frame, all 338,688 bytes, in a stand-alone program under the address and undefined-behaviour sanitizers."""
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
typedef int (*draw_fn)(mg_env*, const void*, int64_t, const int32_t*, int64_t, int, void*, void*);
int main(void) {
    save_fn s = &mg_save_debug_frames;
    draw_fn d = &mg_draw_debug_frames;
    printf("%d\n", s != 0 && d != 0);
    return 0;
}
"""


def test_header_declares_the_calls_in_plain_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not installed")
    src = tmp_path / "use_debug_frames.c"
    src.write_text(PROGRAM)
    obj = tmp_path / "use_debug_frames.o"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert obj.exists()
    header = open(os.path.join(ROOT, "include", "memgym.h")).read()
    for words in ("DEBUG-VIEW RECORDS", "int mg_save_debug_frames(", "int mg_draw_debug_frames(", "Entries must be DISTINCT", "undefined", "debug_frame_saves",
                  "debug_frame_draws", "[count][336 y][336 x][3]", "[count][84 x][84 y][3]", "#define MG_STATE_VERSION 8u"):
        assert words in header, words
    assert "the debug view (mg_render_debug);" not in header  # no longer out of scope of the frame records


def test_native_declares_the_entry_points():
    from memory_gym_amd import _native

    for name, n_args in (("mg_save_debug_frames", 5), ("mg_draw_debug_frames", 8)):
        assert hasattr(_native.LIB, name), "libmemgym_hip.so does not export " + name
        assert len(getattr(_native.LIB, name).argtypes) == n_args
    assert _native.LIB.mg_save_debug_frames.argtypes[2] is C.c_int32
    at = _native.LIB.mg_draw_debug_frames.argtypes
    assert at[2] is C.c_int64 and at[4] is C.c_int64 and at[5] is C.c_int
    # a NULL handle: refused before a GPU is touched
    assert _native.LIB.mg_save_debug_frames(None, None, 1, None, None) == -1
    assert _native.LIB.mg_draw_debug_frames(None, None, 1, None, 1, 336, None, None) == -1


def test_python_surface():
    import inspect

    import memory_gym_amd
    from memory_gym_amd.vec_env import VecMemoryGym, check_frame_draw

    assert list(inspect.signature(VecMemoryGym.save_debug_frames).parameters)[1:] == ["idx", "out"]
    p = inspect.signature(VecMemoryGym.draw_debug_frames).parameters
    assert list(p)[1:] == ["records", "pick", "out", "size"]
    assert p["pick"].default is None and p["out"].default is None and p["size"].default == 336
    assert all(v.default is None for v in list(inspect.signature(VecMemoryGym.save_debug_frames).parameters.values())[1:])
    assert issubclass(memory_gym_amd.DebugFrameRecords, memory_gym_amd.FrameRecords)
    assert VecMemoryGym.DEBUG_SIZES == {84: (84, 84, 3), 336: (336, 336, 3)}
    assert "draw_debug_frames" in VecMemoryGym.ERROR_BITS[512] and "save_debug_frames" in VecMemoryGym.ERROR_BITS[512]
    # debug-view records are not frame records: draw_frames refuses them whatever their layout
    import torch

    rec = memory_gym_amd.DebugFrameRecords(torch.zeros((3, 16), dtype=torch.uint8), 5)
    assert rec.count == 3 and rec.layout == 5
    with pytest.raises(ValueError, match="draw_debug_frames"):
        check_frame_draw(rec, 5, 16)


def test_host_sequences_that_name_an_instance_twice_are_refused():
    import torch
    from memory_gym_amd.vec_env import _distinct_host_index

    for ok in (None, [0, 7, 23], [-1, -1, 4], np.array([3, 2, 1]), torch.tensor([5, -1, -1, 6]), (1,)):
        _distinct_host_index("save_debug_frames", ok)
    for bad in ([0, 7, 7], np.array([3, 2, 3]), torch.tensor([5, 5], dtype=torch.int32), (1, -1, 1)):
        with pytest.raises(ValueError, match="more than once"):
            _distinct_host_index("save_debug_frames", bad)


def test_the_stretch_mapping_under_the_sanitizers(tmp_path):
    """tests/host/debug_stretch_check.cpp, a stand-alone program (its own main) over csrc/mg_debug_stream_out.hpp, built with
    -fsanitize=address,undefined: the kernel's mapping function expands a pseudo-random frame; the result equals numpy's x4 repeat of the transposed
    frame over all 338,688 bytes."""
    if not shutil.which("g++"):
        pytest.skip("g++ not installed")
    exe = tmp_path / "debug_stretch_check"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "host", "debug_stretch_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    frame = np.random.Generator(np.random.PCG64(336)).integers(0, 256, (84, 84, 3), dtype=np.uint8)  # [x][y][c]
    frame[83, 83] = (1, 2, 3)  # the frame's last pixel: its last dword is the buffer's last
    fin, fout = tmp_path / "frame.bin", tmp_path / "view.bin"
    frame.tofile(str(fin))
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
    got = np.fromfile(str(fout), dtype=np.uint8)
    assert got.size == 338688
    want = np.repeat(np.repeat(frame.transpose(1, 0, 2), 4, axis=0), 4, axis=1)  # [y][x][c], every pixel four times per axis
    assert want.shape == (336, 336, 3)
    assert np.array_equal(got.reshape(336, 336, 3), want)
