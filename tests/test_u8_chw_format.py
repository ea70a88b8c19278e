"""CPU: the uint8 image-order observation format as the header, the Python mirror and the observation-buffer allocator see it
(include/memgym.h MG_OBS_U8_CYX; VecMemoryGym.OBS_FORMATS["u8_chw"]).  It is one byte per element: a buffer of it is dealt to the
memory zones exactly like a buffer of the reference-order uint8 frames."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "endless-memory-gym_amd"))
from memory_gym_amd import _native  # noqa: E402


def test_header_codes():
    text = open(os.path.join(ROOT, "include", "memgym.h")).read()
    codes = {name: int(value) for name, value in re.findall(r"^#define (MG_OBS_\w+_(?:XYC|CYX)) (\d+)\s*$", text, re.M)}
    assert codes == {"MG_OBS_U8_XYC": 0, "MG_OBS_F32_CYX": 1, "MG_OBS_F16_CYX": 2, "MG_OBS_BF16_CYX": 3, "MG_OBS_U8_CYX": 4}


def test_python_name():
    import torch
    from memory_gym_amd.vec_env import VecMemoryGym

    assert VecMemoryGym.OBS_FORMATS["u8_chw"] == (4, torch.uint8, (3, 84, 84))
    assert VecMemoryGym.OBS_FORMATS["u8_xyc"] == (0, torch.uint8, (84, 84, 3))  # the old names keep their codes
    assert [VecMemoryGym.OBS_FORMATS[f][0] for f in ("f32_chw", "f16_chw", "bf16_chw")] == [1, 2, 3]


def test_observation_buffer_plan_is_the_uint8_one():
    """mg_obs_plan (the order mg_obs_alloc_for deals pieces to the zones, no GPU needed) for 65,536 frames of this format: the frame is
    21,168 bytes, and the plan is the one recorded for the reference-order uint8 frames before this format existed."""
    import numpy as np
    import torch
    from memory_gym_amd.vec_env import VecMemoryGym

    def frame_bytes(name):
        _, dt, shape = VecMemoryGym.OBS_FORMATS[name]
        return int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()

    def plan(frame, zones):
        z = (C.c_int * 256)()
        piece, lead = C.c_size_t(), C.c_size_t()
        k = _native.LIB.mg_obs_plan(65536 * frame, frame, zones, C.byref(piece), C.byref(lead), z, 256)
        return k, piece.value, lead.value, list(z[:k])

    assert frame_bytes("u8_chw") == 21168
    recorded = {2: [0, 1, 0, 1, 0], 3: [0, 1, 2, 0, 1]}
    for zones, want in recorded.items():
        got = plan(frame_bytes("u8_chw"), zones)
        assert got == plan(frame_bytes("u8_xyc"), zones)  # whatever the allocator does for the reference-order frame today ...
        assert got == (5, 318767104, 102760448, want)     # ... which is what it did before this format existed
