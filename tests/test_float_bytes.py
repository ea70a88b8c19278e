"""CPU: a float observation names its byte.  The float stream-out formats hold byte / 255 as float32, or that quotient rounded to float16 /
bfloat16 (include/memgym.h MG_OBS_F32_CYX / F16_CYX / BF16_CYX); round(x * 255) recovers the byte from every one of the 3 x 256 values, so
a test may turn float rows back into the uint8 [x][y][c] frame the oracle digests (tests/chw_referee.py: unit_values, float_rows_to_bytes).

Why it holds: neighbouring bytes are 1 / 255 = 3.9e-3 apart; bfloat16 keeps 8 significant bits, so below 1 its rounding error is at most
2^-9 = 1.95e-3 relative to a value < 1, i.e. less than half that spacing, and x * 255 lies within 0.5 of the byte."""
import numpy as np
import pytest

from chw_referee import float_rows_to_bytes, unit_values

FORMATS = ("f32_chw", "f16_chw", "bf16_chw")


@pytest.mark.parametrize("fmt", FORMATS)
def test_round_recovers_every_byte(fmt):
    import torch

    v = unit_values(fmt)
    back = torch.round(v.to(torch.float32) * 255.0)
    assert back.dtype == torch.float32 and torch.equal(back, torch.arange(256, dtype=torch.float32))
    assert len(torch.unique(v)) == 256  # (and no two bytes share a value)


@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_come_back_in_frame_order(fmt):
    import torch

    g = np.random.Generator(np.random.PCG64(1))
    frames = g.integers(0, 256, (3, 84, 84, 3)).astype(np.uint8)  # [k][x][y][c]
    frames[0].reshape(-1)[:256] = np.arange(256)  # every byte occurs
    rows = unit_values(fmt)[torch.from_numpy(frames.transpose(0, 3, 2, 1).astype(np.int64))]  # [k][c][y][x]
    assert rows.shape == (3, 3, 84, 84)
    assert np.array_equal(float_rows_to_bytes(rows).numpy(), frames)
