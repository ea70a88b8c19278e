// mg_debug_stream_out.hpp -- the x4 IMAGE-ORDER stream-out of mg_draw_debug_frames (include/memgym.h): the reference's debug_rgb_array, straight from
// the LDS frame.  pygame.transform.scale(surface, (336, 336)) of the 84x84 debug surface repeats every pixel four times per axis, and
// fliplr(rot90(array3d, 3)) puts it in image order: out[Y][X][c] = frame[X >> 2][Y >> 2][c] (mg_render_debug reaches the same bytes with a second
// pass over HBM, debug_stretch_kernel).
//
// The frame sits in LDS as [x][y][c], column stride 252 B.  An output row is 336 x 3 = 1,008 B = 63 16-byte chunks, rows 4 y .. 4 y + 3 are equal, and
// 12 output bytes are one source pixel four times: R G B R | G B R G | B R G B.  So the row repeats every 48 B = three chunks = four source pixels, and
// chunk q = 3 m + r is made of the two neighbouring pixels x = 4 m + r and x + 1 -- 12 + 4, 8 + 8 or 4 + 12 bytes -- namely dwords r .. r + 3 of the
// six dwords the pair spells.  debug336_chunk() below is that mapping, for the device and for the host (tests/host/debug_stretch_check.cpp expands a
// whole frame with it under the sanitizers).
//
// store_debug336(): lane l < 252 of the 256 owns chunk q = l % 63 of source row y = 4 k + l / 63 in round k = 0 .. 20, so its two pixels' LDS
// addresses advance by 12 B per round (the dword alignment and r never change), consecutive lanes take consecutive chunks of a row (63 lanes write
// one row's 1,008 contiguous bytes, a wave just over a kilobyte) and the chunk, built once, is stored to the four rows.  Per frame: 5,292 chunks,
// 21,168 16-byte stores, 338,688 B.  Plain stores; the row offset is 64-bit.  The LDS reads of a wave hit columns 63 dwords apart: bank -x, no
// conflict beyond the pairs a chunk shares with its neighbour.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "mg_stream_out.hpp"
#define MG_HOST_DEVICE __host__ __device__
#else
#define MG_HOST_DEVICE
#endif

namespace mg {

constexpr int DEBUG336 = 336;                            // pixels per axis of the stretched view
constexpr int DEBUG336_ROW_BYTES = DEBUG336 * 3;          // 1,008
constexpr int DEBUG336_ROW_CHUNKS = DEBUG336_ROW_BYTES / 16;  // 63
constexpr size_t DEBUG336_BYTES = (size_t)DEBUG336 * DEBUG336_ROW_BYTES;  // 338,688 per view
constexpr int DEBUG336_SRC = 84, DEBUG336_SRC_COL_BYTES = DEBUG336_SRC * 3;  // the source frame: [84 x][84 y][3], 252 B per column
static_assert(DEBUG336_ROW_BYTES % 48 == 0 && DEBUG336_ROW_CHUNKS % 3 == 0, "a row is whole periods of three chunks");

// r | g << 8 | b << 16 of source pixel (x, y): two aligned dword reads around its three bytes (the last pixel of the frame ends with its dword: the
// second read is clamped to the frame's last dword and contributes nothing there)
MG_HOST_DEVICE inline uint32_t debug336_pixel(const uint32_t* frame_dw, int x, int y) {
    const int at = x * DEBUG336_SRC_COL_BYTES + y * 3, dw = at >> 2, last = DEBUG336_SRC * DEBUG336_SRC_COL_BYTES / 4 - 1;
    const uint64_t two = (uint64_t)frame_dw[dw] | ((uint64_t)frame_dw[dw < last ? dw + 1 : last] << 32);
    return (uint32_t)(two >> (8 * (at & 3))) & 0x00FFFFFFu;
}

// THE MAPPING: the 16 bytes of chunk q (0 .. 62) of output rows 4 y .. 4 y + 3, as four little-endian dwords
MG_HOST_DEVICE inline void debug336_chunk(const uint32_t* frame_dw, int y, int q, uint32_t out[4]) {
    const int m = q / 3, r = q - 3 * m, x = 4 * m + r;  // x + 1 <= 83: r = 2 gives x = 4 m + 2
    const uint32_t a = debug336_pixel(frame_dw, x, y), b = debug336_pixel(frame_dw, x + 1, y);
    // a pixel four times = three dwords: RGBR GBRG BRGB
    const uint32_t a0 = a | (a << 24), a1 = (a >> 8) | (a << 16), a2 = (a >> 16) | (a << 8);
    const uint32_t b0 = b | (b << 24), b1 = (b >> 8) | (b << 16), b2 = (b >> 16) | (b << 8);
    out[0] = r == 0 ? a0 : (r == 1 ? a1 : a2);
    out[1] = r == 0 ? a1 : (r == 1 ? a2 : b0);
    out[2] = r == 0 ? a2 : (r == 1 ? b0 : b1);
    out[3] = r == 0 ? b0 : (r == 1 ? b1 : b2);
}

#ifdef __HIPCC__
// Row `row` of a [count][336 y][336 x][3] buffer <- the LDS frame.  Reads the frame only; any lane may call it on its own (lanes 252 .. 255 idle).
__device__ __forceinline__ void store_debug336(const uint8_t* __restrict__ frame, void* __restrict__ rgb, int row, int tid) {
    if (tid >= 4 * DEBUG336_ROW_CHUNKS) return;
    const uint32_t* frame_dw = reinterpret_cast<const uint32_t*>(frame);
    const int y0 = tid / DEBUG336_ROW_CHUNKS, q = tid - y0 * DEBUG336_ROW_CHUNKS;
    uint8_t* dst = static_cast<uint8_t*>(rgb) + (size_t)row * DEBUG336_BYTES + (size_t)(4 * y0) * DEBUG336_ROW_BYTES + 16 * q;
#pragma unroll 3
    for (int k = 0; k < DEBUG336_SRC / 4; ++k) {
        uint32_t w[4];
        debug336_chunk(frame_dw, 4 * k + y0, q, w);
        u32x4 v;
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        u32x4* o = reinterpret_cast<u32x4*>(dst + (size_t)k * (16 * DEBUG336_ROW_BYTES));
        o[0] = v;
        o[DEBUG336_ROW_CHUNKS] = v;
        o[2 * DEBUG336_ROW_CHUNKS] = v;
        o[3 * DEBUG336_ROW_CHUNKS] = v;
    }
}
#endif

}  // namespace mg
