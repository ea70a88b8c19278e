// mg_mortar_handover.hpp -- Mortar Mayhem family: the 64-bit word in which a step lane of the one-launch step (mortar_step_raster_kernel) hands its
// instance's frame descriptor to the frame workgroup of the SAME launch.  ONE word because a naturally aligned 64-bit access is single-copy atomic:
// a reader that sees the epoch sees every other field of the same store, so the hand-over is one store and one load with no wait between words.
// No HIP and no project includes: host programs include this file as it is (tests/test_mortar_handover_pack.py).
#pragma once
#include <cstdint>

namespace mg {
// low bit to high:  sx 16 | sy 16 | tmpl 15 | ring_on 1 | sprite 4 | glyph 4 | epoch 8   (the fields of MortarDesc the frame loop uses; glyph_x0 is a
// launch constant, ring_x / ring_y are the debug view's).  The epoch is the top byte of the high dword.
constexpr int HANDOVER_SX_SHIFT = 0, HANDOVER_SY_SHIFT = 16, HANDOVER_TMPL_SHIFT = 32, HANDOVER_RING_SHIFT = 47, HANDOVER_SPRITE_SHIFT = 48,
              HANDOVER_GLYPH_SHIFT = 52, HANDOVER_EPOCH_SHIFT = 56;
constexpr uint32_t HANDOVER_TMPL_NONE = 0x7FFF;  // MortarDesc::tmpl 0xFFFF, "leave the frame untouched"
constexpr uint32_t HANDOVER_TMPL_MAX = 0x7FFE;   // largest template index the word carries
constexpr uint32_t HANDOVER_NIBBLE_NONE = 0xF;   // MortarDesc::sprite / glyph 0xFF, "none" (sprites are 0..7, glyphs 0..9)
static_assert(HANDOVER_SX_SHIFT == 0 && HANDOVER_SY_SHIFT - HANDOVER_SX_SHIFT == 16 && HANDOVER_TMPL_SHIFT - HANDOVER_SY_SHIFT == 16, "sx, sy: 16 bits each");
static_assert(HANDOVER_RING_SHIFT - HANDOVER_TMPL_SHIFT == 15 && HANDOVER_SPRITE_SHIFT - HANDOVER_RING_SHIFT == 1, "tmpl 15 bits, ring_on 1");
static_assert(HANDOVER_GLYPH_SHIFT - HANDOVER_SPRITE_SHIFT == 4 && HANDOVER_EPOCH_SHIFT - HANDOVER_GLYPH_SHIFT == 4, "sprite, glyph: 4 bits each");
static_assert(HANDOVER_EPOCH_SHIFT + 8 == 64 && HANDOVER_EPOCH_SHIFT - 32 == 24, "the epoch is the top byte of the word (and of its high dword)");

struct Handover {  // the fields with MortarDesc's values (tmpl 0xFFFF, sprite / glyph 0xFF where the word holds its "none" codes)
    int32_t sx, sy;
    uint32_t tmpl, ring_on, sprite, glyph, epoch;
};

// (built as two dwords: that is how both ends hold the word in registers)
constexpr uint32_t handover_lo(int32_t sx, int32_t sy) { return ((uint32_t)sx & 0xFFFFu) | ((uint32_t)sy & 0xFFFFu) << (HANDOVER_SY_SHIFT - HANDOVER_SX_SHIFT); }
constexpr uint32_t handover_hi(uint32_t tmpl, uint32_t ring_on, uint32_t sprite, uint32_t glyph, uint32_t epoch) {
    return (tmpl == 0xFFFFu ? HANDOVER_TMPL_NONE : tmpl & 0x7FFFu) << (HANDOVER_TMPL_SHIFT - 32) | (ring_on ? 1u : 0u) << (HANDOVER_RING_SHIFT - 32) |
           (sprite == 0xFFu ? HANDOVER_NIBBLE_NONE : sprite & 0xFu) << (HANDOVER_SPRITE_SHIFT - 32) |
           (glyph == 0xFFu ? HANDOVER_NIBBLE_NONE : glyph & 0xFu) << (HANDOVER_GLYPH_SHIFT - 32) | (epoch & 0xFFu) << (HANDOVER_EPOCH_SHIFT - 32);
}
constexpr uint64_t pack_handover(int32_t sx, int32_t sy, uint32_t tmpl, uint32_t ring_on, uint32_t sprite, uint32_t glyph, uint32_t epoch) {
    return (uint64_t)handover_hi(tmpl, ring_on, sprite, glyph, epoch) << 32 | handover_lo(sx, sy);
}
// (from the two dwords, which is how the frame loop holds the word: scalar registers)
constexpr Handover unpack_handover(uint32_t lo, uint32_t hi) {
    const uint32_t tmpl = hi & 0x7FFFu, sprite = (hi >> (HANDOVER_SPRITE_SHIFT - 32)) & 0xFu, glyph = (hi >> (HANDOVER_GLYPH_SHIFT - 32)) & 0xFu;
    return Handover{(int32_t)(int16_t)(uint16_t)(lo & 0xFFFFu), (int32_t)(int16_t)(uint16_t)(lo >> 16), tmpl == HANDOVER_TMPL_NONE ? 0xFFFFu : tmpl,
                    (hi >> (HANDOVER_RING_SHIFT - 32)) & 1u, sprite == HANDOVER_NIBBLE_NONE ? 0xFFu : sprite, glyph == HANDOVER_NIBBLE_NONE ? 0xFFu : glyph,
                    hi >> (HANDOVER_EPOCH_SHIFT - 32)};
}
constexpr Handover unpack_handover(uint64_t w) { return unpack_handover((uint32_t)w, (uint32_t)(w >> 32)); }

static_assert(unpack_handover(pack_handover(-1, -32768, 36, 1, 7, 9, 255)).sx == -1 && unpack_handover(pack_handover(-1, -32768, 36, 1, 7, 9, 255)).sy == -32768,
              "sx, sy are sign-extended");
static_assert(unpack_handover(pack_handover(0, 0, 0xFFFF, 0, 0xFF, 0xFF, 1)).tmpl == 0xFFFF && unpack_handover(pack_handover(0, 0, 0xFFFF, 0, 0xFF, 0xFF, 1)).sprite == 0xFF &&
                  unpack_handover(pack_handover(0, 0, 0xFFFF, 0, 0xFF, 0xFF, 1)).glyph == 0xFF,
              "the none codes come back as MortarDesc's");
static_assert(pack_handover(0, 0, 0, 0, 0, 0, 0) == 0, "a zeroed word is epoch 0: never a one-launch epoch");
}  // namespace mg
