"""CPU: the 64-bit hand-over word of the mortar family's one-launch step (csrc/mg_mortar_handover.hpp) round-trips every field.

A stand-alone host program (its own main, g++; a second build with -fsanitize=address,undefined) includes ONLY that header and
packs / unpacks every combination of the edge values below; it also flips each field alone and asserts that no other field of the
unpacked record moves (no field leaks into another)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "endless-memory-gym_amd", "csrc")

PROGRAM = r"""
#include "mg_mortar_handover.hpp"
#include <cstdio>
using namespace mg;
static long long fails = 0, checks = 0;
static void expect(bool ok, const char* what, uint64_t w) {
    ++checks;
    if (!ok && fails++ < 10) std::printf("FAIL %s (word %016llx)\n", what, (unsigned long long)w);
}
static bool same(const Handover& a, const Handover& b) {
    return a.sx == b.sx && a.sy == b.sy && a.tmpl == b.tmpl && a.ring_on == b.ring_on && a.sprite == b.sprite && a.glyph == b.glyph && a.epoch == b.epoch;
}
int main() {
    const int32_t xs[] = {-32768, -1, 0, 1, 83, 32767};
    const uint32_t tmpls[] = {0, 1, 37, HANDOVER_TMPL_MAX, 0xFFFF};
    const uint32_t sprites[] = {0, 1, 2, 3, 4, 5, 6, 7, 0xFF};
    const uint32_t glyphs[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0xFF};
    const uint32_t epochs[] = {1, 2, 254, 255};
    for (int32_t sx : xs) for (int32_t sy : xs) for (uint32_t t : tmpls) for (uint32_t sp : sprites) for (uint32_t gl : glyphs)
    for (uint32_t ring = 0; ring < 2; ++ring) for (uint32_t ep : epochs) {
        const uint64_t w = pack_handover(sx, sy, t, ring, sp, gl, ep);
        const Handover want{sx, sy, t, ring, sp, gl, ep};
        const Handover got = unpack_handover(w);
        expect(same(got, want), "round trip", w);
        expect(same(unpack_handover((uint32_t)w, (uint32_t)(w >> 32)), want), "round trip from the two dwords", w);
        expect((uint32_t)(w >> 56) == ep && ((uint32_t)(w >> 32) >> 24) == ep, "the epoch is the top byte of the word and of its high dword", w);
        // one field changed, every other field of the unpacked record unchanged -- and the word differs in that field's bits only
        struct { Handover h; uint64_t mask; } alt[] = {
            {{sx == 83 ? -83 : 83, sy, t, ring, sp, gl, ep}, 0xFFFFull},
            {{sx, sy == 83 ? -83 : 83, t, ring, sp, gl, ep}, 0xFFFFull << 16},
            {{sx, sy, t == 36 ? 35u : 36u, ring, sp, gl, ep}, 0x7FFFull << 32},
            {{sx, sy, t, ring ^ 1u, sp, gl, ep}, 1ull << 47},
            {{sx, sy, t, ring, sp == 3 ? 0xFFu : 3u, gl, ep}, 0xFull << 48},
            {{sx, sy, t, ring, sp, gl == 9 ? 0xFFu : 9u, ep}, 0xFull << 52},
            {{sx, sy, t, ring, sp, gl, ep == 77 ? 78u : 77u}, 0xFFull << 56},
        };
        for (const auto& a : alt) {
            const uint64_t w2 = pack_handover(a.h.sx, a.h.sy, a.h.tmpl, a.h.ring_on, a.h.sprite, a.h.glyph, a.h.epoch);
            expect(same(unpack_handover(w2), a.h), "round trip of the altered record", w2);
            expect(w2 != w && ((w2 ^ w) & ~a.mask) == 0, "a field changed bits outside its own", w2);
        }
    }
    expect(pack_handover(0, 0, 0, 0, 0, 0, 0) == 0, "the zero word", 0);
    std::printf("%lld checks, %lld failures\n", checks, fails);
    return fails ? 1 : 0;
}
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_handover_word_round_trips(tmp_path, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the host program"
    src = tmp_path / "handover_pack.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "handover_pack"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags + ["-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " 0 failures" in r.stdout, r.stdout[-500:]
