#!/usr/bin/env python3
"""tools/lds_bank_count.py -- the LDS bank picture of the MG_OBS_U8_CYX transpose (csrc/mg_stream_out.hpp, frame_to_cyx), counted over the
frame's real addresses; no GPU, no compiler.  The table of profiles/u8_chw.md is this script's output.

Rule: ds_read_b32 / ds_write_b32 / ds_read_u8 see 32 banks of one dword; conflicts arise within a 32-lane half of a wave; lanes on the same
dword are served together (a broadcast read, one merged write); an access costs one extra cycle per further distinct dword on its
busiest bank.  An access = one instruction of one half-wave with at least one active lane.  DERIVED figures: nothing here is measured.

The frame is [x][y][c] before (column stride 252 B = 63 dwords) and [c][y][x] after (row stride 84 B = 21 dwords).  A block is four columns
(x = 4 xg ..) by twelve in-column bytes (y = 4 k .., three channels): twelve dword reads, twelve dword writes; 21 x 21 blocks."""
from collections import defaultdict

SCREEN, COL_DW, ROW_DW, KB = 84, 63, 21, 21


def cost(instr):
    """instr: one instruction as a list of (lane, dword) over the whole workgroup -> (half-wave accesses, extra cycles, halves beyond 2-way)"""
    halves = defaultdict(lambda: defaultdict(set))
    for lane, dw in instr:
        halves[lane // 32][dw % 32].add(dw)
    ways = [max(len(s) for s in banks.values()) for banks in halves.values()]
    return len(ways), sum(w - 1 for w in ways), sum(w > 2 for w in ways)


def total(instrs):
    return tuple(map(sum, zip(*(cost(i) for i in instrs))))


def blocks(slot_to_block, slots):
    """reads and writes of the 4-column x 12-byte scheme; slot_to_block(u) -> (k, xg) or None for an idle lane"""
    reads, writes = [], []
    for r in range((slots + 255) // 256):
        lanes = [(t, slot_to_block(t + 256 * r)) for t in range(256)]
        lanes = [(t, b) for t, b in lanes if b is not None]
        for m in range(3):
            for i in range(4):
                reads.append([(t, (4 * xg + i) * COL_DW + 3 * k + m) for t, (k, xg) in lanes])
        for o in range(12):  # in-column byte o = 3 j + c of the block -> row 84 c + 4 k + j
            writes.append([(t, 4 * k * ROW_DW + xg + ((o % 3) * SCREEN + o // 3) * ROW_DW) for t, (k, xg) in lanes])
    return total(reads), total(writes)


def tiled(tk, txg):
    """half-waves of tk k-blocks x txg column groups (tk * txg = 32); tiles run over k first; a k past the last takes an earlier block of
    its own half-wave, the lanes past the last slot their first block again, as frame_to_cyx does (no lane idle)"""
    tiles_k = (KB + tk - 1) // tk
    per_tile = tk * ROW_DW
    slots = tiles_k * per_tile

    def block(u1):
        u = u1 if u1 < slots else u1 - 256
        kt, rem = divmod(u, per_tile)
        valid = min(tk, KB - kt * tk)  # k-blocks of this tile that exist
        return kt * tk + rem % tk % valid, rem // tk
    return blocks(block, ((slots + 255) // 256) * 256)


def byte_gather():
    """the float formats' gather asked for this format: lane q builds the 16-byte chunk q of the output from sixteen byte reads"""
    instrs = []
    for base in range(0, 1323, 256):
        for j in range(16):
            one = []
            for t in range(min(256, 1323 - base)):
                b = 16 * (base + t) + j
                c, y, x = b // (SCREEN * SCREEN), b // SCREEN % SCREEN, b % SCREEN
                one.append((t, (x * 4 * COL_DW + 3 * y + c) // 4))
            instrs.append(one)
    return total(instrs)


if __name__ == "__main__":
    def built(u1):  # frame_to_cyx, line by line
        slots = ((KB + 7) // 8) * 8 * ROW_DW
        u = u1 if u1 < slots else u1 - 256
        kt, rem = divmod(u, 8 * ROW_DW)
        k1 = kt * 8 + (rem & 7)
        return (k1 if k1 < KB else k1 - 5), rem >> 3
    covered = {built(u) for u in range(512)}
    assert covered == {(k, xg) for k in range(KB) for xg in range(ROW_DW)}, "frame_to_cyx's slots do not cover the 441 blocks"
    assert tiled(8, 4) == blocks(built, 512)
    print("%-44s %-28s %s" % ("gather", "reads: accesses extra >2-way", "writes: accesses extra >2-way"))
    print("%-44s %-28s" % ("byte reads, one 16-byte chunk per lane", "%d %d %d" % byte_gather()))
    rows = [("blocks, lanes along k", lambda u: (u % KB, u // KB) if u < KB * ROW_DW else None, KB * ROW_DW),
            ("blocks, lanes along xg", lambda u: (u // ROW_DW, u % ROW_DW) if u < KB * ROW_DW else None, KB * ROW_DW)]
    for name, f, slots in rows:
        rd, wr = blocks(f, slots)
        print("%-44s %-28s %s" % (name, "%d %d %d" % rd, "%d %d %d" % wr))
    for tk, txg in ((8, 4), (4, 8), (16, 2), (2, 16)):
        rd, wr = tiled(tk, txg)
        print("%-44s %-28s %s" % ("blocks, %d k x %d xg per half-wave%s" % (tk, txg, " (built)" if tk == 8 else ""), "%d %d %d" % rd, "%d %d %d" % wr))
