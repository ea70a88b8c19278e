// mg_mystery_endless.hpp -- Endless-MysteryPath-v0, the device functions: the segment store, the two halves of a step around a due segment (emp_step_a / emp_step_b),
// the resets, one queue entry (emp_serve_entry), lazy initial segments and records ahead of time.  Its kernels: mg_mystery_endless_launch.hpp.
#pragma once
#include "mg_family.hpp"
#include "mg_mystery_path.hpp"

namespace mg {
// CharacterController.step for Endless-MysteryPath (unclamped), whose x is EMP_AX (the finite variants' is move_agent)
__device__ __forceinline__ void emp_move_agent(const MysteryParams& P, MysteryCore& s, int a0, int a1) {
    int ax = EMP_AX(s), ay = s.ay;
    free_move(a0, a1, P.v_axis_i, P.v_diag_i, ax, ay, s.rot8, false, P.agent_radius, SCREEN - P.agent_radius, P.agent_radius,
              SCREEN - P.agent_radius);
    EMP_AX(s) = ax;
    s.ay = (int16_t)ay;
}

__device__ __forceinline__ uint8_t* seg_ptr(const MysteryIO& io, int i, int seg) {
    return io.segs + ((size_t)i * io.seg_rows + seg) * SEG_STRIDE;
}
__device__ __forceinline__ int node_x(int seg, uint8_t b) { return seg * (G + 1) + (b & 7); }
__device__ __forceinline__ int node_y(uint8_t b) { return (b >> 3) & 7; }

// One 52-byte segment record in registers.  The segment store is cold in every step (the observation stream evicts
// it), so walking it byte by byte made each access a dependent ~1 us global round trip; a record is fetched with 13
// dword loads in flight together and then indexed in registers.
struct SegRec {
    uint32_t w[SEG_STRIDE / 4];
    int seg;  // -1: nothing loaded
    __device__ __forceinline__ void load(const MysteryIO& io, int i, int sg) {
        if (sg == seg) return;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(seg_ptr(io, i, sg));
#pragma unroll
        for (int j = 0; j < SEG_STRIDE / 4; ++j) w[j] = p[j];
        seg = sg;
    }
    // the record of segment sg: from `other` if that holds it (prefetched), else from memory
    __device__ __forceinline__ void load_or_take(const MysteryIO& io, int i, int sg, const SegRec& other) {
        if (sg == seg) return;
        if (other.seg == sg) {
#pragma unroll
            for (int j = 0; j < SEG_STRIDE / 4; ++j) w[j] = other.w[j];
            seg = sg;
            return;
        }
        load(io, i, sg);
    }
    __device__ __forceinline__ uint8_t byte(int p) const {  // p = 0: node count, 1..: nodes
        uint32_t v = w[0];
#pragma unroll
        for (int j = 1; j < SEG_STRIDE / 4; ++j) v = (p >> 2) == j ? w[j] : v;
        return (uint8_t)(v >> (8 * (p & 3)));
    }
};

// EndlessMysteryPath.add_path_segment (pygame_assets.py:544-604), served by the whole wave: every lane passes the number
// of segments its instance still needs (3 at reset, 1 when the agent enters the last-but-one segment, else 0).  All 64
// lanes, converged.  The finished record is assembled in LDS and written to the instance's segment store as 13 dwords.
__device__ void serve_emp(const MysteryIO& io, const PathWS& W, int i, int want, MysteryCore& s, Pcg& g) {
    const int lane = threadIdx.x & 63;
    int todo_n = want;
    WaveRng wr;
    if (__ballot(todo_n > 0)) wr.load_jump(W.jump);
    for (;;) {
        const uint64_t todo = __ballot(todo_n > 0);
        if (!todo) break;
        const int L = __ffsll((unsigned long long)todo) - 1;
        Pcg bg = bcast(g, L);
        wr.take(bg);
        const int have = bcast((int)s.have_start, L), endy = bcast((int)s.end_y, L);
        const int sy = have ? endy : wr.integers(0, G);
        const int ey = wr.integers(0, G);
        int node = 0;
        uint64_t pm = 0;
        uint64_t walls_unused = 0;
        int len = coop_path(wr, W, 0, sy, G - 1, ey, node, pm, walls_unused);
        wr.give(bg);
        if (len < 0) {
            if (lane == 0) raise_error(io.err, 2);
            len = 0;
        }
        // the segment record as stored: byte 0 = node count, bytes 1..len = the path START first (our list is END first:
        // position p sits in lane len-1-p), byte len+1 = the transition node at x = 8*seg + 7, zeros after it.
        // Assembled in LDS by 52 lanes, written by 13 lanes as dwords (the requester alone copied it byte by byte before).
        uint8_t* stage = W.stage();
        {
            const int from = len - lane;  // lane b in 1..len holds path position b-1
            const int nd = __shfl(node, from >= 0 && from < 64 ? from : 0);
            const int x = nd / G, y = nd - x * G;
            int b = 0;
            if (lane == 0) b = len + 1;
            else if (lane <= len) b = x | (y << 3);
            else if (lane == len + 1) b = 7 | (ey << 3);
            stage[lane] = (uint8_t)b;
        }
        const int nseg = bcast((int)s.num_seg, L);
        if (nseg < io.seg_rows && lane < SEG_STRIDE / 4)
            reinterpret_cast<uint32_t*>(seg_ptr(io, bcast(i, L), nseg))[lane] = reinterpret_cast<const uint32_t*>(stage)[lane];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the requester's lane reads the record back (emp_post_reset, SegRec)
        if (lane == L) {
            g = bg;
            s.have_start = 1;
            s.end_y = (int8_t)ey;
            EMP_PRE(s) = 0;  // the stream has moved: a record generated ahead of time no longer continues it
            if (s.num_seg >= io.seg_rows) raise_error(io.err, 4);
            else s.num_seg++;
            todo_n--;
        }
    }
}

// nxt_seg / nxt_w0: dword 0 (node count + first three nodes) of segment nxt_seg if the caller has requested it early, else -1
__device__ void emp_direction(const MysteryIO& io, int i, MysteryCore& s, float* gt, SegRec& R, int nxt_seg = -1, uint32_t nxt_w0 = 0) {
    R.load(io, i, s.cur_node_seg);
    const uint8_t cb = R.byte(1 + s.cur_node_idx);
    int cx = node_x(s.cur_node_seg, cb), cy = node_y(cb);
    int nseg = s.cur_node_seg, nidx = s.cur_node_idx + 1;
    if (nidx >= R.byte(0)) {
        nseg++;
        nidx = 0;
    }
    if (nseg < s.num_seg) {
        uint8_t nb;
        if (nseg == R.seg) {
            nb = R.byte(1 + nidx);
        } else if (nseg == nxt_seg && nidx == 0) {
            nb = (uint8_t)(nxt_w0 >> 8);
        } else {  // first node of the following segment (keeps R on the current one for the past-path walk)
            nb = seg_ptr(io, i, nseg)[1 + nidx];
        }
        int x = node_x(nseg, nb) - cx, y = node_y(nb) - cy;
        if (x == 1) { s.td[0] = 1; s.td[1] = 0; s.td[2] = 0; }
        else if (y == -1) { s.td[0] = 0; s.td[1] = 1; s.td[2] = 0; }
        else if (y == 1) { s.td[0] = 0; s.td[1] = 0; s.td[2] = 1; }
    }
    if (gt) {
        gt[0] = (float)s.td[0];
        gt[1] = (float)s.td[1];
        gt[2] = (float)s.td[2];
    }
}

// ---- the past-path walk on whole segment records (emp_fill_desc) ----
// Highest position p in [1, hi] of a record whose node lies in column x_rel == rel, 0 if none (rel > 7: none).  Four node bytes per word;
// ~((x + 0x7F..) | x | 0x7F..) flags exactly the zero bytes of x (bytes <= 7 here: no carry between bytes).
__device__ __forceinline__ int seg_last_in_column(const uint32_t (&w)[SEG_STRIDE / 4], int hi, int rel) {
    int pos = 0;
    const uint32_t t4 = (uint32_t)(rel & 7) * 0x01010101u;
    const bool possible = rel <= 7;
#pragma unroll
    for (int j = 0; j < SEG_STRIDE / 4; ++j) {  // (upwards: the highest word with a match is taken last)
        const uint32_t x = (w[j] & 0x07070707u) ^ t4;
        uint32_t z = ~((x + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in every byte of x that is zero
        const int last = hi - 4 * j;                            // bytes 0 .. last of this word are positions <= hi
        if (j >= 2 && !__ballot(last >= 0)) break;              // (no lane of the wave has a node this far into its record: paths are ~10-20 nodes)
        const uint32_t upto = last >= 3 ? 0xFFFFFFFFu : (last < 0 ? 0u : (0xFFFFFFFFu >> (8 * (3 - last))));
        z &= upto;
        if (j == 0) z &= ~0xFFu;  // byte 0 of the record is the node count
        if (z) pos = 4 * j + ((31 - __clz((int)z)) >> 3);
    }
    return possible ? pos : 0;
}
// Occupancy of the nodes at positions lo .. hi of a record: bit 8 x_rel + y (bits 8 x_rel + 7 stay clear).  Bytes outside the range are
// replaced by a node (7, 7) that no path has (y <= 6) before the four bytes of a word are turned into bits.
__device__ __forceinline__ uint64_t seg_occupancy(const uint32_t (&w)[SEG_STRIDE / 4], int lo, int hi) {
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < SEG_STRIDE / 4; ++j) {
        const int first = lo - 4 * j, last = hi - 4 * j;  // bytes first .. last of this word are in range
        if (j >= 2 && !__ballot(last >= 0)) break;        // (wave-uniform: nothing of any lane's range lies in this word or behind it)
        const uint32_t from = first <= 0 ? 0xFFFFFFFFu : (first > 3 ? 0u : (0xFFFFFFFFu << (8 * first)));
        const uint32_t upto = last >= 3 ? 0xFFFFFFFFu : (last < 0 ? 0u : (0xFFFFFFFFu >> (8 * (3 - last))));
        const uint32_t keep = from & upto;
        const uint32_t sw = ((w[j] & 0x07070707u) << 3) | ((w[j] >> 3) & 0x07070707u);  // x_rel and y swapped: 8 x_rel + y per byte
        const uint32_t v = (sw & keep) | (0x3F3F3F3Fu & ~keep);
        m |= 1ull << (v & 63u);
        m |= 1ull << ((v >> 8) & 63u);
        m |= 1ull << ((v >> 16) & 63u);
        m |= 1ull << (v >> 24);
    }
    return m & 0x7F7F7F7F7F7F7F7Full;
}
// The occupancy of one segment (8 columns x 7 rows, a byte per column) into the descriptor's mask: bit 7 col + y, col = cbase + x_rel
// (cbase = the segment's first column minus past_x, -8 .. 15; columns outside 0 .. 15 hold no node of the walk)
__device__ __forceinline__ void emp_deposit(uint64_t occ, int cbase, uint64_t& mask0, uint64_t& mask1) {
    uint64_t dense = 0;  // 7 bits per column, column x_rel at bit 7 x_rel
#pragma unroll
    for (int c = 0; c < 8; ++c) dense |= ((occ >> (8 * c)) & 0x7Full) << (7 * c);
    const int sh = 7 * cbase;  // -56 .. 105
    if (sh >= 64) {
        mask1 |= dense << (sh - 64);
    } else if (sh > 0) {
        mask0 |= dense << sh;
        mask1 |= dense >> (64 - sh);
    } else {
        mask0 |= dense >> (-sh);
    }
}

// WHOLE: the past-path walk on whole records (the step kernel, one lane per instance: its longest phase under a path-following agent);
// false: the reference's loop -- the fused raster / service launch calls this for the few instances it resets or finishes, inside a
// register budget that sets how many frame workgroups a CU holds (the whole-record form there: 310 us per launch instead of 135).
template <bool WHOLE>
__device__ void emp_fill_desc(const MysteryParams& P, const MysteryIO& io, int i, const MysteryCore& s, MysteryDesc& d, int nx, SegRec& R,
                              const SegRec Rprev) {  // (by value: as a reference the caller's record stayed in scratch)
    memset(&d, 0, sizeof(d));
    d.valid = 1;
    d.sprite = s.rot8;
    d.sx = (int16_t)((s.sx * P.tile + P.agent_radius - P.sprite_dim / 2) - P.camera_offset);  // agent_draw_x (fixed at reset)
    d.sy = (int16_t)(s.ay - P.sprite_dim / 2);
    d.cross_on = (P.visual_feedback && s.cross_on) ? 1 : 0;
    d.cross_x = (int16_t)(s.cross_x - P.cross_dim / 2);
    d.cross_y = (int16_t)(s.cross_y - P.cross_dim / 2);
    d.bg_on = P.show_background ? 1 : 0;
    d.bg_phase = s.bg;
    if (P.show_stamina) {
        d.stamina_on = 1;
        int st = s.stamina < P.stamina_level ? s.stamina : P.stamina_level;
        d.stamina_red = (uint8_t)(int)(SCREEN * (1 - ((double)st / P.stamina_level)));
    }
    uint64_t mask0 = 0, mask1 = 0;
    if (P.show_past_path) {  // _draw_past_path (endless_mystery_path.py:111-132)
        const int x0 = nx - 1;
        if (x0 >= 0) {
            const int past_x = x0 - P.depth > 0 ? x0 - P.depth : 0;
            d.tile_x0 = past_x * P.tile - s.camera_x;
            // The reference walks the path backwards from the node before the agent's, tile by tile, until it has drawn one in column
            // past_x.  As a loop per lane that was the longest phase of the step under an agent that FOLLOWS its path (up to ~35 tiles,
            // each a run-time indexed byte of a record held in registers: 9.8 us of a wave's 20, profiles/r06_emp.md).  The walk only
            // ever touches the record of the current node's segment and the one before it (the window is at most depth + 2 <= 9 columns,
            // a segment has 8, and the stored path is 4-connected), so it is done on whole records instead: the STOP position = the
            // last node before the agent's in column past_x (four node bytes per word, exact zero-byte flags), the tiles = the nodes
            // between it and the agent's as a 64-bit occupancy (bit 8 x_rel + y), repacked to the descriptor's 7 bits per column.
            const int C = s.cur_node_seg;
            const bool cur_in_R = C == R.seg, cur_in_prev = C == Rprev.seg;
            // (depth < 2: the first node of the walk may already lie left of past_x when the agent has just stepped off the path -- the
            // reference's loop ends there; the whole-record form assumes the walk starts inside the window.  Uniform per handle.)
            const bool generic = !WHOLE || P.depth < 2 || !(cur_in_R || cur_in_prev) || (cur_in_R && C > 0 && Rprev.seg != C - 1);
            bool done_fast = false;
            if constexpr (WHOLE) if (__builtin_expect(!generic, 1)) {
                uint32_t wc[SEG_STRIDE / 4];
#pragma unroll
                for (int j = 0; j < SEG_STRIDE / 4; ++j) wc[j] = cur_in_R ? R.w[j] : Rprev.w[j];
                const int hi_c = s.cur_node_idx;  // positions 1 .. cur_node_idx hold the nodes before the agent's
                const int rel_c = past_x - C * (G + 1);
                const int stop_c = (rel_c >= 0 && hi_c >= 1) ? seg_last_in_column(wc, hi_c, rel_c) : 0;
                const uint64_t occ_c = seg_occupancy(wc, stop_c ? stop_c : 1, hi_c);
                emp_deposit(occ_c, C * (G + 1) - past_x, mask0, mask1);
                done_fast = true;
                if (!stop_c && C > 0) {  // the walk goes on in the segment before
                    if (cur_in_R) {
                        const int n_p = (int)(Rprev.w[0] & 0xFFu);
                        const int rel_p = past_x - (C - 1) * (G + 1);
                        const int stop_p = rel_p >= 0 ? seg_last_in_column(Rprev.w, n_p, rel_p) : 0;
                        const uint64_t occ_p = seg_occupancy(Rprev.w, stop_p ? stop_p : 1, n_p);
                        emp_deposit(occ_p, (C - 1) * (G + 1) - past_x, mask0, mask1);
                        if (!stop_p && C - 1 > 0) done_fast = false;  // (cannot happen: past_x >= 8 C - 8; the loop below is the definition)
                    } else {
                        done_fast = false;  // (the segment before the previous one: cannot happen either, see above)
                    }
                }
            }
            if (__builtin_expect(!done_fast, 0)) {  // the reference's loop, literally
                mask0 = mask1 = 0;
                int x = x0, seg = s.cur_node_seg, idx = s.cur_node_idx - 1;
                while (x >= past_x && x >= 0) {
                    if (idx < 0) {
                        seg--;
                        if (seg < 0) break;
                        R.load_or_take(io, i, seg, Rprev);
                        idx = R.byte(0) - 1;
                    }
                    R.load_or_take(io, i, seg, Rprev);
                    uint8_t b = R.byte(1 + idx);
                    x = node_x(seg, b);
                    int y = node_y(b);
                    int col = x - past_x;
                    if (col >= 0 && col < 16) {
                        const int cell = col * G + y;  // (a run-time index into d.tile_mask would put the descriptor into scratch)
                        const uint64_t bit = 1ull << (cell & 63);
                        if (cell < 64) mask0 |= bit;
                        else mask1 |= bit;
                    } else if (col >= 16) {
                        raise_error(io.err, 16);
                    }
                    if (x == past_x) break;
                    idx--;
                }
            }
        }
    }
    d.tile_mask[0] = mask0;
    d.tile_mask[1] = mask1;
}

// ---- lazy initial segments --------------------------------------------------------------------------------------------
// The reference's reset generates three path segments (endless_mystery_path.py:222-224 -> pygame_assets.py:523-527), ~30 us
// of dependent work each for a wave: the critical path of the step's fused raster / service launch.  Only the FIRST one is
// needed for the reset frame, its ground truth and the next steps (the agent starts eight tiles before the second): with
// P.lazy a reset generates one segment and records two as OWED (MysteryCore::path_len); each of the instance's next steps
// queues ONE owed segment as a background job nobody waits for -- served by the lane-per-path generator beside the frames
// (emp_raster_serve_kernel) -- and everything that could observe the difference generates what is owed first: a step that
// gets near the end of what exists (emp_step_a), the next reset (RNG order: the old episode's owed segments are generated,
// and discarded, before the new episode's first), and every look at the state (Family::sync_state: checkpoints, RNG words,
// the debug view).  The instance's random numbers are consumed in exactly the reference's order; nothing else draws from
// the stream of an Endless Mystery Path instance.
// ---- the next episode's first segment, ahead of time (round 5) ------------------------------------------------------------
// With lazy resets a step's queue still held one entry per finishing instance (~1,200 of 32,768 per step under random
// actions): one path of the wave-cooperative generator each, ~30 us of a wave's time and the reason the fused launch needs ~200
// registers per lane.  But nothing draws from an Endless-MysteryPath instance's stream except its segments, so once an episode's
// segments exist the stream stands exactly where the NEXT reset will find it -- unless the agent reaches the last-but-one segment
// first and a new one is appended.  P.pre: an instance that is owed nothing and has no such record generates the next episode's
// first segment as one more background job (lane-per-path generator, beside the frames, from a COPY of its stream) into
// io.aux[i], with the stream as it stands behind it; EMP_PRE(s) says the record is there.  A step that ends the episode then
// resets the instance itself (emp_step_b<true>): the record becomes segment 0, the instance's stream becomes the record's, two
// segments are owed -- the same draws in the same order as the reference's reset, and no queue entry.  Whatever advances
// the stream first (a due segment, any other reset path) clears the flag; the record is never looked at without it.

// EndlessMysteryPathEnv.reset (endless_mystery_path.py:195-280) around the three initial segments (serve_emp)
__device__ __forceinline__ void emp_pre_reset(MysteryCore& s) {
    s.t = 0;
    s.ep_sum = 0.0;
    s.ep_len = 0;
    s.num_seg = 0;
    s.have_start = 0;
    EMP_PRE(s) = 0;
}
// everything of the reset behind the segments except the frame descriptor; R: segment 0's record, its first node flagged
__device__ __forceinline__ void emp_post_reset_state(const MysteryParams& P, const MysteryIO& io, int i, MysteryCore& s, float* gt, SegRec& R) {
    const uint8_t b1 = R.byte(1);
    s.sx = (uint8_t)node_x(0, b1);
    s.sy = (uint8_t)node_y(b1);
    s.camera_x = P.camera_offset;
    s.bg = 0;
    s.ax = 0;  // (finite variants only)
    EMP_AX(s) = s.sx * P.tile + P.agent_radius;
    s.ay = (int16_t)(s.sy * P.tile + P.agent_radius);
    s.rot8 = 6;  // 270 degrees
    s.cur_node_seg = 0;
    s.cur_node_idx = 0;
    emp_direction(io, i, s, gt, R);
    s.off = 0;
    s.cross_on = 0;
    s.cross_x = s.cross_y = 0;
    s.cur_seg = 0;
    s.fails = 0;
    s.n_falloff = 0;
    EMP_FLO(s) = 0x7FFFFFFF;  // no segment holds a stamina flag
    EMP_FHI(s) = -1;
    s.stamina = P.stamina_level;
    s.max_x = 0;
    s.tiles_visited = 0;
}
__device__ void emp_post_reset(const MysteryParams& P, const MysteryIO& io, int i, MysteryCore& s, MysteryDesc& d, float* gt) {
    SegRec R;
    R.seg = -1;
    R.load(io, i, 0);
    R.w[0] |= 0x4000u;  // the first node of the path shall not yield any reward (bit 6 of byte 1)
    *reinterpret_cast<uint32_t*>(seg_ptr(io, i, 0)) = R.w[0];
    emp_post_reset_state(P, io, i, s, gt, R);
    SegRec none;
    none.seg = -1;
    emp_fill_desc<false>(P, io, i, s, d, EMP_AX(s) / P.tile, R, none);
    d.cross_on = 0;
    if (P.show_stamina) d.stamina_red = 0;
}

// EndlessMysteryPathEnv.step (endless_mystery_path.py:282-444), first part: move; returns 1 if a new segment is due
// (`current_segment > num_segments - 2`, :333-335), which the wave then generates before the second part runs.
// Bit 0 of the result: a segment is due; bit 1: the instance has reached the capacity of its segment store (EMP_CAP).
constexpr int EMP_DUE = 1, EMP_CAP = 2;
__device__ int emp_step_a(const MysteryParams& P, int i, MysteryCore& s, int a, int& nx, int& ny, int* io_err) {
    int a0 = a == 1 ? 2 : 0, a1 = a == 2 ? 1 : (a == 3 ? 2 : 0);
    if (!s.off) {
        const int before = EMP_AX(s);
        emp_move_agent(P, s, a0, a1);
        const int vx = EMP_AX(s) - before;
        s.camera_x += vx;  // camera follows the agent's x velocity
        // bg_scroll -= velocity.x; once |bg_scroll| >= tile it becomes (|bg_scroll| % |velocity.x|) * sign, which is 0:
        // it has only ever moved in steps of the same velocity.x (endless_mystery_path.py:311-316)
        int bg = s.bg + vx;
        s.bg = (uint8_t)(bg >= P.tile ? bg % vx : bg);
    } else {
        s.bg = 0;
        EMP_AX(s) = s.sx * P.tile + P.agent_radius;
        s.ay = (int16_t)(s.sy * P.tile + P.agent_radius);
        emp_move_agent(P, s, 0, 0);
        s.camera_x = P.camera_offset;
    }
    nx = floordiv_pos(EMP_AX(s), P.tile);
    ny = floordiv_pos(s.ay, P.tile);
    s.cur_seg = nx / (G + 1);
    // `current_segment > num_segments - 2` counts the owed segments as the reference has them; and whatever this step could
    // read of a segment that is still owed (the next node's direction at the end of the last generated segment) makes the
    // owed ones due now -- conservative: within two columns of the end of what exists
    int owed = EMP_OWED(s);
    if (s.cur_seg > s.num_seg + owed - 2 && s.num_seg + owed >= P.seg_cap) {
        // the segment store is full (the reference's list is unbounded, pygame_assets.py:559): nothing is appended, this step ends the
        // episode and says why (include/memgym.h: mg_info_buffers.capacity_dev, error bit 4); what is owed is generated if the step can see it
        raise_error(io_err, 4);
        return 2 | ((owed > 0 && nx >= (G + 1) * s.num_seg - 2) ? 1 : 0);
    }
    if (s.cur_seg > s.num_seg + owed - 2) {
        // Round 5: the segment the reference appends now (:333-335) is OWED like a reset's second and third -- the agent has only
        // entered the last but one, the new one starts eight columns ahead -- and generated by the next background job instead of by
        // a queue entry of this step (an agent that follows its path appended one every ~8 steps: thousands of cooperative paths per
        // step at 32,768 instances).  Nothing else draws from the stream, so the order of its draws is the reference's.
        if (!P.lazy_append || owed >= 200) return 1;
        EMP_OWED(s) = (uint8_t)(++owed);
        EMP_PRE(s) = 0;  // (a record ahead of time continued the stream as it stood BEFORE this segment)
    }
    return (owed > 0 && nx >= (G + 1) * s.num_seg - 2) ? 1 : 0;
}
#ifdef MG_LAB_EMP_CLOCK
__global__ void lab_wbl2_kernel() { asm volatile("buffer_wbl2 sc0 sc1\n\ts_waitcnt vmcnt(0)" ::: "memory"); }
#endif
#ifdef MG_LAB_EMP_CLOCK  // measurement builds only: phases of emp_step_kernel per wave (constant-rate clock, 10 ns)
static __device__ unsigned long long g_lab_step_clock[12 * 4096];
#define LAB_STEP_CLOCK(slot) do { const int wv_ = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; \
    __builtin_amdgcn_s_waitcnt(0); /* everything issued so far has completed: the phases are what the wave waited for */ \
    if ((threadIdx.x & 63) == __builtin_ctzll(__ballot(1)) && wv_ < 4096) g_lab_step_clock[12 * wv_ + (slot)] = wall_clock64(); } while (0)
#else
#define LAB_STEP_CLOCK(slot) do { } while (0)
#endif

// second part; returns true if the instance finished and is to be reset in this call by somebody else (a queue entry).
// OWN_RESET (emp_step_kernel): an instance whose next episode's first segment exists already (EMP_PRE) is reset right here, and
// everything the step can need from memory -- the segment records AND the instance's aux line (that record, the head of the
// fall-off list) -- is requested in ONE batch: the kernel is a chain of dependent memory round trips on 512 waves (~2 us each on a
// memory system the observation stream has just swept; rounds 3-4: records, then the fall-off list, then the stamina flags'
// records, then the queue's counter), not a matter of bytes (profiles/r03_emp.md section 7, r05_emp.md).
// FINAL (mg_step with mg_info_buffers.final_obs_dev, round 6): the frame descriptor of a finished instance's TERMINAL state goes to
// io.tdesc[i] before anybody resets it (drawn into final_obs_dev by a sparse raster launch behind the fused one); the tail runs twice for
// such an instance -- one copy of emp_fill_desc either way, and for FINAL = false the code of rounds 3-5 (a loop of exactly one pass).
template <bool OWN_RESET, bool WHOLE_DESC = false, bool FINAL = false>
__device__ bool emp_step_b(const MysteryParams& P, const MysteryIO& io, int i, MysteryCore& s, int nx, int ny, float* reward_out,
                           uint8_t* done_out, float* gt, const mg_info_dev& info, int autoreset, MysteryDesc& d, bool cap = false) {
    typedef uint32_t q4 __attribute__((ext_vector_type(4)));
    double reward = 0.0;
    bool done = cap;  // cap: the segment store is full and the reference would append now (emp_step_a) -- the episode ends here
    const int seg = s.cur_seg;
    SegRec R, Rprev;
    R.seg = -1;
    Rprev.seg = -1;
    // The segment store is cold (6.6 KB per instance, evicted by the observation stream): every dependent access is a ~2 us
    // round trip.  The records this step can touch -- the agent's segment, the one before it (past-path tiles), the head of
    // the one after it (the direction to the next node) -- are requested together, before the first of them is used.
    // (the next segment's head is read unconditionally, from a clamped index: inside a branch the compiler consumed it there
    // and waited for it before the two records were even requested)
    const int nxt_seg = seg + 1 < s.num_seg ? seg + 1 : -1;
    const int nxt_safe = nxt_seg >= 0 ? nxt_seg : 0;
    uint32_t* const aux = io.aux + (size_t)i * AUX_WORDS;
    uint32_t nxt_w0 = *reinterpret_cast<const uint32_t*>(seg_ptr(io, i, nxt_safe));
    // (both records unconditionally too, from clamped indices -- segment 0's slot always exists: behind a branch the compiler waits
    // for a load where the branches join, i.e. before the next request is issued)
    const bool have_prev = seg >= 1 && seg - 1 < s.num_seg, have_cur = seg >= 0 && seg < s.num_seg;
    Rprev.load(io, i, have_prev ? seg - 1 : 0);
    R.load(io, i, have_cur ? seg : 0);
    Rprev.seg = have_prev ? seg - 1 : -1;
    R.seg = have_cur ? seg : -1;
    q4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0, a4 = a0, f0 = a0, f1 = a0, f2 = a0;
    if (OWN_RESET) {
        const q4* aq = reinterpret_cast<const q4*>(aux);
        a0 = aq[0]; a1 = aq[1]; a2 = aq[2]; a3 = aq[3]; a4 = aq[4];  // the record generated ahead of time
        f0 = aq[5]; f1 = aq[6]; f2 = aq[7];                          // fall-off keys 0..11
        asm volatile("" : "+v"(f2));  // (a use the compiler cannot move: every request above is issued before the first wait)
    }
    asm volatile("" : "+v"(nxt_w0));
    LAB_STEP_CLOCK(5);
    bool on_path = false;
    if (seg < s.num_seg) {
        uint8_t* sp = seg_ptr(io, i, seg);
        const uint32_t* w = R.w;
        const int n = (int)(w[0] & 0xFFu);
        const int dx = nx - seg * (G + 1);
        const bool addressable = (unsigned)dx < 8u && (unsigned)ny < 8u;  // node bytes hold x_rel and y in 3 bits each
        const uint32_t target = (uint32_t)(dx & 7) | ((uint32_t)(ny & 7) << 3);
        // first node (list order) on the agent's tile, four node bytes per word at once (round 5; byte by byte the search was
        // 2.7 us of every wave's 17): a byte's low six bits equal the target iff they XOR to zero, and in (x - 0x01..) & ~x &
        // 0x80.. the LOWEST flag marks the lowest zero byte exactly.  Bytes behind the list are zero and can only match behind
        // every real node: a first match beyond the node count means there is none.
        int hit = 0;
        uint32_t hb = 0;
        const uint32_t t4 = target * 0x01010101u;
#pragma unroll
        for (int j = SEG_STRIDE / 4 - 1; j >= 0; --j) {  // (downwards: the lowest word with a match is taken last)
            uint32_t x = (w[j] & 0x3F3F3F3Fu) ^ t4;
            if (j == 0) x |= 0xFFu;  // byte 0 is the node count
            const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;
            if (z) {
                const int k = (__ffs((int)z) - 1) >> 3;
                hit = 4 * j + k;
                hb = (w[j] >> (8 * k)) & 0xFFu;
            }
        }
        if (!(addressable && hit >= 1 && hit <= n)) hit = 0;
        if (hit) {
            uint8_t b = (uint8_t)hb;
            on_path = true;
            s.cur_node_seg = seg;
            s.cur_node_idx = hit - 1;
            bool is_start = nx == s.sx && ny == s.sy;
            if (!(b & 0x40) && !is_start) {
                reward += P.r_progress;
                s.tiles_visited++;
                b |= 0x40;
            }
            if (!(b & 0x80) && !is_start) {
                reward += P.r_dense;
                s.stamina = P.stamina_level;
                b |= 0x80;
                EMP_FLO(s) = seg < EMP_FLO(s) ? seg : EMP_FLO(s);  // segments that may hold stamina flags
                EMP_FHI(s) = seg > EMP_FHI(s) ? seg : EMP_FHI(s);
            }
            sp[hit] = b;
        }
    }
    LAB_STEP_CLOCK(6);
    if (!on_path) {
        reward += P.r_fall;
        s.fails++;
        if (P.visual_feedback) s.cross_on = 1;
        s.off = 1;
        if (nx < s.max_x) {
            done = true;
        } else {
            uint32_t* fl = aux + AUX_FALL;
            const uint32_t key = emp_fall_key(nx, ny);
            const int nf = s.n_falloff;
            bool found = false;
            int k0 = 0;
            if (OWN_RESET) {  // the first twelve keys came with the batch above; slots >= n_falloff hold stale keys
                found = (0 < nf && f0.x == key) || (1 < nf && f0.y == key) || (2 < nf && f0.z == key) || (3 < nf && f0.w == key) ||
                        (4 < nf && f1.x == key) || (5 < nf && f1.y == key) || (6 < nf && f1.z == key) || (7 < nf && f1.w == key) ||
                        (8 < nf && f2.x == key) || (9 < nf && f2.y == key) || (10 < nf && f2.z == key) || (11 < nf && f2.w == key);
                k0 = 12;
            }
            for (int k = k0; k < nf; k += 4) {  // four entries per load
                const uint4 v = reinterpret_cast<const uint4*>(fl)[k >> 2];
                found = found || v.x == key || (k + 1 < nf && v.y == key) || (k + 2 < nf && v.z == key) || (k + 3 < nf && v.w == key);
            }
            if (found) done = true;
            if (!found) {
                if (s.n_falloff < P.fall_cap) fl[s.n_falloff++] = key;
                else {  // the list of fall-off cells is full (the reference's is unbounded, endless_mystery_path.py:385-393): the episode ends
                    raise_error(io.err, 8);
                    done = cap = true;
                }
            }
        }
        // reset all stamina flags -- only segments visited since the last reset can hold any; whole records at a time
        // (bytes past the node count are unused).  The agent's segment and the one before it are in registers already, as they
        // are in memory (no node was flagged in this step: the agent is not on the path).
        for (int q = EMP_FLO(s); q <= EMP_FHI(s) && q < s.num_seg; ++q) {
            uint32_t* wp = reinterpret_cast<uint32_t*>(seg_ptr(io, i, q));
            uint32_t w[SEG_STRIDE / 4];
            if (q == R.seg) {
#pragma unroll
                for (int j = 0; j < SEG_STRIDE / 4; ++j) w[j] = R.w[j];
            } else if (q == Rprev.seg) {
#pragma unroll
                for (int j = 0; j < SEG_STRIDE / 4; ++j) w[j] = Rprev.w[j];
            } else {
#pragma unroll
                for (int j = 0; j < SEG_STRIDE / 4; ++j) w[j] = wp[j];
            }
            wp[0] = w[0] & 0x7F7F7FFFu;  // byte 0 is the node count
#pragma unroll
            for (int j = 1; j < SEG_STRIDE / 4; ++j) wp[j] = w[j] & 0x7F7F7F7Fu;
        }
        EMP_FLO(s) = 0x7FFFFFFF;
        EMP_FHI(s) = -1;
        s.stamina = P.stamina_level;
    } else {
        s.cross_on = 0;
        s.off = 0;
    }
    LAB_STEP_CLOCK(7);
    s.cross_x = (int16_t)(EMP_AX(s) - s.camera_x);  // (relative to the camera, which moves with the agent: a few tiles at most)
    s.cross_y = s.ay;
    reward += P.r_step;
    s.stamina--;
    if (s.stamina == 0) done = true;
    s.t++;
    if (s.t == P.max_steps) done = true;
    emp_direction(io, i, s, gt, R, nxt_seg, nxt_w0);
    LAB_STEP_CLOCK(8);
    if (nx > s.max_x && on_path) s.max_x = nx;
    s.ep_sum += reward;
    s.ep_len++;
    if (done) {
        if (info.ep_reward_dev) info.ep_reward_dev[i] = s.ep_sum;
        if (info.ep_length_dev) info.ep_length_dev[i] = s.ep_len;
        if (info.aux_dev[0]) info.aux_dev[0][i] = (float)s.fails;
        if (info.aux_dev[1]) info.aux_dev[1][i] = (float)s.max_x;
        if (info.aux_dev[2]) info.aux_dev[2][i] = (float)s.tiles_visited;
    }
    reward_out[i] = (float)reward;
    if (info.reward64_dev) info.reward64_dev[i] = reward;  // the reference's Python float, unrounded
    done_out[i] = done ? 1 : 0;
    if (info.capacity_dev) info.capacity_dev[i] = cap ? 1 : 0;
    LAB_STEP_CLOCK(9);
    bool fresh = false;
    auto own_reset = [&]() {
        // EndlessMysteryPathEnv.reset (endless_mystery_path.py:195-280) with the first segment taken from the record that was
        // generated ahead of time; the stream continues behind that segment's draws, the other two segments are owed
        emp_pre_reset(s);
        R.w[0] = a0.x | 0x4000u;  // the first node of the path shall not yield any reward
        R.w[1] = a0.y; R.w[2] = a0.z; R.w[3] = a0.w;
        R.w[4] = a1.x; R.w[5] = a1.y; R.w[6] = a1.z; R.w[7] = a1.w;
        R.w[8] = a2.x; R.w[9] = a2.y; R.w[10] = a2.z; R.w[11] = a2.w;
        R.w[12] = a3.x;
        R.seg = 0;
        Rprev.seg = -1;
        uint32_t* dst = reinterpret_cast<uint32_t*>(seg_ptr(io, i, 0));
#pragma unroll
        for (int j = 0; j < SEG_STRIDE / 4; ++j) dst[j] = R.w[j];
        io.rng.s_lo[i] = (uint64_t)a4.x | ((uint64_t)a4.y << 32);
        io.rng.s_hi[i] = (uint64_t)a4.z | ((uint64_t)a4.w << 32);
        io.rng.buf[i] = (uint64_t)a3.y | ((uint64_t)(a3.z & 1u) << 32);
        s.num_seg = 1;
        s.have_start = 1;
        s.end_y = (int8_t)((a3.z >> 8) & 0xFFu);
        EMP_OWED(s) = 2;
        if (LAB_BUILD && io.stats) atomicAdd(io.stats + 2, 1ull);  // mg_debug_counter "emp_own_resets" (lab build: tests)
        emp_post_reset_state(P, io, i, s, gt, R);
        nx = EMP_AX(s) / P.tile;
        fresh = true;
    };
    if (!FINAL) {  // (rounds 3-5, as it was)
        if (done && autoreset) {
            if (!(OWN_RESET && P.lazy && EMP_PRE(s) && EMP_OWED(s) == 0)) return true;
            own_reset();
        }
        emp_fill_desc<WHOLE_DESC>(P, io, i, s, d, nx, R, Rprev);
    } else {
        const bool fin = done && autoreset;
#pragma nounroll
        for (int pass = fin ? 0 : 1; pass < 2; ++pass) {  // a finished instance: the terminal descriptor first
            if (fin && pass == 1) {
                if (!(OWN_RESET && P.lazy && EMP_PRE(s) && EMP_OWED(s) == 0)) return true;
                own_reset();
            }
            emp_fill_desc<WHOLE_DESC>(P, io, i, s, d, nx, R, Rprev);
            if (pass == 0) {
                io.tdesc[i] = d;
                if (LAB_BUILD && !OWN_RESET && io.stats) atomicAdd(io.stats + 4, 1ull);  // mg_debug_counter "emp_final_served" (lab build: tests)
            }
        }
    }
    if (fresh) {
        d.cross_on = 0;
        if (P.show_stamina) d.stamina_red = 0;
    }
    LAB_STEP_CLOCK(10);
    return false;
}

// One queue entry, served by one converged wave whose lane 0 plays the instance's lane: "append a segment, finish the step"
// and / or "reset" (three segments), state, stream and frame descriptor written back.
template <bool FINAL = false>
__device__ void emp_serve_entry(const MysteryParams& P, const MysteryIO& io, const PathWS& W, int entry, const int64_t* seeds, float* reward_out,
                                uint8_t* done_out, float* gt, const mg_info_dev& info, int autoreset, MysteryDesc* d_out = nullptr) {
    const bool me = (threadIdx.x & 63) == 0;
    const int i = entry & EMP_Q_INST;
    float* gti = gt ? gt + 3 * i : nullptr;
    Pcg g;
    MysteryCore s;
    MysteryDesc d;
    if (me) {
        if (seeds) g.seed((uint64_t)seeds[i]);
        else g.load(io.rng, i);
        s = io.core[i];
    } else {
        g.clear();
        memset(&s, 0, sizeof(s));
    }
    int reset_me = 1;
    if (entry & (EMP_Q_SEGMENT | EMP_Q_OWED)) {
        // the new segment is due: whatever is still owed comes first (stream order), or -- emp_step_a's conservative test --
        // only what is owed is due and `current_segment > num_segments - 2` does not hold yet
        int want = 0;
        bool cap = false;
        if (me) {
            if (entry & EMP_Q_OWED) {  // a background job: one owed segment, nothing else
                want = EMP_OWED(s) > 0 ? 1 : 0;
                EMP_OWED(s) = (uint8_t)(EMP_OWED(s) - want);
            } else {
                const bool append = s.cur_seg > s.num_seg + EMP_OWED(s) - 2;
                cap = append && s.num_seg + EMP_OWED(s) >= P.seg_cap;  // (emp_step_a has raised the error bit; the step below ends the episode)
                want = EMP_OWED(s) + ((append && !cap) ? 1 : 0);
                EMP_OWED(s) = 0;
            }
        }
        serve_emp(io, W, i, want, s, g);
        if (entry & EMP_Q_OWED) {  // only the fields a segment changes: the frame and the rest of the record are this step's already
            if (me && want) {
                io.core[i] = s;
                g.store(io.rng, i);
            }
            return;
        }
        if (me)
            reset_me = emp_step_b<false, false, FINAL>(P, io, i, s, floordiv_pos(EMP_AX(s), P.tile), floordiv_pos(s.ay, P.tile), reward_out, done_out,
                                         gti, info, autoreset, d, cap) ? 1 : 0;
        reset_me = bcast(reset_me, 0);
    }
    if (reset_me) {
        // segments the finished episode is still owed are generated first (and discarded): they come first in the stream
        const int owed_old = bcast((me && !seeds) ? (int)EMP_OWED(s) : 0, 0);  // (a re-seeded instance starts a new stream)
        if (owed_old) serve_emp(io, W, i, me ? owed_old : 0, s, g);
        if (me) emp_pre_reset(s);
        serve_emp(io, W, i, me ? (P.lazy ? 1 : 3) : 0, s, g);
        if (me) {
            EMP_OWED(s) = P.lazy ? 2 : 0;
            emp_post_reset(P, io, i, s, d, gti);
        }
    }
    if (me) {
        d.valid = DESC_SERVED;
        io.core[i] = s;
        g.store(io.rng, i);
        io.desc[i] = d;
        if (d_out) *d_out = d;  // (the fused kernel composes the frame from this copy)
    }
}

// EndlessMysteryPath.add_path_segment (pygame_assets.py:544-604) by one lane: the draws and the path; the record goes to dst
// (13 dwords: byte 0 = node count, then the path START first, then the transition node, see serve_emp).  Returns the end row.
__device__ int lane_segment_record(const MysteryIO& io, const LaneWS& W, bool have_start, int end_y, Pcg& g, uint32_t* dst) {
    const int sy = have_start ? end_y : g.integers(0, G);
    const int ey = g.integers(0, G);
    uint64_t pm = 0, wl = 0;
    int len = lane_path(g, W, 0, sy, G - 1, ey, pm, wl);
    if (len < 0) {
        raise_error(io.err, 2);
        len = 0;
    }
    if (dst) {
        for (int j = 0; j < SEG_STRIDE / 4; ++j) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int p = 4 * j + b;
                uint32_t v = 0;
                if (p == 0) v = (uint32_t)(len + 1);
                else if (p <= len) {
                    const int nd = (int)W.key(len - p);
                    v = (uint32_t)((nd / G) | ((nd % G) << 3));
                } else if (p == len + 1) v = (uint32_t)(7 | (ey << 3));
                word |= v << (8 * b);
            }
            dst[j] = word;
        }
    }
    return ey;
}
__device__ void lane_segment(const MysteryIO& io, const LaneWS& W, int i, MysteryCore& s, Pcg& g) {
    const bool room = s.num_seg < io.seg_rows;
    const int ey = lane_segment_record(io, W, s.have_start != 0, (int)s.end_y, g, room ? reinterpret_cast<uint32_t*>(seg_ptr(io, i, s.num_seg)) : nullptr);
    if (room) s.num_seg++;
    else raise_error(io.err, 4);
    s.have_start = 1;
    s.end_y = (int8_t)ey;
    EMP_PRE(s) = 0;  // the stream has moved: a record generated ahead of time no longer continues it
}

// One background job by one lane: the instance's next owed segment (lazy initial segments, EMP_OWED) -- or, ahead = true and
// nothing owed, the NEXT episode's first segment from a copy of the stream (EMP_PRE).  (One call site of the generator for both:
// with two the compiler turns it into a real function call, 1,300 B of stack per lane in the fused launch.)
__device__ __forceinline__ void lane_owed_segment(const MysteryIO& io, const LaneWS& W, int i, int how_many, bool ahead = false) {
    MysteryCore s = io.core[i];
    int owed = EMP_OWED(s);
    const bool pre_job = owed <= 0;
    if (pre_job && (!ahead || EMP_PRE(s))) return;
    Pcg g;
    g.load(io.rng, i);
    uint32_t* const rec = io.aux + (size_t)i * AUX_WORDS;
    for (int k = 0; k < how_many && (owed > 0 || pre_job); ++k) {
        const bool room = s.num_seg < io.seg_rows;
        uint32_t* dst = pre_job ? rec : (room ? reinterpret_cast<uint32_t*>(seg_ptr(io, i, s.num_seg)) : nullptr);
        // (a reset's first segment draws its start row)
        const int ey = lane_segment_record(io, W, !pre_job && s.have_start != 0, (int)s.end_y, g, dst);
        if (pre_job) {
            rec[13] = g.buf;
            rec[14] = (g.has ? 1u : 0u) | ((uint32_t)ey << 8);
            rec[16] = (uint32_t)g.state;
            rec[17] = (uint32_t)(g.state >> 32);
            rec[18] = (uint32_t)(g.state >> 64);
            rec[19] = (uint32_t)(g.state >> 96);
            EMP_PRE(s) = 1;  // (the instance's own stream stays where it is)
            io.core[i] = s;
            if (io.stats) atomicAdd(io.stats + 3, 1ull);  // mg_debug_counter "emp_ahead_records"
            return;
        }
        if (room) s.num_seg++;
        else raise_error(io.err, 4);
        s.have_start = 1;
        s.end_y = (int8_t)ey;
        EMP_PRE(s) = 0;
        --owed;
    }
    // only the fields a segment changes: the instance's record belongs to nobody else between its step and its next step
    EMP_OWED(s) = (uint8_t)owed;
    io.core[i] = s;
    g.store(io.rng, i);
}
}  // namespace mg
