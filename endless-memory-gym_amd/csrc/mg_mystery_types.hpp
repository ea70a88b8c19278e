// mg_mystery_types.hpp -- Mystery Path family: the grid and aux-line constants, the records its launches share (MysteryParams, MysteryCore, MysteryDesc, MysteryIO),
// the queue's counters and entry tags.  Every other mg_mystery_*.hpp includes this one; mg_mystery.hip says which of them holds what.
#pragma once
#include "mg_device.hpp"

namespace mg {
constexpr int G = 7;             // grid_dim
constexpr int SEG_STRIDE = 52;   // bytes per stored segment: [0] = length, [1..50] nodes
constexpr int MAX_SEG = 128;
constexpr int MAX_FALL = 128;
constexpr int ST_CROSS = 8;
constexpr int TILE = SCREEN / G;   // 12 px
// Endless: AUX_WORDS words per instance.  The first 128-byte line holds what a step may need besides the state and segment records,
// so that ONE batch of loads fetches it (emp_step_b): words 0..19 the EMP_PRE record (0..12 the segment record, SEG_STRIDE bytes; 13
// the stream's buffered half; 14 = has_buffered | end_y << 8; 16..19 the stream's 128-bit state behind the segment's draws, low word
// first), words 20..31 the first twelve fall-off keys; the list goes on behind them (MAX_FALL keys, emp_fall_key).
constexpr int AUX_FALL = 20, AUX_WORDS = 160;
static_assert(AUX_FALL + MAX_FALL <= AUX_WORDS && AUX_WORDS % 32 == 0, "the fall-off list must fit behind the record");
// A fall-off cell's key: column x in bits 0..17, row y + EMP_KEY_YBIAS in bits 18..31.  Injective over every cell an episode can fall
// into: x in 0 .. 8 * 32,767 - 1 (the agent never moves left of its start; mg_set_capacity's largest segment store ends the episode
// before it enters segment 32,767) and y in -EMP_KEY_YBIAS .. 2^14 - 1 - EMP_KEY_YBIAS (the unclamped vertical move leaves rows 0..6 by
// one tile at most).  Rounds 1-6 kept x in 16 bits: cells 65,536 columns apart shared a key (a second fall there ended the episode).
constexpr int EMP_KEY_XBITS = 18, EMP_KEY_YBIAS = 1024, EMP_MAX_SEG_CAP = 32767;
static_assert(8 * EMP_MAX_SEG_CAP <= (1 << EMP_KEY_XBITS) && EMP_KEY_YBIAS + 8 <= (1 << (32 - EMP_KEY_XBITS)), "fall-off keys must be injective");
__host__ __device__ __forceinline__ uint32_t emp_fall_key(int nx, int ny) {
    return (uint32_t)nx | ((uint32_t)(ny + EMP_KEY_YBIAS) << EMP_KEY_XBITS);
}
constexpr int STAMINA_W = 4;      // int(16 * SCALE)

struct MysteryParams {
    int endless, grid, n;
    int max_steps, show_origin, show_goal, visual_feedback, show_past_path, show_background, show_stamina, stamina_level, depth;
    int agent_radius, sprite_dim, v_axis_i, v_diag_i, tile, cross_dim;
    int camera_offset;  // integral at the supported camera_offset_scale values
    int svc_prio;       // wave priority of the path-service waves inside the fused raster launches (s_setprio)
    int lazy;           // Endless: a reset generates ONE of its three initial segments, the other two are owed (see EMP_OWED)
    int path_help;      // frame workgroups help with long path queues (MEMGYM_PATH_HELP=0: the 128 dedicated workgroups alone, round 2)
    int bg_coop;        // Endless, fused launch: owed segments as queue entries of the service waves (small launches), not one per lane of frame workgroups
    int lazy_append;    // Endless, lazy: a segment appended during an episode is owed too, not a queue entry of the step (emp_step_a)
    int pre;            // Endless, lazy: the NEXT episode's first segment is generated ahead of time as a background job (see EMP_PRE)
    int seg_cap, fall_cap;  // Endless: segments / fall-off cells an episode may reach (MAX_SEG / MAX_FALL; the lab build lowers them for tests)
    OptList cardinal;
    double r_goal, r_fall, r_progress, r_dense, r_step;
};

struct __attribute__((aligned(16))) MysteryCore {
    int16_t ax, ay;                     // ax: finite variants (endless: EMP_AX)
    uint8_t rot8, off, cross_on, path_len;  // path_len: finite variants; endless: segments OWED to the instance (EMP_OWED below)
    uint8_t sx, sy, ex, ey;
    int16_t cross_x, cross_y;           // fall_off_rect centre
    int32_t fails, t, ep_len, stamina;
    int32_t max_x, tiles_visited, cur_seg, num_seg;
    int32_t cur_node_seg, cur_node_idx, camera_x, n_falloff;
    uint64_t path_mask, visited_mask;   // finite: bit (x*7+y); endless: EMP_AX (path_mask), EMP_FLO / EMP_FHI (visited_mask)
    double ep_sum;
    uint8_t td[3], have_start;
    int8_t end_y;
    uint8_t gx, gy;       // grid controller position (MysteryPath-Grid-v0)
    uint8_t bg;           // endless: -bg_scroll, the scrolling background's phase in pixels (< tile)
};
static_assert(sizeof(MysteryCore) == 96, "MysteryCore must be 96 bytes");
// endless: [EMP_FLO, EMP_FHI] = range of segments that may hold stamina flags (empty: lo > hi).  Two 32-bit halves of the finite variants'
// visited_mask (rounds 1-5: the grid controller's two position bytes, which capped the segment store at 255 records).
#define EMP_FLO(s) (reinterpret_cast<int32_t*>(&(s).visited_mask)[0])
#define EMP_FHI(s) (reinterpret_cast<int32_t*>(&(s).visited_mask)[1])
#define EMP_OWED(s) ((s).path_len)  // endless: segments the instance is owed ("lazy initial segments" below)
// endless: the agent's absolute x in pixels, 32 bits (the reference's pygame rects are C ints): the low half of the finite variants'
// path_mask, the high half unused.  Up to 8 x 32,767 columns of 12 px (mg_set_capacity "path_segments"): 3.1 M px.  Rounds 1-6 kept it
// in `ax`, 16 bits, which wrapped after 32,767 px (segment ~341).  `ay` and the fields relative to the camera stay 16-bit.
#define EMP_AX(s) (reinterpret_cast<int32_t*>(&(s).path_mask)[0])
#define EMP_PRE(s) ((s).ex)         // endless: io.aux[i] holds the next episode's first segment (ex / ey: the finite variants' goal)
// The whole record as six 16-byte loads issued together.  Field by field the compiler split it into eleven odd-sized loads
// and issued three of them only after the first uses: a second memory round trip (3-4 us on a cold state array) at the head
// of the one-lane-per-instance step kernel (profiles/r03_emp.md, section 7).
__device__ __forceinline__ MysteryCore load_core(const MysteryCore* p) {
    typedef uint32_t q4 __attribute__((ext_vector_type(4)));
    const q4* src = reinterpret_cast<const q4*>(p);
    union { q4 q[6]; MysteryCore c; } u;
#pragma unroll
    for (int k = 0; k < 6; ++k) u.q[k] = src[k];
    return u.c;
}

struct __attribute__((aligned(16))) MysteryDesc {
    uint8_t valid, sprite, n_tiles, cross_on;
    int16_t sx, sy, cross_x, cross_y;        // top-left of the sprite / of the cross stamp
    uint8_t goal_on, goal_x, goal_y, origin_on, origin_x, origin_y, stamina_on, stamina_red;
    // past-path tiles (endless): bit (col*7 + row) of the 16-column x 7-row window whose column 0 is drawn at tile_x0
    uint64_t tile_mask[2];
    int32_t tile_x0;
    uint8_t bg_on, bg_phase, pad8[2];        // show_background: template = icy columns shifted left by bg_phase pixels
    uint32_t pad[2];
};
static_assert(sizeof(MysteryDesc) == 64, "MysteryDesc must be 64 bytes");

struct MysteryIO {
    MysteryCore* core;
    uint8_t* segs;      // endless: [N][seg_rows][SEG_STRIDE]; node byte = x_rel | y<<3 | rvis<<6 | svis<<7.  finite: [N][PATH_ORDER_STRIDE], see path_order()
    int seg_rows;       // segment records per instance (MAX_SEG by default; mg_set_capacity "path_segments")
    RngSoA rng;
    MysteryDesc* desc;
    int* err;
    int* queue;  // endless: instances waiting for a reset, filled by the step / enqueue kernels, drained by emp_serve_kernel
    uint64_t* walls;  // finite: [N] wall cells of the current path generation (bit x*7+y), read by the debug view only
    int* qctr;   // QC_COUNT entries, QC_HEAD pops beyond the static first round, QC_LEFT workgroups that left emp_serve_kernel
    int* bgq;    // endless, bg_coop: instances that are owed a segment nobody waits for yet (QC_BG_COUNT entries, popped by the service waves)
    uint8_t* bgflag;  // endless, larger launches: [N] 1 = the instance has a background job in this step's raster launch (lane-per-path service)
    uint32_t* aux;  // endless: [N][AUX_WORDS] the next episode's first segment, generated ahead of time (EMP_PRE), and the fall-off list
    const uint4* jump;  // [64][2] PCG64 jump constants {A^(k+1), S_(k+1)} (WaveRng)
    // telemetry of the finite variants' path generation inside the step's launches (bench.py: C3's measured reset share):
    // [0] wave-ticks (real-time clock, 10 ns) spent generating paths, [1] paths generated; mg_debug_counter "path_gen_ticks" / "path_gen_paths"
    // finite: [5] those of [1] that the lane-per-path generator of mass resets made; mg_debug_counter "path_lane_paths"
    // endless: [2] resets a step did itself from a record generated ahead of time (counted by the lab build only), [3] such records generated
    unsigned long long* stats;
    // per-instance option sets (mg_set_option_set / mg_bind_option_sets): instance i runs under sets[set_of[i]]; both NULL while the
    // handle has one set.  Read by the <PS = true> forms of the reset / step / queue-server kernels only.
    const struct MysteryParams* sets;
    const int32_t* set_of;
    MysteryDesc* tdesc;  // finite variants, FINAL forms of the step / raster kernels (terminal observations kept): [N] terminal-frame descriptors
};
// Finite variants: the ORDER of the current path as the reference's list has it -- END first, a byte per node, flat index x*7+y, path_len of them -- written where a
// path is generated (serve_mp, the lane generator's caller) and read by the expert kernel alone (mg_mystery_expert.hpp); the step needs only path_mask.  It lives in
// the pointer the endless variant uses for its segment store: a finite handle has no segments, and MysteryIO -- an argument of every kernel of the family -- stays as it is.
constexpr int PATH_ORDER_STRIDE = 64;
static_assert(G * G <= PATH_ORDER_STRIDE, "a path visits a cell once");
__device__ __forceinline__ uint8_t* path_order(const MysteryIO& io, int i) { return io.segs + (size_t)i * PATH_ORDER_STRIDE; }
constexpr int QC_COUNT = 0, QC_HEAD = 32, QC_LEFT = 64, QC_BG_COUNT = 96, QC_WORDS = 160;  // one 128-byte line each
// MysteryDesc::valid: 0 = leave the frame alone (masked reset), 1 = draw, 2 = the instance has a queue entry, 3 = served (and, in
// the fused launch, drawn by the workgroup that served it).  Only emp_raster_serve_kernel's frame workgroups tell 1 from 2 / 3.
constexpr uint8_t DESC_QUEUED = 2, DESC_SERVED = 3;
// Entries of the endless variant's queue (io.queue): instance | EMP_Q_SEGMENT = "append one segment, then finish the step (which may end in a reset)";
// plain instance = "reset".
constexpr int EMP_Q_SEGMENT = 1 << 30;
constexpr int EMP_Q_OWED = 1 << 29;  // "generate one of the segments this instance is owed" (a background job served like an entry: bg_coop)
constexpr int EMP_Q_INST = EMP_Q_OWED - 1;

__device__ __forceinline__ int floordiv_pos(int a, int b) {
    int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
}  // namespace mg
