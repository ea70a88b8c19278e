// mg_spot_types.hpp -- Searing Spotlights family (included by mg_spot.hip only, which says which mg_spot_*.hpp holds what): the constants and the records its launches
// share -- SpotParams, SpotCore, the one-line frame descriptor SpotDesc with its word view (SpotView), the sticky bits of SpotCore::pad, SpotIO, the reset queue's
// counters and descriptor tags, and the argument structs of the step and of the fused raster / reset launch.  Every other mg_spot_*.hpp includes this one.
#pragma once
#include "mg_family.hpp"
#include "mg_raster.hpp"

namespace mg {
constexpr int SLOTS = 16;
constexpr int MAX_COINS = 8;
constexpr int MAX_HOLES = 16;  // = SLOTS: a frame shows at most one disc per slot
constexpr int LAYER_COIN_ABOVE = 1, LAYER_EXIT_ABOVE = 2, LAYER_AGENT_TOP = 4;  // SpotDesc::coin_above: what is drawn over the dark layer

struct SpotParams {
    int endless, n;
    int max_steps, steps_per_coin, initial_spawns, spawn_interval, interval0, num_spawns;
    int visual_feedback, dim_duration, dim_step, light_threshold;
    int black_background, hide_chessboard;  // repaint the instance's background surfaces for good (see BG_MODE_SHIFT)
    int ordered_holes;              // a spotlight with a border has been possible: hole words in LIST order, border composer
    int layer_flags;                // LAYER_EXIT_ABOVE (exit_visible) | LAYER_AGENT_TOP (agent_visible), OR-ed into SpotDesc::coin_above
    int coin_enabled, coin_show_duration, coins_visible, sample_agent_position, show_last_action, show_last_positive_reward;
    int use_exit;                   // finite variant; 0: no exit is spawned, the instance's EARLIER exit stays in the frame (spot_reset)
    int r_lo, r_hi;                 // radius = integers(r_lo, r_hi)
    int agent_radius, sprite_half, coin_radius;
    int v_axis_i, v_diag_i;
    int spawn_clamp;                // _process_spawn_pos offset
    int bar_x, bar_w, quarter, bar_h;
    // finite variant: the Exit stamps the handle holds, one pair (closed, open) per GENERATION = distinct exit_scale still on
    // some instance's screen (a stale exit keeps the size it was made with: exit_gen_of); exit_gen = the one new exits get,
    // exit_halves = (int(20 * exit_scale) >> 1) of each generation, a byte each
    int exit_gen;
    uint64_t exit_halves;
    double speed_lo, speed_hi, damage, agent_health, exit_radius, half_diag;
    double r_inside, r_outside, r_death, r_coin, r_exit;
    OptList num_coins;
    const double* cos_tab;          // [360] integer degrees, exact for multiples of 90
    const double* sin_tab;
    const uint4* jump;              // [16][2] PCG64 jump constants {A^(k+1), S_(k+1)} (new_spots_at_reset)
    int lab_fallback;               // lab build (MEMGYM_SPOT_RESET_FALLBACK=k): every k-th instance takes new_spots_at_reset's fall-back, as after a rejected draw (tests)
};

struct __attribute__((aligned(16))) SpotCore {
    int16_t ax, ay;
    uint8_t rot8, alpha, la0, la1;
    uint8_t red_w, n_spots, exit_open, n_coins;
    uint8_t n_intervals, last_pos, bg_red, has_coin;
    int32_t spawn_timer, t, coin_t, coins_collected;
    int16_t coin_x, coin_y, exit_x, exit_y;
    int32_t num_coins, ep_len;
    double health, ep_sum;
    uint64_t order;  // spotlight list: nibble k = slot of the k-th element
    // pad: debug view, bit 31 = a sprite has been shown, 18..16 sprite, 15..8 y + 128, 7..0 x + 128;
    //      bits 21..20 / 23..22 = what the blue / red background surface of this instance looks like (BG_CHESS / WHITE / BLACK)
    uint32_t free_mask, pad;
};
static_assert(sizeof(SpotCore) == 80, "SpotCore must be 80 bytes");

// The frame descriptor: 32 dwords = ONE 128-byte line (round 4; it was 160 bytes over two or three lines).
//   w0  valid | bg << 8 | sprite << 16 | alpha << 24          w1  sx | sy << 16 (int16 each)
//   w2  n_holes | n_coins << 8 | coin_above << 16 | red_w << 24
//   w3  c_base | c_act0 << 8 | c_act1 << 16 | c_bar << 24      w4  bar_x | bar_w << 8 | quarter << 16 | exit_stamp << 24
//   w5  exit_x | exit_y << 16                                  w6, w7  unused
//   w8 .. w15  coins: (x + 128) | (y + 128) << 16, top-left of the coin stamp        w16 .. w31 holes
// The composers address it by WORD through scalar loads (SpotView over a pointer in the constant address space).
struct __attribute__((aligned(128))) SpotDesc {
    uint32_t valid : 8, bg : 8, sprite : 8, alpha : 8;
    int32_t sx : 16, sy : 16;
    uint32_t n_holes : 8, n_coins : 8, coin_above : 8, red_w : 8;
    uint32_t c_base : 8, c_act0 : 8, c_act1 : 8, c_bar : 8;
    uint32_t bar_x : 8, bar_w : 8, quarter : 8, exit_stamp : 8;
    int32_t exit_x : 16, exit_y : 16;
    uint32_t pad[2];
    uint32_t coins[MAX_COINS];
    uint32_t holes[MAX_HOLES];
};
static_assert(sizeof(SpotDesc) == 128 && MAX_HOLES == 16 && MAX_COINS == 8, "SpotDesc is one 128-byte line");
constexpr int DW_COINS = 8, DW_HOLES = 16;

struct DescWordsMem {  // the descriptor in memory, written by an EARLIER launch: scalar loads
    cptr<uint32_t> p;
    __device__ __forceinline__ uint32_t w(int k) const { return p[k]; }
};
template <class W>
struct SpotView {
    W s;
    __device__ __forceinline__ uint32_t valid() const { return s.w(0) & 0xFFu; }
    __device__ __forceinline__ uint32_t bg() const { return (s.w(0) >> 8) & 0xFFu; }
    __device__ __forceinline__ uint32_t sprite() const { return (s.w(0) >> 16) & 0xFFu; }
    __device__ __forceinline__ uint32_t alpha() const { return s.w(0) >> 24; }
    __device__ __forceinline__ int sx() const { return (int)(int16_t)(s.w(1) & 0xFFFFu); }
    __device__ __forceinline__ int sy() const { return (int)s.w(1) >> 16; }
    __device__ __forceinline__ int n_holes() const { return (int)(s.w(2) & 0xFFu); }
    __device__ __forceinline__ int n_coins() const { return (int)((s.w(2) >> 8) & 0xFFu); }
    __device__ __forceinline__ uint32_t coin_above() const { return (s.w(2) >> 16) & 0xFFu; }
    __device__ __forceinline__ int red_w() const { return (int)(s.w(2) >> 24); }
    __device__ __forceinline__ uint32_t c_base() const { return s.w(3) & 0xFFu; }
    __device__ __forceinline__ uint32_t c_act0() const { return (s.w(3) >> 8) & 0xFFu; }
    __device__ __forceinline__ uint32_t c_act1() const { return (s.w(3) >> 16) & 0xFFu; }
    __device__ __forceinline__ uint32_t c_bar() const { return s.w(3) >> 24; }
    __device__ __forceinline__ int bar_x() const { return (int)(s.w(4) & 0xFFu); }
    __device__ __forceinline__ int bar_w() const { return (int)((s.w(4) >> 8) & 0xFFu); }
    __device__ __forceinline__ int quarter() const { return (int)((s.w(4) >> 16) & 0xFFu); }
    __device__ __forceinline__ uint32_t exit_stamp() const { return s.w(4) >> 24; }
    __device__ __forceinline__ int exit_x() const { return (int)(int16_t)(s.w(5) & 0xFFFFu); }
    __device__ __forceinline__ int exit_y() const { return (int)s.w(5) >> 16; }
    __device__ __forceinline__ int coin_x(int k) const { return (int)(s.w(DW_COINS + k) & 0xFFFFu) - 128; }
    __device__ __forceinline__ int coin_y(int k) const { return (int)(s.w(DW_COINS + k) >> 16) - 128; }
    __device__ __forceinline__ uint32_t hole(int h) const { return s.w(DW_HOLES + h); }
};
typedef SpotView<DescWordsMem> SpotViewMem;
__device__ __forceinline__ SpotViewMem view_of(cptr<SpotDesc> dp) { return SpotViewMem{DescWordsMem{(cptr<uint32_t>)dp}}; }

constexpr int ST_COIN = 8, ST_EXIT0 = 9;  // exit of generation g: closed ST_EXIT0 + 2 g, open ST_EXIT0 + 2 g + 1
constexpr int EXIT_GENS = 8;
// hide_chessboard / black_background paint over the two background surfaces an environment object keeps for its lifetime
// (searing_spotlights.py:349-351, 234-235, 420-421; endless :313-315, 223-224, 376-377): per instance, sticky across
// episodes and option changes.  Templates: 0 blue board, 1 red board, 2 white, 3 black.
constexpr uint32_t BG_CHESS = 0, BG_WHITE = 1, BG_BLACK = 2, BG_MODE_SHIFT = 20, BG_MODE_MASK = 0xFu << BG_MODE_SHIFT;
// SpotCore::pad bit 24: the instance has had an exit (searing_spotlights.py: self.exit exists); sticky like the board modes
// bits 27..25: the generation of that exit (SpotParams::exit_gen when it was spawned) -- self.exit is an object of its own in the
// reference: with use_exit = False it stays on screen as it was made, also once exit_scale has changed (searing_spotlights.py:431-435)
constexpr uint32_t PAD_HAS_EXIT = 1u << 24, PAD_EXIT_GEN_SHIFT = 25, PAD_EXIT_GEN_MASK = (uint32_t)(EXIT_GENS - 1) << PAD_EXIT_GEN_SHIFT;
constexpr uint32_t PAD_STICKY = BG_MODE_MASK | PAD_HAS_EXIT | PAD_EXIT_GEN_MASK;
__device__ __forceinline__ int exit_gen_of(uint32_t pad) { return (int)((pad & PAD_EXIT_GEN_MASK) >> PAD_EXIT_GEN_SHIFT); }
constexpr int ERR_NO_EXIT = 256;  // include/memgym.h: use_exit = False for an instance that never had an exit
__device__ __forceinline__ uint32_t bg_mode(uint32_t pad, int red) { return (pad >> (BG_MODE_SHIFT + 2 * red)) & 3u; }
__device__ __forceinline__ uint32_t bg_set(uint32_t pad, int red, uint32_t m) {
    return (pad & ~(3u << (BG_MODE_SHIFT + 2 * red))) | (m << (BG_MODE_SHIFT + 2 * red));
}
__device__ __forceinline__ uint8_t bg_template(uint32_t pad, int red) {
    const uint32_t m = bg_mode(pad, red);
    return (uint8_t)(m == BG_CHESS ? (uint32_t)red : 1u + m);
}
constexpr int BAR_H = 4;  // top bar height: int(16 * SCALE)

struct SpotIO {
    SpotCore* core;
    // A spotlight's slot record, [N][16] each: where it is on its way (t, f64), how fast (f64), its three angles in degrees (u32:
    // start | target << 9 | offset << 18, each already % 360) and its radius (u8, bit 7: has_border).  The six end points of
    // Spotlight.__init__ are c + cos/sin(angle) * (half_diag + radius): the same expression gives the same doubles at every step, so
    // they are recomputed from the (cache-resident) trig tables instead of stored -- round 3 kept them (six f64 arrays): 1,312 B of
    // slot state per instance, read by a step kernel that is a burst of cold loads (profiles/r04_spot_step.md); now 336 B.
    // `done` is t == 1.0 (the step clamps t to exactly 1.0 when it raises it, and nothing else writes either).
    double *sp_t, *sp_speed;
    uint32_t* sp_ang;
    uint8_t* sp_r;
    uint32_t* coins;  // [N][MAX_COINS] (x | y<<16), finite variant
    RngSoA rng;
    SpotDesc* desc;
    int* err;
    // resets put off by the step kernel and served inside the raster launch (spot_raster_serve_kernel)
    int* queue;  // [N] instances
    int* qctr;   // SQ_COUNT entries, SQ_LEFT service workgroups that have finished (the last one clears both)
    // per-instance option sets (mg_set_option_set / mg_bind_option_sets): instance i runs under sets[set_of[i]]; both NULL while
    // the handle has ONE set -- the kernels then take the parameters from their arguments
    const SpotParams* sets;
    const int32_t* set_of;
};
constexpr int SQ_COUNT = 0, SQ_LEFT = 32, SQ_WORDS = 64;  // one 128-byte line each
// SpotDesc::valid: 0 = leave the frame alone (masked reset), 1 = draw, 2 = a reset is queued, 3 = reset and drawn by a service
// workgroup.  The frame workgroups of the fused launch draw 1 only, everything else (raster_only, debug view) draws != 0.
constexpr uint32_t DESC_QUEUED = 2, DESC_SERVED = 3;

// What a step needs besides the instance: ONE struct, the head of the kernel-argument segment of both step kernels.
struct SpotStepArgs {
    SpotParams P;
    SpotIO io;
    const int32_t* actions;
    float* reward_out;
    uint8_t* done_out;
    float* gt;
    mg_info_dev info;
    int autoreset, defer;
};

// all arguments in one struct = the kernel-argument segment: the service workgroups read theirs through a pointer the compiler cannot
// see through, where they are used (held in scalar registers for the length of the service loop they spilled into vector lanes)
struct SpotServeArgs {
    const SpotDesc* descs;
    RasterAtlas A;
    void* obs;
    int n;
    SpotParams P;
    SpotIO io;
    float* gt;
    // Resets a serving workgroup takes per round: as few as serve every queued instance in ONE round (the launch is as long as a
    // reset plus the frames its workgroup draws behind it: 4,096 instances 74 -> 117 M env-steps/s with one instead of eight),
    // within [batch_min, batch_max] (host: 1 .. 8 up to 12,288 instances -- a step in which every instance is truncated at once
    // still takes few rounds -- and 8 beyond, where eight measured 1-2 % ahead of the adaptive choice).  profiles/r04_spot_step.md section 4.
    int batch_min, batch_max;
    void* final_obs;  // FINAL form (terminal observations kept, mg_info_buffers.final_obs_dev), else NULL
};
}  // namespace mg
