// mg_mortar_types.hpp -- Mortar Mayhem family (included by mg_mortar.hip only, which says which mg_mortar_*.hpp holds what): the variant constants and the records its
// launches share -- MortarParams, the 64-byte MortarState, the 16-byte frame descriptor MortarDesc, MortarIO and MortarStepArgs.  Every other mg_mortar_*.hpp includes this one.
#pragma once
#include "mg_family.hpp"
#include "mg_mortar_handover.hpp"
#include "mg_raster_v1.hpp"

namespace mg {
using namespace v1;  // raster generation 1 (see mg_raster_v1.hpp)
enum { V_GRID = 0, V_FREE = 1, V_ENDLESS = 2 };

struct MortarParams {
    int variant, N, allowed, visual_feedback, max_steps, initial_count;
    int taskb;                   // MortarMayhemB*: no display phase, spawn offset for the free controller, vector obs
    int cmd_cap;                 // per-instance command list capacity
    int arena_x0, tile;          // arena top-left (x == y) and tile size in px
    int radius, sprite_dim;      // agent radius, sprite box
    int glyph_x0;                // blit position of the command glyph (x == y)
    int v_axis_i, v_diag_i;      // free controller: int(speed), int(speed/sqrt2)
    int off_lo, off_hi;          // endless: spawn offset = integers(off_lo, off_hi)
    double v_axis, v_diag;       // screen-wrap controller: un-truncated velocities
    OptList command_count, show_dur, show_delay, expl_dur, expl_delay;
    double r_fail, r_succ, r_ep_succ, r_new;
};

// 64-byte per-instance record
struct __attribute__((aligned(16))) MortarState {
    int16_t ax, ay;          // agent rect centre
    int16_t disp_x, disp_y;  // centre of the rect the frame shows (differs from ax/ay only through the Endless stale-sprite quirk)
    uint8_t rot8 : 3;        // agent.rotation / 45
    uint8_t disp_is_agent : 1;  // rotated_agent_rect is the live agent's rect
    uint8_t tiles_on : 1;
    uint8_t disp_sprite;     // sprite index the frame shows, 0xFF = none yet
    int8_t tx, ty;           // target tile
    int8_t nx, ny;           // normalized agent position
    uint16_t num_cmds, cur_cmd;
    uint16_t vis_pos, vis_len, vis_base;  // display schedule: next entry, length, first command it covers
    uint16_t cmd_steps, verify_step;
    // this episode's draws from the "sample one per episode" lists: 16 bits each (round 5; bytes before -- the reference takes
    // any int, mortar_mayhem_grid.py:253-254,268-269); the host refuses only what overflows the 16-bit display schedule
    uint16_t show_dur, show_delay, expl_dur, expl_delay;
    uint8_t gx, gy;          // grid controller position
    int32_t ep_len, t, total_completed;
    uint32_t dbg_pops;       // debug view only: entries popped from the reference's CLONE of the display schedule (one per debug
                             // render while the real schedule holds entries; copied anew at reset and at an endless regeneration,
                             // mortar_mayhem_grid.py:122,257, endless_mortar_mayhem.py:321)
    double ep_sum;
};
static_assert(sizeof(MortarState) == 64, "MortarState must be 64 bytes");

// per-instance frame descriptor: what the raster kernel composes (template -> agent sprite -> command glyph)
struct __attribute__((aligned(16))) MortarDesc {
    int16_t sx, sy;    // sprite top-left on screen
    uint16_t tmpl;     // background template index, 0xFFFF = leave the frame untouched (masked reset)
    uint8_t sprite;    // 0..7, 0xFF none
    uint8_t glyph;     // 0..9 (9 = blank), 0xFF none
    int16_t glyph_x0;  // blit position of the glyph (x == y)
    int16_t ring_x, ring_y;  // debug view only: top-left of the target ring stamp
    uint8_t ring_on;
    uint8_t reserved;  // (0; the one-launch step's epoch until that step got a hand-over word of its own, mg_mortar_handover.hpp)
};
static_assert(sizeof(MortarDesc) == 16, "MortarDesc must be 16 bytes");
constexpr int STAMP_SPRITE0 = 0, STAMP_GLYPH0 = 8, STAMP_RING = 18;

struct MortarIO {
    MortarState* state;
    uint8_t* cmds;
    RngSoA rng;
    MortarDesc* desc;
    float* vec;  // [N][180] caller buffer bound with mg_bind_vector_obs (MortarMayhemB*), or NULL
    int* err;    // sticky error bits (mg_poll_errors / mg_peek_errors)
    // per-instance option sets (mg_set_option_set / mg_bind_option_sets): instance i runs under sets[set_of[i]]; both NULL while
    // the handle has ONE set -- the kernels then take the parameters from their arguments (scalar registers) as ever
    const MortarParams* sets;
    const int32_t* set_of;
};
constexpr int ERR_CMD_OVERFLOW = 32;  // include/memgym.h: Endless Mortar Mayhem command list longer than its capacity

// What a step needs besides the instance index: ONE struct, so that it is the head of the kernel-argument segment of both
// step kernels (mortar_step_raster_kernel reads it a second time through the segment pointer, see there).
struct MortarStepArgs {
    MortarParams P;
    int n;
    MortarIO io;
    const int32_t* actions;
    float* reward_out;
    uint8_t* done_out;
    float* gt;
    mg_info_dev info;
    int autoreset;
    uint64_t* handover;  // one-launch step: [N] hand-over words (mg_mortar_handover.hpp), step lane -> frame workgroup of the same launch
    uint64_t* tdesc;     // FINAL form of the one-launch step (terminal observations kept): [N] words of the terminal frames (same layout, epoch 0)
};
// Largest arena the host accepts (arena_size, Endless: 6): template indices are 1 + tx * N + ty <= N * N, far inside the hand-over word's 15 bits
constexpr int MORTAR_MAX_N = 6;
static_assert(MORTAR_MAX_N * MORTAR_MAX_N <= (int)HANDOVER_TMPL_MAX, "a template index the host accepts does not fit the hand-over word");
}  // namespace mg
