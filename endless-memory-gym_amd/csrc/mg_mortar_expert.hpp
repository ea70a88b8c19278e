// mg_mortar_expert.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): the scripted teacher of all five ids, oracle/mgo_mortar.c mm_expert restated on
// MortarState -- wait while commands are shown and while the tiles are on, else move to the target tile.  mortar_expert_lane is the teacher of ONE instance:
// mortar_expert_kernel (mg_expert_actions) and mortar_advance_kernel (mg_advance, mg_mortar_advance.hpp) both call it.
#pragma once
#include "mg_expert.hpp"
#include "mg_mortar_types.hpp"

namespace mg {
__device__ __forceinline__ void mortar_expert_lane(const MortarParams& P0, const MortarIO& io, const ExpertArgs& x, int i) {
    const MortarParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    const MortarState s = io.state[i];
    const bool grid = P.variant == V_GRID;
    int a0 = 0, a1 = 0;
    // (MortarMayhemB*: no display phase -- vis_len is 0 from the reset on)
    const bool wait = s.vis_pos < s.vis_len || s.tiles_on;
    if (!wait && grid) {
        if (!(s.gx == s.tx && s.gy == s.ty)) a0 = expert_grid_action(s.rot8 * 45, expert_grid_facing(s.tx - s.gx, s.ty - s.gy));
    } else if (!wait) {
        int dx = P.arena_x0 + P.tile * s.tx + P.tile / 2 - s.ax, dy = P.arena_x0 + P.tile * s.ty + P.tile / 2 - s.ay;
        if (P.variant == V_ENDLESS) {  // the arena wraps: the shorter way round
            const int w = SCREEN, h = SCREEN / 2;
            dx = ((dx + h) % w + w) % w - h;
            dy = ((dy + h) % w + w) % w - h;
        }
        a0 = expert_axis_action(dx, P.v_axis_i);
        a1 = expert_axis_action(dy, P.v_axis_i);
    }
    expert_store(x, i, grid, a0, a1);
}

__global__ __launch_bounds__(EXPERT_BLOCK) void mortar_expert_kernel(MortarParams P0, int n, MortarIO io, ExpertArgs x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mortar_expert_lane(P0, io, x, i);
}
}  // namespace mg
