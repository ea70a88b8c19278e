// mg_spot_expert.hpp -- Searing Spotlights family (included by mg_spot.hip only): the scripted teacher of both ids, oracle/mgo_spot.c sp_expert restated on
// SpotCore -- the (first remaining) coin, then the exit.
#pragma once
#include "mg_expert.hpp"
#include "mg_spot_types.hpp"

namespace mg {
__global__ __launch_bounds__(EXPERT_BLOCK) void spot_expert_kernel(SpotParams P0, SpotIO io, ExpertArgs x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P0.n) return;
    const SpotParams& P = io.set_of ? io.sets[set_index(io.set_of, i)] : P0;
    const SpotCore s = io.core[i];
    // The finite variant's coins: io.coins holds the reference's LIST -- spot_step_body closes the gap of a collected coin by moving the later
    // entries down one place, exactly list.remove(), and a reset writes the coins in the order it places them -- so the oracle's "first remaining
    // coin" is entry 0 whatever was collected before.  (Read unconditionally: behind the tests below it would be a second round trip.)
    const uint32_t c0 = io.coins[(size_t)i * MAX_COINS];
    bool go = true;
    int tx = 0, ty = 0;
    if (P.endless) {
        go = P.coin_enabled != 0;
        tx = s.coin_x;
        ty = s.coin_y;
    } else if (s.num_coins > 0 && s.n_coins > 0) {
        tx = (int)(int16_t)(c0 & 0xFFFFu);
        ty = (int)(c0 >> 16);
    } else if (P.use_exit) {
        tx = s.exit_x;
        ty = s.exit_y;
    } else {
        go = false;
    }
    const int a0 = go ? expert_axis_action(tx - s.ax, P.v_axis_i) : 0, a1 = go ? expert_axis_action(ty - s.ay, P.v_axis_i) : 0;
    expert_store(x, i, false, a0, a1);
}
}  // namespace mg
