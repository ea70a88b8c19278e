// mg_mortar_play.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): mortar_play_kernel, mg_play's K steps of a CALLER-SUPPLIED action tape as ONE
// launch.  A LANE per instance runs the loop of include/memgym.h's definition by itself: the step in its plain two-launch form (mortar_step_body<false, false, PS>)
// with MortarStepArgs::actions pointing at row t of the tape -- lane i reads tape[t][i], coalesced across the wave --, auto-reset by the mode, sums and the count
// of played steps in registers, the traces stored to [t][i].  The step's results travel through the handle's scratch rows exactly as they do between the launches
// of the loop form -- row i is written and read by lane i alone, and a lane that reads what it stored itself is ordered -- so the kernel has no barrier, no atomic
// (but the error word's) and no waiting, and nothing it computes can differ from the loop's.  MG_PLAY_EPISODE: a lane leaves its step loop at its own `done`
// (the wave goes on until its last lane has), then zeroes the rest of its trace column; a lane that is not alive at the start only writes zeros.
// No frame is drawn; the descriptors the last step of each instance leaves are what mg_render draws.
#pragma once
#include "mg_mortar_advance.hpp"
#include "mg_mortar_step.hpp"

namespace mg {
struct MortarPlayArgs {
    int steps;             // 1 .. ADVANCE_MAX_STEPS
    int first, last;       // the call's first launch: alive from the caller's mask, sums and `played` from zero; a later one continues what the launch before it
                           // stored.  Every launch but the last stores the alive bytes for the next
    int episode;           // MG_PLAY_EPISODE
    int row;               // entries per tape row: num_envs x action_dim
    const uint8_t* active; // the caller's mask or NULL (read by the first launch)
    uint8_t* alive;        // [n] scratch: the loop's mask from launch to launch
    float* reward_trace;   // row 0 of this launch, or NULL
    uint8_t* done_trace;
    int32_t* played;       // [n] or NULL
    mg_advance_out out;
};

template <bool PS>
__global__ __launch_bounds__(256) void mortar_play_kernel(MortarStepArgs a, MortarPlayArgs v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const mg_advance_out& o = v.out;
    double reward_sum = 0.0, ep_reward_sum = 0.0, aux_sum[MORTAR_INFO_SLOTS] = {0.0, 0.0};
    int32_t episodes = 0, played = 0;
    int64_t ep_length_sum = 0;
    bool alive;
    if (v.first) alive = v.active ? v.active[i] != 0 : true;
    else {
        alive = v.alive[i] != 0;
        if (v.played) played = v.played[i];
        if (o.reward_sum_dev) reward_sum = o.reward_sum_dev[i];
        if (o.episodes_dev) episodes = o.episodes_dev[i];
        if (o.ep_reward_sum_dev) ep_reward_sum = o.ep_reward_sum_dev[i];
        if (o.ep_length_sum_dev) ep_length_sum = o.ep_length_sum_dev[i];
#pragma unroll
        for (int k = 0; k < MORTAR_INFO_SLOTS; ++k)
            if (o.aux_sum_dev[k]) aux_sum[k] = o.aux_sum_dev[k][i];
    }
    int t = 0;
    if (alive) {
        for (; t < v.steps;) {
            mortar_step_body<false, false, PS>(i, a, 0u, nullptr, 0u, a.actions + (size_t)t * (size_t)v.row);  // (a.actions: row 0 of this launch)
            const size_t at = (size_t)t * (size_t)a.n + (size_t)i;
            const bool d = a.done_out[i] != 0;
            if (v.reward_trace) v.reward_trace[at] = a.reward_out[i];
            if (v.done_trace) v.done_trace[at] = d ? 1 : 0;
            reward_sum += a.info.reward64_dev[i];
            ++played;
            ++t;
            if (d) {
                ++episodes;
                ep_reward_sum += a.info.ep_reward_dev[i];
                ep_length_sum += a.info.ep_length_dev[i];
#pragma unroll
                for (int k = 0; k < MORTAR_INFO_SLOTS; ++k) aux_sum[k] += (double)a.info.aux_dev[k][i];
                if (v.episode) {
                    alive = false;
                    break;
                }
            }
        }
    }
    for (; t < v.steps; ++t) {  // not alive (any more): the zeros the masked step writes for an inactive instance
        const size_t at = (size_t)t * (size_t)a.n + (size_t)i;
        if (v.reward_trace) v.reward_trace[at] = 0.0f;
        if (v.done_trace) v.done_trace[at] = 0;
    }
    if (!v.last) v.alive[i] = alive ? 1 : 0;
    if (v.played) v.played[i] = played;
    if (o.reward_sum_dev) o.reward_sum_dev[i] = reward_sum;
    if (o.episodes_dev) o.episodes_dev[i] = episodes;
    if (o.ep_reward_sum_dev) o.ep_reward_sum_dev[i] = ep_reward_sum;
    if (o.ep_length_sum_dev) o.ep_length_sum_dev[i] = ep_length_sum;
#pragma unroll
    for (int k = 0; k < MORTAR_INFO_SLOTS; ++k)
        if (o.aux_sum_dev[k]) o.aux_sum_dev[k][i] = aux_sum[k];
}
}  // namespace mg
