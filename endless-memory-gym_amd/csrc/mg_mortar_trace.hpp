// mg_mortar_trace.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): mortar_advance_traced_kernel and mortar_play_traced_kernel, the in-launch forms of
// mg_advance_traced / mg_play_traced (include/memgym.h).  Kernels of their own next to mortar_advance_kernel / mortar_play_kernel -- the same lane-per-instance loop,
// no barrier, no atomic (but the error word's), no waiting -- which leave behind, per step t and instance i, what the loop of the definition leaves:
//   actions[t][i]   the action played: the teacher's lane stores it STRAIGHT into the trace row and the step reads it from there (the row is the loop form's A)
//   labels[t][i]    the teacher evaluated a second time at eps 0 in the state before the step (only where the caller asked for labels)
//   reward / done   the step's R / D rows
//   frames[t][i]    the 16-byte MortarDesc the step has just stored to io.desc[i]: the lane re-reads its own row (a lane that reads what it stored itself is
//                   ordered) and stores it as ONE 16-byte vector -- a wave's 64 descriptors are 1 KiB contiguous.  Kept in registers across the step instead, the
//                   descriptor would have to become a result of mortar_step_body, i.e. change the body the existing kernels share.
// Every trace offset is 64-bit: [steps][num_envs] rows of one launch pass 4 GiB at 270,336 instances x 1,024 steps x 16 B.
// MG_PLAY_EPISODE: a lane that has left its step loop, and a lane that never was alive, fills the remaining frames rows with the descriptor it has (the terminal
// one; the one from before the call) and the remaining reward / done rows with zeros -- what mg_save_frames gives after a masked step that left the instance alone.
#pragma once
#include "mg_mortar_advance.hpp"
#include "mg_mortar_play.hpp"

namespace mg {
struct MortarTraceRows {   // row 0 of this launch; any may be NULL
    MortarDesc* frames;    // [steps][n]
    int32_t* actions;      // [steps][n * action_dim]   (advance only)
    int32_t* labels;       // [steps][n * action_dim]   (advance only)
    float* reward;         // [steps][n]                (advance only: play's travel in MortarPlayArgs)
    uint8_t* done;         // [steps][n]
};

template <bool PS>
__global__ __launch_bounds__(256) void mortar_advance_traced_kernel(MortarStepArgs a, MortarAdvanceArgs v, MortarTraceRows tr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const mg_advance_out& o = v.out;
    double reward_sum = 0.0, ep_reward_sum = 0.0, aux_sum[MORTAR_INFO_SLOTS] = {0.0, 0.0};
    int32_t episodes = 0;
    int64_t ep_length_sum = 0;
    if (!v.first) {
        if (o.reward_sum_dev) reward_sum = o.reward_sum_dev[i];
        if (o.episodes_dev) episodes = o.episodes_dev[i];
        if (o.ep_reward_sum_dev) ep_reward_sum = o.ep_reward_sum_dev[i];
        if (o.ep_length_sum_dev) ep_length_sum = o.ep_length_sum_dev[i];
#pragma unroll
        for (int k = 0; k < MORTAR_INFO_SLOTS; ++k)
            if (o.aux_sum_dev[k]) aux_sum[k] = o.aux_sum_dev[k][i];
    }
    const size_t row = (size_t)a.n * (a.P.variant == V_GRID ? 1u : 2u);  // entries per action row (the variant belongs to the env id, not to an option set)
    for (int t = 0; t < v.steps; ++t) {
        const uint64_t base = expert_base(v.seed, v.step0 + (uint64_t)t);
        int32_t* const act = tr.actions ? tr.actions + (size_t)t * row : v.actions;
        mortar_expert_lane(a.P, a.io, ExpertArgs{v.eps, base, act}, i);
        if (tr.labels) mortar_expert_lane(a.P, a.io, ExpertArgs{0.0, base, tr.labels + (size_t)t * row}, i);
        mortar_step_body<false, false, PS>(i, a, 0u, nullptr, 0u, act);
        const size_t at = (size_t)t * (size_t)a.n + (size_t)i;
        const bool d = a.done_out[i] != 0;
        if (tr.reward) tr.reward[at] = a.reward_out[i];
        if (tr.done) tr.done[at] = d ? 1 : 0;
        if (tr.frames) tr.frames[at] = a.io.desc[i];
        reward_sum += a.info.reward64_dev[i];
        if (d) {
            ++episodes;
            ep_reward_sum += a.info.ep_reward_dev[i];
            ep_length_sum += a.info.ep_length_dev[i];
#pragma unroll
            for (int k = 0; k < MORTAR_INFO_SLOTS; ++k) aux_sum[k] += (double)a.info.aux_dev[k][i];
        }
    }
    if (o.reward_sum_dev) o.reward_sum_dev[i] = reward_sum;
    if (o.episodes_dev) o.episodes_dev[i] = episodes;
    if (o.ep_reward_sum_dev) o.ep_reward_sum_dev[i] = ep_reward_sum;
    if (o.ep_length_sum_dev) o.ep_length_sum_dev[i] = ep_length_sum;
#pragma unroll
    for (int k = 0; k < MORTAR_INFO_SLOTS; ++k)
        if (o.aux_sum_dev[k]) o.aux_sum_dev[k][i] = aux_sum[k];
}

// mortar_play_kernel with the frame rows: v.reward_trace / v.done_trace are the trace's reward / done rows
template <bool PS>
__global__ __launch_bounds__(256) void mortar_play_traced_kernel(MortarStepArgs a, MortarPlayArgs v, MortarDesc* frames) {
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
            if (frames) frames[at] = a.io.desc[i];
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
    if (t < v.steps) {  // not alive (any more): the descriptor the instance keeps, and the zeros the masked step writes for an inactive instance
        const MortarDesc kept = a.io.desc[i];
        for (; t < v.steps; ++t) {
            const size_t at = (size_t)t * (size_t)a.n + (size_t)i;
            if (v.reward_trace) v.reward_trace[at] = 0.0f;
            if (v.done_trace) v.done_trace[at] = 0;
            if (frames) frames[at] = kept;
        }
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
