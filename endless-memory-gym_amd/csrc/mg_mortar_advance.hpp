// mg_mortar_advance.hpp -- Mortar Mayhem family (included by mg_mortar.hip only): mortar_advance_kernel, mg_advance's K steps under the scripted teacher as ONE
// launch.  A LANE per instance runs the loop of include/memgym.h's definition by itself: the teacher's action (mortar_expert_lane, the hash draw of step0 + t),
// the step with auto-reset in its plain two-launch form (mortar_step_body<false, false, PS>), the sums in registers.  The action and the step's results travel
// through the handle's scratch arrays exactly as they do between the launches of the loop form -- row i is written and read by lane i alone, and a lane that
// reads what it stored itself is ordered -- so the kernel has no barrier, no atomic (but the error word's) and no waiting, and nothing it computes can differ
// from the loop's.  No frame is drawn; the descriptors the last step leaves are what mg_render draws.
#pragma once
#include "mg_mortar_expert.hpp"
#include "mg_mortar_step.hpp"

namespace mg {
constexpr int ADVANCE_MAX_STEPS = 1024;  // per launch: the host splits a longer call, so that no single kernel runs long
constexpr int MORTAR_INFO_SLOTS = 2;     // the aux slots the family names (MortarFamily::info_name)

struct MortarAdvanceArgs {
    int steps;           // 1 .. ADVANCE_MAX_STEPS
    int first;           // the call's first launch: the sums start from zero; a later one continues what the launch before it stored
    double eps;
    uint64_t seed, step0;  // this launch's first step number
    int32_t* actions;    // == MortarStepArgs::actions, writable
    mg_advance_out out;
};

template <bool PS>
__global__ __launch_bounds__(256) void mortar_advance_kernel(MortarStepArgs a, MortarAdvanceArgs v) {
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
    for (int t = 0; t < v.steps; ++t) {
        mortar_expert_lane(a.P, a.io, ExpertArgs{v.eps, expert_base(v.seed, v.step0 + (uint64_t)t), v.actions}, i);
        mortar_step_body<false, false, PS>(i, a, 0u);
        reward_sum += a.info.reward64_dev[i];
        if (a.done_out[i]) {
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
}  // namespace mg
