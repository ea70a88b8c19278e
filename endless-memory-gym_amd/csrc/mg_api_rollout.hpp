// mg_api_rollout.hpp -- the rollout calls of include/memgym.h: mg_advance / mg_advance_traced (K steps under the scripted teacher) and mg_play /
// mg_play_traced (K steps of a caller's tape), headless.  A family that runs the loop inside its own launches takes the call (Family::advance, play and
// their traced forms); otherwise the loop of the definition runs here, one step at a time, with the two accumulate kernels below for the sums.
// Included by mg_api.hip alone, behind mg_api_records.hpp (save_frame_rows).
#pragma once
#include <cstddef>

#include "mg_api_records.hpp"
#include "mg_expert.hpp"

// One step of mg_advance's loop form into the call's sums (the three families share it): row i of the step's reward64 / done / episode
// record, added to -- at the call's first step: stored as -- sum i.  The same additions in the same order as mortar_advance_kernel's.
__global__ __launch_bounds__(256) void advance_accumulate_kernel(int n, int first, mg_info_dev ib, const uint8_t* __restrict__ done, mg_advance_out o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool d = done[i] != 0;
    if (o.reward_sum_dev) o.reward_sum_dev[i] = (first ? 0.0 : o.reward_sum_dev[i]) + ib.reward64_dev[i];
    if (o.episodes_dev) o.episodes_dev[i] = (first ? 0 : o.episodes_dev[i]) + (d ? 1 : 0);
    if (o.ep_reward_sum_dev && (first || d)) o.ep_reward_sum_dev[i] = (first ? 0.0 : o.ep_reward_sum_dev[i]) + (d ? ib.ep_reward_dev[i] : 0.0);
    if (o.ep_length_sum_dev && (first || d)) o.ep_length_sum_dev[i] = (first ? (int64_t)0 : o.ep_length_sum_dev[i]) + (d ? (int64_t)ib.ep_length_dev[i] : (int64_t)0);
#pragma unroll
    for (int k = 0; k < MG_INFO_SLOTS; ++k)
        if (o.aux_sum_dev[k] && ib.aux_dev[k] && (first || d)) o.aux_sum_dev[k][i] = (first ? 0.0 : o.aux_sum_dev[k][i]) + (d ? (double)ib.aux_dev[k][i] : 0.0);
}

// One step of mg_play's loop form: advance_accumulate_kernel's additions in its order (a paused instance's rows are the zeros of the masked step: its sums
// stay 0), then the step counts where the instance was alive, and MG_PLAY_EPISODE: an instance that has just finished is alive no longer.
// (A body of its own, like every kernel form here: DESIGN.md 3.4a.)
__global__ __launch_bounds__(256) void play_accumulate_kernel(int n, int first, int episode, mg_info_dev ib, const uint8_t* __restrict__ done, uint8_t* alive,
                                                              int32_t* played, mg_advance_out o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool d = done[i] != 0;
    if (o.reward_sum_dev) o.reward_sum_dev[i] = (first ? 0.0 : o.reward_sum_dev[i]) + ib.reward64_dev[i];
    if (o.episodes_dev) o.episodes_dev[i] = (first ? 0 : o.episodes_dev[i]) + (d ? 1 : 0);
    if (o.ep_reward_sum_dev && (first || d)) o.ep_reward_sum_dev[i] = (first ? 0.0 : o.ep_reward_sum_dev[i]) + (d ? ib.ep_reward_dev[i] : 0.0);
    if (o.ep_length_sum_dev && (first || d)) o.ep_length_sum_dev[i] = (first ? (int64_t)0 : o.ep_length_sum_dev[i]) + (d ? (int64_t)ib.ep_length_dev[i] : (int64_t)0);
#pragma unroll
    for (int k = 0; k < MG_INFO_SLOTS; ++k)
        if (o.aux_sum_dev[k] && ib.aux_dev[k] && (first || d)) o.aux_sum_dev[k][i] = (first ? 0.0 : o.aux_sum_dev[k][i]) + (d ? (double)ib.aux_dev[k][i] : 0.0);
    const bool a = alive ? alive[i] != 0 : true;
    if (played) played[i] = (first ? 0 : played[i]) + (a ? 1 : 0);
    if (episode && d) alive[i] = 0;  // (episode: alive is the handle's scratch row, never NULL)
}

namespace {
// mg_advance_out as the caller's header laid it out (include/memgym.h): a shorter struct lacks the later slots.  -> the sums, all NULL without `out`
mg_advance_out read_sums(const std::string& who, const mg_advance_out* out) {
    mg_advance_out o;
    memset(&o, 0, sizeof(o));
    if (out) {
        const size_t sz = out->struct_size;
        if (sz < offsetof(mg_advance_out, aux_sum_dev) || sz > sizeof(o) + 16 * sizeof(void*) || sz % sizeof(void*) != 0)
            throw std::runtime_error(who + "mg_advance_out.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h; set it to sizeof(mg_advance_out)");
        memcpy(&o, out, sz < sizeof(o) ? sz : sizeof(o));
    }
    o.struct_size = sizeof(o);
    return o;
}

// mg_rollout_trace as the caller's header laid it out (include/memgym.h), checked like mg_advance_out: -> the rows, all NULL without a trace
mg::TraceRows read_trace(const std::string& who, const mg_rollout_trace* trace, bool teacher) {
    mg_rollout_trace t;
    memset(&t, 0, sizeof(t));
    if (trace) {
        const size_t sz = trace->struct_size;
        if (sz < sizeof(t) || sz > sizeof(t) + 16 * sizeof(void*) || sz % sizeof(void*) != 0)
            throw std::runtime_error(who + "mg_rollout_trace.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h; set it to sizeof(mg_rollout_trace)");
        memcpy(&t, trace, sizeof(t));
    }
    if ((uintptr_t)t.frames_dev & 15u) throw std::runtime_error(who + "mg_rollout_trace.frames_dev is not 16-byte aligned");
    if (!teacher && (t.actions_dev || t.labels_dev))
        throw std::runtime_error(who + "mg_rollout_trace.actions_dev / labels_dev are set: the tape is the caller's and there is no teacher (mg_advance_traced fills them)");
    if (((uintptr_t)t.actions_dev | (uintptr_t)t.labels_dev) & 7u) throw std::runtime_error(who + "mg_rollout_trace.actions_dev / labels_dev are not 8-byte aligned");
    return mg::TraceRows{t.frames_dev, t.actions_dev, t.labels_dev, t.reward_dev, t.done_dev};
}

// row t of a frame trace <- the descriptor rows as they stand: mg_save_frames(env, NULL, num_envs, ...) without its checks and its counter
void save_frame_row(mg_env* env, void* frames, int t, hipStream_t st) {
    const size_t row = (size_t)env->num_envs * env->fam->frame_rows().second;
    save_frame_rows(env, nullptr, env->num_envs, (char*)frames + (size_t)t * row, st);
}

// mg_advance and mg_advance_traced (trace == NULL: the untraced call, launch for launch what it was).  who: "mg_x: "
void advance_call(mg_env* env, const std::string& who, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out,
                  const mg_rollout_trace* trace, void* stream) {
    require_started(env, who);
    if (steps < 1) throw std::runtime_error(who + "steps < 1");
    if (!(eps >= 0.0 && eps <= 1.0)) throw std::runtime_error(who + "eps outside [0, 1]");
    const mg_advance_out o = read_sums(who, out);
    const mg::TraceRows T = read_trace(who, trace, true);
    const bool traced = trace != nullptr;
    if (traced) require_geometry(env, who, "before the next step");
    hipStream_t st = (hipStream_t)stream;
    mg::Family* f = env->fam;
    const int n = env->num_envs;
    mg_env::Rollout& A = env->adv;
    first_call(A, who, st, [&] { A.alloc(f, n, true); });
    float* gt = f->gt_dim() ? gt_dev : nullptr;
    const mg::AdvanceArgs args{steps, eps, seed, step0, A.actions.p, A.reward.p, A.done.p, gt, A.ib, o};
    if (traced ? f->advance_traced(args, T, st) : f->advance(args, st)) {
        env->advance_fused_steps += steps;
        if (traced) env->traced_steps += steps, env->traced_fused_steps += steps;
        return;
    }
    const size_t row = (size_t)n * (size_t)f->action_dim();
    for (int t = 0; t < steps; ++t) {  // the loop of the definition; the trace rows, where given, ARE its A, R and D
        int32_t* a = T.actions ? T.actions + (size_t)t * row : A.actions.p;
        float* r = T.reward ? T.reward + (size_t)t * (size_t)n : A.reward.p;
        uint8_t* d = T.done ? T.done + (size_t)t * (size_t)n : A.done.p;
        const uint64_t base = mg::expert_base(seed, step0 + (uint64_t)t);
        f->expert_actions(mg::ExpertArgs{eps, base, a}, st);
        if (T.labels) f->expert_actions(mg::ExpertArgs{0.0, base, T.labels + (size_t)t * row}, st);
        f->step(a, nullptr, nullptr, r, d, gt, &A.ib, 1, st);
        if (out) mg::launch_checked(advance_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, t == 0 ? 1 : 0, A.ib, d, o);
        if (T.frames) save_frame_row(env, T.frames, t, st);
    }
    env->headless_steps += steps;
    if (traced) env->traced_steps += steps;
}

// mg_play and mg_play_traced (frames_dev: the trace's frame rows; traced: the call came with a trace.  Without one: mg_play, launch for launch what it was)
void play_call(mg_env* env, const std::string& who, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, float* reward_trace_dev,
               uint8_t* done_trace_dev, int32_t* steps_played_dev, float* gt_dev, const mg_advance_out* sums, void* frames_dev, bool traced, void* stream) {
    require_started(env, who);
    if (steps < 1) throw std::runtime_error(who + "steps < 1");
    if (!tape_dev) throw std::runtime_error(who + "tape_dev is NULL");
    if (mode != MG_PLAY_THROUGH && mode != MG_PLAY_EPISODE) throw std::runtime_error(who + "mode is neither MG_PLAY_THROUGH nor MG_PLAY_EPISODE");
    require_geometry(env, who, "before the next step");
    const mg_advance_out o = read_sums(who, sums);
    hipStream_t st = (hipStream_t)stream;
    mg::Family* f = env->fam;
    const int n = env->num_envs;
    mg_env::Rollout& P = env->ply;
    first_call(P, who, st, [&] { P.alloc(f, n, false); });
    const int episode = mode == MG_PLAY_EPISODE ? 1 : 0;
    float* gt = f->gt_dim() ? gt_dev : nullptr;
    const mg::PlayArgs args{steps, episode, tape_dev, active_dev, reward_trace_dev, done_trace_dev, steps_played_dev, P.reward.p, P.done.p, P.alive.p, gt, P.ib, o};
    if (traced ? f->play_traced(args, frames_dev, st) : f->play(args, st)) {
        env->play_fused_steps += steps;
        if (traced) env->traced_steps += steps, env->traced_fused_steps += steps;
        return;
    }
    // the loop of the definition.  The mask of step t: the caller's while it cannot change (MG_PLAY_THROUGH), else the handle's alive row
    const uint8_t* mask = active_dev;
    if (episode) {
        if (active_dev) MG_HIP(hipMemcpyAsync(P.alive.p, active_dev, (size_t)n, hipMemcpyDeviceToDevice, st));
        else MG_HIP(hipMemsetAsync(P.alive.p, 1, (size_t)n, st));
        mask = P.alive.p;
    }
    const size_t row = (size_t)n * (size_t)f->action_dim();
    const bool accumulate = sums || steps_played_dev || episode;
    for (int t = 0; t < steps; ++t) {
        float* r = reward_trace_dev ? reward_trace_dev + (size_t)t * (size_t)n : P.reward.p;
        uint8_t* d = done_trace_dev ? done_trace_dev + (size_t)t * (size_t)n : P.done.p;
        f->step(tape_dev + (size_t)t * row, mask, nullptr, r, d, gt, &P.ib, episode ? 0 : 1, st);
        if (accumulate)
            mg::launch_checked(play_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, t == 0 ? 1 : 0, episode, P.ib, d,
                               episode ? P.alive.p : (uint8_t*)active_dev, steps_played_dev, o);
        if (frames_dev) save_frame_row(env, frames_dev, t, st);  // (an instance the step left alone keeps its descriptor: its row repeats it)
    }
    env->headless_steps += steps;
    if (mask) env->masked_steps += steps;
    if (traced) env->traced_steps += steps;
}
}  // namespace

extern "C" {

int mg_advance(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out, void* stream) {
    return guarded(env, [&] { advance_call(env, "mg_advance: ", steps, eps, seed, step0, gt_dev, out, nullptr, stream); });
}

int mg_advance_traced(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out,
                      const mg_rollout_trace* trace, void* stream) {
    return guarded(env, [&] { advance_call(env, "mg_advance_traced: ", steps, eps, seed, step0, gt_dev, out, trace, stream); });
}

int mg_play(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, float* reward_trace_dev, uint8_t* done_trace_dev,
            int32_t* steps_played_dev, float* gt_dev, const mg_advance_out* sums, void* stream) {
    return guarded(env, [&] {
        play_call(env, "mg_play: ", tape_dev, steps, mode, active_dev, reward_trace_dev, done_trace_dev, steps_played_dev, gt_dev, sums, nullptr, false, stream);
    });
}

int mg_play_traced(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, int32_t* steps_played_dev, float* gt_dev,
                   const mg_advance_out* sums, const mg_rollout_trace* trace, void* stream) {
    return guarded(env, [&] {
        const mg::TraceRows T = read_trace("mg_play_traced: ", trace, false);
        play_call(env, "mg_play_traced: ", tape_dev, steps, mode, active_dev, T.reward, T.done, steps_played_dev, gt_dev, sums, T.frames, trace != nullptr, stream);
    });
}

}  // extern "C"
