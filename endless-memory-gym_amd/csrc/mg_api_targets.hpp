// mg_api_targets.hpp -- the rollout-target calls of include/memgym.h: mg_rollout_targets / mg_sum_columns (kernels, refusals and the arithmetic:
// mg_targets.hpp).  Neither keeps scratch in the handle, so even a handle's first call can be captured.  Included by mg_api.hip alone.
#pragma once
#include "mg_api_env.hpp"
#include "mg_targets.hpp"

namespace {
// mg_rollout_targets' one launch: EXTRA where skip / trunc / final_value are there, COL where the moments are wanted
template <bool EXTRA, bool COL>
void launch_targets(const mg::TargetArrays& A, int steps, int n, float gamma, float gl, hipStream_t st) {
    mg::launch_checked(mg::rollout_targets_kernel<mg::TARGETS_T, EXTRA, COL>, dim3((n + mg::TARGETS_BLOCK - 1) / mg::TARGETS_BLOCK), dim3(mg::TARGETS_BLOCK), 0, st,
                       A, steps, n, gamma, gl);
}
}  // namespace

extern "C" {

int mg_rollout_targets(mg_env* env, const float* reward_dev, const uint8_t* done_dev, const float* value_dev, int32_t steps, const int32_t* steps_of_dev,
                       const uint8_t* skip_dev, const uint8_t* trunc_dev, const float* final_value_dev, float gamma, float lambda, float* adv_dev,
                       float* ret_dev, uint8_t* valid_dev, double* col_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_rollout_targets: ";
        require_started(env, who);
        const mg::TargetArrays A = {reward_dev, done_dev, value_dev, steps_of_dev, skip_dev, trunc_dev, final_value_dev, adv_dev, ret_dev, valid_dev, col_dev};
        if (const char* no = mg::rollout_targets_refusal(A, steps, env->num_envs, gamma, lambda)) throw std::runtime_error(who + no);
        const float gl = gamma * lambda;
        const bool extra = skip_dev || trunc_dev || final_value_dev;
        hipStream_t st = (hipStream_t)stream;
        if (extra) {
            if (col_dev) launch_targets<true, true>(A, steps, env->num_envs, gamma, gl, st);
            else launch_targets<true, false>(A, steps, env->num_envs, gamma, gl, st);
        } else {
            if (col_dev) launch_targets<false, true>(A, steps, env->num_envs, gamma, gl, st);
            else launch_targets<false, false>(A, steps, env->num_envs, gamma, gl, st);
        }
        ++env->rollout_targets;
    });
}

int mg_sum_columns(mg_env* env, const double* col_dev, int32_t rows, double* out_dev, void* stream) {
    return guarded(env, [&] {
        if (const char* no = mg::sum_columns_refusal(col_dev, rows, out_dev)) throw std::runtime_error(std::string("mg_sum_columns: ") + no);
        mg::launch_checked(mg::sum_columns_kernel, dim3((unsigned)rows), dim3(mg::SUM_LANES), 0, (hipStream_t)stream, col_dev, env->num_envs, out_dev);
    });
}

}  // extern "C"
