// mg_api_windows.hpp -- the memory-window calls of include/memgym.h: mg_episode_positions / mg_window_picks / mg_gather_rows_padded (kernels and
// refusals: mg_windows.hpp).  None of them keeps scratch in the handle, so even a handle's first call can be captured.  Included by mg_api.hip alone.
#pragma once
#include <algorithm>

#include "mg_api_env.hpp"
#include "mg_windows.hpp"

namespace {
// mg_gather_rows_padded's one launch with accesses of type V: the PACKED form for rows of few accesses, else the ROW form
template <typename V>
void launch_gather(bool packed, const void* src, int n_rows, int64_t row_bytes, const int32_t* pick, int64_t count, void* dst, int* err, hipStream_t st) {
    const int units = (int)(row_bytes / (int64_t)sizeof(V));
    if (packed) {
        const int64_t blocks = (count * units + mg::WIN_BLOCK - 1) / mg::WIN_BLOCK;
        mg::launch_checked(mg::gather_packed_kernel<V>, dim3((unsigned)std::min<int64_t>(blocks, mg::GATHER_MAX_GRID)), dim3(mg::WIN_BLOCK), 0, st, (const V*)src,
                           n_rows, units, pick, count, (V*)dst, err);
    } else {
        const int64_t per_block = (int64_t)mg::GATHER_WAVES * mg::GATHER_ROWS, blocks = (count + per_block - 1) / per_block;
        mg::launch_checked(mg::gather_rows_kernel<V>, dim3((unsigned)std::min<int64_t>(blocks, mg::GATHER_MAX_GRID)), dim3(mg::WIN_BLOCK), 0, st, (const V*)src,
                           n_rows, units, pick, count, (V*)dst, err);
    }
}
}  // namespace

extern "C" {

int mg_episode_positions(mg_env* env, const uint8_t* done_dev, int32_t steps, const int32_t* steps_of_dev, const int32_t* pos0_dev, int32_t* pos_dev,
                         void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_episode_positions: ";
        require_started(env, who);
        if (const char* no = mg::positions_refusal(done_dev, steps, pos_dev, env->num_envs)) throw std::runtime_error(who + no);
        const int n = env->num_envs;
        mg::launch_checked(mg::episode_positions_kernel, dim3((n + mg::WIN_BLOCK - 1) / mg::WIN_BLOCK), dim3(mg::WIN_BLOCK), 0, (hipStream_t)stream, done_dev,
                           steps, n, steps_of_dev, pos0_dev, pos_dev);
        ++env->episode_positions;
    });
}

int mg_window_picks(mg_env* env, const int32_t* pos_dev, int32_t steps, const int32_t* sel_dev, int32_t m, int32_t window, int32_t lag, int32_t back,
                    int32_t* pick_dev, uint8_t* mask_dev, int32_t* len_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_window_picks: ";
        if (const char* no = mg::window_picks_refusal(pos_dev, steps, sel_dev != nullptr, m, window, lag, back, pick_dev, env->num_envs))
            throw std::runtime_error(who + no);
        ++env->window_picks;
        if (m == 0) return;
        const int64_t lanes = (int64_t)m * window;
        mg::launch_checked(mg::window_picks_kernel, dim3((unsigned)((lanes + mg::WIN_BLOCK - 1) / mg::WIN_BLOCK)), dim3(mg::WIN_BLOCK), 0, (hipStream_t)stream,
                           pos_dev, steps, env->num_envs, sel_dev, m, window, lag, back, pick_dev, mask_dev, len_dev, env->fam->error_word());
    });
}

int mg_gather_rows_padded(mg_env* env, const void* src_dev, int64_t n_rows, int64_t row_bytes, const int32_t* pick_dev, int64_t count, void* dst_dev,
                          void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_gather_rows_padded: ";
        if (const char* no = mg::gather_rows_refusal(src_dev, n_rows, row_bytes, pick_dev != nullptr, count, dst_dev)) throw std::runtime_error(who + no);
        ++env->row_gathers;
        if (count == 0) return;
        hipStream_t st = (hipStream_t)stream;
        int* err = env->fam->error_word();
        const uint32_t width = mg::gather_width(src_dev, dst_dev, row_bytes);
        const bool packed = mg::gather_packed(row_bytes, width);
        const int rows = (int)n_rows;
        switch (width) {
            case 16: launch_gather<mg::gather_vec16>(packed, src_dev, rows, row_bytes, pick_dev, count, dst_dev, err, st); break;
            case 8: launch_gather<mg::gather_vec8>(packed, src_dev, rows, row_bytes, pick_dev, count, dst_dev, err, st); break;
            case 4: launch_gather<uint32_t>(packed, src_dev, rows, row_bytes, pick_dev, count, dst_dev, err, st); break;
            case 2: launch_gather<uint16_t>(packed, src_dev, rows, row_bytes, pick_dev, count, dst_dev, err, st); break;
            default: launch_gather<uint8_t>(packed, src_dev, rows, row_bytes, pick_dev, count, dst_dev, err, st); break;
        }
    });
}

}  // extern "C"
