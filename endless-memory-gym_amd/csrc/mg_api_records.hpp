// mg_api_records.hpp -- the record calls of include/memgym.h: instance records (mg_save_instances / mg_load_instances; kernels: mg_instances.hpp), frame
// records (mg_save_frames / mg_draw_frames; mg_frame_records.hpp and the gather forms of the two raster skeletons), episode sequences (mg_split_episodes /
// mg_sequence_picks / mg_draw_frames_padded; mg_sequences.hpp and the PAD forms of the gather rasters) and debug-view records (mg_save_debug_frames /
// mg_draw_debug_frames; the picked *_debug_desc kernels of the three families, mg_debug_stream_out.hpp).  Every call starts with record_call()
// (mg_api_env.hpp).  Included by mg_api.hip alone, in front of mg_api_rollout.hpp: the traced rollouts keep their frames with frame_rows_save_kernel.
#pragma once
#include "mg_api_env.hpp"
#include "mg_frame_records.hpp"
#include "mg_instances.hpp"
#include "mg_sequences.hpp"

// mg_save_frames: record j <- descriptor row of instance idx[j] (idx == NULL: instance j).  A lane moves one 16-byte vector; a descriptor is 1, 4 or 8 of
// them.  An entry < 0 is skipped, one >= num_envs is skipped and flagged (once, by the lane of its first vector); a skipped entry's record is not written.
__global__ __launch_bounds__(256) void frame_rows_save_kernel(const row_vec16* __restrict__ descs, int vec_per_row, const int32_t* __restrict__ idx, int count,
                                                              int num_envs, row_vec16* __restrict__ rec, int* err) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t / vec_per_row;
    if (j >= count) return;
    const int q = (int)(t - j * vec_per_row);
    const int i = idx ? idx[j] : (int)j;
    if (i < 0) return;
    if (i >= num_envs) {
        if (q == 0) __hip_atomic_fetch_or(err, mg::ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    rec[j * vec_per_row + q] = descs[(int64_t)i * vec_per_row + q];
}

namespace {
// `count` entries of idx (NULL: the first `count` instances) -> records at `rec`: mg_save_frames' launch, and a row of a rollout's frame trace
void save_frame_rows(mg_env* env, const int32_t* idx, int count, void* rec, hipStream_t st) {
    const std::pair<const void*, size_t> rows = env->fam->frame_rows();
    const int vec_per_row = (int)(rows.second / 16);
    const int64_t lanes = (int64_t)count * vec_per_row;
    mg::launch_checked(frame_rows_save_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, (const row_vec16*)rows.first, vec_per_row, idx, count,
                       env->num_envs, (row_vec16*)rec, env->fam->error_word());
}

// grid and block of instance_rows_kernel over `count` entries
dim3 instance_grid(const mg::InstanceRows& t, int count) { return dim3((count + mg::INSTANCE_WAVES - 1) / mg::INSTANCE_WAVES, mg::instance_splits(t)); }
const dim3 INSTANCE_BLOCK(64 * mg::INSTANCE_WAVES);
}  // namespace

extern "C" {

// ---- instance records ----
size_t mg_instance_bytes(const mg_env* env) {
    if (!env || !env->fam) return 0;
    try {
        return mg::make_instance_rows(env->fam->instance_rows()).rec_bytes;
    } catch (const std::exception& e) {
        mg::set_error(e.what());
        return 0;
    }
}

uint64_t mg_instance_layout(const mg_env* env) {
    if (!env || !env->fam) return 0;
    return (env->serial << 24) | (env->fam->geometry_generation() & 0xFFFFFFull);
}

int mg_save_instances(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream) {
    return guarded(env, [&] {
        const bool work = record_call(env, "mg_save_instances: ", mg::frame_save_refusal(count, rec_dev), count);
        const mg::InstanceRows t = mg::make_instance_rows(env->fam->instance_rows());
        if (!work) return;
        hipStream_t st = (hipStream_t)stream;
        env->fam->before_instance_save(st);
        mg::launch_checked(mg::instance_rows_kernel<true>, instance_grid(t, count), INSTANCE_BLOCK, 0, st, t, idx_dev, nullptr, nullptr, count, env->num_envs,
                           (char*)rec_dev, env->fam->error_word());
        ++env->instance_saves;
    });
}

int mg_load_instances(mg_env* env, const int32_t* idx_dev, const int32_t* rec_of_dev, int32_t count, const void* rec_dev, void* obs_dev, void* stream) {
    return guarded(env, [&] {
        const bool work = record_call(env, "mg_load_instances: ", mg::frame_save_refusal(count, rec_dev), count);
        const mg::InstanceRows t = mg::make_instance_rows(env->fam->instance_rows());
        if (!work) return;
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs;
        mg_env::Instances& I = env->inst;
        first_call(I, "mg_load_instances: ", st, [&] {
            I.claim.alloc(n);
            I.mask.alloc(n);
        });
        uint8_t* const mask = obs_dev ? I.mask.p : nullptr;
        if (mask) MG_HIP(hipMemsetAsync(mask, 0, (size_t)n, st));
        mg::launch_checked(mg::load_claim_kernel, dim3((count + 255) / 256), dim3(256), 0, st, idx_dev, rec_of_dev, count, n, I.claim.p, mask,
                           env->fam->error_word());
        mg::launch_checked(mg::instance_rows_kernel<false>, instance_grid(t, count), INSTANCE_BLOCK, 0, st, t, idx_dev, rec_of_dev, I.claim.p, count, n,
                           (char*)rec_dev, env->fam->error_word());
        if (mask) env->fam->raster_only(obs_dev, mask, st);  // the masked step's dense launch: the loaded instances' frames, other rows untouched
        ++env->instance_loads;
    });
}

// ---- frame records ----
size_t mg_frame_record_bytes(const mg_env* env) {
    if (!env || !env->fam) return 0;
    return env->fam->frame_rows().second;
}

uint64_t mg_frame_layout(const mg_env* env) {
    if (!env || !env->fam) return 0;
    return mg::frame_layout_value(env->serial, env->fam->geometry_generation(), env->fam->frame_generation());
}

int mg_save_frames(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream) {
    return guarded(env, [&] {
        if (!record_call(env, "mg_save_frames: ", mg::frame_save_refusal(count, rec_dev), count)) return;
        save_frame_rows(env, idx_dev, count, rec_dev, (hipStream_t)stream);
        ++env->frame_saves;
    });
}

int mg_draw_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format, void* obs_dev, void* stream) {
    return guarded(env, [&] {
        if (!record_call(env, "mg_draw_frames: ", mg::frame_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, format, obs_dev), count)) return;
        env->fam->draw_records(rec_dev, (int)n_records, pick_dev, (int)count, format, obs_dev, (hipStream_t)stream);
        ++env->frame_draws;
    });
}

// ---- episode sequences ----
int mg_split_episodes(mg_env* env, const uint8_t* done_dev, int32_t steps, const int32_t* steps_of_dev, const uint8_t* start_dev, int32_t length,
                      mg_sequence* seq_dev, int32_t capacity, int32_t* count_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_split_episodes: ";
        require_started(env, who);
        if (const char* no = mg::split_refusal(done_dev, steps, length, seq_dev, capacity, count_dev, env->num_envs)) throw std::runtime_error(who + no);
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs, blocks = (n + mg::SEQ_BLOCK - 1) / mg::SEQ_BLOCK;
        mg_env::Sequences& Q = env->seq;
        first_call(Q, who, st, [&] {
            Q.first.alloc(n);
            Q.block_sum.alloc(blocks);
        });
        const dim3 block(mg::SEQ_BLOCK);
        mg::launch_checked(mg::seq_count_kernel, dim3(blocks), block, 0, st, done_dev, steps, n, steps_of_dev, length, Q.first.p, Q.block_sum.p);
        mg::launch_checked(mg::seq_scan_kernel, dim3(1), block, 0, st, Q.block_sum.p, blocks, count_dev);
        if (capacity > 0)
            mg::launch_checked(mg::seq_write_kernel, dim3(blocks), block, 0, st, done_dev, steps, n, steps_of_dev, start_dev, length, Q.first.p, Q.block_sum.p,
                               (int4*)seq_dev, capacity);
        ++env->sequence_splits;
    });
}

int mg_sequence_picks(mg_env* env, const mg_sequence* seq_dev, const int32_t* count_dev, int32_t capacity, const int32_t* sel_dev, int32_t m,
                      int32_t length, int32_t* pick_dev, uint8_t* mask_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_sequence_picks: ";
        if (const char* no = mg::picks_refusal(seq_dev, count_dev, capacity, m, length, pick_dev)) throw std::runtime_error(who + no);
        if (m == 0) return;
        const int64_t lanes = (int64_t)m * length;
        mg::launch_checked(mg::seq_picks_kernel, dim3((unsigned)((lanes + mg::SEQ_BLOCK - 1) / mg::SEQ_BLOCK)), dim3(mg::SEQ_BLOCK), 0, (hipStream_t)stream,
                           (const int4*)seq_dev, count_dev, capacity, sel_dev, m, length, env->num_envs, pick_dev, mask_dev, env->fam->error_word());
    });
}

int mg_draw_frames_padded(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format, void* obs_dev,
                          void* stream) {
    return guarded(env, [&] {
        if (!record_call(env, "mg_draw_frames_padded: ", mg::frame_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, format, obs_dev), count)) return;
        env->fam->draw_records_padded(rec_dev, (int)n_records, pick_dev, (int)count, format, obs_dev, (hipStream_t)stream);
        ++env->padded_draws;
    });
}

// ---- debug-view records ----
int mg_save_debug_frames(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream) {
    return guarded(env, [&] {
        const char* also = !idx_dev && count > env->num_envs ? "idx_dev is NULL and count > num_envs" : nullptr;
        if (!record_call(env, "mg_save_debug_frames: ", mg::frame_save_refusal(count, rec_dev), count, also)) return;
        env->fam->save_debug_records(idx_dev, count, rec_dev, (hipStream_t)stream);
        ++env->debug_frame_saves;
    });
}

int mg_draw_debug_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int size, void* rgb_dev, void* stream) {
    return guarded(env, [&] {
        if (!record_call(env, "mg_draw_debug_frames: ", mg::debug_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, size, rgb_dev), count)) return;
        env->fam->draw_debug_records(rec_dev, (int)n_records, pick_dev, (int)count, size, rgb_dev, (hipStream_t)stream);
        ++env->debug_frame_draws;
    });
}

}  // extern "C"
