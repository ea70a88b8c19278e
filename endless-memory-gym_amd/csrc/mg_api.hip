// mg_api.hip -- the C ABI of include/memgym.h on top of the per-family implementations (mg_family.hpp).  The one translation unit of the ABI: the handle's
// life, its options and the step calls are here, the rest in headers that only this file includes.
//
//   mg_api_env.hpp      struct mg_env (the handle), the error string, guarded() / DeviceGuard, and the heads the entry points share: require_started,
//                       require_geometry, first_call ("the first call allocates and cannot be captured"), record_call
//   mg_api_records.hpp  instance records, frame records, episode sequences, debug-view records; frame_rows_save_kernel
//   mg_api_rollout.hpp  mg_advance / mg_advance_traced / mg_play / mg_play_traced: the loops of their definitions, advance_accumulate_kernel,
//                       play_accumulate_kernel, the readers of mg_advance_out and mg_rollout_trace
//   mg_api_single.hpp   the single-instance fast path (mg_single_open / mg_single_reset / mg_single_step)
//   mg_api_state.hpp    checkpoints, profiling, error words, peer access, mg_debug_counter, mg_debug_rng / mg_debug_set_rng
//   mg_api_windows.hpp  memory windows: mg_episode_positions / mg_window_picks / mg_gather_rows_padded (kernels: mg_windows.hpp)
//   mg_api_targets.hpp  rollout targets: mg_rollout_targets / mg_sum_columns (kernels and arithmetic: mg_targets.hpp)
//
// Here, in this order: make_family / destroy_family; next_flags_kernel; then ONE block with C linkage: copy_rows_kernel and debug_stretch_kernel (their
// symbols have always been the unmangled names), step_call (the body of mg_step and mg_step_masked), and the entry points -- mg_last_error, mg_create /
// mg_destroy, the getters, options and option sets, capacities, the observation format, mg_reset, mg_render, mg_render_debug, mg_step, mg_step_masked,
// mg_step_next, mg_expert_actions, mg_ground_truth64.
#include <algorithm>
#include <mutex>

#include "mg_api_env.hpp"
#include "mg_api_records.hpp"
#include "mg_api_rollout.hpp"
#include "mg_api_single.hpp"
#include "mg_api_state.hpp"
#include "mg_api_targets.hpp"
#include "mg_api_windows.hpp"
#include "mg_expert.hpp"
#include "mg_lab.hpp"

namespace {
mg::Family* make_family(int family, int variant, int n) {
    if (family == 0) return mg::make_mortar(variant, n);
    if (family == 1) return mg::make_spot(variant, n);
    return mg::make_mystery(variant, n);
}
void destroy_family(mg_env* e) {
    if (e->single.host) {  // (the family holds device views of it: mg_destroy synchronises first)
        if (e->vec_dev && e->vec_dev == (float*)(e->single.dev + e->single.o_vec)) e->vec_dev = e->vec_dev_caller;  // never leave a pointer into freed memory
        (void)hipHostFree(e->single.host);
        e->single = mg_env::Single();
    }
    delete e->fam;
    e->fam = nullptr;
}
size_t obs_bytes_of(int f) {
    const size_t elem = f == MG_OBS_F32_CYX ? 4 : ((f == MG_OBS_F16_CYX || f == MG_OBS_BF16_CYX) ? 2 : 1);  // (MG_OBS_U8_XYC, MG_OBS_U8_CYX: one byte)
    return elem * 84 * 84 * 3;
}
}  // namespace

// mg_step_next, composed form, first launch: the mask of the masked step (active = !restart) and a copy of the flags for the masked reset behind it --
// restart may be the caller's done_dev, which the step overwrites: the copy is what makes that legal.
__global__ __launch_bounds__(256) void next_flags_kernel(int n, const uint8_t* __restrict__ restart, uint8_t* __restrict__ active, uint8_t* __restrict__ restart_copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool again = restart[i] != 0;
    active[i] = again ? 0 : 1;
    restart_copy[i] = again ? 1 : 0;
}

extern "C" {

// Rows of the observation buffer whose flag is set, copied to the same rows of another buffer (mg_step with mg_info_buffers.final_obs_dev:
// after a step without auto-reset the rows of the finished instances ARE the terminal observations).  A workgroup looks at 16 flags with one
// load and copies the rows a ballot names, six 16-byte vectors per lane in flight (a uint8 row is 1,323 vectors: one round); rows are whole
// vectors in every output format.
constexpr int COPY_CHUNK = 16;
__global__ __launch_bounds__(256) void copy_rows_kernel(const uint8_t* __restrict__ flags, const row_vec16* __restrict__ src, row_vec16* __restrict__ dst,
                                                      int n, int vec_per_row) {
    const int tid = threadIdx.x;
    for (int base = blockIdx.x * COPY_CHUNK; base < n; base += gridDim.x * COPY_CHUNK) {
        const int e = base + (tid & (COPY_CHUNK - 1));
        uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__ballot(e < n && flags[e] != 0)) & ((1u << COPY_CHUNK) - 1u);
        while (m) {
            const size_t row = (size_t)(base + __builtin_ctz(m)) * (size_t)vec_per_row;
            m &= m - 1;
            for (int q0 = 0; q0 < vec_per_row; q0 += 6 * 256) {
                row_vec16 v[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const int q = q0 + tid + 256 * k;
                    if (q < vec_per_row) v[k] = src[row + q];
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const int q = q0 + tid + 256 * k;
                    if (q < vec_per_row) dst[row + q] = v[k];
                }
            }
        }
    }
}

namespace {
// pygame.transform.scale(surface, (336, 336)) of an 84x84 surface = every pixel four times per axis (transform.c stretch()),
// then fliplr(rot90(array3d, 3)) = image order: out[n][y][x][c] = frame[n][x / 4][y / 4][c]
__global__ __launch_bounds__(256) void debug_stretch_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n) {
    const size_t total = (size_t)n * 336 * 336;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(p % 336), y = (int)((p / 336) % 336);
        const size_t e = p / (336 * 336);
        const uint8_t* src = frames + e * MG_OBS_BYTES + ((size_t)(x >> 2) * 84 + (y >> 2)) * 3;
        uint8_t* dst = out + p * 3;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
    }
}
}  // namespace

// mg_step and mg_step_masked (`who` names the entry point in messages).  active == NULL: every instance steps, in the family's own arrangement.
// active != NULL: the same three branches with the mask handed through to Family::step -- a masked step never takes a family's fused forms, so
// kept terminal observations always go the generic way: inactive instances report done == 0 there, and the copy and the masked reset need nothing new.
static void step_call(mg_env* env, const char* who, const int32_t* actions_dev, const uint8_t* active_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev,
                      float* gt_dev, const mg_info_buffers* info, int autoreset, hipStream_t st) {
    if (!actions_dev || !reward_dev || !done_dev) throw std::runtime_error(std::string(who) + ": NULL buffer");
    const mg::InfoArgs ia = mg::read_info(info);
    if (const char* no = mg::final_frames_refusal(ia, !obs_dev)) throw std::runtime_error(std::string(who) + ": " + no);
    const mg_info_dev& ib = ia.dev;
    mg::Family* f = env->fam;
    if (!obs_dev || ia.final_frames) {  // a headless step: the family's plain arrangement without its raster launch
        // (with final_frames_dev: the RECORDS form of its step kernel keeps the terminal frames' descriptors; a drawn call is that arrangement and the
        // family's dense raster launch behind it -- the plain arrangement, include/memgym.h)
        f->step(actions_dev, active_dev, nullptr, reward_dev, done_dev, gt_dev, &ib, autoreset, st, ia.final_frames);
        if (ia.final_frames) ++env->final_frame_steps;
        if (!obs_dev) ++env->headless_steps;
        else f->raster_only(obs_dev, active_dev, st);
        if (active_dev) ++env->masked_steps;
        if (ib.gt64_dev) f->ground_truth64(ib.gt64_dev, st, active_dev);
        return;
    }
    if (autoreset && ib.final_obs_dev && (active_dev || !(mg::sparse_masked_raster() && f->keeps_final_obs(st)))) {
        // terminal frames wanted: step without auto-reset (obs rows of finished instances = terminal frames), keep
        // a copy of exactly those rows, then reset the finished instances with seed=None -- the same RNG
        // consumption and frames as the fused path (tests/test_gpu_vector_api.py)
        ++env->final_obs_generic_steps;
        f->step(actions_dev, active_dev, obs_dev, reward_dev, done_dev, gt_dev, &ib, 0, st);
        if (mg::sparse_masked_raster()) {  // the rows are there: copied, not drawn again (round 6)
            const int n = env->num_envs, vec_per_row = (int)(mg_obs_bytes(env) / 16);
            mg::launch_checked(copy_rows_kernel, dim3(std::min((n + COPY_CHUNK - 1) / COPY_CHUNK, 16384)), dim3(256), 0, st, done_dev, (const row_vec16*)obs_dev,
                               (row_vec16*)ib.final_obs_dev, n, vec_per_row);
        } else f->raster_only(ib.final_obs_dev, done_dev, st);
        f->reset(nullptr, done_dev, obs_dev, gt_dev, st);
    } else {
        f->step(actions_dev, active_dev, obs_dev, reward_dev, done_dev, gt_dev, &ib, autoreset, st);
    }
    if (active_dev) ++env->masked_steps;
    if (ib.gt64_dev) f->ground_truth64(ib.gt64_dev, st, active_dev);
}

const char* mg_last_error(void) { return mg::g_last_error.c_str(); }

int mg_create(const char* env_id, int32_t num_envs, int device, mg_env** out) {
    try {
        if (!env_id || !out || num_envs < 1) {
            mg::set_error("mg_create: bad arguments");
            return -1;
        }
        DeviceGuard guard(device);
        std::string id(env_id);
        int family = -1, variant = 0;
        if (id == "MortarMayhem-Grid-v0") { family = 0; variant = 0; }
        else if (id == "MortarMayhem-v0") { family = 0; variant = 1; }
        else if (id == "Endless-MortarMayhem-v0") { family = 0; variant = 2; }
        else if (id == "MortarMayhemB-Grid-v0") { family = 0; variant = 3; }
        else if (id == "MortarMayhemB-v0") { family = 0; variant = 4; }
        else if (id == "Endless-SearingSpotlights-v0") { family = 1; variant = 1; }
        else if (id == "SearingSpotlights-v0") { family = 1; variant = 0; }
        else if (id == "MysteryPath-v0") { family = 2; variant = 0; }
        else if (id == "Endless-MysteryPath-v0") { family = 2; variant = 1; }
        else if (id == "MysteryPath-Grid-v0") { family = 2; variant = 2; }
        else {
            mg::set_error("mg_create: environment id not available in this build: " + id);
            return -5;
        }
        mg_env* e = new mg_env();
        e->device = device;
        e->num_envs = num_envs;
        e->id = id;
        e->family = family;
        e->variant = variant;
        static std::mutex serial_mutex;
        static uint64_t serials = 0;
        {
            std::lock_guard<std::mutex> lock(serial_mutex);
            e->serial = ++serials;
        }
        try {
            e->fam = make_family(family, variant, num_envs);
        } catch (...) {
            delete e;
            throw;
        }
        *out = e;
        return 0;
    } catch (const std::exception& e) {
        mg::set_error(e.what());
        return -1;
    }
}

void mg_destroy(mg_env* env) {
    if (!env) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(env->device);
    (void)hipDeviceSynchronize();
    destroy_family(env);
    delete env;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int32_t mg_num_envs(const mg_env* env) { return env ? env->num_envs : 0; }
int32_t mg_action_dim(const mg_env* env) { return env ? env->fam->action_dim() : 0; }
int32_t mg_gt_dim(const mg_env* env) { return env ? env->fam->gt_dim() : 0; }
int32_t mg_vec_dim(const mg_env* env) { return env ? env->fam->vec_dim() : 0; }
int mg_bind_vector_obs(mg_env* env, float* vec_dev) {
    return guarded(env, [&] {
        if (env->fam->vec_dim() == 0 && vec_dev) throw std::runtime_error("mg_bind_vector_obs: this env id has no vector observation");
        env->vec_dev = env->vec_dev_caller = vec_dev;
        env->fam->bind_vector_obs(vec_dev);
    });
}
const char* mg_info_name(const mg_env* env, int k) { return env ? env->fam->info_name(k) : nullptr; }

int mg_set_option(mg_env* env, const char* key, const double* values, int n) {
    return guarded(env, [&] {
        if (!key || !values || n < 1) throw mg::OptionError{-3, "mg_set_option: bad arguments"};
        env->fam->set_option(key, values, n);
    });
}

int mg_set_option_set(mg_env* env, int set_id, const char* key, const double* values, int n) {
    return guarded(env, [&] {
        if (!key || !values || n < 1) throw mg::OptionError{-3, "mg_set_option_set: bad arguments"};
        if (set_id < 0 || set_id >= MG_MAX_OPTION_SETS) throw mg::OptionError{-3, "mg_set_option_set: set index out of range"};
        env->fam->set_option_set(set_id, key, values, n);
    });
}

int mg_bind_option_sets(mg_env* env, const int32_t* set_of_dev) {
    return guarded(env, [&] {
        env->fam->bind_option_sets(set_of_dev);
    });
}

int mg_set_capacity(mg_env* env, const char* what, int64_t value) {
    return guarded(env, [&] {
        if (!what) throw mg::OptionError{-3, "mg_set_capacity: NULL"};
        if (env->started) throw std::runtime_error("mg_set_capacity: before the first mg_reset / mg_set_state");
        env->fam->set_capacity(what, value);
    });
}
int64_t mg_capacity(mg_env* env, const char* what) {
    int64_t v = -1;
    const int rc = guarded(env, [&] {
        if (!what) throw mg::OptionError{-3, "mg_capacity: NULL"};
        v = env->fam->capacity(what);
    });
    return rc == 0 ? v : -1;
}

int mg_set_obs_format(mg_env* env, int format) {
    return guarded(env, [&] {
        if (format != MG_OBS_U8_XYC && format != MG_OBS_F32_CYX && format != MG_OBS_F16_CYX && format != MG_OBS_BF16_CYX && format != MG_OBS_U8_CYX)
            throw mg::OptionError{-3, "mg_set_obs_format: unknown format"};
        env->obs_format = env->fam->obs_format = format;
    });
}

size_t mg_obs_bytes(const mg_env* env) {
    if (!env) return 0;
    return obs_bytes_of(env->obs_format);
}

int mg_reset(mg_env* env, const int64_t* seeds_dev, const uint8_t* mask_dev, void* obs_dev, float* gt_dev, void* stream) {
    return guarded(env, [&] {
        if (!obs_dev) throw std::runtime_error("mg_reset: obs_dev is NULL");
        env->fam->reset(seeds_dev, mask_dev, obs_dev, gt_dev, (hipStream_t)stream);
        env->started = true;
    });
}

int mg_render(mg_env* env, void* obs_dev, void* stream) {
    return guarded(env, [&] {
        if (!obs_dev) throw std::runtime_error("mg_render: obs_dev is NULL");
        env->fam->raster_only(obs_dev, nullptr, (hipStream_t)stream);
    });
}

int mg_render_debug(mg_env* env, uint8_t* rgb_dev, void* stream) {
    return guarded(env, [&] {
        if (!rgb_dev) throw std::runtime_error("mg_render_debug: rgb_dev is NULL");
        hipStream_t st = (hipStream_t)stream;
        uint8_t* frames = nullptr;
        MG_HIP(hipMalloc((void**)&frames, (size_t)env->num_envs * MG_OBS_BYTES));
        try {
            env->fam->sync_state();
            env->fam->raster_debug(frames, st);
            const size_t total = (size_t)env->num_envs * 336 * 336;
            const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 65536);
            mg::launch_checked(debug_stretch_kernel, dim3(grid), dim3(256), 0, st, frames, rgb_dev, env->num_envs);
            MG_HIP(hipStreamSynchronize(st));
        } catch (...) {
            (void)hipFree(frames);
            throw;
        }
        MG_HIP(hipFree(frames));
    });
}

int mg_step(mg_env* env, const int32_t* actions_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
            const mg_info_buffers* info, int autoreset, void* stream) {
    return guarded(env, [&] { step_call(env, "mg_step", actions_dev, nullptr, obs_dev, reward_dev, done_dev, gt_dev, info, autoreset, (hipStream_t)stream); });
}

int mg_step_masked(mg_env* env, const int32_t* actions_dev, const uint8_t* active_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
                   const mg_info_buffers* info, int autoreset, void* stream) {
    return guarded(env, [&] {
        require_started(env, "mg_step_masked: ");
        step_call(env, "mg_step_masked", actions_dev, active_dev, obs_dev, reward_dev, done_dev, gt_dev, info, autoreset, (hipStream_t)stream);
    });
}

int mg_step_next(mg_env* env, const int32_t* actions_dev, const uint8_t* restart_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
                 const mg_info_buffers* info, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_step_next: ";
        require_started(env, who);
        if (!actions_dev || !restart_dev || !obs_dev || !reward_dev || !done_dev)
            throw std::runtime_error(who + "NULL buffer (actions_dev, restart_dev, obs_dev, reward_dev and done_dev are required: mg_reset has no headless form)");
        const mg::InfoArgs ia = mg::read_info(info);
        if (ia.dev.final_obs_dev || ia.final_frames)
            throw std::runtime_error(who + "final_obs_dev / final_frames_dev are set: there are no terminal rows in this mode, the terminal frame is the observation");
        mg::Family* f = env->fam;
        require_geometry(env, who, "before the next step");
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs;
        mg_env::Next& X = env->nxt;
        first_call(X, who, st, [&] {
            X.active.alloc(n);
            X.restart.alloc(n);
        });
        const mg_info_dev& ib = ia.dev;
        if (f->step_next(actions_dev, restart_dev, X.restart.p, obs_dev, reward_dev, done_dev, gt_dev, &ib, st)) {
            ++env->next_fused_steps;
        } else {  // the pair of the definition
            mg::launch_checked(next_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, restart_dev, X.active.p, X.restart.p);
            f->step(actions_dev, X.active.p, obs_dev, reward_dev, done_dev, gt_dev, &ib, 0, st);
            f->reset(nullptr, X.restart.p, obs_dev, gt_dev, st);
        }
        ++env->next_steps;
        if (ib.gt64_dev) f->ground_truth64(ib.gt64_dev, st);
    });
}

int mg_expert_actions(mg_env* env, double eps, uint64_t seed, uint64_t step, int32_t* actions_dev, void* stream) {
    return guarded(env, [&] {
        if (!actions_dev) throw std::runtime_error("mg_expert_actions: actions_dev is NULL");
        require_started(env, "mg_expert_actions: ");
        if (!(eps >= 0.0 && eps <= 1.0)) throw std::runtime_error("mg_expert_actions: eps outside [0, 1]");
        env->fam->expert_actions(mg::ExpertArgs{eps, mg::expert_base(seed, step), actions_dev}, (hipStream_t)stream);
    });
}

int mg_ground_truth64(mg_env* env, double* gt64_dev, void* stream) {
    return guarded(env, [&] {
        if (!env->fam->gt_dim()) return;
        if (!gt64_dev) throw std::runtime_error("mg_ground_truth64: gt64_dev is NULL");
        env->fam->sync_state();
        env->fam->ground_truth64(gt64_dev, (hipStream_t)stream);
    });
}

}  // extern "C"
