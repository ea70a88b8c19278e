// mg_api.hip -- the C ABI of include/memgym.h on top of the per-family implementations.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <map>
#include <mutex>

#include "mg_expert.hpp"
#include "mg_family.hpp"
#include "mg_frame_records.hpp"
#include "mg_instances.hpp"
#include "mg_lab.hpp"
#include "mg_sequences.hpp"

namespace mg {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
}  // namespace mg

// One handle = one device, num_envs instances, one Family object (state, atlases, queues); everything runs on the caller's stream.
// (Rounds 3-5 could split a handle into "instance groups" on streams of their own -- mg_set_groups; measured x0.8 on ROCm 7.2,
// profiles/r03_groups.md -- removed in round 6: dead weight in the ABI, the checkpoint header and this file.)
struct mg_env {
    mg::Family* fam = nullptr;
    int device = 0;
    int num_envs = 0;
    int variant = 0, family = 0;  // what make_* was called with
    bool started = false;         // a reset has happened
    int64_t final_obs_generic_steps = 0;  // mg_debug_counter: mg_step calls that kept terminal observations on the generic path (see mg_step)
    int64_t masked_steps = 0;          // mg_debug_counter: mg_step_masked calls with active_dev != NULL
    int64_t headless_steps = 0;        // mg_debug_counter: mg_step calls with obs_dev == NULL, and the steps of mg_advance's loop form
    int64_t final_frame_steps = 0;     // mg_debug_counter: mg_step / mg_step_masked calls with mg_info_buffers.final_frames_dev
    int64_t advance_fused_steps = 0;   // mg_debug_counter: steps mg_advance took inside a family's own launches (Family::advance)
    // mg_advance: what the loop of its definition passes from launch to launch, allocated at the handle's first call (include/memgym.h)
    struct Advance {
        bool ready = false;
        mg::DevArray<int32_t> actions, ep_length;
        mg::DevArray<float> reward, aux[MG_INFO_SLOTS];
        mg::DevArray<uint8_t> done;
        mg::DevArray<double> reward64, ep_reward;
        mg_info_dev ib;
    } adv;
    int64_t play_fused_steps = 0;      // mg_debug_counter: steps mg_play took inside a family's own launches (Family::play)
    int64_t traced_steps = 0, traced_fused_steps = 0;  // mg_debug_counter: steps of mg_advance_traced / mg_play_traced calls with a trace; those taken in-launch
    // mg_play: what the loop of its definition passes from launch to launch, allocated at the handle's first call (include/memgym.h)
    struct Play {
        bool ready = false;
        mg::DevArray<uint8_t> alive, done;
        mg::DevArray<int32_t> ep_length;
        mg::DevArray<float> reward, aux[MG_INFO_SLOTS];
        mg::DevArray<double> reward64, ep_reward;
        mg_info_dev ib;
    } ply;
    // mg_save_instances / mg_load_instances: the handle's number in this process (mg_instance_layout), the host-side counters, and what a load passes
    // from its claim launch to the launches behind it, allocated at the handle's first load (include/memgym.h)
    uint64_t serial = 0;
    int64_t instance_saves = 0, instance_loads = 0;
    int64_t frame_saves = 0, frame_draws = 0;  // mg_debug_counter: mg_save_frames / mg_draw_frames calls with count > 0
    int64_t debug_frame_saves = 0, debug_frame_draws = 0;  // mg_debug_counter: mg_save_debug_frames / mg_draw_debug_frames calls with count > 0
    // mg_split_episodes / mg_draw_frames_padded: the host-side counters, and what a split passes from its count launch to its write launch, allocated at
    // the handle's first split (include/memgym.h)
    int64_t sequence_splits = 0, padded_draws = 0;
    struct Sequences {
        bool ready = false;
        mg::DevArray<int32_t> first;      // [num_envs] the sequences of the workgroup's instances in front of this one
        mg::DevArray<int32_t> block_sum;  // [ceil(num_envs / SEQ_BLOCK)] the workgroup's sum, then the sum of the workgroups in front of it
    } seq;
    struct Instances {
        bool ready = false;
        mg::DevArray<int32_t> claim;  // [num_envs] the entry of the current load that holds the instance
        mg::DevArray<uint8_t> mask;   // [num_envs] the row mask a load with obs_dev draws by
    } inst;
    // mg_step_next: the calls, those that took a family's own kernel (Family::step_next), and the two flag rows of the handle's scratch, allocated at the
    // handle's first call (include/memgym.h)
    int64_t next_steps = 0, next_fused_steps = 0;
    struct Next {
        bool ready = false;
        mg::DevArray<uint8_t> active, restart;  // [num_envs] each: !restart_dev[i] (the composed form's mask) and a copy of restart_dev, which may be done_dev
    } nxt;
    std::string id;
    int obs_format = MG_OBS_U8_XYC;
    float* vec_dev = nullptr;     // the caller's vector-observation binding (mg_bind_vector_obs), or the single-instance block's
    float* vec_dev_caller = nullptr;
    int prof_stride = 0;
    // mg_single_open: pinned, device-mapped host buffers of the single-instance fast path (host address, device address)
    struct Single {
        bool open = false;
        char *host = nullptr, *dev = nullptr;
        size_t bytes = 0;
        size_t o_action = 0, o_seed = 0, o_obs = 0, o_vec = 0, o_reward32 = 0, o_reward = 0, o_done = 0, o_gt32 = 0, o_gt = 0, o_ep_reward = 0,
               o_ep_length = 0, o_aux = 0, o_flag = 0;
        uint32_t ticket = 0;      // completion flag protocol of mg_single_step (see there)
        bool use_flag = true;     // single_wait: false once this runtime has refused a stream memory operation
    } single;
};

namespace {
struct StateHeader {
    char magic[8];
    uint32_t version, num_envs;
    uint64_t payload, id_hash;
    uint8_t pad[32];
};
static_assert(sizeof(StateHeader) == 64, "state header is 64 bytes");
uint64_t fnv1a(const std::string& s) {
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
    return h;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        MG_HIP(hipGetDevice(&prev));
        if (prev != device) MG_HIP(hipSetDevice(device));
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

template <typename F>
int guarded(mg_env* env, F&& f) {
    try {
        if (!env || !env->fam) {
            mg::set_error("null handle");
            return -1;
        }
        DeviceGuard guard(env->device);  // the caller's current device is left as it was
        f();
        return 0;
    } catch (const mg::OptionError& e) {
        mg::set_error(e.msg);
        return e.code;
    } catch (const std::exception& e) {
        mg::set_error(e.what());
        return -1;
    }
}
}  // namespace

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

extern "C" {

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

// Rows of the observation buffer whose flag is set, copied to the same rows of another buffer (mg_step with mg_info_buffers.final_obs_dev:
// after a step without auto-reset the rows of the finished instances ARE the terminal observations).  A workgroup looks at 16 flags with one
// load and copies the rows a ballot names, six 16-byte vectors per lane in flight (a uint8 row is 1,323 vectors: one round); rows are whole
// vectors in every output format.
typedef uint32_t row_vec16 __attribute__((ext_vector_type(4)));
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
            hipLaunchKernelGGL(debug_stretch_kernel, dim3(grid), dim3(256), 0, st, frames, rgb_dev, env->num_envs);
            MG_HIP(hipGetLastError());
            MG_HIP(hipStreamSynchronize(st));
        } catch (...) {
            (void)hipFree(frames);
            throw;
        }
        MG_HIP(hipFree(frames));
    });
}

}  // extern "C"
namespace {
// mg_step and mg_step_masked (`who` names the entry point in messages).  active == NULL: every instance steps, in the family's own arrangement.
// active != NULL: the same three branches with the mask handed through to Family::step -- a masked step never takes a family's fused forms, so
// kept terminal observations always go the generic way: inactive instances report done == 0 there, and the copy and the masked reset need nothing new.
void step_call(mg_env* env, const char* who, const int32_t* actions_dev, const uint8_t* active_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev,
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
            hipLaunchKernelGGL(copy_rows_kernel, dim3(std::min((n + COPY_CHUNK - 1) / COPY_CHUNK, 16384)), dim3(256), 0, st, done_dev, (const row_vec16*)obs_dev,
                               (row_vec16*)ib.final_obs_dev, n, vec_per_row);
            MG_HIP(hipGetLastError());
        } else f->raster_only(ib.final_obs_dev, done_dev, st);
        f->reset(nullptr, done_dev, obs_dev, gt_dev, st);
    } else {
        f->step(actions_dev, active_dev, obs_dev, reward_dev, done_dev, gt_dev, &ib, autoreset, st);
    }
    if (active_dev) ++env->masked_steps;
    if (ib.gt64_dev) f->ground_truth64(ib.gt64_dev, st, active_dev);
}
}  // namespace
extern "C" {

int mg_step(mg_env* env, const int32_t* actions_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
            const mg_info_buffers* info, int autoreset, void* stream) {
    return guarded(env, [&] { step_call(env, "mg_step", actions_dev, nullptr, obs_dev, reward_dev, done_dev, gt_dev, info, autoreset, (hipStream_t)stream); });
}

int mg_step_masked(mg_env* env, const int32_t* actions_dev, const uint8_t* active_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
                   const mg_info_buffers* info, int autoreset, void* stream) {
    return guarded(env, [&] {
        if (!env->started) throw std::runtime_error("mg_step_masked: before the first mg_reset / mg_set_state");
        step_call(env, "mg_step_masked", actions_dev, active_dev, obs_dev, reward_dev, done_dev, gt_dev, info, autoreset, (hipStream_t)stream);
    });
}

}  // extern "C"
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

int mg_step_next(mg_env* env, const int32_t* actions_dev, const uint8_t* restart_dev, void* obs_dev, float* reward_dev, uint8_t* done_dev, float* gt_dev,
                 const mg_info_buffers* info, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_step_next: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (!actions_dev || !restart_dev || !obs_dev || !reward_dev || !done_dev)
            throw std::runtime_error(who + "NULL buffer (actions_dev, restart_dev, obs_dev, reward_dev and done_dev are required: mg_reset has no headless form)");
        const mg::InfoArgs ia = mg::read_info(info);
        if (ia.dev.final_obs_dev || ia.final_frames)
            throw std::runtime_error(who + "final_obs_dev / final_frames_dev are set: there are no terminal rows in this mode, the terminal frame is the observation");
        mg::Family* f = env->fam;
        if (f->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset before the next step");
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs;
        mg_env::Next& X = env->nxt;
        if (!X.ready) {  // the handle's first call: the only one that allocates (and therefore not capturable)
            if (mg::stream_capturing(st))
                throw std::runtime_error(who + "the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
            X.active.alloc(n);
            X.restart.alloc(n);
            X.ready = true;
        }
        const mg_info_dev& ib = ia.dev;
        if (f->step_next(actions_dev, restart_dev, X.restart.p, obs_dev, reward_dev, done_dev, gt_dev, &ib, st)) {
            ++env->next_fused_steps;
        } else {  // the pair of the definition
            hipLaunchKernelGGL(next_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, restart_dev, X.active.p, X.restart.p);
            MG_HIP(hipGetLastError());
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
        if (!env->started) throw std::runtime_error("mg_expert_actions: before the first mg_reset / mg_set_state");
        if (!(eps >= 0.0 && eps <= 1.0)) throw std::runtime_error("mg_expert_actions: eps outside [0, 1]");
        env->fam->expert_actions(mg::ExpertArgs{eps, mg::expert_base(seed, step), actions_dev}, (hipStream_t)stream);
    });
}

}  // extern "C"
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
// mg_save_frames' row-gather launch (defined with the frame records below): the traced loop forms keep each step's descriptor rows with it
__global__ __launch_bounds__(256) void frame_rows_save_kernel(const row_vec16* __restrict__ descs, int vec_per_row, const int32_t* __restrict__ idx, int count,
                                                              int num_envs, row_vec16* __restrict__ rec, int* err);
namespace {
// mg_rollout_trace as the caller's header laid it out (include/memgym.h), checked like mg_advance_out: -> the rows, all NULL without a trace
mg::TraceRows read_trace(const std::string& who, const mg_rollout_trace* trace, bool teacher) {
    mg_rollout_trace t;
    memset(&t, 0, sizeof(t));
    if (trace) {
        const size_t sz = trace->struct_size;
        if (sz < sizeof(t) || sz > sizeof(t) + 16 * sizeof(void*) || sz % sizeof(void*) != 0)
            throw std::runtime_error(who + ": mg_rollout_trace.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h; set it to sizeof(mg_rollout_trace)");
        memcpy(&t, trace, sizeof(t));
    }
    if ((uintptr_t)t.frames_dev & 15u) throw std::runtime_error(who + ": mg_rollout_trace.frames_dev is not 16-byte aligned");
    if (!teacher && (t.actions_dev || t.labels_dev))
        throw std::runtime_error(who + ": mg_rollout_trace.actions_dev / labels_dev are set: the tape is the caller's and there is no teacher (mg_advance_traced fills them)");
    if (((uintptr_t)t.actions_dev | (uintptr_t)t.labels_dev) & 7u) throw std::runtime_error(who + ": mg_rollout_trace.actions_dev / labels_dev are not 8-byte aligned");
    return mg::TraceRows{t.frames_dev, t.actions_dev, t.labels_dev, t.reward_dev, t.done_dev};
}

// row t of a frame trace <- the descriptor rows as they stand: mg_save_frames(env, NULL, num_envs, ...) without its checks and its counter
void save_frame_row(mg_env* env, void* frames, int t, hipStream_t st) {
    const std::pair<const void*, size_t> rows = env->fam->frame_rows();
    const int n = env->num_envs, vec_per_row = (int)(rows.second / 16);
    const int64_t lanes = (int64_t)n * vec_per_row;
    hipLaunchKernelGGL(frame_rows_save_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, (const row_vec16*)rows.first, vec_per_row,
                       (const int32_t*)nullptr, n, n, (row_vec16*)((char*)frames + (size_t)t * (size_t)n * rows.second), env->fam->error_word());
    MG_HIP(hipGetLastError());
}

// mg_advance and mg_advance_traced (trace == NULL: the untraced call, launch for launch what it was)
void advance_call(mg_env* env, const std::string& who, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out,
                  const mg_rollout_trace* trace, void* stream) {
    if (!env->started) throw std::runtime_error(who + ": before the first mg_reset / mg_set_state");
    if (steps < 1) throw std::runtime_error(who + ": steps < 1");
    if (!(eps >= 0.0 && eps <= 1.0)) throw std::runtime_error(who + ": eps outside [0, 1]");
    mg_advance_out o;
    memset(&o, 0, sizeof(o));
    if (out) {  // (as the caller's header laid it out: a shorter struct lacks the later slots)
        const size_t sz = out->struct_size;
        if (sz < offsetof(mg_advance_out, aux_sum_dev) || sz > sizeof(o) + 16 * sizeof(void*) || sz % sizeof(void*) != 0)
            throw std::runtime_error(who + ": mg_advance_out.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h; set it to sizeof(mg_advance_out)");
        memcpy(&o, out, sz < sizeof(o) ? sz : sizeof(o));
    }
    o.struct_size = sizeof(o);
    const mg::TraceRows T = read_trace(who, trace, true);
    const bool traced = trace != nullptr;
    if (traced && env->fam->geometry_dirty()) throw std::runtime_error(who + ": options that change geometry need a reset before the next step");
    hipStream_t st = (hipStream_t)stream;
    mg::Family* f = env->fam;
    const int n = env->num_envs;
    mg_env::Advance& A = env->adv;
    if (!A.ready) {  // the handle's first call: the only one that allocates (and therefore not capturable)
        if (mg::stream_capturing(st))
            throw std::runtime_error(who + ": the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
        A.actions.alloc((size_t)n * 2);
        A.reward.alloc(n);
        A.done.alloc(n);
        A.reward64.alloc(n);
        A.ep_reward.alloc(n);
        A.ep_length.alloc(n);
        memset(&A.ib, 0, sizeof(A.ib));
        A.ib.struct_size = sizeof(A.ib);
        A.ib.reward64_dev = A.reward64.p;
        A.ib.ep_reward_dev = A.ep_reward.p;
        A.ib.ep_length_dev = A.ep_length.p;
        for (int k = 0; k < MG_INFO_SLOTS && f->info_name(k); ++k) {
            A.aux[k].alloc(n);
            A.ib.aux_dev[k] = A.aux[k].p;
        }
        A.ready = true;
    }
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
        if (out) {
            hipLaunchKernelGGL(advance_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, t == 0 ? 1 : 0, A.ib, (const uint8_t*)d, o);
            MG_HIP(hipGetLastError());
        }
        if (T.frames) save_frame_row(env, T.frames, t, st);
    }
    env->headless_steps += steps;
    if (traced) env->traced_steps += steps;
}
}  // namespace
extern "C" {

int mg_advance(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out, void* stream) {
    return guarded(env, [&] { advance_call(env, "mg_advance", steps, eps, seed, step0, gt_dev, out, nullptr, stream); });
}

int mg_advance_traced(mg_env* env, int32_t steps, double eps, uint64_t seed, uint64_t step0, float* gt_dev, const mg_advance_out* out,
                      const mg_rollout_trace* trace, void* stream) {
    return guarded(env, [&] { advance_call(env, "mg_advance_traced", steps, eps, seed, step0, gt_dev, out, trace, stream); });
}

}  // extern "C"
// One step of mg_play's loop form: advance_accumulate_kernel's additions in its order (a paused instance's rows are the zeros of the masked step: its sums
// stay 0), then the step counts where the instance was alive, and MG_PLAY_EPISODE: an instance that has just finished is alive no longer.
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
// mg_play and mg_play_traced (frames_dev: the trace's frame rows; traced: the call came with a trace.  Without one: mg_play, launch for launch what it was)
void play_call(mg_env* env, const std::string& who, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, float* reward_trace_dev,
               uint8_t* done_trace_dev, int32_t* steps_played_dev, float* gt_dev, const mg_advance_out* sums, void* frames_dev, bool traced, void* stream) {
    if (!env->started) throw std::runtime_error(who + ": before the first mg_reset / mg_set_state");
    if (steps < 1) throw std::runtime_error(who + ": steps < 1");
    if (!tape_dev) throw std::runtime_error(who + ": tape_dev is NULL");
    if (mode != MG_PLAY_THROUGH && mode != MG_PLAY_EPISODE) throw std::runtime_error(who + ": mode is neither MG_PLAY_THROUGH nor MG_PLAY_EPISODE");
    if (env->fam->geometry_dirty()) throw std::runtime_error(who + ": options that change geometry need a reset before the next step");
    mg_advance_out o;
    memset(&o, 0, sizeof(o));
    if (sums) {  // (as the caller's header laid it out: a shorter struct lacks the later slots)
        const size_t sz = sums->struct_size;
        if (sz < offsetof(mg_advance_out, aux_sum_dev) || sz > sizeof(o) + 16 * sizeof(void*) || sz % sizeof(void*) != 0)
            throw std::runtime_error(who + ": mg_advance_out.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h; set it to sizeof(mg_advance_out)");
        memcpy(&o, sums, sz < sizeof(o) ? sz : sizeof(o));
    }
    o.struct_size = sizeof(o);
    hipStream_t st = (hipStream_t)stream;
    mg::Family* f = env->fam;
    const int n = env->num_envs;
    mg_env::Play& P = env->ply;
    if (!P.ready) {  // the handle's first call: the only one that allocates (and therefore not capturable)
        if (mg::stream_capturing(st))
            throw std::runtime_error(who + ": the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
        P.alive.alloc(n);
        P.reward.alloc(n);
        P.done.alloc(n);
        P.reward64.alloc(n);
        P.ep_reward.alloc(n);
        P.ep_length.alloc(n);
        memset(&P.ib, 0, sizeof(P.ib));
        P.ib.struct_size = sizeof(P.ib);
        P.ib.reward64_dev = P.reward64.p;
        P.ib.ep_reward_dev = P.ep_reward.p;
        P.ib.ep_length_dev = P.ep_length.p;
        for (int k = 0; k < MG_INFO_SLOTS && f->info_name(k); ++k) {
            P.aux[k].alloc(n);
            P.ib.aux_dev[k] = P.aux[k].p;
        }
        P.ready = true;
    }
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
        if (accumulate) {
            hipLaunchKernelGGL(play_accumulate_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, t == 0 ? 1 : 0, episode, P.ib, (const uint8_t*)d,
                               episode ? P.alive.p : (uint8_t*)active_dev, steps_played_dev, o);
            MG_HIP(hipGetLastError());
        }
        if (frames_dev) save_frame_row(env, frames_dev, t, st);  // (an instance the step left alone keeps its descriptor: its row repeats it)
    }
    env->headless_steps += steps;
    if (mask) env->masked_steps += steps;
    if (traced) env->traced_steps += steps;
}
}  // namespace
extern "C" {

int mg_play(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, float* reward_trace_dev, uint8_t* done_trace_dev,
            int32_t* steps_played_dev, float* gt_dev, const mg_advance_out* sums, void* stream) {
    return guarded(env, [&] {
        play_call(env, "mg_play", tape_dev, steps, mode, active_dev, reward_trace_dev, done_trace_dev, steps_played_dev, gt_dev, sums, nullptr, false, stream);
    });
}

int mg_play_traced(mg_env* env, const int32_t* tape_dev, int32_t steps, int mode, const uint8_t* active_dev, int32_t* steps_played_dev, float* gt_dev,
                   const mg_advance_out* sums, const mg_rollout_trace* trace, void* stream) {
    return guarded(env, [&] {
        const mg::TraceRows T = read_trace("mg_play_traced", trace, false);
        play_call(env, "mg_play_traced", tape_dev, steps, mode, active_dev, T.reward, T.done, steps_played_dev, gt_dev, sums, T.frames, trace != nullptr, stream);
    });
}

// ---- instance records (include/memgym.h: mg_save_instances / mg_load_instances; the kernels: mg_instances.hpp) ----
}  // extern "C"
namespace {
// head of both calls: the refusals of include/memgym.h, then the family's row table
mg::InstanceRows instance_call(mg_env* env, const char* who, int32_t count, const void* rec_dev) {
    if (!env->started) throw std::runtime_error(std::string(who) + ": before the first mg_reset / mg_set_state");
    if (count < 0) throw std::runtime_error(std::string(who) + ": count < 0");
    if (!rec_dev || ((uintptr_t)rec_dev & 15u)) throw std::runtime_error(std::string(who) + ": rec_dev is NULL or not 16-byte aligned");
    if (env->fam->geometry_dirty()) throw std::runtime_error(std::string(who) + ": options that change geometry need a reset first");
    return mg::make_instance_rows(env->fam->instance_rows());
}
}  // namespace
extern "C" {

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
        const mg::InstanceRows t = instance_call(env, "mg_save_instances", count, rec_dev);
        if (count == 0) return;
        hipStream_t st = (hipStream_t)stream;
        env->fam->before_instance_save(st);
        hipLaunchKernelGGL(mg::instance_rows_kernel<true>, dim3((count + mg::INSTANCE_WAVES - 1) / mg::INSTANCE_WAVES, mg::instance_splits(t)),
                           dim3(64 * mg::INSTANCE_WAVES), 0, st, t, idx_dev, (const int32_t*)nullptr, (const int32_t*)nullptr, count, env->num_envs,
                           (char*)rec_dev, env->fam->error_word());
        MG_HIP(hipGetLastError());
        ++env->instance_saves;
    });
}

int mg_load_instances(mg_env* env, const int32_t* idx_dev, const int32_t* rec_of_dev, int32_t count, const void* rec_dev, void* obs_dev, void* stream) {
    return guarded(env, [&] {
        const mg::InstanceRows t = instance_call(env, "mg_load_instances", count, rec_dev);
        if (count == 0) return;
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs;
        mg_env::Instances& I = env->inst;
        if (!I.ready) {  // the handle's first load: the only one that allocates (and therefore not capturable)
            if (mg::stream_capturing(st))
                throw std::runtime_error("mg_load_instances: the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
            I.claim.alloc(n);
            I.mask.alloc(n);
            I.ready = true;
        }
        if (obs_dev) MG_HIP(hipMemsetAsync(I.mask.p, 0, (size_t)n, st));
        hipLaunchKernelGGL(mg::load_claim_kernel, dim3((count + 255) / 256), dim3(256), 0, st, idx_dev, rec_of_dev, count, n, I.claim.p,
                           obs_dev ? I.mask.p : (uint8_t*)nullptr, env->fam->error_word());
        MG_HIP(hipGetLastError());
        hipLaunchKernelGGL(mg::instance_rows_kernel<false>, dim3((count + mg::INSTANCE_WAVES - 1) / mg::INSTANCE_WAVES, mg::instance_splits(t)),
                           dim3(64 * mg::INSTANCE_WAVES), 0, st, t, idx_dev, rec_of_dev, (const int32_t*)I.claim.p, count, n, (char*)rec_dev,
                           env->fam->error_word());
        MG_HIP(hipGetLastError());
        if (obs_dev) env->fam->raster_only(obs_dev, I.mask.p, st);  // the masked step's dense launch: the loaded instances' frames, other rows untouched
        ++env->instance_loads;
    });
}

}  // extern "C"
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
extern "C" {

// ---- frame records (include/memgym.h: mg_save_frames / mg_draw_frames; mg_frame_records.hpp and the gather forms of the two raster skeletons) ----
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
        const std::string who = "mg_save_frames: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::frame_save_refusal(count, rec_dev)) throw std::runtime_error(who + no);
        if (env->fam->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset first");
        if (count == 0) return;
        const std::pair<const void*, size_t> rows = env->fam->frame_rows();
        const int vec_per_row = (int)(rows.second / 16);
        const int64_t lanes = (int64_t)count * vec_per_row;
        hipLaunchKernelGGL(frame_rows_save_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const row_vec16*)rows.first,
                           vec_per_row, idx_dev, count, env->num_envs, (row_vec16*)rec_dev, env->fam->error_word());
        MG_HIP(hipGetLastError());
        ++env->frame_saves;
    });
}

int mg_draw_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format, void* obs_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_draw_frames: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::frame_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, format, obs_dev)) throw std::runtime_error(who + no);
        if (env->fam->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset first");
        if (count == 0) return;
        env->fam->draw_records(rec_dev, (int)n_records, pick_dev, (int)count, format, obs_dev, (hipStream_t)stream);
        ++env->frame_draws;
    });
}

// ---- episode sequences (include/memgym.h: mg_split_episodes / mg_sequence_picks / mg_draw_frames_padded; mg_sequences.hpp and the PAD forms of the two
// gather rasters) ----
int mg_split_episodes(mg_env* env, const uint8_t* done_dev, int32_t steps, const int32_t* steps_of_dev, const uint8_t* start_dev, int32_t length,
                      mg_sequence* seq_dev, int32_t capacity, int32_t* count_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_split_episodes: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::split_refusal(done_dev, steps, length, seq_dev, capacity, count_dev, env->num_envs)) throw std::runtime_error(who + no);
        hipStream_t st = (hipStream_t)stream;
        const int n = env->num_envs, blocks = (n + mg::SEQ_BLOCK - 1) / mg::SEQ_BLOCK;
        mg_env::Sequences& Q = env->seq;
        if (!Q.ready) {
            if (mg::stream_capturing(st))
                throw std::runtime_error(who + "the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
            Q.first.alloc(n);
            Q.block_sum.alloc(blocks);
            Q.ready = true;
        }
        hipLaunchKernelGGL(mg::seq_count_kernel, dim3(blocks), dim3(mg::SEQ_BLOCK), 0, st, done_dev, steps, n, steps_of_dev, length, Q.first.p, Q.block_sum.p);
        MG_HIP(hipGetLastError());
        hipLaunchKernelGGL(mg::seq_scan_kernel, dim3(1), dim3(mg::SEQ_BLOCK), 0, st, Q.block_sum.p, blocks, count_dev);
        MG_HIP(hipGetLastError());
        if (capacity > 0) {
            hipLaunchKernelGGL(mg::seq_write_kernel, dim3(blocks), dim3(mg::SEQ_BLOCK), 0, st, done_dev, steps, n, steps_of_dev, start_dev, length,
                               (const int32_t*)Q.first.p, (const int32_t*)Q.block_sum.p, (int4*)seq_dev, capacity);
            MG_HIP(hipGetLastError());
        }
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
        hipLaunchKernelGGL(mg::seq_picks_kernel, dim3((unsigned)((lanes + mg::SEQ_BLOCK - 1) / mg::SEQ_BLOCK)), dim3(mg::SEQ_BLOCK), 0, (hipStream_t)stream,
                           (const int4*)seq_dev, count_dev, capacity, sel_dev, m, length, env->num_envs, pick_dev, mask_dev, env->fam->error_word());
        MG_HIP(hipGetLastError());
    });
}

int mg_draw_frames_padded(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int format, void* obs_dev,
                          void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_draw_frames_padded: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::frame_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, format, obs_dev)) throw std::runtime_error(who + no);
        if (env->fam->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset first");
        if (count == 0) return;
        env->fam->draw_records_padded(rec_dev, (int)n_records, pick_dev, (int)count, format, obs_dev, (hipStream_t)stream);
        ++env->padded_draws;
    });
}

// ---- debug-view records (include/memgym.h: mg_save_debug_frames / mg_draw_debug_frames; the picked *_debug_desc kernels of the three families, the debug
// gather forms of the two raster skeletons, mg_debug_stream_out.hpp) ----
int mg_save_debug_frames(mg_env* env, const int32_t* idx_dev, int32_t count, void* rec_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_save_debug_frames: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::frame_save_refusal(count, rec_dev)) throw std::runtime_error(who + no);
        if (env->fam->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset first");
        if (!idx_dev && count > env->num_envs) throw std::runtime_error(who + "idx_dev is NULL and count > num_envs");
        if (count == 0) return;
        env->fam->save_debug_records(idx_dev, count, rec_dev, (hipStream_t)stream);
        ++env->debug_frame_saves;
    });
}

int mg_draw_debug_frames(mg_env* env, const void* rec_dev, int64_t n_records, const int32_t* pick_dev, int64_t count, int size, void* rgb_dev, void* stream) {
    return guarded(env, [&] {
        const std::string who = "mg_draw_debug_frames: ";
        if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
        if (const char* no = mg::debug_draw_refusal(rec_dev, n_records, pick_dev != nullptr, count, size, rgb_dev)) throw std::runtime_error(who + no);
        if (env->fam->geometry_dirty()) throw std::runtime_error(who + "options that change geometry need a reset first");
        if (count == 0) return;
        env->fam->draw_debug_records(rec_dev, (int)n_records, pick_dev, (int)count, size, rgb_dev, (hipStream_t)stream);
        ++env->debug_frame_draws;
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

// ---- the single-instance fast path (include/memgym.h: mg_single_io) ----
} // extern "C"
namespace {
// Wait for everything enqueued on `st` WITHOUT hipStreamSynchronize (round 6): a stream memory operation writes the
// call's ticket into the pinned block behind the step's launches (the command processor executes it when they have completed -- and
// with them their stores into the same pinned block), and the host polls that word.  hipStreamSynchronize on this runtime costs
// more than the step's kernels once the work is this small.  A wait that takes longer than 50 ms (a fault, a debugger) falls back to the
// synchronising call, which also reports the stream's error; a runtime without stream memory operations synchronises as before.
void single_wait(mg_env::Single& S, hipStream_t st, bool stored = false) {
    if (S.use_flag) {
        // stored: the step's own last kernel stores the ticket (Family::done_flag_stored; S.ticket was advanced when it said so)
        const uint32_t want = stored ? S.ticket : ++S.ticket;
        if (stored || hipStreamWriteValue32(st, S.dev + S.o_flag, want, 0) == hipSuccess) {
            volatile uint32_t* flag = (volatile uint32_t*)(S.host + S.o_flag);
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t spins = 0;; ++spins) {
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) return;
                __builtin_ia32_pause();
                if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
            }
        } else {
            (void)hipGetLastError();
            S.use_flag = false;
        }
    }
    MG_HIP(hipStreamSynchronize(st));
}
}  // namespace
extern "C" {
int mg_single_open(mg_env* env, mg_single_io* io) {
    return guarded(env, [&] {
        if (!io || io->struct_size != sizeof(mg_single_io)) throw std::runtime_error("mg_single_open: set io->struct_size = sizeof(mg_single_io)");
        if (env->num_envs != 1) throw std::runtime_error("mg_single_open: the handle must hold exactly one instance");
        mg_env::Single& S = env->single;
        if (!S.open) {
            size_t o = 0;
            auto take = [&](size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; };
            S.o_action = take(8); S.o_seed = take(8);
            S.o_obs = take(84 * 84 * 3 * 4);  // room for every observation format
            S.o_vec = take(sizeof(float) * 256);
            S.o_reward32 = take(4); S.o_reward = take(8); S.o_done = take(1);
            S.o_gt32 = take(sizeof(float) * 8); S.o_gt = take(sizeof(double) * 8);
            S.o_ep_reward = take(8); S.o_ep_length = take(4); S.o_aux = take(sizeof(float) * MG_INFO_SLOTS * 64);  // (one 256-byte line per slot)
            S.o_flag = take(4);
            S.bytes = o;
            MG_HIP(hipHostMalloc((void**)&S.host, S.bytes, hipHostMallocMapped | hipHostMallocCoherent));
            memset(S.host, 0, S.bytes);
            MG_HIP(hipHostGetDevicePointer((void**)&S.dev, S.host, 0));
            S.open = true;
        }
        if (env->fam->vec_dim()) {  // the vector observation is written at every reset, into the mapped buffer from now on (io->vec;
            env->vec_dev = (float*)(S.dev + S.o_vec);  // a buffer bound earlier with mg_bind_vector_obs is no longer written)
            env->fam->bind_vector_obs(env->vec_dev);
        }
        io->obs = S.host + S.o_obs;
        io->vec = env->fam->vec_dim() ? (float*)(S.host + S.o_vec) : nullptr;
        io->reward = (double*)(S.host + S.o_reward);
        io->done = (uint8_t*)(S.host + S.o_done);
        io->gt = (double*)(S.host + S.o_gt);
        io->ep_reward = (double*)(S.host + S.o_ep_reward);
        io->ep_length = (int32_t*)(S.host + S.o_ep_length);
        for (int k = 0; k < MG_INFO_SLOTS; ++k) io->aux[k] = (float*)(S.host + S.o_aux + 256 * k);
    });
}

int mg_single_reset(mg_env* env, int64_t seed, int has_seed, void* stream) {
    return guarded(env, [&] {
        mg_env::Single& S = env->single;
        if (!S.open) throw std::runtime_error("mg_single_reset: mg_single_open first");
        hipStream_t st = (hipStream_t)stream;
        *(int64_t*)(S.host + S.o_seed) = seed;
        mg::Family* f = env->fam;
        f->reset(has_seed ? (const int64_t*)(S.dev + S.o_seed) : nullptr, nullptr, S.dev + S.o_obs, f->gt_dim() ? (float*)(S.dev + S.o_gt32) : nullptr, st);
        f->ground_truth64((double*)(S.dev + S.o_gt), st);
        env->started = true;
        single_wait(S, st);
    });
}

int mg_single_step(mg_env* env, int32_t a0, int32_t a1, void* stream) {
    int flags = 0;
    const int rc = guarded(env, [&] {
        mg_env::Single& S = env->single;
        if (!S.open) throw std::runtime_error("mg_single_step: mg_single_open first");
        hipStream_t st = (hipStream_t)stream;
        int32_t* act = (int32_t*)(S.host + S.o_action);
        act[0] = a0;
        act[1] = a1;
        mg_info_dev ib;
        memset(&ib, 0, sizeof(ib));
        ib.struct_size = sizeof(ib);
        ib.ep_reward_dev = (double*)(S.dev + S.o_ep_reward);
        ib.ep_length_dev = (int32_t*)(S.dev + S.o_ep_length);
        for (int k = 0; k < MG_INFO_SLOTS; ++k) ib.aux_dev[k] = (float*)(S.dev + S.o_aux + 256 * k);
        ib.reward64_dev = (double*)(S.dev + S.o_reward);
        mg::Family* f = env->fam;
        f->want_done_flag((uint32_t*)(S.dev + S.o_flag), S.ticket + 1);
        f->step((const int32_t*)(S.dev + S.o_action), nullptr, S.dev + S.o_obs, (float*)(S.dev + S.o_reward32), (uint8_t*)(S.dev + S.o_done),
                f->gt_dim() ? (float*)(S.dev + S.o_gt32) : nullptr, &ib, 0, st);
        const bool stored = f->done_flag_stored();  // the step's own last kernel stores the ticket: nothing may follow it (gt_dim() is 0 then)
        if (stored) ++S.ticket;
        f->ground_truth64((double*)(S.dev + S.o_gt), st);
        single_wait(S, st, stored);
        flags = f->peek_errors();  // (the word lives in pinned host memory: a plain read; saves the caller a second native call per step)
    });
    return rc != 0 ? rc : flags;
}

size_t mg_state_size(const mg_env* env) {
    if (!env) return 0;
    size_t t = sizeof(StateHeader);
    for (auto& b : env->fam->state_blobs()) t += b.second;
    return t;
}

int mg_get_state(mg_env* env, void* host_buf, size_t size) {
    return guarded(env, [&] {
        if (!host_buf || size < mg_state_size(env)) throw std::runtime_error("mg_get_state: buffer too small");
        MG_HIP(hipDeviceSynchronize());
        env->fam->sync_state();
        StateHeader h;
        memset(&h, 0, sizeof(h));
        memcpy(h.magic, "MGSTATE1", 8);
        h.version = MG_STATE_VERSION;
        h.num_envs = (uint32_t)env->num_envs;
        h.payload = mg_state_size(env) - sizeof(StateHeader);
        h.id_hash = fnv1a(env->id);
        memcpy(host_buf, &h, sizeof(h));
        char* p = (char*)host_buf + sizeof(StateHeader);
        for (auto& b : env->fam->state_blobs()) {
            MG_HIP(hipMemcpy(p, b.first, b.second, hipMemcpyDeviceToHost));
            p += b.second;
        }
    });
}

int mg_set_state(mg_env* env, const void* host_buf, size_t size) {
    return guarded(env, [&] {
        if (!host_buf || size < sizeof(StateHeader)) throw std::runtime_error("mg_set_state: buffer too small for a state header");
        StateHeader h;
        memcpy(&h, host_buf, sizeof(h));
        if (memcmp(h.magic, "MGSTATE1", 8) != 0) throw std::runtime_error("mg_set_state: not a memgym state blob (bad magic)");
        if (h.version != MG_STATE_VERSION)
            throw std::runtime_error("mg_set_state: state version " + std::to_string(h.version) + ", this library reads version " +
                                     std::to_string(MG_STATE_VERSION));
        if (h.id_hash != fnv1a(env->id)) throw std::runtime_error("mg_set_state: the blob belongs to another env id than " + env->id);
        if (h.num_envs != (uint32_t)env->num_envs)
            throw std::runtime_error("mg_set_state: the blob holds " + std::to_string(h.num_envs) + " instances, the handle " +
                                     std::to_string(env->num_envs));
        if (h.payload != mg_state_size(env) - sizeof(StateHeader) || size < mg_state_size(env))
            throw std::runtime_error("mg_set_state: payload size differs from this handle's state");
        MG_HIP(hipDeviceSynchronize());
        const char* p = (const char*)host_buf + sizeof(StateHeader);
        for (auto& b : env->fam->state_blobs()) {
            MG_HIP(hipMemcpy(b.first, p, b.second, hipMemcpyHostToDevice));
            p += b.second;
        }
        env->fam->on_state_loaded();  // reset(seed=None) / auto-reset are legal on a restored handle
        env->started = true;
    });
}

int mg_set_profiling(mg_env* env, int on) {
    return guarded(env, [&] {
        env->prof_stride = on < 0 ? 0 : on;
        env->fam->prof.stride = env->prof_stride;
        env->fam->prof.count[0] = env->fam->prof.count[1] = 0;
    });
}

int mg_get_profile(mg_env* env, int kind, double* total_ms, int64_t* launches) {
    return guarded(env, [&] {
        if (kind < 0 || kind > 1 || !total_ms || !launches) throw std::runtime_error("mg_get_profile: bad arguments");
        env->fam->prof.collect(kind, total_ms, launches);
    });
}

int mg_poll_errors(mg_env* env, int* flags) {
    return guarded(env, [&] {
        if (!flags) throw std::runtime_error("mg_poll_errors: NULL");
        MG_HIP(hipDeviceSynchronize());
        *flags = env->fam->poll_errors();
    });
}

int mg_peek_errors(mg_env* env, int* flags) {
    return guarded(env, [&] {
        if (!flags) throw std::runtime_error("mg_peek_errors: NULL");
        *flags = env->fam->peek_errors();
    });
}

int mg_enable_peer_access(int device, int peer_device) {
    try {
        int prev = 0;
        MG_HIP(hipGetDevice(&prev));
        struct Restore {
            int d;
            ~Restore() { (void)hipSetDevice(d); }
        } restore{prev};
        if (device == peer_device) return 0;
        int can = 0;
        MG_HIP(hipDeviceCanAccessPeer(&can, device, peer_device));
        if (!can) {
            mg::set_error("device " + std::to_string(device) + " has no peer access to device " + std::to_string(peer_device));
            return -1;
        }
        MG_HIP(hipSetDevice(device));
        hipError_t e = hipDeviceEnablePeerAccess(peer_device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
            (void)hipGetLastError();
            mg::set_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            return -1;
        }
        (void)hipGetLastError();
        return 0;
    } catch (const std::exception& e) {
        mg::set_error(e.what());
        return -1;
    }
}

int mg_debug_counter(mg_env* env, const char* name, int64_t* value) {
    return guarded(env, [&] {
        if (!name || !value) throw std::runtime_error("mg_debug_counter: NULL");
        MG_HIP(hipDeviceSynchronize());
        if (std::string(name) == "final_obs_generic_steps") {  // every id: which way mg_step kept the terminal observations is decided in this file
            *value = env->final_obs_generic_steps;
            return;
        }
        if (std::string(name) == "headless_steps" || std::string(name) == "advance_fused_steps") {  // every id: counted in this file
            *value = std::string(name) == "headless_steps" ? env->headless_steps : env->advance_fused_steps;
            return;
        }
        if (std::string(name) == "play_fused_steps") {  // every id: counted in this file (only the mortar family has the form)
            *value = env->play_fused_steps;
            return;
        }
        if (std::string(name) == "traced_steps" || std::string(name) == "traced_fused_steps") {  // every id: counted in this file
            *value = std::string(name) == "traced_steps" ? env->traced_steps : env->traced_fused_steps;
            return;
        }
        if (std::string(name) == "instance_saves" || std::string(name) == "instance_loads") {  // every id: counted in this file
            *value = std::string(name) == "instance_saves" ? env->instance_saves : env->instance_loads;
            return;
        }
        if (std::string(name) == "frame_saves" || std::string(name) == "frame_draws") {  // every id: counted in this file
            *value = std::string(name) == "frame_saves" ? env->frame_saves : env->frame_draws;
            return;
        }
        if (std::string(name) == "sequence_splits" || std::string(name) == "padded_draws") {  // every id: counted in this file
            *value = std::string(name) == "sequence_splits" ? env->sequence_splits : env->padded_draws;
            return;
        }
        if (std::string(name) == "debug_frame_saves" || std::string(name) == "debug_frame_draws") {  // every id: counted in this file
            *value = std::string(name) == "debug_frame_saves" ? env->debug_frame_saves : env->debug_frame_draws;
            return;
        }
        if (std::string(name) == "masked_steps") {  // every id: counted in this file
            *value = env->masked_steps;
            return;
        }
        if (std::string(name) == "next_steps" || std::string(name) == "next_fused_steps") {  // every id: counted in this file
            *value = std::string(name) == "next_steps" ? env->next_steps : env->next_fused_steps;
            return;
        }
        if (std::string(name) == "final_frame_steps") {  // every id: counted in this file
            *value = env->final_frame_steps;
            return;
        }
        if (!env->fam->debug_counter(name, value)) throw std::runtime_error(std::string("mg_debug_counter: no counter named ") + name + " for " + env->id);
    });
}

int mg_debug_rng(mg_env* env, int32_t i, uint64_t* out) {
    return guarded(env, [&] {
        if (i < 0 || i >= env->num_envs) throw std::runtime_error("mg_debug_rng: index out of range");
        MG_HIP(hipDeviceSynchronize());
        env->fam->sync_state();
        env->fam->debug_rng(i, out);
    });
}

int mg_debug_set_rng(mg_env* env, int32_t i, const uint64_t* in) {
    return guarded(env, [&] {
        if (i < 0 || i >= env->num_envs) throw std::runtime_error("mg_debug_set_rng: index out of range");
        if (!in) throw std::runtime_error("mg_debug_set_rng: NULL");
        if (!(in[3] & 1)) throw std::runtime_error("mg_debug_set_rng: a PCG64 increment is odd");
        MG_HIP(hipDeviceSynchronize());
        env->fam->sync_state();
        env->fam->debug_set_rng(i, in);
    });
}

}  // extern "C"
