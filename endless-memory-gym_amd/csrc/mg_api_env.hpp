// mg_api_env.hpp -- what every part of the C ABI (mg_api.hip and the mg_api_*.hpp it includes) works on: the handle, the error string, the wrapper
// that turns exceptions into return codes, and the heads the entry points share.  Included by mg_api.hip alone.
#pragma once
#include <string>

#include "mg_family.hpp"

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
    int64_t play_fused_steps = 0;      // mg_debug_counter: steps mg_play took inside a family's own launches (Family::play)
    int64_t traced_steps = 0, traced_fused_steps = 0;  // mg_debug_counter: steps of mg_advance_traced / mg_play_traced calls with a trace; those taken in-launch
    // mg_advance / mg_play: what the loop of the call's definition passes from launch to launch (include/memgym.h).  One type, two blocks: each is
    // allocated at the handle's first call of its own entry point, with the one row the other has no use for left out
    struct Rollout {
        bool ready = false;
        mg::DevArray<int32_t> actions;  // mg_advance alone: [num_envs * 2] the teacher's actions of a step
        mg::DevArray<uint8_t> alive;    // mg_play alone: [num_envs] the mask of MG_PLAY_EPISODE from launch to launch
        mg::DevArray<int32_t> ep_length;
        mg::DevArray<float> reward, aux[MG_INFO_SLOTS];
        mg::DevArray<uint8_t> done;
        mg::DevArray<double> reward64, ep_reward;
        mg_info_dev ib;
        void alloc(const mg::Family* f, size_t n, bool teacher) {
            if (teacher) actions.alloc(n * 2);
            else alive.alloc(n);
            reward.alloc(n);
            done.alloc(n);
            reward64.alloc(n);
            ep_reward.alloc(n);
            ep_length.alloc(n);
            memset(&ib, 0, sizeof(ib));
            ib.struct_size = sizeof(ib);
            ib.reward64_dev = reward64.p;
            ib.ep_reward_dev = ep_reward.p;
            ib.ep_length_dev = ep_length.p;
            for (int k = 0; k < MG_INFO_SLOTS && f->info_name(k); ++k) {
                aux[k].alloc(n);
                ib.aux_dev[k] = aux[k].p;
            }
        }
    } adv, ply;
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
    int64_t episode_positions = 0, window_picks = 0, row_gathers = 0;  // mg_debug_counter: mg_episode_positions / mg_window_picks / mg_gather_rows_padded calls
    int64_t rollout_targets = 0;  // mg_debug_counter: mg_rollout_targets calls that were not refused
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

// a 16-byte vector: what the row copies of the step's terminal observations and of the frame records move
typedef uint32_t row_vec16 __attribute__((ext_vector_type(4)));

namespace {
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

// ---- heads the entry points share.  `who` is the entry point's prefix WITH its colon and blank ("mg_x: "): every text a caller receives is spelt here once ----
void require_started(const mg_env* env, const std::string& who) {
    if (!env->started) throw std::runtime_error(who + "before the first mg_reset / mg_set_state");
}
// `before`: what the reset must come before -- "first", or "before the next step" (the text of the families' own guard, Family::require_geometry)
void require_geometry(const mg_env* env, const std::string& who, const char* before) {
    if (env->fam->geometry_dirty()) throw mg::stale_geometry(who, before);
}

// The first call of an entry point that keeps scratch rows in the handle (S: one of mg_env's blocks with a `ready` flag) is the only one that allocates,
// and therefore cannot be captured into a graph
template <class Scratch, class Alloc>
void first_call(Scratch& S, const std::string& who, hipStream_t st, Alloc&& alloc) {
    if (S.ready) return;
    if (mg::stream_capturing(st)) throw std::runtime_error(who + "the handle's first call allocates its scratch and cannot be captured; call it once eagerly");
    alloc();
    S.ready = true;
}

// Head of the record calls (instance, frame and debug-view records, saved or drawn), in the order callers rely on: started; `no`, what the call's own
// refusal function (mg_frame_records.hpp) has to say about its arguments, or NULL; the geometry; `also`, a refusal that comes behind the geometry.
// false: count == 0, there is nothing to do
bool record_call(const mg_env* env, const std::string& who, const char* no, int64_t count, const char* also = nullptr) {
    require_started(env, who);
    if (no) throw std::runtime_error(who + no);
    require_geometry(env, who, "first");
    if (also) throw std::runtime_error(who + also);
    return count != 0;
}
}  // namespace
