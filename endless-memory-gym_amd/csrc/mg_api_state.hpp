// mg_api_state.hpp -- what include/memgym.h offers around a handle's state: checkpoints (mg_state_size / mg_get_state / mg_set_state), kernel timing,
// the error word, peer access, and the debug counters and RNG access the tests use.  Included by mg_api.hip alone.
#pragma once
#include "mg_api_env.hpp"

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

// mg_debug_counter: the counters the C ABI keeps in the handle itself, for every env id (which way mg_step kept the terminal observations, how many steps
// a rollout took inside a family's launches, ...: the comments are at the members, mg_api_env.hpp); a family's own go through Family::debug_counter
struct HandleCounter {
    const char* name;
    int64_t mg_env::*count;
};
const HandleCounter HANDLE_COUNTERS[] = {
    {"final_obs_generic_steps", &mg_env::final_obs_generic_steps}, {"headless_steps", &mg_env::headless_steps},
    {"advance_fused_steps", &mg_env::advance_fused_steps}, {"play_fused_steps", &mg_env::play_fused_steps},
    {"traced_steps", &mg_env::traced_steps}, {"traced_fused_steps", &mg_env::traced_fused_steps},
    {"instance_saves", &mg_env::instance_saves}, {"instance_loads", &mg_env::instance_loads},
    {"frame_saves", &mg_env::frame_saves}, {"frame_draws", &mg_env::frame_draws},
    {"sequence_splits", &mg_env::sequence_splits}, {"padded_draws", &mg_env::padded_draws},
    {"debug_frame_saves", &mg_env::debug_frame_saves}, {"debug_frame_draws", &mg_env::debug_frame_draws},
    {"masked_steps", &mg_env::masked_steps}, {"next_steps", &mg_env::next_steps},
    {"next_fused_steps", &mg_env::next_fused_steps}, {"final_frame_steps", &mg_env::final_frame_steps},
    {"episode_positions", &mg_env::episode_positions}, {"window_picks", &mg_env::window_picks},
    {"row_gathers", &mg_env::row_gathers}, {"rollout_targets", &mg_env::rollout_targets},
};
}  // namespace

extern "C" {

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
        for (const HandleCounter& c : HANDLE_COUNTERS) {  // every id: counted in the C ABI's own code
            if (std::string(name) == c.name) {
                *value = env->*c.count;
                return;
            }
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
