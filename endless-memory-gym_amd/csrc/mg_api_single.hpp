// mg_api_single.hpp -- the single-instance fast path of include/memgym.h (mg_single_io): a handle of one instance whose actions, observation and step
// results live in one pinned, device-mapped block, so that a step is a few stores, the family's launches and a poll.  Included by mg_api.hip alone.
#pragma once
#include <chrono>

#include "mg_api_env.hpp"

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

}  // extern "C"
