// tests/c_abi/c_abi_instances.cpp -- TEST INFRASTRUCTURE.  mg_save_instances / mg_load_instances as a C++ trainer calls them: no Python, no torch.
// Two handles of the same env id, seeds and actions.  Handle A saves every instance, leaves the common trajectory for a while, loads the records
// (instance i <- record (i + 7) % n) and must from then on equal the never-loaded twin B row for row ((i + 7) % n): frames, rewards, dones.
// Usage: c_abi_instances ENV_ID NUM_ENVS STEPS   -> prints "OK ..." and exits 0, or the first mismatch and exits 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "memgym.h"

#define HIP_OK(e)                                                                  \
    do {                                                                           \
        hipError_t e_ = (e);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_));                \
            return 2;                                                              \
        }                                                                          \
    } while (0)
#define MG_OK(e)                                                                   \
    do {                                                                           \
        if ((e) != 0) {                                                            \
            fprintf(stderr, "%s: %s\n", #e, mg_last_error());                      \
            return 2;                                                              \
        }                                                                          \
    } while (0)

static uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s ENV_ID NUM_ENVS STEPS\n", argv[0]);
        return 2;
    }
    const char* env_id = argv[1];
    const int n = atoi(argv[2]), steps = atoi(argv[3]);
    const size_t frame = 84 * 84 * 3;
    const int pre = 30, away = 15;

    HIP_OK(hipSetDevice(0));
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    mg_env *A = nullptr, *B = nullptr;
    MG_OK(mg_create(env_id, n, 0, &A));
    MG_OK(mg_create(env_id, n, 0, &B));
    const int adim = mg_action_dim(A), n_act = adim == 1 ? 4 : 3;

    uint8_t *obs_a, *obs_b, *done_a, *done_b, *rec;
    float *rew_a, *rew_b;
    int32_t *act_a, *act_b, *idx, *rec_of;
    int64_t* seeds;
    HIP_OK(hipMalloc((void**)&obs_a, frame * n));
    HIP_OK(hipMalloc((void**)&obs_b, frame * n));
    HIP_OK(hipMalloc((void**)&done_a, n));
    HIP_OK(hipMalloc((void**)&done_b, n));
    HIP_OK(hipMalloc((void**)&rew_a, sizeof(float) * n));
    HIP_OK(hipMalloc((void**)&rew_b, sizeof(float) * n));
    HIP_OK(hipMalloc((void**)&act_a, sizeof(int32_t) * n * 2));
    HIP_OK(hipMalloc((void**)&act_b, sizeof(int32_t) * n * 2));
    HIP_OK(hipMalloc((void**)&idx, sizeof(int32_t) * n));
    HIP_OK(hipMalloc((void**)&rec_of, sizeof(int32_t) * n));
    HIP_OK(hipMalloc((void**)&seeds, sizeof(int64_t) * n));

    // before the first reset both calls are refused
    if (mg_save_instances(A, nullptr, n, obs_a, stream) != -1) { printf("a save before the first reset was not refused\n"); return 1; }

    std::vector<int64_t> h_seeds(n);
    std::vector<int32_t> h_idx(n), h_rec(n), perm(n);
    for (int i = 0; i < n; ++i) {
        h_seeds[i] = 77 + i;
        h_idx[i] = i;
        perm[i] = h_rec[i] = (i + 7) % n;
    }
    HIP_OK(hipMemcpy(seeds, h_seeds.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(idx, h_idx.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rec_of, h_rec.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    MG_OK(mg_reset(A, seeds, nullptr, obs_a, nullptr, stream));
    MG_OK(mg_reset(B, seeds, nullptr, obs_b, nullptr, stream));

    const size_t rec_bytes = mg_instance_bytes(A);
    if (rec_bytes == 0 || rec_bytes % 16 != 0) { printf("mg_instance_bytes = %zu\n", rec_bytes); return 1; }
    if (mg_instance_layout(A) == mg_instance_layout(B)) { printf("two handles share a layout value\n"); return 1; }
    HIP_OK(hipMalloc((void**)&rec, rec_bytes * n));

    std::vector<int32_t> h_act((size_t)n * 2), h_act_p((size_t)n * 2);
    auto draw = [&](uint64_t t, uint64_t salt) {
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < adim; ++k) h_act[(size_t)i * adim + k] = (int32_t)(mix(salt ^ (t * 1315423911ull + (uint64_t)i * 2 + k)) % (uint64_t)n_act);
    };
    // the common trajectory
    for (int t = 0; t < pre; ++t) {
        draw(t, 1);
        HIP_OK(hipMemcpy(act_a, h_act.data(), sizeof(int32_t) * n * adim, hipMemcpyHostToDevice));
        MG_OK(mg_step(A, act_a, obs_a, rew_a, done_a, nullptr, nullptr, 1, stream));
        MG_OK(mg_step(B, act_a, obs_b, rew_b, done_b, nullptr, nullptr, 1, stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    MG_OK(mg_save_instances(A, nullptr, n, rec, stream));
    for (int t = 0; t < away; ++t) {  // A alone, other actions
        draw(t, 2);
        HIP_OK(hipMemcpy(act_a, h_act.data(), sizeof(int32_t) * n * adim, hipMemcpyHostToDevice));
        MG_OK(mg_step(A, act_a, obs_a, rew_a, done_a, nullptr, nullptr, 1, stream));
        HIP_OK(hipStreamSynchronize(stream));
    }
    MG_OK(mg_load_instances(A, idx, rec_of, n, rec, obs_a, stream));
    HIP_OK(hipStreamSynchronize(stream));

    std::vector<uint8_t> fa(frame * n), fb(frame * n), da(n), db(n);
    std::vector<float> ra(n), rb(n);
    auto compare = [&](int t) -> int {
        HIP_OK(hipMemcpy(fa.data(), obs_a, frame * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(fb.data(), obs_b, frame * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            if (memcmp(&fa[frame * i], &fb[frame * perm[i]], frame) != 0) {
                printf("step %d: the frame of instance %d differs from the twin's instance %d\n", t, i, perm[i]);
                return 1;
            }
        return 0;
    };
    if (int rc = compare(-1)) return rc;
    long ended = 0;
    for (int t = 0; t < steps; ++t) {
        draw(t, 3);  // the twin's actions; A's row i takes the twin's row perm[i]
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < adim; ++k) h_act_p[(size_t)i * adim + k] = h_act[(size_t)perm[i] * adim + k];
        HIP_OK(hipMemcpy(act_b, h_act.data(), sizeof(int32_t) * n * adim, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(act_a, h_act_p.data(), sizeof(int32_t) * n * adim, hipMemcpyHostToDevice));
        MG_OK(mg_step(A, act_a, obs_a, rew_a, done_a, nullptr, nullptr, 1, stream));
        MG_OK(mg_step(B, act_b, obs_b, rew_b, done_b, nullptr, nullptr, 1, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (int rc = compare(t)) return rc;
        HIP_OK(hipMemcpy(ra.data(), rew_a, sizeof(float) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(rb.data(), rew_b, sizeof(float) * n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(da.data(), done_a, n, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(db.data(), done_b, n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) {
            if (memcmp(&ra[i], &rb[perm[i]], sizeof(float)) != 0 || da[i] != db[perm[i]]) {
                printf("step %d: reward / done of instance %d differ from the twin's instance %d\n", t, i, perm[i]);
                return 1;
            }
            ended += da[i];
        }
    }
    int flags = 0;
    MG_OK(mg_poll_errors(A, &flags));
    if (flags) { printf("error bits 0x%x\n", flags); return 1; }
    int64_t saves = 0, loads = 0;
    MG_OK(mg_debug_counter(A, "instance_saves", &saves));
    MG_OK(mg_debug_counter(A, "instance_loads", &loads));
    if (saves != 1 || loads != 1) { printf("counters: %lld saves, %lld loads\n", (long long)saves, (long long)loads); return 1; }
    printf("OK %s: %d instances, %d steps after the load equal the twin's, %ld episodes ended, %zu bytes per record\n", env_id, n, steps, ended, rec_bytes);
    mg_destroy(A);
    mg_destroy(B);
    return 0;
}
