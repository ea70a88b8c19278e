// mg_expert_hash.hpp -- the random branch of the scripted teacher (include/memgym.h: mg_expert_actions), shared by the three families' expert kernels:
// with probability eps instance i plays a uniformly random action instead of its expert action.  The numbers are a counter-based hash of
// (seed, step, i) -- oracle/mgo_api.c mgo_batch_expert, restated here operation by operation -- and belong to the caller, not to any instance's
// PCG64 stream.  No HIP and no project includes: host programs include this file as it is (tests/test_expert_hash.py).
#pragma once
#include <cstdint>

namespace mg {
constexpr uint64_t expert_mix64(uint64_t z) {  // (mgo_mix64: splitmix64's finaliser behind its increment)
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// what every instance of a call shares: computed once on the host and handed to the kernel
constexpr uint64_t expert_base(uint64_t seed, uint64_t step) { return expert_mix64(seed ^ (step * 0xD1B54A32D192ED03ull)); }

struct ExpertDraw {
    bool random;     // the instance plays (a0, a1) instead of its expert action
    int32_t a0, a1;  // Discrete: a0 in 0..3, a1 = 0; MultiDiscrete: 0..2 each
};
constexpr ExpertDraw expert_draw(uint64_t base, uint64_t i, double eps, bool discrete) {
    const uint64_t h = expert_mix64(base + i);
    if (!((double)(h >> 11) * (1.0 / 9007199254740992.0) < eps)) return ExpertDraw{false, 0, 0};
    const uint64_t h2 = expert_mix64(h);
    return ExpertDraw{true, (int32_t)(h2 % (discrete ? 4u : 3u)), discrete ? 0 : (int32_t)((h2 >> 20) % 3u)};
}
}  // namespace mg
