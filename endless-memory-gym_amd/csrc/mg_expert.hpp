// mg_expert.hpp -- what the three families' expert kernels share (include/memgym.h: mg_expert_actions): the launch shape -- one LANE per instance, one small
// launch per call, nothing but loads of the records the step kernels keep and one store of the action --, the eps-random branch (mg_expert_hash.hpp) and
// the two controllers' "move towards" rules as the oracle's expert hooks write them (oracle/mgo_mortar.c mm_expert, mgo_mystery.c mpf_expert, mgo_spot.c sp_expert).
#pragma once
#include "mg_expert_hash.hpp"
#include "mg_family.hpp"

namespace mg {
struct ExpertArgs {
    double eps;
    uint64_t base;     // expert_base(seed, step)
    int32_t* actions;  // int32 [n] (Discrete) or [n][2]: the layout mg_step reads
};
constexpr int EXPERT_BLOCK = 256;
inline dim3 expert_grid(int n) { return dim3((unsigned)((n + EXPERT_BLOCK - 1) / EXPERT_BLOCK)); }

#ifdef __HIPCC__
// grid controller (actions 0 none, 1 turn left, 2 turn right, 3 forward): face `want` degrees, then move
__device__ __forceinline__ int expert_grid_action(int rot, int want) {
    if (rot == want) return 3;
    const int d = ((want - rot) % 360 + 360) % 360;
    return (d == 90 || d == 180) ? 1 : 2;
}
__device__ __forceinline__ int expert_grid_facing(int dx, int dy) { return dx > 0 ? 270 : (dx < 0 ? 90 : (dy < 0 ? 0 : 180)); }
// free controller, one axis (0 none, 1 towards smaller, 2 towards larger): stand still within `slack` pixels
__device__ __forceinline__ int expert_axis_action(int d, int slack) { return abs(d) < slack ? 0 : (d < 0 ? 1 : 2); }
// the expert action (a0, a1) of instance i, or the random one its draw gives it
__device__ __forceinline__ void expert_store(const ExpertArgs& x, int i, bool discrete, int a0, int a1) {
    const ExpertDraw r = expert_draw(x.base, (uint64_t)i, x.eps, discrete);
    a0 = r.random ? r.a0 : a0;
    a1 = r.random ? r.a1 : a1;
    if (discrete) x.actions[i] = a0;
    else *reinterpret_cast<int2*>(x.actions + 2 * (size_t)i) = make_int2(a0, a1);
}
#endif
}  // namespace mg
