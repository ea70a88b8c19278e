// mg_info.hpp -- mg_info_buffers (include/memgym.h) as the library takes it in: the caller's struct read by its struct_size, split into the part the
// kernels carry by value (mg_info_dev) and the members that are younger than that part, and what mg_step refuses of them whatever the handle's state.
// Host code that compiles without a GPU compiler (tests/host/info_buffers_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../include/memgym.h"

// mg_info_buffers as the kernels see it: the members up to capacity_dev, in the header's order.  The step kernels carry it BY VALUE in their argument
// structs (a.info), so a member appended to the public struct would shift every kernel's argument layout; members younger than capacity_dev
// (final_frames_dev) therefore travel as arguments of their own, of the kernel forms that use them alone.
struct mg_info_dev {
    size_t struct_size;
    double* ep_reward_dev;
    int32_t* ep_length_dev;
    float* aux_dev[MG_INFO_SLOTS];
    void* final_obs_dev;
    double* reward64_dev;
    double* gt64_dev;
    uint8_t* capacity_dev;
};
static_assert(sizeof(mg_info_dev) == 120 && sizeof(mg_info_dev) == offsetof(mg_info_buffers, final_frames_dev) &&
                  offsetof(mg_info_dev, final_obs_dev) == offsetof(mg_info_buffers, final_obs_dev) &&
                  offsetof(mg_info_dev, capacity_dev) == offsetof(mg_info_buffers, capacity_dev),
              "mg_info_dev is mg_info_buffers up to capacity_dev: the kernels' argument layout");

namespace mg {

struct InfoArgs {
    mg_info_dev dev;     // all NULL where the caller passed none, or a shorter (older) struct
    void* final_frames;  // mg_info_buffers.final_frames_dev
};

constexpr size_t INFO_SIZE_MIN = offsetof(mg_info_buffers, final_obs_dev);  // the episode-record pointers every layout has
// Nothing larger than this build's struct plus room for a few future members is a layout of include/memgym.h.  (A caller built against the header of
// round 2 -- no struct_size member -- has a device POINTER in this place: 8-aligned and huge.)
constexpr size_t INFO_SIZE_MAX = sizeof(mg_info_buffers) + 16 * sizeof(void*);

// mg_info_buffers as the caller's header laid it out (include/memgym.h: struct_size); throws what mg_step reports
inline InfoArgs read_info(const mg_info_buffers* info) {
    InfoArgs r;
    memset(&r, 0, sizeof(r));
    r.dev.struct_size = sizeof(r.dev);
    if (!info) return r;
    const size_t sz = info->struct_size;
    if (sz < INFO_SIZE_MIN || sz > INFO_SIZE_MAX || sz % sizeof(void*) != 0)
        throw std::runtime_error("mg_step: mg_info_buffers.struct_size = " + std::to_string(sz) + " is not a layout of include/memgym.h (" +
                                 std::to_string(sizeof(mg_info_buffers)) + " in this build); set it to sizeof(mg_info_buffers)");
    mg_info_buffers ib;
    memset(&ib, 0, sizeof(ib));
    memcpy(&ib, info, sz < sizeof(ib) ? sz : sizeof(ib));  // a shorter (older) struct: the fields it lacks stay NULL
    memcpy(&r.dev, &ib, sizeof(r.dev));
    r.dev.struct_size = sizeof(r.dev);
    r.final_frames = ib.final_frames_dev;
    return r;
}

// What mg_step / mg_step_masked refuse of the terminal-frame members whatever the handle's state: NULL = nothing, else the words of the refusal.
inline const char* final_frames_refusal(const InfoArgs& a, bool headless) {
    if (a.final_frames && a.dev.final_obs_dev) return "final_frames_dev together with final_obs_dev: terminal frames are kept as records or as frames, the caller picks one";
    if ((uintptr_t)a.final_frames & 15u) return "final_frames_dev is not 16-byte aligned";
    if (headless && a.dev.final_obs_dev) return "obs_dev is NULL (a headless step) together with final_obs_dev: terminal observations are frames";
    return nullptr;
}

}  // namespace mg
