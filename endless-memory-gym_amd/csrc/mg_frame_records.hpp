// mg_frame_records.hpp -- mg_save_frames / mg_draw_frames (include/memgym.h): a frame kept as the descriptor row its step left, drawn later by the
// gather forms of the two raster skeletons (mg_raster_gather_v1.hpp, mg_raster_gather.hpp).  Here: what the two calls refuse, the layout value, the
// bytes of one observation row: host code that compiles without a GPU compiler (tests/host/frame_records_check.cpp).  The save's row gather is in mg_api_records.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/memgym.h"

namespace mg {

constexpr int ERR_FRAME_INDEX = 512;  // include/memgym.h: an instance index beyond the handle's instances / a pick outside the call's records; the entry was skipped

// mg_frame_layout: bit 63 (no mg_instance_layout value has it), the handle's number in the process, and a count of everything that makes a stored
// descriptor draw differently: the rebuilds mg_instance_layout counts (`geometry`) plus the changes of a composer, atlas or template choice that
// happen without one (`frames`: Family::frame_gen_).  Both only ever grow, so their sum changes whenever either does.
inline uint64_t frame_layout_value(uint64_t serial, uint64_t geometry, uint64_t frames) {
    return (1ull << 63) | ((serial & 0x7FFFFFFFFFull) << 24) | ((geometry + frames) & 0xFFFFFFull);
}

// bytes of one observation row in `format`; 0 = not a format of include/memgym.h
inline size_t frame_row_bytes(int format) {
    switch (format) {
        case MG_OBS_U8_XYC:
        case MG_OBS_U8_CYX: return (size_t)MG_OBS_BYTES;
        case MG_OBS_F16_CYX:
        case MG_OBS_BF16_CYX: return (size_t)MG_OBS_BYTES * 2;
        case MG_OBS_F32_CYX: return (size_t)MG_OBS_BYTES * 4;
        default: return 0;
    }
}

inline bool aligned16(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }

// What mg_save_frames refuses whatever the handle's state: NULL = nothing, else the words of the refusal.
inline const char* frame_save_refusal(int32_t count, const void* rec_dev) {
    if (count < 0) return "count < 0";
    if (!aligned16(rec_dev)) return "rec_dev is NULL or not 16-byte aligned";
    return nullptr;
}

// The same for mg_draw_frames.  The launch walks rows and records with 32-bit counters (row offsets are 64-bit), hence the two upper limits.
inline const char* frame_draw_refusal(const void* rec_dev, int64_t n_records, bool has_pick, int64_t count, int format, const void* obs_dev) {
    if (count < 0) return "count < 0";
    if (!aligned16(rec_dev)) return "rec_dev is NULL or not 16-byte aligned";
    if (!aligned16(obs_dev)) return "obs_dev is NULL or not 16-byte aligned";
    if (!frame_row_bytes(format)) return "unknown format";
    if (n_records > (int64_t)INT32_MAX) return "n_records > INT32_MAX";
    if (count > (int64_t)INT32_MAX) return "count > INT32_MAX";
    if (count > 0 && n_records < 1) return "n_records < 1 with count > 0";
    if (!has_pick && count > n_records) return "pick_dev is NULL and count > n_records";
    return nullptr;
}

// The same for mg_draw_debug_frames: mg_draw_frames' refusals with a size, 84 or 336, in place of a format.
inline const char* debug_draw_refusal(const void* rec_dev, int64_t n_records, bool has_pick, int64_t count, int size, const void* rgb_dev) {
    if (size != 84 && size != 336) return "size is neither 84 nor 336";
    if (!aligned16(rgb_dev)) return "rgb_dev is NULL or not 16-byte aligned";
    return frame_draw_refusal(rec_dev, n_records, has_pick, count, MG_OBS_U8_XYC, rgb_dev);
}

}  // namespace mg
