// mg_windows.hpp -- mg_episode_positions / mg_window_picks / mg_gather_rows_padded (include/memgym.h, MEMORY WINDOWS): the position of every store row
// inside its episode, the [m][window] picks of sliding windows that may reach back into the previous trace, and the gather of [count] rows of any byte
// length with zero rows at the pads.  Nothing here depends on the family: included from mg_api_windows.hpp only.
// The first part -- what the three calls refuse, and the access width the gather's host side chooses -- is host code that compiles without a GPU compiler
// (tests/host/windows_check.cpp); the kernels follow behind __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/memgym.h"
#include "mg_frame_records.hpp"

namespace mg {

// What mg_episode_positions refuses whatever the handle's state: NULL = nothing, else the words of the refusal.
inline const char* positions_refusal(const void* done_dev, int32_t steps, const void* pos_dev, int32_t num_envs) {
    if (!done_dev) return "done_dev is NULL";
    if (!pos_dev) return "pos_dev is NULL";
    if (steps < 1) return "steps < 1";
    if (((int64_t)steps + 1) * (int64_t)num_envs > (int64_t)INT32_MAX) return "(steps + 1) * num_envs > INT32_MAX";
    return nullptr;
}

// The same for mg_window_picks.
inline const char* window_picks_refusal(const void* pos_dev, int32_t steps, bool has_sel, int32_t m, int32_t window, int32_t lag, int32_t back,
                                        const void* pick_dev, int32_t num_envs) {
    if (!pos_dev) return "pos_dev is NULL";
    if (!pick_dev) return "pick_dev is NULL";
    if (steps < 1) return "steps < 1";
    if (m < 0) return "m < 0";
    if (window < 1) return "window < 1";
    if (lag < 0) return "lag < 0";
    if (back < 0) return "back < 0";
    if ((int64_t)m * (int64_t)window > (int64_t)INT32_MAX) return "m * window > INT32_MAX";
    if (((int64_t)back + (int64_t)steps + 1) * (int64_t)num_envs > (int64_t)INT32_MAX) return "(back + steps + 1) * num_envs > INT32_MAX";
    if (!has_sel && (int64_t)m > ((int64_t)steps + 1) * (int64_t)num_envs) return "sel_dev is NULL and m > (steps + 1) * num_envs";
    return nullptr;
}

// The same for mg_gather_rows_padded.  Rows and picks are counted in 32 bits (a pick is an int32), byte offsets in 64.  The two ranges the host knows --
// n_rows rows of the source, count rows of the destination -- must not share a byte.
inline const char* gather_rows_refusal(const void* src_dev, int64_t n_rows, int64_t row_bytes, bool has_pick, int64_t count, const void* dst_dev) {
    if (count < 0) return "count < 0";
    if (n_rows < 0) return "n_rows < 0";
    if (row_bytes < 1) return "row_bytes < 1";
    if (n_rows > (int64_t)INT32_MAX) return "n_rows > INT32_MAX";
    if (count > (int64_t)INT32_MAX) return "count > INT32_MAX";
    if (row_bytes > (int64_t)INT32_MAX) return "row_bytes > INT32_MAX";
    if (!has_pick && count > n_rows) return "pick_dev is NULL and count > n_rows";
    if (count == 0) return nullptr;
    if (!dst_dev) return "dst_dev is NULL";
    if (!src_dev && n_rows > 0) return "src_dev is NULL";
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + (uintptr_t)n_rows * (uintptr_t)row_bytes;
    const uintptr_t d0 = (uintptr_t)dst_dev, d1 = d0 + (uintptr_t)count * (uintptr_t)row_bytes;
    if (s0 < d1 && d0 < s1) return "src_dev and dst_dev overlap";
    return nullptr;
}

// Bytes per access of the gather: the widest of 16 / 8 / 4 / 2 / 1 that divides row_bytes and both base addresses, so that every row of either side
// starts on a multiple of it (csrc/mg_instances.hpp's row table chooses the same way for its rows).
inline uint32_t gather_width(const void* src_dev, const void* dst_dev, int64_t row_bytes) {
    const uintptr_t all = (uintptr_t)src_dev | (uintptr_t)dst_dev | (uintptr_t)row_bytes | 16u;
    return (uint32_t)(all & (~all + 1u));  // the lowest set bit
}

// A row of fewer units than this takes the PACKED form (lanes over the flattened units); from here on the ROW form (a wave per row) has at least half
// of its lanes at work.
constexpr int64_t GATHER_ROW_FORM_UNITS = 32;
inline bool gather_packed(int64_t row_bytes, uint32_t width) { return row_bytes / (int64_t)width < GATHER_ROW_FORM_UNITS; }

}  // namespace mg

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "mg_sequences.hpp"

namespace mg {

constexpr int WIN_BLOCK = 256;

// mg_episode_positions: lane i walks column i of done.  The lanes of a wave read 64 neighbouring bytes of a done row and store 64 neighbouring int32
// (seq_count_kernel's walk).  A position stops counting at INT32_MAX.
__global__ __launch_bounds__(WIN_BLOCK) void episode_positions_kernel(const uint8_t* __restrict__ done, int steps, int num_envs,
                                                                     const int32_t* __restrict__ steps_of, const int32_t* __restrict__ pos0,
                                                                     int32_t* __restrict__ pos) {
    const int i = blockIdx.x * WIN_BLOCK + threadIdx.x;
    if (i >= num_envs) return;
    const int n_i = seq_steps_of(steps_of, i, steps);
    int p = 0;
    if (pos0) {
        const int v = pos0[i];
        p = v < 0 ? 0 : v;
    }
    const uint8_t* col = done + i;
    int32_t* out = pos + i;
    out[0] = p;
    for (int t = 0; t < steps; ++t) {
        if (t < n_i) p = col[(size_t)t * num_envs] != 0 ? 0 : (p == INT32_MAX ? p : p + 1);
        out[(size_t)(t + 1) * num_envs] = p;
    }
}

// mg_window_picks: a lane per element of pick[m][window].  The sample's position is one 4-byte load, the same for the `window` lanes of a row.
__global__ __launch_bounds__(WIN_BLOCK) void window_picks_kernel(const int32_t* __restrict__ pos, int steps, int num_envs, const int32_t* __restrict__ sel,
                                                                int m, int window, int lag, int back, int32_t* __restrict__ pick,
                                                                uint8_t* __restrict__ mask, int32_t* __restrict__ len_out, int* err) {
    const int64_t e = (int64_t)blockIdx.x * WIN_BLOCK + threadIdx.x;
    if (e >= (int64_t)m * window) return;
    const int j = (int)(e / window), l = (int)(e - (int64_t)j * window);
    const int64_t samples = ((int64_t)steps + 1) * num_envs;
    const int64_t s = sel ? (int64_t)sel[j] : (int64_t)j;
    int p = -1, len = 0;
    if (s >= 0 && s < samples) {
        const int t = (int)(s / num_envs), i = (int)(s - (int64_t)t * num_envs);
        const int64_t first = (int64_t)t - (int64_t)pos[s];  // the episode's first row
        const int64_t hi = (int64_t)t - lag;
        int64_t lo = hi - window + 1;
        lo = lo < first ? first : lo;
        lo = lo < -(int64_t)back ? -(int64_t)back : lo;
        len = hi >= lo ? (int)(hi - lo + 1) : 0;
        if (l < len) p = (int)(((int64_t)back + lo + l) * num_envs + i);
    } else if (s >= samples && l == 0) {  // (sel is set: without it the host has checked m)
        __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    pick[e] = p;
    if (mask) mask[e] = p >= 0 ? 1 : 0;
    if (len_out && l == 0) len_out[j] = len;
}

// ---- mg_gather_rows_padded.  V: the access, 16 / 8 / 4 / 2 / 1 bytes (gather_width); `units` of it make a row.
typedef uint32_t gather_vec16 __attribute__((ext_vector_type(4)));
typedef uint32_t gather_vec8 __attribute__((ext_vector_type(2)));

constexpr int GATHER_ROWS = 4;    // ROW form: rows a wave has in flight
constexpr int GATHER_WAVES = WIN_BLOCK / 64;
constexpr unsigned GATHER_MAX_GRID = 1u << 16;  // workgroups of a launch: beyond 16.7 M lanes every lane walks on with the grid's stride

// the pick of output row j, wave-uniform in the ROW form: >= 0 a source row, -1 a pad, -2 skip (beyond the rows of the call, or out of range: flagged by
// the caller's first lane)
__device__ __forceinline__ int gather_pick_of(const int32_t* __restrict__ pick, int64_t j, int64_t count, int n_rows, bool* flag) {
    *flag = false;
    if (j >= count) return -2;
    const int p = pick ? pick[j] : (int)j;
    if (p < 0) return -1;
    if (p >= n_rows) {
        *flag = true;
        return -2;
    }
    return p;
}

// ROW form: a wave takes GATHER_ROWS neighbouring output rows at a time and walks them together, 64 units of each per round: the loads of the round are
// all issued before its first store.  A pad row is stored from a register of zeros and loads nothing.
template <typename V>
__global__ __launch_bounds__(WIN_BLOCK) void gather_rows_kernel(const V* __restrict__ src, int n_rows, int units, const int32_t* __restrict__ pick,
                                                               int64_t count, V* __restrict__ dst, int* err) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * GATHER_WAVES;
    for (int64_t j0 = wave * GATHER_ROWS; j0 < count; j0 += waves * GATHER_ROWS) {
        int p[GATHER_ROWS];
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            bool flag;
            p[r] = __builtin_amdgcn_readfirstlane(gather_pick_of(pick, j0 + r, count, n_rows, &flag));
            if (flag && lane == 0) __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        for (int q = lane; q < units; q += 64) {
            V v[GATHER_ROWS];
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r) {
                v[r] = V{};
                if (p[r] >= 0) v[r] = src[(int64_t)p[r] * units + q];
            }
#pragma unroll
            for (int r = 0; r < GATHER_ROWS; ++r)
                if (p[r] >= -1) dst[(j0 + r) * units + q] = v[r];
        }
    }
}

// PACKED form for short rows: lanes over the flattened count * units accesses, so that a wave is not spent on a 4-byte row.
template <typename V>
__global__ __launch_bounds__(WIN_BLOCK) void gather_packed_kernel(const V* __restrict__ src, int n_rows, int units, const int32_t* __restrict__ pick,
                                                                 int64_t count, V* __restrict__ dst, int* err) {
    const int64_t total = count * units, stride = (int64_t)gridDim.x * WIN_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * WIN_BLOCK + threadIdx.x; e < total; e += stride) {
        const int64_t j = e / units;
        const int q = (int)(e - j * units);
        bool flag;
        const int p = gather_pick_of(pick, j, count, n_rows, &flag);
        if (flag && q == 0) __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (p < -1) continue;
        V v = V{};
        if (p >= 0) v = src[(int64_t)p * units + q];
        dst[e] = v;
    }
}

}  // namespace mg
#endif  // __HIPCC__
