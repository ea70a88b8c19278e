// mg_sequences.hpp -- mg_split_episodes / mg_sequence_picks (include/memgym.h): a rollout's done rows cut into episode sequences of at most `length` steps,
// and the sequences turned into [m][length] picks for mg_draw_frames_padded.  Nothing here depends on the family: included from mg_api_records.hpp only.
// The table's ORDER is part of the definition -- (instance, t0) ascending -- so no atomic decides where an entry lands: a lane per instance counts its
// sequences, a scan over the instances gives every lane its first entry, a lane per instance walks its column again and writes.  Lanes of a wave read 64
// neighbouring bytes of a done row in both walks.  Three small launches: count (with the scan inside each workgroup), the scan of the workgroups' sums
// (one workgroup), write.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/memgym.h"
#include "mg_frame_records.hpp"

namespace mg {

constexpr int SEQ_BLOCK = 256;
static_assert(sizeof(mg_sequence) == 16, "an entry of the table is stored as one 16-byte vector");

// What mg_split_episodes refuses whatever the handle's state: NULL = nothing, else the words of the refusal.
inline const char* split_refusal(const void* done_dev, int32_t steps, int32_t length, const void* seq_dev, int32_t capacity, const void* count_dev,
                                 int32_t num_envs) {
    if (!done_dev) return "done_dev is NULL";
    if (!count_dev) return "count_dev is NULL";
    if (steps < 1) return "steps < 1";
    if (length < 1) return "length < 1";
    if (capacity < 0) return "capacity < 0";
    if (capacity > 0 && !aligned16(seq_dev)) return "seq_dev is NULL or not 16-byte aligned with capacity > 0";
    if (((int64_t)steps + 1) * (int64_t)num_envs > (int64_t)INT32_MAX) return "(steps + 1) * num_envs > INT32_MAX";
    return nullptr;
}

// The same for mg_sequence_picks.
inline const char* picks_refusal(const void* seq_dev, const void* count_dev, int32_t capacity, int32_t m, int32_t length, const void* pick_dev) {
    if (!count_dev) return "count_dev is NULL";
    if (capacity < 0) return "capacity < 0";
    if (capacity > 0 && !aligned16(seq_dev)) return "seq_dev is NULL or not 16-byte aligned with capacity > 0";
    if (m < 0) return "m < 0";
    if (length < 1) return "length < 1";
    if (!pick_dev) return "pick_dev is NULL";
    if ((int64_t)m * (int64_t)length > (int64_t)INT32_MAX) return "m * length > INT32_MAX";
    return nullptr;
}

// n_i of the definition
__device__ __forceinline__ int seq_steps_of(const int32_t* __restrict__ steps_of, int i, int steps) {
    if (!steps_of) return steps;
    const int v = steps_of[i];
    return v < 0 ? 0 : (v > steps ? steps : v);
}

// exclusive scan of one int per lane over a workgroup of SEQ_BLOCK lanes; *total = the workgroup's sum (valid in every lane).  A collective call.
__device__ __forceinline__ int seq_block_scan(int v, int* total) {
    __shared__ int wave_sum[SEQ_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();  // (a second call in one kernel: the last call's sums have been read)
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEQ_BLOCK / 64; ++w) {
        const int s = wave_sum[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

// Launch 1: lane i counts the sequences of instance i; first[i] <- the number of sequences of the workgroup's instances in front of i, block_sum[b] <- the
// workgroup's sum.
__global__ __launch_bounds__(SEQ_BLOCK) void seq_count_kernel(const uint8_t* __restrict__ done, int steps, int num_envs, const int32_t* __restrict__ steps_of,
                                                              int length, int32_t* __restrict__ first, int32_t* __restrict__ block_sum) {
    const int i = blockIdx.x * SEQ_BLOCK + threadIdx.x;
    int c = 0;
    if (i < num_envs) {
        const int n_i = seq_steps_of(steps_of, i, steps);
        const uint8_t* col = done + i;
        int t0 = 0;
        for (int t = 0; t < n_i; ++t) {
            const bool d = col[(size_t)t * num_envs] != 0;
            if (d || t - t0 + 1 == length || t == n_i - 1) {
                ++c;
                t0 = t + 1;
            }
        }
    }
    int total;
    const int before = seq_block_scan(c, &total);
    if (i < num_envs) first[i] = before;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// Launch 2, ONE workgroup: block_sum[b] <- the sum of the workgroups in front of b; *count <- the sum of all, the true number of sequences.
__global__ __launch_bounds__(SEQ_BLOCK) void seq_scan_kernel(int32_t* __restrict__ block_sum, int blocks, int32_t* __restrict__ count) {
    int carry = 0;
    for (int base = 0; base < blocks; base += SEQ_BLOCK) {
        const int b = base + threadIdx.x;
        const int v = b < blocks ? block_sum[b] : 0;
        int total;
        const int before = seq_block_scan(v, &total);
        if (b < blocks) block_sum[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *count = carry;
}

// Launch 3: lane i walks instance i again and writes its entries from block_sum[b] + first[i] on, as long as they lie below `capacity`.
__global__ __launch_bounds__(SEQ_BLOCK) void seq_write_kernel(const uint8_t* __restrict__ done, int steps, int num_envs, const int32_t* __restrict__ steps_of,
                                                              const uint8_t* __restrict__ start, int length, const int32_t* __restrict__ first,
                                                              const int32_t* __restrict__ block_sum, int4* __restrict__ seq, int capacity) {
    const int i = blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (i >= num_envs) return;
    int at = block_sum[blockIdx.x] + first[i];
    if (at >= capacity) return;
    const int n_i = seq_steps_of(steps_of, i, steps);
    const uint8_t* col = done + i;
    bool is_first = start ? start[i] != 0 : true;
    int t0 = 0;
    for (int t = 0; t < n_i; ++t) {
        const bool d = col[(size_t)t * num_envs] != 0;
        if (d || t - t0 + 1 == length || t == n_i - 1) {
            seq[at] = make_int4(i, t0, t - t0 + 1, (is_first ? MG_SEQ_FIRST : 0) | (d ? MG_SEQ_LAST : 0));
            if (++at >= capacity) return;
            t0 = t + 1;
            is_first = d;
        }
    }
}

// mg_sequence_picks: a lane per element of pick[m][length].  The sequence's entry is one 16-byte load, the same for the `length` lanes of a row.
__global__ __launch_bounds__(SEQ_BLOCK) void seq_picks_kernel(const int4* __restrict__ seq, const int32_t* __restrict__ count, int capacity,
                                                              const int32_t* __restrict__ sel, int m, int length, int num_envs, int32_t* __restrict__ pick,
                                                              uint8_t* __restrict__ mask, int* err) {
    const int64_t e = (int64_t)blockIdx.x * SEQ_BLOCK + threadIdx.x;
    if (e >= (int64_t)m * length) return;
    const int j = (int)(e / length), l = (int)(e - (int64_t)j * length);
    const int have = *count, valid = have < capacity ? (have < 0 ? 0 : have) : capacity;
    const int s = sel ? sel[j] : j;
    int p = -1;
    if (s >= 0 && s < valid) {
        const int4 q = seq[s];  // {instance, t0, len, flags}
        if (l < q.z) p = (q.y + l) * num_envs + q.x;
    } else if (s >= valid && sel && l == 0) {
        __hip_atomic_fetch_or(err, ERR_FRAME_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    pick[e] = p;
    if (mask) mask[e] = p >= 0 ? 1 : 0;
}

}  // namespace mg
