// mg_targets.hpp -- mg_rollout_targets / mg_sum_columns (include/memgym.h, ROLLOUT TARGETS): generalised advantage estimates, returns, a valid mask and
// per-instance moments of a rollout's reward / done / value rows, one lane per instance walking its column backwards, and the fixed-order sum of
// per-instance columns.  Nothing here depends on the family: included from mg_api_targets.hpp only.
// The first part -- what the two calls refuse, the arithmetic of one row and the walk of one column -- is host code too and compiles without a GPU
// compiler (tests/host/rollout_targets_check.cpp): the kernel is that walk with a lane for `i`.  The kernels follow behind __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/memgym.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MG_TARGETS_HD __host__ __device__ __forceinline__
#else
#define MG_TARGETS_HD inline
#endif
// Every float operation of the definition is rounded on its own: no multiply is fused into an add, whatever -ffp-contract says on the command line.
#ifdef __clang__
#define MG_TARGETS_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MG_TARGETS_UNROLL _Pragma("unroll")
#else
#define MG_TARGETS_NO_CONTRACT
#define MG_TARGETS_UNROLL
#endif

namespace mg {

// Rows of a block: the walk issues every load of TARGETS_T rows before it uses the first (profiles/rollout_targets.md holds the values tried).
#ifndef MG_TARGETS_T
#define MG_TARGETS_T 16
#endif
constexpr int TARGETS_T = MG_TARGETS_T;

// The arrays of a call, as the header names them; optional ones may be NULL.
struct TargetArrays {
    const float* reward;
    const uint8_t* done;
    const float* value;
    const int32_t* steps_of;
    const uint8_t* skip;
    const uint8_t* trunc;
    const float* final_value;
    float* adv;
    float* ret;
    uint8_t* valid;
    double* col;
};

// ---- what the calls refuse whatever the handle's state: NULL = nothing, else the words of the refusal ----
inline bool targets_share_a_byte(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline const char* rollout_targets_refusal(const TargetArrays& A, int32_t steps, int32_t num_envs, float gamma, float lambda) {
    if (!A.reward) return "reward_dev is NULL";
    if (!A.done) return "done_dev is NULL";
    if (!A.value) return "value_dev is NULL";
    if (!A.adv && !A.ret && !A.valid && !A.col) return "adv_dev, ret_dev, valid_dev and col_dev are all NULL";
    if (steps < 1) return "steps < 1";
    if (((int64_t)steps + 1) * (int64_t)num_envs > (int64_t)INT32_MAX) return "(steps + 1) * num_envs > INT32_MAX";
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return "gamma outside [0, 1]";
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return "lambda outside [0, 1]";
    if (A.final_value && !A.trunc) return "final_value_dev without trunc_dev";
    const uint64_t n = (uint64_t)num_envs, kn = (uint64_t)steps * n;
    struct Range {
        const void* p;
        uint64_t bytes;
        const char* name;
    };
    const Range in[] = {{A.reward, kn * 4, "reward_dev"}, {A.done, kn, "done_dev"},   {A.value, (kn + n) * 4, "value_dev"},         {A.steps_of, n * 4, "steps_of_dev"},
                        {A.skip, kn, "skip_dev"},         {A.trunc, kn, "trunc_dev"}, {A.final_value, kn * 4, "final_value_dev"}};
    const Range out[] = {{A.adv, kn * 4, "adv_dev"}, {A.ret, kn * 4, "ret_dev"}, {A.valid, kn, "valid_dev"}, {A.col, 3 * n * 8, "col_dev"}};
    static thread_local char text[64];
    for (int o = 0; o < 4; ++o) {
        for (const Range& r : in)
            if (targets_share_a_byte(out[o].p, out[o].bytes, r.p, r.bytes)) {
                snprintf(text, sizeof(text), "%s and %s overlap", out[o].name, r.name);
                return text;
            }
        for (int q = 0; q < o; ++q)
            if (targets_share_a_byte(out[o].p, out[o].bytes, out[q].p, out[q].bytes)) {
                snprintf(text, sizeof(text), "%s and %s overlap", out[q].name, out[o].name);
                return text;
            }
    }
    return nullptr;
}

inline const char* sum_columns_refusal(const void* col_dev, int32_t rows, const void* out_dev) {
    if (!col_dev) return "col_dev is NULL";
    if (!out_dev) return "out_dev is NULL";
    if (rows < 1) return "rows < 1";
    return nullptr;
}

// ---- the arithmetic of the definition, written once for the kernel and the host ----
struct TargetRow {
    float a, ret;
};

// One row with a target.  next_v: value[t+1]; trunc_v: what a truncated end bootstraps from (final_value[t], or value[t+1]); a: the advantage of row
// t + 1.  The multiply by nv = 0 and the add of gl * 0 stay: they are what turns a -0.0 into the loop's +0.0.
MG_TARGETS_HD TargetRow target_row(float r, float v, float next_v, float trunc_v, bool done, bool trunc, float a, float gamma, float gl) {
    MG_TARGETS_NO_CONTRACT
    const float nv = done ? (trunc ? trunc_v : 0.0f) : next_v;
    const float carry = done ? 0.0f : a;
    const float delta = (r + gamma * nv) - v;
    TargetRow o;
    o.a = delta + gl * carry;
    o.ret = o.a + v;
    return o;
}

// count, sum and sum of squares of a column's valid advantages, in the walk's order; (double)a * (double)a is one rounded multiply, then the add
struct TargetMoments {
    double count, sum, sq;
};
MG_TARGETS_HD void target_moments_add(TargetMoments& m, float a) {
    MG_TARGETS_NO_CONTRACT
    const double d = (double)a;
    const double dd = d * d;
    m.count = m.count + 1.0;
    m.sum = m.sum + d;
    m.sq = m.sq + dd;
}

// n_i of mg_split_episodes (mg_sequences.hpp seq_steps_of, which is device code only)
MG_TARGETS_HD int targets_steps_of(const int32_t* steps_of, int i, int steps) {
    if (!steps_of) return steps;
    const int v = steps_of[i];
    return v < 0 ? 0 : (v > steps ? steps : v);
}

// Column i of the definition, t = steps - 1 down to 0, in blocks of T rows: a block's loads are all issued before its first row is computed, so that a
// column waits for memory once per block and not once per row.  value[t+1] is the row the walk loaded one step earlier.  EXTRA: skip / trunc /
// final_value may be there (each still NULL or not); without it none of the three is looked at.  COL: the moments are kept and written.
// The loads of a block stand in straight-line code -- no branch, so no copy of a loaded register at a join, which would wait for the load: a row
// below 0 of the last block loads row 0 again, and an optional array that is not there loads from `done` / `reward` in its place, the values unused.
template <int T, bool EXTRA, bool COL>
MG_TARGETS_HD void targets_walk_column(const TargetArrays& A, int steps, int num_envs, int i, float gamma, float gl) {
    const size_t n = (size_t)num_envs;
    const bool has_skip = EXTRA && A.skip, has_trunc = EXTRA && A.trunc, has_final = EXTRA && A.final_value;
    const float* __restrict__ reward = A.reward + i;
    const uint8_t* __restrict__ done = A.done + i;
    const float* __restrict__ value = A.value + i;
    const uint8_t* __restrict__ skip = has_skip ? A.skip + i : done;
    const uint8_t* __restrict__ trunc = has_trunc ? A.trunc + i : done;
    const float* __restrict__ final_value = has_final ? A.final_value + i : reward;
    float* __restrict__ adv = A.adv ? A.adv + i : nullptr;
    float* __restrict__ ret = A.ret ? A.ret + i : nullptr;
    uint8_t* __restrict__ valid = A.valid ? A.valid + i : nullptr;
    const int n_i = targets_steps_of(A.steps_of, i, steps);
    float a = 0.0f;
    float next_v = value[(size_t)steps * n];
    TargetMoments m = {0.0, 0.0, 0.0};
    for (int hi = steps; hi > 0; hi -= T) {  // rows hi - 1 .. max(hi - T, 0)
        float r[T], v[T], fv[T];
        uint32_t d[T], s[T], tr[T];
        MG_TARGETS_UNROLL
        for (int j = 0; j < T; ++j) {
            const int t = hi - 1 - j;
            const size_t at = (size_t)(t > 0 ? t : 0) * n;
            r[j] = reward[at];
            d[j] = done[at];
            v[j] = value[at];
            if (EXTRA) {
                s[j] = skip[at];
                tr[j] = trunc[at];
                fv[j] = final_value[at];
            }
        }
        MG_TARGETS_UNROLL
        for (int j = 0; j < T; ++j) {
            const int t = hi - 1 - j;
            if (t >= 0) {
                const size_t at = (size_t)t * n;
                const bool has_target = t < n_i && !(has_skip && s[j] != 0);
                const TargetRow o = target_row(r[j], v[j], next_v, has_final ? fv[j] : next_v, d[j] != 0, has_trunc && tr[j] != 0, a, gamma, gl);
                a = has_target ? o.a : 0.0f;
                if (adv) adv[at] = a;
                if (ret) ret[at] = has_target ? o.ret : 0.0f;
                if (valid) valid[at] = has_target ? 1 : 0;
                if (COL && has_target) target_moments_add(m, a);
                next_v = v[j];
            }
        }
    }
    if (COL) {
        A.col[i] = m.count;
        A.col[n + i] = m.sum;
        A.col[2 * n + i] = m.sq;
    }
}

// mg_sum_columns' order: SUM_LANES partial sums -- lane l starts at 0.0 and adds instances l, l + SUM_LANES, ... ascending -- then the halving tree
// part[l] += part[l + h] for h = SUM_LANES / 2, ..., 1.  The host form, for the stand-alone check; the kernel below is the same order on one workgroup.
constexpr int SUM_LANES = 256;
inline double sum_columns_row(const double* row, int num_envs) {
    double part[SUM_LANES];
    for (int l = 0; l < SUM_LANES; ++l) {
        part[l] = 0.0;
        for (int i = l; i < num_envs; i += SUM_LANES) part[l] = part[l] + row[i];
    }
    for (int h = SUM_LANES / 2; h >= 1; h >>= 1)
        for (int l = 0; l < h; ++l) part[l] = part[l] + part[l + h];
    return part[0];
}

}  // namespace mg

#ifdef __HIPCC__
namespace mg {

// A wave per workgroup: 16,384 instances are 256 workgroups, one per CU, and the lanes of a wave read 256 neighbouring bytes of a float row and 64 of a
// flag row, and store the same shapes.  No LDS, no atomic, no scratch.
constexpr int TARGETS_BLOCK = 64;

template <int T, bool EXTRA, bool COL>
__global__ __launch_bounds__(TARGETS_BLOCK) void rollout_targets_kernel(TargetArrays A, int steps, int num_envs, float gamma, float gl) {
    const int i = blockIdx.x * TARGETS_BLOCK + threadIdx.x;
    if (i < num_envs) targets_walk_column<T, EXTRA, COL>(A, steps, num_envs, i, gamma, gl);
}

// mg_sum_columns: workgroup r sums row r of col in the order of sum_columns_row
__global__ __launch_bounds__(SUM_LANES) void sum_columns_kernel(const double* __restrict__ col, int num_envs, double* __restrict__ out) {
    __shared__ double part[SUM_LANES];
    const int l = threadIdx.x;
    const double* row = col + (size_t)blockIdx.x * (size_t)num_envs;
    double s = 0.0;
    int i = l;
    for (; i + 7 * SUM_LANES < num_envs; i += 8 * SUM_LANES) {  // eight loads in flight, added in the order of the definition
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = row[i + k * SUM_LANES];
#pragma unroll
        for (int k = 0; k < 8; ++k) s = s + x[k];
    }
    for (; i < num_envs; i += SUM_LANES) s = s + row[i];
    part[l] = s;
    __syncthreads();
    for (int h = SUM_LANES / 2; h >= 1; h >>= 1) {
        if (l < h) part[l] = part[l] + part[l + h];
        __syncthreads();
    }
    if (l == 0) out[blockIdx.x] = part[0];
}

}  // namespace mg
#endif  // __HIPCC__
