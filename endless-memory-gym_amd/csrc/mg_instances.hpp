// mg_instances.hpp -- mg_save_instances / mg_load_instances (include/memgym.h): per-instance records to and from caller-owned device memory.
// One generic row copy over the table a family declares (Family::instance_rows): every array of a family that really is [num_envs][row] is a row
// of the table, and a record is the rows of ONE instance side by side, each starting at a multiple of 16 bytes.  The host part (the table) compiles
// without a GPU compiler; the kernels need hipcc.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

namespace mg {

constexpr int INSTANCE_MAX_ROWS = 16;
constexpr int ERR_INSTANCE_INDEX = 512;         // include/memgym.h: an index beyond the handle's instances / the call's records; the entry was skipped
constexpr uint32_t INSTANCE_SPLIT_BYTES = 16384;  // a row longer than this is shared by several waves (the grid's second dimension)
constexpr int INSTANCE_WAVES = 4;               // records per workgroup: one wave each

// The table as the kernels take it, by value: uniform for the launch, so every field a wave reads sits in SGPRs.
struct InstanceRows {
    int rows;
    uint32_t rec_bytes;               // bytes of one record, a multiple of 16
    char* base[INSTANCE_MAX_ROWS];    // the family's array: instance i's row starts at base + i * bytes
    uint32_t bytes[INSTANCE_MAX_ROWS];
    uint32_t offset[INSTANCE_MAX_ROWS];  // of the row inside a record, a multiple of 16
    uint32_t width[INSTANCE_MAX_ROWS];   // bytes per access: the widest of 16 / 8 / 4 / 1 that divides `bytes` (the arrays' bases and the records are 16-byte aligned,
                                         // so instance i's row is aligned to the largest power of two in `bytes`, and the record side to 16)
};

inline uint32_t instance_row_width(size_t bytes) { return bytes % 16 == 0 ? 16u : (bytes % 8 == 0 ? 8u : (bytes % 4 == 0 ? 4u : 1u)); }

// rows: (device pointer, bytes per instance) as Family::instance_rows() lists them
inline InstanceRows make_instance_rows(const std::vector<std::pair<void*, size_t>>& rows) {
    if (rows.empty() || rows.size() > (size_t)INSTANCE_MAX_ROWS) throw std::runtime_error("instance_rows: 1 .. 16 rows");
    InstanceRows t;
    t.rows = (int)rows.size();
    size_t at = 0;
    for (int r = 0; r < INSTANCE_MAX_ROWS; ++r) {
        const bool live = r < t.rows;
        const size_t b = live ? rows[r].second : 0;
        if (live && (b == 0 || b > 0x7FFFFFFFu || !rows[r].first)) throw std::runtime_error("instance_rows: a row of 0 bytes, of 2 GiB or more, or without an array");
        t.base[r] = live ? (char*)rows[r].first : nullptr;
        t.bytes[r] = (uint32_t)b;
        t.offset[r] = (uint32_t)at;
        t.width[r] = live ? instance_row_width(b) : 1u;
        at += (b + 15) & ~(size_t)15;
        if (at > 0x7FFFFFFFu) throw std::runtime_error("instance_rows: a record of 2 GiB or more");
    }
    t.rec_bytes = (uint32_t)at;
    return t;
}

// waves per record: the longest row in pieces of INSTANCE_SPLIT_BYTES
inline int instance_splits(const InstanceRows& t) {
    uint32_t longest = 0;
    for (int r = 0; r < t.rows; ++r) longest = t.bytes[r] > longest ? t.bytes[r] : longest;
    const uint32_t s = (longest + INSTANCE_SPLIT_BYTES - 1) / INSTANCE_SPLIT_BYTES;
    return s < 1 ? 1 : (s > 4096 ? 4096 : (int)s);
}

// What entry j of a call names, and whether it is served (the rule of include/memgym.h, restated once for the kernels and for the host-side check of it):
// 0 = skipped silently (a negative instance index: padding), 1 = served, -1 = skipped and flagged (ERR_INSTANCE_INDEX)
#ifdef __HIPCC__
__host__ __device__
#endif
inline int instance_entry(int i, int r, int num_envs, int count) {
    if (i < 0) return 0;
    if (i >= num_envs || r < 0 || r >= count) return -1;
    return 1;
}

#ifdef __HIPCC__
typedef uint32_t inst_vec16 __attribute__((ext_vector_type(4)));

// units lo .. hi-1 of one row, 64 lanes side by side, four accesses per lane in flight
template <typename T>
__device__ __forceinline__ void move_row(const char* __restrict__ src_row, char* __restrict__ dst_row, uint32_t lo, uint32_t hi, uint32_t lane) {
    const T* __restrict__ src = reinterpret_cast<const T*>(src_row);
    T* __restrict__ dst = reinterpret_cast<T*>(dst_row);
    uint32_t u = lo + lane;
    for (; u + 192u < hi; u += 256u) {
        const T a = src[u], b = src[u + 64u], c = src[u + 128u], d = src[u + 192u];
        dst[u] = a;
        dst[u + 64u] = b;
        dst[u + 128u] = c;
        dst[u + 192u] = d;
    }
    for (; u < hi; u += 64u) dst[u] = src[u];
}

// A wave owns entry j of the call (and, where the grid has a second dimension, the blockIdx.y-th piece of every row of it).  SAVE: record j <- instance
// idx[j].  LOAD: instance idx[j] <- record rec_of[j], if the claim launch in front of it (load_claim_kernel) left the instance to this entry.
// No LDS, no barrier, no communication; plain stores.
template <bool SAVE>
__global__ __launch_bounds__(64 * INSTANCE_WAVES) void instance_rows_kernel(InstanceRows t, const int32_t* __restrict__ idx, const int32_t* __restrict__ rec_of,
                                                                            const int32_t* __restrict__ claim, int count, int num_envs, char* rec, int* err) {
    const uint32_t lane = threadIdx.x & 63u;
    const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * INSTANCE_WAVES + (threadIdx.x >> 6)));
    if (j >= count) return;
    const int i = __builtin_amdgcn_readfirstlane(idx ? idx[j] : j);
    const int r = __builtin_amdgcn_readfirstlane((!SAVE && rec_of) ? rec_of[j] : j);
    const int what = instance_entry(i, r, num_envs, count);
    if (what != 1) {
        if (SAVE && what < 0 && lane == 0 && blockIdx.y == 0) raise_error(err, ERR_INSTANCE_INDEX);  // (a load's entries are flagged by its claim launch)
        return;
    }
    if (!SAVE && __builtin_amdgcn_readfirstlane(claim[i]) != j) return;  // another entry of this call names the same instance and holds it
    char* const record = rec + (size_t)r * t.rec_bytes;
    const uint32_t split = blockIdx.y, splits = gridDim.y;
    for (int k = 0; k < t.rows; ++k) {
        const uint32_t w = t.width[k], units = t.bytes[k] / w;
        const uint32_t per = (((units + splits - 1u) / splits) + 63u) & ~63u;  // whole rounds of the wave: pieces start on a 64-unit boundary
        const uint32_t lo = split * per, hi = lo + per < units ? lo + per : units;
        if (lo >= hi) continue;
        char* const inst_row = t.base[k] + (size_t)i * t.bytes[k];
        char* const rec_row = record + t.offset[k];
        const char* src = SAVE ? inst_row : rec_row;
        char* dst = SAVE ? rec_row : inst_row;
        if (w == 16u) move_row<inst_vec16>(src, dst, lo, hi, lane);
        else if (w == 8u) move_row<uint64_t>(src, dst, lo, hi, lane);
        else if (w == 4u) move_row<uint32_t>(src, dst, lo, hi, lane);
        else move_row<uint8_t>(src, dst, lo, hi, lane);
    }
}

// In front of a load: entry j claims its instance -- claim[i] = j, a plain store; where several entries name one instance, one of the stores stays and
// the load serves that entry alone, so the instance ends up holding ONE whole record -- and marks it in the row mask the frames are drawn by.  Entries
// beyond the handle's instances or the call's records are flagged here, once per entry.
__global__ __launch_bounds__(256) void load_claim_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ rec_of, int count, int num_envs,
                                                         int32_t* __restrict__ claim, uint8_t* __restrict__ mask, int* err) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int i = idx ? idx[j] : j;
    const int what = instance_entry(i, rec_of ? rec_of[j] : j, num_envs, count);
    if (what < 0) raise_error(err, ERR_INSTANCE_INDEX);
    if (what != 1) return;
    claim[i] = j;
    if (mask) mask[i] = 1;
}
#endif

}  // namespace mg
