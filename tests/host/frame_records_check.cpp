// tests/host/frame_records_check.cpp -- TEST INFRASTRUCTURE.  The host code of csrc/mg_frame_records.hpp without a GPU: the layout value (unique per handle,
// new with every rebuild and every composer change, never equal to an mg_instance_layout value), the bytes of an observation row per format, and what
// mg_save_frames / mg_draw_frames refuse -- each error of include/memgym.h, and the calls it must let through.  It also replays the save's row gather on the
// host over buffers of exactly the sizes the C ABI asks for, so a build with -fsanitize=address,undefined sees an index that leaves a row or a record.
// Prints "OK" and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "../../endless-memory-gym_amd/csrc/mg_frame_records.hpp"

static int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

static bool says(const char* got, const char* want) { return got && strstr(got, want); }

// frame_rows_save_kernel's walk (mg_api_records.hpp), lane by lane: -> entries flagged
static int save_walk(const std::vector<unsigned char>& descs, int vec_per_row, const std::vector<int32_t>* idx, int count, int num_envs, std::vector<unsigned char>& rec) {
    int flagged = 0;
    const int64_t lanes = (((int64_t)count * vec_per_row + 255) / 256) * 256;  // whole workgroups, as launched
    for (int64_t t = 0; t < lanes; ++t) {
        const int64_t j = t / vec_per_row;
        if (j >= count) continue;
        const int q = (int)(t - j * vec_per_row);
        const int i = idx ? idx->at((size_t)j) : (int)j;
        if (i < 0) continue;
        if (i >= num_envs) {
            flagged += q == 0;
            continue;
        }
        memcpy(rec.data() + ((size_t)j * vec_per_row + q) * 16, descs.data() + ((size_t)i * vec_per_row + q) * 16, 16);
    }
    return flagged;
}

int main() {
    // ---- the layout value
    std::set<uint64_t> seen;
    for (uint64_t serial = 1; serial <= 40; ++serial)
        for (uint64_t geometry = 1; geometry <= 6; ++geometry)
            for (uint64_t frames = 0; frames <= 1; ++frames) {
                const uint64_t v = mg::frame_layout_value(serial, geometry, frames);
                if (!(v >> 63)) return fail("bit 63 marks a frame layout");
                if (((v >> 24) & 0x7FFFFFFFFFull) != serial) return fail("the handle's number is part of the value");
                if (v == ((serial << 24) | (geometry & 0xFFFFFFull))) return fail("equal to the handle's mg_instance_layout value");
                if (v == mg::frame_layout_value(serial, geometry + 1, frames) || v == mg::frame_layout_value(serial, geometry, frames + 1))
                    return fail("a rebuild or a composer change left the value as it was");
                if (frames == 0 && !seen.insert(v).second) return fail("two handles share a value");
            }
    if (mg::frame_layout_value(1, 0xFFFFFF, 1) >> 24 != mg::frame_layout_value(1, 0, 0) >> 24) return fail("the count wrapped into the handle's number");
    if (mg::frame_layout_value(0x7FFFFFFFFFull, 1, 0) >> 63 != 1) return fail("a large handle number reached bit 63");

    // ---- bytes of a row
    if (mg::frame_row_bytes(MG_OBS_U8_XYC) != 21168 || mg::frame_row_bytes(MG_OBS_U8_CYX) != 21168 || mg::frame_row_bytes(MG_OBS_F16_CYX) != 42336 ||
        mg::frame_row_bytes(MG_OBS_BF16_CYX) != 42336 || mg::frame_row_bytes(MG_OBS_F32_CYX) != 84672)
        return fail("frame_row_bytes of a format");
    for (int f = -3; f < 12; ++f)
        if ((mg::frame_row_bytes(f) != 0) != (f >= 0 && f <= 4)) return fail("frame_row_bytes of an unknown format");
    for (int f = 0; f <= 4; ++f)
        if (mg::frame_row_bytes(f) % 16) return fail("a row is whole 16-byte vectors in every format");

    // ---- refusals
    alignas(16) static unsigned char rec[256], obs[256];
    if (mg::frame_save_refusal(0, rec) || mg::frame_save_refusal(INT32_MAX, rec)) return fail("a legal save was refused");
    if (!says(mg::frame_save_refusal(-1, rec), "count < 0") || !says(mg::frame_save_refusal(4, nullptr), "rec_dev") || !says(mg::frame_save_refusal(4, rec + 8), "rec_dev"))
        return fail("a save that must be refused");
    const int64_t big = (int64_t)INT32_MAX;
    if (mg::frame_draw_refusal(rec, 8, false, 8, MG_OBS_U8_XYC, obs) || mg::frame_draw_refusal(rec, 8, false, 1, MG_OBS_F32_CYX, obs) ||
        mg::frame_draw_refusal(rec, 1, true, 5000000, MG_OBS_BF16_CYX, obs) || mg::frame_draw_refusal(rec, big, true, big, MG_OBS_U8_CYX, obs) ||
        mg::frame_draw_refusal(rec, 0, false, 0, MG_OBS_U8_XYC, obs) || mg::frame_draw_refusal(rec, 8, true, 0, MG_OBS_F16_CYX, obs))
        return fail("a legal draw was refused");
    struct {
        const void *rec, *obs;
        int64_t n_records, count;
        bool pick;
        int format;
        const char* words;
    } bad[] = {{rec, obs, 8, -1, false, 0, "count < 0"},        {nullptr, obs, 8, 8, false, 0, "rec_dev"},       {rec + 4, obs, 8, 8, false, 0, "rec_dev"},
               {rec, nullptr, 8, 8, false, 0, "obs_dev"},       {rec, obs + 8, 8, 8, false, 0, "obs_dev"},       {rec, obs, 0, 1, true, 0, "n_records < 1"},
               {rec, obs, -5, 1, true, 0, "n_records < 1"},     {rec, obs, 8, 8, false, 5, "unknown format"},    {rec, obs, 8, 8, false, -1, "unknown format"},
               {rec, obs, 8, 9, false, 0, "count > n_records"}, {rec, obs, big + 1, 8, true, 0, "n_records > "}, {rec, obs, 8, big + 1, true, 0, "count > INT32_MAX"}};
    for (const auto& b : bad)
        if (!says(mg::frame_draw_refusal(b.rec, b.n_records, b.pick, b.count, b.format, b.obs), b.words)) {
            printf("want: %s\n", b.words);
            return fail("a draw that must be refused");
        }

    // ---- the save's walk: 16 / 64 / 128-byte descriptors, counts that fill no workgroup, every index rule
    for (int vec_per_row : {1, 4, 8}) {
        const int num_envs = 200;
        std::vector<unsigned char> descs((size_t)num_envs * vec_per_row * 16);
        for (size_t k = 0; k < descs.size(); ++k) descs[k] = (unsigned char)(k * 7 + k / 251);
        for (int count : {1, 3, 63, 200, 257}) {
            std::vector<int32_t> idx((size_t)count);
            for (int j = 0; j < count; ++j) idx[(size_t)j] = (j * 37 + 5) % num_envs;
            int want_flags = 0;
            if (count > 2) { idx[1] = -1; idx[2] = num_envs; want_flags = 1; }
            if (count > 60) { idx[60] = INT32_MAX; idx[61] = INT32_MIN; want_flags = 2; }
            std::vector<unsigned char> out((size_t)count * vec_per_row * 16, 0xA5);
            if (save_walk(descs, vec_per_row, &idx, count, num_envs, out) != want_flags) return fail("entries flagged");
            for (int j = 0; j < count; ++j) {
                const int i = idx[(size_t)j];
                const size_t b = (size_t)vec_per_row * 16;
                const bool skipped = i < 0 || i >= num_envs;
                for (size_t k = 0; k < b; ++k)
                    if (out[(size_t)j * b + k] != (skipped ? 0xA5 : descs[(size_t)i * b + k])) return fail("a record row after the walk");
            }
            if (count <= num_envs) {  // idx == NULL: instance j
                std::vector<unsigned char> all((size_t)count * vec_per_row * 16, 0);
                if (save_walk(descs, vec_per_row, nullptr, count, num_envs, all) != 0 || memcmp(all.data(), descs.data(), all.size()) != 0) return fail("idx == NULL");
            }
        }
    }
    printf("OK\n");
    return 0;
}
