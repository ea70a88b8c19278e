// tests/host/instances_table_check.cpp -- TEST INFRASTRUCTURE.  The host half of csrc/mg_instances.hpp without a GPU: the row table
// (offsets, widths, record size), the split of long rows over waves and the rule by which an entry of a call is served, skipped or
// flagged.  It walks every (row, split, lane) the kernels would and marks the bytes they touch in host buffers of exactly the sizes
// the C ABI asks for, so a build with -fsanitize=address,undefined sees any index that leaves a row or a record.
// Prints "OK" and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../endless-memory-gym_amd/csrc/mg_instances.hpp"

static int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

// the kernel's walk over one entry, on the host: every unit of every row exactly once
static int walk(const mg::InstanceRows& t, int splits, int i, int r, std::vector<std::vector<unsigned char>>& arrays, std::vector<unsigned char>& rec, bool save) {
    for (int split = 0; split < splits; ++split)
        for (int k = 0; k < t.rows; ++k) {
            const uint32_t w = t.width[k], units = t.bytes[k] / w;
            const uint32_t per = (((units + splits - 1u) / splits) + 63u) & ~63u;
            const uint32_t lo = split * per, hi = lo + per < units ? lo + per : units;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t u = lo + lane; u < hi; u += 64) {
                    unsigned char* a = arrays[k].data() + (size_t)i * t.bytes[k] + (size_t)u * w;
                    unsigned char* b = rec.data() + (size_t)r * t.rec_bytes + t.offset[k] + (size_t)u * w;
                    if (save) memcpy(b, a, w);
                    else memcpy(a, b, w);
                }
        }
    return 0;
}

int main() {
    // widths
    if (mg::instance_row_width(16) != 16 || mg::instance_row_width(53248) != 16 || mg::instance_row_width(312) != 8 || mg::instance_row_width(8) != 8 ||
        mg::instance_row_width(260) != 4 || mg::instance_row_width(180) != 4 || mg::instance_row_width(13) != 1 || mg::instance_row_width(1) != 1)
        return fail("instance_row_width");
    // entries
    const int n = 200, count = 65;
    if (mg::instance_entry(-1, 0, n, count) != 0 || mg::instance_entry(-2147483647 - 1, 99, n, count) != 0 || mg::instance_entry(0, 0, n, count) != 1 ||
        mg::instance_entry(n - 1, count - 1, n, count) != 1 || mg::instance_entry(n, 0, n, count) != -1 || mg::instance_entry(2147483647, 0, n, count) != -1 ||
        mg::instance_entry(3, count, n, count) != -1 || mg::instance_entry(3, -1, n, count) != -1 || mg::instance_entry(3, 2147483647, n, count) != -1)
        return fail("instance_entry");
    // tables: the shapes the families declare (bytes per instance), plus rows of awkward sizes
    const std::vector<std::vector<size_t>> shapes = {{96, 32, 16, 8, 8, 8, 8, 8}, {96, 512, 16, 8, 8, 8, 8, 8, 720}, {128, 312, 64, 640, 8, 8, 8, 8, 8},
                                                     {128, 53248, 64, 640, 8, 8, 8, 8, 8}, {13, 1, 260, 17000, 16388, 7}, {16}};
    for (const auto& shape : shapes) {
        std::vector<std::vector<unsigned char>> arrays(shape.size());
        std::vector<std::pair<void*, size_t>> rows;
        for (size_t k = 0; k < shape.size(); ++k) {
            arrays[k].resize(shape[k] * n);
            for (size_t b = 0; b < arrays[k].size(); ++b) arrays[k][b] = (unsigned char)(b * 131 + k * 17 + 1);
            rows.push_back({arrays[k].data(), shape[k]});
        }
        const mg::InstanceRows t = mg::make_instance_rows(rows);
        const int splits = mg::instance_splits(t);
        size_t sum = 0;
        for (int k = 0; k < t.rows; ++k) {
            if (t.offset[k] % 16 != 0 || t.offset[k] != sum || t.bytes[k] % t.width[k] != 0) return fail("offsets / widths of a table");
            sum += (t.bytes[k] + 15) / 16 * 16;
        }
        if (t.rec_bytes != sum || t.rec_bytes % 16 != 0) return fail("record size");
        std::vector<unsigned char> rec((size_t)t.rec_bytes * count, 0);
        const std::vector<std::vector<unsigned char>> before = arrays;
        for (int j = 0; j < count; ++j) walk(t, splits, (j * 3) % n, j, arrays, rec, true);  // record j <- instance 3 j
        if (arrays != before) return fail("a save wrote to an instance");
        for (int j = 0; j < count; ++j) walk(t, splits, n - 1 - j, j, arrays, rec, false);  // instance n-1-j <- record j
        for (int j = 0; j < count; ++j)
            for (int k = 0; k < t.rows; ++k)
                if (memcmp(arrays[k].data() + (size_t)(n - 1 - j) * shape[k], before[k].data() + (size_t)((j * 3) % n) * shape[k], shape[k]) != 0)
                    return fail("a loaded row differs from the saved one");
        for (int i = 0; i < n - count; ++i)
            for (int k = 0; k < t.rows; ++k)
                if (memcmp(arrays[k].data() + (size_t)i * shape[k], before[k].data() + (size_t)i * shape[k], shape[k]) != 0) return fail("an instance nobody named changed");
    }
    // refusals of the table
    try {
        std::vector<std::pair<void*, size_t>> rows(17, {(void*)&n, 8});
        mg::make_instance_rows(rows);
        return fail("17 rows were accepted");
    } catch (const std::exception&) {
    }
    try {
        mg::make_instance_rows({{(void*)&n, 0}});
        return fail("a row of 0 bytes was accepted");
    } catch (const std::exception&) {
    }
    printf("OK\n");
    return 0;
}
