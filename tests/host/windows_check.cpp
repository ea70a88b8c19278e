// tests/host/windows_check.cpp -- TEST INFRASTRUCTURE.  The host part of csrc/mg_windows.hpp without a GPU and without a GPU compiler: what
// mg_episode_positions, mg_window_picks and mg_gather_rows_padded refuse, the access width the gather chooses from (src, dst, row_bytes), and which of its
// two forms a row takes.  Built with -fsanitize=address,undefined and run as a program; prints "OK" and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <string.h>

#include "../../endless-memory-gym_amd/csrc/mg_windows.hpp"

static int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

static bool says(const char* got, const char* want) { return got && strstr(got, want); }

int main() {
    using namespace mg;
    alignas(16) static char a[4096], b[4096];
    const int32_t big = INT32_MAX;

    // mg_episode_positions
    if (positions_refusal(a, 1, b, 1) || positions_refusal(a, 1030, b, 257)) return fail("legal positions were refused");
    if (!says(positions_refusal(nullptr, 4, b, 7), "done_dev") || !says(positions_refusal(a, 4, nullptr, 7), "pos_dev") ||
        !says(positions_refusal(a, 0, b, 7), "steps < 1") || !says(positions_refusal(a, -3, b, 7), "steps < 1"))
        return fail("positions: a NULL buffer or steps < 1 was accepted");
    if (!says(positions_refusal(a, 3, b, 1 << 29), "INT32_MAX") || positions_refusal(a, 3, b, (1 << 29) - 1) || !says(positions_refusal(a, big, b, 2), "INT32_MAX"))
        return fail("positions: the int32 limit of (steps + 1) * num_envs");

    // mg_window_picks
    if (window_picks_refusal(a, 4, false, 35, 3, 0, 0, b, 7) || window_picks_refusal(a, 4, true, 1000, 3, 9, 4, b, 7) ||
        window_picks_refusal(a, 4, true, 0, 1, 0, 0, b, 7))
        return fail("legal picks were refused");
    if (!says(window_picks_refusal(nullptr, 4, true, 1, 3, 0, 0, b, 7), "pos_dev") || !says(window_picks_refusal(a, 4, true, 1, 3, 0, 0, nullptr, 7), "pick_dev"))
        return fail("picks: a NULL buffer was accepted");
    if (!says(window_picks_refusal(a, 0, true, 1, 3, 0, 0, b, 7), "steps < 1") || !says(window_picks_refusal(a, 4, true, -1, 3, 0, 0, b, 7), "m < 0") ||
        !says(window_picks_refusal(a, 4, true, 1, 0, 0, 0, b, 7), "window < 1") || !says(window_picks_refusal(a, 4, true, 1, 3, -1, 0, b, 7), "lag < 0") ||
        !says(window_picks_refusal(a, 4, true, 1, 3, 0, -1, b, 7), "back < 0"))
        return fail("picks: an integer out of range was accepted");
    if (!says(window_picks_refusal(a, 4, true, 1 << 16, 1 << 15, 0, 0, b, 7), "m * window") || window_picks_refusal(a, 4, true, 1 << 16, (1 << 15) - 1, 0, 0, b, 7))
        return fail("picks: the int32 limit of m * window");
    if (!says(window_picks_refusal(a, 2, true, 1, 3, 0, 1, b, 1 << 29), "(back + steps + 1)") || window_picks_refusal(a, 2, true, 1, 3, 0, 0, b, 1 << 29) ||
        !says(window_picks_refusal(a, 2, true, 1, 3, 0, big, b, 1), "(back + steps + 1)"))
        return fail("picks: the int32 limit of (back + steps + 1) * num_envs");
    if (!says(window_picks_refusal(a, 4, false, 36, 3, 0, 0, b, 7), "sel_dev is NULL") || window_picks_refusal(a, 4, true, 36, 3, 0, 0, b, 7))
        return fail("picks: m beyond the samples without a selection");

    // mg_gather_rows_padded
    if (gather_rows_refusal(a, 4, 768, true, 5, b) || gather_rows_refusal(a, 4, 1, false, 4, b) || gather_rows_refusal(a + 1, 4, 3, true, 9, b + 3) ||
        gather_rows_refusal(nullptr, 0, 8, true, 0, nullptr) || gather_rows_refusal(nullptr, 0, 8, true, 3, b))
        return fail("a legal gather was refused");
    if (!says(gather_rows_refusal(a, 4, 8, true, -1, b), "count < 0") || !says(gather_rows_refusal(a, -1, 8, true, 1, b), "n_rows < 0") ||
        !says(gather_rows_refusal(a, 4, 0, true, 1, b), "row_bytes < 1") || !says(gather_rows_refusal(a, 4, 8, false, 5, b), "count > n_rows") ||
        !says(gather_rows_refusal(a, (int64_t)1 << 31, 8, true, 1, b), "n_rows > INT32_MAX") || !says(gather_rows_refusal(a, 4, 8, true, (int64_t)1 << 31, b), "count > INT32_MAX") ||
        !says(gather_rows_refusal(a, 4, (int64_t)1 << 31, true, 1, b), "row_bytes > INT32_MAX"))
        return fail("gather: a count or size out of range was accepted");
    if (!says(gather_rows_refusal(a, 4, 8, true, 1, nullptr), "dst_dev") || !says(gather_rows_refusal(nullptr, 4, 8, true, 1, b), "src_dev"))
        return fail("gather: a NULL buffer was accepted");
    // overlap: [a, a + 4 * 64) against [dst, dst + 2 * 64)
    if (!says(gather_rows_refusal(a, 4, 64, true, 2, a), "overlap") || !says(gather_rows_refusal(a, 4, 64, true, 2, a + 255), "overlap") ||
        !says(gather_rows_refusal(a + 127, 4, 64, true, 2, a), "overlap") || gather_rows_refusal(a, 4, 64, true, 2, a + 256) ||
        gather_rows_refusal(a + 128, 4, 64, true, 2, a))
        return fail("gather: the overlap of the two ranges");

    // the access width: the widest of 16 / 8 / 4 / 2 / 1 that divides row_bytes and both bases
    struct {
        int so, dof;
        int64_t bytes;
        uint32_t want;
    } const cases[] = {{0, 0, 16, 16}, {0, 0, 768, 16},  {0, 0, 4100, 4}, {0, 0, 48, 16}, {0, 0, 6, 2},  {0, 0, 1, 1},  {0, 0, 8, 8},   {0, 0, 24, 8},
                       {8, 0, 768, 8}, {0, 4, 768, 4},   {2, 0, 768, 2},  {0, 2, 16, 2},  {1, 0, 768, 1}, {0, 1, 16, 1}, {16, 32, 4, 4}, {4, 12, 4096, 4},
                       {2, 2, 4100, 2}, {3, 0, 4100, 1}, {0, 0, 3, 1},    {0, 0, 12, 4},  {0, 0, 2, 2},  {32, 64, 2048, 16}};
    for (const auto& c : cases) {
        const uint32_t w = gather_width(a + c.so, b + c.dof, c.bytes);
        if (w != c.want) {
            printf("src + %d, dst + %d, %lld bytes: width %u, expected %u\n", c.so, c.dof, (long long)c.bytes, w, c.want);
            return fail("the access width");
        }
        if (c.bytes % w || ((uintptr_t)(a + c.so) % w) || ((uintptr_t)(b + c.dof) % w)) return fail("the width does not divide what it must");
    }
    if (gather_width(nullptr, nullptr, 1 << 20) != 16) return fail("the width is at most 16");
    // the form: fewer than GATHER_ROW_FORM_UNITS accesses per row -> PACKED
    if (!gather_packed(4, 4) || !gather_packed(1, 1) || !gather_packed(6, 2) || !gather_packed(48, 16) || !gather_packed(496, 16) || gather_packed(512, 16) ||
        gather_packed(768, 16) || gather_packed(4100, 4) || gather_packed(4100, 1) || gather_packed(32, 1) || !gather_packed(31, 1))
        return fail("the form of a row");
    printf("OK\n");
    return 0;
}
