// tests/host/debug_stretch_check.cpp -- TEST INFRASTRUCTURE.  The x4 image-order stream-out of mg_draw_debug_frames without a GPU: the chunk-to-source-byte
// mapping of csrc/mg_debug_stream_out.hpp (debug336_chunk, the function the kernel calls) expands a whole 84 x 84 x 3 frame here, lane by lane and round by
// round as store_debug336 walks it, from a source buffer of exactly 21,168 bytes into a view of exactly 338,688 -- so a build with
// -fsanitize=address,undefined sees any read or store that leaves either.  Also: every byte of the view is written exactly once, and what
// mg_draw_debug_frames refuses (csrc/mg_frame_records.hpp: debug_draw_refusal).
//   debug_stretch_check FRAME_IN VIEW_OUT     reads 21,168 bytes, writes 338,688; prints "OK" and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../endless-memory-gym_amd/csrc/mg_debug_stream_out.hpp"
#include "../../endless-memory-gym_amd/csrc/mg_frame_records.hpp"

static int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

static bool says(const char* got, const char* want) { return got && strstr(got, want); }

int main(int argc, char** argv) {
    using namespace mg;
    if (argc != 3) return fail("usage: debug_stretch_check FRAME_IN VIEW_OUT");
    const size_t frame_bytes = (size_t)DEBUG336_SRC * DEBUG336_SRC_COL_BYTES;
    if (frame_bytes != 21168 || DEBUG336_BYTES != 338688 || DEBUG336_ROW_CHUNKS != 63) return fail("the constants");
    std::vector<uint32_t> frame(frame_bytes / 4);  // (dwords: the LDS frame is read as aligned dwords)
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(frame.data(), 1, frame_bytes, f) != frame_bytes) return fail("cannot read the frame");
    fclose(f);

    std::vector<uint8_t> view(DEBUG336_BYTES, 0);
    std::vector<uint8_t> written(DEBUG336_BYTES, 0);
    for (int tid = 0; tid < 256; ++tid) {  // store_debug336's walk, row 0 of the output
        if (tid >= 4 * DEBUG336_ROW_CHUNKS) continue;
        const int y0 = tid / DEBUG336_ROW_CHUNKS, q = tid - y0 * DEBUG336_ROW_CHUNKS;
        const size_t base = (size_t)(4 * y0) * DEBUG336_ROW_BYTES + 16 * (size_t)q;
        for (int k = 0; k < DEBUG336_SRC / 4; ++k) {
            uint32_t w[4];
            debug336_chunk(frame.data(), 4 * k + y0, q, w);
            for (int rep = 0; rep < 4; ++rep) {
                const size_t at = base + (size_t)k * (16 * DEBUG336_ROW_BYTES) + (size_t)rep * DEBUG336_ROW_CHUNKS * 16;
                memcpy(&view.at(at), w, 16);  // (.at(): the first byte; the sanitizer watches the other fifteen)
                for (int b = 0; b < 16; ++b) ++written.at(at + b);
            }
        }
    }
    for (size_t b = 0; b < DEBUG336_BYTES; ++b)
        if (written[b] != 1) return fail("a byte of the view is written more than once, or never");
    // the mapping against its definition, byte by byte: out[Y][X][c] = frame[X >> 2][Y >> 2][c]
    const uint8_t* src = reinterpret_cast<const uint8_t*>(frame.data());
    for (int Y = 0; Y < DEBUG336; ++Y)
        for (int X = 0; X < DEBUG336; ++X)
            for (int c = 0; c < 3; ++c)
                if (view[((size_t)Y * DEBUG336 + X) * 3 + c] != src[(size_t)(X >> 2) * DEBUG336_SRC_COL_BYTES + (size_t)(Y >> 2) * 3 + c]) return fail("a byte of the view");
    f = fopen(argv[2], "wb");
    if (!f || fwrite(view.data(), 1, view.size(), f) != view.size()) return fail("cannot write the view");
    fclose(f);

    // mg_draw_debug_frames' refusals
    alignas(16) static char rec[64], rgb[64];
    if (debug_draw_refusal(rec, 4, false, 4, 336, rgb) || debug_draw_refusal(rec, 4, true, 1000, 84, rgb) || debug_draw_refusal(rec, 4, false, 0, 336, rgb))
        return fail("a legal draw was refused");
    if (!says(debug_draw_refusal(rec, 4, false, 4, 0, rgb), "size") || !says(debug_draw_refusal(rec, 4, false, 4, 168, rgb), "size") ||
        !says(debug_draw_refusal(rec, 4, false, 4, -336, rgb), "size"))
        return fail("a size other than 84 / 336 was accepted");
    if (!says(debug_draw_refusal(rec, 4, false, 4, 336, nullptr), "rgb_dev") || !says(debug_draw_refusal(rec, 4, false, 4, 336, rgb + 8), "rgb_dev") ||
        !says(debug_draw_refusal(nullptr, 4, false, 4, 336, rgb), "rec_dev") || !says(debug_draw_refusal(rec + 4, 4, false, 4, 84, rgb), "rec_dev"))
        return fail("a NULL or misaligned buffer was accepted");
    if (!says(debug_draw_refusal(rec, 4, false, -1, 336, rgb), "count < 0") || !says(debug_draw_refusal(rec, 4, false, 5, 336, rgb), "count > n_records") ||
        !says(debug_draw_refusal(rec, 0, true, 1, 336, rgb), "n_records < 1") || !says(debug_draw_refusal(rec, (int64_t)1 << 31, true, 1, 336, rgb), "INT32_MAX") ||
        !says(debug_draw_refusal(rec, 4, true, (int64_t)1 << 31, 336, rgb), "INT32_MAX"))
        return fail("a count or n_records out of range was accepted");
    printf("OK\n");
    return 0;
}
